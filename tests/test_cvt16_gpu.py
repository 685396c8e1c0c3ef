"""The 16-bit operand conversion kernels, bit for bit at every edge: spe_cvt_bf16 / spe_cvt_bf16_h / spe_cvt_bf16_multi (one tile body,
cvt_bf16_tile of csrc/gemm_bf16.hip), spe_cvt_f16 (csrc/misc.hip), the Python caches in front of them (spe_amd/kernels.py: cvt_bf16, act16,
weight16, _refresh_weights16, weightcat16, weightcat_f16, cvt_f16) and the kind-32 fragment record of spe_attn_pack / spe_attn_pack_multi.

Reference: tests/cvt16_ref.py (integer restatements of the roundings, checked against torch by tests/test_cvt16_ref_cpu.py); cases and
values: tests/cvt16_cases.py.  Every 16-bit output is compared as raw int16 patterns with torch.equal, NaN by position.  Every output
buffer sits inside a canary pattern - the other columns of a wide `out`, guard rows before and after, the floats around `colsum` - and the
whole buffer is compared, so a store outside the stated extent fails the same assertion.  Inputs are padded with NaN (row padding of x and
aux), which a read outside [R, C] would carry into an output.  Every launch is repeated and must give the same bits.

The only tolerances:
  colsum   |got - colsum64| <= R 2^-24 sum_r |x[r][c]| (any fp32 summation order of R terms, gamma_(R-1) <= R u for R <= 4096); onto a
           running value c0 the sum has R + 1 terms in an unknown order: (R + 1) 2^-24 (|c0| + sum |x|);
  GELU     bf16(ref64 - d) <= out <= bf16(ref64 + d) with d = delta |x|, delta = 4 x the worst |fp32 - fp64| / |x| of the kernel's own formula
           x (cdf + h pdf) evaluated with torch on the host of the run (the factor 4 is the margin for __expf and the spe_erff polynomial,
           as in profiles/f32_gemm_edges.txt); both roundings fp64 -> fp32 -> bf16 are monotone, so an fp32 value inside [ref64 - d, ref64 + d]
           lands inside the interval of the roundings.
Lines starting with CVT16 are recorded in profiles/cvt16_edges.txt."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvt16_cases as CS  # noqa: E402
import cvt16_ref as CR  # noqa: E402
import kv_layout as KV  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A                 # neither a NaN nor a zero in bf16 or fp16
FCANARY = 12345.5               # around colsum
GUARD = 2                       # guard rows before and after every 16-bit output
FGUARD = 8
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


_BITS = {}


def _bits_tensor(name):
    if name not in _BITS:
        _BITS[name] = CR.bits_to_f32(torch.tensor(getattr(CS, name), dtype=torch.int64))
    return _BITS[name]


def _data(R, C, seed, bits="MAIN_BITS"):
    """randn * 3 [R, C] with the value list scattered into three quarters of it: the whole list where it fits, else a window that moves
    with the seed."""
    vals = _bits_tensor(bits)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R * C, generator=g) * 3.0
    n = min(len(vals), max(1, (3 * R * C) // 4))
    pos = torch.randperm(R * C, generator=g)[:n]
    idx = (torch.arange(n) + seed * 37) % len(vals)
    x[pos] = vals[idx]
    return x.view(R, C)


def _xbuf(dev, x, ldx, xoff=0):
    """x [R, C] inside NaN padding with row stride ldx, `xoff` floats past the (16-byte aligned) allocation -> (device storage, host copy
    of it, address of x[0][0])."""
    R, C = x.shape
    st = torch.full((xoff + R * ldx + 4,), float("nan"))
    st[xoff:xoff + R * ldx].view(R, ldx)[:, :C] = x
    d = st.to(dev)
    assert d.data_ptr() % 16 == 0
    return d, st, d.data_ptr() + 4 * xoff


class Block16:
    """An int16 device matrix [GUARD + rows + GUARD, ld] full of canaries; the kernel's output is the block of `width` columns at column
    `off` of its middle rows."""

    def __init__(self, dev, rows, width, ld, off=0):
        assert off + width <= ld
        self.rows, self.width, self.ld, self.off = rows, width, ld, off
        self.full = torch.full((rows + 2 * GUARD, ld), CANARY, dtype=torch.int16, device=dev)

    @property
    def ptr(self):
        return self.full.data_ptr() + 2 * (GUARD * self.ld + self.off)

    def view(self):
        return self.full[GUARD:GUARD + self.rows, self.off:self.off + self.width]

    def expect(self, ref):
        e = torch.full(self.full.shape, CANARY, dtype=torch.int16)
        e[GUARD:GUARD + self.rows, self.off:self.off + self.width] = ref
        return e

    def untouched(self):
        return bool((self.full == CANARY).all())

    def get(self):
        return self.full.cpu()


class FBlock:
    """colsum [C] between float canaries."""

    def __init__(self, dev, C, init=None):
        h = torch.full((C + 2 * FGUARD,), FCANARY)
        h[FGUARD:FGUARD + C] = 0.0 if init is None else init
        self.C, self.host, self.full = C, h, h.to(dev)

    @property
    def ptr(self):
        return self.full.data_ptr() + 4 * FGUARD

    def view(self):
        return self.full[FGUARD:FGUARD + self.C]

    def reset(self):
        self.full.copy_(self.host)

    def get(self):
        f = self.full.cpu()
        assert torch.equal(f[:FGUARD], self.host[:FGUARD]) and torch.equal(f[FGUARD + self.C:], self.host[FGUARD + self.C:]), "colsum canaries"
        return f[FGUARD:FGUARD + self.C]


def _assert_bits(got, want, fmt, what):
    """Equality of bit patterns; NaN by position (its payload is the producer's business)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ng, nw = CR.is_nan16(got, fmt), CR.is_nan16(want, fmt)
    assert torch.equal(ng, nw), "%s: NaN positions differ at %d elements" % (what, int((ng != nw).sum()))
    bad = got.masked_fill(ng, 0) != want.masked_fill(nw, 0)
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d patterns differ, first at %s: got 0x%04x want 0x%04x"
                             % (what, int(bad.sum()), bad.numel(), i, int(got[i]) & 0xFFFF, int(want[i]) & 0xFFFF))


def _launch(K, c, xptr, bufs, colsum=None, auxptr=None, act=0):
    o = lambda k: bufs[k].ptr if k in bufs else None
    if c["entry"] == "h":
        K._call("spe_cvt_bf16_h", xptr, c["ldx"], c["R"], c["C"], o("out"), o("lo"), c["ldo"], o("T"), c["ldt"], K._st())
    else:
        K._call("spe_cvt_bf16", xptr, c["ldx"], c["R"], c["C"], o("out"), o("lo"), c["ldo"], o("T"), c["ldt"],
                None if colsum is None else colsum.ptr, auxptr, int(act), K._st())


def _make_bufs(dev, c):
    bufs = {}
    for k in ("out", "lo"):
        if k in c["outputs"]:
            bufs[k] = Block16(dev, c["R"], c["C"], c["ldo"], c["off"])
    if "T" in c["outputs"]:
        bufs["T"] = Block16(dev, c["C"], c["ldt"], c["ldt"])
    return bufs


def _check_16(c, bufs, v, tag):
    """The 16-bit outputs of a launch on the fp32 values v [R, C] (x, or x after the activation backward) -> the buffers as read."""
    hi = CR.bf16_rne_bits(v)
    got = {k: b.get() for k, b in bufs.items()}
    if "out" in bufs:
        _assert_bits(got["out"], bufs["out"].expect(hi), "bf16", tag + " out")
    if "lo" in bufs:
        if c["entry"] == "h":
            _assert_bits(got["lo"], bufs["lo"].expect(CR.f16_sat_bits(v)), "f16", tag + " out_h")
        else:
            _assert_bits(got["lo"], bufs["lo"].expect(CR.lo_bits(v)), "bf16", tag + " out_lo")
    if "T" in bufs:
        _assert_bits(got["T"], bufs["T"].expect(CR.transposeT(hi, c["ldt"])), "bf16", tag + " outT")
    return got


def _colsum_check(got, x64sum, sabs, R, c0=None, extra=None):
    """-> worst |got - ref| / bound of a column sum."""
    if c0 is None:
        ref, bound = x64sum, R * U * sabs
    else:
        ref, bound = c0.double() + x64sum, (R + 1) * U * (c0.double().abs() + sabs)
    if extra is not None:
        bound = bound + extra
    err = (got.double() - ref).abs()
    assert torch.isfinite(got).all() and (err <= bound).all(), (float(err.max()), float((err / bound.clamp_min(1e-300)).max()))
    return float((err / bound.clamp_min(1e-300)).max())


# ---- spe_cvt_bf16 / spe_cvt_bf16_h over the geometry list ----------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(CS.GEOMETRY)), ids=[c["name"] for c in CS.GEOMETRY])
def test_cvt_geometry(dev, ci):
    from spe_amd import kernels as K
    c = CS.GEOMETRY[ci]
    R, C = c["R"], c["C"]
    with_sum = "colsum" in c["outputs"]
    x = _data(R, C, ci + 1, "FINITE_BITS" if with_sum else "MAIN_BITS")
    xd, xh, xptr = _xbuf(dev, x, c["ldx"], c["xoff"])
    assert xptr % 16 == 4 * c["xoff"]
    bufs = _make_bufs(dev, c)
    cs = FBlock(dev, C) if with_sum else None
    _launch(K, c, xptr, bufs, cs)
    got = _check_16(c, bufs, x, c["name"])
    ratio = None
    if with_sum:
        s1 = cs.get()
        ratio = _colsum_check(s1, CR.colsum64(x), x.double().abs().sum(0), R)
        cs.reset()
    _launch(K, c, xptr, bufs, cs)
    for k, b in bufs.items():
        assert torch.equal(b.get(), got[k]), c["name"] + " second call: " + k
    if with_sum:
        assert torch.equal(cs.get().view(torch.int32), s1.view(torch.int32)), c["name"] + " second call: colsum"
    assert torch.equal(xd.cpu().view(torch.int32), xh.view(torch.int32))
    print("CVT16 geometry %-40s %s R=%d C=%d ldx=%d xoff=%d off=%d ldo=%d ldt=%d -> bits equal, canaries intact%s"
          % (c["name"], "spe_cvt_bf16_h" if c["entry"] == "h" else "spe_cvt_bf16", R, C, c["ldx"], c["xoff"], c["off"], c["ldo"], c["ldt"],
             "" if ratio is None else ", colsum err / bound %.3f" % ratio))


def test_cvt_wrapper_and_pinned_outcomes(dev):
    """Through K.cvt_bf16 (fresh tensors, ldt rounded up to 64): the outcomes the reference defines for the special values."""
    from spe_amd import kernels as K
    names = ("zero", "tie_even", "tie_odd", "tie_ulp", "bf16_max", "to_inf", "inf", "nan", "f16_sat", "f16_sub")
    bits = [b for k in names for b in CS.NAMED[k]]
    x = CR.bits_to_f32(torch.tensor(bits * 4, dtype=torch.int64))[:5 * 29].view(5, 29)
    xd = x.to(dev)
    lo = torch.empty((5, 29), device=dev, dtype=torch.bfloat16)
    out, outT = K.cvt_bf16(xd, True, True, out_lo=lo)
    h16 = torch.empty((5, 29), device=dev, dtype=torch.float16)
    out2, outT2 = K.cvt_bf16(xd, True, True, out_lo=h16, lo_f16=True)
    hi = CR.bf16_rne_bits(x)
    assert outT.shape == (29, 64)
    for o, t in ((out, outT), (out2, outT2)):
        _assert_bits(o.view(torch.int16).cpu(), hi, "bf16", "wrapper out")
        _assert_bits(t.view(torch.int16).cpu(), CR.transposeT(hi, 64), "bf16", "wrapper outT")
    glo, gh = lo.view(torch.int16).cpu(), h16.view(torch.int16).cpu()
    _assert_bits(glo, CR.lo_bits(x), "bf16", "wrapper out_lo")
    _assert_bits(gh, CR.f16_sat_bits(x), "f16", "wrapper out_h")
    flat, flo, fh = x.view(-1), glo.view(-1).to(torch.int64) & 0xFFFF, gh.view(-1).to(torch.int64) & 0xFFFF
    xb = x.view(torch.int32).view(-1).to(torch.int64) & 0xFFFFFFFF
    inf = torch.isinf(flat)
    assert inf.sum() >= 2 and (flo[inf] & 0x7FFF > 0x7F80).all()                              # infinite x: NaN low part
    for b, want in ((0x7F7F8000, 0xFF80), (0xFF7F8000, 0x7F80), (0x7F7FFFFF, 0xFF80), (0xFF7FFFFF, 0x7F80)):
        assert (flo[xb == b] == want).all() and (xb == b).any()                               # rounds to bf16 infinity: opposite infinite low part
    assert (fh[flat == 1e9] == 0x7BFF).all() and (fh[flat == -1e9] == 0xFBFF).all() and (fh[flat == 65520.0] == 0x7BFF).all()
    nan = torch.isnan(flat)
    assert nan.any() and (fh[nan] & 0x7FFF > 0x7C00).all()                                    # a NaN stays a NaN
    small = (flat.abs() < 2.0 ** -14) & (flat != 0)
    want = flat.clamp(-65504.0, 65504.0).half().view(torch.int16).to(torch.int64) & 0xFFFF
    assert small.sum() >= 8 and torch.equal(fh[small], want[small])                           # fp16 subnormals: torch's exactly


def test_cvt_fp32_subnormal_inputs(dev):
    """fp32 subnormal inputs: the bf16 copy is the reference pattern or a zero of the same sign (the device's denormal mode decides); the
    low part is the same statement about x - bf16(x) with the device's own high part; the fp16 copy is a signed zero either way."""
    from spe_amd import kernels as K
    x = _bits_tensor("SUBNORMAL_BITS")
    n = len(x)
    x = x.view(1, n)
    c = dict(entry="cvt", R=1, C=n, ldx=n, xoff=0, off=0, ldo=n, ldt=1, outputs=("out", "lo", "T"))
    xd, xh, xptr = _xbuf(dev, x, n)
    report = []
    for entry in ("cvt", "h"):
        c["entry"] = entry
        bufs = _make_bufs(dev, c)
        _launch(K, c, xptr, bufs)
        got = {k: b.get() for k, b in bufs.items()}
        hi = got["out"][GUARD:GUARD + 1]
        ref = CR.bf16_rne_bits(x)
        zero = ref & torch.tensor(-0x8000, dtype=torch.int16)
        kept, flushed = hi == ref, hi == zero
        assert (kept | flushed).all(), "bf16 of an fp32 subnormal is neither the reference nor a signed zero"
        assert torch.equal(got["out"], bufs["out"].expect(hi)) and torch.equal(got["T"], bufs["T"].expect(CR.transposeT(hi, 1)))
        if entry == "h":
            assert torch.equal(got["lo"], bufs["lo"].expect(CR.f16_sat_bits(x)))
        else:
            d = x - CR.bf16_bits_to_f32(hi)
            lref = CR.bf16_rne_bits(d)
            lzero = lref & torch.tensor(-0x8000, dtype=torch.int16)
            lo = got["lo"][GUARD:GUARD + 1]
            assert ((lo == lref) | (lo == lzero)).all() and torch.equal(got["lo"], bufs["lo"].expect(lo))
            report.append("low part: %d reference, %d zero" % (int((lo == lref).sum()), int(((lo == lzero) & (lo != lref)).sum())))
        nz = ref != zero                        # inputs whose reference result is not a zero anyway
        report.append("%s: %d of %d kept as bf16 subnormals, %d flushed to a signed zero"
                      % (entry, int((kept & nz).sum()), int(nz.sum()), int((flushed & nz & ~kept).sum())))
        _launch(K, c, xptr, bufs)
        assert all(torch.equal(b.get(), got[k]) for k, b in bufs.items())
    print("CVT16 fp32-subnormal inputs (%d patterns): %s" % (n, "; ".join(report)))


# ---- colsum ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C,ldt", CS.COLSUM, ids=["%dx%d%s" % (R, C, "" if t is None else "-ldt%d" % t) for R, C, t in CS.COLSUM])
def test_colsum_bound(dev, R, C, ldt):
    from spe_amd import kernels as K
    x = _data(R, C, R * 7 + C, "FINITE_BITS")
    xd = x.to(dev)
    s64, sabs = CR.colsum64(x), x.double().abs().sum(0)
    g = torch.Generator().manual_seed(R + C)
    c0 = torch.randn(C, generator=g) * 5.0
    c = dict(entry="cvt", R=R, C=C, ldx=C, xoff=0, off=0, ldo=C, ldt=ldt or R, outputs=("T",) if ldt else ())
    worst = []
    for init in (None, c0):
        cs = FBlock(dev, C, init)
        bufs = _make_bufs(dev, c)
        runs = []
        for _ in range(2):
            cs.reset()
            if ldt:
                _launch(K, c, xd.data_ptr(), bufs, cs)
                _check_16(c, bufs, x, "colsum %dx%d ldt %d" % (R, C, ldt))
            else:
                K.cvt_bf16(xd, want=False, colsum_out=cs.view())
            runs.append(cs.get())
        worst.append(_colsum_check(runs[0], s64, sabs, R, init))
        assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "two launches, two column sums"
    print("CVT16 colsum %dx%d%s err / bound: zeroed %.3f, running %.3f" % (R, C, "" if ldt is None else " ldt %d" % ldt, worst[0], worst[1]))


# ---- the activation backward folded into the read -----------------------------------------------------------------------------------------
def _aux_values(R, C, act, seed):
    g = torch.Generator().manual_seed(seed)
    if act == 1:
        a = torch.randn(R * C, generator=g)
        sp = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 3.0, -3.0])
    else:
        # |aux| up to 6, dense around the zero crossing of gelu' near -0.7518 and around 0
        a = torch.cat([torch.linspace(-6.0, 6.0, 193), -0.7518 + torch.linspace(-0.01, 0.01, 41), torch.linspace(-1e-3, 1e-3, 21),
                       torch.randn(R * C, generator=g) * 2.0])[:R * C].clamp(-6.0, 6.0)
        a = a[torch.randperm(a.numel(), generator=g)]
        sp = torch.tensor([0.0, -0.0, 6.0, -6.0, -0.7518])
    pos = torch.randperm(R * C, generator=g)[:3 * len(sp)]
    a[pos] = sp.repeat(3)
    return a.view(R, C)


@pytest.mark.parametrize("act,R,C,ldx", CS.ACT, ids=["%s-%dx%d-ldx%d" % ("relu" if a == 1 else "gelu", R, C, l) for a, R, C, l in CS.ACT])
def test_act_backward_in_the_read(dev, act, R, C, ldx):
    from spe_amd import kernels as K
    aux = _aux_values(R, C, act, R + C + act)
    ad, ah, aptr = _xbuf(dev, aux, ldx)
    c = dict(entry="cvt", R=R, C=C, ldx=ldx, xoff=0, off=0, ldo=C, ldt=R + 3, outputs=("out", "lo", "T"))
    if act == 1:
        # an equality: bf16(x) where aux > 0, else +0 - whatever x is (the special values included)
        x = _data(R, C, 5 * R + C, "MAIN_BITS")
        xd, xh, xptr = _xbuf(dev, x, ldx)
        v = torch.where(aux > 0, x, torch.zeros(()))
        assert (aux == 0).sum() >= 6 and (v.view(torch.int32)[aux == 0] == 0).all()
        bufs = _make_bufs(dev, c)
        _launch(K, c, xptr, bufs, None, aptr, 1)
        got = _check_16(c, bufs, v, "relu")
        _launch(K, c, xptr, bufs, None, aptr, 1)
        assert all(torch.equal(b.get(), got[k]) for k, b in bufs.items())
        # with the column sum, on finite data: the selection is exact, the plain bound holds for the selected values
        x = _data(R, C, 5 * R + C + 1, "FINITE_BITS")
        xd, xh, xptr = _xbuf(dev, x, ldx)
        v = torch.where(aux > 0, x, torch.zeros(()))
        cs, bufs = FBlock(dev, C), _make_bufs(dev, c)
        _launch(K, c, xptr, bufs, cs, aptr, 1)
        _check_16(c, bufs, v, "relu + colsum")
        s1 = cs.get()
        ratio = _colsum_check(s1, CR.colsum64(v), v.double().abs().sum(0), R)
        cs.reset()
        _launch(K, c, xptr, bufs, cs, aptr, 1)
        assert torch.equal(cs.get().view(torch.int32), s1.view(torch.int32))
        print("CVT16 act relu %dx%d ldx %d: bits equal (aux = +0 and -0 give +0), colsum err / bound %.3f" % (R, C, ldx, ratio))
    else:
        g = torch.Generator().manual_seed(R * C)
        x = torch.randn(R, C, generator=g) * 3.0
        x.view(-1)[torch.randperm(R * C, generator=g)[:4]] = torch.tensor([0.0, -0.0, 1024.0, -2.0 ** -20])
        xd, xh, xptr = _xbuf(dev, x, ldx)
        ref = CR.act_bwd64(x, aux, 2)
        nz = x != 0
        meas = ((CR.gelu_bwd_f32_formula(x, aux).double() - ref).abs()[nz] / x.double().abs()[nz]).max().item()
        delta = 4.0 * meas
        d = delta * x.double().abs()
        lo_v = CR.bf16_bits_to_f32(CR.bf16_rne_bits((ref - d).float())).double()
        hi_v = CR.bf16_bits_to_f32(CR.bf16_rne_bits((ref + d).float())).double()
        c["outputs"] = ("out", "T")
        cs, bufs = FBlock(dev, C), _make_bufs(dev, c)
        _launch(K, c, xptr, bufs, cs, aptr, 2)
        got = {k: b.get() for k, b in bufs.items()}
        o = got["out"][GUARD:GUARD + R]
        ov = CR.bf16_bits_to_f32(o).double()
        assert not CR.is_nan16(o, "bf16").any() and ((lo_v <= ov) & (ov <= hi_v)).all(), \
            "gelu: %d elements outside the interval" % int(((ov < lo_v) | (ov > hi_v)).sum())
        assert torch.equal(got["out"], bufs["out"].expect(o))                                # canaries
        assert torch.equal(got["T"], bufs["T"].expect(CR.transposeT(o, c["ldt"])))           # the transpose holds the same patterns
        exact = int((ov == CR.bf16_bits_to_f32(CR.bf16_rne_bits(ref.float())).double()).sum())
        s1 = cs.get()
        ratio = _colsum_check(s1, ref.sum(0), ref.abs().sum(0), R, extra=R * delta * x.double().abs().sum(0))
        cs.reset()
        _launch(K, c, xptr, bufs, cs, aptr, 2)
        assert all(torch.equal(b.get(), got[k]) for k, b in bufs.items()) and torch.equal(cs.get().view(torch.int32), s1.view(torch.int32))
        print("CVT16 act gelu %dx%d ldx %d: fp32 formula on the CPU worst |fp32 - fp64| / |x| = %.3e, delta = %.3e; all %d outputs inside "
              "[bf16(ref - d), bf16(ref + d)], %d equal to bf16(ref64); colsum err / bound %.3f" % (R, C, ldx, meas, delta, R * C, exact, ratio))
    assert torch.equal(ad.cpu().view(torch.int32), ah.view(torch.int32)) and torch.equal(xd.cpu().view(torch.int32), xh.view(torch.int32))


# ---- spe_cvt_f16 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C,ldx,ldo", CS.F16, ids=["%dx%d-ldx%d-ldo%d" % f for f in CS.F16])
def test_cvt_f16(dev, R, C, ldx, ldo):
    from spe_amd import kernels as K
    x = _data(R, C, R + C + ldx, "VALUE_BITS")
    xd, xh, xptr = _xbuf(dev, x, ldx)
    b = Block16(dev, R, C, ldo)
    xv = xd.as_strided((R, C), (ldx, 1), 0)
    K.cvt_f16(xv, out=b.view())
    g1 = b.get()
    _assert_bits(g1, b.expect(CR.f16_sat_bits(x)), "f16", "spe_cvt_f16")
    K.cvt_f16(xv, out=b.view())
    assert torch.equal(b.get(), g1)
    print("CVT16 spe_cvt_f16 %dx%d ldx %d ldo %d -> bits equal, canaries intact" % (R, C, ldx, ldo))


@pytest.mark.parametrize("why,C,ldx,ldo,xoff", [("C%4", 6, 8, 8, 0), ("ldx%4", 8, 9, 8, 0), ("ldo%4", 8, 8, 10, 0), ("x-unaligned", 8, 8, 8, 1)])
def test_cvt_f16_refusals(dev, why, C, ldx, ldo, xoff):
    from spe_amd import kernels as K
    from spe_amd.lib import SpeLibraryError
    R = 5
    xd, xh, xptr = _xbuf(dev, torch.ones(R, C), ldx, xoff)
    b = Block16(dev, R, C, ldo)
    with pytest.raises(SpeLibraryError, match="status -2"):
        K._call("spe_cvt_f16", xptr, ldx, R, C, b.ptr, ldo, K._st())
    torch.cuda.synchronize()
    assert b.untouched()


# ---- spe_cvt_bf16_multi with a hand-built table ---------------------------------------------------------------------------------------------
JOB_DTYPE = np.dtype([("x", "<u8"), ("out", "<u8"), ("outT", "<u8"), ("ldt", "<i8"), ("R", "<i4"), ("C", "<i4"), ("tile0", "<i4"),
                      ("tiles_c", "<i4"), ("out_lo", "<u8"), ("flags", "<i8")])

ONE_TILE = [(1, 1), (64, 64)] + [(1 + (i * 13) % 64, 1 + (i * 29) % 64) for i in range(38)]
MULTI_TABLES = {
    "one-job": [dict(R=65, C=129, ldt=65, outs=("out", "lo", "T"), flags=0)],
    "40-one-tile-jobs": [dict(R=R, C=C, ldt=R, outs=("out", "lo", "T"), flags=i & 1) for i, (R, C) in enumerate(ONE_TILE)],
    "mixed-null": [
        dict(R=1, C=200, ldt=1, outs=("out", "lo", "T"), flags=0), dict(R=200, C=1, ldt=203, outs=("lo", "T"), flags=0),
        dict(R=65, C=129, ldt=65 + 68, outs=("out", "T"), flags=0), dict(R=8, C=8, ldt=8, outs=("out", "lo"), flags=1),
        dict(R=65, C=129, ldt=68, outs=("out", "lo", "T"), flags=1), dict(R=200, C=1, ldt=268, outs=("T",), flags=0),
        dict(R=1, C=200, ldt=69, outs=("lo",), flags=1), dict(R=8, C=8, ldt=8 + 68, outs=("out", "lo", "T"), flags=0),
        dict(R=1, C=200, ldt=4, outs=("out",), flags=0), dict(R=8, C=8, ldt=11, outs=("lo", "T"), flags=1),
    ],
}


@pytest.mark.parametrize("name", list(MULTI_TABLES))
def test_cvt_multi_hand_built_table(dev, name):
    """The job table as kernels._refresh_weights16 builds it (64-byte records through K.host_table), tile0 / tiles_c / total_tiles from the
    header's rule: tiles_c = ceil(C / 64), tile0 = running sum of tiles_c * ceil(max(R, ldt) / 64)."""
    from spe_amd import kernels as K
    jobs = MULTI_TABLES[name]
    assert JOB_DTYPE.itemsize == 64
    rec = np.zeros(len(jobs), dtype=JOB_DTYPE)
    keep, t0 = [], 0
    for i, j in enumerate(jobs):
        R, C, ldt = j["R"], j["C"], j["ldt"]
        x = _data(R, C, 100 + i, "MAIN_BITS")
        xd = x.to(dev)
        c = dict(entry="h" if j["flags"] & 1 else "cvt", R=R, C=C, ldx=C, xoff=0, off=0, ldo=C, ldt=ldt, outputs=j["outs"])
        bufs = _make_bufs(dev, c)
        assert xd.data_ptr() % 16 == 0
        tc = (C + 63) // 64
        p = lambda k: bufs[k].ptr if k in bufs else 0
        rec[i] = (xd.data_ptr(), p("out"), p("T"), ldt, R, C, t0, tc, p("lo"), j["flags"])
        t0 += tc * ((max(R, ldt) + 63) // 64)
        keep.append((c, x, xd, bufs))
    if name == "40-one-tile-jobs":
        assert t0 == 40 and [int(v) for v in rec["tile0"]] == list(range(40))
    table = K.host_table(rec.view(np.uint8), dev)
    K._call("spe_cvt_bf16_multi", table.data_ptr(), len(jobs), t0, K._st())
    got = [_check_16(c, bufs, x, "%s job %d (%dx%d)" % (name, i, c["R"], c["C"])) for i, (c, x, xd, bufs) in enumerate(keep)]
    K._call("spe_cvt_bf16_multi", table.data_ptr(), len(jobs), t0, K._st())
    for (c, x, xd, bufs), g1 in zip(keep, got):
        assert all(torch.equal(b.get(), g1[k]) for k, b in bufs.items())
        assert torch.equal(xd.cpu().view(torch.int32), x.view(torch.int32))
    print("CVT16 multi %-18s %d jobs, %d tiles -> bits equal, canaries intact" % (name, len(jobs), t0))


# ---- through the caches ---------------------------------------------------------------------------------------------------------------------
def _i16(t):
    return t.contiguous().view(torch.int16).cpu()


def _check_weight(W_host, W16, W16T, lo, f16, tag):
    hi = CR.bf16_rne_bits(W_host)
    _assert_bits(_i16(W16), hi, "bf16", tag + " W16")
    assert W16T.shape == (W_host.shape[1], W_host.shape[0])
    _assert_bits(_i16(W16T), CR.transposeT(hi, W_host.shape[0]), "bf16", tag + " W16T")
    if lo is not None:
        assert lo.dtype == (torch.float16 if f16 else torch.bfloat16)
        _assert_bits(_i16(lo), CR.f16_sat_bits(W_host) if f16 else CR.lo_bits(W_host), "f16" if f16 else "bf16", tag + " W16lo")


def test_cached_copies_and_batched_refresh(dev):
    """weight16 / act16 / weightcat16 / weightcat_f16: all three copies against the reference bits, and again - every weight, every copy -
    after a raw in-place update + weights_changed() (the one-launch refresh through spe_cvt_bf16_multi)."""
    from spe_amd import kernels as K
    prec = K.get_precision()
    try:
        K.set_precision("bf16s")
        shapes = [(65, 129), (72, 200), (8, 8), (1, 200), (200, 1), (64, 64)]
        hosts = [_data(R, C, 300 + i, "MAIN_BITS") for i, (R, C) in enumerate(shapes)]
        Ws = [h.to(dev) for h in hosts]
        f16 = [False, True, False, True, False, True]
        for W, h, f in zip(Ws, hosts, f16):
            c = K.weight16(W, lo=True, f16=f)
            assert c.kind == (K.KIND_F16 if f else K.KIND_LO)
            _check_weight(h, c.w16, c.w16T, c.second, f, "weight16 %s" % (tuple(h.shape),))
            assert K.weight16(W, lo=True, f16=f).second is c.second                 # cached
        # activations
        xh = _data(67, 40, 400, "MAIN_BITS")
        xd = xh.to(dev)

        def check_act(x16, x16lo, lf, tag):
            _assert_bits(_i16(x16), CR.bf16_rne_bits(xh), "bf16", tag + " x16")
            _assert_bits(_i16(x16lo), CR.f16_sat_bits(xh) if lf else CR.lo_bits(xh), "f16" if lf else "bf16", tag + " x16lo")
        for lf in (False, True):
            check_act(*K.act16(xd, want_lo=True, lo_f16=lf), lf, "act16")
        # ... remembered on the tensor the caller holds: the same tensors again, re-made after a write, and when the other kind of second
        # copy is asked for (low part -> fp16 -> low part)
        src = xd.clone()
        x16, x16lo = K.act16(src.view(67, 40), src, want_lo=True)
        again = K.act16(src.view(67, 40), src, want_lo=True)
        assert again[0] is x16 and again[1] is x16lo
        assert K.act16(src.view(67, 40), src)[0] is x16                                   # no second copy asked for: any kind serves
        src.add_(1)
        xh = src.cpu()                                                                    # what the copies are now made of
        y16, y16lo = K.act16(src.view(67, 40), src, want_lo=True)
        assert y16 is not x16 and y16lo is not x16lo
        check_act(y16, y16lo, False, "act16 after add_")
        for lf in (True, False):
            z16, z16lo = K.act16(src.view(67, 40), src, want_lo=True, lo_f16=lf)
            assert z16 is not y16 and z16lo is not y16lo and src._spe16.kind == (K.KIND_F16 if lf else K.KIND_LO)
            check_act(z16, z16lo, lf, "act16 other kind")
            y16, y16lo = z16, z16lo
        # a weight cached without a low part (precision bf16) gets one when a lookup asks for it
        K.set_precision("bf16")
        Wn = hosts[0].to(dev)
        c = K.weight16(Wn)
        assert c.second is None and c.kind is None and K.weight16(Wn) is c
        K.set_precision("bf16s")
        c2 = K.weight16(Wn, lo=True)
        assert c2 is not c and c2.kind == K.KIND_LO and K._W16[(Wn.data_ptr(), 65, 129)] is c2
        _check_weight(hosts[0], c2.w16, c2.w16T, c2.second, False, "weight16 bf16 -> lo")
        # stacks of weights that share an input
        cat_h = [_data(R, 40, 500 + R, "MAIN_BITS") for R in (24, 65, 8)]
        cat = [h.to(dev) for h in cat_h]
        bs = [torch.full((h.shape[0],), float(i), device=dev) for i, h in enumerate(cat_h)]

        def check_cat():
            allh = torch.cat(cat_h, 0)
            c = K.weightcat16(cat, bs, lo=True)
            _check_weight(allh, c.w16, c.w16T, c.second, False, "weightcat16")
            assert torch.equal(c.bias.cpu(), torch.cat([b.cpu() for b in bs]))
            ch = K.weightcat_f16(cat, bs)
            assert ch.kind == K.KIND_F16 and ch.w16 is None and ch.w16T is None
            _assert_bits(_i16(ch.second), CR.f16_sat_bits(allh), "f16", "weightcat_f16")
            assert torch.equal(ch.bias.cpu(), c.bias.cpu())
        check_cat()
        # raw update: new values under unchanged version counters, then the epoch bump of a raw-pointer optimizer
        vers = [W._version for W in Ws + cat]
        for i, (W, h) in enumerate(zip(Ws + cat, hosts + cat_h)):
            h.copy_(_data(h.shape[0], h.shape[1], 700 + i, "MAIN_BITS"))
            W.data.view(torch.int32).copy_(h.view(torch.int32).to(dev))             # .data: no version bump, as a raw-pointer kernel
        assert [W._version for W in Ws + cat] == vers
        K.weights_changed()
        first = K.weight16(Ws[2], lo=True)
        key = lambda W: (W.data_ptr(), W.shape[0], W.shape[1])
        for W, h, f in zip(Ws, hosts, f16):
            c = K._W16[key(W)]
            assert c.epoch == K._W16_EPOCH                                          # refreshed by the one launch, not on demand
            _check_weight(h, c.w16, c.w16T, c.second, f, "refreshed %s" % (tuple(h.shape),))
        assert first.w16 is K._W16[key(Ws[2])].w16
        check_cat()
    finally:
        K.set_precision(prec)
    print("CVT16 caches: weight16 (low part and fp16 second copy), act16, weightcat16, weightcat_f16 and the batched refresh -> bits equal")


# ---- refusals and empty calls ----------------------------------------------------------------------------------------------------------------
def test_cvt_refusal_and_empty_calls(dev):
    from spe_amd import kernels as K
    from spe_amd.lib import SpeLibraryError
    R, C = 9, 12
    xd, xh, xptr = _xbuf(dev, torch.ones(R, C), C)
    c = dict(entry="cvt", R=R, C=C, ldx=C, xoff=0, off=0, ldo=C, ldt=R - 1, outputs=("out", "lo", "T"))
    for entry in ("cvt", "h"):
        c["entry"] = entry
        bufs = _make_bufs(dev, dict(c, ldt=R))
        cs = FBlock(dev, C, torch.full((C,), 2.5)) if entry == "cvt" else None
        with pytest.raises(SpeLibraryError, match="status -2"):
            _launch(K, c, xptr, bufs, cs)                                  # outT with ldt < R
        for R0, C0 in ((0, C), (R, 0), (0, 0)):
            _launch(K, dict(c, R=R0, C=C0, ldt=R), xptr, bufs, cs)         # status 0, nothing written
        torch.cuda.synchronize()
        assert all(b.untouched() for b in bufs.values())
        if cs is not None:
            assert torch.equal(cs.get(), torch.full((C,), 2.5))
    b = Block16(dev, R, C, C)
    for R0, C0 in ((0, C), (R, 0)):
        K._call("spe_cvt_f16", xptr, C, R0, C0, b.ptr, C, K._st())
    K._call("spe_cvt_bf16_multi", None, 0, 0, K._st())
    torch.cuda.synchronize()
    assert b.untouched()


# ---- the kind-32 fragment record ---------------------------------------------------------------------------------------------------------------
PACK_DH = (8, 16, 17, 24, 32, 33, 40, 48, 49, 64)
PACK_N = (1, 17, 100)


@pytest.mark.parametrize("N", PACK_N)
@pytest.mark.parametrize("dh", PACK_DH)
def test_attn_pack_kind32_bit_exact(dev, dh, N):
    """K.attn_pack and K.attn_pack_multi kinds 32 / 32 + F16 against kv_layout.pack32t of the rounded scale * x (bf16 RNE / saturating
    fp16), bit for bit, zeros in the padding rows and dims included; x is a strided slice of a packed qkv tensor [B, N, 3, H, dh] as the
    attention node passes it.  spe_attn_pack16 (kind 16) against kv_layout.pack16 of the bf16 rounding."""
    from spe_amd import kernels as K
    B, H = 2, 4
    g = torch.Generator().manual_seed(N * 100 + dh)
    qkv = torch.randn(B, N, 3, H, dh, generator=g) * 3.0
    sp = torch.tensor([b for k in CS.NAMED if k != "f32_sub" for b in CS.NAMED[k]], dtype=torch.int64)
    flat = qkv.view(-1)
    n = min(len(sp), flat.numel() // 2)
    flat[torch.randperm(flat.numel(), generator=g)[:n]] = CR.bits_to_f32(sp)[:n]
    qd = qkv.to(dev)
    scale = float(np.float32(dh ** -0.5 * K.LOG2E))
    for which in (0, 1, 2):
        x, xh = qd[:, :, which], qkv[:, :, which]
        assert x.stride() == (N * 3 * H * dh, 3 * H * dh, dh, 1)
        y = xh * torch.tensor(scale, dtype=torch.float32)
        want = {("bf16", True): KV.pack32t(CR.bf16_rne_bits(y)), ("f16", True): KV.pack32t(CR.f16_sat_bits(y)),
                ("bf16", False): KV.pack32t(CR.bf16_rne_bits(xh)), ("f16", False): KV.pack32t(CR.f16_sat_bits(xh))}
        single = K.attn_pack(x, scale)
        assert single.shape == (B, H, (N + 15) // 16, K.frag_record_elems(dh)) and single.dtype == torch.bfloat16
        _assert_bits(_i16(single), want[("bf16", True)], "bf16", "spe_attn_pack")
        outs = K.attn_pack_multi([(x, scale, 32), (x, scale, 32 + K.F16), (x, 1.0, 32), (x, 1.0, 32 + K.F16), (x, 1.0, 16)])
        for o, (fmt, scaled) in zip(outs[:4], (("bf16", True), ("f16", True), ("bf16", False), ("f16", False))):
            assert o.dtype == (torch.float16 if fmt == "f16" else torch.bfloat16)
            _assert_bits(_i16(o), want[(fmt, scaled)], fmt, "attn_pack_multi kind 32 %s scale %s" % (fmt, scaled))
        w16 = KV.pack16(CR.bf16_rne_bits(xh))
        _assert_bits(_i16(outs[4]), w16, "bf16", "attn_pack_multi kind 16")
        _assert_bits(_i16(K.attn_pack16(x)), w16, "bf16", "spe_attn_pack16")
    print("CVT16 pack kind 32 N=%d dh=%d (q, k, v slices of [2, %d, 3, 4, %d]) -> bits equal" % (N, dh, N, dh))
