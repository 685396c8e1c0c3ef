"""The lower half of csrc/rowops.hip - spe_colsum, spe_layerscale_residual_fwd / _bwd / _bwd16 / _bwd16d, spe_act_bwd, spe_dropout - and
the reduction engine under it (csrc/det_reduce.h; the deferred sums of csrc/misc.hip) against the fp64 restatements and bounds of
tests/rowsum_ref.py, at every dispatch edge of the launchers.  The cases are those of tests/rowsum_cases.py: each names the kernel and the
member count of the cross-workgroup sum it hits, and tests/test_rowsum_plan_cpu.py holds the launchers to those claims without a GPU.

  colsum      the wide, tall4 and generic kernels at their column and row edges, 1 / 2 / 16 / 17 / 64 (capped) / 257 members, strided
              views with canaries behind column C, a view one float off alignment, accumulate onto a running sum and accumulate = 0
              onto canaries, `out` inside a longer canary buffer, R = 0 both ways;
  lsres_fwd   one lane to the grid-stride loop, the per-sample scale (one scale exactly 0: those rows are x, bit for bit);
  lsres_bwd   the rows kernel (C = 4 .. 1024; 1 .. 128 capped members) and the generic kernel (C > 1024, C % 4, misaligned dy; up to the
              256-member cap): dy bit for bit, dgamma under the summation bound, onto a running sum;
  bwd16(d)    both template variants, R = 1 .. 16385 (several tiles per workgroup), ldt beyond the rounded R (all-padding tiles written as
              zeros - +0.0 or -0.0, the sign of gamma - into a canary-filled dy16T), y as fp32 / fp16, either 16-bit output alone, dropout and DropPath scales (the keep-scales
              recovered from spe_dropout: flat index by flat index the four-at-a-time draw is the one-at-a-time draw), every refusal;
  act_bwd     ReLU bit for bit on signed zeros, denormals and infinities; GELU on a grid of h over [-12, 12], at +-40 and on random h,
              allowed 4 x the error of torch's own fp32 autograd of F.gelu on the same inputs + 2^-23 (in units of |dy|);
  dropout     n = 1 .. 8192 * 256 + 1, p in {0, 0.1, 0.5}: outputs exactly x * 0 or x * fp32(1 / (1 - p)), a mask that ignores x, repeats
              with (seed, offset) and changes with the offset;
  engine      every reduction runs twice, bitwise equal; the deferred sums directly: destinations untouched until the flush, the 24-entry
              table, the 40 segments, a small arena, a launch larger than the arena, two launches into one destination, a destination
              outside the registered ranges, one-member launches, a NULL db; at the end no ticket is left behind.

Measured figures: profiles/rowsum_edges.txt (every line this module prints with the prefix ROWSUM)."""
import contextlib
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rownorm_ref as rr  # noqa: E402
import rowsum_cases as C  # noqa: E402
import rowsum_ref as rs  # noqa: E402

pytestmark = pytest.mark.gpu

FILL16, FILL32 = 0x5A5A, 0x5A5A5A5A      # what every canary holds (fp32 1.5e16, bf16 1.5e16: never produced here)
PAD = 8                                   # canary floats in front of and behind an output


def _filled(n, dtype, dev):
    if dtype == torch.float32:
        return torch.full((n,), FILL32, dtype=torch.int32, device=dev).view(torch.float32)
    return torch.full((n,), FILL16, dtype=torch.int16, device=dev).view(dtype)


def _untouched(t):
    return bool((rs.bits(t) == (FILL32 if t.dtype == torch.float32 else FILL16)).all())


def _framed(n, dtype, dev, off=0):
    """(buffer, view of n elements that starts PAD + off elements in): canaries all round the view."""
    buf = _filled(n + 2 * PAD + off, dtype, dev)
    return buf, buf[PAD + off:PAD + off + n]


def _frame_ok(buf, n, off=0):
    return _untouched(buf[:PAD + off]) and _untouched(buf[PAD + off + n:])


def _p(t):
    return None if t is None else t.data_ptr()


def _rc(name, *args):
    """Status of an entry point (no exception)."""
    from spe_amd import kernels as K
    st = K._st()
    if K._RWS is None:
        K._register_reduce_ws()
    return getattr(K.lib.load(), name)(*args, st)


def _plan(c):
    from spe_amd import kernels as K
    ld = None
    if c["launcher"] == "colsum":
        ld = c["C"] + c.get("pad", 0)
    elif c["launcher"] == "lsres_bwd16":
        ld = C.ldt_of(c)
    plan = K.rowops_plan(c["launcher"], c["R"], c["C"], ld=ld, aligned=C.aligned_of(c))
    assert plan["status"] == 0 and (plan["kernel"], plan["members"]) == (c["kernel"], c["members"]), (c["id"], plan)
    return plan


def _say(*a):
    print("ROWSUM", *a)


def _fig(d):
    return " ".join(f"{k} {v:.3e}" for k, v in d.items())


# ------------------------------------------------------------------------------------------------------------------------------
# spe_colsum
# ------------------------------------------------------------------------------------------------------------------------------
def _colsum_input(c, dev):
    """x [R, C] as a view with row stride C + pad that starts `off` floats into its buffer; everything else in the buffer is canary."""
    R, Cc, pad, off = c["R"], c["C"], c.get("pad", 0), c.get("off", 0)
    g = torch.Generator().manual_seed(7 * R + Cc + pad)
    buf = _filled(R * (Cc + pad) + off + 4, torch.float32, dev)
    x = buf[off:off + R * (Cc + pad)].view(R, Cc + pad)[:, :Cc]
    x.copy_(torch.randn(R, Cc, generator=g).to(dev))
    return buf, x, (torch.randn(Cc, generator=g) * 3).to(dev)


@pytest.mark.parametrize("c", C.COLSUM, ids=lambda c: c["id"])
def test_colsum(dev, c):
    from spe_amd import kernels as K
    plan = _plan(c)
    R, Cc = c["R"], c["C"]
    buf, x, out0 = _colsum_input(c, dev)
    assert x.stride(0) == Cc + c.get("pad", 0) and (x.data_ptr() % 16 == 0) == C.aligned_of(c)
    figs = {}
    for acc in (True, False):
        runs = []
        for _ in range(2):
            fb, out = _framed(Cc, torch.float32, dev)
            if acc:
                out.copy_(out0)
            K.colsum(x, out=out, accumulate=acc)
            assert _frame_ok(fb, Cc), (c["id"], acc, "stored outside out")
            runs.append(out.clone())
        assert torch.equal(rs.bits(runs[0]), rs.bits(runs[1])), (c["id"], acc, "two runs differ")
        ref, mag = rs.colsum(x, out0 if acc else None)
        n = rs.n_add(plan["kernel"], R, plan["members"], acc)
        figs[f"acc{int(acc)}/bound"] = rs.worst_ratio(runs[0].double() - ref, rs.sum_bound(n, mag))
        figs[f"acc{int(acc)}_rel"] = rs.rel(runs[0], ref)
        assert bool(torch.isfinite(runs[0]).all()), (c["id"], acc, "a canary entered the sum")
    _say("colsum", c["id"], c["kernel"], f"members {c['members']}", _fig(figs))
    assert figs["acc1/bound"] <= 1.0 and figs["acc0/bound"] <= 1.0, (c["id"], figs)
    assert figs["acc1_rel"] < rs.REL_COLSUM and figs["acc0_rel"] < rs.REL_COLSUM, (c["id"], figs)
    assert rs.bits(buf).ne(FILL32).sum().item() <= R * Cc, "the input buffer was written"


@pytest.mark.parametrize("Cc", [4, 91, 4096])
def test_colsum_no_rows(dev, Cc):
    """R = 0: accumulate = 0 overwrites out with zeros, accumulate = 1 leaves it alone; the neighbours keep their canaries."""
    from spe_amd import kernels as K
    x = torch.empty((0, Cc), device=dev)
    fb, out = _framed(Cc, torch.float32, dev)
    K.colsum(x, out=out, accumulate=True)
    assert _untouched(fb)
    K.colsum(x, out=out, accumulate=False)
    assert bool((rs.bits(out) == 0).all()) and _frame_ok(fb, Cc)


# ------------------------------------------------------------------------------------------------------------------------------
# spe_layerscale_residual_fwd / _bwd
# ------------------------------------------------------------------------------------------------------------------------------
def _scales(R, rps, dev):
    """DropPath scales of ceil(R / rps) samples: sample 0 is dropped (exactly 0), the others hold inexact fp32 values."""
    if not rps:
        return None
    n = -(-R // rps)
    return torch.tensor([0.0, 1.0 / 0.7, 1.25, 1.0 / 0.9][:n] + [1.0 / 0.7] * max(n - 4, 0), dtype=torch.float32, device=dev)


@pytest.mark.parametrize("c", C.LSRES_FWD, ids=lambda c: c["id"])
def test_lsres_fwd(dev, c):
    _plan(c)
    R, Cc, rps = c["R"], c["C"], c.get("rps", 0)
    g = torch.Generator().manual_seed(3 * R + Cc)
    x, y = torch.randn(R, Cc, generator=g).to(dev), torch.randn(R, Cc, generator=g).to(dev)
    gamma = torch.randn(Cc, generator=g).to(dev)
    ss = _scales(R, rps, dev)
    fb, out = _framed(R * Cc, torch.float32, dev)
    assert _rc("spe_layerscale_residual_fwd", _p(x), _p(y), _p(gamma), _p(ss), _p(out), R, Cc, max(rps, 1)) == 0
    out = out.view(R, Cc)
    ref, bound = rs.lsres_fwd(x, y, gamma, ss, max(rps, 1))
    figs = {"out/bound": rs.worst_ratio(out.double() - ref, bound), "rel": rs.rel(out, ref)}
    _say("lsres_fwd", c["id"], _fig(figs))
    assert _frame_ok(fb, R * Cc) and figs["out/bound"] <= 1.0 and figs["rel"] < 1e-6, (c["id"], figs)
    if rps:
        assert torch.equal(rs.bits(out[:rps]), rs.bits(x[:rps])), "a dropped sample is x, bit for bit"


def test_lsres_fwd_refuses_odd_columns(dev):
    x = torch.randn(10, 6, device=dev)
    fb, out = _framed(60, torch.float32, dev)
    for Cc in (6, 5, 2):
        assert _rc("spe_layerscale_residual_fwd", _p(x), _p(x), _p(x), None, _p(out), 60 // Cc, Cc, 1) == -2
    assert _untouched(fb)


@pytest.mark.parametrize("c", C.LSRES_BWD, ids=lambda c: c["id"])
def test_lsres_bwd(dev, c):
    plan = _plan(c)
    R, Cc, rps, off, pre = c["R"], c["C"], c.get("rps", 0), c.get("off", 0), c.get("prefill", 0)
    g = torch.Generator().manual_seed(5 * R + Cc)
    dout, y = torch.randn(R, Cc, generator=g).to(dev), torch.randn(R, Cc, generator=g).to(dev)
    gamma = torch.randn(Cc, generator=g).to(dev)
    dg0 = (torch.randn(Cc, generator=g) * 3).to(dev) if pre else torch.zeros(Cc, device=dev)
    ss = _scales(R, rps, dev)
    dy_ref, dg_ref, mag = rs.lsres_bwd(dout, y, gamma, ss, max(rps, 1))
    runs = []
    for _ in range(2):
        fb, dy = _framed(R * Cc, torch.float32, dev, off)
        assert (dy.data_ptr() % 16 == 0) == (off % 4 == 0)
        fg, dg = _framed(Cc, torch.float32, dev)
        dg.copy_(dg0)
        assert _rc("spe_layerscale_residual_bwd", _p(dout), _p(y), _p(gamma), _p(ss), _p(dy), _p(dg), R, Cc, max(rps, 1)) == 0
        assert _frame_ok(fb, R * Cc, off) and _frame_ok(fg, Cc), (c["id"], "stored outside dy / dgamma")
        assert torch.equal(rs.bits(dy.view(R, Cc)), rs.bits(dy_ref)), (c["id"], "dy is (dout s) gamma, bit for bit")
        runs.append(dg.clone())
    assert torch.equal(rs.bits(runs[0]), rs.bits(runs[1])), (c["id"], "two runs differ")
    n = rs.n_add(plan["kernel"], R, plan["members"], True)
    ref = dg_ref + dg0.double()
    figs = {"dgamma/bound": rs.worst_ratio(runs[0].double() - ref, rs.sum_bound(n, mag + dg0.double().abs(), extra=2)),
            "dgamma_rel": rs.rel(runs[0], ref)}
    _say("lsres_bwd", c["id"], c["kernel"], f"members {c['members']}", _fig(figs))
    assert figs["dgamma/bound"] <= 1.0 and figs["dgamma_rel"] < rs.REL_GRAD, (c["id"], figs)


# ------------------------------------------------------------------------------------------------------------------------------
# spe_layerscale_residual_bwd16 / _bwd16d
# ------------------------------------------------------------------------------------------------------------------------------
SEED, OFFSET = 1234, 5


def _keep(R, Cc, p, dev):
    """The keep-scales of the (SEED, OFFSET) stream, element row * C + col being the flat index: spe_dropout of ones."""
    from spe_amd import kernels as K
    if not p:
        return None
    keep = K.dropout(torch.ones(R * Cc, device=dev), p, SEED, OFFSET).view(R, Cc)
    rate = rs.check_keep(keep.cpu(), p)
    _say("keep", f"R{R} C{Cc} p {p}", f"rate {rate:.4f}")
    return keep


def _bwd16_inputs(R, Cc, f16, rps, dev, seed):
    g = torch.Generator().manual_seed(seed)
    dout, y = torch.randn(R, Cc, generator=g).to(dev), torch.randn(R, Cc, generator=g).to(dev)
    gamma = (torch.randn(Cc, generator=g) * 0.3).to(dev)
    pre = (torch.randn(2, Cc, generator=g) * 3).to(dev)
    return dout, (y.half() if f16 else y), gamma, _scales(R, rps, dev), pre


def _bwd16_call(entry, dout, y, gamma, dy16, dy16T, ldt, db, dg, R, Cc, p=0.0, ss=None, rps=1):
    f16 = int(y.dtype == torch.float16)
    if entry == "bwd16d":
        return _rc("spe_layerscale_residual_bwd16d", _p(dout), _p(y), f16, _p(gamma), _p(dy16), _p(dy16T), ldt, _p(db), _p(dg), R, Cc,
                   float(p), SEED, OFFSET, _p(ss), rps)
    return _rc("spe_layerscale_residual_bwd16", _p(dout), _p(y), f16, _p(gamma), _p(dy16), _p(dy16T), ldt, _p(db), _p(dg), R, Cc)


@pytest.mark.parametrize("c", C.LSRES_BWD16, ids=lambda c: c["id"])
def test_lsres_bwd16(dev, c):
    plan = _plan(c)
    R, Cc, ldt = c["R"], c["C"], C.ldt_of(c)
    entry, p, rps, outs, pre_on = c.get("entry", "bwd16"), c.get("p", 0.0), c.get("rps", 0), c.get("outs", "both"), c.get("prefill", 0)
    dout, y, gamma, ss, pre = _bwd16_inputs(R, Cc, c.get("f16", 0), rps, dev, 11 * R + Cc)
    if not pre_on:
        pre = torch.zeros_like(pre)
    keep = _keep(R, Cc, p, dev)
    ref = rs.lsres_bwd16(dout, y, gamma, keep, ss, max(rps, 1), ldt)
    runs = []
    for _ in range(2):
        f1, dy16 = _framed(R * Cc, torch.bfloat16, dev)
        f2, dy16T = _framed(Cc * ldt, torch.bfloat16, dev)
        fs, sums = _framed(2 * Cc, torch.float32, dev)
        sums.copy_(pre.view(-1))
        dg, db = sums[:Cc], sums[Cc:]
        rc = _bwd16_call(entry, dout, y, gamma, dy16 if outs != "T" else None, dy16T if outs != "row" else None, ldt, db, dg, R, Cc, p, ss, max(rps, 1))
        assert rc == 0, (c["id"], rc)
        assert _frame_ok(f1, R * Cc) and _frame_ok(f2, Cc * ldt) and _frame_ok(fs, 2 * Cc), (c["id"], "stored outside an output")
        if outs == "T":
            assert _untouched(dy16)
        else:
            assert torch.equal(rs.bits(dy16.view(R, Cc)), rs.bits(ref["dy16"])), (c["id"], "dy16 is bf16(((dout s) keep) gamma), bit for bit")
        if outs == "row":
            assert _untouched(dy16T)
        else:
            got = rs.bits(dy16T.view(Cc, ldt))
            assert torch.equal(got[:, :R], rs.bits(ref["dy16T"])[:, :R]), (c["id"], "dy16T is the transpose of dy16")
            # zeros by value, exactly: the kernel stages 0 * gamma for a row past R, so the padding under a negative gamma is -0.0 (bits
            # 0x8000) - as an operand of the weight-gradient product it adds what +0.0 adds
            assert bool((dy16T.view(Cc, ldt)[:, R:].float() == 0).all()), (c["id"], "the columns from R to ldt are exact zeros")
        runs.append(sums.clone())
    assert torch.equal(rs.bits(runs[0]), rs.bits(runs[1])), (c["id"], "two runs differ")
    tiles = ldt // 64
    n = rs.n_add(plan["kernel"], R, plan["members"], True, tiles=tiles)
    dgr, dbr = ref["dgamma"] + pre[0].double(), ref["db"] + pre[1].double()
    figs = {"dgamma/bound": rs.worst_ratio(runs[0][:Cc].double() - dgr, rs.sum_bound(n, ref["dgamma_mag"] + pre[0].double().abs(), extra=1)),
            "db/bound": rs.worst_ratio(runs[0][Cc:].double() - dbr, rs.sum_bound(n, ref["db_mag"] + pre[1].double().abs())),
            "dgamma_rel": rs.rel(runs[0][:Cc], dgr), "db_rel": rs.rel(runs[0][Cc:], dbr)}
    _say("lsres_bwd16", c["id"], c["kernel"], f"members {c['members']}", _fig(figs))
    assert figs["dgamma/bound"] <= 1.0 and figs["db/bound"] <= 1.0, (c["id"], figs)
    assert figs["dgamma_rel"] < rs.REL_GRAD and figs["db_rel"] < rs.REL_GRAD, (c["id"], figs)


@pytest.mark.parametrize("r", C.BWD16_REFUSALS, ids=lambda r: r["id"])
def test_lsres_bwd16_refusals(dev, r):
    """-2, and every output keeps its canaries."""
    R, Cc, off = r["R"], r["C"], r.get("off", 0)
    ldt = r.get("ldt", -(-R // 64) * 64)
    dout, y, gamma, _, _ = _bwd16_inputs(R, Cc, 0, 0, dev, 3)
    ss = torch.ones(2, device=dev) if "rps" in r else None
    f1, dy16 = _framed(R * Cc, torch.bfloat16, dev, 2 * off)              # off floats = 4 bytes = 2 bf16 off alignment
    f2, dy16T = _framed(Cc * max(ldt, R), torch.bfloat16, dev)
    fs, sums = _framed(2 * Cc, torch.float32, dev)
    entry = "bwd16d" if ("p" in r or "rps" in r) else "bwd16"
    rc = _bwd16_call(entry, dout, y, gamma, dy16, dy16T, ldt, sums[Cc:], sums[:Cc], R, Cc, r.get("p", 0.0), ss, r.get("rps", 1))
    assert rc == -2, (r["id"], rc)
    torch.cuda.synchronize()
    assert _untouched(f1) and _untouched(f2) and _untouched(fs), r["id"]


# ------------------------------------------------------------------------------------------------------------------------------
# spe_act_bwd
# ------------------------------------------------------------------------------------------------------------------------------
def _act(dy, aux, mode, n):
    fb, dx = _framed(n, torch.float32, dy.device)
    assert _rc("spe_act_bwd", _p(dy), _p(aux), _p(dx), n, mode) == 0
    assert _frame_ok(fb, n), "stored outside dx"
    return dx


@pytest.mark.parametrize("c", C.ACT_BWD, ids=lambda c: c["id"])
def test_act_bwd_relu_exact(dev, c):
    _plan(c)
    n = c["R"]
    g = torch.Generator().manual_seed(n)
    den = 2.0 ** -149
    special = torch.tensor([0.0, -0.0, den, -den, float("inf"), float("-inf")])
    aux = torch.randn(n, generator=g)
    idx = torch.arange(0, n, max(n // 64, 1))
    aux[idx] = special[torch.arange(idx.numel()) % 6]
    aux[:4] = special[:4]
    if n >= 8:
        aux[-2:] = special[4:]
    dy = torch.randn(n, generator=g)
    aux, dy = aux.to(dev), dy.to(dev)
    assert rs.bits(aux[:4]).tolist() == [0, -2 ** 31, 1, -2 ** 31 + 1]          # the zeros and denormals arrived on the device as such
    dx = _act(dy, aux, 1, n)
    assert torch.equal(rs.bits(dx), rs.bits(rs.relu_bwd(dy, aux))), c["id"]
    _say("act_bwd relu", c["id"], "bit for bit")


def _gelu_check(dev, dy, h, tag):
    n = h.numel()
    dx = _act(dy, h, 2, n)
    yard = rs.gelu_err_units(rs.torch_gelu_bwd(dy, h), dy, h)
    mine = rs.gelu_err_units(dx, dy, h)
    figs = {"kernel_units": mine, "torch_fp32_units": yard, "allowance": rs.gelu_allowance(yard), "rel": rs.rel(dx, rs.gelu_bwd(dy, h))}
    _say("act_bwd gelu", tag, _fig(figs))
    assert bool(torch.isfinite(dx).all()) and mine <= rs.gelu_allowance(yard) and figs["rel"] < rs.REL_GRAD, (tag, figs)
    return dx


@pytest.mark.parametrize("c", C.ACT_BWD, ids=lambda c: c["id"])
def test_act_bwd_gelu_random(dev, c):
    n = c["R"]
    g = torch.Generator().manual_seed(n + 1)
    h, dy = (torch.randn(n, generator=g) * 3).to(dev), torch.randn(n, generator=g).to(dev)
    _gelu_check(dev, dy, h, c["id"])


def test_act_bwd_gelu_grid(dev):
    g = torch.Generator().manual_seed(9)
    h = torch.cat([torch.linspace(-12, 12, 4801), torch.tensor([40.0, -40.0, 0.0])]).to(dev)
    dy = torch.randn(4804, generator=g).to(dev)
    dx = _gelu_check(dev, dy, h, "grid [-12, 12] and +-40")
    assert torch.equal(rs.bits(dx[4801:4802]), rs.bits(dy[4801:4802])), "gelu'(40) is exactly 1"
    assert dx[4802].item() == 0.0, "gelu'(-40) is exactly +-0"


def test_act_bwd_refuses_odd_counts(dev):
    x = torch.randn(1024, device=dev)
    fb, dx = _framed(1024, torch.float32, dev)
    for n in (1, 2, 1022, 1023):
        for mode in (1, 2):
            assert _rc("spe_act_bwd", _p(x), _p(x), _p(dx), n, mode) == -2
    assert _untouched(fb)


# ------------------------------------------------------------------------------------------------------------------------------
# spe_dropout
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", C.DROPOUT_P)
@pytest.mark.parametrize("c", C.DROPOUT, ids=lambda c: c["id"])
def test_dropout(dev, c, p):
    _plan(c)
    n = c["R"]
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    x[x == 0] = 1.0
    x = x.to(dev)

    def run(inp, offset):
        fb, y = _framed(n, torch.float32, dev)
        assert _rc("spe_dropout", _p(inp), _p(y), n, float(p), SEED, offset) == 0
        assert _frame_ok(fb, n), "stored outside y"
        return y

    y = run(x, OFFSET)
    mask = rs.check_dropout(x, y, p)
    ones = torch.ones(n, device=dev)
    assert torch.equal(rs.check_dropout(ones, run(ones, OFFSET), p), mask), "the mask depends on x"
    assert torch.equal(rs.bits(run(x, OFFSET)), rs.bits(y)), "two calls with one (seed, offset) differ"
    rate = mask.double().mean().item()
    _say("dropout", c["id"], f"p {p} keep rate {rate:.4f}")
    if p == 0:
        assert torch.equal(rs.bits(y), rs.bits(x))
        return
    if n >= 255:
        assert not torch.equal(rs.check_dropout(x, run(x, OFFSET + 1), p), mask), "two offsets give one mask"
        assert abs(rate - (1 - p)) <= (0.03 if n > 10000 else 0.12)       # 255 draws: four standard deviations of a binomial at p = 0.5


# ------------------------------------------------------------------------------------------------------------------------------
# the deferred sums, directly
# ------------------------------------------------------------------------------------------------------------------------------
def _pending():
    from spe_amd import kernels as K
    return K.lib.load().spe_reduce_pending()


@contextlib.contextmanager
def _deferral(flat, arena_bytes):
    from spe_amd import kernels as K
    K.defer_reductions(None)
    K._DEFER_ARENA = None                   # an arena of this test's size; the next owner of the buckets allocates its own again
    try:
        K.defer_reductions([flat], arena_bytes=arena_bytes)
        assert K._DEFER_FLATS is not None, "deferral is switched off (SPE_DEFER_REDUCE=0)"
        yield
    finally:
        K.defer_reductions(None)
        K._DEFER_ARENA = None


class _Prob:
    """One lsres_bwd16 problem: inputs, fp64 sums, the bounds of the tree and of the flush."""

    def __init__(self, dev, R, Cc, seed):
        from spe_amd import kernels as K
        self.R, self.C, self.ldt = R, Cc, -(-R // 64) * 64
        self.dout, self.y, self.gamma, _, _ = _bwd16_inputs(R, Cc, 0, 0, dev, seed)
        self.ref = rs.lsres_bwd16(self.dout, self.y, self.gamma)
        plan = K.rowops_plan("lsres_bwd16", R, Cc)
        self.members, self.kernel = plan["members"], plan["kernel"]
        self.dy16 = torch.empty(R * Cc, dtype=torch.bfloat16, device=dev)

    def launch(self, dg, db):
        assert _bwd16_call("bwd16", self.dout, self.y, self.gamma, self.dy16, None, self.ldt, db, dg, self.R, self.C) == 0

    def bounds(self, deferred, pre_dg=None, pre_db=None):
        n = rs.n_add(self.kernel, self.R, self.members, True, tiles=self.ldt // 64, deferred=deferred)
        mg = self.ref["dgamma_mag"] + (0 if pre_dg is None else pre_dg.double().abs())
        mb = self.ref["db_mag"] + (0 if pre_db is None else pre_db.double().abs())
        return rs.sum_bound(n, mg, extra=1), rs.sum_bound(n, mb)

    def check(self, dg, db, deferred, tag, pre_dg=None, pre_db=None):
        bg, bb = self.bounds(deferred, pre_dg, pre_db)
        rg = self.ref["dgamma"] + (0 if pre_dg is None else pre_dg.double())
        figs = {}
        if dg is not None:
            figs["dgamma/bound"] = rs.worst_ratio(dg.double() - rg, bg)
        if db is not None:
            figs["db/bound"] = rs.worst_ratio(db.double() - (self.ref["db"] + (0 if pre_db is None else pre_db.double())), bb)
        _say("deferred" if deferred else "tree", tag, f"members {self.members}", _fig(figs))
        assert all(v <= 1.0 for v in figs.values()), (tag, figs)


def _tickets_clean():
    from spe_amd import kernels as K
    torch.cuda.synchronize()
    return not bool(K._RWS[:64 * 1024].any())


def test_deferred_basics(dev):
    """Destinations inside the registered range stay as they were until the flush; then they hold the sums (flush order: same bound as
    the tree, and the tree's result to within both bounds).  One-member launches, a destination outside the range: immediate.  NULL db."""
    from spe_amd import kernels as K
    Cc = 64
    pr = _Prob(dev, 129, Cc, 21)
    g = torch.Generator().manual_seed(1)
    flat0 = (torch.randn(4096, generator=g) * 3).to(dev)
    tree = flat0[:2 * Cc].clone()
    pr.launch(tree[:Cc], tree[Cc:])
    pr.check(tree[:Cc], tree[Cc:], False, "bwd16 R129", flat0[:Cc], flat0[Cc:2 * Cc])
    results = []
    for _ in range(2):
        flat = flat0.clone()
        with _deferral(flat, 1 << 20):
            assert _pending() == 0
            pr.launch(flat[:Cc], flat[Cc:2 * Cc])
            assert _pending() == 1
            torch.cuda.synchronize()
            assert torch.equal(rs.bits(flat), rs.bits(flat0)), "a deferred destination changed before the flush"
            K.reduce_flush()
            assert _pending() == 0
            pr.check(flat[:Cc], flat[Cc:2 * Cc], True, "bwd16 R129", flat0[:Cc], flat0[Cc:2 * Cc])
            assert torch.equal(rs.bits(flat[2 * Cc:]), rs.bits(flat0[2 * Cc:])), "the flush wrote outside its destinations"
            bt, bd = pr.bounds(False, flat0[:Cc], flat0[Cc:2 * Cc]), pr.bounds(True, flat0[:Cc], flat0[Cc:2 * Cc])
            assert rs.worst_ratio(flat[:Cc].double() - tree[:Cc].double(), bt[0] + bd[0]) <= 1.0
            assert rs.worst_ratio(flat[Cc:2 * Cc].double() - tree[Cc:].double(), bt[1] + bd[1]) <= 1.0
            results.append(flat[:2 * Cc].clone())
            # NULL db: dgamma alone is deferred
            pr.launch(flat[1024:1024 + Cc], None)
            assert _pending() == 1
            K.reduce_flush()
            pr.check(flat[1024:1024 + Cc], None, True, "bwd16 R129 db NULL", flat0[1024:1024 + Cc])
            assert torch.equal(rs.bits(flat[1024 + Cc:]), rs.bits(flat0[1024 + Cc:]))
            # a destination outside the registered range: the tree, at once, bit for bit what the tree gave without deferral
            out_db = flat0[Cc:2 * Cc].clone()
            flat[:Cc] = flat0[:Cc]
            pr.launch(flat[:Cc], out_db)
            assert _pending() == 0
            assert torch.equal(rs.bits(flat[:Cc]), rs.bits(tree[:Cc])) and torch.equal(rs.bits(out_db), rs.bits(tree[Cc:]))
            # one member (R <= 64): stored directly, never deferred
            one = _Prob(dev, 64, Cc, 22)
            assert one.members == 1
            one.launch(flat[2048:2048 + Cc], flat[2048 + Cc:2048 + 2 * Cc])
            assert _pending() == 0
            one.check(flat[2048:2048 + Cc], flat[2048 + Cc:2048 + 2 * Cc], True, "bwd16 R64", flat0[2048:2048 + Cc], flat0[2048 + Cc:2048 + 2 * Cc])
    assert torch.equal(rs.bits(results[0]), rs.bits(results[1])), "two deferred runs differ"
    assert _tickets_clean()


def test_deferred_layernorm_bwd(dev):
    """The LayerNorm backward's dgamma / dbeta as deferred sums: untouched until the flush, then inside the bounds of rownorm_ref."""
    from spe_amd import kernels as K
    R, Cc, eps = 100, 64, 1e-6
    g = torch.Generator().manual_seed(31)
    x, dy = (torch.randn(R, Cc, generator=g) * 3 + 1).to(dev), torch.randn(R, Cc, generator=g).to(dev)
    gamma, beta = torch.randn(Cc, generator=g).to(dev), torch.randn(Cc, generator=g).to(dev)
    _, mean, rstd = K.layernorm_fwd(x, gamma, beta, eps)
    dx_t, dg_t, db_t = K.layernorm_bwd(dy, x, gamma, mean, rstd)
    _, dg_ref, db_ref, _ = rr.ln_bwd(dy, x, gamma, eps)
    b = rr.ln_bwd_bounds(dy, x, gamma, eps)
    flat = torch.zeros(1024, device=dev)
    with _deferral(flat, 1 << 20):
        dx, _, _ = K.layernorm_bwd(dy, x, gamma, mean, rstd, dg_out=flat[:Cc], db_out=flat[Cc:2 * Cc])
        assert _pending() == 1
        torch.cuda.synchronize()
        assert not bool(flat.any()), "a deferred destination changed before the flush"
        K.reduce_flush()
        assert _pending() == 0 and torch.equal(rs.bits(dx), rs.bits(dx_t)) and not bool(flat[2 * Cc:].any())
        figs = {"dgamma/bound": rr.worst_ratio(flat[:Cc].double() - dg_ref, b["dgamma"]), "dbeta/bound": rr.worst_ratio(flat[Cc:2 * Cc].double() - db_ref, b["dbeta"]),
                "dgamma_vs_tree": rs.rel(flat[:Cc], dg_t), "dbeta_vs_tree": rs.rel(flat[Cc:2 * Cc], db_t)}
        _say("deferred layernorm_bwd R100 C64 members 7", _fig(figs))
        assert figs["dgamma/bound"] <= 1.0 and figs["dbeta/bound"] <= 1.0 and figs["dgamma_vs_tree"] < 1e-5 and figs["dbeta_vs_tree"] < 1e-5, figs


def test_deferred_table_full(dev):
    """24 launches pending, then a 25th: the library flushes the 24 by itself (pending 24 -> 1).  The 24 are conversions with a column sum
    (spe_cvt_bf16: one segment each, so the table fills before the 40 segments do); the 25th is an lsres_bwd16."""
    from spe_amd import kernels as K
    Cc = 64
    pr = _Prob(dev, 129, Cc, 23)
    g = torch.Generator().manual_seed(29)
    x = torch.randn(129, Cc, generator=g).to(dev)
    ref, mag = rs.colsum(x)
    flat = torch.zeros(26 * Cc, device=dev)
    rows = flat.view(26, Cc)
    with _deferral(flat, 1 << 20):
        for k in range(24):
            K.cvt_bf16(x, True, colsum_out=rows[k])
            assert _pending() == k + 1, k
        torch.cuda.synchronize()
        assert not bool(flat.any()), "a deferred destination changed before the flush"
        pr.launch(rows[24], rows[25])
        assert _pending() == 1
        torch.cuda.synchronize()
        assert not bool(rows[24:].any()), "the 25th launch is still pending"
        figs = {"colsum/bound": rs.worst_ratio(rows[0].double() - ref, rs.sum_bound(128, mag)), "rel": rs.rel(rows[0], ref)}      # T - 1 additions at most
        _say("deferred cvt_bf16 colsum R129 C64, table full", _fig(figs))
        assert figs["colsum/bound"] <= 1.0 and figs["rel"] < rs.REL_COLSUM, figs
        assert all(torch.equal(rs.bits(rows[k]), rs.bits(rows[0])) for k in range(1, 24)), "an entry of the automatic flush differs"
        K.reduce_flush()
        assert _pending() == 0
        pr.check(rows[24], rows[25], True, "table full, 25th launch")


def test_deferred_segments_full(dev):
    """The LayerNorm backward with the LayerScale ride-along records 4 segments: 10 launches fill the 40, the 11th flushes them."""
    from spe_amd import kernels as K
    R, Cc, eps = 100, 64, 1e-6
    g = torch.Generator().manual_seed(33)
    x, dy, lsy = (torch.randn(R, Cc, generator=g) * 3 + 1).to(dev), torch.randn(R, Cc, generator=g).to(dev), torch.randn(R, Cc, generator=g).to(dev)
    gamma, beta, lgam = (torch.randn(Cc, generator=g).to(dev) for _ in range(3))
    _, mean, rstd = K.layernorm_fwd(x, gamma, beta, eps)
    _, dg_t, db_t, (_, ldb_t, ldg_t) = K.layernorm_bwd(dy, x, gamma, mean, rstd, ls=(lsy, lgam, None, None))
    flat = torch.zeros(11 * 4 * Cc, device=dev)
    rows = flat.view(11, 4, Cc)
    with _deferral(flat, 1 << 20):
        for k in range(11):
            K.layernorm_bwd(dy, x, gamma, mean, rstd, dg_out=rows[k, 0], db_out=rows[k, 1], ls=(lsy, lgam, rows[k, 2], rows[k, 3]))
            assert _pending() == (k + 1 if k < 10 else 1), k
        torch.cuda.synchronize()
        assert not bool(rows[10].any()) and bool(rows[9].any())
        K.reduce_flush()
        assert _pending() == 0
        assert all(torch.equal(rs.bits(rows[k]), rs.bits(rows[0])) for k in range(1, 11))
        figs = {n: rs.rel(rows[0, i], t) for i, (n, t) in enumerate((("dgamma", dg_t), ("dbeta", db_t), ("ls_db", ldb_t), ("ls_dg", ldg_t)))}
        _say("deferred layernorm_bwd_ls vs tree, 40 segments", _fig(figs))
        assert all(v < 1e-5 for v in figs.values()), figs
    # two segments per launch (lsres_bwd16): 20 launches fill the 40, the 21st flushes them
    pr = _Prob(dev, 129, Cc, 34)
    flat = torch.zeros(21 * 2 * Cc, device=dev)
    rows = flat.view(21, 2, Cc)
    with _deferral(flat, 1 << 20):
        for k in range(21):
            pr.launch(rows[k, 0], rows[k, 1])
            assert _pending() == (k + 1 if k < 20 else 1), k
        torch.cuda.synchronize()
        assert not bool(rows[20].any()) and bool(rows[19].any())
        K.reduce_flush()
        assert _pending() == 0
        pr.check(rows[0, 0], rows[0, 1], True, "40 segments, entry 0")
        assert all(torch.equal(rs.bits(rows[k]), rs.bits(rows[0])) for k in range(1, 21))


def test_deferred_small_arena(dev):
    """An arena of 1024 floats: two launches of 384 fit, the third flushes them first; a launch that needs more than the whole arena
    takes the tree (immediate) and leaves the pending one pending."""
    from spe_amd import kernels as K
    Cc = 64
    pr, big = _Prob(dev, 129, Cc, 24), _Prob(dev, 16385, Cc, 25)
    assert big.members * 2 * Cc > 1024
    flat = torch.zeros(4 * 2 * Cc, device=dev)
    rows = flat.view(4, 2, Cc)
    with _deferral(flat, 4096):
        for k, want in ((0, 1), (1, 2), (2, 1)):
            pr.launch(rows[k, 0], rows[k, 1])
            assert _pending() == want, k
        torch.cuda.synchronize()
        assert bool(rows[0].any()) and bool(rows[1].any()) and not bool(rows[2].any())
        big.launch(rows[3, 0], rows[3, 1])
        assert _pending() == 1
        torch.cuda.synchronize()
        assert not bool(rows[2].any())
        big.check(rows[3, 0], rows[3, 1], False, "larger than the arena R16385")
        K.reduce_flush()
        assert _pending() == 0
        pr.check(rows[2, 0], rows[2, 1], True, "small arena, third launch")
        assert torch.equal(rs.bits(rows[1]), rs.bits(rows[0])) and torch.equal(rs.bits(rows[2]), rs.bits(rows[0]))
    assert _tickets_clean()


def test_deferred_overlap(dev):
    """Two launches into one destination: the second flushes the first (one producer per destination and flush); the end is the sum."""
    from spe_amd import kernels as K
    Cc = 64
    a, b = _Prob(dev, 129, Cc, 26), _Prob(dev, 200, Cc, 27)
    flat = torch.zeros(2 * Cc, device=dev)
    with _deferral(flat, 1 << 20):
        a.launch(flat[:Cc], flat[Cc:])
        assert _pending() == 1
        b.launch(flat[:Cc], flat[Cc:])
        assert _pending() == 1
        torch.cuda.synchronize()
        a.check(flat[:Cc], flat[Cc:], True, "overlap, first launch flushed")
        mid = flat.clone()
        K.reduce_flush()
        assert _pending() == 0
        b.check(flat[:Cc], flat[Cc:], True, "overlap, sum of both", mid[:Cc], mid[Cc:])


# ------------------------------------------------------------------------------------------------------------------------------
# last: nothing is left behind
# ------------------------------------------------------------------------------------------------------------------------------
def test_workspace_is_left_clean(dev):
    """After everything above: no ticket is non-zero, nothing is pending, and a small colsum and lsres_bwd still match their reference."""
    from spe_amd import kernels as K
    assert _pending() == 0 and K._DEFER_FLATS is None
    assert _tickets_clean(), "a ticket of the reduction workspace was left non-zero"
    g = torch.Generator().manual_seed(41)
    x = torch.randn(300, 64, generator=g).to(dev)
    out = K.colsum(x, out=torch.zeros(64, device=dev))
    ref, mag = rs.colsum(x)
    plan = K.rowops_plan("colsum", 300, 64)
    assert plan["members"] == 5
    r1 = rs.worst_ratio(out.double() - ref, rs.sum_bound(rs.n_add(plan["kernel"], 300, 5, False), mag))
    dout, y, gamma = torch.randn(300, 64, generator=g).to(dev), torch.randn(300, 64, generator=g).to(dev), torch.randn(64, generator=g).to(dev)
    dy, dg = K.layerscale_residual_bwd(dout, y, gamma, None, 1, dg_out=torch.zeros(64, device=dev))
    dy_ref, dg_ref, mag2 = rs.lsres_bwd(dout, y, gamma)
    plan = K.rowops_plan("lsres_bwd", 300, 64)
    r2 = rs.worst_ratio(dg.double() - dg_ref, rs.sum_bound(rs.n_add(plan["kernel"], 300, plan["members"], False), mag2, extra=2))
    _say("hygiene", f"colsum/bound {r1:.3e} dgamma/bound {r2:.3e}")
    assert r1 <= 1.0 and r2 <= 1.0 and torch.equal(rs.bits(dy), rs.bits(dy_ref))
    assert _tickets_clean()
