"""The small-row Linear kernels (csrc/linear_small.hip: spe_linear_small_fwd / _bwd / _group_fwd / _group_bwd, six kernel instances) against
fp64 references, EXACTLY, at every chunk, tile, stride, NULL-pointer and store-path edge (cases and the edges each reaches:
tests/linear_small_cases.py, whose coverage tests/test_linear_small_plan_cpu.py proves without a device; references and bounds:
tests/linear_small_ref.py).  The entries are called through their C ABI so that strides, NULL pointers and misaligned bases can be
passed; the production wrappers kernels.linear_fwd / linear_bwd / linear_group_fwd / linear_group_bwd are called once each.

Operands.  Small integers times powers of two that sit only on indices no product of the call contracts, so that every fp32 partial sum is
an integer below 2^24 times one scale - exact in any order; each test asserts that bound in fp64 before it trusts equality.
  forward, plain   x integers in [-255, 255] (bf16 holds them), W integers in [-4, 4] times 2^f[n], bias an integer times 2^f[n]
  forward, split   x integers of up to 12 significant bits: both halves of the in-kernel split are nonzero and bf16(x) + bf16(x - bf16(x)) == x
                   (asserted); W16 and W16lo two independent integer arrays in [-4, 4] times 2^f[n]; the reference is xh Wh + xh Wl + xl Wh -
                   the kernel drops lo x lo, and that is pinned.  The bit count shrinks until the 2^24 bound holds for the case's K.
  "ties"           x odd integers of 9 bits, each exactly halfway between two bf16 neighbours: staging must round to nearest even
  backward         dy integers in [-255, 255] without a scale (it is contracted over n for dx and over r for dW); the rows of WT16 and the
                   columns of x16 carry 2^f[k] / 2^g[k]; where db is the only output dy holds 12-bit integers, which bf16 cannot: db is the
                   sum of dy' itself.  ReLU: aux holds +0, -0, positive and negative values, pinning aux > 0.
  groups           every block has its own random weights, biases, addends and gradients
Bounded cases, two kinds only: GELU and its derivative against the fp64 formula (c times the unit error, c = 4 x the worst ratio of the
plain fp32 formula measured in the same run with torch on the host on the same arguments; the factor 4 covers spe_erff / __expf against
libm), and one random-normal case per instance against the rounding bounds of tests/linear_small_ref.py, printed next to the ratio of the
torch emulation.

Buffers.  Every input is a block of a NaN-filled buffer (3 rows behind, 16 elements before, x also between the rows when ldx = K + 12): a
finite result proves that nothing outside the block entered a product.  Every output is NaN-filled with 2 rows behind and 8 elements
before and behind; everything outside the contract region must still be NaN afterwards, and a second call must give the same bits.
Measured: profiles/linear_small_edges.txt (every line this module prints with the prefix LINSMALL)."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_small_cases as C  # noqa: E402
import linear_small_ref as REF  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
BF = torch.bfloat16
TWO24 = 2.0 ** 24


class In:
    """A 2-D (or 1-D) operand as a block of a NaN-filled buffer: 16 elements before it, 3 rows behind it, ld - C columns around each row."""

    def __init__(self, t, dtype, dev, ld=None, col0=0):
        t2 = t.reshape(1, -1) if t.dim() == 1 else t
        R, Cc = t2.shape
        ld = ld or Cc
        self.flat = torch.full((16 + (R + 3) * ld,), NAN, dtype=dtype, device=dev)
        view = self.flat[16:].view(R + 3, ld)[:R, col0:col0 + Cc]
        view.copy_(t2.to(dev))
        assert torch.equal(view.double(), t2.to(dev).double()), "the operand is not exact in its storage type"
        assert int(torch.isnan(self.flat).sum()) == self.flat.numel() - R * Cc
        self.ptr, self.ld = view.data_ptr(), ld
        assert self.ptr % 16 == 0


class Out:
    """A [rows, cols] result with row stride ld inside a NaN-filled buffer: 8 + off elements before it (off = 1: one element behind a
    16-byte boundary), 2 rows and 8 elements behind it."""

    def __init__(self, rows, cols, dev, ld=None, off=0, dtype=torch.float32):
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        self.start = 8 + off
        self.flat = torch.full((self.start + (rows + 2) * self.ld + 8,), NAN, dtype=dtype, device=dev)
        self.ptr = self.flat.data_ptr() + self.start * self.flat.element_size()
        assert self.flat.data_ptr() % 16 == 0 and self.ptr % 16 == (off * self.flat.element_size()) % 16

    def _region(self, flat):
        return flat[self.start:self.start + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]

    def inside(self):
        return self._region(self.flat)

    def outside_is_nan(self):
        c = self.flat.clone()
        self._region(c).fill_(NAN)
        return bool(torch.isnan(c).all())

    def all_nan(self):
        return bool(torch.isnan(self.flat).all())

    def bits(self):
        return self.flat.view(torch.int16 if self.flat.dtype == BF else torch.int32).clone()


def _ptr(o):
    return None if o is None else o.ptr


def _same_bits(outs, first):
    return all(torch.equal(o.bits(), b) for o, b in zip(outs, first))


def _check_exact(out, ref64, tag):
    got = out.inside()
    assert bool(torch.isfinite(got).all()), f"{tag}: NaN or inf inside the result - something outside the operand blocks entered a product"
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64), f"{tag}: the reference is not an fp32 number"
    assert torch.equal(got, ref), f"{tag}: {int((got != ref).sum())} of {ref.numel()} elements differ from the fp64 reference, " \
                                  f"first at {[int(v) for v in (got != ref).nonzero()[0]]}"
    assert out.outside_is_nan(), f"{tag}: a store left the contract region"


def _check_bounded(out, ref64, bound, tag):
    got = out.inside()
    assert bool(torch.isfinite(got).all()), f"{tag}: NaN or inf inside the result"
    ratio = float(((got.double() - ref64).abs() / bound.clamp_min(1e-300)).max())
    assert out.outside_is_nan(), f"{tag}: a store left the contract region"
    return ratio


def _scales(g, n, gelu_typ=None):
    """Powers of two for an index that is not contracted; gelu_typ: the typical size of the unscaled product, divided out (results of order 1)."""
    if gelu_typ is not None:
        return 2.0 ** (-round(math.log2(gelu_typ)) + torch.randint(-1, 2, (n,), generator=g).double())
    return 2.0 ** torch.randint(-12, 13, (n,), generator=g).double()


def _signed_bits(g, shape, bits):
    """Random integers with exactly `bits` significant bits (top bit set), either sign."""
    v = torch.randint(2 ** (bits - 1), 2 ** bits, shape, generator=g).double()
    return v * (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()


def _gelu_c(arg, formula32, ref64, unit):
    """c = 4 x the worst ratio of the plain fp32 formula, evaluated with torch on the host on the same arguments; -> (c, that ratio)."""
    f32 = formula32(arg.float().cpu()).double()
    worst = float(((f32 - ref64.cpu()).abs() / unit.cpu()).max())
    return 4.0 * worst, worst


# ---- forward ------------------------------------------------------------------------------------------------------------------------------
def _fwd_operands(c, dev, seed, nblk=1):
    """-> (x fp64 [R, K], [Wh_i], [Wl_i] or None, f [N], bits) for nblk blocks sharing x; exactness of the split asserted here."""
    R, N, K_, split, fl = c["R"], c["N"], c["K"], c["split"], c.get("flags", "")
    g = torch.Generator().manual_seed(seed)
    bits = 12 if split else 8
    if "t" in fl:
        x, hand = REF.ties_bf16(g, (R, K_))
        assert torch.equal(REF.hilo(x)[0], hand)                   # the reference rounds ties to even, worked out by hand
        bits = 9
    else:
        while (2 ** bits) * 8 * K_ + 2 ** 12 >= TWO24:             # (|xh| + |xl|) (|Wh| + |Wl|) K + addend + bias stays below 2^24
            bits -= 1
        assert bits >= (10 if split else 8)
        x = _signed_bits(g, (R, K_), bits) if split else REF.ints(g, (R, K_), 255)
    typ = (2 ** bits) * 0.6 * 2.6 * math.sqrt(K_) if c.get("act") == 2 else None
    f = _scales(g, N, typ)
    Whs = [REF.ints(g, (N, K_), 4) * f[:, None] for _ in range(nblk)]
    Wls = [REF.ints(g, (N, K_), 4) * f[:, None] for _ in range(nblk)] if split else None
    xh, xl = REF.hilo(x)
    assert torch.equal(xh + xl, x)
    if split:
        assert bool((xl != 0).any()) and bool((xh != 0).all())   # both halves of the in-kernel split are live
    elif "t" not in fl:
        assert not bool(xl.any())
    return x, Whs, Wls, f, g


def _assert_fwd_exact(x, Wh, Wl, f, extra):
    xh, xl = REF.hilo(x)
    mag = (xh.abs() + xl.abs()) @ (Wh.abs() + (Wl.abs() if Wl is not None else 0)).t() + extra
    assert float((mag / f[None, :]).max()) < TWO24


@pytest.mark.parametrize("c", C.FWD_CASES, ids=lambda c: c["id"])
def test_linear_small_fwd(dev, c):
    """spe_linear_small_fwd, one case of tests/linear_small_cases.py on the instance the launcher's own plan names, every ldc variant: y, pre
    and x16_out equal to the fp64 reference (GELU and random-normal: inside the bound), nothing written outside, the same bits twice."""
    from spe_amd import kernels as K
    R, N, K_, split, act, fl = c["R"], c["N"], c["K"], c["split"], c["act"], c["flags"]
    ldx = K_ + (12 if "s" in fl else 0)
    plan = K.linear_small_plan("fwd", R, N, K_, ldx=ldx, split=split)
    name = C.kernel_name("fwd", plan)
    assert plan["status"] == 0 and name == C.instance_of(c)
    random = "r" in fl
    if random:
        x32, Wh, Wl = REF.random_operands(c, dev)
        x, g = x32.double(), torch.Generator().manual_seed(5)
        bias = torch.randn((N,), generator=g).double().to(dev) if "b" in fl else None
        pre64 = x @ (Wh + (Wl if split else 0)).t() + (bias if bias is not None else 0)
        mag = x.abs() @ (Wh + (Wl if split else 0)).abs().t()
        bound = (REF.bound_split if split else REF.bound_plain)(mag, K_) + 2.0 ** -24 * (bias.abs() if bias is not None else 0)
        emu = REF.emulate_nt(x32, Wh, Wl).double() + (bias if bias is not None else 0)
        emu_ratio = float(((emu - pre64).abs() / bound).max())
        assert emu_ratio <= 1.0
    else:
        x, Whs, Wls, f, g = _fwd_operands(c, dev, 1000 + R + 7 * N + 13 * K_ + split)
        Wh, Wl = Whs[0].to(dev), (Wls[0].to(dev) if split else None)
        x, f = x.to(dev), f.to(dev)
        bias = (REF.ints(g, (N,), 1000).to(dev) * f) if "b" in fl else None
        _assert_fwd_exact(x, Wh, Wl, f, bias.abs() if bias is not None else 0)
        pre64, _ = REF.fwd_ref(x, Wh, Wl, bias)
    y64 = REF.act64(pre64, act)
    xin = In(x, torch.float32, dev, ld=ldx, col0=4 if "s" in fl else 0)
    Win, Wlin = In(Wh, BF, dev), (In(Wl, BF, dev) if split else None)
    bin_ = In(bias, torch.float32, dev) if bias is not None else None
    x16_ref = REF.rne_bf16(x.float())
    variants = [("ldc=N", N, 0), ("ldc=N+4", N + 4, 0)] + ([("ldc=N+1", N + 1, 0), ("ldc=N, y + 1 float", N, 1)] if "u" in fl else [])
    notes = []
    for vname, ldc, off in variants:
        tag = f"{c['id']} {vname}"
        y = Out(R, N, dev, ld=ldc, off=off)
        pre = Out(R, N, dev, ld=ldc) if "p" in fl else None
        x16 = Out(R, K_, dev, dtype=BF) if "x" in fl else None
        outs = [o for o in (y, pre, x16) if o is not None]
        args = (xin.ptr, ldx, Win.ptr, _ptr(Wlin), _ptr(bin_), y.ptr, _ptr(pre), _ptr(x16), R, N, K_, ldc, act, K._st())
        K._call("spe_linear_small_fwd", *args)
        first = [o.bits() for o in outs]
        if random:
            ratio = _check_bounded(y, pre64, bound, tag)
            notes = [f"y {ratio:.3f} of the bound (emulation {emu_ratio:.3f})"]
            assert ratio <= 1.0, notes
        elif act == 2:
            ref = REF.gelu64(pre64)
            unit = 2.0 ** -24 * (ref.abs() + pre64.abs()).clamp_min(1e-300)
            cc, f32r = _gelu_c(pre64, lambda v: 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752)), ref, unit)
            ratio = _check_bounded(y, ref, unit, tag)
            notes = [f"gelu kernel {ratio:.3f} fp32 formula {f32r:.3f} c {cc:.3f}"]
            assert ratio <= cc, notes
        else:
            _check_exact(y, y64, tag)
        if pre is not None and not random:
            _check_exact(pre, pre64, tag + " pre")
        if x16 is not None:
            assert torch.equal(x16.inside().float(), x16_ref), f"{tag}: x16_out is not bf16(x) bit for bit"
            assert x16.outside_is_nan(), f"{tag}: x16_out written outside [R, K]"
        K._call("spe_linear_small_fwd", *args)
        assert _same_bits(outs, first), f"{tag}: a second call gave other bits"
    kind = notes[0] if notes else "exact"
    print(f"LINSMALL {c['id']:44s} -> {name:38s} grid {plan['grid_x']:4d}  {kind}  states: {' | '.join(s.split(': ', 1)[1] for s in C.states_of(c))}")


# ---- backward ----------------------------------------------------------------------------------------------------------------------------
def _relu_aux(g, shape):
    """Forward outputs of a ReLU with every kind of value the mask must tell apart: +0, -0, positive, negative."""
    kind = torch.randint(0, 4, shape, generator=g)
    mag = torch.randint(1, 100, shape, generator=g).float() / 8
    aux = torch.where(kind == 2, mag, torch.where(kind == 3, -mag, torch.zeros(shape)))
    aux = torch.where(kind == 1, -torch.zeros(shape), aux)
    assert bool(((aux == 0) & torch.signbit(aux)).any()) and bool(((aux == 0) & ~torch.signbit(aux)).any())
    return aux


def _dgelu_ratios(dy, h, got):
    """Worst |x - dy gelu'(h)| / (2^-24 |dy| (0.5 (1 + |erf|) + |h| pdf)) - the unit is the sum of the formula's terms in magnitude, which covers
    the cancellation in 1 + erf - of the kernel's dy' and of the fp32 formula with torch on the host; -> (kernel, fp32, c)."""
    dy64, h64 = dy.double().cpu(), h.double().cpu()
    ref = dy64 * REF.dgelu64(h64)
    pdf = torch.exp(-0.5 * h64 * h64) / math.sqrt(2.0 * math.pi)
    unit = (2.0 ** -24 * dy64.abs() * (0.5 * (1.0 + torch.erf(h64 / math.sqrt(2.0)).abs()) + h64.abs() * pdf)).clamp_min(1e-300)

    def formula32(v):
        d32 = dy.float().cpu()
        return d32 * (0.5 * (1.0 + torch.erf(v * 0.70710678118654752)) + v * (0.3989422804014327 * torch.exp(-0.5 * v * v)))
    cc, f32r = _gelu_c(h, formula32, ref, unit)
    return float(((got.double().cpu() - ref).abs() / unit).max()), f32r, cc


@pytest.mark.parametrize("c", C.BWD_CASES, ids=lambda c: c["id"])
def test_linear_small_bwd(dev, c):
    """spe_linear_small_bwd: each want set, both instances, the row chunk, clamp and store-guard edges, the activation derivatives: dx, dW and
    db equal to the fp64 reference (GELU derivative and random-normal: inside the bound), nothing written outside, the same bits twice."""
    from spe_amd import kernels as K
    R, N, K_, w, act, fl = c["R"], c["N"], c["K"], c["wants"], c["act"], c["flags"]
    plan = K.linear_small_plan("bwd", R, N, K_, dx="x" in w, dW="w" in w, db="b" in w)
    assert plan["status"] == 0 and (C.kernel_name("bwd", plan) if plan["grid_x"] else None) == C.instance_of(c)
    assert (plan["tiles_dx"], plan["tiles_dw"]) == C.tiles_of(c)[:2]
    g = torch.Generator().manual_seed(2000 + R + 7 * N + 13 * K_ + len(w) + act)
    random, notes, aux = "r" in fl, [], None
    if random:
        dy32, x16, WT = REF.random_operands(c, dev)
        dy = dy32.double()
    else:
        if act == 2:                                    # R = 1, db only: db is dy' itself
            assert w == "b" and R == 1
            dy = (torch.randn((R, N), generator=g) * 2).double().to(dev)
        else:
            dy = (_signed_bits(g, (R, N), 12) if "w" in fl else REF.ints(g, (R, N), 255)).to(dev)
            assert ("w" in fl) == (w == "b") or w == ""
        gk, fk = _scales(g, K_).to(dev), _scales(g, K_).to(dev)
        x16 = REF.ints(g, (R, K_), 4).to(dev) * gk[None, :]
        WT = REF.ints(g, (K_, N), 4).to(dev) * fk[:, None]
    if act == 1:
        aux = _relu_aux(g, (R, N)).to(dev)
    elif act == 2:
        aux = (torch.randn((R, N), generator=g) * 1.5).to(dev)
    r = REF.bwd_ref(dy, None if aux is None else aux.double(), act, x16, WT)
    if not random and act != 2:                         # exact in any order
        assert float(r["mdb"].max()) < TWO24
        assert "x" not in w or float((r["mdx"] / fk[None, :]).max()) < TWO24
        assert "w" not in w or float((r["mdw"] / gk[None, :]).max()) < TWO24
        if w != "b":
            assert torch.equal(REF.rne_bf16(r["dyp"].float()).double(), r["dyp"])      # bf16 holds dy'
        else:
            assert not torch.equal(REF.rne_bf16(r["dyp"].float()).double(), r["dyp"])  # ... and here it does not: db must not go through it
    dyin, auxin = In(dy, torch.float32, dev), (In(aux, torch.float32, dev) if aux is not None else None)
    xin, win = (In(x16, BF, dev) if "w" in w else None), (In(WT, BF, dev) if "x" in w else None)
    dx = Out(R, K_, dev) if "x" in w else None
    dW = Out(N, K_, dev) if "w" in w else None
    db = Out(1, N, dev) if "b" in w else None
    outs = [o for o in (dx, dW, db) if o is not None]
    args = (dyin.ptr, _ptr(auxin), act, _ptr(xin), _ptr(win), _ptr(dx), _ptr(dW), _ptr(db), R, N, K_, K._st())
    K._call("spe_linear_small_bwd", *args)
    first = [o.bits() for o in outs]
    tag = c["id"]
    if random:
        emu_dyp = dy32
        for o, key, mkey, depth, emu in ((dx, "dx", "mdx", N, lambda: REF.emulate_nt(emu_dyp, WT)), (dW, "dW", "mdw", R, lambda: REF.emulate_tn(emu_dyp, x16))):
            if o is not None:
                ref = dy.t() @ x16 if key == "dW" else dy @ WT.t()
                bound = REF.bound_plain(r[mkey], depth)
                er = float(((emu().double() - ref).abs() / bound).max())
                kr = _check_bounded(o, ref, bound, f"{tag} {key}")
                notes.append(f"{key} {kr:.3f} of the bound (emulation {er:.3f})")
                assert er <= 1.0 and kr <= 1.0, notes
        if db is not None:
            bound = REF.bound_db(r["mdb"], R)[None, :]
            er = float(((REF.emulate_db(dy32).double()[None, :] - r["db"][None, :]).abs() / bound).max())
            kr = _check_bounded(db, r["db"][None, :], bound, f"{tag} db")
            notes.append(f"db {kr:.3f} of the bound (emulation {er:.3f})")
            assert er <= 1.0 and kr <= 1.0, notes
    elif act == 2:
        assert bool(torch.isfinite(db.inside()).all()) and db.outside_is_nan()
        kr, f32r, cc = _dgelu_ratios(dy, aux, db.inside())
        notes.append(f"gelu' kernel {kr:.3f} fp32 formula {f32r:.3f} c {cc:.3f}")
        assert kr <= cc, notes
    else:
        if dx is not None:
            _check_exact(dx, r["dx"], tag + " dx")
        if dW is not None:
            _check_exact(dW, r["dW"], tag + " dW")
        if db is not None:
            _check_exact(db, r["db"][None, :], tag + " db")
    K._call("spe_linear_small_bwd", *args)
    assert _same_bits(outs, first), f"{tag}: a second call gave other bits"
    name = C.instance_of(c) or "nothing launched (status 0)"
    print(f"LINSMALL {c['id']:44s} -> {name:38s} grid {plan['grid_x']:4d} = {plan['tiles_dx']} dx + {plan['tiles_dw']} dW/db  "
          f"{'; '.join(notes) if notes else 'exact'}  states: {' | '.join(s.split(': ', 1)[1] for s in C.states_of(c))}")


# ---- group forward -----------------------------------------------------------------------------------------------------------------------
def _table(K, ptrs):
    return K._ptr_array([p or 0 for p in ptrs])


@pytest.mark.parametrize("c", C.GROUP_FWD_CASES, ids=lambda c: c["id"])
def test_linear_small_group_fwd(dev, c):
    """spe_linear_small_group_fwd: every block's y equal to x W_i^T + add_i + bias_i in fp64 with its OWN weights, addend and bias (NULL
    elements and NULL tables included), x16_out bit for bit, nothing written outside, the same bits twice."""
    from spe_amd import kernels as K
    R, nb, N, K_, split, fl = c["R"], c["nblk"], c["N"], c["K"], c["split"], c["flags"]
    ldx = K_ + (12 if "s" in fl else 0)
    plan = K.linear_small_plan("group_fwd", R, N, K_, nblk=nb, ldx=ldx, split=split)
    name = C.kernel_name("group_fwd", plan)
    assert plan["status"] == 0 and name == C.instance_of(c)
    x, Whs, Wls, f, g = _fwd_operands(c, dev, 3000 + R + 7 * N + 13 * K_ + nb, nblk=nb)
    x, f = x.to(dev), f.to(dev)
    has = lambda kind, i: kind == "all" or (kind == "mixed" and not C.mixed_null(i))      # noqa: E731
    biases = [REF.ints(g, (N,), 1000).to(dev) * f if has(c["bias"], i) else None for i in range(nb)]
    adds = [REF.ints(g, (R, N), 1000).to(dev) * f[None, :] if has(c["add"], i) else None for i in range(nb)]
    if c["bias"] == "mixed" or c["add"] == "mixed":
        assert any(v is None for v in (biases if c["bias"] == "mixed" else adds)) and any(v is not None for v in biases + adds)
    Whs = [w.to(dev) for w in Whs]
    Wls = [w.to(dev) for w in Wls] if split else None
    for i in range(nb):
        _assert_fwd_exact(x, Whs[i], Wls[i] if split else None, f, (biases[i].abs() if biases[i] is not None else 0) + (adds[i].abs() if adds[i] is not None else 0))
    refs = REF.group_fwd_ref(x, Whs, Wls, biases, adds)
    xin = In(x, torch.float32, dev, ld=ldx, col0=4 if "s" in fl else 0)
    Win, Wlin = [In(w, BF, dev) for w in Whs], ([In(w, BF, dev) for w in Wls] if split else None)
    bin_ = [None if b is None else In(b, torch.float32, dev) for b in biases]
    ain = [None if a is None else In(a, torch.float32, dev) for a in adds]
    ys = [Out(R, N, dev) for _ in range(nb)]
    x16 = Out(R, K_, dev, dtype=BF) if "x" in fl else None
    args = (xin.ptr, ldx, _table(K, [w.ptr for w in Win]), _table(K, [w.ptr for w in Wlin]) if split else None,
            None if c["bias"] == "none" else _table(K, [_ptr(b) for b in bin_]), None if c["add"] == "none" else _table(K, [_ptr(a) for a in ain]),
            _table(K, [y.ptr for y in ys]), _ptr(x16), R, nb, N, K_, K._st())
    K._call("spe_linear_small_group_fwd", *args)
    outs = ys + ([x16] if x16 is not None else [])
    first = [o.bits() for o in outs]
    for i in range(nb):
        _check_exact(ys[i], refs[i], f"{c['id']} y[{i}]")
    if x16 is not None:
        assert torch.equal(x16.inside().float(), REF.rne_bf16(x.float())) and x16.outside_is_nan()
    K._call("spe_linear_small_group_fwd", *args)
    assert _same_bits(outs, first)
    print(f"LINSMALL {c['id']:58s} -> {name:38s} grid {plan['grid_x']:4d}  exact  states: {' | '.join(s.split(': ', 1)[1] for s in C.states_of(c))}")


# ---- group backward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.GROUP_BWD_CASES, ids=lambda c: c["id"])
def test_linear_small_group_bwd(dev, c):
    """spe_linear_small_group_bwd: dx the sum over the outputs that have a gradient, dW_i / db_i of each from its OWN dy; outputs without a
    gradient leave their dW / db all NaN; with every dy NULL dx comes back all zeros and no dW tile is launched."""
    from spe_amd import kernels as K
    R, nb, N, K_ = c["R"], c["nblk"], c["N"], c["K"]
    anyw = C.any_dw(c)
    plan = K.linear_small_plan("group_bwd", R, N, K_, nblk=nb, dx=c["dx"], any_dw=anyw)
    assert plan["status"] == 0 and (C.kernel_name("group_bwd", plan) if plan["grid_x"] else None) == C.instance_of(c)
    assert (plan["tiles_dx"], plan["tiles_dw"]) == C.tiles_of(c)[:2]
    g = torch.Generator().manual_seed(4000 + R + 7 * N + 13 * K_ + nb)
    dys = [None if C.no_grad(c["dy"], i, nb) else REF.ints(g, (R, N), 255).to(dev) for i in range(nb)]
    gk = _scales(g, K_).to(dev)
    x16 = REF.ints(g, (R, K_), 4).to(dev) * gk[None, :]
    fk = _scales(g, K_).to(dev)
    WTs = [REF.ints(g, (K_, N), 4).to(dev) * fk[:, None] for _ in range(nb)]
    live = [d for d in dys if d is not None]
    if live:
        assert float((sum(d.abs() @ WT.abs().t() for d, WT in zip(dys, WTs) if d is not None) / fk[None, :]).max()) < TWO24
        assert max(float((d.abs().t() @ x16.abs() / gk[None, :]).max()) for d in live) < TWO24 and 255 * R < TWO24
    rdx, rdW, rdb = REF.group_bwd_ref(dys, x16, WTs if c["dx"] else None)
    has = lambda kind, i: kind == "all" or (kind == "mixed" and not C.mixed_null(i))      # noqa: E731
    dyin = [None if d is None else In(d, torch.float32, dev) for d in dys]
    xin, win = In(x16, BF, dev), [In(w, BF, dev) for w in WTs]
    dx = Out(R, K_, dev) if c["dx"] else None
    dWs = [Out(N, K_, dev) if has(c["dW"], i) else None for i in range(nb)]
    dbs = [Out(1, N, dev) if has(c["db"], i) else None for i in range(nb)]
    args = (_table(K, [_ptr(d) for d in dyin]), xin.ptr, _table(K, [w.ptr for w in win]) if c["dx"] else None, _ptr(dx),
            None if c["dW"] == "none" else _table(K, [_ptr(o) for o in dWs]), None if c["db"] == "none" else _table(K, [_ptr(o) for o in dbs]),
            R, nb, N, K_, K._st())
    K._call("spe_linear_small_group_bwd", *args)
    outs = [o for o in [dx] + dWs + dbs if o is not None]
    first = [o.bits() for o in outs]
    tag = c["id"]
    if dx is not None:
        _check_exact(dx, rdx, tag + " dx")
        if not live:
            assert bool((dx.inside() == 0).all()), f"{tag}: dx of a group without any gradient is not all zeros"
    for i in range(nb):
        for o, ref, nm in ((dWs[i], rdW[i], "dW"), (dbs[i], None if rdb[i] is None else rdb[i][None, :], "db")):
            if o is None:
                continue
            if dys[i] is None:
                assert o.all_nan(), f"{tag}: {nm}[{i}] of an output without a gradient was written"
            else:
                _check_exact(o, ref, f"{tag} {nm}[{i}]")
    K._call("spe_linear_small_group_bwd", *args)
    assert _same_bits(outs, first)
    name = C.instance_of(c) or "nothing launched (status 0)"
    print(f"LINSMALL {c['id']:58s} -> {name:38s} grid {plan['grid_x']:4d} = {plan['tiles_dx']} dx + {plan['tiles_dw']} dW/db  exact  "
          f"states: {' | '.join(s.split(': ', 1)[1] for s in C.states_of(c))}")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _refusal_kit(dev, K, name, base, outs):
    from spe_amd.lib import SpeLibraryError

    def call(**kw):
        a = dict(base, **kw)
        K._call(name, *[a[k] for k in base], K._st())

    def refused(**kw):
        with pytest.raises(SpeLibraryError, match="status -2$"):
            call(**kw)
        assert all(o.all_nan() for o in outs), (name, kw)

    def nothing(**kw):
        call(**kw)
        assert all(o.all_nan() for o in outs), (name, kw)
    return refused, nothing


def test_linear_small_fwd_refusals(dev):
    """Every -2 of spe_linear_small_fwd as the code checks it (K only - N, ldc, y, pre and bias are free), R or N <= 0: status 0; the
    NaN-filled outputs untouched after each."""
    from spe_amd import kernels as K
    R, N, K_ = 33, 40, 24
    x, W, Wl = In(torch.ones(R, K_), torch.float32, dev, ld=K_ + 12, col0=4), In(torch.ones(N, K_), BF, dev), In(torch.ones(N, K_), BF, dev)
    b = In(torch.ones(N), torch.float32, dev)
    y, pre, x16 = Out(R, N, dev), Out(R, N, dev), Out(R, K_, dev, dtype=BF)
    base = dict(x=x.ptr, ldx=x.ld, W=W.ptr, Wl=Wl.ptr, b=b.ptr, y=y.ptr, pre=pre.ptr, x16=x16.ptr, R=R, N=N, K=K_, ldc=N, act=0)
    refused, nothing = _refusal_kit(dev, K, "spe_linear_small_fwd", base, [y, pre, x16])
    for K_bad in (0, -8, 4, 20, 25):
        refused(K=K_bad)
    for ldx in (K_ + 1, K_ + 2, K_ + 3):
        refused(ldx=ldx)
    for which in ("x", "W", "Wl", "x16"):
        for off in ((2, 4) if which != "x" else (4, 8)):         # 2 or 4 bytes (fp32 x: 4 or 8) off a 16-byte boundary
            refused(**{which: base[which] + off})
    for kw in (dict(R=0), dict(R=-1), dict(N=0), dict(N=-8), dict(R=0, K=4), dict(N=0, ldx=K_ + 1)):
        nothing(**kw)


def test_linear_small_bwd_refusals(dev):
    from spe_amd import kernels as K
    R, N, K_ = 33, 40, 24
    dy, aux = In(torch.ones(R, N), torch.float32, dev), In(torch.ones(R, N), torch.float32, dev)
    x16, WT = In(torch.ones(R, K_), BF, dev), In(torch.ones(K_, N), BF, dev)
    dx, dW, db = Out(R, K_, dev), Out(N, K_, dev), Out(1, N, dev)
    base = dict(dy=dy.ptr, aux=None, act=0, x16=x16.ptr, WT=WT.ptr, dx=dx.ptr, dW=dW.ptr, db=db.ptr, R=R, N=N, K=K_)
    refused, nothing = _refusal_kit(dev, K, "spe_linear_small_bwd", base, [dx, dW, db])
    for K_bad in (4, 20, 25):
        refused(K=K_bad)
    for N_bad in (4, 36, 41):
        refused(N=N_bad)
    for which in ("dy", "x16", "WT", "dx", "dW"):
        for off in ((4, 8) if which in ("dy", "dx", "dW") else (2, 4)):
            refused(**{which: base[which] + off})
    refused(aux=aux.ptr + 4, act=1); refused(aux=aux.ptr + 8, act=2)
    refused(WT=None)                                             # dx without WT16
    refused(x16=None)                                            # dW without x16
    refused(aux=aux.ptr, act=0); refused(aux=aux.ptr, act=3)     # aux with an act that has no derivative
    for kw in (dict(R=0), dict(N=0), dict(K=0), dict(R=-1), dict(K=-8), dict(R=0, N=4), dict(dx=None, dW=None, db=None)):
        nothing(**kw)


def test_linear_small_group_fwd_refusals(dev):
    from spe_amd import kernels as K
    R, nb, N, K_ = 33, 3, 32, 24
    x = In(torch.ones(R, K_), torch.float32, dev, ld=K_ + 12, col0=4)
    Ws, Wls = [In(torch.ones(N, K_), BF, dev) for _ in range(17)], [In(torch.ones(N, K_), BF, dev) for _ in range(17)]
    bs, adds = [In(torch.ones(N), torch.float32, dev) for _ in range(17)], [In(torch.ones(R, N), torch.float32, dev) for _ in range(17)]
    ys, x16 = [Out(R, N, dev) for _ in range(17)], Out(R, K_, dev, dtype=BF)
    tab = lambda objs, patch=None: _table(K, [(patch or {}).get(i, o.ptr) for i, o in enumerate(objs)])      # noqa: E731
    base = dict(x=x.ptr, ldx=x.ld, W=tab(Ws), Wl=tab(Wls), b=tab(bs), add=tab(adds), y=tab(ys), x16=x16.ptr, R=R, nblk=nb, N=N, K=K_)
    refused, nothing = _refusal_kit(dev, K, "spe_linear_small_group_fwd", base, ys + [x16])
    for K_bad in (0, 4, 20):
        refused(K=K_bad)
    for N_bad in (8, 24, 40):
        refused(N=N_bad)
    for ldx in (K_ + 1, K_ + 2):
        refused(ldx=ldx)
    refused(nblk=17)
    for off in (4, 8):
        refused(x=x.ptr + off)
    for off in (2, 4):
        refused(x16=x16.ptr + off)
        refused(W=tab(Ws, {1: Ws[1].ptr + off})); refused(Wl=tab(Wls, {2: Wls[2].ptr + off}))
    for off in (4, 8):
        refused(y=tab(ys, {0: ys[0].ptr + off})); refused(add=tab(adds, {1: adds[1].ptr + off}))
    refused(W=tab(Ws, {1: 0})); refused(y=tab(ys, {2: 0})); refused(Wl=tab(Wls, {0: 0}))        # NULL elements the header forbids
    for kw in (dict(R=0), dict(N=0), dict(nblk=0), dict(nblk=-1), dict(R=0, nblk=17), dict(N=0, K=4)):
        nothing(**kw)


def test_linear_small_group_bwd_refusals(dev):
    from spe_amd import kernels as K
    R, nb, N, K_ = 33, 3, 128, 24
    dys = [In(torch.ones(R, N), torch.float32, dev) for _ in range(17)]
    x16, WTs = In(torch.ones(R, K_), BF, dev), [In(torch.ones(K_, N), BF, dev) for _ in range(17)]
    dx, dWs, dbs = Out(R, K_, dev), [Out(N, K_, dev) for _ in range(17)], [Out(1, N, dev) for _ in range(17)]
    tab = lambda objs, patch=None: _table(K, [(patch or {}).get(i, o.ptr) for i, o in enumerate(objs)])      # noqa: E731
    base = dict(dy=tab(dys), x16=x16.ptr, WT=tab(WTs), dx=dx.ptr, dW=tab(dWs), db=tab(dbs), R=R, nblk=nb, N=N, K=K_)
    refused, nothing = _refusal_kit(dev, K, "spe_linear_small_group_bwd", base, [dx] + dWs + dbs)
    for K_bad in (4, 20):
        refused(K=K_bad)
    for N_bad in (32, 64, 96, 192):
        refused(N=N_bad)
    refused(nblk=17)
    for off in (2, 4):
        refused(x16=x16.ptr + off); refused(WT=tab(WTs, {1: WTs[1].ptr + off}))
    for off in (4, 8):
        refused(dx=dx.ptr + off); refused(dy=tab(dys, {2: dys[2].ptr + off})); refused(dW=tab(dWs, {0: dWs[0].ptr + off}))
    refused(WT=None)                                             # dx without WT16 ...
    refused(WT=tab(WTs, {1: 0}))                                 # ... or with a NULL element
    refused(x16=None)                                            # dW without x16
    for kw in (dict(R=0), dict(N=0), dict(K=0), dict(nblk=0), dict(R=0, nblk=17), dict(K=0, N=32),
               dict(dx=None, dW=None, db=None), dict(dx=None, dy=_table(K, [0, 0, 0]))):
        nothing(**kw)


# ---- the production wrappers, once each ---------------------------------------------------------------------------------------------------
def test_linear_small_wrappers_exact(dev):
    """kernels.linear_fwd / linear_bwd / linear_group_fwd / linear_group_bwd as the product calls them (cached bf16 weight parts of an fp32
    weight, the x16 side output handed from the forward to the backward, NULL entries for outputs without a gradient): exact."""
    from spe_amd import kernels as K
    g = torch.Generator().manual_seed(77)
    R, N, K_ = 200, 40, 24
    prev = K.get_precision()
    K.set_precision("bf16s")
    try:
        f = torch.ones(N).double()                   # the backward's dx contracts over n: the weight rows carry no scale here
        x = _signed_bits(g, (R, K_), 10).to(dev)                                     # 2^10 x 2^9 x K < 2^24
        W = (_signed_bits(g, (N, K_), 9) * f[:, None]).to(dev)                       # an fp32 weight: the cache splits it into (hi, lo)
        b = (REF.ints(g, (N,), 1000) * f).to(dev)
        assert K._lin_small_ok(R, N, K_)
        Wh, Wl = REF.hilo(W)
        assert torch.equal(Wh + Wl, W) and bool(Wl.any())
        _assert_fwd_exact(x, Wh, Wl, f.to(dev), b.abs())
        pre64, _ = REF.fwd_ref(x, Wh, Wl, b)
        Wp = W.float().contiguous()
        y, pre, x16 = K.linear_fwd(x.float().contiguous(), Wp, b.float(), act=1, want_pre=True)
        assert torch.equal(pre.double(), pre64) and torch.equal(y.double(), pre64.clamp_min(0)) and x16.dtype == BF
        assert torch.equal(x16.float(), REF.rne_bf16(x.float()))
        dy = REF.ints(g, (R, N), 15).to(dev)
        r = REF.bwd_ref(dy, y.double(), 1, x16.double(), Wh.t().contiguous())
        assert float(r["mdx"].max()) < TWO24 and float(r["mdw"].max()) < TWO24
        dx, dW, db = K.linear_bwd(dy.float().contiguous(), x16, Wp, act=1, act_aux=y)
        assert torch.equal(dx.double(), r["dx"]) and torch.equal(dW.double(), r["dW"]) and torch.equal(db.double(), r["db"])
        # groups: two Linears of 128 columns on one input, the second without a gradient
        Ng = 128
        fg = torch.ones(Ng).double()
        Ws = [(_signed_bits(g, (Ng, K_), 9) * fg[:, None]).to(dev).float().contiguous() for _ in range(2)]
        bs = [(REF.ints(g, (Ng,), 1000) * fg).to(dev).float() for _ in range(2)]
        add0 = (REF.ints(g, (R, Ng), 1000) * fg[None, :]).to(dev).float().contiguous()
        assert K.linear_group_ok(R, Ws, bs)
        ys, x16g = K.linear_group_fwd(x.float().contiguous(), Ws, bs, adds=[add0, None])
        for i in range(2):
            h, lo = REF.hilo(Ws[i].double())
            _assert_fwd_exact(x, h, lo, fg.to(dev), bs[i].double().abs() + (add0.double().abs() if i == 0 else 0))
            ref, _ = REF.fwd_ref(x, h, lo, bs[i].double(), add0.double() if i == 0 else None)
            assert torch.equal(ys[i].double(), ref), i
        assert torch.equal(x16g.float(), REF.rne_bf16(x.float()))
        dyg = REF.ints(g, (R, Ng), 15).to(dev)
        gdx, gdW, gdb = K.linear_group_bwd([dyg.float().contiguous(), None], x16g, Ws, True, [None, None], [None, None])
        rdx, rdW, rdb = REF.group_bwd_ref([dyg, None], x16g.double(), [REF.hilo(w.double())[0].t().contiguous() for w in Ws])
        assert gdW[1] is None and gdb[1] is None and 15 * 512 * 2 * Ng < TWO24 and 15 * 1024 * R < TWO24
        assert torch.equal(gdW[0].double(), rdW[0]) and torch.equal(gdb[0].double(), rdb[0]) and torch.equal(gdx.double(), rdx)
    finally:
        K.set_precision(prev)
    print("LINSMALL wrappers: linear_fwd / linear_bwd (R=200 N=40 K=24, ReLU, bf16s) and linear_group_fwd / linear_group_bwd (2 x 128 columns, "
          "one addend, one output without a gradient)  exact")
