"""The fp32-operand strided GEMM (spe_gemm_f32 / spe_gemm_ex, csrc/gemm.hip: spe_gemm_kernel<T, TA, TB, SPLIT>) against an fp64 product,
EXACTLY, on all 12 instances at every loader, contraction, store, batch, split and tile-order state (cases: tests/f32_gemm_cases.py, whose
coverage tests/test_f32_gemm_plan_cpu.py proves without a device).  The method is that of tests/test_tn_gemm_gpu.py.

Operands.  Integers times powers of two: row m of op(A) is scaled by 2^e[m], column n of op(B) by 2^f[n], e and f random in [-12, 12] per
batch.  One operand is wide, the other holds integers in [-4, 4]; the roles swap in every second case.  Both are random and asymmetric: a
transposed, shifted or mis-tiled read cannot reproduce the sums.
  plain instances (operands rounded to bf16 while staged): wide integers in [-255, 255], which bf16 holds exactly.  The "ties" cases use
    16-bit integers, a quarter of them exact ties between two bf16 values (odd multiples of 2^7 in [2^15, 2^16), of 2^6 and 2^5 in the two
    binades below); every plain reference takes the operands as x.to(bfloat16).double(), so those cases pin round-to-nearest-even.
  SPLIT instances (hi = bf16(x), lo = bf16(x - hi), product hi hi + hi lo + lo hi): wide integers of 16 bits for K <= 64, 12 bits for
    K <= 1024, 10 bits beyond.  hi + lo reproduces a 16-bit integer exactly (|lo| <= 128) and the narrow operand has no low part, so the
    three-term product IS the fp64 product of the fp32 operands: a missing or mis-paired cross term fails.  The "both10" cases have both
    operands 10-bit and K <= 15; their reference is Ah Bh + Ah Bl + Al Bh in fp64 - the three-term contract itself (Al Bl is not computed).
Every test first asserts in fp64 that (|A| |B|).max() / 2^(e[m] + f[n]) < 2^24.  All partial sums are then integers below 2^24 times the
scale, so fp32 accumulation is exact IN ANY ORDER.  That is also why the atomic split-K path can be compared bit for bit here: the order in
which the splits' atomic adds arrive does not change an exact sum (there the bound includes what C held: (2 |C0| + |A| |B|) / scale).

Reference.  r = float32(float32(alpha) * product) (the fp64 product is exact, so this is one rounding); with a bias, pre = float32(r + bias),
one more fp32 rounding - emulated step by step.  C2 equals pre; C equals pre under act 0 and max(pre, 0) under ReLU.  "Equal" is
torch.equal: every value identical, no NaN; the sign of a zero is not compared.  alpha = 0.7 unsplit, 0.5 split (slab sums and atomic sums
stay exact).  Slab launches assert the SUM of the slabs.  Atomic launches find exact integers of the same scale in C and must return
their sum with the product.
GELU (act 2).  With C2 proven exact, C is compared with the fp64 GELU of C2 element by element under c * 2^-24 * (|ref| + |pre|) (the second
term covers the cancellation in 1 + erf).  c is not fixed in advance: the fp32 formula 0.5 x (1 + erf(x / sqrt 2)) evaluated with torch on
the CPU over the same pre-activations is measured against fp64 in the same unit, and c is 4 times that worst ratio (spe_erff documents about
1 ulp plus 2 ulp of its __expf term, libm less than 1).  These cases are scaled so that at least a quarter of the pre-activations lie in
|x| < 3 (asserted).
Random operands.  One random-normal case per instance with the element-wise bound 2^-8 |A| |B| (plain) and (3 * 2^-18 + (K / 32 + 3) *
2^-24) |A| |B| (SPLIT); a torch emulation of the staging roundings must stay inside the bound before the kernel is asked to.

Memory.  Every operand is a strided block inside a larger buffer filled with NaN - the in-row padding up to the next multiple of 4, which the
vector loaders read by design and must mask, the gaps between batches and 8 elements in front and behind included: a finite result proves
that nothing outside the blocks entered a product.  Where the vector flag is set the rows are 16-byte aligned and padded as the kernel's
contract demands.  C and C2 are NaN-filled with canary rows and floats around them: everything outside [M, N] of every batch and slab must
still be NaN afterwards.  A second call (atomics: from the same initial contents) gives the same bits.
Measured: profiles/f32_gemm_edges.txt (every line this module prints with the prefix F32GEMM)."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f32_gemm_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
BF = torch.bfloat16


def _wide_bits(c):
    if c["prec"] == 0:
        return 16 if c["ops"] == "ties" else 8
    if c["ops"] == "both10":
        return 10
    return 16 if c["K"] <= 64 else 12 if c["K"] <= 1024 else 10


def _ints(g, shape, bits, ties=False):
    hi = 2 ** bits - 1
    v = torch.randint(-hi, hi + 1, shape, generator=g).double()
    if ties:                                    # a quarter: (2 j + 1) * 2^(p - 8), j in [128, 256): midway between two bf16 values of binade p
        p = torch.randint(13, 16, shape, generator=g).double()
        j = torch.randint(128, 256, shape, generator=g).double()
        sgn = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
        t = sgn * (2 * j + 1) * 2.0 ** (p - 8)
        v = torch.where(torch.rand(shape, generator=g) < 0.25, t, v)
    return v


def _operands(c, seed):
    """-> logical fp64 operands A [b0, b1, M, K], B [b0, b1, K, N] as stored (fp32 / bf16 exact) and scale [b0, b1, M, N] (None: random)."""
    g = torch.Generator().manual_seed(seed)
    b0, b1, M, N, K_ = c["b0"], c["b1"], c["M"], c["N"], c["K"]
    if c["ops"] == "random":
        return torch.randn(b0, b1, M, K_, generator=g).double(), torch.randn(b0, b1, K_, N, generator=g).double(), None
    bits = _wide_bits(c)
    a_wide = not c["swap"]
    if c["ops"] == "both10":
        abits = bbits = 10
    else:
        abits, bbits = (bits, None) if a_wide else (None, bits)
    if c["a16"] and abits is not None:
        abits = 8                               # a bf16-stored A holds 8 significant bits
    Ai = _ints(g, (b0, b1, M, K_), abits, c["ops"] == "ties") if abits else torch.randint(-4, 5, (b0, b1, M, K_), generator=g).double()
    Bi = _ints(g, (b0, b1, K_, N), bbits, c["ops"] == "ties") if bbits else torch.randint(-4, 5, (b0, b1, K_, N), generator=g).double()
    if c["epi"] == "gelu":                      # pre-activations of order 1: the product's typical size, a power of two, divided out
        typ = 0.7 * math.sqrt(K_) * (2.0 ** (abits or bbits)) / math.sqrt(3) * 2.6
        sh = -round(math.log2(typ))
        e = sh + torch.randint(-1, 2, (b0, b1, M, 1), generator=g).double()
        f = torch.randint(-1, 2, (b0, b1, 1, N), generator=g).double()
    else:
        e = torch.randint(-12, 13, (b0, b1, M, 1), generator=g).double()
        f = torch.randint(-12, 13, (b0, b1, 1, N), generator=g).double()
    return Ai * 2.0 ** e, Bi * 2.0 ** f, 2.0 ** (e + f)


def _place(x, L, dtype, dev):
    """The [b0, b1, R, C] tensor x as a strided block of a NaN-filled flat buffer -> (flat, address of the block)."""
    flat = torch.full((L["numel"],), NAN, device=dev, dtype=dtype)
    assert flat.data_ptr() % 16 == 0
    b0, b1 = x.shape[:2]
    view = flat.as_strided((b0, b1, L["R"], L["C"]), (L["s0"], L["s1"], L["ld"], 1), L["off"])
    view.copy_(x.to(dev))
    assert torch.equal(view.double(), x.to(dev)), "the operand is not exact in its storage type"
    assert int(torch.isnan(flat).sum()) == flat.numel() - x.numel()
    return flat, flat.data_ptr() + L["off"] * flat.element_size()


def _hilo(x):
    hi = x.float().to(BF).double()
    return hi, (x - hi).float().to(BF).double()


def _product(c, A, B):
    """The fp64 product the instance must deliver before alpha, and |A| |B| as the instance sees the operands."""
    if c["prec"] == 0:
        Ar, Br = A.float().to(BF).double(), B.float().to(BF).double()
        return Ar @ Br, Ar.abs() @ Br.abs()
    Ah, Al = _hilo(A)
    Bh, Bl = _hilo(B)
    if c["ops"] == "random":
        pass
    elif c["ops"] != "both10":                  # hi + lo is the operand itself, and one of them has no low part
        assert torch.equal(Ah + Al, A) and torch.equal(Bh + Bl, B) and (not bool(Al.any()) or not bool(Bl.any()))
    else:
        assert bool(Al.any()) and bool(Bl.any())
    return Ah @ Bh + Ah @ Bl + Al @ Bh, A.abs() @ B.abs()


def _launch(K, c, L, flatA, flatB, flatC, flatC2, bias, alpha, act):
    ta, tb = C.LAYOUTS[c["layout"]]
    pa = flatA.data_ptr() + L["a"]["off"] * flatA.element_size()
    pb = flatB.data_ptr() + 4 * L["b"]["off"]
    pc = flatC.data_ptr() + 4 * L["c"]["off"]
    pc2 = None if flatC2 is None else flatC2.data_ptr() + 4 * L["c"]["off2"]
    pbias = None if bias is None else bias.data_ptr()
    assert pc % 16 == 4 * (L["c"]["off"] % 4) and (pc2 is None or pc2 % 16 == 4 * (L["c"]["off2"] % 4))
    args = (c["M"], c["N"], c["K"], L["a"]["ld"], L["b"]["ld"], L["c"]["ld"], ta, tb, c["b0"], c["b1"],
            L["a"]["s0"], L["a"]["s1"], L["b"]["s0"], L["b"]["s1"], L["c"]["s0"], L["c"]["s1"], float(alpha), act, c["splitk"], c["prec"], K._st())
    if c["a16"]:
        K._call("spe_gemm_ex", pa, 1, pb, pc, pbias, pc2, *args)
    else:
        K._call("spe_gemm_f32", pa, pb, pc, pbias, pc2, *args)


def _gelu_ratios(pre, got):
    """Worst |x - gelu64(pre)| / (2^-24 (|gelu64| + |pre|)) for the kernel's C and for the fp32 formula in torch on the CPU."""
    x = pre.double().cpu()
    ref = 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    unit = (2.0 ** -24 * (ref.abs() + x.abs())).clamp_min(1e-300)
    x32 = pre.float().cpu()
    f32 = 0.5 * x32 * (1.0 + torch.erf(x32 * 0.70710678118654752))
    return float(((got.double().cpu() - ref).abs() / unit).max()), float(((f32.double() - ref).abs() / unit).max())


@pytest.mark.parametrize("idx", range(len(C.GPU_CASES)), ids=lambda i: C.GPU_CASES[i]["id"])
def test_f32_gemm_every_state(dev, idx):
    """One case of tests/f32_gemm_cases.py on the instance the launcher's own plan names: strided operands inside NaN, the result equal to
    the fp64 reference (GELU and random-normal cases: inside their element-wise bound), nothing stored outside [M, N] of any batch or
    slab, the same bits from a second call."""
    from spe_amd import kernels as K
    c = C.GPU_CASES[idx]
    L = C.layout(c)
    plan = K.gemm_plan(**C.plan_args(c))
    name = C.kernel_name(plan)
    assert name in C.INSTANCES and plan["T"] == c["T"]
    ta, tb = C.LAYOUTS[c["layout"]]
    b0, b1, M, N, K_ = c["b0"], c["b1"], c["M"], c["N"], c["K"]
    A, B, scale = _operands(c, 7919 * idx + 13)
    A, B = A.to(dev), B.to(dev)
    flatA, pa = _place(A.transpose(2, 3) if ta else A, L["a"], BF if c["a16"] else torch.float32, dev)
    flatB, pb = _place(B.transpose(2, 3) if tb else B, L["b"], torch.float32, dev)
    assert (pa % 16, pb % 16) == (C.plan_args(c)["a_mod16"], C.plan_args(c)["b_mod16"])
    split = c["splitk"] != 1
    alpha = 0.5 if split else 0.7
    a32 = float(torch.tensor(alpha, dtype=torch.float32))
    random = c["ops"] == "random"
    prod, absprod = _product(c, A, B)
    if not random:
        scale = scale.to(dev)
        assert float((absprod / scale).max()) < 2.0 ** 24      # fp32 accumulation is exact in any order
    r = (a32 * prod).float()

    # ---- the output buffers: NaN everywhere; the atomic path finds exact integers of the same scale inside [M, N]
    nslab = -c["splitk"] if c["splitk"] < 0 else 1
    atomic = c["splitk"] > 1
    LC = L["c"]
    extent = (b0 - 1) * LC["s0"] + (b1 - 1) * LC["s1"] + M * LC["ld"]
    numel = C.GUARD + 1 + (nslab - 1) * plan["slab"] + extent + 2 * LC["ld"] + C.GUARD
    flatC = torch.full((numel,), NAN, device=dev)
    assert flatC.data_ptr() % 16 == 0
    shape, strides = (nslab, b0, b1, M, N), (plan["slab"], LC["s0"], LC["s1"], LC["ld"], 1)
    inside = torch.zeros(numel, dtype=torch.bool, device=dev)
    inside.as_strided(shape, strides, LC["off"]).fill_(True)
    assert int(inside.sum()) == nslab * b0 * b1 * M * N          # the blocks of the batches and slabs do not overlap
    Cview = flatC.as_strided(shape, strides, LC["off"])
    if atomic:
        g = torch.Generator().manual_seed(idx)
        C0 = (torch.randint(-1000, 1001, (b0, b1, M, N), generator=g).double().to(dev) * scale).float()
        assert float(((2 * C0.double().abs() + absprod) / scale).max()) < 2.0 ** 24
        Cview[0].copy_(C0)
    has_epi = c["epi"] != "none"
    flatC2 = bias = None
    act = {"none": 0, "bias": 0, "relu": 1, "gelu": 2}[c["epi"]]
    pre = r
    if has_epi:
        flatC2 = torch.full((numel,), NAN, device=dev)
        g = torch.Generator().manual_seed(idx + 1)
        mag = 0.5 if c["epi"] == "gelu" else float(r.abs().median())
        bias = (torch.randn(N, generator=g) * mag).to(dev)
        pre = (r.double() + bias.double()).float()               # one more fp32 rounding
    init = flatC.clone()

    _launch(K, c, L, flatA, flatB, flatC, flatC2, bias, alpha, act)
    first = flatC.clone()
    got = Cview
    tag = c["id"]
    assert bool(torch.isfinite(got).all()), f"{tag}: NaN or inf inside [M, N] - something outside the operand blocks entered the product"
    assert bool(torch.isnan(flatC[~inside]).all()), f"{tag}: a store to C left [M, N] of its batch or slab"
    worst = None
    if has_epi:
        inside2 = torch.zeros(numel, dtype=torch.bool, device=dev)
        inside2.as_strided(shape, strides, LC["off2"]).fill_(True)
        got2 = flatC2.as_strided(shape, strides, LC["off2"])[0]
        assert bool(torch.isnan(flatC2[~inside2]).all()), f"{tag}: a store to C2 left [M, N] of its batch"
        assert torch.equal(got2, pre), f"{tag}: C2: {int((got2 != pre).sum())} of {pre.numel()} elements differ from the reference"
    if random:
        exact = a32 * (A @ B)                                    # the fp64 product of the fp32 operands
        unit = (2.0 ** -8 if c["prec"] == 0 else 3 * 2.0 ** -18 + (K_ / 32 + 3) * 2.0 ** -24) * a32 * (A.abs() @ B.abs())
        emu = float(((a32 * prod - exact).abs() / unit).max())   # correct arithmetic with the staging roundings
        assert emu < 1.0, f"{tag}: the bound does not hold for correct arithmetic ({emu:.3f})"
        worst = float(((got[0].double() - exact).abs() / unit).max())
        print(f"F32GEMM {tag}: emulation {emu:.3f} of the bound, kernel {worst:.3f}")
        assert worst < 1.0, f"{tag}: {worst:.3f} of the element-wise bound"
    elif atomic:
        want = (C0.double() + r.double()).float()
        assert torch.equal(got[0], want), f"{tag}: {int((got[0] != want).sum())} of {want.numel()} elements differ from C0 + product"
    elif nslab > 1:
        total = got.double().sum(0).float()
        assert torch.equal(total, r), f"{tag}: {int((total != r).sum())} of {r.numel()} elements of the slab sum differ from the fp64 product"
    elif c["epi"] == "gelu":
        assert float((pre.abs() < 3).float().mean()) >= 0.25, f"{tag}: fewer than a quarter of the pre-activations in |x| < 3"
        worst, cpu = _gelu_ratios(pre, got[0])
        print(f"F32GEMM {tag}: GELU worst error / (2^-24 (|ref| + |pre|)): fp32 formula on the CPU {cpu:.3f}, kernel {worst:.3f}, c = {4 * cpu:.3f}")
        assert worst <= 4 * cpu, f"{tag}: GELU {worst:.3f} units, allowed {4 * cpu:.3f}"
    else:
        want = pre.clamp_min(0) if act == 1 else pre
        assert torch.equal(got[0], want), f"{tag}: {int((got[0] != want).sum())} of {want.numel()} elements differ from the fp64 product, " \
            f"max |diff| / |ref| {float(((got[0].double() - want.double()).abs() / want.double().abs().clamp_min(1e-30)).max()):.3e}"
    # a second call, from the same contents, gives the same bits
    first2 = flatC2.clone() if has_epi else None
    flatC.copy_(init)
    _launch(K, c, L, flatA, flatB, flatC, flatC2, bias, alpha, act)
    assert torch.equal(flatC.view(torch.int32), first.view(torch.int32)), f"{tag}: a second call gave other bits"
    if has_epi:
        assert torch.equal(flatC2.view(torch.int32), first2.view(torch.int32)), f"{tag}: a second call gave other bits in C2"
    st = sorted(C.states(c, plan))
    kind = "bounded" if random or c["epi"] == "gelu" else "exact"
    print(f"F32GEMM {tag:28s} -> {name}  k-tiles per split {C.kt_per_split(c, plan)[:6]}{'...' if plan['splitk'] > 6 else ''}  "
          f"grid.x {plan['grid_x']}  {kind}{'' if worst is None else f' {worst:.3f}'}  states: {' '.join(st)}")


def test_f32_gemm_refusals(dev):
    """-2, -3, -4, -5 and the M <= 0 / N <= 0 / empty-batch no-op from spe_gemm_f32 itself, with valid pointers: the status, and a
    NaN-filled C that nobody touched."""
    from spe_amd import kernels as K
    from spe_amd.lib import SpeLibraryError
    M, N, K_ = 66, 70, 160
    A = torch.ones(M * K_ + 64, device=dev)
    B = torch.ones(N * K_ + 64, device=dev)
    bias = torch.ones(N, device=dev)
    Cb = torch.full((8 * M * N,), NAN, device=dev)
    C2 = torch.full((M * N,), NAN, device=dev)

    def call(M=M, N=N, K_=K_, ta=0, tb=1, b0=1, b1=1, bias=None, C2=None, act=0, splitk=1):
        K._call("spe_gemm_f32", A.data_ptr(), B.data_ptr(), Cb.data_ptr(), None if bias is None else bias.data_ptr(),
                None if C2 is None else C2.data_ptr(), M, N, K_, K_ if not ta else M, K_ if tb else N, N, ta, tb, b0, b1, 0, 0, 0, 0, 0, 0,
                1.0, act, splitk, 0, K._st())

    def refused(status, **kw):
        assert K.gemm_plan(kw.get("M", M), kw.get("N", N), kw.get("K_", K_), K_, K_, N, kw.get("ta", 0), kw.get("tb", 1), splitk=kw.get("splitk", 1),
                           epilogue=any(kw.get(k) is not None for k in ("bias", "C2")) or kw.get("act", 0) != 0) is None
        with pytest.raises(SpeLibraryError, match=f"status {status}$"):
            call(**kw)
        assert bool(torch.isnan(Cb).all()) and bool(torch.isnan(C2).all())

    refused(-2, ta=1, tb=1)
    refused(-3, splitk=2, bias=bias); refused(-3, splitk=-2, C2=C2); refused(-3, splitk=5, act=1); refused(-3, splitk=2, act=2)
    refused(-4, K_=0); refused(-4, K_=-3)
    refused(-5, splitk=-6); refused(-5, K_=1, splitk=-2)
    for kw in (dict(M=0), dict(N=0), dict(M=-1), dict(b0=0), dict(b1=0), dict(M=0, K_=0)):      # nothing to do
        call(**kw)
        assert bool(torch.isnan(Cb).all())
    call(splitk=-5)                                                          # the last slab count that is taken: 5 k-tiles
    assert bool(torch.isfinite(Cb[:5 * M * N]).all()) and bool(torch.isnan(Cb[5 * M * N:]).all())
    print("F32GEMM refusals: -2 (both transposes) -3 (split with bias / C2 / act) -4 (K <= 0) -5 (more slabs than k-tiles) 0 (empty): C untouched")
