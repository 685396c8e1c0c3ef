"""The weight-gradient TN GEMM (spe_gemm_bf16tn, csrc/gemm_bf16tn.hip) and its production wrapper kernels._dw16_tn against an fp64
product, EXACTLY, at every launch site, pipeline state, stride and store path (shapes: tests/tn_gemm_cases.py, whose coverage
tests/test_tn_gemm_plan_cpu.py proves without a device).

Operands.  One operand holds integers in [-255, 255] (all 8 significand bits of bf16), the other integers in [-4, 4]; the roles swap in
every second case.  Column m of A is scaled by 2^e[m] and column n of B by 2^f[n], e and f in [-12, 12].  Every partial sum of C[m, n] is
then an integer below 255 * 4 * R times 2^(e[m] + f[n]): below 2^24 for R <= 16448, so fp32 accumulation is exact IN ANY ORDER, and so is
the sum of the slabs of a split.  Each test asserts that bound, (|A|^T |B|).max() < 2^24 times the scale in fp64, before it trusts
equality.  Both operands are random and asymmetric: a transposed, shifted or mis-tiled read cannot reproduce the sums.

Reference.  (float32(alpha) as a double * (A.double().T @ B.double())).float(): the fp64 product is exact, the one fp32 rounding of
acc * alpha is the only rounding anywhere.  Unsplit cases use alpha = 0.7, split cases alpha = 0.5 (so the slab sum stays exact) and assert
the SUM of the slabs: how the rows are divided among them is not part of the contract of include/spe_hip.h.  "Equal" is torch.equal on
fp32 - every value identical, no NaN; only the sign of a zero is not compared (a contraction of one row leaves -0 in the fp64 product
where an accumulator that starts at +0 holds +0).

Buffers.  A is a column block (from column 8) of an [R + 3, M + 16] bf16 buffer, B (from column 16) of an [R + 3, N + 24] one, everything
around the blocks NaN, the 3 rows beyond R included: a finite result proves that nothing outside the blocks entered the product.  C is
[M + 2, ldc] pre-filled with NaN (slabs: |splitk| x [M, ldc] and 2 more rows): everything outside [M, N] must still be NaN afterwards.
ldc = N and N + 4 take the vector stores; ldc = N + 1, and ldc = N with C one float behind a 16-byte boundary, the scalar ones.
Measured: profiles/tn_gemm_edges.txt (every line this module prints with the prefix TNGEMM)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tn_gemm_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _exact_operands(R, M, N, seed, swap, dev, lda=None, a_col=8, ldb=None, b_col=16):
    """-> (A view [R + 3, lda - a_col] whose [:R, :M] is the operand, B view likewise, A block as fp64, B block as fp64)."""
    g = torch.Generator().manual_seed(seed)
    wide, narrow = (255, 4) if not swap else (4, 255)
    Ai = torch.randint(-wide, wide + 1, (R, M), generator=g).double()
    Bi = torch.randint(-narrow, narrow + 1, (R, N), generator=g).double()
    e = torch.randint(-12, 13, (M,), generator=g).double()
    f = torch.randint(-12, 13, (N,), generator=g).double()
    A, B = (Ai * 2.0 ** e).to(dev), (Bi * 2.0 ** f).to(dev)
    lda, ldb = lda or M + 16, ldb or N + 24
    bufA = torch.full((R + 3, lda), NAN, device=dev, dtype=torch.bfloat16)
    bufB = torch.full((R + 3, ldb), NAN, device=dev, dtype=torch.bfloat16)
    bufA[:R, a_col:a_col + M] = A.to(torch.bfloat16)
    bufB[:R, b_col:b_col + N] = B.to(torch.bfloat16)
    A16, B16 = bufA[:, a_col:], bufB[:, b_col:]
    assert A16.data_ptr() % 16 == 0 and B16.data_ptr() % 16 == 0 and A16.stride(0) == lda and B16.stride(0) == ldb
    Ad, Bd = A16[:R, :M].double(), B16[:R, :N].double()
    assert torch.equal(Ad, A) and torch.equal(Bd, B)                       # bf16 holds them exactly
    assert int(torch.isnan(bufA).sum()) == bufA.numel() - R * M and int(torch.isnan(bufB).sum()) == bufB.numel() - R * N
    # fp32 accumulation is exact in any order: every partial sum is an integer below 2^24 times 2^(e[m] + f[n])
    scale = (2.0 ** e).to(dev)[:, None] * (2.0 ** f).to(dev)[None, :]
    assert float(((Ad.abs().t() @ Bd.abs()) / scale).max()) < 2.0 ** 24
    return A16, B16, Ad, Bd


def _reference(Ad, Bd, alpha):
    a32 = float(torch.tensor(alpha, dtype=torch.float32))
    return (a32 * (Ad.t() @ Bd)).float()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run_and_check(K, A16, B16, ref, M, N, R, splitk, ldc, offset, alpha, tag):
    """One call into NaN-filled memory (twice: the second must give the same bits); the product region equals ref, the rest stays NaN."""
    dev = ref.device
    nslab = max(1, -splitk)
    flat = torch.full((offset + nslab * M * ldc + 2 * ldc + 4,), NAN, device=dev)
    assert flat.data_ptr() % 16 == 0
    Cbuf = flat[offset:offset + nslab * M * ldc + 2 * ldc]
    assert Cbuf.data_ptr() % 16 == 4 * offset
    K.gemm16_tn(A16, B16, Cbuf, M, N, R, A16.stride(0), B16.stride(0), ldc, alpha=alpha, splitk=splitk)
    first = flat.clone()
    slabs = Cbuf[:nslab * M * ldc].view(nslab, M, ldc)
    inside = slabs[:, :, :N]
    assert bool(torch.isfinite(inside).all()), f"{tag}: NaN or inf inside [M, N] - something outside the operand blocks entered the product"
    got = inside.sum(0) if nslab > 1 else inside[0]
    assert torch.equal(got, ref), f"{tag}: {int((got != ref).sum())} of {M * N} elements differ from the fp64 product, " \
                                  f"max |diff| / |ref| {float(((got.double() - ref.double()).abs() / ref.double().abs().clamp_min(1e-30)).max()):.3e}"
    # canaries: columns >= N of every row of every slab, the two rows behind the last slab, the floats before and behind the buffer
    assert bool(torch.isnan(slabs[:, :, N:]).all()), f"{tag}: a store went past column N"
    assert bool(torch.isnan(Cbuf[nslab * M * ldc:]).all()), f"{tag}: a store went past row M"
    assert bool(torch.isnan(flat[:offset]).all()) and bool(torch.isnan(flat[offset + Cbuf.numel():]).all()), f"{tag}: a store left the buffer"
    K.gemm16_tn(A16, B16, Cbuf, M, N, R, A16.stride(0), B16.stride(0), ldc, alpha=alpha, splitk=splitk)
    assert torch.equal(_bits(flat), _bits(first)), f"{tag}: a second call gave other bits"


@pytest.mark.parametrize("idx", range(len(C.GPU_CASES)), ids=lambda i: "x".join(map(str, C.GPU_CASES[i])))
def test_tn_gemm_every_site_exact(dev, idx):
    """Every launch site and pipeline state of spe_gemm_bf16tn (tests/tn_gemm_cases.py), strided operands inside NaN, each ldc variant:
    equal to the fp64 product, nothing stored outside [M, N], the same bits from a second call."""
    from spe_amd import kernels as K
    M, N, R, splitk = case = C.GPU_CASES[idx]
    A16, B16, Ad, Bd = _exact_operands(R, M, N, 1000 * idx + R, idx % 2 == 1, dev)
    plan = K.gemm16_tn_plan(M, N, R, splitk, lda=A16.stride(0), ldb=B16.stride(0))
    name = C.kernel_name(plan)
    assert name in C.INSTANCES
    alpha = 0.5 if splitk < 0 else 0.7
    ref = _reference(Ad, Bd, alpha)
    variants = [("ldc=N", N, 0), ("ldc=N+4", N + 4, 0)]
    if case in C.SCALAR_STORE_CASES:
        variants += [("ldc=N+1", N + 1, 0), ("ldc=N, C + 1 float", N, 1)]
    for vname, ldc, offset in variants:
        _run_and_check(K, A16, B16, ref, M, N, R, splitk, ldc, offset, alpha, f"{case} {vname}")
    rtiles, rt = -(-R // 64), plan["rt_per_split"]
    per_split = [max(0, min(rtiles, (z + 1) * rt) - z * rt) for z in range(plan["splits"])]
    print(f"TNGEMM {str(case):28s} -> {name:30s} row tiles per split {per_split}  variants {[v[0] for v in variants]}  exact")


def test_tn_gemm_refusals(dev):
    """Each status of tests/test_tn_gemm_plan_cpu.py::test_status_codes from spe_gemm_bf16tn itself, the pointer-alignment part of -2,
    and M = 0 / N = 0 (status 0, nothing launched): the NaN-filled output is untouched after each."""
    from spe_amd import kernels as K
    from spe_amd.lib import SpeLibraryError
    M, N, R = 72, 136, 400
    A16, B16, _, _ = _exact_operands(R, M, N, 5, False, dev)
    lda, ldb = A16.stride(0), B16.stride(0)
    Cb = torch.full((8 * (M + 2) * (N + 4),), NAN, device=dev)

    def refused(status, A=A16, B=B16, M=M, N=N, R=R, lda=lda, ldb=ldb, splitk=1):
        with pytest.raises(SpeLibraryError, match=f"status {status}$"):
            K.gemm16_tn(A, B, Cb, M, N, R, lda, ldb, N, splitk=splitk)
        assert bool(torch.isnan(Cb).all())

    refused(-2, M=70); refused(-2, N=132)
    refused(-2, lda=lda + 4); refused(-2, ldb=ldb + 4)
    refused(-2, splitk=2); refused(-2, splitk=7)
    refused(-4, R=0); refused(-4, R=-1)
    refused(-5, splitk=-8); refused(-5, R=1, splitk=-2)
    for which, t in (("A", A16), ("B", B16)):           # an operand 2 bytes behind a 16-byte boundary
        off2 = t.as_strided((1,), (1,), t.storage_offset() + 1)
        assert off2.data_ptr() == t.data_ptr() + 2
        refused(-2, **{which: off2})
    for kw in (dict(M=0), dict(N=0)):                   # nothing to do
        K.gemm16_tn(A16, B16, Cb, kw.get("M", M), kw.get("N", N), R, lda, ldb, N)
        assert bool(torch.isnan(Cb).all())
    K.gemm16_tn(A16, B16, Cb, M, N, R, lda, ldb, N, splitk=-7)             # the last split count that is taken: 7 row tiles
    assert bool(torch.isfinite(Cb[:7 * M * N]).all()) and bool(torch.isnan(Cb[7 * M * N:]).all())


# (N_out, K_in, R, splits expected of kernels._dw16_tn, instance, lda in units of N_out, dW_out given)
DW_CASES = [
    (384, 384, 400, 1, (64, 64), 1, True),              # no split: straight store into the view
    (384, 384, 1100, 2, (64, 64), 1, True),
    (384, 384, 8300, 14, (64, 64), 1, True),            # 130 row tiles, 10 per split: the last slab is empty
    (1536, 384, 8300, 14, (128, 128), 1, True),
    (384, 384, 1100, 2, (64, 64), 3, True),             # the middle block of a [R, 3 N] matrix (the grouped Linears, the decoder's memory side)
    (384, 384, 400, 1, (64, 64), 1, False),             # dW_out = None: a fresh tensor ...
    (384, 384, 1100, 2, (64, 64), 1, False),            # ... and the slab sum onto a zeroed one
]


@pytest.mark.parametrize("N,Kd,R,sk,inst,blocks,given", DW_CASES)
def test_dw16_tn_wrapper_exact(dev, N, Kd, R, sk, inst, blocks, given):
    """kernels._dw16_tn as the product calls it (auto_splitk, slabs, the column sum that OVERWRITES the bucket view): equal to the fp64
    product on the exact operands, written into a NaN-filled view in the middle of a NaN-filled flat buffer that is otherwise untouched."""
    from spe_amd import kernels as K
    assert min(K.auto_splitk(N, Kd, R, 1), max(1, R // 64)) == sk
    lda = blocks * N
    plan = K.gemm16_tn_plan(N, Kd, R, -sk if sk > 1 else 1, lda=lda, ldb=Kd)
    assert (plan["BM"], plan["BN"]) == inst
    dy16, x16, Ad, Bd = _exact_operands(R, N, Kd, 7 * R + N + blocks, blocks > 1, dev, lda=lda, a_col=N if blocks > 1 else 0, ldb=Kd, b_col=0)
    dy16, x16 = dy16[:R], x16[:R]
    if blocks > 1:
        assert bool(torch.isnan(dy16[:, N:]).all())                        # the neighbouring block
    ref = _reference(Ad, Bd, 1.0)
    pad = 192
    flat = torch.full((N * Kd + 2 * pad,), NAN, device=dev)
    view = flat[pad:pad + N * Kd].view(N, Kd) if given else None
    for _ in range(2):                                                     # the second step finds last step's gradient in the view
        dW = K._dw16_tn(dy16, x16, N, Kd, R, view, lda=lda if blocks > 1 else None)
        assert dW.shape == (N, Kd)
        assert torch.equal(dW, ref), f"{int((dW != ref).sum())} of {N * Kd} elements differ from the fp64 product"
        if given:
            assert dW.data_ptr() == view.data_ptr()
        assert bool(torch.isnan(flat[:pad]).all()) and bool(torch.isnan(flat[pad + N * Kd:]).all())
        if not given:
            assert bool(torch.isnan(flat).all())
    print(f"TNGEMM _dw16_tn N={N} K={Kd} R={R} lda={lda} dW_out={'view' if given else 'None'} -> {sk} split(s) on {C.kernel_name(plan)}  exact")
