"""The reference, the bounds and the case list of tests/test_mha_gpu.py, checked without a GPU: the fp64 restatement against torch's
softmax attention and autograd, a torch emulation of the kernels' arithmetic against the bounds, the coverage of the case list, and
the pinned chunk counts against spe_mha_plan (a host-only entry point)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mha_cases as C  # noqa: E402
import mha_ref as R  # noqa: E402

IDS = [C.case_id(c) for c in C.GPU_CASES]
SMALL = [c for c in C.GPU_CASES if c[0] * c[1] * c[2] * c[3] <= 200000]


def test_case_ids_are_unique():
    assert len(set(IDS)) == len(IDS)
    assert 80 <= len(IDS) <= 140


def test_plan_restatement_reproduces_the_table():
    """The four rows of B = H = 1, Lq <= 64 worked out by hand from spe_mha_plan."""
    assert C.plan(1, 1, 64, 128)[1:] == (8, 4, 2, 4)
    assert C.plan(1, 1, 64, 144)[1:] == (9, 5, 2, 4)
    assert C.plan(1, 1, 64, 272)[1:] == (17, 5, 4, 2)
    assert C.plan(1, 1, 64, 336)[1:] == (21, 5, 5, 1)
    assert C.plan(32, 32, 64, 128)[3] == 1 and C.plan(16, 16, 17, 515)[1:] == (33, 9, 4, 6)


@pytest.mark.parametrize("case", C.GPU_CASES, ids=IDS)
def test_pinned_nch_is_the_plan(case):
    from spe_amd import kernels as K
    B, H, Lq, Lk = case[:4]
    assert K.mha_plan(B, H, Lq, Lk) == case[9] == C.plan(B, H, Lq, Lk)[3]


def test_cases_reach_every_site():
    hit = set()
    for c in C.GPU_CASES:
        hit |= C.sites(c)
    assert C.REQUIRED - hit == set(), sorted(C.REQUIRED - hit)
    assert all(c[3] <= 600 and c[2] <= 200 for c in C.GPU_CASES)


def test_every_batch_keeps_a_key():
    for c in C.GPU_CASES:
        rows = C.mask_rows(c)
        if rows is None:
            continue
        assert len(rows) == c[0] and all(len(r) == c[3] for r in rows)
        for b, r in enumerate(rows):
            if c[6] == "all_padded_batch" and b == C.ALL_PADDED_BATCH:
                assert all(r)
            else:
                assert not all(r), (c, b)
            if c[6] == "one_key":
                assert r.count(0) == 1 and r[C.one_key(c, b)] == 0
        if c[6] == "one_key" and c[0] > 1:
            assert len({C.one_key(c, b) for b in range(c[0])}) == c[0]
        if c[6] in ("chunk0", "chunk_mid", "chunk_last"):
            _, ntk, ch_len, nch, _ = C.fill(c[2], c[3], c[9])
            ch = {"chunk0": 0, "chunk_mid": nch // 2, "chunk_last": nch - 1}[c[6]]
            assert 0 < ch < nch - 1 or c[6] != "chunk_mid"
            assert all(all(r[16 * ch_len * ch:16 * ch_len * (ch + 1)]) for r in rows)


def test_operands_are_on_the_16_bit_grid():
    for c in SMALL[::5]:
        op = R.operands(c)
        for n in ("q", "k", "v", "do"):
            x = op[n]
            assert torch.equal(x.half().double(), x) and torch.equal(x.bfloat16().double(), x), (c, n)


def test_score_families_do_what_they_say():
    for c in C.GPU_CASES:
        if c[7] == "normal" or c[6] != "none":
            continue
        op = R.operands(c)
        s = torch.einsum("bqhd,bkhd->bhqk", op["q"], op["k"])
        tmax = torch.stack([s[..., 16 * t:16 * t + 16].amax(-1) for t in range((c[3] + 15) // 16)], -1)
        if c[7] == "ascending":
            assert bool((tmax[..., 1:] > tmax[..., :-1]).all())
        elif c[7] == "descending":
            assert bool((tmax[..., 1:] < tmax[..., :-1]).all())
        elif c[7] == "wide":
            assert float(s.max() - s.min()) >= 55
        else:
            ties = C.tie_keys(c[3])
            assert len({t // 16 for t in ties}) >= 3
            assert bool((s[..., ties] == s.amax(-1, keepdim=True)).all())


@pytest.mark.parametrize("case", SMALL[::3], ids=[C.case_id(c) for c in SMALL[::3]])
@pytest.mark.parametrize("drop", [False, True])
def test_reference_is_torch_softmax_attention(case, drop):
    """O, LSE and the three gradients of the restatement against softmax attention in fp64 with autograd, to 1e-12."""
    B, H, Lq, Lk, dk, dv = case[:6]
    op = R.operands(case)
    p = 0.3 if drop else 0.0
    keep = R.host_keep(case[:8] + (p, case[9])) if drop else None
    ref = R.reference(op, p, keep)
    live = ~ref["dead"]
    q, k, v = (op[n].clone().requires_grad_() for n in ("q", "k", "v"))
    z = torch.einsum("bqhd,bkhd->bhqk", q, k) * R.LN2
    if op["mask"] is not None:
        z = z.masked_fill(op["mask"][:, None, None, :], float("-inf"))
    Pm = z.softmax(-1)
    if drop:
        Pm = Pm * keep / (1.0 - p)
    O = torch.einsum("bhqk,bkhd->bqhd", Pm, v)
    gq, gk, gv = torch.autograd.grad(O[live], (q, k, v), op["do"][live])
    # the restatement rounds D to fp32 (as handed to the kernel): compare with the unrounded D put back
    refx = R.reference(op, p, keep)
    tol = lambda a, b: float((a - b).abs().max() / (1.0 + b.abs().max()))
    assert tol(ref["O"][live], O[live].detach()) < 1e-12
    lse = torch.logsumexp(z, -1) * R.LOG2E
    assert tol(ref["LSE"][live], lse[live].detach()) < 1e-12
    assert tol(ref["dv"][live], gv[live]) < 1e-12
    # q^ carries scale * log2 e: dq = scale * log2 e * d/dq^
    D64 = (op["do"] * O.detach()).sum(-1).permute(0, 2, 1)
    fix = refx["P"] * (ref["D"] - D64)[..., None]                                # dS(fp32 D) - dS(fp64 D), [B,H,Lq,Lk]
    dq_fix = op["scale"] * torch.einsum("bhqk,bkhd->bqhd", fix, op["k"])
    dk_fix = R.LN2 * torch.einsum("bhqk,bqhd->bkhd", fix, op["q"])
    assert tol((ref["dq"] + dq_fix)[live], (gq * op["scale"] * R.LOG2E)[live]) < 1e-12
    assert tol((ref["dk"] + dk_fix)[live], gk[live]) < 1e-12


_worst = {}


@pytest.mark.parametrize("case", C.GPU_CASES, ids=IDS)
def test_emulation_fits_the_bounds(case):
    """fp32 sums, per-tile online softmax in the planned chunks with merge, p through fp16, dS and P kd through bf16: at or below
    1.0 x bound on every case for O and LSE, and for dq, dk, dv at or below 1.0 x the bound with a bf16 rounding at its worst case
    2^-8 (mha_ref: ub), so the tolerance the GPU test asserts (2 x bound) is not measured on the code under test."""
    B, H, Lq, Lk, dk, dv, mfam, sfam, p, nch = case
    ch_len = C.fill(Lq, Lk, nch)[2]
    op = R.operands(case)
    keep = R.host_keep(case)
    ref = R.reference(op, p, keep, nch)
    live = ~ref["dead"]
    O, LSE, dq, dk_, dv_ = R.emulate(op, ch_len, p, keep, ref["LSE"], ref["D"])
    r = dict(O=R.ratio(O, ref["O"], ref["bO"], live), LSE=R.ratio(LSE, ref["LSE"], ref["bLSE"], live))
    for n, x in (("dq", dq), ("dk", dk_), ("dv", dv_)):
        r[n] = R.ratio(x, ref[n], ref["b" + n], live)                 # against what the GPU test doubles: up to 2 (mha_ref: ub)
        r[n + "w"] = R.ratio(x, ref[n], ref["b" + n + "w"], live)     # one bf16 rounding at its worst, 2^-8
        assert bool((ref["b" + n + "w"] <= 2 * ref["b" + n]).all())
    print("MHAEMU", C.case_id(case), " ".join("%s=%.3f" % kv for kv in r.items()))
    for n, x in r.items():
        _worst[n] = max(_worst.get(n, 0.0), x)
    assert all(x <= (2.0 if n in ("dq", "dk", "dv") else 1.0) for n, x in r.items()), r
    if nch > 1:                      # the backward also accepts one chunk on a multi-chunk shape
        _, _, dq1, _, _ = R.emulate(op, ch_len, p, keep, ref["LSE"], ref["D"], bwd_ch_len=(Lk + 15) // 16)
        assert R.ratio(dq1, ref["dq"], ref["bdqw"], live) <= 1.0


def test_emulation_worst_ratios():
    """Prints the worst ratio per output over the whole list (recorded in profiles/mha_edges.txt)."""
    print("MHAEMU worst", " ".join("%s=%.3f" % kv for kv in sorted(_worst.items())))
    assert all(x <= (2.0 if n in ("dq", "dk", "dv") else 1.0) for n, x in _worst.items())


def test_bounds_are_tight_enough_to_see_a_wrong_kernel():
    """The bounds are a small fraction of the outputs: a dropped rescale, a leaked key or ln 2 for 1 is orders above them."""
    case = (2, 4, 17, 272, 96, 48, "none", "normal", 0, 4)
    op = R.operands(case)
    ref = R.reference(op, nch=4)
    for n in ("O", "dq", "dk", "dv"):             # a few unit roundoffs of the largest entry (the sums cancel, the bounds do not)
        assert float(ref["b" + n].max()) < 5 * (R.U16 if n == "O" else R.UB) * float(ref[n].abs().max()), n
    assert float(ref["bLSE"].max()) < 1e-4
    # natural log in place of log2 in LSE, and a dropped ln 2 in dk
    assert float((ref["LSE"] * (1 - R.LN2)).abs().max() / ref["bLSE"].max()) > 100
    assert float((ref["dk"] * (1 / R.LN2 - 1)).abs().max() / ref["bdk"].max()) > 100
