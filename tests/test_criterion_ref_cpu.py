"""The references of tests/criterion_ref.py checked against independent restatements, and the conditions under which
tests/test_criterion_kernels_gpu.py may assert what it asserts, checked on every input of tests/criterion_cases.py.  No GPU, nothing of
spe_amd.

  assignment  lsap_lowest_index against scipy.optimize.linear_sum_assignment: identical pairs where the optimum is unique (cont,
              mixed_scale - the licence for demanding SciPy's pairs of the kernel), the same optimal total, exactly, on the integer
              families, the same multiset of (query, base column) on duplicated target columns;
  focal       focal_ref against binary_cross_entropy_with_logits + autograd; no `saturated` logit near the clamp threshold; the fp32
              composition inside the bounds the kernel is held to;
  box losses  on the dyadic family the fp32 and fp64 autograd gradients agree to 1e-6 (the ties coincide);
  cost        the fp32 composition of the matcher cost inside matcher_cost_tol, element by element, on all three logit families;
  NMS         greedy_nms_ref against the brute force of tests/test_round5_gpu.py;
  jitter      jitter_pick_ref's order, fill and all-fail / all-pass boxes.
Lines with the prefix CRITERION-CPU are the reference's own figures recorded in profiles/criterion_edges.txt."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import criterion_cases as cc  # noqa: E402
import criterion_ref as cr  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------------------
# assignment
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", cc.HUNG_FAMILIES)
@pytest.mark.parametrize("case", cc.HUNG_CASES, ids=cc.hung_id)
def test_lsap_lowest_index_vs_scipy(case, fam):
    L, Q, sizes = case
    cost, base = cc.hung_cost(case, fam)
    sci = cr.assignment_triples(cost, L, Q, sizes, linear_sum_assignment)
    low = cr.assignment_triples(cost, L, Q, sizes, cr.lsap_lowest_index)
    cr.check_assignment(*low, case)
    cr.check_assignment(*sci, case)
    ts, tl = cr.assignment_totals(cost, sci[0], sci[1], case), cr.assignment_totals(cost, low[0], low[1], case)
    if fam in cc.HUNG_UNIQUE:
        # the condition of the GPU module: should a seed ever violate it, the seed changes (criterion_cases.HUNG_RESEED), not this line
        assert all(torch.equal(a, b) for a, b in zip(sci, low)), "the optimum of this case is not unique"
    elif fam in cc.HUNG_INTEGER:
        assert torch.equal(ts, tl), (ts, tl)                 # sums of small integers (and of 2.5): exact in fp64
    else:
        ms = sorted(zip(sci[0].tolist(), base[sci[1]].tolist()))
        ml = sorted(zip(low[0].tolist(), base[low[1]].tolist()))
        assert ms == ml, "differs from SciPy by more than a permutation of identical targets"
        assert torch.allclose(ts, tl, rtol=1e-12, atol=0)


def test_lsap_lowest_index_takes_the_lowest_query_among_ties():
    """All costs equal: target i goes to query i.  Two equal cheapest queries: the lower one."""
    q, t = cr.lsap_lowest_index(np.full((7, 4), 2.5))
    assert q.tolist() == [0, 1, 2, 3] and t.tolist() == [0, 1, 2, 3]
    blk = np.array([[5.0], [1.0], [3.0], [1.0]])
    q, t = cr.lsap_lowest_index(blk)
    assert q.tolist() == [1] and t.tolist() == [0]


def test_lsap_lowest_index_is_quick():
    import time
    blk = 3 * torch.randn(1024, 128, generator=torch.Generator().manual_seed(1)).numpy()
    t0 = time.perf_counter()
    q, t = cr.lsap_lowest_index(blk)
    dt = time.perf_counter() - t0
    i, j = linear_sum_assignment(blk)
    assert np.array_equal(q, i) and np.array_equal(t, j)
    assert dt < 1.0, dt


def test_hungarian_cases_sit_on_the_boundaries():
    sizes = {(Q, n) for _, Q, ss in cc.HUNG_CASES for n in ss if n}
    assert {128, 129, 320, 321, 512, 513, 1024} <= {Q for Q, _ in sizes}
    assert any(n * Q == cc.HUNG_LDS_FLOATS for Q, n in sizes)
    for Q in (193, 320, 512, 1024):
        st = {cc.staged(Q, n) for q, n in sizes if q == Q and n > 1}
        assert st == {True, False}, Q
    assert all(n <= Q for Q, n in sizes)


# ------------------------------------------------------------------------------------------------------------------------------
# focal loss
# ------------------------------------------------------------------------------------------------------------------------------
def _focal_bce(logits, tclass, roww, alpha, gamma):
    """The formula of tests/test_kernels_gpu.py::test_matcher_cost_and_losses, with alpha < 0 switching alpha_t off."""
    L, R, Kc = logits.shape
    x = logits.double().requires_grad_()
    t = torch.nn.functional.one_hot(tclass.long(), Kc + 1)[..., :Kc].double()
    prob = x.sigmoid()
    ce = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction="none")
    pt = (prob * t + (1 - prob) * (1 - t)).clamp(1e-5, 1 - 1e-5)
    w = 1.0 if roww is None else roww.double()[..., None]
    at = (alpha * t + (1 - alpha) * (1 - t)) if alpha >= 0 else 1.0
    ref = (at * w * ce * (1 - pt) ** gamma).sum((1, 2))
    (rg,) = torch.autograd.grad(ref.sum(), x)
    return ref.detach(), rg


_FOCAL32 = {}


@pytest.mark.parametrize("fam", cc.FOCAL_FAMILIES)
@pytest.mark.parametrize("L,R,Kc", cc.FOCAL_SHAPES)
def test_focal_ref(L, R, Kc, fam):
    x, tclass, roww = cc.focal_inputs(L, R, Kc, fam)
    assert bool((tclass == Kc).any()) and int(tclass.max()) <= Kc and int(tclass.min()) >= 0
    if fam == "saturated":
        assert float((x.abs() - cr.CLAMP_LOGIT).abs().min()) > 0.25
    if fam == "ties":
        top = x == x.max(-1, keepdim=True).values
        assert bool((top.sum(-1) >= min(2, Kc)).all())
        if Kc > 65 and R >= 4:
            assert bool((top[..., :64].sum(-1) == 0).any()) and bool((top.sum(-1) == Kc).any())
    am = cr.argmax_lowest(x)
    assert bool((x.gather(-1, am[..., None])[..., 0] == x.max(-1).values).all())
    lower = torch.arange(Kc).expand_as(x) < am[..., None]
    assert not bool(((x == x.max(-1, keepdim=True).values) & lower).any()), "argmax_lowest is not the lowest"
    for rw in (None, roww):
        for alpha, gamma in cc.FOCAL_PARAMS:
            loss, grad, am2 = cr.focal_ref(x, tclass, rw, alpha, gamma)
            rl, rg = _focal_bce(x, tclass, rw, alpha, gamma)
            assert torch.equal(am2, am)
            assert torch.allclose(loss, rl, rtol=1e-12, atol=0) and torch.allclose(grad, rg, rtol=1e-9, atol=1e-12), (alpha, gamma)
            # the same composition in fp32 against the figures the kernel is held to
            l32, g32, _ = cr.focal_ref(x, tclass, rw, alpha, gamma, dtype=torch.float32)
            fig = _FOCAL32.setdefault(fam, {"loss": 0.0, "grad": 0.0, "grad/bound": 0.0})
            fig["loss"] = max(fig["loss"], cr.rel(l32, loss))
            fig["grad"] = max(fig["grad"], cr.rel(g32, grad))
            fig["grad/bound"] = max(fig["grad/bound"], float(((g32.double() - grad).abs() / cr.focal_grad_tol(grad)).max()))
            if fam == "saturated":
                assert cr.rel(l32, loss) < 1e-5 and float(((g32.double() - grad).abs() / cr.focal_grad_tol(grad)).max()) <= 1.0, fig


def test_focal_fp32_composition_figures():
    """Runs after test_focal_ref (file order): the fp32 torch composition's own distance from fp64, per family."""
    assert set(_FOCAL32) == set(cc.FOCAL_FAMILIES), "run together with test_focal_ref: it collects these figures"
    for fam, fig in _FOCAL32.items():
        print("CRITERION-CPU focal fp32 composition", fam, " ".join(f"{k} {v:.3e}" for k, v in fig.items()))
        assert fig["loss"] < 1e-5, (fam, fig)


# ------------------------------------------------------------------------------------------------------------------------------
# box losses
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,L", cc.BOX_CASES)
def test_box_loss_ref_dyadic_ties_coincide(n, L):
    pred, srow, tbox, w, lidx = cc.box_inputs(n, L, "dyadic")
    for t in (pred[srow], tbox):
        u = t.double() * 64
        assert bool((u == u.round()).all()) and float(u.min()) >= 8 and float(u.max()) <= 56
    assert srow.unique().numel() == n
    if L > 1:
        assert not bool((lidx == L // 2).any()) and (n < 3 or bool((lidx[1:] < lidx[:-1]).any()))
    for wt in (None, w):
        s64, g1, g2 = cr.box_loss_ref(pred, srow, tbox, wt, lidx, L)
        s32, h1, h2 = cr.box_loss_ref(pred, srow, tbox, wt, lidx, L, dtype=torch.float32)
        assert torch.equal(h1.double(), g1), "L1 signs differ between fp32 and fp64"
        assert float((h2.double() - g2).abs().max()) < 1e-6, float((h2.double() - g2).abs().max())
        assert cr.rel(s32, s64) < 1e-6
    if n >= len(cc.DYADIC_SPECIAL):
        s, t = cr.to_xyxy(pred[srow].double()), cr.to_xyxy(tbox.double())
        k = len(cc.DYADIC_SPECIAL)
        shared = (s[:k] == t[:k]).sum(1).tolist()
        assert shared[:4] == [4, 1, 2, 3]
        gi = cr.giou_diag(s[:k], t[:k])
        assert float(gi[0]) == 1.0 and float(gi[6]) < 0 and float(gi[7]) < 0 and float(gi[8]) < 0
        d = (pred[srow][:k] - tbox[:k]) == 0
        assert d[9:13].sum(1).tolist() == [1, 1, 1, 1]
        _, g1, _ = cr.box_loss_ref(pred, srow, tbox, None, lidx, L)
        assert bool((g1[:k][d] == 0).all()) and bool((g1[:k][~d].abs() == 1).all())


def test_box_loss_ref_tie_gradients_are_split():
    """An identical pair: GIoU is 1 and every min / max is a tie; torch splits them 1/2 - 1/2, so the gradient is half of what either
    one-sided choice gives, not zero and not the full one."""
    p = torch.tensor([[0.5, 0.5, 0.25, 0.25]])
    _, _, g = cr.box_loss_ref(p, torch.tensor([0]), p.clone(), None, torch.tensor([0]), 1)
    # every path from a coordinate to the loss passes one min / max, so the 1/2 split is the mean of the two one-sided slopes: a central difference
    eps = 1e-6
    fd = torch.zeros(4, dtype=torch.float64)
    for j in range(4):
        pp, pm = p.double().clone(), p.double().clone()
        pp[0, j] += eps; pm[0, j] -= eps
        f = lambda z: float(1 - cr.giou_diag(cr.to_xyxy(z), cr.to_xyxy(p.double())))
        fd[j] = (f(pp) - f(pm)) / (2 * eps)
    assert torch.allclose(g[0], fd, atol=1e-5), (g, fd)


def test_box_loss_bwd_ref_adds_repeated_rows():
    for n in cc.BWD_N:
        srow, lidx, g1, g2, c1, c2, P = cc.bwd_inputs(n)
        d = cr.box_loss_bwd_ref(srow, lidx, g1, g2, c1, c2, (P, 4))
        if n >= 3:
            assert int((srow == srow[0]).sum()) == 3
        want = torch.zeros(P, 4, dtype=torch.float64)
        for i in range(n):
            want[srow[i]] += float(c1[lidx[i]]) * g1[i].double() + float(c2[lidx[i]]) * g2[i].double()
        assert torch.allclose(d, want, rtol=1e-12, atol=1e-15)


# ------------------------------------------------------------------------------------------------------------------------------
# matcher cost
# ------------------------------------------------------------------------------------------------------------------------------
def _giou_plain(a, b):
    """Scalar GIoU of two xyxy boxes in Python floats."""
    iw, ih = max(min(a[2], b[2]) - max(a[0], b[0]), 0.0), max(min(a[3], b[3]) - max(a[1], b[1]), 0.0)
    inter = iw * ih
    uni = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    ea = max(max(a[2], b[2]) - min(a[0], b[0]), 0.0) * max(max(a[3], b[3]) - min(a[1], b[1]), 0.0)
    return inter / uni - (ea - uni) / ea


def test_matcher_cost_ref_layout_and_formula():
    """A few elements of the packed cost recomputed one by one in Python floats."""
    import math
    case = cc.COST_CASES[1]
    L, B, Q, Kc, sizes = case
    logits, boxes, ids, tb = cc.cost_inputs(case, "plain")
    wc, wb, wg = cc.COST_WEIGHTS
    cost, xs = cr.matcher_cost_ref(logits, boxes, ids, tb, sizes, wc, wb, wg)
    toff = cr.toff_of(sizes)
    assert cost.shape == (L, Q * toff[-1])
    for l, b, q, j in ((0, 1, 0, 0), (1, 1, 16, 2), (0, 4, 3, 14), (1, 4, 16, 0)):
        t = toff[b] + j
        x = float(logits[l, b, q, ids[t]])
        p = 1 / (1 + math.exp(-x))
        cls = 0.25 * (1 - p) ** 2 * -math.log(p + 1e-8) - 0.75 * p ** 2 * -math.log(1 - p + 1e-8)
        s, g = boxes[l, b, q].double().tolist(), tb[t].double().tolist()
        l1 = sum(abs(u - v) for u, v in zip(s, g))
        xy = lambda z: (z[0] - z[2] / 2, z[1] - z[3] / 2, z[0] + z[2] / 2, z[1] + z[3] / 2)
        want = wb * l1 + wc * cls - wg * _giou_plain(xy(s), xy(g))
        e = Q * toff[b] + q * sizes[b] + j
        assert abs(float(cost[l, e]) - want) < 1e-12 and float(xs[l, e]) == x


@pytest.mark.parametrize("fam", list(cc.COST_FAMILIES))
def test_matcher_cost_fp32_composition_inside_the_bound(fam):
    worst = 0.0
    for case in cc.COST_CASES:
        L, B, Q, Kc, sizes = case
        logits, boxes, ids, tb = cc.cost_inputs(case, fam)
        lo, hi = cc.COST_FAMILIES[fam]
        assert float(logits.abs().min()) >= lo and float(logits.abs().max()) <= hi
        c64, xs = cr.matcher_cost_ref(logits, boxes, ids, tb, sizes, *cc.COST_WEIGHTS)
        c32, _ = cr.matcher_cost_ref(logits, boxes, ids, tb, sizes, *cc.COST_WEIGHTS, dtype=torch.float32)
        ratio = (c32.double() - c64).abs() / cr.matcher_cost_tol(xs, *cc.COST_WEIGHTS)
        assert bool(torch.isfinite(c32).all())
        worst = max(worst, float(ratio.max()))
    print("CRITERION-CPU cost fp32 composition", fam, f"error/bound {worst:.3f}")
    assert worst < 1.0, worst


def test_class_cost_tol_follows_the_conditioning():
    t = cr.class_cost_tol(torch.tensor([0.0, 6.0, 12.0, 17.0, 25.0, 40.0, -40.0]))
    assert abs(float(t[0]) - 2e-5) < 1e-6 and float(t[1]) < 1e-4
    assert 1e-2 < float(t[2]) < 1e-1 and float(t[3]) > 1.0 and float(t[4]) > 1.0


# ------------------------------------------------------------------------------------------------------------------------------
# NMS, jitter
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cc.NMS_N)
def test_greedy_nms_ref_vs_bruteforce(n):
    """Class by class, as test_per_class_nms_vs_bruteforce does, at every size of the GPU module (4096: ~0.7 s per image and count)."""
    from test_round5_gpu import _greedy_nms_bruteforce as brute
    boxes, labels, scores, counts = cc.nms_inputs(n)
    for img in range(cc.NMS_IMAGES):
        for count in (None, counts[img]):
            m = n if count is None else count
            keep = cr.greedy_nms_ref(boxes[img], labels[img], cc.NMS_THR, count)
            want = torch.zeros(n, dtype=torch.bool)
            for pc in sorted(set(labels[img][:m].tolist())):
                idx = ((labels[img] == pc) & (torch.arange(n) < m)).nonzero().reshape(-1)
                want[idx[brute(boxes[img][idx], scores[img][idx], cc.NMS_THR)]] = True
            assert torch.equal(keep, want), (n, img, count)
            assert not bool(keep[m:].any())
        if n >= 8:
            lab = labels[img]
            sc = scores[img]
            assert bool((lab[1:] >= lab[:-1]).all()) and bool(((sc[1:] <= sc[:-1]) | (lab[1:] > lab[:-1])).all()) and int((lab == 9).sum()) == 4
            assert int(cr.greedy_nms_ref(boxes[img], lab, cc.NMS_THR)[lab == 9].sum()) == 3         # 0.5015 suppresses, 0.4993 does not
        if n >= 700:
            assert int((labels[img] == 0).sum()) > 256


@pytest.mark.parametrize("M,ncand,ratio", cc.JITTER_CASES)
def test_jitter_pick_ref(M, ncand, ratio):
    box, scale = cc.jitter_inputs(M, ncand, ratio)
    out = cr.jitter_pick_ref(box, scale, ratio)
    assert out.shape == (M, ratio, 4) and torch.equal(out[:, -1], box)
    cand = scale * box[:, None, :]
    for m in range(M):
        a, b = cr.to_xyxy(cand[m].double()), cr.to_xyxy(box[m].double())
        if M > 1 and m == 0:
            continue                         # the 1e-6 box: its IoU is rounding noise; the reference must keep nothing (below)
        inter = (torch.minimum(a[:, 2:], b[2:]) - torch.maximum(a[:, :2], b[:2])).clamp(min=0).prod(1)
        iou = inter / ((a[:, 2:] - a[:, :2]).prod(1) + (b[2:] - b[:2]).prod() - inter)        # fp64, of the fp32 candidates
        if ncand and float((iou - 0.7).abs().min()) < 1e-6:
            continue                         # a candidate on the threshold: fp32 may decide either way
        picked = cand[m][iou > 0.7][:ratio - 1]
        k = picked.shape[0]
        assert torch.equal(out[m, :k], picked) and bool((out[m, k:] == box[m]).all()), m
    if M > 1:
        assert bool((out[0] == box[0]).all()), "a candidate of the 1e-6 box passed"
        if ncand >= ratio - 1:
            assert torch.equal(out[1, :ratio - 1], cand[1, :ratio - 1]), "a candidate of the narrow jitter failed"
