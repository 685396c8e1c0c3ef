"""The seven set-criterion kernels of csrc/loss.hip against the plain references of tests/criterion_ref.py, on the inputs of
tests/criterion_cases.py (whose conditions tests/test_criterion_ref_cpu.py checks without a GPU):

  assignment  hungarian_kernel<2 / 5 / 8 / 16> at both sides of every CPL boundary, LDS-staged and unstaged problems in one launch, empty
              images, unique optima (SciPy's pairs) and exact ties (the documented lowest-index rule; validity and SciPy's optimal total
              whatever the rule), and one SetCriterion call on one-to-many targets with exact duplicates;
  focal       one to 257 row blocks (one block, a full group of 16, the second group, more than 16 groups), one to three lane passes,
              alpha < 0, gamma 0 / 0.5 / 2, logits past the p_t clamp, tied maxima; two launches give the same bits;
  box losses  one pair to three 1024-pair chunks, 1 / 6 / 512 layers, no weights, identical / nested / disjoint / edge-sharing boxes
              whose min / max ties coincide in fp32 and fp64, a layer without pairs, sums that accumulate; the scatter with a row
              matched three times;
  cost        elements across a block edge, empty images before, between and after, saturated logits, the degenerate-box flag;
  NMS         1 to 4096 detections per image, a class longer than the 256-thread stride, with and without counts;
  jitter      0 to 1000 candidates, 1 to 70 rows per box, boxes whose candidates all fail or all pass;
  refusals    Q = 1025, L = 513, nmax = 4097, a misaligned scale pointer.
Every entry point is called through spe_amd.lib.call on outputs allocated here: longer than needed by a guard region and pre-filled
with a bit pattern the kernel cannot produce, so a store behind the end and an element never stored both show.
Measured figures: profiles/criterion_edges.txt (every line this module prints with the prefix CRITERION)."""
import functools
import os
import sys
import time

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import criterion_cases as cc  # noqa: E402
import criterion_ref as cr  # noqa: E402

pytestmark = pytest.mark.gpu

T0 = time.perf_counter()
GUARD = 64                               # elements behind the end of every output
FILL = {torch.float32: 0x5A5A5A5A, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.uint8: 0x5A}
# (fp32 1.5e16, int 1.5e9 / 6.5e18, byte 90: no cost, gradient, row index, layer, class or keep flag of these tests has that value)
FIGS = {}                                # (kernel, family) -> {figure: maximum}, printed by the last test


def _filled(n, dtype, dev):
    """n elements + the guard, all holding the pattern."""
    raw = {torch.float32: torch.int32, torch.uint8: torch.uint8}.get(dtype, dtype)
    return torch.full((n + GUARD,), FILL[dtype], dtype=raw, device=dev).view(dtype)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _untouched(t):
    return bool((_bits(t) == FILL[t.dtype]).all())


def _all_written(t):
    return not bool((_bits(t) == FILL[t.dtype]).any())


def _check_stores(name, t, n):
    assert _untouched(t[n:]), (name, "stored behind the end")
    assert _all_written(t[:n]), (name, "an element was never stored")


def _note(kernel, fam, **figs):
    d = FIGS.setdefault((kernel, fam), {})
    for k, v in figs.items():
        d[k] = max(d.get(k, 0.0), float(v))


def _p(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------------------------------------
# assignment
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hung_expected(idx, fam):
    from scipy.optimize import linear_sum_assignment
    case = cc.HUNG_CASES[idx]
    L, Q, sizes = case
    cost, base = cc.hung_cost(case, fam)
    return (cost, base, cr.assignment_triples(cost, L, Q, sizes, linear_sum_assignment),
            cr.assignment_triples(cost, L, Q, sizes, cr.lsap_lowest_index))


def _run_hungarian(K, cost, sizes, L, Q, dev):
    B, total = len(sizes), sum(sizes)
    toff = torch.tensor(cr.toff_of(sizes), dtype=torch.int32, device=dev)
    n = L * total
    srow, gidx, lidx = _filled(n, torch.int64, dev), _filled(n, torch.int64, dev), _filled(n, torch.int32, dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    costd = cost.to(dev).contiguous()
    K.lib.call("spe_hungarian", costd.data_ptr(), toff.data_ptr(), srow.data_ptr(), gidx.data_ptr(), lidx.data_ptr(), err.data_ptr(),
               L, B, Q, K._st())
    return srow, gidx, lidx, err, n


@pytest.mark.parametrize("fam", cc.HUNG_FAMILIES)
@pytest.mark.parametrize("case", cc.HUNG_CASES, ids=cc.hung_id)
def test_hungarian(dev, case, fam):
    from spe_amd import kernels as K
    L, Q, sizes = case
    cost, base, sci, low = _hung_expected(cc.HUNG_CASES.index(case), fam)
    srow, gidx, lidx, err, n = _run_hungarian(K, cost, sizes, L, Q, dev)
    for name, t in (("srow", srow), ("gidx", gidx), ("lidx", lidx)):
        _check_stores(name, t, n)
    assert int(err.item()) == 0
    got = (srow[:n].cpu(), gidx[:n].cpu(), lidx[:n].cpu().long())
    # whatever the tie rule: a valid assignment of SciPy's optimal total
    cr.check_assignment(*got, case)
    tg, ts = cr.assignment_totals(cost, got[0], got[1], case), cr.assignment_totals(cost, sci[0], sci[1], case)
    same_sci = all(torch.equal(a, b) for a, b in zip(got, sci))
    same_low = all(torch.equal(a, b) for a, b in zip(got, low))
    print("CRITERION hungarian", cc.hung_id(case), fam, f"pairs==scipy {int(same_sci)} pairs==lowest-index {int(same_low)}",
          f"total-scipy {float((tg - ts).abs().max()):.3e}")
    _note("hungarian", fam, scipy_pairs_differ=not same_sci, lowest_index_pairs_differ=not same_low,
          total_minus_scipy=float((tg - ts).abs().max()))
    if fam == "dupcol":
        assert sorted(zip(got[0].tolist(), base[got[1]].tolist())) == sorted(zip(sci[0].tolist(), base[sci[1]].tolist())), \
            "differs from SciPy by more than a permutation of identical targets"
        assert torch.allclose(tg, ts, rtol=1e-12, atol=0)
    else:
        assert torch.equal(tg, ts), (tg, ts)
    if fam in cc.HUNG_UNIQUE:
        assert same_sci, "unique optimum, yet not SciPy's pairs"
    if fam != "zeros_signed":             # the kernel's integer keys put -0.0 before +0.0; the restatement's comparisons do not
        assert same_low, "not the lowest-index rule the kernel documents"


def test_hungarian_empty_images_shift_nothing(dev):
    """The (2, 128, [128, 0, 17]) problem with its empty image removed gives the same pairs, image index aside."""
    from spe_amd import kernels as K
    case = cc.HUNG_CASES[5]
    L, Q, sizes = case
    assert sizes == [128, 0, 17]
    cost, _ = cc.hung_cost(case, "cont")
    a = _run_hungarian(K, cost, sizes, L, Q, dev)
    b = _run_hungarian(K, cost, [128, 17], L, Q, dev)
    n = a[4]
    assert n == b[4] and torch.equal(a[1][:n], b[1][:n]) and torch.equal(a[2][:n], b[2][:n])
    sa, sb = a[0][:n].cpu(), b[0][:n].cpu()
    la, lb = sa // (3 * Q), sb // (2 * Q)
    ia, ib = (sa // Q) % 3, (sb // Q) % 2
    assert torch.equal(la, lb) and torch.equal(sa % Q, sb % Q) and torch.equal(ia.clamp(max=1) * (ia > 0), ib)
    assert set(ia.tolist()) == {0, 2}


@pytest.mark.parametrize("seed", [170, 280, 457])
def test_criterion_ties_from_duplicated_targets_are_harmless(dev, seed):
    """SetCriterion on 5x one-to-many targets that went through jitter_targets and hold 1e-6-sized boxes (no jittered copy passes the IoU
    test, so their five rows are exact duplicates and the cost matrix has identical columns): the device assignment and the host (SciPy)
    one match the same queries but hand some of them different copies (asserted: the seeds were searched for it, most seeds give identical
    pairs; and wherever the two differ, the two target rows are bit-identical), yet every loss and both gradients agree.  The targets are
    drawn and jittered on the host (jitter_targets' elementwise path, torch's CPU generator), so the case does not depend on the device's
    random stream.  (Seeds 143, 161 and 489 also give differing pairs, but between two distinct 1e-6 boxes whose totals tie exactly in fp32:
    there the two optimal assignments are different sets of pairs, the losses need not agree, and the identical-rows assertion rejects them.)"""
    from spe_amd.models import conditional_detr as cd
    from spe_amd.models.matcher import HungarianMatcher
    g = torch.Generator().manual_seed(seed)
    L, B, Q, Kc = 3, 2, 50, 21
    outs = []
    for l in range(L):
        outs.append({"pred_logits": torch.randn(B, Q, Kc, generator=g).to(dev).requires_grad_(),
                     "pred_boxes": (torch.rand(B, Q, 4, generator=g) * 0.4 + 0.2).to(dev).requires_grad_()})
    outputs = dict(outs[0]); outputs["aux_outputs"] = outs[1:]
    targets = []
    for b in range(B):
        n = 5 + b
        lab = torch.randint(0, Kc, (n,), generator=g)
        il = torch.zeros(Kc, dtype=torch.int64); il[lab] = 1
        boxes = torch.rand(n, 4, generator=g) * 0.4 + 0.2
        boxes[:3, 2:] = 1e-6
        targets.append({"labels": lab, "boxes": boxes, "img_label": il})
    torch.manual_seed(31)
    tcp = cd.jitter_targets(targets, 5, 0.1)
    for b in range(B):
        tb = tcp[b]["boxes"].view(-1, 5, 4)
        assert tb.shape[0] == 5 + b and bool((tb[:3] == targets[b]["boxes"][:3, None]).all()), "the copies of a 1e-6 box are not exact duplicates"
        assert not bool((tb[3:, 0] == tb[3:, 4]).all(-1).any()), "an ordinary box kept no jittered copy"
    targets = [{k: v.to(dev) for k, v in t.items()} for t in targets]
    tcp = [{k: v.to(dev) for k, v in t.items()} for t in tcp]
    crit = cd.SetCriterion(Kc, HungarianMatcher(2.0, 5.0, 2.0, match_ratio=5), {"loss_ce": 2.0}, 0.25, ["labels", "boxes", "cardinality"], 2.0,
                           0.1).to(dev).eval()
    assert crit.hung_match_ratio == 5
    leaves = [o[k] for o in outs for k in ("pred_logits", "pred_boxes")]
    with torch.no_grad():               # the two assignments pair some duplicates differently
        lg, bx = (torch.stack([o[k] for o in outs]).detach() for k in ("pred_logits", "pred_boxes"))
        flat = crit.matcher.match_flat(lg, bx, tcp)
        host = crit.matcher.match_many(lg, bx, tcp)
        toff = cr.toff_of([len(t["labels"]) for t in tcp])
        hs = torch.cat([(l * B + b) * Q + host[l][b][0] for l in range(L) for b in range(B)])
        hg = torch.cat([toff[b] + host[l][b][1] for l in range(L) for b in range(B)])
        ds, dg = flat[0].cpu(), flat[1].cpu()
        assert torch.equal(ds, hs), "the two assignments match different queries: more than a permutation of duplicates"
        differ = dg != hg
        print("CRITERION criterion_ties pairs in which device and host assignment differ:", int(differ.sum()), "of", hg.numel())
        assert int(differ.sum()) > 0, "both assignments pair the duplicates alike: the case no longer shows that a different pairing is harmless"
        tbox = torch.cat([t["boxes"] for t in tcp]).cpu()
        tlab = torch.cat([t["labels"] for t in tcp]).cpu()
        assert torch.equal(_bits(tbox[dg[differ]]), _bits(tbox[hg[differ]])) and torch.equal(tlab[dg[differ]], tlab[hg[differ]]), \
            "a query got two different targets: a tie between distinct targets, not between copies"

    def run():
        losses = crit(outputs, targets, targets_cp=tcp)
        total = sum(v for k, v in losses.items() if v.requires_grad)
        return losses, torch.autograd.grad(total, leaves)
    a, ga = run()
    orig = HungarianMatcher.match_flat
    try:
        HungarianMatcher.match_flat = lambda self, *args: None
        b_, gb = run()
    finally:
        HungarianMatcher.match_flat = orig
    assert set(a) == set(b_) and any(k.startswith("loss_giou") for k in a)
    for k in a:
        assert torch.allclose(a[k], b_[k], rtol=1e-6, atol=1e-7), (k, a[k], b_[k])
    for x, y in zip(ga, gb):
        assert float(x.abs().max()) > 0 and torch.allclose(x, y, rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------------------------------------------------------------------------
# focal loss
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", cc.FOCAL_FAMILIES)
@pytest.mark.parametrize("L,R,Kc", cc.FOCAL_SHAPES)
def test_focal(dev, L, R, Kc, fam):
    from spe_amd import kernels as K
    x, tclass, roww = cc.focal_inputs(L, R, Kc, fam)
    xd, td, wd = x.to(dev), tclass.to(dev), roww.to(dev)
    for rw, rwd in ((None, None), (roww, wd)):
        for alpha, gamma in cc.FOCAL_PARAMS:
            rl, rg, ra = cr.focal_ref(x, tclass, rw, alpha, gamma)
            runs = []
            for _ in range(2):           # tickets reset, fixed order: the second launch gives the same bits
                grad, amax = _filled(L * R * Kc, torch.float32, dev), _filled(L * R, torch.int32, dev)
                loss = _filled(L, torch.float32, dev)
                loss[:L] = 0            # the kernel accumulates into it
                K.lib.call("spe_focal_loss", xd.data_ptr(), td.data_ptr(), _p(rwd), grad.data_ptr(), loss.data_ptr(), amax.data_ptr(), L, R, Kc,
                           alpha, gamma, K._st())
                _check_stores("grad", grad, L * R * Kc)
                _check_stores("argmax", amax, L * R)
                assert _untouched(loss[L:])
                runs.append((loss[:L].cpu(), grad[:L * R * Kc].cpu().view(L, R, Kc), amax[:L * R].cpu().view(L, R)))
            (loss, grad, amax), again = runs
            assert torch.equal(_bits(loss), _bits(again[0])) and torch.equal(_bits(grad), _bits(again[1])), "two launches, two results"
            assert torch.equal(amax.long(), ra), "argmax (lowest index among equal maxima)"
            gerr = (grad.double() - rg).abs()
            figs = {"loss": cr.rel(loss, rl), "grad": cr.rel(grad, rg), "grad/bound": float((gerr / cr.focal_grad_tol(rg)).max())}
            _note("focal", fam, **figs)
            tag = f"L{L} R{R} Kc{Kc} {fam} roww{int(rw is not None)} alpha{alpha:g} gamma{gamma:g}"
            print("CRITERION focal", tag, " ".join(f"{k} {v:.3e}" for k, v in figs.items()))
            assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all()), tag
            assert figs["loss"] < 1e-5, (tag, figs)
            if fam == "saturated":
                assert figs["grad/bound"] <= 1.0, (tag, figs)
            else:
                assert figs["grad"] < 1e-4, (tag, figs)


# ------------------------------------------------------------------------------------------------------------------------------
# box losses
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", cc.BOX_FAMILIES)
@pytest.mark.parametrize("n,L", cc.BOX_CASES)
def test_box_loss(dev, n, L, fam):
    from spe_amd import kernels as K
    pred, srow, tbox, w, lidx = cc.box_inputs(n, L, fam)
    pd, sd, td, wd, ld = (t.to(dev).contiguous() for t in (pred, srow, tbox, w, lidx))
    pre = (0.5 + 0.125 * (torch.arange(2 * L) % 8)).view(L, 2)             # sums accumulates: a known non-zero start
    for wt, wtd in ((None, None), (w, wd)):
        rs, r1, r2 = cr.box_loss_ref(pred, srow, tbox, wt, lidx, L)
        sums = _filled(2 * L, torch.float32, dev)
        sums[:2 * L] = pre.reshape(-1).to(dev)
        g1, g2 = _filled(n * 4, torch.float32, dev), _filled(n * 4, torch.float32, dev)
        K.lib.call("spe_box_loss", pd.data_ptr(), sd.data_ptr(), td.data_ptr(), _p(wtd), ld.data_ptr(), sums.data_ptr(), g1.data_ptr(),
                   g2.data_ptr(), n, L, K._st())
        _check_stores("g_l1", g1, n * 4)
        _check_stores("g_giou", g2, n * 4)
        assert _untouched(sums[2 * L:])
        got = sums[:2 * L].cpu().view(L, 2)
        g1, g2 = g1[:n * 4].cpu().view(n, 4), g2[:n * 4].cpu().view(n, 4)
        empty = torch.ones(L, dtype=torch.bool)
        empty[lidx.long()] = False
        assert L == 1 or bool(empty.any())
        assert torch.equal(got[empty], pre[empty]), "a layer without pairs changed its sum"
        figs = {"sums": cr.rel(got, pre.double() + rs), "sums-pre": cr.rel(got.double() - pre.double(), rs), "g_l1": cr.rel(g1, r1),
                "g_giou": cr.rel(g2, r2)}
        _note("box_loss", fam, **figs)
        tag = f"n{n} L{L} {fam} w{int(wt is not None)}"
        print("CRITERION box_loss", tag, " ".join(f"{k} {v:.3e}" for k, v in figs.items()))
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(g2).all()), tag
        assert figs["sums"] < 1e-5 and figs["sums-pre"] < 1e-5 and figs["g_l1"] < 1e-6 and figs["g_giou"] < 1e-4, (tag, figs)
        if fam == "dyadic":
            assert torch.equal(g1.double(), r1), (tag, "g_l1 is +-w or 0 exactly")


@pytest.mark.parametrize("n", cc.BWD_N)
def test_box_loss_bwd_scatter(dev, n):
    from spe_amd import kernels as K
    srow, lidx, g1, g2, c1, c2, P = cc.bwd_inputs(n)
    ref = cr.box_loss_bwd_ref(srow, lidx, g1, g2, c1, c2, (P, 4))
    dpred = _filled(P * 4, torch.float32, dev)
    dpred[:P * 4] = 0                    # an accumulating scatter
    args = [t.to(dev).contiguous() for t in (srow, lidx, g1, g2, c1, c2)]
    K.lib.call("spe_box_loss_bwd", *[t.data_ptr() for t in args], dpred.data_ptr(), n, K._st())
    assert _untouched(dpred[P * 4:])
    got = dpred[:P * 4].cpu().view(P, 4)
    hit = torch.zeros(P, dtype=torch.bool)
    hit[srow] = True
    assert bool((got[~hit] == 0).all()), "a row nobody matched received a gradient"
    fig = cr.rel(got, ref)
    _note("box_loss_bwd", "-", scatter=fig)
    print("CRITERION box_loss_bwd", f"n{n} rel {fig:.3e}")
    assert fig < 1e-4
    if n >= 3:                          # the row matched three times, on its own
        r = int(srow[0])
        assert cr.rel(got[r], ref[r]) < 1e-4 and float(ref[r].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------------------
# matcher cost
# ------------------------------------------------------------------------------------------------------------------------------
def _run_cost(K, case, tensors, dev):
    L, B, Q, Kc, sizes = case
    logits, boxes, ids, tb = tensors
    total = sum(sizes)
    n = L * Q * total
    toff = torch.tensor(cr.toff_of(sizes), dtype=torch.int32, device=dev)
    cost = _filled(n, torch.float32, dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    dv = [t.to(dev).contiguous() for t in (logits, boxes, ids, tb)]
    K.lib.call("spe_matcher_cost", *[t.data_ptr() for t in dv], toff.data_ptr(), total, cost.data_ptr(), err.data_ptr(), L, B, Q, Kc,
               *cc.COST_WEIGHTS, K._st())
    _check_stores("cost", cost, n)
    return cost[:n].cpu().view(L, Q * total), int(err.item())


@pytest.mark.parametrize("fam", list(cc.COST_FAMILIES))
@pytest.mark.parametrize("case", cc.COST_CASES, ids=lambda c: "L%d-B%d-Q%d-Kc%d" % c[:4])
def test_matcher_cost(dev, case, fam):
    from spe_amd import kernels as K
    L, B, Q, Kc, sizes = case
    tensors = cc.cost_inputs(case, fam)
    got, flag = _run_cost(K, case, tensors, dev)
    assert flag == 0 and bool(torch.isfinite(got).all())
    c64, xs = cr.matcher_cost_ref(*tensors, sizes, *cc.COST_WEIGHTS)
    c32, _ = cr.matcher_cost_ref(*tensors, sizes, *cc.COST_WEIGHTS, dtype=torch.float32)
    tol = cr.matcher_cost_tol(xs, *cc.COST_WEIGHTS)
    ratio, ratio32 = (got.double() - c64).abs() / tol, (c32.double() - c64).abs() / tol
    toff = cr.toff_of(sizes)
    for l in range(L):
        for b in range(B):             # block by block: which image went wrong, should one
            blk = ratio[l, Q * toff[b]:Q * toff[b + 1]]
            assert blk.numel() == 0 or float(blk.max()) < 1.0, (l, b, float(blk.max()))
    figs = {"kernel error/bound": float(ratio.max()), "fp32 composition error/bound": float(ratio32.max()),
            "kernel max abs error": float((got.double() - c64).abs().max())}
    _note("matcher_cost", fam, **figs)
    print("CRITERION matcher_cost", "L%d B%d Q%d Kc%d" % case[:4], fam, " ".join(f"{k} {v:.3e}" for k, v in figs.items()))


def test_matcher_cost_degenerate_boxes_raise_bit0_only(dev):
    from spe_amd import kernels as K
    case, tensors = cc.cost_degenerate_inputs()
    got, flag = _run_cost(K, case, tensors, dev)
    assert flag == 1, flag
    assert bool(torch.isfinite(got).all())


# ------------------------------------------------------------------------------------------------------------------------------
# NMS, jitter
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cc.NMS_N)
def test_nms_sorted(dev, n):
    from spe_amd import kernels as K
    boxes, labels, _, counts = cc.nms_inputs(n)
    bd, ld = boxes.to(dev).contiguous(), labels.to(dev).contiguous()
    I = cc.NMS_IMAGES
    for cnt in (None, counts):
        cd_ = None if cnt is None else torch.tensor(cnt, dtype=torch.int32, device=dev)
        keep = _filled(I * n, torch.uint8, dev)
        K.lib.call("spe_nms_sorted", bd.data_ptr(), ld.data_ptr(), _p(cd_), keep.data_ptr(), I, n, cc.NMS_THR, K._st())
        _check_stores("keep", keep, I * n)
        got = keep[:I * n].cpu().view(I, n)
        assert int(got.max()) <= 1
        want = torch.stack([cr.greedy_nms_ref(boxes[i], labels[i], cc.NMS_THR, None if cnt is None else cnt[i]) for i in range(I)])
        kept = int(want.sum())
        print("CRITERION nms", f"n{n} counts {cnt} kept {kept} differing {int((got.bool() != want).sum())}")
        _note("nms", "-", differing_flags=int((got.bool() != want).sum()))
        assert torch.equal(got.bool(), want), (n, cnt)
        if cnt is not None:
            assert not bool(got[1].any()) and not bool(got[2, n // 2:].any())


@pytest.mark.parametrize("M,ncand,ratio", cc.JITTER_CASES)
def test_jitter_pick(dev, M, ncand, ratio):
    from spe_amd import kernels as K
    box, scale = cc.jitter_inputs(M, ncand, ratio)
    want = cr.jitter_pick_ref(box, scale, ratio)
    bd, sd = box.to(dev).contiguous(), scale.to(dev).contiguous()
    assert sd.data_ptr() % 16 == 0
    out = _filled(M * ratio * 4, torch.float32, dev)
    K.lib.call("spe_jitter_pick", bd.data_ptr(), sd.data_ptr(), out.data_ptr(), M, ncand, ratio, K._st())
    _check_stores("out", out, M * ratio * 4)
    got = out[:M * ratio * 4].cpu().view(M, ratio, 4)
    _note("jitter_pick", "-", differing_boxes=int((_bits(got) != _bits(want)).any(-1).sum()))
    assert torch.equal(_bits(got), _bits(want)), (M, ncand, ratio)


# ------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_alone(dev):
    from spe_amd import kernels as K
    from spe_amd.lib import SpeLibraryError
    # Q = 1025
    Q = 1025
    cost = torch.randn(1, Q * 2, device=dev)
    toff = torch.tensor([0, 2], dtype=torch.int32, device=dev)
    srow, gidx, lidx = _filled(2, torch.int64, dev), _filled(2, torch.int64, dev), _filled(2, torch.int32, dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(SpeLibraryError):
        K.lib.call("spe_hungarian", cost.data_ptr(), toff.data_ptr(), srow.data_ptr(), gidx.data_ptr(), lidx.data_ptr(), err.data_ptr(),
                   1, 1, Q, K._st())
    torch.cuda.synchronize()
    assert _untouched(srow) and _untouched(gidx) and _untouched(lidx) and int(err.item()) == 0
    # L = 513
    pred, srw, tbox, w, li = (t.to(dev).contiguous() for t in cc.box_inputs(600, 512, "plain"))
    sums, g1, g2 = _filled(2 * cc.BOX_L_REFUSED, torch.float32, dev), _filled(2400, torch.float32, dev), _filled(2400, torch.float32, dev)
    with pytest.raises(SpeLibraryError):
        K.lib.call("spe_box_loss", pred.data_ptr(), srw.data_ptr(), tbox.data_ptr(), w.data_ptr(), li.data_ptr(), sums.data_ptr(),
                   g1.data_ptr(), g2.data_ptr(), 600, cc.BOX_L_REFUSED, K._st())
    torch.cuda.synchronize()
    assert _untouched(sums) and _untouched(g1) and _untouched(g2)
    # nmax = 4097
    n = cc.NMS_REFUSED
    boxes = torch.rand(1, n, 4, device=dev)
    labels = torch.zeros(1, n, dtype=torch.int64, device=dev)
    keep = _filled(n, torch.uint8, dev)
    with pytest.raises(SpeLibraryError):
        K.lib.call("spe_nms_sorted", boxes.data_ptr(), labels.data_ptr(), None, keep.data_ptr(), 1, n, cc.NMS_THR, K._st())
    torch.cuda.synchronize()
    assert _untouched(keep)
    # scale one float behind a 16-byte boundary
    box, scale = cc.jitter_inputs(9, 64, 5)
    buf = torch.zeros(scale.numel() + 4, device=dev)
    assert buf.data_ptr() % 16 == 0
    sc = buf[1:1 + scale.numel()].copy_(scale.reshape(-1).to(dev))
    assert sc.data_ptr() % 16 == 4
    out = _filled(9 * 5 * 4, torch.float32, dev)
    bd = box.to(dev)
    with pytest.raises(SpeLibraryError):
        K.lib.call("spe_jitter_pick", bd.data_ptr(), sc.data_ptr(), out.data_ptr(), 9, 64, 5, K._st())
    torch.cuda.synchronize()
    assert _untouched(out)
    sc2 = sc.clone()                    # the same call is taken once the pointer is aligned
    assert sc2.data_ptr() % 16 == 0
    K.lib.call("spe_jitter_pick", bd.data_ptr(), sc2.data_ptr(), out.data_ptr(), 9, 64, 5, K._st())
    assert torch.equal(_bits(out[:180].cpu().view(9, 5, 4)), _bits(cr.jitter_pick_ref(box, scale, 5)))


def test_zz_record(dev):
    """Last in the file: the maxima of everything above, one line per kernel and family, and the module's run time."""
    for (kernel, fam), figs in sorted(FIGS.items()):
        print("CRITERION max", kernel, fam, " ".join(f"{k} {v:.3e}" for k, v in figs.items()))
    print(f"CRITERION module wall time {time.perf_counter() - T0:.1f} s")
