"""The VOC metric kernels (csrc/voc_eval.hip) on the device against the fp64 numpy restatement (tests/voc_eval_ref.py) and the recorded
results of the reference's evaluator (tests/golden/voc_eval_*.pt).

spe_voc_match and spe_voc_ap are called through the C ABI on buffers this file owns: longer than needed by a guard band and pre-filled
with a sentinel, so an entry that was not written, or one written past the end, shows.  The kernels restate numpy's fp64 arithmetic
without FMA contraction, so the equalities are those of tests/test_voc_meter_cpu.py: flags, fp64 scores, the integer counters, rec,
prec and AP07 bitwise (NaN matching NaN); area AP within nd * 2^-52 (two summation orders of <= nd terms with partial sums <= 1)."""
import functools

import numpy as np
import pytest
import torch

import voc_eval_cases as cases
import voc_eval_ref as R
from voc_eval_cases import as_numpy, check_against, load_golden, run_meter, same

pytestmark = pytest.mark.gpu

GUARD, FLAG_FILL, SCORE_FILL, COUNT_BASE = 64, 0xAB, -7.25, 1000


@functools.lru_cache(maxsize=None)
def case_and_ref(name, integer_dets, roundtrip):
    """(C, images, per-image match_image results): computed once per case, shared, never written to."""
    C, images = cases.match_case(name, integer_dets=integer_dets)
    return C, images, [R.match_image(im, C, 0.5, roundtrip) for im in images]


def call_match(dev, C, images, roundtrip, max_det=None, max_gt=None, expect=0, ovthresh=0.5):
    """spe_voc_match through the C ABI -> (flags, scores, counters [3, C]) as numpy, guard bands checked."""
    from spe_amd import kernels as K, lib
    cat = lambda k, dt: torch.from_numpy(np.concatenate([np.asarray(im[k]).reshape((-1, 4) if "boxes" in k else -1) for im in images])
                                         ).to(dev, dt).contiguous()
    nd, ng = [im["scores"].size for im in images], [im["gt_labels"].size for im in images]
    off = lambda n: torch.tensor(np.concatenate(([0], np.cumsum(n))), dtype=torch.int32, device=dev)
    args = [cat("boxes", torch.float32), cat("scores", torch.float32), cat("labels", torch.int64), off(nd),
            cat("gt_boxes", torch.float64), cat("gt_labels", torch.int64), cat("difficult", torch.uint8), off(ng)]
    flags = torch.full((sum(nd) + GUARD,), FLAG_FILL, dtype=torch.uint8, device=dev)
    scores = torch.full((sum(nd) + GUARD,), SCORE_FILL, dtype=torch.float64, device=dev)
    cnt = (COUNT_BASE + torch.arange(3 * (C + 8), dtype=torch.int32, device=dev)).view(3, C + 8).contiguous()
    ss, cs = (1000.0, 10.0) if roundtrip else (0.0, 0.0)
    f = getattr(lib.load(), "spe_voc_match")
    rc = f(*[a.data_ptr() for a in args], len(images), C, max(nd) if max_det is None else max_det, max(ng) if max_gt is None else max_gt,
           ovthresh, ss, cs, flags.data_ptr(), scores.data_ptr(), cnt[0].data_ptr(), cnt[1].data_ptr(), cnt[2].data_ptr(), K._st())
    torch.cuda.synchronize()
    assert rc == expect, rc
    flags, scores, cnt = flags.cpu().numpy(), scores.cpu().numpy(), cnt.cpu().numpy()
    n = sum(nd)
    assert (flags[n:] == FLAG_FILL).all() and (scores[n:] == SCORE_FILL).all(), "written past the end"
    base = COUNT_BASE + np.arange(3 * (C + 8)).reshape(3, C + 8)
    assert (cnt[:, C:] == base[:, C:]).all(), "counter written past num_classes"
    return flags[:n], scores[:n], (cnt - base)[:, :C]


@pytest.mark.parametrize("roundtrip", [True, False])
@pytest.mark.parametrize("integer_dets", [False, True])
@pytest.mark.parametrize("name", list(cases.MATCH_CASES))
def test_match_c_abi(dev, name, integer_dets, roundtrip):
    C, images, ref = case_and_ref(name, integer_dets, roundtrip)
    flags, scores, cnt = call_match(dev, C, images, roundtrip)
    assert not (flags == FLAG_FILL).any() and not (scores == SCORE_FILL).any(), "an entry was not written"
    assert same(flags, np.concatenate([r[0] for r in ref]))
    assert same(scores.view(np.int64), np.concatenate([r[1] for r in ref]).view(np.int64))
    for k in range(3):
        assert same(cnt[k], sum(r[2 + k] for r in ref)), ("npos", "nimgs", "hits")[k]


@pytest.mark.parametrize("roundtrip", [True, False])
@pytest.mark.parametrize("name", list(cases.MATCH_CASES))
def test_match_through_meter(dev, name, roundtrip):
    C, images, _ = case_and_ref(name, False, roundtrip)
    ref = meter_ref(name, roundtrip)
    out = run_meter(images, C, device=dev, file_roundtrip=roundtrip).summarize(return_curves=True)
    check_against(out, ref, C)
    assert same(out["npos"], ref["npos"]) and same(out["nimgs"], ref["nimgs"])
    one_by_one = run_meter(images, C, [[i] for i in range(len(images))][::-1], device=dev, file_roundtrip=roundtrip)
    check_against(one_by_one.summarize(return_curves=True), ref, C)


@functools.lru_cache(maxsize=None)
def meter_ref(name, roundtrip):
    C, images, _ = case_and_ref(name, False, roundtrip)
    return R.evaluate(images, C, 0.5, roundtrip)


def test_overlap_bits_and_strict_threshold(dev):
    """The device overlap is numpy's, bit for bit, and the test against it is strict: for pairs whose widths are decimal fractions
    (ground truth here too, so that every product of the formula rounds and a contracted multiply-add lands on another double) a threshold set to the numpy
    overlap itself leaves a false positive, the double just below it gives a true positive."""
    rng = np.random.default_rng(314)
    for k in range(64):
        gt = np.round(np.array([[40, 30, 40 + rng.uniform(30, 200), 30 + rng.uniform(30, 200)]]) + rng.uniform(0, 1, 4), 1)
        det = (gt[0] - 1 + rng.uniform(-9, 9, 4)).astype(np.float32)[None]
        im = {"boxes": det, "scores": np.array([0.5], np.float32), "labels": np.array([1]), "gt_boxes": gt, "gt_labels": np.array([1]),
              "difficult": np.array([False]), "image_id": k}
        ov = float(R.overlaps(R.quantise(im["scores"], det, True)[1][0], gt.astype(np.float64))[0])
        assert 0.3 < ov < 1.0
        at, below = (call_match(dev, 1, [im], True, ovthresh=th)[0].tolist() for th in (ov, np.nextafter(ov, 0.0)))
        assert (at, below) == ([2], [1]), (k, ov, at, below)


def _big_image(n_det, n_gt):
    rng = np.random.default_rng([n_det, n_gt])
    return cases.make_image(rng, 1, [n_gt], [n_det], label_noise=False)


def test_match_limits(dev):
    """4096 detections and 1024 ground-truth boxes in one image are accepted (and right); one more of either is refused with -2 and
    nothing is written.  One class: one wave walks all 4096 x 1024 pairs."""
    im = _big_image(cases.MAX_DET, cases.MAX_GT)
    flags, scores, cnt = call_match(dev, 1, [im], True)
    rf, rs, a, b, h = R.match_image(im, 1, 0.5, True)
    assert same(flags, rf) and same(scores.view(np.int64), rs.view(np.int64))
    assert same(cnt, np.stack([a, b, h]))
    for nd, ng in ((cases.MAX_DET + 1, 3), (3, cases.MAX_GT + 1)):
        flags, scores, cnt = call_match(dev, 1, [_big_image(nd, ng)], True, expect=-2)
        assert (flags == FLAG_FILL).all() and (scores == SCORE_FILL).all() and (cnt == 0).all()
    # a caller that understates the counts: the kernel skips the image instead of overrunning its LDS
    flags, scores, cnt = call_match(dev, 1, [_big_image(3, cases.MAX_GT + 1)], True, max_gt=cases.MAX_GT)
    assert (flags == FLAG_FILL).all() and (cnt == 0).all()
    from spe_amd.lib import SpeLibraryError
    with pytest.raises((SpeLibraryError, ValueError)):
        run_meter([_big_image(cases.MAX_DET + 1, 3)], 1, device=dev)


def call_ap(dev, flags, seg, npos, curves):
    from spe_amd import kernels as K, lib
    C, n = npos.size, flags.size
    fl = torch.from_numpy(flags).to(dev)
    so, npd = torch.from_numpy(seg).to(dev), torch.from_numpy(npos).to(dev)
    ap = torch.full((2, C + GUARD), SCORE_FILL, dtype=torch.float64, device=dev)
    rp = torch.full((2, n + GUARD), SCORE_FILL, dtype=torch.float64, device=dev)
    lib.call("spe_voc_ap", fl.data_ptr(), so.data_ptr(), npd.data_ptr(), C, ap[0].data_ptr(), ap[1].data_ptr(),
             rp[0].data_ptr() if curves else None, rp[1].data_ptr() if curves else None, K._st())
    ap, rp = ap.cpu().numpy(), rp.cpu().numpy()
    assert (ap[:, C:] == SCORE_FILL).all() and (rp[:, n:] == SCORE_FILL).all(), "written past the end"
    if not curves:
        assert (rp == SCORE_FILL).all()
    return ap[0, :C], ap[1, :C], rp[0, :n], rp[1, :n]


@functools.lru_cache(maxsize=None)
def streams_and_ref():
    flags, seg, npos = cases.ap_streams()
    ref = []
    for c in range(npos.size):
        rec, prec = R.curve(flags[seg[c]:seg[c + 1]], npos[c])
        ref.append((rec, prec, R.ap07(rec, prec), R.ap_area(rec, prec)))
    return flags, seg, npos, ref


def test_ap_streams_cover_the_cases():
    flags, seg, npos, _ = streams_and_ref()
    nd = np.diff(seg)
    assert set(nd.tolist()) == set(cases.AP_ND) and set(npos.tolist()) >= {0, 1} and npos.max() > 1
    kinds = set()
    for c in range(npos.size):
        f = set(flags[seg[c]:seg[c + 1]].tolist())
        kinds.add("random" if len(f) > 1 else {1: "tp", 2: "fp", 0: "ignored"}[f.pop()] if f else "empty")
    assert kinds >= {"tp", "fp", "ignored", "random"}


@pytest.mark.parametrize("curves", [True, False])
def test_ap_streams(dev, curves):
    flags, seg, npos, ref = streams_and_ref()
    ap07, area, rec, prec = call_ap(dev, flags, seg, npos, curves)
    for c in range(npos.size):
        s, e = seg[c], seg[c + 1]
        r_rec, r_prec, r07, r_area = ref[c]
        if curves:
            assert same(rec[s:e], r_rec) and same(prec[s:e], r_prec), c
        assert same(ap07[c], r07), (c, ap07[c], r07)
        assert (np.isnan(area[c]) and np.isnan(r_area)) or abs(area[c] - r_area) <= (e - s) * 2.0 ** -52, (c, area[c], r_area)


@pytest.mark.parametrize("name", cases.GOLDENS)
def test_golden_on_device(dev, name):
    g = load_golden(name)
    C, images = g["num_classes"], g["images"]
    out = run_meter(images, C, device=dev, ovthresh=g["ovthresh"]).summarize(return_curves=True)
    ref = R.evaluate(as_numpy(images), C, g["ovthresh"], True)
    check_against(out, {**{k: g[k] for k in ("rec", "prec", "ap07", "ap_area", "corloc")}, "flags": ref["flags"]}, C)
    assert same(out["npos"], ref["npos"]) and same(out["nimgs"], ref["nimgs"])


def test_two_runs_bitwise_equal(dev):
    C, images, _ = case_and_ref("three_images", False, True)
    runs = [run_meter(images, C, device=dev).summarize(return_curves=True) for _ in range(2)]
    bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t
    for k in ("ap07", "ap_area", "corloc", "npos", "nimgs"):
        assert torch.equal(bits(runs[0][k]), bits(runs[1][k])), k
    for k in ("rec", "prec", "flags"):
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(runs[0][k], runs[1][k])), k


def test_update_does_not_synchronise(dev):
    """update() reads no device data on the host: under torch's sync debug mode any .item() / .cpu() / nonzero would raise."""
    C, images, _ = case_and_ref("two_images_shifted", False, True)
    res, gts = cases.split(images, dev)
    from spe_amd.evalmetrics import VOCDetectionMeter
    m = VOCDetectionMeter(num_classes=C)
    m.update(res[:1], gts[:1])                         # first call: allocations, library load
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.update(res[1:], gts[1:])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    check_against(m.summarize(return_curves=True), meter_ref("two_images_shifted", True), C)
