"""The COCO metric kernels (csrc/coco_eval.hip) on the device against the restatement of COCOeval in tests/coco_eval_ref.py.

spe_coco_match and spe_coco_accumulate are called through the C ABI on buffers this file owns: longer than needed by a guard band and
pre-filled with a sentinel, so an entry that was not written, or one written past the end, shows.  Flag words, ranks, npig, precision,
recall and scores are compared exactly: the kernels take integer counts and correctly rounded fp64 operations in the restatement's
order, without FMA contraction, so there is no tolerance to state."""
import functools

import numpy as np
import pytest
import torch

import coco_eval_cases as cases
import coco_eval_ref as R
from coco_eval_cases import check_against, run_meter, same

pytestmark = pytest.mark.gpu

GUARD, RANK_FILL, WORD_FILL, COUNT_BASE, TABLE_FILL = 64, -77, 0x5A5A5A5A, 1000, -7.25
P = R.params()


def prepare(images, cat_ids):
    """What update() hands the kernel, built with numpy: labels -> category index (len(cat_ids) for unknown ids), detections of an image
    ordered by (index, score descending, incoming).  -> per image (order, dict of arrays)."""
    K = len(cat_ids)
    index = lambda lab: np.array([cat_ids.index(int(x)) if int(x) in cat_ids else K for x in lab], np.int64)
    out = []
    for im in images:
        cat = index(im["labels"])
        o = np.argsort(-im["scores"].astype(np.float64), kind="mergesort")
        o = o[np.argsort(cat[o], kind="mergesort")]
        out.append((o, {"boxes": im["boxes"][o], "cats": cat[o], "gt_boxes": im["gt_boxes"], "gt_cats": index(im["gt_labels"]),
                        "iscrowd": im["iscrowd"], "area": im["area"]}))
    return out


@functools.lru_cache(maxsize=None)
def case_and_ref(name):
    """(cat_ids, images, prepared inputs, per-image match_image results in the prepared order): once per case, shared, read-only."""
    cat_ids, images = cases.case(name)
    prep = prepare(images, cat_ids)
    ref = []
    for im, (o, _) in zip(images, prep):
        rank, words, npig = R.match_image(im, cat_ids)
        ref.append((rank[o], words[o], npig))
    return cat_ids, images, prep, ref


def call_match(dev, K, prep, max_det=None, max_gt=None, expect=0, iou_thrs=None):
    """spe_coco_match through the C ABI -> (rank, words, npig [K,4]) as numpy, guard bands checked."""
    from spe_amd import kernels as Kn, lib
    cat = lambda k, dt, w=None: torch.from_numpy(np.concatenate([np.asarray(p[k]).reshape((-1, w) if w else -1) for _, p in prep])
                                                 ).to(dev, dt).contiguous()
    nd, ng = [p["cats"].size for _, p in prep], [p["gt_cats"].size for _, p in prep]
    off = lambda n: torch.tensor(np.concatenate(([0], np.cumsum(n))), dtype=torch.int32, device=dev)
    thr = torch.from_numpy(np.asarray(P["iouThrs"] if iou_thrs is None else iou_thrs, np.float64)).to(dev)
    rng = torch.from_numpy(np.asarray(P["areaRng"], np.float64).reshape(-1)).to(dev)
    args = [cat("boxes", torch.float32, 4), cat("cats", torch.int64), off(nd), cat("gt_boxes", torch.float64, 4), cat("gt_cats", torch.int64),
            cat("iscrowd", torch.uint8), cat("area", torch.float64), off(ng), thr, rng]
    n = sum(nd)
    rank = torch.full((n + GUARD,), RANK_FILL, dtype=torch.int32, device=dev)
    words = torch.full((n + GUARD, 4), WORD_FILL, dtype=torch.int32, device=dev)
    cnt = (COUNT_BASE + torch.arange((K + 8) * 4, dtype=torch.int32, device=dev)).view(K + 8, 4).contiguous()
    f = getattr(lib.load(), "spe_coco_match")
    rc = f(*[a.data_ptr() for a in args], len(prep), K, max(nd) if max_det is None else max_det, max(ng) if max_gt is None else max_gt,
           P["maxDets"][-1], rank.data_ptr(), words.data_ptr(), cnt.data_ptr(), Kn._st())
    torch.cuda.synchronize()
    assert rc == expect, rc
    rank, words, cnt = rank.cpu().numpy(), words.cpu().numpy(), cnt.cpu().numpy()
    assert (rank[n:] == RANK_FILL).all() and (words[n:] == WORD_FILL).all(), "written past the end"
    base = COUNT_BASE + np.arange((K + 8) * 4).reshape(K + 8, 4)
    assert (cnt[K:] == base[K:]).all(), "counter written past num_cats"
    return rank[:n], words[:n], (cnt - base)[:K]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_match_c_abi(dev, name):
    cat_ids, _, prep, ref = case_and_ref(name)
    rank, words, npig = call_match(dev, len(cat_ids), prep)
    assert not (rank == RANK_FILL).any() and not (words == WORD_FILL).any(), "an entry was not written"
    assert same(rank, np.concatenate([r[0] for r in ref]))
    assert same(words, np.concatenate([r[1] for r in ref]))
    assert same(npig, sum(r[2] for r in ref))


def test_cases_cover_the_match_edges():
    """What the named cases are there for, checked on the restatement's results (no device needed for the claim itself)."""
    cat_ids, images, prep, ref = case_and_ref("counts")
    assert tuple(np.bincount(prep[0][1]["cats"])) == cases.DET_COUNTS
    assert sorted(set(ref[0][0].tolist())) == list(range(-1, 100))                # ranks 0 .. 99 and the dropped mark
    cat_ids, images, prep, ref = case_and_ref("presence")
    have = {(bool((p["cats"] == k).any()), bool((p["gt_cats"] == k).any())) for _, p in prep for k in range(len(cat_ids))}
    assert have == {(True, False), (False, True), (False, False), (True, True)}
    cat_ids, images, prep, ref = case_and_ref("random_small")
    assert any((p["cats"] == len(cat_ids)).any() for _, p in prep) and any((p["gt_cats"] == len(cat_ids)).any() for _, p in prep)


def test_match_limits(dev):
    """512 ground-truth boxes in one image are accepted (and right: the IoU pass takes eight lane strides); one more, or one detection
    more than 4096, is refused with -2 and nothing is written."""
    im = cases.big_image(20, cases.MAX_GT)
    prep = prepare([im], [1])
    rank, words, npig = call_match(dev, 1, prep)
    r_rank, r_words, r_npig = R.match_image(im, [1])
    o = prep[0][0]
    assert same(rank, r_rank[o]) and same(words, r_words[o]) and same(npig, r_npig)
    for nd, ng in ((cases.MAX_DET + 1, 3), (3, cases.MAX_GT + 1)):
        rank, words, npig = call_match(dev, 1, prepare([cases.big_image(nd, ng)], [1]), expect=-2)
        assert (rank == RANK_FILL).all() and (words == WORD_FILL).all() and (npig == 0).all()
    # a caller that understates the counts: the kernel skips the image instead of overrunning its LDS
    rank, words, npig = call_match(dev, 1, prepare([cases.big_image(3, cases.MAX_GT + 1)], [1]), max_gt=cases.MAX_GT)
    assert (rank == RANK_FILL).all() and (npig == 0).all()
    from spe_amd.lib import SpeLibraryError
    with pytest.raises((SpeLibraryError, ValueError)):
        run_meter([cases.big_image(3, cases.MAX_GT + 1)], [1], device=dev)


def test_iou_bits_and_threshold_equality(dev):
    """The device IoU is the restatement's, bit for bit, and `iou < t` is the test: with ground truth whose sides are decimal fractions
    (so that G.w * G.h rounds and a contracted multiply-add would land on another double), a threshold equal to the host's IoU matches,
    the double just above it does not, the double just below it does."""
    rng = np.random.default_rng(2718)
    for k in range(64):
        g = np.round(np.concatenate([rng.uniform(20, 60, 2), rng.uniform(30, 200, 2)]), 1)
        d = np.array([g[0], g[1], g[0] + g[2], g[1] + g[3]]) + rng.uniform(-9, 9, 4)
        im = cases.image(k, [(d.tolist(), .5, 1)], [(g.tolist(), 1, 0, 40. ** 2)])
        ov = R.iou(R.to_xywh(im["boxes"])[0], im["gt_boxes"][0], False)
        assert 0.3 < ov < 1 - 1e-9
        thrs = [ov, np.nextafter(ov, 2.0), np.nextafter(ov, 0.0)] + [2.0] * 7
        _, words, _ = call_match(dev, 1, prepare([im], [1]), iou_thrs=thrs)
        assert (words[0] & 0x3ff).tolist() == [0b101] * 4, (k, ov, words)       # every area range walks the box, ignored or not


def call_accumulate(dev, words, rank, score, seg, npig):
    from spe_amd import kernels as Kn, lib
    K, R_, M = npig.shape[0], P["recThrs"].size, len(P["maxDets"])
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    n_pr, n_rc = cases.T * R_ * K * cases.A * M, cases.T * K * cases.A * M
    pr = torch.full((2, n_pr + GUARD), TABLE_FILL, dtype=torch.float64, device=dev)
    rc = torch.full((n_rc + GUARD,), TABLE_FILL, dtype=torch.float64, device=dev)
    args = [t(words), t(rank), t(score), t(seg), t(npig), torch.tensor(P["maxDets"], dtype=torch.int32, device=dev), t(P["recThrs"])]
    lib.call("spe_coco_accumulate", *[a.data_ptr() for a in args], K, R_, M, pr[0].data_ptr(), rc.data_ptr(), pr[1].data_ptr(), Kn._st())
    pr, rc = pr.cpu().numpy(), rc.cpu().numpy()
    assert (pr[:, n_pr:] == TABLE_FILL).all() and (rc[n_rc:] == TABLE_FILL).all(), "written past the end"
    assert not (pr[:, :n_pr] == TABLE_FILL).any() and not (rc[:n_rc] == TABLE_FILL).any(), "an element was not written"
    return pr[0, :n_pr].reshape(cases.T, R_, K, cases.A, M), rc[:n_rc].reshape(cases.T, K, cases.A, M), pr[1, :n_pr].reshape(cases.T, R_, K, cases.A, M)


@functools.lru_cache(maxsize=None)
def streams_and_ref():
    evals, n_images, K = cases.acc_evals()
    return cases.acc_records(evals, n_images, K), R.accumulate(evals, n_images, K, P)


def test_accumulate_streams(dev):
    """Records per category of 0, 1, 255, 256, 257 and 513, the late maximum, recall 0.25 exactly, npig = 0, the rank filters: what
    tests/test_coco_meter_cpu.py::test_accumulate_streams_cover_the_cases shows the streams to hold."""
    rec, ref = streams_and_ref()
    got = call_accumulate(dev, *rec)
    for g, r, k in zip(got, ref, ("precision", "recall", "scores")):
        assert same(g, r), (k, np.argwhere(g != r)[:5])


@functools.lru_cache(maxsize=None)
def meter_ref(name):
    cat_ids, images, _, _ = case_and_ref(name)
    return R.evaluate(images, cat_ids)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_meter_on_device_equals_cpu_path(dev, name):
    cat_ids, images, _, _ = case_and_ref(name)
    out = run_meter(images, cat_ids, device=dev).summarize(return_records=True)
    cpu = run_meter(images, cat_ids).summarize(return_records=True)
    for k in cpu["records"]:
        assert same(out["records"][k], cpu["records"][k]), k
    assert same(out["npig"], cpu["npig"]) and same(out["stats"], cpu["stats"])
    for k in ("precision", "recall", "scores"):
        assert same(out["eval"][k].view(np.int64), cpu["eval"][k].view(np.int64)), k
    check_against(out, meter_ref(name))
    one_by_one = run_meter(images, cat_ids, [[i] for i in range(len(images))][::-1], device=dev)
    check_against(one_by_one.summarize(return_records=True), meter_ref(name))


def test_two_runs_bitwise_equal(dev):
    cat_ids, images, _, _ = case_and_ref("random_dense")
    a, b = (run_meter(images, cat_ids, device=dev).summarize(return_records=True) for _ in range(2))
    assert all(same(a["records"][k], b["records"][k]) for k in a["records"]) and same(a["npig"], b["npig"])
    assert all(same(a["eval"][k].view(np.int64), b["eval"][k].view(np.int64)) for k in ("precision", "recall", "scores"))
    assert same(a["stats"].view(np.int64), b["stats"].view(np.int64))


def test_update_does_not_synchronise(dev):
    """update() reads no device data on the host: under torch's sync debug mode any .item() / .cpu() / nonzero would raise."""
    cat_ids, images, _, _ = case_and_ref("random_small")
    res, gts = cases.split(images, dev)
    from spe_amd.evalmetrics import COCODetectionMeter
    m = COCODetectionMeter(cat_ids)
    m.update(res[:1], gts[:1])                         # first call: allocations, library load, the parameter arrays
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.update(res[1:3], gts[1:3])
        m.update(res[3:], gts[3:])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    check_against(m.summarize(return_records=True), meter_ref("random_small"))
