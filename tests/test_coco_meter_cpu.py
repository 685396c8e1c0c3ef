"""spe_amd.evalmetrics.COCODetectionMeter on CPU tensors (the numpy composition of the device rules) against the restatement of COCOeval
in tests/coco_eval_ref.py: hand-computed answers first (they hold the restatement itself to the published rules), then the meter
against the restatement on every case of tests/coco_eval_cases.py - flag words, ranks, npig, precision, recall, scores and the twelve
stats with np.array_equal, whatever way the images reach the meter (one call, several, permuted, two ranks over gloo).

No tolerance between the meter and the restatement: both sides take integer counts and correctly rounded fp64 operations in the same
order.  (Only a hand-written "1" is compared loosely, see is_one: the published precision carries 2^-52 in its denominator.)"""
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import coco_eval_cases as cases
import coco_eval_ref as R
from coco_eval_cases import check_against, run_meter, same, split

T = cases.T


@functools.lru_cache(maxsize=None)
def case_and_ref(name):
    """(cat_ids, images, the restatement's evaluation): computed once per case, shared, never written to."""
    cat_ids, images = cases.case(name)
    return cat_ids, images, R.evaluate(images, cat_ids)


def bits(word):
    """flag word -> (matched bits, ignore bits) as 0/1 lists over the ten thresholds."""
    return [(int(word) >> t) & 1 for t in range(T)], [(int(word) >> (T + t)) & 1 for t in range(T)]


# ---- hand-computed answers: the restatement and the meter -------------------------------------------------------------------------
def both(cat_ids, images):
    out = run_meter(images, cat_ids).summarize(return_records=True)
    ref = R.evaluate(images, cat_ids)
    check_against(out, ref)
    return out


def is_one(x):
    """'Precision 1' by the published rule is tp / (tp + fp + 2^-52): 1 / (1 + 2^-52) for a single true positive, one ulp below 1,
    and a mean of such numbers adds a few roundings of 2^-53.  The hand-computed 1 is checked to 2^-50; the exact bits are the
    restatement's, which every test here compares with np.array_equal."""
    return bool((np.abs(np.asarray(x, np.float64) - 1) <= 2.0 ** -50).all())


def test_parameters_are_the_published_ones():
    from spe_amd.evalmetrics import coco_params
    P, Q = R.params(), coco_params()
    assert P["iouThrs"].size == 10 and P["recThrs"].size == 101 and P["maxDets"] == [1, 10, 100]
    assert P["areaRng"] == [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
    assert all(same(P[k], Q[k]) for k in ("iouThrs", "recThrs", "maxDets", "areaRng"))
    assert P["iouThrs"][0] == 0.5 and P["iouThrs"][5] == 0.75           # what summarize() looks up AP50 and AP75 by


def test_detections_equal_to_ground_truth():
    """One 20 x 20 box (small) and one 50 x 50 box (medium), detected exactly: AP = AR = 1 where there is ground truth, -1 for 'large'."""
    ims = [cases.image(1, [((0, 0, 20, 20), .9, 1), ((100, 100, 150, 150), .8, 1)], [([0, 0, 20, 20], 1, 0, None), ([100, 100, 50, 50], 1, 0, None)])]
    out = both([1], ims)
    assert is_one(out["stats"][:5]) and is_one(out["stats"][7:11]) and out["stats"][[5, 11]].tolist() == [-1, -1]
    assert out["stats"][6] == .5                                                 # AR at maxDets 1: one of the two boxes
    assert out["npig"].tolist() == [[2, 1, 1, 0]]
    assert (out["eval"]["precision"][..., 3, :] == -1).all() and is_one(out["eval"]["precision"][..., :3, 2])
    assert (out["eval"]["recall"][:, :, :3, 2] == 1).all()
    assert out["eval"]["counts"] == [10, 101, 1, 4, 3] and out["eval"]["precision"].shape == (10, 101, 1, 4, 3)


def test_no_detections_give_zero():
    ims = [cases.image(1, [], [([0, 0, 20, 20], 1, 0, None)])]
    out = both([1], ims)
    assert out["stats"].tolist() == [0, 0, 0, 0, -1, -1, 0, 0, 0, 0, -1, -1]
    assert out["records"]["rank"].size == 0


def test_category_without_ground_truth_is_minus_one():
    """Category 2 has detections and no ground truth (npig = 0): -1 everywhere, and the means skip it."""
    ims = [cases.image(1, [((0, 0, 20, 20), .9, 1), ((0, 0, 20, 20), .8, 2)], [([0, 0, 20, 20], 1, 0, None)])]
    out = both([1, 2], ims)
    assert (out["eval"]["precision"][:, :, 1] == -1).all() and (out["eval"]["recall"][:, 1] == -1).all()
    assert (out["eval"]["scores"][:, :, 1] == -1).all()
    assert is_one(out["stats"][0]) and out["stats"][8] == 1 and out["npig"][1].tolist() == [0, 0, 0, 0]
    # crowd-only ground truth is the same: nothing to find
    ims = [cases.image(1, [((0, 0, 20, 20), .9, 1)], [([0, 0, 20, 20], 1, 1, None)])]
    assert (both([1], ims)["stats"] == -1).all()


def test_iou_exactly_half():
    cat_ids, images, ref = case_and_ref("half_iou")
    assert R.iou(R.to_xywh(images[0]["boxes"])[0], images[0]["gt_boxes"][0], False) == 0.5
    out = both(cat_ids, images)
    m, ig = bits(out["records"]["words"][0, 0])
    assert m == [1] + [0] * 9 and ig == [0] * 10
    assert is_one(out["stats"][1]) and out["stats"][2] == 0 and abs(out["stats"][0] - 0.1) <= 2.0 ** -50


def test_edge_cases_by_hand():
    w = lambda name: both(*cases.case(name))["records"]
    # equal IoUs: the last box took the first detection, so the second is left with the first box (IoU 2/3) up to 0.65
    r = w("equal_iou")
    assert bits(r["words"][0, 0])[0] == [1] * 7 + [0] * 3                     # 90 / 110 = 0.818
    assert bits(r["words"][1, 0])[0] == [1] * 4 + [0] * 3 + [1] * 3           # 0.5 .. 0.65 the first box; 0.7 .. 0.8 nothing; then the second
    # a plain match is not displaced by the crowd box: tp at 0.5, 0.55; the crowd (ignored) from 0.65 on
    r = w("keep_nonignored")
    m, ig = bits(r["words"][0, 0])
    assert m == [1] * 10 and ig[:2] == [0, 0] and ig[3:] == [1] * 7
    # three detections in one crowd box: matched and ignored at every threshold; the fourth is a plain false positive
    r = w("crowd3")
    assert [bits(x)[0] for x in r["words"][:3, 0]] == [[1] * 10] * 3 and [bits(x)[1] for x in r["words"][:3, 0]] == [[1] * 10] * 3
    assert bits(r["words"][3, 0]) == ([0] * 10, [0] * 10)
    # area fields on the bounds: 32^2 is small and medium, 96^2 medium and large
    out = both(*cases.case("area_edges"))
    assert out["npig"].tolist() == [[2, 1, 2, 1]] and is_one(out["stats"][3:6])
    # the unmatched 200 x 200 detection: ignored in small / medium, a false positive in all / large
    r = w("det_outside")
    assert [bits(x)[1] for x in r["words"][0]] == [[0] * 10, [1] * 10, [1] * 10, [0] * 10] and (r["words"][0] & 0x3ff == 0).all()
    # equal scores keep the incoming order: ranks 0, 1, 2 are the IoUs 0.8, 1.0, 0.9
    r = w("equal_scores")
    assert r["rank"].tolist() == [0, 1, 2]
    assert [sum(bits(x)[0]) for x in r["words"][:, 0]] == [7, 3, 0]            # 0.5 .. 0.8 | 0.85 .. 0.95 | nothing left
    # matched at 0.5 by the first detection, still free at 0.75 for the second
    r = w("free_at_075")
    assert bits(r["words"][0, 0])[0][:2] == [1, 1] and bits(r["words"][0, 0])[0][3:] == [0] * 7
    assert bits(r["words"][1, 0])[0][:2] == [0, 0] and bits(r["words"][1, 0])[0][3:9] == [1] * 6 and bits(r["words"][1, 0])[0][9] == 0


def test_first_hundred_and_ranks():
    cat_ids, images, ref = case_and_ref("counts")
    per_cat = np.bincount(ref["records"]["cat"], minlength=len(cat_ids))
    assert per_cat.tolist() == [min(n, 100) for n in cases.DET_COUNTS]
    rank, words, _ = R.match_image(images[0], cat_ids)
    assert int((rank < 0).sum()) == 1 + 30 and (words[rank < 0] == 0).all()


# ---- the meter's CPU path against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CASES))
def test_meter_equals_restatement(name):
    cat_ids, images, ref = case_and_ref(name)
    check_against(run_meter(images, cat_ids).summarize(return_records=True), ref)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_batch_composition_and_order(name):
    cat_ids, images, ref = case_and_ref(name)
    n = len(images)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5)).tolist()
    for batches in ([[i] for i in range(n)], [perm], [perm[:1], perm[1:]], [list(range(n))[::-1]]):
        check_against(run_meter(images, cat_ids, [b for b in batches if b]).summarize(return_records=True), ref)


@functools.lru_cache(maxsize=None)
def streams_and_ref():
    evals, n_images, K = cases.acc_evals()
    return cases.acc_records(evals, n_images, K), R.accumulate(evals, n_images, K, R.params())


def test_accumulate_streams_cover_the_cases():
    (words, rank, score, seg, npig), (precision, recall, _) = streams_and_ref()
    assert tuple(np.diff(seg)[:6]) == cases.ACC_ND and (npig[6] == 0).all() and (npig[7] == 4).all() and 0 in npig[1]
    assert (precision[:, :, 6] == -1).all() and (precision[:, :, 0] == 0).all() and (recall[:, 0] == 0).all()
    assert R.params()["recThrs"][25] == 0.25 and (recall[:, 7, :, 2] == 0.25).all()            # tp = 1 of npig = 4: recThrs[25] exactly
    assert (np.abs(precision[:, :26, 7, :, 2] - 0.5) < 1e-15).all() and (precision[:, 26:, 7, :, 2] == 0).all()
    assert (recall[:, 7, :, 0] == 0).all()                                     # maxDets 1: the first record, a false positive, alone
    assert 0 < recall[:, 2:6, :, 2].min() and recall[:, 2:6].max() < 1 and (precision[:, -1, 2:6] == 0).all()     # rc < 1: the tail of precision is 0
    assert (precision[:, 0, 5, 0, 2] == 512 / 513).all()                       # the late maximum reached the first record
    assert not same(precision[..., 0], precision[..., 1]) and not same(precision[..., 1], precision[..., 2])      # the rank filters bite


def test_accumulate_host_streams():
    from spe_amd.evalmetrics import _coco_accumulate_host
    (words, rank, score, seg, npig), ref = streams_and_ref()
    P = R.params()
    got = _coco_accumulate_host(*[torch.from_numpy(x) for x in (words, rank, score, seg, npig)],
                                torch.tensor(P["maxDets"], dtype=torch.int32), torch.from_numpy(P["recThrs"]))
    for g, r, k in zip(got, ref, ("precision", "recall", "scores")):
        assert same(g.numpy(), r), k


def test_duplicate_image_id_raises():
    cat_ids, images, _ = case_and_ref("presence")
    m = run_meter(images, cat_ids)
    m.summarize()
    m.update(*split(images[1:2]))
    with pytest.raises(ValueError, match="image id"):
        m.summarize()
    m.reset()
    m.update(*split(images))
    m.summarize()


def test_limits():
    from spe_amd.evalmetrics import COCODetectionMeter
    with pytest.raises(ValueError, match=str(cases.MAX_GT)):
        run_meter([cases.big_image(1, cases.MAX_GT + 1)], [1])
    with pytest.raises(ValueError, match=str(cases.MAX_DET)):
        run_meter([cases.big_image(cases.MAX_DET + 1, 1)], [1])
    with pytest.raises(RuntimeError):
        COCODetectionMeter([1]).summarize()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out, idle_rank=None):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ok, sizes = True, []
    for name in cases.CASES:
        cat_ids, images = cases.case(name)
        single = run_meter(images, cat_ids).summarize(return_records=True)
        mine = [i for i in range(len(images)) if (i * 7 + 3) % 5 % world == rank]      # an uneven split; a rank may see no image
        if idle_rank is not None:                                                      # every image to rank 0, none to the idle rank
            mine = [] if rank == idle_rank else list(range(len(images)))
        m = run_meter(images, cat_ids, [b for b in (mine[:1], mine[1:]) if b])
        m.merge()
        got = m.summarize(return_records=True)
        ok = ok and all(same(got[k], single[k]) for k in ("stats", "npig"))
        ok = ok and all(same(got["eval"][k], single["eval"][k]) for k in ("precision", "recall", "scores"))
        ok = ok and all(same(got["records"][k], single["records"][k]) for k in single["records"])
        try:
            m.merge()
            ok = False
        except RuntimeError:
            pass
        sizes.append(len(mine))
    out[rank] = (ok, sizes)
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_world2_merge():
    world = 2
    port = _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    res = dict(out)
    assert res[0][0] and res[1][0], res
    assert [a + b for a, b in zip(res[0][1], res[1][1])] == [len(cases.case(n)[1]) for n in cases.CASES]


def test_gloo_world2_merge_with_a_rank_that_saw_no_image():
    world = 2
    port = _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out, 1), nprocs=world, join=True)      # rank 1 makes no update() call at all, in any case
    res = dict(out)
    assert res[0][0] and res[1][0], res
    assert res[0][1] == [len(cases.case(n)[1]) for n in cases.CASES] and not any(res[1][1])


def test_merge_without_process_group_is_a_noop():
    cat_ids, images, _ = case_and_ref("presence")
    m = run_meter(images, cat_ids)
    a = m.summarize()
    m.merge()
    m.merge()
    assert same(m.summarize()["stats"], a["stats"])
