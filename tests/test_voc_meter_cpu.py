"""spe_amd.evalmetrics.VOCDetectionMeter on CPU tensors (the numpy composition of the device rules): the recorded results of the
reference's own evaluator (tests/golden/voc_eval_*.pt, tools/gen_voc_eval_golden.py), invariance to how the images reach the meter,
the dropped labels, the duplicate-id error, the world-2 merge over gloo and the strict threshold without the file round trip.

Equalities: flags, rec, prec and AP07 bitwise (NaN matches NaN: rec of a class without non-difficult ground truth); area AP within
nd * 2^-52 absolute, nd the detections of the class - two summation orders (numpy's pairwise, the meter's fixed one) of at most nd
fp64 terms whose partial sums are <= 1 differ by at most nd roundings of 2^-53 each, on either side."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import voc_eval_cases as cases
import voc_eval_ref as R
from voc_eval_cases import as_numpy, check_against, load_golden, run_meter, same, split

@pytest.mark.parametrize("name", cases.GOLDENS)
def test_golden(name):
    g = load_golden(name)
    C, images = g["num_classes"], g["images"]
    out = run_meter(images, C, ovthresh=g["ovthresh"]).summarize(return_curves=True)
    ref = R.evaluate(as_numpy(images), C, g["ovthresh"], True)
    check_against(out, {**{k: g[k] for k in ("rec", "prec", "ap07", "ap_area", "corloc")}, "flags": ref["flags"]}, C)
    assert same(out["npos"], ref["npos"]) and same(out["nimgs"], ref["nimgs"])
    assert same(out["map"], np.mean(g["ap07"].numpy())) and same(out["mean_corloc"], np.mean(g["corloc"].numpy()))
    area = run_meter(images, C, ovthresh=g["ovthresh"]).summarize(use_07_metric=False)
    assert same(area["ap"], area["ap_area"]) and same(out["ap"], out["ap07"])


def test_edges_outcomes():
    """The six edge classes of voc_eval_edges, outcome by outcome (1 tp, 2 fp, 0 neither), in curve order."""
    g = load_golden("voc_eval_edges")
    out = run_meter(g["images"], 6).summarize(return_curves=True)
    assert [f.tolist() for f in out["flags"]] == [[], [], [0, 2, 2], [1, 2], [1, 1, 2], [0, 2, 0, 1]]
    assert out["npos"].tolist() == [1, 0, 0, 2, 2, 1] and out["nimgs"].tolist() == [1, 0, 1, 1, 2, 1]
    assert out["ap07"][:2].tolist() == [0.0, 0.0] and out["ap_area"][:2].tolist() == [0.0, 0.0]     # no detections: 0 whatever npos is
    assert out["ap07"][2] == 0.0 and np.isnan(float(out["ap_area"][2])) and np.isnan(out["rec"][2].numpy()).all()  # detections, npos = 0
    assert not np.isnan(out["map"])                    # the 11-point mean is finite here; the area one is NaN (np.mean propagates)
    assert np.isnan(run_meter(g["images"], 6).summarize(use_07_metric=False)["map"])


def test_batch_composition_and_order():
    g = load_golden("voc_eval_small")
    C, images = g["num_classes"], g["images"]
    n = len(images)
    whole = run_meter(images, C).summarize(return_curves=True)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5)).tolist()
    for batches in ([[i] for i in range(n)], [perm], [perm[:7], perm[7:8], perm[8:]], [list(range(n))[::-1]]):
        out = run_meter(images, C, batches).summarize(return_curves=True)
        for k in ("ap07", "ap_area", "corloc", "npos", "nimgs"):
            assert same(out[k], whole[k]), k
        for c in range(C):
            assert all(same(out[k][c], whole[k][c]) for k in ("flags", "rec", "prec"))


def test_unsorted_detections_are_ordered():
    """Detections that do not arrive in per_class_nms order are matched in (label ascending, score descending) all the same."""
    g = load_golden("voc_eval_small")
    C, images = g["num_classes"], g["images"]
    gen = torch.Generator().manual_seed(9)
    shuffled = []
    for im in images:
        p = torch.randperm(im["scores"].numel(), generator=gen)
        shuffled.append({**im, "boxes": im["boxes"][p], "scores": im["scores"][p], "labels": im["labels"][p]})
    a, b = run_meter(images, C).summarize(return_curves=True), run_meter(shuffled, C).summarize(return_curves=True)
    assert same(a["ap07"], b["ap07"]) and same(a["ap_area"], b["ap_area"]) and same(a["corloc"], b["corloc"])
    assert all(same(a["flags"][c], b["flags"][c]) for c in range(C))


def test_labels_outside_classes_are_dropped():
    C, images = cases.match_case("two_images_shifted", integer_dets=False)
    clean = [{**im, **{k: im[k][(im["labels"] >= 1) & (im["labels"] <= C)] for k in ("boxes", "scores", "labels")}} for im in images]
    assert sum(im["labels"].size for im in images) == sum(im["labels"].size for im in clean) + 6 * len(images)
    a, b = run_meter(images, C).summarize(return_curves=True), run_meter(clean, C).summarize(return_curves=True)
    ref = R.evaluate(images, C)
    for out in (a, b):
        check_against(out, ref, C)


def test_duplicate_image_id_raises():
    g = load_golden("voc_eval_edges")
    m = run_meter(g["images"], 6)
    m.summarize()
    m.update(*split(g["images"][1:2]))
    with pytest.raises(ValueError, match="image id"):
        m.summarize()
    m.reset()
    m.update(*split(g["images"]))
    m.summarize()
    with pytest.raises(ValueError):
        run_meter(g["images"], 6, [[0, 1, 0]]).summarize()


def test_limits():
    im = {"boxes": np.zeros((cases.MAX_DET + 1, 4), np.float32), "scores": np.zeros(cases.MAX_DET + 1, np.float32),
          "labels": np.ones(cases.MAX_DET + 1, np.int64), "gt_boxes": np.zeros((0, 4)), "gt_labels": np.zeros(0, np.int64),
          "difficult": np.zeros(0, bool), "image_id": 0}
    with pytest.raises(ValueError, match="4096"):
        run_meter([im], 2)


def test_strict_threshold_without_round_trip():
    """ovthresh = 0.5, raw coordinates: ground truth (1,1,10,10) covers 100 pixels; the detection over its top half overlaps by
    exactly 50/100 = 0.5 and stays a false positive (the test is `>`), 51/100 is a true positive."""
    def one(box):
        return {"boxes": np.array([box], np.float32), "scores": np.array([0.5], np.float32), "labels": np.array([1]),
                "gt_boxes": np.array([[1, 1, 10, 10]]), "gt_labels": np.array([1]), "difficult": np.array([False]), "image_id": 1}
    half = one([0, 0, 9, 4])                # + 1: (1,1,10,5): 10 x 5 = 50, union 100
    assert R.overlaps(R.quantise(half["scores"], half["boxes"], False)[1][0], np.array([[1., 1., 10., 10.]]))[0] == 0.5
    out = run_meter([half], 1, file_roundtrip=False).summarize(return_curves=True)
    assert out["flags"][0].tolist() == [2] and out["corloc"].tolist() == [0.0] and out["ap07"].tolist() == [0.0]
    more = one([0, 0, 9, 4.1])              # intersection 10 x 5.1 = 51 of 100: no decimal round trip, so the .1 survives
    out = run_meter([more], 1, file_roundtrip=False).summarize(return_curves=True)
    assert out["flags"][0].tolist() == [1] and out["corloc"].tolist() == [1.0]
    assert same(out["ap_area"], [1.0])


def test_raw_scores_without_round_trip():
    """file_roundtrip=False on a whole case: raw fp32 scores, double(x) + 1.0, against the restatement in the same mode."""
    g = load_golden("voc_eval_edges")
    images = as_numpy(g["images"])
    out = run_meter(images, 6, file_roundtrip=False).summarize(return_curves=True)
    check_against(out, R.evaluate(images, 6, 0.5, False), 6)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out, idle_rank=None):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g = load_golden("voc_eval_small")
    C, images = g["num_classes"], g["images"]
    single = run_meter(images, C).summarize(return_curves=True)
    mine = [i for i in range(len(images)) if (i * 7 + 3) % 5 % world == rank]      # an uneven split
    if idle_rank is not None:                                                      # every image to rank 0, none to the idle rank
        mine = [] if rank == idle_rank else list(range(len(images)))
    m = run_meter(images, C, [b for b in (mine[:5], mine[5:]) if b])
    m.merge()
    got = m.summarize(return_curves=True)
    ok = all(same(got[k], single[k]) for k in ("ap07", "ap_area", "corloc", "npos", "nimgs", "map", "mean_corloc"))
    ok = ok and all(same(got[k][c], single[k][c]) for k in ("flags", "rec", "prec") for c in range(C))
    try:
        m.merge()
        ok = False
    except RuntimeError:
        pass
    out[rank] = (ok, len(mine))
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_world2_merge():
    world = 2
    port = _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    res = dict(out)
    assert res[0][0] and res[1][0], res
    assert res[0][1] + res[1][1] == 40 and res[0][1] != res[1][1]


def test_gloo_world2_merge_with_a_rank_that_saw_no_image():
    world = 2
    port = _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out, 1), nprocs=world, join=True)      # rank 1 makes no update() call at all
    assert dict(out) == {0: (True, 40), 1: (True, 0)}


def test_merge_without_process_group_is_a_noop():
    g = load_golden("voc_eval_edges")
    m = run_meter(g["images"], 6)
    a = m.summarize()
    m.merge()
    m.merge()
    assert same(m.summarize()["ap07"], a["ap07"])
