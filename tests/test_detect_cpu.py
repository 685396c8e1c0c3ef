"""The detection head and the evaluation loops without a GPU: the restatement tests/detect_ref.py against the existing
PostProcess -> per_class_nms path, spe_amd.infer.detect on CPU tensors against the restatement at every case of tests/detect_cases.py,
and spe_amd.engine.evaluate_det_voc / evaluate_refinements with a stub model that returns canned outputs.

The VOC loop and the golden.  tests/golden/voc_eval_small.pt holds 126 detections that never went through an NMS: the per-class NMS
of the loop suppresses 18 of them (labels 1, 2 and 4) and PostProcess clamps 3 negative coordinates to 0, so the loop cannot see
"exactly the golden's detections".  What the head keeps is asserted against detect_ref: the golden's detections with the clamp, minus
those a greedy per-class NMS at 0.5 removes, in the golden's order.  Of the recorded numbers the loop reproduces bitwise what those
two steps cannot change - CorLoc of every class (it looks at the best detection of a class only, which an NMS never removes) and AP07
of the class that loses nothing; AP07 of every class is bitwise that of the restated reference evaluator (tests/voc_eval_ref.py, which
test_voc_meter_cpu holds to the same golden) on the kept detections."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import coco_eval_cases as coco_cases
import criterion_ref as cr
import detect_cases as cases
import detect_loops as loops
import detect_ref as dr
import voc_eval_cases as voc_cases
import voc_eval_ref as voc_ref
from spe_amd import engine, infer
from spe_amd.models.conditional_detr import PostProcess

_REF = {}


def ref_of(name, nms=True):
    """detect_ref of a case, computed once."""
    if (name, nms) not in _REF:
        logits, boxes, sizes, k = cases.inputs(name)
        _REF[(name, nms)] = dr.detect_ref(logits, boxes, sizes, k, cases.IOU_THR, nms)
    return _REF[(name, nms)]


def same_list(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for key in ("scores", "labels", "boxes"):
            assert g[key].shape == w[key].shape and torch.equal(g[key], w[key]), key


def existing_path(logits, boxes, sizes, k, thr):
    return infer.per_class_nms(PostProcess()({"pred_logits": logits, "pred_boxes": boxes}, sizes, k), thr)


# ---- the restatement against the existing path -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.DISTINCT)
def test_ref_equals_postprocess_then_nms(name):
    logits, boxes, sizes, k = cases.inputs(name)
    prob = logits.sigmoid().reshape(logits.shape[0], -1)
    for p in prob:                                            # the reference path is unambiguous: no two scores are equal
        assert torch.unique(p).numel() == p.numel()
    same_list(dr.results_of(ref_of(name)), existing_path(logits, boxes, sizes, k, cases.IOU_THR))


def test_nms_pairs_straddle_the_threshold():
    """IoU 0.5015 suppresses, 0.4993 does not: three of the four boxes of class 4 survive."""
    ref = ref_of("nms_pairs")
    assert ((ref["label"] == 4).sum(1) == 3).all() and ((ref_of("nms_pairs", False)["label"] == 4).sum(1) == 4).all()


def test_canonical_key_orders_like_topk():
    x = torch.tensor([0.0, -0.0, 1.0, -1.0, float("inf"), float("-inf"), float("nan"), 1e-45, -1e-45])
    key = dr.canonical_key(x)
    assert key[0] == key[1] and key[6] == 0xFFFFFFFF and key[4] < key[6] and key[5] == key.min()
    order = np.argsort(key, kind="stable")
    assert order.tolist() == [5, 3, 8, 0, 1, 7, 2, 4, 6]
    assert torch.equal(torch.from_numpy(key.astype(np.int64)), infer.select_key(x))


# ---- infer.detect on CPU tensors -------------------------------------------------------------------------------------------------------
def check_detections(det, ref, k):
    assert dr.same_bits(det.logits, ref["logit"])
    assert torch.equal(det.labels, ref["label"]) and torch.equal(det.boxes, ref["box"])
    assert torch.equal(det.queries, ref["query"]) and torch.equal(det.counts, ref["count"])
    assert det.queries.dtype == torch.int32 and det.counts.dtype == torch.int32 and det.labels.dtype == torch.int64
    pad = det.padded()
    assert len(pad) == det.logits.shape[0]
    for b, p in enumerate(pad):
        n = int(ref["count"][b])
        assert p["scores"].shape == (k,) and p["labels"].shape == (k,) and p["boxes"].shape == (k, 4)
        assert (p["labels"][n:] == -1).all() and (p["scores"][n:] == 0).all() and (p["boxes"][n:] == 0).all()
        assert (p["labels"][:n] >= 0).all()
    if not torch.isnan(ref["logit"]).any():                   # NaN scores do not compare equal
        same_list(det.results(), dr.results_of(ref))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_infer_detect_cpu(name):
    logits, boxes, sizes, k = cases.inputs(name)
    det = infer.detect({"pred_logits": logits, "pred_boxes": boxes}, sizes, k, cases.IOU_THR)
    check_detections(det, ref_of(name), k)


@pytest.mark.parametrize("name", cases.NO_NMS)
def test_infer_detect_cpu_without_nms(name):
    logits, boxes, sizes, k = cases.inputs(name)
    det = infer.detect({"pred_logits": logits, "pred_boxes": boxes}, sizes, k, cases.IOU_THR, nms=False)
    check_detections(det, ref_of(name, False), k)
    assert (det.counts == k).all()


def test_without_nms_is_postprocess_reordered():
    logits, boxes, sizes, k = cases.inputs("voc")
    det = infer.detect({"pred_logits": logits, "pred_boxes": boxes}, sizes, k, nms=False).results()
    for r, p in zip(det, PostProcess()({"pred_logits": logits, "pred_boxes": boxes}, sizes, k)):
        o = torch.sort(p["labels"], stable=True).indices      # PostProcess's list is score-descending
        assert torch.equal(r["scores"], p["scores"][o]) and torch.equal(r["labels"], p["labels"][o]) and torch.equal(r["boxes"], p["boxes"][o])


def test_integer_sizes_and_refusals():
    logits, boxes, sizes, k = cases.inputs("n1023_k300")
    a = infer.detect({"pred_logits": logits, "pred_boxes": boxes}, sizes.long(), k)          # orig_size arrives as int64
    assert torch.equal(a.boxes, ref_of("n1023_k300")["box"])
    for bad in (0, logits.shape[1] * logits.shape[2] + 1):
        with pytest.raises(ValueError):
            infer.detect({"pred_logits": logits, "pred_boxes": boxes}, sizes, bad)
    with pytest.raises(ValueError):
        infer.detect({"pred_logits": torch.zeros(1, 2000, 1), "pred_boxes": torch.zeros(1, 2000, 4)}, sizes[:1], 1025)


# ---- evaluate_det_voc ------------------------------------------------------------------------------------------------------------------
def _voc_golden():
    g = voc_cases.load_golden("voc_eval_small")
    return g, g["images"], g["num_classes"]


def _check_voc_precondition(images, kept):
    """What the head keeps of every image: the golden's detections, clamped at 0, minus what a greedy per-class NMS removes, in the
    golden's order (after the decimal round trip of the result files, which is all the evaluator sees); background rows besides."""
    lost = np.zeros(8, int)
    for im, r in zip(images, kept):
        box = im["boxes"].clamp(min=0)
        keep = cr.greedy_nms_ref(box, im["labels"], 0.5) if len(box) else torch.zeros(0, dtype=torch.bool)
        np.add.at(lost, im["labels"][~keep].numpy(), 1)
        real = r["labels"] >= 1
        assert (r["labels"][~real] == 0).all() and torch.equal(r["labels"][real], im["labels"][keep])
        qs, qb = voc_ref.quantise(r["scores"][real].numpy(), r["boxes"][real].numpy(), True)
        ws, wb = voc_ref.quantise(im["scores"][keep].numpy(), box[keep].numpy(), True)
        assert np.array_equal(qs, ws) and np.array_equal(qb, wb)
    return lost


def _kept_images(images, kept):
    out = []
    for im, r in zip(images, kept):
        real = r["labels"] >= 1
        out.append({**{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in im.items()}, "boxes": r["boxes"][real].numpy(),
                    "scores": r["scores"][real].numpy(), "labels": r["labels"][real].numpy()})
    return out


@pytest.mark.parametrize("with_flip", [False, True])
def test_evaluate_det_voc(with_flip, capsys):
    g, images, C = _voc_golden()
    batch = 8
    model, loader, base_ds, canned = loops.voc_run(images, C, batch, flip=with_flip)
    merged = [loops.flip_merged(c) for c in canned] if with_flip else canned
    if with_flip:
        assert all(m["pred_logits"].shape[1] == 600 for m in merged)
    want_meter, kept = loops.voc_expected(images, C, merged, batch)
    lost = _check_voc_precondition(images, kept)
    crit = loops.StubCriterion()
    out = engine.evaluate_det_voc(model, crit, {}, loader, base_ds, torch.device("cpu"), None, None, with_flip=with_flip, num_classes=C)
    assert model.evaled and crit.evaled and model.calls == len(loader)
    want = want_meter.summarize()
    for key in ("ap07", "ap_area", "corloc", "npos", "nimgs", "map", "mean_corloc"):
        assert voc_cases.same(out[key], want[key]), key
    ref = voc_ref.evaluate(_kept_images(images, kept), C, 0.5, True)
    assert voc_cases.same(out["ap07"], ref["ap07"]) and voc_cases.same(out["corloc"], ref["corloc"])
    assert voc_cases.same(out["corloc"], g["corloc"])                                   # the golden, every class
    untouched = [c for c in range(C) if lost[c + 1] == 0]
    assert untouched and lost.sum() == 18
    for c in untouched:
        assert voc_cases.same(out["ap07"][c], g["ap07"][c])                             # the golden, where the NMS removes nothing
    text = capsys.readouterr().out
    assert "VOC07 metric? Yes" in text and "Mean AP = {:.4f}".format(out["map"]) in text
    assert "CorLoc for class1 = {:.4f}".format(float(out["corloc"][0])) in text and "Test:" in text


# ---- evaluate_refinements --------------------------------------------------------------------------------------------------------------
def _coco_images():
    cat_ids, images = coco_cases.case("random_small")
    return cat_ids, images


def test_evaluate_refinements(capsys):
    cat_ids, images = _coco_images()
    batch = 4
    model, crit, loader, base_ds, canned = loops.coco_run(images, batch)
    base_ds = type("DS", (dict,), {"getCatIds": lambda self: cat_ids})(base_ds)
    stats, meter = engine.evaluate_refinements(model, crit, {"bbox": None}, loader, base_ds, torch.device("cpu"), None, refine_stage=1)
    assert model.evaled and crit.evaled
    assert crit.seen == [["labels", "boxes", "cardinality"]] * len(loader) and crit.losses == ["labels", "boxes", "cardinality", "image_label"]
    want = loops.coco_expected(images, cat_ids, canned, batch).summarize()
    assert len(stats["coco_eval_bbox"]) == 12 and coco_cases.same(stats["coco_eval_bbox"], want["stats"])
    assert coco_cases.same(meter.summarize()["stats"], want["stats"]) and (want["stats"] > 0).any()
    ledger = loops.ledger_restatement(crit, canned)
    assert set(stats) == set(ledger) | {"coco_eval_bbox"}
    for k, v in ledger.items():
        assert stats[k] == v, (k, stats[k], v)
    text = capsys.readouterr().out
    assert "Averaged stats:" in text and "Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ]" in text
    # the label set of a plain mapping serves as the category list
    model, crit, loader, plain, _ = loops.coco_run(images, batch)
    stats2, _ = engine.evaluate_refinements(model, crit, {"bbox": None}, loader, plain, torch.device("cpu"), None, refine_stage=1)
    labels = sorted({int(c) for im in images for c in im["gt_labels"]})
    assert coco_cases.same(stats2["coco_eval_bbox"], loops.coco_expected(images, labels, canned, batch).summarize()["stats"])


@pytest.mark.parametrize("key", ["segm", "panoptic"])
def test_evaluate_refinements_refuses_masks(key):
    cat_ids, images = _coco_images()
    model, crit, loader, base_ds, _ = loops.coco_run(images, 4)
    with pytest.raises(NotImplementedError):
        engine.evaluate_refinements(model, crit, {"bbox": None, key: None}, loader, base_ds, torch.device("cpu"), None)
    assert model.calls == 0


# ---- no host read inside the batch loop ------------------------------------------------------------------------------------------------
class _Trap:
    """Tensor.item / Tensor.tolist raise from the model's first call until the loader is exhausted.  The one read the loops are meant to
    make in between - the ledger's summary and the host timers behind a log line - is let through; the summaries after the loop are free anyway."""

    def __init__(self, monkeypatch):
        from spe_amd.steplog import SmoothedValue, StepLedger
        self.on = False

        def guard(fn):
            def guarded(t, *a, **k):
                if self.on:
                    raise AssertionError("host read of a tensor inside the batch loop")
                return fn(t, *a, **k)
            return guarded

        def free(fn):
            def freed(*a, **k):
                was, self.on = self.on, False
                try:
                    return fn(*a, **k)
                finally:
                    self.on = was
            return freed
        monkeypatch.setattr(torch.Tensor, "item", guard(torch.Tensor.item))
        monkeypatch.setattr(torch.Tensor, "tolist", guard(torch.Tensor.tolist))
        monkeypatch.setattr(StepLedger, "summary", free(StepLedger.summary))             # the meters of a log line
        monkeypatch.setattr(SmoothedValue, "__str__", free(SmoothedValue.__str__))       # its iteration / data times: host values

    def model(self, model):
        trap = self

        class Armed:
            def eval(self):
                model.eval()

            def __call__(self, samples):
                trap.on = True
                return model(samples)
        return Armed()

    def loader(self, batches):
        trap = self

        class Loader(list):
            def __iter__(self):
                yield from list.__iter__(self)
                trap.on = False
        return Loader(batches)


def test_loops_read_nothing_inside_the_batch_loop(monkeypatch):
    trap = _Trap(monkeypatch)
    g, images, C = _voc_golden()
    model, loader, base_ds, canned = loops.voc_run(images[:16], C, 8)
    out = engine.evaluate_det_voc(trap.model(model), loops.StubCriterion(), {}, trap.loader(loader), base_ds, torch.device("cpu"), None, None,
                                  num_classes=C)
    assert not trap.on and voc_cases.same(out["ap07"], loops.voc_expected(images[:16], C, canned, 8)[0].summarize()["ap07"])
    cat_ids, cimages = _coco_images()
    model, crit, loader, base_ds, canned = loops.coco_run(cimages, 4)
    base_ds = type("DS", (dict,), {"cat_ids": cat_ids})(base_ds)
    stats, _ = engine.evaluate_refinements(trap.model(model), crit, {"bbox": None}, trap.loader(loader), base_ds, torch.device("cpu"), None,
                                           refine_stage=1)
    assert not trap.on and coco_cases.same(stats["coco_eval_bbox"], loops.coco_expected(cimages, cat_ids, canned, 4).summarize()["stats"])
    trap.on = True                                            # the trap itself works
    with pytest.raises(AssertionError, match="host read"):
        torch.zeros(1).item()
    with pytest.raises(AssertionError, match="host read"):
        torch.zeros(2).tolist()
    trap.on = False


# ---- two ranks over gloo ---------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g, images, C = _voc_golden()
    mine = [im for i, im in enumerate(images) if (i * 7 + 3) % 5 % world == rank]           # an uneven split
    model, loader, base_ds, _ = loops.voc_run(mine, C, 8)
    voc = engine.evaluate_det_voc(model, loops.StubCriterion(), {}, loader, base_ds, torch.device("cpu"), None, None, num_classes=C)
    cat_ids, cimages = _coco_images()
    cmine = cimages[rank::world]
    model, crit, loader, base_ds, _ = loops.coco_run(cmine, 1)
    base_ds = type("DS", (dict,), {"cat_ids": cat_ids})(base_ds)
    stats, _ = engine.evaluate_refinements(model, crit, {"bbox": None}, loader, base_ds, torch.device("cpu"), None, refine_stage=1)
    out[rank] = ({k: np.asarray(voc[k]) for k in ("ap07", "ap_area", "corloc", "npos", "nimgs")}, stats, len(mine))
    dist.barrier()
    dist.destroy_process_group()


def test_loops_over_gloo_world2():
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    res = dict(out)
    g, images, C = _voc_golden()
    model, loader, base_ds, _ = loops.voc_run(images, C, 8)
    voc = engine.evaluate_det_voc(model, loops.StubCriterion(), {}, loader, base_ds, torch.device("cpu"), None, None, num_classes=C)
    cat_ids, cimages = _coco_images()
    model, crit, loader, base_ds, canned = loops.coco_run(cimages, 1)         # one image per step on either side: the same steps
    base_ds = type("DS", (dict,), {"cat_ids": cat_ids})(base_ds)
    stats, _ = engine.evaluate_refinements(model, crit, {"bbox": None}, loader, base_ds, torch.device("cpu"), None, refine_stage=1)
    assert res[0][2] + res[1][2] == len(images) and res[0][2] != res[1][2]
    for rank in range(world):
        v, s, _ = res[rank]
        for k in ("ap07", "ap_area", "corloc", "npos", "nimgs"):
            assert voc_cases.same(v[k], voc[k]), (rank, k)
        assert coco_cases.same(s["coco_eval_bbox"], stats["coco_eval_bbox"])
        # the ledger's global averages: fp64 totals of the same n positive terms, added per rank first.  Either order is within
        # (n - 1) 2^-53 of the exact sum, relatively, so the two are within n 2^-52 of each other
        n = len(canned)
        for k, want in stats.items():
            if k != "coco_eval_bbox":
                assert abs(s[k] - want) <= n * 2.0 ** -52 * abs(want), (k, s[k], want)
