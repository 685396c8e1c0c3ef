"""The detection head on the device (csrc/detect.hip: spe_detect; spe_amd.infer.detect) against the CPU restatement tests/detect_ref.py
at every case of tests/detect_cases.py, against PostProcess -> per_class_nms on the same device, run to run, and one batch of
spe_amd.engine.evaluate_det_voc on the device against the CPU run.

Everything the kernel produces is an integer, a copied float or a composition of correctly rounded fp32 operations the restatement
performs in the same order, so every comparison is torch.equal (logits by bit pattern: the cases hold NaNs).  Scores are compared on
one device only: the sigmoid of the host and of the device are two implementations."""
import pytest
import torch

import detect_cases as cases
import detect_loops as loops
import detect_ref as dr
import voc_eval_cases as voc_cases

pytestmark = pytest.mark.gpu

_REF = {}


def ref_of(name, nms=True):
    if (name, nms) not in _REF:
        logits, boxes, sizes, k = cases.inputs(name)
        _REF[(name, nms)] = dr.detect_ref(logits, boxes, sizes, k, cases.IOU_THR, nms)
    return _REF[(name, nms)]


def garbage(B, k, dev):
    """The five output buffers, filled with what no result holds."""
    return (torch.full((B, k), 777.0, device=dev), torch.full((B, k), 123456789, device=dev, dtype=torch.int64),
            torch.full((B, k, 4), -5.0, device=dev), torch.full((B, k), 99999, device=dev, dtype=torch.int32),
            torch.full((B,), -7, device=dev, dtype=torch.int32))


def run_abi(name, nms, dev):
    from spe_amd import kernels as K
    logits, boxes, sizes, k = cases.inputs(name)
    B, Q, Kc = logits.shape
    ld, bd, sd = logits.to(dev), boxes.to(dev), sizes.to(dev)
    out = garbage(B, k, dev)
    K.lib.call("spe_detect", ld.data_ptr(), bd.data_ptr(), sd.data_ptr(), B, Q, Kc, k, cases.IOU_THR, 1 if nms else 0,
               *[t.data_ptr() for t in out], K._st())
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def check(got, ref):
    logit, label, box, query, count = got
    assert torch.equal(count, ref["count"]), (count.tolist(), ref["count"].tolist())
    assert torch.equal(label, ref["label"]) and torch.equal(query, ref["query"])
    assert dr.same_bits(logit, ref["logit"])
    assert torch.equal(box, ref["box"])


@pytest.mark.parametrize("name", list(cases.CASES))
def test_spe_detect(dev, name):
    check(run_abi(name, True, dev), ref_of(name))


@pytest.mark.parametrize("name", cases.NO_NMS)
def test_spe_detect_without_nms(dev, name):
    got = run_abi(name, False, dev)
    check(got, ref_of(name, False))
    assert (got[4] == cases.CASES[name][3]).all()


@pytest.mark.parametrize("name", cases.DISTINCT)
def test_results_equal_postprocess_then_nms_on_the_device(dev, name):
    from spe_amd import infer
    from spe_amd.models.conditional_detr import PostProcess
    logits, boxes, sizes, k = cases.inputs(name)
    outputs = {"pred_logits": logits.to(dev), "pred_boxes": boxes.to(dev)}
    prob = outputs["pred_logits"].sigmoid().reshape(logits.shape[0], -1)
    for p in prob:                                            # no two scores are equal on this device either
        assert torch.unique(p).numel() == p.numel()
    det = infer.detect(outputs, sizes.to(dev), k, cases.IOU_THR)
    want = infer.per_class_nms(PostProcess()(outputs, sizes.to(dev), k), cases.IOU_THR)
    got = det.results()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for key in ("scores", "labels", "boxes"):
            assert g[key].shape == w[key].shape and torch.equal(g[key], w[key]), key
    pad = det.padded()
    for b, p in enumerate(pad):
        n = int(det.counts[b])
        assert p["scores"].shape == (k,) and (p["labels"][n:] == -1).all() and (p["scores"][n:] == 0).all() and (p["boxes"][n:] == 0).all()


@pytest.mark.parametrize("name", ["coco_flip", "quantised", "specials"])
def test_two_runs_are_bitwise_equal(dev, name):
    a, b = run_abi(name, True, dev), run_abi(name, True, dev)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


def test_out_buffers_and_wrapper_checks(dev):
    from spe_amd import kernels as K
    logits, boxes, sizes, k = cases.inputs("n1023_k300")
    ld, bd, sd = logits.to(dev), boxes.to(dev), sizes.to(dev)
    first = K.detect(ld, bd, sd, k, cases.IOU_THR)
    want = [t.clone() for t in first]
    again = K.detect(ld.flip(0).contiguous(), bd.flip(0).contiguous(), sd.flip(0).contiguous(), k, cases.IOU_THR, out=first)
    assert all(a is b for a, b in zip(again, first))
    for a, w in zip(again, want):
        assert torch.equal(a.flip(0).view(torch.int32) if a.dtype == torch.float32 else a.flip(0), w.view(torch.int32) if w.dtype == torch.float32 else w)
    for bad in (0, 1024):
        with pytest.raises(ValueError):
            K.detect(ld, bd, sd, bad, cases.IOU_THR)
    with pytest.raises(ValueError):
        K.detect(ld, bd[:, :5], sd, k, cases.IOU_THR)


@pytest.mark.parametrize("Q,Kc,k,status", cases.REFUSED)
def test_refusals(dev, Q, Kc, k, status):
    """Host returns: the launcher looks at the sizes before it looks at a pointer, nothing is launched."""
    from spe_amd import lib
    assert lib.load().spe_detect(None, None, None, 1, Q, Kc, k, 0.5, 1, None, None, None, None, None, None) == status
    assert lib.load().spe_detect(None, None, None, 0, Q, Kc, k, 0.5, 1, None, None, None, None, None, None) == 0      # no image: nothing to do


def test_detect_into_a_meter_does_not_synchronise(dev):
    """detect(...).padded() -> meter.update() reads no device data on the host: under torch's sync debug mode any .item() / .cpu() /
    boolean-mask indexing would raise (per_class_nms, three mask indexings per image, does)."""
    from spe_amd import infer
    from spe_amd.evalmetrics import VOCDetectionMeter
    from spe_amd.models.conditional_detr import PostProcess
    logits, boxes, sizes, k = cases.inputs("voc")
    outputs, sd = {"pred_logits": logits.to(dev), "pred_boxes": boxes.to(dev)}, sizes.to(dev)
    gts = [{"boxes": torch.tensor([[10, 10, 200, 200]], device=dev), "labels": torch.tensor([3], device=dev),
            "difficult": torch.tensor([False], device=dev), "image_id": torch.tensor(i, device=dev)} for i in range(4)]
    m = VOCDetectionMeter(20)
    m.update(infer.detect(outputs, sd, k, cases.IOU_THR).padded(), gts[:2])               # first call: allocations, library load
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.update(infer.detect(outputs, sd, k, cases.IOU_THR).padded(), gts[2:])
        with pytest.raises(RuntimeError):
            infer.per_class_nms(PostProcess()(outputs, sd, k), cases.IOU_THR)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert m.summarize()["npos"][2] == 4


def test_evaluate_det_voc_on_the_device(dev):
    from spe_amd import engine
    g = voc_cases.load_golden("voc_eval_small")
    images, C = g["images"][:8], g["num_classes"]
    outs = []
    for device in (torch.device("cpu"), dev):
        model, loader, base_ds, _ = loops.voc_run(images, C, 8)
        outs.append(engine.evaluate_det_voc(model, loops.StubCriterion(), {}, loader, base_ds, device, None, None, num_classes=C))
    for key in ("ap07", "ap_area", "corloc", "npos", "nimgs"):
        assert voc_cases.same(outs[0][key], outs[1][key]), key
