"""Stub model, stub criterion and canned batches for the tests of the evaluation loops (spe_amd.engine.evaluate_det_voc,
evaluate_refinements; tests/test_detect_cpu.py, tests/test_detect_gpu.py).

A run's detections (the image dicts of tests/voc_eval_cases.py / tests/coco_eval_cases.py) are encoded as the model output that makes
the detection head return them: detection j of an image is query j, its logit sits in the column of its label, every other entry of
the classes is -inf, and column 0 - a label both meters drop, as engine_loc.py:184 drops the background - holds -20 in every query, so
the top k is the image's detections followed by background rows.  Boxes are normalised by a 512 x 512 frame (a power of two: the scale
back is exact).  What the head keeps of them (the clamp at 0, the per-class NMS) is NOT assumed: the tests take it from detect_ref."""
import copy

import numpy as np
import torch

import detect_ref as dr
from spe_amd.util.misc import NestedTensor

FRAME = 512


def encode(images, Q, Kc):
    """image dicts -> {'pred_logits' [B,Q,Kc], 'pred_boxes' [B,Q,4]} (CPU, fp32)."""
    B = len(images)
    logits = torch.full((B, Q, Kc), float("-inf"))
    logits[:, :, 0] = -20.0
    boxes = torch.zeros(B, Q, 4)
    for b, im in enumerate(images):
        n = len(im["scores"])
        assert n <= Q
        p = torch.as_tensor(im["scores"]).double()
        logits[b, torch.arange(n), torch.as_tensor(im["labels"]).long()] = torch.log(p / (1 - p)).float()
        xy = torch.as_tensor(im["boxes"]).double().reshape(-1, 4)
        boxes[b, :n] = (torch.cat([(xy[:, :2] + xy[:, 2:]) / 2, xy[:, 2:] - xy[:, :2]], 1) / FRAME).float()
    return {"pred_logits": logits, "pred_boxes": boxes}


def samples_of(B, g):
    return NestedTensor(torch.randn(B, 3, 8, 12, generator=g), torch.zeros(B, 8, 12, dtype=torch.bool))


class StubModel:
    """Returns the canned outputs batch by batch.  wrap(outputs) shapes them as the loop expects its model to."""

    def __init__(self, canned, wrap, flip=False):
        self.canned, self.wrap, self.flip, self.calls, self.evaled = canned, wrap, flip, 0, False

    def eval(self):
        self.evaled = True

    def __call__(self, samples):
        out = {k: v.clone().to(samples.tensors.device) for k, v in self.canned[self.calls].items()}
        self.calls += 1
        if self.flip:
            # a symmetric detector: the even detections come from the image, the odd ones from its mirror image, where their centre
            # sits at 1 - cx; decouple_output has to put the two halves side by side along the query axis and mirror the second back
            B, x = out["pred_logits"].shape[0], samples.tensors
            assert x.shape[0] == 2 * B and torch.equal(x[B:], x[:B].flip(-1)) and torch.equal(samples.mask[B:], samples.mask[:B].flip(-1))
            lg, bx = out["pred_logits"], out["pred_boxes"]
            odd = (torch.arange(lg.shape[1], device=lg.device) % 2 == 1)[None, :, None]
            mirrored = bx.clone()
            mirrored[..., 0] = 1 - mirrored[..., 0]
            gone = torch.full_like(lg, float("-inf"))
            gone[:, :, 0] = -25.0
            out = {"pred_logits": torch.cat([torch.where(odd, gone, lg), torch.where(odd, lg, gone)]), "pred_boxes": torch.cat([bx, mirrored])}
        return self.wrap(out)


def flip_merged(canned):
    """What decouple_output makes of StubModel(flip=True)'s output, restated: [B, 2Q, .]."""
    lg, bx = canned["pred_logits"], canned["pred_boxes"]
    odd = (torch.arange(lg.shape[1]) % 2 == 1)[None, :, None]
    gone = torch.full_like(lg, float("-inf"))
    gone[:, :, 0] = -25.0
    back = bx.clone()
    back[..., 0] = 1 - (1 - back[..., 0])
    return {"pred_logits": torch.cat([torch.where(odd, gone, lg), torch.where(odd, lg, gone)], 1), "pred_boxes": torch.cat([bx, back], 1)}


class StubCriterion:
    """Losses that are plain functions of the output, and a record of `losses` at every call."""

    def __init__(self):
        self.losses = ["labels", "boxes", "cardinality", "image_label"]
        self.weight_dict = {"loss_ce": 2.0, "loss_bbox": 5.0, "loss_giou": 2.0, "loss_unused": 1.0}
        self.seen, self.evaled = [], False

    def eval(self):
        self.evaled = True

    def __call__(self, outputs, targets):
        self.seen.append(list(self.losses))
        m = outputs["pred_boxes"].mean()
        return {"loss_ce": m * 1.5, "class_error": m * 100, "loss_bbox": m + 0.25, "loss_giou": m * m, "cardinality_error": m * 3}


def ledger_restatement(criterion, canned):
    """MetricLogger's global averages of the losses StubCriterion gives, as the step ledger documents its arithmetic: fp32 values, fp32
    products, the fp32 weighted sum in key order, each totalled in fp64 and divided by the number of steps."""
    tot, n = {}, 0
    for out in canned:
        ld = copy.deepcopy(criterion)(out, None)
        loss = np.float32(0)
        for k, v in ld.items():
            v = np.float32(v.numpy())
            tot[k + "_unscaled"] = tot.get(k + "_unscaled", 0.0) + float(v)
            if k in criterion.weight_dict:
                s = np.float32(v * np.float32(criterion.weight_dict[k]))
                tot[k] = tot.get(k, 0.0) + float(s)
                loss = np.float32(loss + s)
        tot["loss"] = tot.get("loss", 0.0) + float(loss)
        n += 1
    out = {k: v / n for k, v in tot.items()}
    out["class_error"] = out["class_error_unscaled"]
    return out


# ---- VOC ---------------------------------------------------------------------------------------------------------------------------
def voc_run(images, C, batch, Q=300, device="cpu", flip=False, seed=0):
    """-> (model, loader, base_ds, canned): the arguments of evaluate_det_voc for the images in batches of `batch`."""
    g = torch.Generator().manual_seed(seed)
    canned, loader, base_ds = [], [], {}
    for i in range(0, len(images), batch):
        ims = images[i:i + batch]
        canned.append(encode(ims, Q, C + 1))
        targets = [{"idx": torch.tensor(int(im["image_id"])), "image_size": torch.tensor([FRAME, FRAME])} for im in ims]
        loader.append((samples_of(len(ims), g), targets))
    for im in images:
        base_ds[int(im["image_id"])] = {"boxes": torch.as_tensor(im["gt_boxes"]), "labels": torch.as_tensor(im["gt_labels"]),
                                        "difficult": torch.as_tensor(im["difficult"])}
    return StubModel(canned, lambda o: {0: o}, flip), loader, base_ds, canned


def voc_expected(images, C, canned, batch, k=300):
    """The VOC meter fed by hand with detect_ref's detections of the canned outputs -> (summary, the kept detections per image)."""
    from spe_amd.evalmetrics import VOCDetectionMeter
    m = VOCDetectionMeter(num_classes=C)
    kept = []
    sizes = torch.full((batch, 2), float(FRAME))
    for i, out in zip(range(0, len(images), batch), canned):
        ims = images[i:i + batch]
        res = dr.results_of(dr.detect_ref(out["pred_logits"], out["pred_boxes"], sizes[:len(ims)], k, 0.5))
        kept += res
        m.update(res, [{"boxes": torch.as_tensor(im["gt_boxes"]), "labels": torch.as_tensor(im["gt_labels"]),
                        "difficult": torch.as_tensor(im["difficult"]), "image_id": int(im["image_id"])} for im in ims])
    return m, kept


# ---- COCO --------------------------------------------------------------------------------------------------------------------------
def coco_run(images, batch, Q=100, Kc=92, device="cpu", seed=0):
    """-> (model, criterion, loader, base_ds, canned): the arguments of evaluate_refinements (refine_stage 1)."""
    g = torch.Generator().manual_seed(seed)
    canned, loader, base_ds = [], [], {}
    for i in range(0, len(images), batch):
        ims = images[i:i + batch]
        canned.append(encode(ims, Q, Kc))
        targets = [{"image_id": torch.tensor([int(im["image_id"])]), "orig_size": torch.tensor([FRAME, FRAME])} for im in ims]
        loader.append((samples_of(len(ims), g), targets))
    for im in images:
        base_ds[int(im["image_id"])] = {"boxes": torch.as_tensor(im["gt_boxes"]), "labels": torch.as_tensor(im["gt_labels"]),
                                        "iscrowd": torch.as_tensor(im["iscrowd"]), "area": torch.as_tensor(im["area"])}
    wrong = {"pred_logits": torch.zeros(1, 1, 1), "pred_boxes": torch.zeros(1, 1, 4)}
    model = StubModel(canned, lambda o: {0: {"aux_outputs": [wrong]}, 1: {**wrong, "aux_outputs": [wrong, o]}})
    return model, StubCriterion(), loader, base_ds, canned


def coco_expected(images, cat_ids, canned, batch, k=100):
    from spe_amd.evalmetrics import COCODetectionMeter
    m = COCODetectionMeter(cat_ids)
    sizes = torch.full((batch, 2), float(FRAME))
    for i, out in zip(range(0, len(images), batch), canned):
        ims = images[i:i + batch]
        res = dr.results_of(dr.detect_ref(out["pred_logits"], out["pred_boxes"], sizes[:len(ims)], k, 0.5))
        m.update(res, [{"boxes": torch.as_tensor(im["gt_boxes"]), "labels": torch.as_tensor(im["gt_labels"]),
                        "iscrowd": torch.as_tensor(im["iscrowd"]), "area": torch.as_tensor(im["area"]), "image_id": int(im["image_id"])}
                       for im in ims])
    return m
