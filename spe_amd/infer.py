"""Inference-side post-processing of the SPE detector: the tensor work of
reference engine_loc.py:99-124 (`decouple_output`, flip test-time augmentation) and engine_loc.py:150-174
(`postprocessors['bbox'](outputs, sizes, 300)` followed by per-class torchvision NMS at IoU 0.5).

`per_class_nms` takes PostProcess's list; `detect` is the two steps in one HIP launch without a host read (csrc/detect.hip), which is
what the evaluation loops of spe_amd.engine call.  CUDA tensors take the kernels; CPU tensors take the same rules composed of torch /
numpy operations (the pattern of spe_amd.evalmetrics), which is what the host logic is tested with.
"""
import numpy as np
import torch

from . import kernels as K
from .util import box_ops

_COMBINE = ("pred_logits", "pred_boxes", "x_logits", "x_cls_logits", "cams_cls", "aux_outputs")


def decouple_output(output, bs=2):
    """Merge the outputs of a [images ; horizontally flipped images] batch (engine_loc.py:99-124): flipped boxes get
    cx -> 1 - cx, image-level logits take the element-wise maximum, everything else is concatenated along the query
    axis, recursively for `aux_outputs`.  In place on the dict, like the reference; tensors are not aliased."""
    for k in _COMBINE:
        if k not in output:
            continue
        v = output[k]
        if k == "aux_outputs":
            for i, aux in enumerate(v):
                v[i] = decouple_output(aux, bs=bs)
            continue
        pre, pos = v[:bs], v[bs:2 * bs]
        if k == "pred_boxes":
            pos = pos.clone()
            pos[..., 0] = 1 - pos[..., 0]
        if k in ("x_logits", "x_cls_logits"):
            output[k] = torch.maximum(pre, pos)
            continue
        output[k] = torch.cat((pre, pos), dim=1)
    return output


@torch.no_grad()
def per_class_nms(results, iou_threshold=0.5):
    """results: list (one per image) of {'scores' [n], 'labels' [n], 'boxes' [n,4] xyxy} as returned by PostProcess.
    Returns the list the reference builds at engine_loc.py:154-174: for every predicted class in ascending order the
    NMS survivors in descending score order.  One sort + one HIP launch for the whole batch, no per-class host loop (CPU tensors: the
    same order and a numpy restatement of the launch).  The boolean-mask indexing at the end reads back from the device, three times per
    image; `detect` below does not."""
    if not results:
        return results
    n = results[0]["scores"].numel()
    assert all(r["scores"].numel() == n for r in results), "PostProcess returns the same count for every image"
    scores = torch.stack([r["scores"] for r in results]).float()
    labels = torch.stack([r["labels"] for r in results]).long()
    boxes = torch.stack([r["boxes"] for r in results]).float()
    # order by (label asc, score desc): stable sort by score first, then stable sort by label
    o1 = torch.sort(scores, dim=1, descending=True, stable=True).indices
    o2 = torch.sort(labels.gather(1, o1), dim=1, stable=True).indices
    order = o1.gather(1, o2)
    sl = labels.gather(1, order).contiguous()
    sb = boxes.gather(1, order[..., None].expand(-1, -1, 4)).contiguous()
    ss = scores.gather(1, order)
    keep = K.nms_sorted(sb, sl, iou_threshold) if sb.is_cuda else _nms_sorted_host(sb, sl, iou_threshold)
    out = []
    for i in range(len(results)):
        m = keep[i]
        out.append({"scores": ss[i][m], "labels": sl[i][m], "boxes": sb[i][m]})
    return out


def _nms_sorted_host(boxes, labels, iou_threshold):
    """kernels.nms_sorted on CPU tensors: the same visit order and the same fp32 arithmetic, one rounding per operation (numpy)."""
    bx, lb = boxes.numpy(), labels.numpy()
    I, n = lb.shape
    keep = np.ones((I, n), dtype=bool)
    thr = np.float32(iou_threshold)
    with np.errstate(invalid="ignore", divide="ignore"):
        for img in range(I):
            b, l = bx[img], lb[img]
            assert (np.diff(l) >= 0).all(), "detections must be ordered by label"
            end = np.searchsorted(l, l, side="right")                           # one past the last detection of the label
            area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
            for i in range(n):
                if not keep[img, i] or i + 1 >= end[i]:
                    continue
                s = slice(i + 1, end[i])
                w = np.maximum(np.minimum(b[i, 2], b[s, 2]) - np.maximum(b[i, 0], b[s, 0]), np.float32(0))
                h = np.maximum(np.minimum(b[i, 3], b[s, 3]) - np.maximum(b[i, 1], b[s, 1]), np.float32(0))
                inter = w * h
                keep[img, s] &= ~(inter / (area[i] + area[s] - inter) > thr)
    return torch.from_numpy(keep)


# ---- the detection head: PostProcess + per_class_nms in one launch (csrc/detect.hip) ---------------------------
def select_key(logits):
    """The order the head selects by, as int64: an order-preserving image of the fp32 logit in which -0.0 counts as +0.0 and every NaN
    lies above +inf (torch.topk's order).  Greater key = better; equal keys are taken in ascending flat index."""
    u = logits.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    u = torch.where(u == 0x80000000, torch.zeros_like(u), u)
    key = torch.where((u & 0x80000000) != 0, ~u & 0xFFFFFFFF, u | 0x80000000)
    return torch.where(nan, torch.full_like(u, 0xFFFFFFFF), key)


def _detect_host(logits, boxes, sizes, k, iou_threshold, nms):
    """kernels.detect on CPU tensors, composed of torch operations: the same selection rule, PostProcess's box arithmetic, the order and
    the suppression of per_class_nms.  The same five results, and the scores as a sixth."""
    B, Q, Kc = logits.shape
    if k < 1 or k > Q * Kc:
        raise ValueError(f"detect: k = {k} out of range for {Q * Kc} = {Q} x {Kc} scores per image")
    if k > K.DETECT_MAX_K or Q * Kc > K.DETECT_MAX_N:
        raise ValueError(f"detect: at most k = {K.DETECT_MAX_K} of at most {K.DETECT_MAX_N} scores per image")
    flat = logits.reshape(B, -1)
    idx = torch.sort(select_key(flat), dim=1, descending=True, stable=True).indices[:, :k]
    query, label = torch.div(idx, Kc, rounding_mode="floor"), idx % Kc
    xyxy = box_ops.box_cxcywh_to_xyxy(boxes).clamp(min=0)
    xyxy = torch.gather(xyxy, 1, query.unsqueeze(-1).repeat(1, 1, 4))
    img_h, img_w = sizes.unbind(1)
    xyxy = xyxy * torch.stack([img_w, img_h, img_w, img_h], dim=1)[:, None, :]
    order = torch.sort(label, dim=1, stable=True).indices                      # the list is score-descending already
    label, query = label.gather(1, order), query.gather(1, order)
    logit = flat.gather(1, idx).gather(1, order)
    # PostProcess's own scores: out of the sigmoid of the whole tensor (ATen's CPU sigmoid of a short tensor can differ in the last bit)
    score = logits.sigmoid().reshape(B, -1).gather(1, idx).gather(1, order)
    xyxy = xyxy.gather(1, order[..., None].expand(-1, -1, 4)).contiguous()
    keep = _nms_sorted_host(xyxy, label, iou_threshold) if nms else torch.ones((B, k), dtype=torch.bool)
    front = torch.sort((~keep).to(torch.uint8), dim=1, stable=True).indices     # survivors first, in their order
    keep = keep.gather(1, front)
    out_logit = torch.where(keep, logit.gather(1, front), torch.full_like(logit, float("-inf")))
    out_label = torch.where(keep, label.gather(1, front), torch.full_like(label, -1))
    out_query = torch.where(keep, query.gather(1, front), torch.full_like(query, -1)).to(torch.int32)
    out_box = torch.where(keep[..., None], xyxy.gather(1, front[..., None].expand(-1, -1, 4)), torch.zeros_like(xyxy))
    out_score = torch.where(keep, score.gather(1, front), torch.zeros_like(score))
    return out_logit, out_label, out_box, out_query, keep.sum(1).to(torch.int32), out_score


class Detections:
    """What `detect` returns: per image k rows, the `counts[i]` detections in front - (label ascending, score descending), the order of
    per_class_nms - and a tail of score 0, label -1, box 0, query -1.  All members are tensors on the device of the inputs.

    scores [B,k] (on the device torch.sigmoid of the selected logits, one ATen launch, so bitwise PostProcess's value of that element;
    the host path hands in PostProcess's own values), logits [B,k], labels [B,k] int64, boxes [B,k,4] xyxy in absolute pixels, queries
    [B,k] int32 (the source query of every row), counts [B] int32."""

    def __init__(self, logits, labels, boxes, queries, counts, scores=None):
        self.logits, self.labels, self.boxes, self.queries, self.counts = logits, labels, boxes, queries, counts
        self.scores = torch.sigmoid(logits) if scores is None else scores       # the tail: sigmoid(-inf) = 0

    def padded(self):
        """One dict {'scores','labels','boxes'} per image: views with exactly k rows, no host read.  Both detection meters drop labels
        outside their range, so the list goes straight into `meter.update()`."""
        return [{"scores": s, "labels": l, "boxes": b} for s, l, b in zip(self.scores, self.labels, self.boxes)]

    def results(self):
        """The list the reference's loops build (per_class_nms's), trimmed to `counts`: ONE host copy of the B counts."""
        return [{"scores": s[:c], "labels": l[:c], "boxes": b[:c]}
                for s, l, b, c in zip(self.scores, self.labels, self.boxes, self.counts.tolist())]


@torch.no_grad()
def detect(outputs, target_sizes, keep_queries=100, iou_threshold=0.5, nms=True):
    """outputs: {'pred_logits' [B,Q,Kc], 'pred_boxes' [B,Q,4]}; target_sizes [B,2] (h, w) -> Detections.  With nms=True `.results()` is
    per_class_nms(PostProcess()(outputs, target_sizes, keep_queries), iou_threshold); with nms=False it is PostProcess's list in
    (label, score) order.  Equal scores are taken in ascending (query, class) order, where torch.topk promises nothing.  On the device:
    one HIP launch plus the sigmoid of the [B,k] selected logits, no host read; CPU tensors take the same rules composed of torch
    operations."""
    logits, boxes = outputs["pred_logits"], outputs["pred_boxes"]
    assert len(logits) == len(target_sizes) and target_sizes.shape[1] == 2
    logits, boxes = logits.float().contiguous(), boxes.float().contiguous()
    sizes = target_sizes.to(device=logits.device, dtype=torch.float32).contiguous()
    if logits.is_cuda:
        return Detections(*K.detect(logits, boxes, sizes, keep_queries, iou_threshold, nms))
    return Detections(*_detect_host(logits, boxes, sizes, int(keep_queries), iou_threshold, nms))


# ---- the stage k+1 training targets: PostProcessRefine's picks in one launch (csrc/train_targets.hip) ------------
class ClassTable:
    """The class ids PostProcessRefine picks for, per image sorted and below Kc, in the forms the pick needs: `lists` (host), `off`
    (host offsets [B + 1]), and on the device `labels` int64 [U], `cls` int32 [U], `cls_off` int32 [B + 1] - ONE pinned upload, made
    once per step and shared by the refinement stages.  `host` is None for a table gathered from device tensors (nobody has seen its
    values on the host: the library cannot check them)."""

    def __init__(self, lists, device):
        self.lists = [[int(c) for c in l] for l in lists]
        self.off = [0]
        for l in self.lists:
            self.off.append(self.off[-1] + len(l))
        U, B = self.off[-1], len(self.lists)
        flat = np.array([c for l in self.lists for c in l], np.int64)
        self.host = (flat.astype(np.int32), np.array(self.off, np.int32))
        self.device = torch.device(device)
        if self.device.type == "cuda":
            raw = K.host_table(np.concatenate([flat.view(np.uint8), self.host[0].view(np.uint8), self.host[1].view(np.uint8)]), device)
            self._raw = raw
            self.labels = raw[:8 * U].view(torch.int64)
            self.cls, self.cls_off = raw[8 * U:12 * U].view(torch.int32), raw[12 * U:12 * U + 4 * (B + 1)].view(torch.int32)
        else:
            self.labels = torch.from_numpy(flat)
            self.cls = self.cls_off = None

    def per_image(self):
        """One int64 view per image on the device: what a target dict carries as 'labels_unique'.  Every view knows its table."""
        out = []
        for b in range(len(self.lists)):
            v = self.labels[self.off[b]:self.off[b + 1]]
            v._spe_class_table = (self, b)
            out.append(v)
        return out

    @classmethod
    def of(cls, labs, device):
        """The table behind a batch's 'labels_unique' tensors: the one they are views of, or a new one - from host tensors by value, from
        device tensors gathered on the device (two launches, no host read, no host check)."""
        tags = [getattr(l, "_spe_class_table", None) for l in labs]
        if tags and all(t is not None and t[0] is tags[0][0] and t[1] == b for b, t in enumerate(tags)) \
                and len(tags) == len(tags[0][0].lists) and tags[0][0].device == torch.device(device):
            return tags[0][0]
        if not any(l.is_cuda for l in labs):
            return cls([l.reshape(-1).tolist() for l in labs], device)
        self = cls.__new__(cls)
        self.lists = self.host = None
        self.off = [0]
        for l in labs:
            self.off.append(self.off[-1] + l.numel())
        self.device = torch.device(device)
        self.labels = torch.cat([l.reshape(-1).to(device=device, dtype=torch.int64) for l in labs]) if labs else torch.zeros((0,), dtype=torch.int64, device=device)
        self.cls = self.labels.to(torch.int32)
        key = (self.device, tuple(self.off))
        if key not in _OFFSET_TABLES:                    # a loader's batches repeat a few size patterns: one upload each
            if len(_OFFSET_TABLES) >= 256:
                _OFFSET_TABLES.clear()
            _OFFSET_TABLES[key] = K.host_table(np.array(self.off, np.int32).view(np.uint8), device).view(torch.int32)
        self.cls_off = _OFFSET_TABLES[key]
        return self


_OFFSET_TABLES = {}         # (device, offsets) -> the offsets on the device, for the tables gathered from device tensors


def _refine_pick_host(prob, boxes, table):
    """kernels.refine_pick on CPU tensors: torch.max's own pick per image and the three gathers of PostProcessRefine."""
    top_values, top_indexes = torch.max(prob, dim=1)
    B, Kc = top_values.shape
    lab = table.labels
    if lab.numel() and (int(lab.min()) < 0 or int(lab.max()) >= Kc):
        raise ValueError(f"refine_targets: class ids must lie in [0, {Kc})")
    img = torch.repeat_interleave(torch.arange(B), torch.tensor([table.off[b + 1] - table.off[b] for b in range(B)], dtype=torch.long))
    q = top_indexes[img, lab]
    return top_values[img, lab], q.to(torch.int32), boxes[img, q]


@torch.no_grad()
def refine_targets(outputs, classes):
    """outputs: {'pred_logits' [B, Q, Kc], 'pred_boxes' [B, Q, 4]}; classes: per image the sorted class ids below Kc (host lists) or a
    ClassTable -> {'scores' [U], 'labels' [U] int64, 'boxes' [U, 4] normalised cxcywh, 'queries' [U] int32, 'offsets' host list [B + 1]}:
    PostProcessRefine's per-image results, flat - for every class of an image the best query by torch.max's rule over the probabilities
    (the sigmoid ATen computes, one launch: bitwise PostProcessRefine's scores), equal probabilities to the lowest query, the first NaN
    before everything.  On the device: the sigmoid and ONE HIP launch, no host read; CPU tensors take torch.max and the gathers."""
    logits, boxes = outputs["pred_logits"], outputs["pred_boxes"]
    table = classes if isinstance(classes, ClassTable) else ClassTable(classes, logits.device)
    if len(table.off) != logits.shape[0] + 1:
        raise ValueError(f"refine_targets: {len(table.off) - 1} class lists for {logits.shape[0]} images")
    prob = logits.sigmoid()
    if logits.is_cuda:
        scores, queries, picked = K.refine_pick(prob.float().contiguous(), boxes.float().contiguous(), table.cls, table.cls_off, host=table.host)
    else:
        scores, queries, picked = _refine_pick_host(prob, boxes, table)
    return {"scores": scores, "labels": table.labels, "boxes": picked, "queries": queries, "offsets": table.off}


# ---- pseudo labels as detector output (reference engine_loc.py:204-220) --------------------------------------------------------------------
@torch.no_grad()
def pseudo_label_to_det_out(pseudo_label, target_sizes):
    """Same signature and result as engine_loc.py:204-220: per image {'scores', 'labels', 'boxes'} with the pseudo boxes as xyxy in absolute
    pixels - box_cxcywh_to_xyxy, clamp(min=0), times [w, h, w, h] of target_sizes [B, 2] (h, w) - and a score of 1 for every row, in the
    labels' INTEGER dtype, as the reference has it.  The list goes into VOCDetectionMeter.update() like a detector's; an ATen composition,
    no kernel.  For counting hits while training runs see evalmetrics.PseudoLabelMeter."""
    assert target_sizes.shape[1] == 2
    results = []
    for p, size in zip(pseudo_label, target_sizes):
        img_h, img_w = size
        scale = torch.stack([img_w, img_h, img_w, img_h], dim=0).unsqueeze(0)
        boxes = box_ops.box_cxcywh_to_xyxy(p["boxes"]).clamp(min=0) * scale
        results.append({"scores": torch.ones_like(p["labels"]), "labels": p["labels"], "boxes": boxes})
    return results
