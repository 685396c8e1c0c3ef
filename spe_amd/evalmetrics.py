"""Metrics of the SPE evaluation loops, kept on the device: the two detection meters and, at the end of the file, the multi-label
classification AP of the image-level logits (`ClassificationAPMeter`: reference cams_deit.py:493-574; `spe_cls_ap`)
and the meters of the TRAINING loops: the quality of their pseudo labels (`PseudoLabelMeter`; `spe_pseudo_quality`; section 8o) and the
recall of a stage's query boxes before the pick (`ProposalRecallMeter`; `spe_proposal_recall`; section 8p).

PASCAL VOC: the last step of reference
`engine_loc.evaluate_det_voc` (engine_loc.py:176-197), i.e. `evaluate_detections` -> `voc_eval` (datasets/voc_voc.py:366-437,
datasets/voc_eval.py) for AP / mAP and `evaluate_discovery` -> `dis_eval` (voc_voc.py:454-488, datasets/dis_eval.py) for CorLoc.

The reference writes every detection to per-class text files, parses them and the XML annotations back and walks one global,
score-sorted list per class in Python.  Whether a detection is a true or a false positive depends only on the detections of the same
image and class before it, so here the greedy matching runs per batch, straight after `infer.per_class_nms`
(`spe_voc_match`: one wave per (image, class)), only flags, scores and integer counters are kept, and `summarize()` is one sort and
one launch (`spe_voc_ap`: one workgroup per class).  DESIGN.md section 8g has the decomposition, the tie rule and the argument for the
decimal round trip.

COCO: the last step of reference `engine.evaluate` / `evaluate_refinements` (`CocoEvaluator.update`, `accumulate`, `summarize` of
datasets/coco_eval.py, i.e. COCOeval for 'bbox').  The same decomposition: `COCODetectionMeter` matches per batch
(`spe_coco_match`), keeps flag words, ranks and one integer counter, and builds the precision / recall tables once
(`spe_coco_accumulate`).  DESIGN.md section 8i.

What the two have in common - record columns, the single upload of a batch, the batch and curve orders, the process-group merge -
is `_DetectionMeter`; the matching rules, the host restatements and the result builders are each meter's own.

CUDA tensors take the HIP kernels; CPU tensors take a numpy composition of the same rules (the pattern of
models/conditional_detr.jitter_targets), which is what the host logic, the goldens and the process-group merge are tested with.
"""
import numpy as np
import torch

from . import kernels as K

_SCORE_SCALE, _COORD_SCALE = 1000.0, 10.0      # '{:.3f}' / '{:.1f}' of voc_voc.py:383-386


def _overlaps(det, gt):
    """One detection [4] against ground truth [g,4] in fp64, the operation order of voc_eval.py:169-182 (what csrc/voc_eval.hip does)."""
    w = np.maximum(np.minimum(gt[:, 2], det[2]) - np.maximum(gt[:, 0], det[0]) + 1., 0.)
    h = np.maximum(np.minimum(gt[:, 3], det[3]) - np.maximum(gt[:, 1], det[1]) + 1., 0.)
    inter = w * h
    return inter / ((det[2] - det[0] + 1.) * (det[3] - det[1] + 1.) + (gt[:, 2] - gt[:, 0] + 1.) * (gt[:, 3] - gt[:, 1] + 1.) - inter)


def _match_host(det_boxes, det_scores, det_labels, det_off, gt_boxes, gt_labels, gt_difficult, gt_off, max_det, max_gt,
                ovthresh, score_scale, coord_scale, npos, nimgs, hits):
    """kernels.voc_match on CPU tensors (same arguments, same results, same limits)."""
    if max_det > K.VOC_MAX_DET or max_gt > K.VOC_MAX_GT:
        raise ValueError(f"at most {K.VOC_MAX_DET} detections and {K.VOC_MAX_GT} ground-truth boxes per image")
    C = npos.numel()
    s64 = det_scores.numpy().astype(np.float64)
    qs = np.rint(s64 * score_scale) / score_scale if score_scale else s64
    if coord_scale:
        bx = np.rint((det_boxes.numpy() + np.float32(1.0)).astype(np.float64) * coord_scale) / coord_scale
    else:
        bx = det_boxes.numpy().astype(np.float64) + 1.0
    lab, doff = det_labels.numpy(), det_off.numpy()
    gb, gl, gd, goff = gt_boxes.numpy(), gt_labels.numpy(), gt_difficult.numpy().astype(bool), gt_off.numpy()
    flags = np.zeros(lab.shape[0], dtype=np.uint8)
    cnt = np.zeros((3, C), dtype=np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(doff.shape[0] - 1):
            d0, d1, g0, g1 = doff[i], doff[i + 1], goff[i], goff[i + 1]
            for c in range(C):
                g = np.nonzero(gl[g0:g1] == c + 1)[0] + g0
                cnt[0, c] += int((~gd[g]).sum())
                cnt[1, c] += int(g.size > 0)
                used = np.zeros(g.size, dtype=bool)
                d = np.nonzero(lab[d0:d1] == c + 1)[0] + d0
                for k, j in enumerate(d):
                    ovmax, jmax = -np.inf, -1
                    if g.size:
                        ov = _overlaps(bx[j], gb[g])
                        ovmax, jmax = np.max(ov), int(np.argmax(ov))
                    over = bool(ovmax > ovthresh)
                    if k == 0 and over:
                        cnt[2, c] += 1
                    if not over or (not gd[g[jmax]] and used[jmax]):
                        flags[j] = 2
                    elif not gd[g[jmax]]:
                        flags[j], used[jmax] = 1, True
    npos += torch.from_numpy(cnt[0]); nimgs += torch.from_numpy(cnt[1]); hits += torch.from_numpy(cnt[2])
    return torch.from_numpy(flags), torch.from_numpy(qs)


def _ap_host(flags, seg_off, npos, want_curve):
    """kernels.voc_ap on CPU tensors."""
    fl, off, C = flags.numpy(), seg_off.numpy(), npos.numel()
    ap07, area = np.zeros(C), np.zeros(C)
    rec_all, prec_all = np.zeros(fl.shape[0]), np.zeros(fl.shape[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in range(C):
            f = fl[off[c]:off[c + 1]]
            tp, fp = np.cumsum((f == 1).astype(np.float64)), np.cumsum((f == 2).astype(np.float64))
            rec = tp / float(npos[c])
            prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
            rec_all[off[c]:off[c + 1]], prec_all[off[c]:off[c + 1]] = rec, prec
            ap = 0.
            for t in np.arange(0., 1.1, 0.1):
                p = np.max(prec[rec >= t]) if np.sum(rec >= t) else 0.
                ap = ap + p / 11.
            ap07[c] = ap
            mrec, mpre = np.concatenate(([0.], rec, [1.])), np.concatenate(([0.], prec, [0.]))
            mpre = np.maximum.accumulate(mpre[::-1])[::-1]
            i = np.where(mrec[1:] != mrec[:-1])[0]
            area[c] = np.cumsum((mrec[i + 1] - mrec[i]) * mpre[i + 1])[-1]         # a fixed, sequential order
    t = torch.from_numpy
    return t(ap07), t(area), (t(rec_all) if want_curve else None), (t(prec_all) if want_curve else None)


def _all_gather_rows(t, world, group):
    """Rows of every rank, concatenated in rank order (the counts differ: pad to the largest)."""
    import torch.distributed as dist
    n = torch.tensor([t.shape[0]], dtype=torch.int64, device=t.device)
    ns = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(ns, n, group=group)
    ns = [int(x) for x in ns]
    pad = torch.zeros((max(max(ns), 1),) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    pad[:t.shape[0]] = t
    outs = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(outs, pad, group=group)
    return torch.cat([o[:k] for o, k in zip(outs, ns)])


class _DetectionMeter:
    """What the two meters share: the record columns, the single host -> device copy of a batch, the two orders (of a batch, of the
    curves) and the process-group merge.  A subclass declares _SCHEMA (record column -> (dtype, trailing shape)) and _MAX_GT, provides
    _start(dev) - the first use of a device: self._device and the int32 counter tensor self._counters - and keeps its own matching and
    its own result builder."""
    _SCHEMA, _MAX_GT = {}, 0

    def reset(self):
        self._device = None
        self._n, self._cols = 0, None          # records: capacity-sized tensors, the first _n rows valid
        self._ids = []                         # image ids of every update (images without detections included)
        self._counters = None                  # int32, on the device: what merge() all-reduces
        self._merged = False

    def _records(self):
        """The valid rows of every column (views; empty columns before the first record)."""
        if self._cols is None:
            return {k: torch.empty((0,) + shape, dtype=dt, device=self._device) for k, (dt, shape) in self._SCHEMA.items()}
        return {k: self._cols[k][:self._n] for k in self._SCHEMA}

    def _append(self, new):
        n = new[next(iter(self._SCHEMA))].shape[0]
        if self._cols is None or self._n + n > next(iter(self._cols.values())).shape[0]:
            cap, old = max(2 * (self._n + n), 4096), self._cols               # geometric growth
            self._cols = {k: torch.empty((cap,) + shape, dtype=dt, device=self._device) for k, (dt, shape) in self._SCHEMA.items()}
            for k, v in (old or {}).items():
                self._cols[k][:self._n] = v[:self._n]
        for k in self._SCHEMA:
            self._cols[k][self._n:self._n + n] = new[k]
        self._n += n

    def _collect(self, results, gts, gt_fields, pos=False):
        """The checks of update(), the concatenations and the ONE copy (from pinned memory, asynchronous on the device path) of what the
        host knows from the shapes - offsets, the image of every row, with `pos` its position inside the image - and of the image ids.
        gt_fields: ground-truth key -> torch.uint8 (a flag) or torch.float64.  -> None for an empty batch, else the named tensors."""
        name = type(self).__name__
        if self._merged:
            raise RuntimeError(f"{name}: update() after merge(); reset() first")
        if len(results) != len(gts):
            raise ValueError(f"{name}.update: one ground-truth dict per result")
        if not results:
            return None
        dev = results[0]["scores"].device
        if self._device is None:
            self._start(dev)
        elif dev != self._device:
            raise ValueError(f"{name}: tensors on {dev}, earlier updates on {self._device}")
        nd = [int(r["scores"].shape[0]) for r in results]                       # host lengths: the shapes we are handed
        ng = [int(g["labels"].shape[0]) for g in gts]
        if max(nd) > K.MAX_DET or max(ng) > self._MAX_GT:
            raise ValueError(f"at most {K.MAX_DET} detections and {self._MAX_GT} ground-truth boxes per image")
        b = {"max_det": max(nd), "max_gt": max(ng),
             "scores": torch.cat([r["scores"].reshape(-1) for r in results]).float(),
             "labels": torch.cat([r["labels"].reshape(-1) for r in results]).long(),
             "boxes": torch.cat([r["boxes"].reshape(-1, 4) for r in results]).float(),
             "gboxes": torch.cat([g["boxes"].reshape(-1, 4) for g in gts]).to(dev, torch.float64).contiguous(),
             "glabels": torch.cat([g["labels"].reshape(-1) for g in gts]).to(dev, torch.int64)}
        for k, dt in gt_fields.items():
            v = torch.cat([g[k].reshape(-1) for g in gts])
            b[k] = v.to(dev).ne(0).to(torch.uint8) if dt == torch.uint8 else v.to(dev, dt).contiguous()
        ids = [g["image_id"] for g in gts]
        ids_dev = None
        if any(torch.is_tensor(i) for i in ids):
            ids_dev, ids = torch.stack([torch.as_tensor(i).reshape(()).to(dev, torch.int64) for i in ids]), []
        parts = {"det_off": np.concatenate([[0], np.cumsum(nd)]), "gt_off": np.concatenate([[0], np.cumsum(ng)]),
                 "img": np.repeat(np.arange(len(nd)), nd)}
        if pos:
            parts["pos"] = np.concatenate([np.arange(n) for n in nd])
        parts["ids"] = ids
        host = torch.from_numpy(np.concatenate(list(parts.values())).astype(np.int64))
        if dev.type == "cuda":
            host = host.pin_memory().to(dev, non_blocking=True)
        b.update(zip(parts, host.split([len(p) for p in parts.values()])))
        for k in ("det_off", "gt_off") + (("pos",) if pos else ()):
            b[k] = b[k].to(torch.int32)
        if ids_dev is not None:
            b["ids"] = ids_dev
        self._ids.append(b["ids"])
        return b

    @staticmethod
    def _order_batch(scores, img, cls, nkeys):
        """(cls ascending, score descending) inside every image, equal scores in incoming order; per_class_nms output already is."""
        o1 = torch.sort(scores, descending=True, stable=True).indices
        o2 = torch.sort(img[o1] * nkeys + cls[o1], stable=True).indices
        return o1[o2]

    def merge(self, group=None):
        """Gather the records of every rank and all-reduce the counters: afterwards every rank summarizes the whole run.  A no-op
        without an initialised process group."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        if self._merged:
            raise RuntimeError(f"{type(self).__name__}: merge() called twice; reset() first")
        if self._device is None:                                                # a rank that saw no image
            self._start(torch.device("cuda" if dist.get_backend(group) == "nccl" else "cpu"))
        dev, world = self._device, dist.get_world_size(group)
        self._cols = {k: _all_gather_rows(v, world, group) for k, v in self._records().items()}
        self._n = next(iter(self._cols.values())).shape[0]
        self._ids = [_all_gather_rows(torch.cat(self._ids) if self._ids else torch.empty((0,), dtype=torch.int64, device=dev), world, group)]
        dist.all_reduce(self._counters, group=group)
        self._merged = True

    def _check_run(self):
        if self._counters is None:
            raise RuntimeError(f"{type(self).__name__}.summarize: nothing accumulated")
        ids = torch.sort(torch.cat(self._ids)).values
        if bool((ids[1:] == ids[:-1]).any()):
            raise ValueError(f"{type(self).__name__}: an image id was accumulated twice")

    def _curve_order(self, keys, ngroups, want):
        """Curve order by stable sorts, last key first (keys[-1]: the class / category, then 'score' descending, then the rest ascending).
        -> (the columns `want` in that order, seg_off int32 [ngroups + 1]); records of group `ngroups` (dropped ones) lie behind."""
        col = self._records()
        o = torch.sort(col[keys[0]], stable=True).indices
        for k in keys[1:]:
            o = o[torch.sort(col[k][o], descending=k == "score", stable=True).indices]
        col = {k: col[k][o].contiguous() for k in want}
        return col, torch.searchsorted(col[keys[-1]], torch.arange(ngroups + 1, device=self._device)).to(torch.int32)


class VOCDetectionMeter(_DetectionMeter):
    """Accumulates VOC AP / mAP and CorLoc over an evaluation run.

        m = VOCDetectionMeter(num_classes=20, ovthresh=0.5, file_roundtrip=True)
        m.update(results, gts)     # per batch, straight after per_class_nms
        m.merge()                  # once, when the images were split over ranks
        out = m.summarize(use_07_metric=True)

    results: the list `infer.per_class_nms` returns - per image {'scores' [n], 'labels' [n] (1 .. num_classes; anything else is
    dropped like engine_loc.py:184 drops 0), 'boxes' [n,4] xyxy in 0-based pixels}.  gts: per image {'boxes' [g,4] in the annotation
    frame (the XML's integer pixel coordinates), 'labels' [g], 'difficult' [g], 'image_id' (int or 0-d tensor)}.

    file_roundtrip=True reproduces the reference's numbers: its evaluator reads scores and boxes back from text files written with
    '{:.3f}' and, after + 1, '{:.1f}'.  False matches on the raw fp32 scores and double(x) + 1.0.

    Inside an (image, class) the detections are matched in descending score, equal scores in their incoming order.  The curve of a
    class is ordered by score descending, then image_id ascending, then the position inside the image - the order of the reference's
    result file - so the numbers do not depend on batch order or on how the images were split over ranks.  update() does not read
    device data on the host."""

    def __init__(self, num_classes=20, ovthresh=0.5, file_roundtrip=True):
        self.num_classes, self.ovthresh, self.file_roundtrip = int(num_classes), float(ovthresh), bool(file_roundtrip)
        self.reset()

    _SCHEMA = {"score": (torch.float64, ()), "flag": (torch.uint8, ()), "cls": (torch.int64, ()), "img": (torch.int64, ()),
               "ord": (torch.int32, ())}
    _MAX_GT = K.VOC_MAX_GT

    def _start(self, dev):
        self._device, self._counters = dev, torch.zeros((3, self.num_classes), dtype=torch.int32, device=dev)      # npos, nimgs, hits

    @torch.no_grad()
    def update(self, results, gts):
        b = self._collect(results, gts, {"difficult": torch.uint8}, pos=True)
        if b is None:
            return
        C, labels = self.num_classes, b["labels"]
        # labels outside 1 .. C gather at the two ends of the image
        cls = torch.where((labels >= 1) & (labels <= C), labels, torch.where(labels < 1, 0, C + 1))
        order = self._order_batch(b["scores"], b["img"], cls, C + 2)
        scores, cls, boxes = b["scores"][order].contiguous(), cls[order].contiguous(), b["boxes"][order].contiguous()
        match = K.voc_match if self._device.type == "cuda" else _match_host
        ss, cs = (_SCORE_SCALE, _COORD_SCALE) if self.file_roundtrip else (0.0, 0.0)
        flags, qscores = match(boxes, scores, cls, b["det_off"], b["gboxes"], b["glabels"], b["difficult"], b["gt_off"], b["max_det"],
                               b["max_gt"], self.ovthresh, ss, cs, self._counters[0], self._counters[1], self._counters[2])
        self._append({"score": qscores, "flag": flags, "cls": torch.where(cls == 0, C + 1, cls) - 1, "img": b["ids"][b["img"]],
                      "ord": b["pos"]})

    @torch.no_grad()
    def summarize(self, use_07_metric=True, return_curves=False):
        """-> {'ap' [C] (the 11-point metric or the area), 'ap07' [C], 'ap_area' [C], 'map', 'corloc' [C], 'mean_corloc', 'npos' [C],
        'nimgs' [C]}: fp64 / int32 CPU tensors and floats; a class without ground-truth images has corloc NaN and one with detections
        but no non-difficult ground truth has area AP NaN, as in the reference, and the means propagate them (np.mean).
        return_curves adds 'rec', 'prec', 'flags': per class, in curve order."""
        C = self.num_classes
        self._check_run()
        # class, score descending, image id, position inside the image; dropped labels (class C) lie behind
        col, seg_off = self._curve_order(("ord", "img", "score", "cls"), C, ("flag", "cls"))
        flags = col["flag"]
        npos = self._counters[0].contiguous()
        ap = K.voc_ap if self._device.type == "cuda" else _ap_host
        ap07, area, rec, prec = ap(flags, seg_off, npos, return_curves)
        cnt = self._counters.cpu().numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            corloc = cnt[2].astype(np.float64) / cnt[1].astype(np.float64)
        ap07, area = ap07.cpu(), area.cpu()
        chosen = ap07 if use_07_metric else area
        out = {"ap": chosen, "ap07": ap07, "ap_area": area, "map": float(np.mean(chosen.numpy())),
               "corloc": torch.from_numpy(corloc), "mean_corloc": float(np.mean(corloc)),
               "npos": torch.from_numpy(cnt[0].copy()), "nimgs": torch.from_numpy(cnt[1].copy())}
        if return_curves:
            off = seg_off.cpu().tolist()
            rec, prec, flags = rec.cpu(), prec.cpu(), flags.cpu()
            for k, v in (("rec", rec), ("prec", prec), ("flags", flags)):
                out[k] = [v[off[c]:off[c + 1]] for c in range(C)]
        return out


# ---- COCO: the AP / AR tables of COCOeval (reference engine.evaluate -> datasets/coco_eval.py) --------------------------------------
def coco_params():
    """COCOeval's Params for iouType 'bbox', computed by numpy exactly as published; the device only ever sees these arrays."""
    return {"iouThrs": np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True),
            "recThrs": np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True),
            "maxDets": [1, 10, 100],
            "areaRng": [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]],
            "areaRngLbl": ["all", "small", "medium", "large"]}


def _coco_match_host(det_boxes, det_cats, det_off, gt_boxes, gt_cats, gt_iscrowd, gt_area, gt_off, iou_thrs, area_rng, max_det, max_gt,
                     top, npig):
    """kernels.coco_match on CPU tensors (same arguments, same results, same limits): per (image, category) the detections in order,
    per detection the IoUs once and the 40 (area range, threshold) walks side by side - the layout of the kernel's lanes."""
    if max_det > K.COCO_MAX_DET or max_gt > K.COCO_MAX_GT:
        raise ValueError(f"at most {K.COCO_MAX_DET} detections and {K.COCO_MAX_GT} ground-truth boxes per image")
    Kc, T, A = npig.shape[0], K.COCO_T, K.COCO_A
    bx, dc, doff = det_boxes.numpy(), det_cats.numpy(), det_off.numpy()
    dx, dy = bx[:, 0].astype(np.float64), bx[:, 1].astype(np.float64)
    dw, dh = (bx[:, 2] - bx[:, 0]).astype(np.float64), (bx[:, 3] - bx[:, 1]).astype(np.float64)      # fp32 differences, widened
    darea = dw * dh
    gb, gc, goff = gt_boxes.numpy().reshape(-1, 4), gt_cats.numpy(), gt_off.numpy()
    crowd_all, area_all = gt_iscrowd.numpy().astype(bool), gt_area.numpy()
    rng = area_rng.numpy().reshape(A, 2)
    lo, hi = rng[:, 0], rng[:, 1]
    thr = np.minimum(iou_thrs.numpy(), 1 - 1e-10)
    rank = np.full(dc.shape[0], -1, np.int32)
    words = np.zeros((dc.shape[0], A), np.int32)
    cnt = np.zeros((Kc, A), np.int32)
    ai, ti = np.meshgrid(np.arange(A), np.arange(T), indexing="ij")
    shifts = np.arange(T, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(doff.shape[0] - 1):
            d0, d1, g0, g1 = doff[i], doff[i + 1], goff[i], goff[i + 1]
            for c in np.union1d(dc[d0:d1], gc[g0:g1]):
                if c < 0 or c >= Kc:
                    continue
                g = np.nonzero(gc[g0:g1] == c)[0] + g0
                d = (np.nonzero(dc[d0:d1] == c)[0] + d0)[:top]
                G = g.size
                crowd, gx, gy, gw, gh = crowd_all[g], gb[g, 0], gb[g, 1], gb[g, 2], gb[g, 3]
                ig = crowd[None, :] | (area_all[g][None, :] < lo[:, None]) | (area_all[g][None, :] > hi[:, None])      # [A,G]
                cnt[c] += (~ig).sum(1).astype(np.int32)
                gm = np.zeros((A, T, G), bool)
                for r, j in enumerate(d):
                    w = np.minimum(dx[j] + dw[j], gx + gw) - np.maximum(dx[j], gx)
                    h = np.minimum(dy[j] + dh[j], gy + gh) - np.maximum(dy[j], gy)
                    inter = w * h
                    o = np.where((w > 0) & (h > 0), inter / np.where(crowd, darea[j], darea[j] + gw * gh - inter), 0.)
                    best, m = np.broadcast_to(thr, (A, T)).copy(), np.full((A, T), -1)
                    free = np.ones((A, T), bool)
                    for group in (False, True):
                        for q in range(G):
                            take = (ig[:, q] == group)[:, None] & free & ~(gm[:, :, q] & (not crowd[q])) & ~(o[q] < best)
                            best[take], m[take] = o[q], q
                        free = m < 0                       # the ignored group is walked only where nothing matched
                    dm = m >= 0
                    dig = np.broadcast_to(((darea[j] < lo) | (darea[j] > hi))[:, None], (A, T))
                    if G:
                        dig = np.where(dm, ig[ai, np.maximum(m, 0)], dig)
                    gm[ai[dm], ti[dm], m[dm]] = True
                    rank[j] = r
                    words[j] = ((dm.astype(np.int64) << shifts).sum(1) | (dig.astype(np.int64) << (shifts + T)).sum(1)).astype(np.int32)
    npig += torch.from_numpy(cnt)
    return torch.from_numpy(rank), torch.from_numpy(words)


def _coco_accumulate_host(words, rank, scores, seg_off, npig, max_dets, rec_thrs):
    """kernels.coco_accumulate on CPU tensors."""
    T, A = K.COCO_T, K.COCO_A
    wd, rk, sc, off = words.numpy(), rank.numpy(), scores.numpy(), seg_off.numpy()
    npg, lims, thr = npig.numpy(), max_dets.numpy(), rec_thrs.numpy()
    Kc, M, R = npg.shape[0], lims.size, thr.size
    precision, recall, score_at = -np.ones((T, R, Kc, A, M)), -np.ones((T, Kc, A, M)), -np.ones((T, R, Kc, A, M))
    tbits = np.arange(T)[:, None]
    for k in range(Kc):
        seg = slice(off[k], off[k + 1])
        for m in range(M):
            part = rk[seg] < lims[m]
            w, s = wd[seg][part], sc[seg][part].astype(np.float64)
            nd = s.size
            for a in range(A):
                if npg[k, a] == 0:
                    continue
                mt, ig = ((w[:, a][None, :] >> tbits) & 1).astype(bool), ((w[:, a][None, :] >> (tbits + T)) & 1).astype(bool)
                tp, fp = np.cumsum(mt & ~ig, axis=1).astype(np.float64), np.cumsum(~mt & ~ig, axis=1).astype(np.float64)
                rc = tp / npg[k, a]
                pr = tp / ((fp + tp) + np.spacing(1))
                env = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]
                recall[:, k, a, m] = rc[:, -1] if nd else 0
                for t in range(T):
                    at = np.searchsorted(rc[t], thr, side="left")
                    ok = at < nd
                    precision[t, :, k, a, m] = np.where(ok, env[t][np.minimum(at, max(nd - 1, 0))], 0.) if nd else 0.
                    score_at[t, :, k, a, m] = np.where(ok, s[np.minimum(at, max(nd - 1, 0))], 0.) if nd else 0.
    t = torch.from_numpy
    return t(precision), t(recall), t(score_at)


class COCODetectionMeter(_DetectionMeter):
    """Accumulates the COCO detection metrics over an evaluation run: the twelve numbers of COCOeval.summarize() for 'bbox' and the
    precision / recall / scores tables behind them (what the reference's CocoEvaluator returns as coco_eval['bbox'].stats / .eval).

        m = COCODetectionMeter(cat_ids)
        m.update(results, gts)     # per batch, straight after per_class_nms
        m.merge()                  # once, when the images were split over ranks
        out = m.summarize()        # {'stats' [12], 'eval': {...}, 'npig' [K,4]}

    results: the list `infer.per_class_nms` returns - per image {'scores' [n] fp32, 'labels' [n] category ids (ids outside cat_ids are
    dropped), 'boxes' [n,4] xyxy fp32 in absolute pixels}.  gts: per image {'boxes' [g,4] xywh (the annotation's bbox), 'labels' [g],
    'iscrowd' [g], 'area' [g] (the annotation's own field, not w * h), 'image_id' (int or 0-d tensor)}.

    Inside an (image, category) the detections are matched in descending score, equal scores in their incoming order, the first 100
    only.  The curve of a category is ordered by score descending, then image id ascending, then that rank - the order COCOeval's stable
    sort gives its image-sorted lists - so nothing depends on batch order or on how the images were split over ranks.  update() does not
    read device data on the host.  DESIGN.md section 8i has the rules, the tie order, the limits and what is (not) pinned."""

    def __init__(self, cat_ids):
        self.cat_ids = sorted({int(c) for c in cat_ids})
        if not self.cat_ids:
            raise ValueError("COCODetectionMeter: no categories")
        self.params = coco_params()
        self.reset()

    _SCHEMA = {"score": (torch.float32, ()), "words": (torch.int32, (K.COCO_A,)), "rank": (torch.int32, ()), "cat": (torch.int64, ()),
               "img": (torch.int64, ())}
    _MAX_GT = K.COCO_MAX_GT

    def _start(self, dev):
        """First use of a device: the counter npig and the parameter arrays (numpy's values) in one copy."""
        P, Kc = self.params, len(self.cat_ids)
        self._device = dev
        self._counters = torch.zeros((Kc, K.COCO_A), dtype=torch.int32, device=dev)
        f = torch.from_numpy(np.concatenate([P["iouThrs"], np.asarray(P["areaRng"], np.float64).reshape(-1), P["recThrs"]]))
        i = torch.tensor(self.cat_ids + list(P["maxDets"]), dtype=torch.int64)
        if dev.type == "cuda":
            f, i = f.pin_memory().to(dev, non_blocking=True), i.pin_memory().to(dev, non_blocking=True)
        T, A = K.COCO_T, K.COCO_A
        self._dev_params = {"iouThrs": f[:T], "areaRng": f[T:T + 2 * A], "recThrs": f[T + 2 * A:], "cat_ids": i[:Kc],
                            "maxDets": i[Kc:].to(torch.int32)}

    @torch.no_grad()
    def update(self, results, gts):
        b = self._collect(results, gts, {"iscrowd": torch.uint8, "area": torch.float64})
        if b is None:
            return
        # category id -> index into cat_ids; ids that are not in the list become Kc and gather at the end of the image
        Kc, cid = len(self.cat_ids), self._dev_params["cat_ids"]

        def index_of(lab):
            at = torch.searchsorted(cid, lab).clamp(max=Kc - 1)
            return torch.where(cid[at] == lab, at, Kc)
        cat, gcat = index_of(b["labels"]), index_of(b["glabels"])
        order = self._order_batch(b["scores"], b["img"], cat, Kc + 1)
        scores, cat, boxes = b["scores"][order].contiguous(), cat[order].contiguous(), b["boxes"][order].contiguous()
        match = K.coco_match if self._device.type == "cuda" else _coco_match_host
        rank, words = match(boxes, cat, b["det_off"], b["gboxes"], gcat, b["iscrowd"], b["area"], b["gt_off"], self._dev_params["iouThrs"],
                            self._dev_params["areaRng"], b["max_det"], b["max_gt"], self.params["maxDets"][-1], self._counters)
        # a detection that was not evaluated (no category, or past the first 100) moves behind every category
        self._append({"score": scores, "words": words, "rank": rank, "cat": torch.where(rank < 0, Kc, cat), "img": b["ids"][b["img"]]})

    @torch.no_grad()
    def summarize(self, return_records=False):
        """-> {'stats': the twelve numbers of COCOeval.summarize() (fp64 [12]: AP, AP50, AP75, AP small / medium / large at maxDets 100; AR at
        maxDets 1 / 10 / 100, AR small / medium / large at 100), 'eval': {'params', 'counts' [T,R,K,A,M], 'precision' [T,R,K,A,M], 'recall'
        [T,K,A,M], 'scores' [T,R,K,A,M]} as COCOeval.eval holds them (-1: no ground truth to find), 'npig' int32 [K,4]} - numpy arrays.
        return_records adds 'records': 'cat' (index into cat_ids), 'img', 'rank', 'score', 'words' [n,4] of the evaluated detections, per
        category in curve order."""
        self._check_run()
        Kc, P = len(self.cat_ids), self.params
        # category, score descending, image id, rank; category Kc (not evaluated) lies behind
        col, seg_off = self._curve_order(("rank", "img", "score", "cat"), Kc, tuple(self._SCHEMA))
        acc = K.coco_accumulate if self._device.type == "cuda" else _coco_accumulate_host
        precision, recall, scores = acc(col["words"], col["rank"], col["score"], seg_off, self._counters.contiguous(),
                                        self._dev_params["maxDets"], self._dev_params["recThrs"])
        precision, recall, scores = precision.cpu().numpy(), recall.cpu().numpy(), scores.cpu().numpy()

        def one(ap, iou_thr=None, area="all", max_dets=100):                    # COCOeval._summarize, on the host
            a, m = P["areaRngLbl"].index(area), P["maxDets"].index(max_dets)
            s = precision[:, :, :, a, m] if ap else recall[:, :, a, m]
            if iou_thr is not None:
                s = s[np.where(iou_thr == P["iouThrs"])[0]]
            return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        d1, d10, d100 = P["maxDets"]
        stats = np.array([one(1, max_dets=d100), one(1, .5, max_dets=d100), one(1, .75, max_dets=d100), one(1, area="small", max_dets=d100),
                          one(1, area="medium", max_dets=d100), one(1, area="large", max_dets=d100), one(0, max_dets=d1),
                          one(0, max_dets=d10), one(0, max_dets=d100), one(0, area="small", max_dets=d100),
                          one(0, area="medium", max_dets=d100), one(0, area="large", max_dets=d100)], np.float64)
        out = {"stats": stats, "npig": self._counters.cpu().numpy().copy(),
               "eval": {"params": {**P, "catIds": list(self.cat_ids)}, "counts": [K.COCO_T, len(P["recThrs"]), Kc, K.COCO_A, len(P["maxDets"])],
                        "precision": precision, "recall": recall, "scores": scores}}
        if return_records:
            end = int(seg_off[-1])
            out["records"] = {k: v[:end].cpu().numpy() for k, v in col.items()}
        return out


# ---- multi-label classification AP (reference cams_deit.py:493-574, AveragePrecisionMeter) --------------------
def _cls_ap_host(scores, targets, n, difficult):
    """kernels.cls_ap on CPU tensors: per class a stable sort by (-score, index) with NaN in front, integer running counts, the fp64
    quotients and their sequential sum.  -> (ap fp64 [C], npos int32 [C], ncounted int32 [C]) as numpy arrays."""
    sc, tg = scores.numpy()[:, :n], targets.numpy()[:, :n]
    C = sc.shape[0]
    ap, npos, ncounted = np.full(C, np.nan), np.zeros(C, np.int32), np.zeros(C, np.int32)
    for c in range(C):
        nan = np.isnan(sc[c])
        order = np.lexsort((np.where(nan, 0.0, -sc[c].astype(np.float64)), ~nan))      # stable; last key first: NaN, then -score (-0.0 == 0.0)
        t = tg[c][order]
        t = t[t != 0] if difficult else t
        positive = t == 1
        npos[c], ncounted[c] = int(positive.sum()), t.size
        if npos[c]:
            terms = np.cumsum(positive)[positive].astype(np.float64) / (np.nonzero(positive)[0] + 1).astype(np.float64)
            ap[c] = np.cumsum(terms)[-1] / float(npos[c])                              # cumsum: a fixed, sequential order
    return ap, npos, ncounted


class ClassificationAPMeter:
    """Accumulates the per-class average precision of multi-label image classification over an evaluation run: the reference's
    AveragePrecisionMeter (cams_deit.py:493-574), what says whether the class tokens ('x_logits', 'x_cls_logits') - and with them the
    CAM branch behind every pseudo box - are healthy.

        m = ClassificationAPMeter(difficult_examples=False)
        m.add(outputs['x_logits'], torch.stack([t['label'] for t in targets]))     # per batch: [B, C] logits, [B, C] multi-hot labels
        m.merge()                  # once, when the images were split over ranks
        out = m.summarize()        # {'ap' fp64 [C], 'map', 'npos' int32 [C], 'ncounted' int32 [C]}
        m.value()                  # the reference's return: ap as fp32 [C]

    reset(), add(output, target) and value() keep the reference's names and shape rules: a 1-D input is one column, a 2-D one is
    [B, C], a later add with another C raises.  Targets of any dtype are reduced to int8 on their device (== 1 -> 1, a positive;
    == 0 -> 0; anything else -> -1, a negative like 0 - but with difficult_examples a 0 is skipped and a -1 is not); scores are kept
    as fp32.  Pass raw logits: a sigmoid is monotone, but its fp32 saturation makes ties the logits do not have.  Storage is class-major
    [C][capacity], on the device of the first add, and grows geometrically; add() does not read device data on the host.

    Per class: higher score first; scores that compare equal in fp32 (+0.0 and -0.0 included) rank by ascending sample index - the
    order of add(), after merge() rank-major; a NaN score ranks before every number, NaNs among themselves by index.  At every counted
    positive, in that order, pos_count / total_count is added in fp64, and the sum is divided by the number of positives.  On
    tie-free input this is the reference's number bit for bit (its torch.sort promises no tie order; this rule is the package's own).
    A class without a counted positive has ap NaN (the reference raises ZeroDivisionError) and takes no part in 'map'; 'map' is NaN
    when no class has one.  CUDA tensors take csrc/cls_ap.hip (one call, one copy per summarize(); it ranks by counting, N comparisons
    per sample and class - 0.4 ms at N 5000, C 90, profiles/cls_ap_meter.txt - and is not meant for millions of samples); CPU tensors
    take a numpy composition of the same rules."""
    _MIN_CAPACITY = 1024

    def __init__(self, difficult_examples=False):
        self.difficult_examples = bool(difficult_examples)
        self.reset()

    def reset(self):
        self._device, self._C, self._n = None, None, 0
        self._scores = self._targets = None    # [C][capacity] fp32 / int8, the first _n columns valid
        self._merged = False

    @staticmethod
    def _columns(x, what):
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.asarray(x))
        if x.dim() == 1:
            return x.reshape(-1, 1)
        if x.dim() != 2:
            raise ValueError(f"wrong {what} size (should be 1D or 2D with one column per class)")
        return x

    def _reserve(self, n, C, dev):
        """Room for n samples: a new allocation and one copy when the capacity is exceeded (geometric growth)."""
        if self._scores is not None and n <= self._scores.shape[1]:
            return
        cap, old = max(2 * n, self._MIN_CAPACITY), (self._scores, self._targets)
        self._scores = torch.empty((C, cap), dtype=torch.float32, device=dev)
        self._targets = torch.empty((C, cap), dtype=torch.int8, device=dev)
        if old[0] is not None:
            self._scores[:, :self._n] = old[0][:, :self._n]
            self._targets[:, :self._n] = old[1][:, :self._n]

    @torch.no_grad()
    def add(self, output, target):
        if self._merged:
            raise RuntimeError("ClassificationAPMeter: add() after merge(); reset() first")
        output, target = self._columns(output, "output"), self._columns(target, "target")
        if output.shape != target.shape:
            raise ValueError(f"ClassificationAPMeter.add: output {tuple(output.shape)} and target {tuple(target.shape)} differ")
        B, C = output.shape
        if self._C is not None and C != self._C:
            raise ValueError("dimensions for output should match previously added examples.")
        if self._device is None:
            self._device = output.device
        elif output.device != self._device:
            raise ValueError(f"ClassificationAPMeter: tensors on {output.device}, earlier adds on {self._device}")
        if self._n + B > K.CLS_AP_MAX_N:
            raise ValueError(f"ClassificationAPMeter: at most {K.CLS_AP_MAX_N} samples")
        self._C = C
        self._reserve(self._n + B, C, self._device)
        target = target.to(self._device)
        code = (target == 1).to(torch.int8) - ((target != 1) & (target != 0)).to(torch.int8)      # 1 / 0 / -1 (a NaN target: -1)
        self._scores[:, self._n:self._n + B] = output.detach().to(torch.float32).t()
        self._targets[:, self._n:self._n + B] = code.t()
        self._n += B

    def merge(self, group=None):
        """Concatenate the samples of every rank in rank order: afterwards every rank summarizes the whole run.  A no-op without an
        initialised process group.  A rank that added nothing takes part (it learns C from the others)."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        if self._merged:
            raise RuntimeError("ClassificationAPMeter: merge() called twice; reset() first")
        if self._device is None:
            self._device = torch.device("cuda" if dist.get_backend(group) == "nccl" else "cpu")
        dev, world = self._device, dist.get_world_size(group)
        width = torch.tensor([self._C or 0], dtype=torch.int64, device=dev)
        dist.all_reduce(width, op=dist.ReduceOp.MAX, group=group)
        C = int(width)
        if self._C is not None and self._C != C:
            raise ValueError("ClassificationAPMeter.merge: the ranks hold different numbers of classes")
        self._merged = True
        if C == 0:                                                              # no rank added anything
            return
        self._C = C
        if self._scores is None:
            self._reserve(0, C, dev)
        rows = [_all_gather_rows(t[:, :self._n].t().contiguous(), world, group) for t in (self._scores, self._targets)]
        self._n = rows[0].shape[0]
        self._scores, self._targets = rows[0].t().contiguous(), rows[1].t().contiguous()

    @torch.no_grad()
    def summarize(self):
        """-> {'ap': fp64 [C] (NaN for a class without a counted positive), 'map': float (the mean over the classes that have one; NaN
        if none has), 'npos': int32 [C], 'ncounted': int32 [C]} - CPU tensors and a float."""
        if self._C is None:
            raise RuntimeError("ClassificationAPMeter.summarize: nothing accumulated")
        C = self._C
        if self._device.type == "cuda":
            out = K.cls_ap(self._scores, self._targets, self._n, self.difficult_examples).cpu()       # one call, one copy
            counts = out[1].view(torch.int32)
            ap, npos, ncounted = out[0].numpy().copy(), counts[:C].numpy().copy(), counts[C:].numpy().copy()
        else:
            ap, npos, ncounted = _cls_ap_host(self._scores, self._targets, self._n, self.difficult_examples)
        have = npos > 0
        return {"ap": torch.from_numpy(ap), "map": float(np.mean(ap[have])) if have.any() else float("nan"),
                "npos": torch.from_numpy(npos), "ncounted": torch.from_numpy(ncounted)}

    def value(self):
        """The reference's return: the AP per class as fp32 [C]; 0 for an empty meter."""
        if self._C is None or self._n == 0:
            return 0
        return self.summarize()["ap"].to(torch.float32)


# ---- pseudo-label quality (csrc/pseudo_quality.hip) ---------------------------------------------------------------
def _pseudo_quality_host(boxes, labels, scores, off, gboxes, glabels, goff, C, iou_thresh, counters):
    """kernels.pseudo_quality on CPU tensors, composed of torch operations per image: box_iou on the corners of both sides (fp32,
    elementwise: one rounding per operation), masks for the same-label pairs, integer counts added into `counters` [10, C + 1]."""
    from .util import box_ops
    thr = torch.tensor(iou_thresh, dtype=torch.float32)
    limit = K.PSEUDO_QUALITY_MAX_ROWS
    B = len(off) - 1
    if any(off[b + 1] - off[b] > limit or goff[b + 1] - goff[b] > limit for b in range(B)):
        raise ValueError(f"PseudoLabelMeter: at most {limit} pseudo rows and {limit} ground-truth rows per image")

    def classes(l):
        return torch.where((l < 0) | (l >= C), torch.full_like(l, -1), l)

    def add(k, cls, values=None):
        counters[k].index_add_(0, cls, torch.ones_like(cls) if values is None else values)

    for b in range(B):
        p, g = slice(off[b], off[b + 1]), slice(goff[b], goff[b + 1])
        pc, gc = classes(labels[p]), classes(glabels[g])
        add(4, torch.where(pc < 0, torch.full_like(pc, C), pc))
        add(7, torch.where(gc < 0, torch.full_like(gc, C), gc))
        iou = box_ops.box_iou(box_ops.box_cxcywh_to_xyxy(boxes[p]), box_ops.box_cxcywh_to_xyxy(gboxes[g]))[0]          # [t, g]
        same = (pc[:, None] == gc[None, :]) & (pc[:, None] >= 0)
        best = torch.where(same & ~torch.isnan(iou), iou, torch.full_like(iou, float("-inf")))
        best = best.max(dim=1).values if iou.shape[1] else torch.full((iou.shape[0],), float("-inf"))
        matched = same.any(dim=1)
        hit = matched & (best > thr)
        add(5, pc[hit])
        add(6, pc[(pc >= 0) & ~matched])
        counted = matched & (best > 0) & torch.isfinite(best)
        q = torch.round(best[counted].clamp(max=1) * float(K.PSEUDO_QUALITY_IOU_SCALE)).to(torch.int64)      # half to even, like llrint
        add(9, pc[counted], q)
        add(8, gc[(same & (iou > thr)).any(dim=0)])
        sc = None if scores is None else scores[p]
        for c in torch.unique(gc[gc >= 0]).tolist():
            rows = torch.nonzero(pc == c).reshape(-1)
            one = torch.tensor([c])
            add(0, one)
            if rows.numel() == 0:
                add(3, one)
                continue
            lead = rows[0]
            if sc is not None:
                s = sc[rows]
                nan = torch.isnan(s)
                # the first NaN, else the first of the largest: argmax of a boolean takes the lowest index
                lead = rows[(nan if bool(nan.any()) else s == s.max()).to(torch.uint8).argmax()]
            if bool(hit[lead]):
                add(1, one)
            if bool(hit[rows].any()):
                add(2, one)
    return counters


class PseudoLabelMeter:
    """How good the boxes are that the refine training loops train on - the CAM boxes of stage 0, PostProcessRefine's picks of the later
    stages - against the loader's ground truth, counted while training runs: CorLoc, precision, recall and mean IoU per class and stage.

        m = PseudoLabelMeter(num_classes=21, stages=["cam", "rf_1", "rf_2"], iou_thresh=0.5)
        m.update("cam", pseudo, gts)      # per batch and stage: one launch on the device, nothing read on the host
        m.merge()                          # once, when the images were split over ranks: an all-reduce of the counters
        out = m.summarize()                # {stage: {'corloc' fp64 [C], 'any_hit', 'precision', 'recall', 'mean_iou', 'mean_corloc', ...}}
        print(m)                           # one line per stage

    pseudo: a camboxes.PseudoTargets, the flat dict of infer.refine_targets ('boxes', 'labels', 'scores', 'offsets'), or the per-image list
    of {'boxes', 'labels'[, 'scores']} that engine.get_refinements_pseudo_label returns.  gts: per image {'boxes' [g, 4], 'labels' [g]} in
    normalised cxcywh, the loader's target rows.  num_classes = C: labels lie in [0, C) - with the loaders' 1-based labels, pass the
    detector's class count (one more than the dataset's).

    Rules (the package's own; csrc/pseudo_quality.hip).  IoU: box_iou on box_cxcywh_to_xyxy of both rows in fp32, the arithmetic the
    criterion applies to these rows.  A label outside [0, C) on either side is counted ('dropped_rows', 'dropped_gts') and takes no
    further part.  Best IoU of a pseudo row: the maximum over its non-NaN IoUs with the same-label ground-truth rows of its image;
    without such a row it is an orphan.  Hit: best IoU > iou_thresh, strict (voc_eval.py, dis_eval.py:146).  A ground-truth row is
    covered when a same-label pseudo row of its image has IoU > iou_thresh with it.  Pair: an (image, class) with a ground-truth row.
    Lead row of a pair: without scores the lowest pseudo row of the class (CAM boxes: the largest border; PostProcessRefine: the only
    one), with scores the largest score - equal scores to the lowest row, the first NaN before everything (spe_refine_pick's rule).
    Per class: corloc = pairs whose lead row hits / pairs, any_hit = pairs with a hit / pairs, precision = rows that hit / rows,
    recall = covered ground-truth rows / ground-truth rows, mean_iou = the mean best IoU of the non-orphan rows, each best IoU capped
    at 1 and rounded to a multiple of 2^-20 (not finite or not positive: 0) - integer sums, so every number is a function of the input
    alone.  A class with a zero denominator is NaN and takes no part in that stage's mean_* value (ClassificationAPMeter's rule).

    The rows are scored in the frame the criterion receives them: CAM rows are normalised by the padded canvas of the batch - with the
    (H, W) -> dsize transposition camboxes._pseudo_labels documents - and ground-truth rows by the image's own size.  On fixed square
    inputs the frames coincide; elsewhere the meter reports the mismatch the criterion trains on, and does not rescale.

    The state is int64 [stages, 10, C + 1] on the device of the first update.  CUDA tensors take spe_pseudo_quality (one launch per
    update, both offset vectors in one pinned upload); CPU tensors take a torch composition of the same rules."""

    def __init__(self, num_classes, stages, iou_thresh=0.5):
        self.num_classes, self.stages, self.iou_thresh = int(num_classes), [str(s) for s in stages], float(iou_thresh)
        if self.num_classes < 1:
            raise ValueError("PseudoLabelMeter: num_classes must be at least 1")
        if len(set(self.stages)) != len(self.stages) or not self.stages:
            raise ValueError("PseudoLabelMeter: stages must be distinct names, at least one")
        self.reset()

    def reset(self):
        self._counters = None              # int64 [S, 10, C + 1] on the device of the first update

    def _state(self, device):
        if self._counters is None:
            self._counters = torch.zeros((len(self.stages), len(K.PSEUDO_QUALITY_COUNTERS), self.num_classes + 1), dtype=torch.int64,
                                         device=device)
        elif self._counters.device != device:
            raise ValueError(f"PseudoLabelMeter: tensors on {device}, earlier updates on {self._counters.device}")
        return self._counters

    @staticmethod
    def _cat(parts, dtype, tail, device):
        parts = [p.detach().reshape((-1,) + tail).to(dtype) for p in parts]
        if not parts:
            return torch.zeros((0,) + tail, dtype=dtype, device=device)
        return (torch.cat(parts) if len(parts) > 1 else parts[0]).contiguous()

    def _flat(self, rows, device, what):
        """-> boxes [n, 4] fp32, labels [n] int64, scores [n] fp32 or None, host offsets - out of any of the accepted forms."""
        if hasattr(rows, "offsets") and hasattr(rows, "boxes"):                                 # camboxes.PseudoTargets
            rows = {"boxes": rows.boxes, "labels": rows.labels, "offsets": rows.offsets}
        if isinstance(rows, dict):
            for k in ("boxes", "labels", "offsets"):
                if k not in rows:
                    raise ValueError(f"PseudoLabelMeter.update: the flat {what} rows have no {k!r}")
            off = [int(o) for o in rows["offsets"]]
            per = [rows]
        else:
            per, off = list(rows), [0]
            for i, r in enumerate(per):
                for k in ("boxes", "labels"):
                    if k not in r:
                        raise ValueError(f"PseudoLabelMeter.update: {what} rows of image {i} have no {k!r}")
                off.append(off[-1] + r["labels"].shape[0])
        if device is None:
            device = per[0]["boxes"].device if per else torch.device("cpu")
        boxes = self._cat([r["boxes"] for r in per], torch.float32, (4,), device)
        labels = self._cat([r["labels"] for r in per], torch.int64, (), device)
        scores = self._cat([r["scores"] for r in per], torch.float32, (), device) if per and all("scores" in r for r in per) else None
        if boxes.shape[0] != off[-1] or labels.shape[0] != off[-1] or (scores is not None and scores.shape[0] != off[-1]):
            raise ValueError(f"PseudoLabelMeter.update: {what} offsets end at {off[-1]}, the rows do not")
        return boxes, labels, scores, off, device

    @torch.no_grad()
    def update(self, stage, pseudo, gts):
        if stage not in self.stages:
            raise ValueError(f"PseudoLabelMeter.update: unknown stage {stage!r}; the meter has {self.stages}")
        boxes, labels, scores, off, device = self._flat(pseudo, None, "pseudo")
        gboxes, glabels, _, goff, device = self._flat(list(gts), device, "ground-truth")
        if len(off) != len(goff):
            raise ValueError(f"PseudoLabelMeter.update: pseudo rows of {len(off) - 1} images, ground truth of {len(goff) - 1}")
        if len(off) == 1:                                                               # an empty batch
            return
        if not (boxes.device == gboxes.device == labels.device == glabels.device == device):
            raise ValueError("PseudoLabelMeter.update: the pseudo rows and the ground truth lie on different devices")
        counters = self._state(device)[self.stages.index(stage)]
        C = self.num_classes
        if device.type != "cuda":
            _pseudo_quality_host(boxes, labels, scores, off, gboxes, glabels, goff, C, self.iou_thresh, counters)
            return
        host = np.array([off, goff], np.int32)
        table = K.host_table(host.view(np.uint8).reshape(-1), device).view(torch.int32).view(2, len(off))      # ONE pinned upload
        K.pseudo_quality(boxes, labels, scores, table[0], gboxes, glabels, table[1], (host[0], host[1]), C, self.iou_thresh, counters)

    def merge(self, group=None):
        """All-reduce of the counters: afterwards every rank summarizes the whole run.  A no-op without an initialised process group; a
        rank that saw no batch takes part with zeros."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        if self._counters is None:
            self._state(torch.device("cuda" if dist.get_backend(group) == "nccl" else "cpu"))
        dist.all_reduce(self._counters, op=dist.ReduceOp.SUM, group=group)

    def counters(self):
        """The raw state as a CPU tensor int64 [stages, 10, C + 1] (zeros before the first update): ONE copy."""
        if self._counters is None:
            return torch.zeros((len(self.stages), len(K.PSEUDO_QUALITY_COUNTERS), self.num_classes + 1), dtype=torch.int64)
        return self._counters.cpu()

    def summarize(self):
        """-> {stage: {'corloc', 'any_hit', 'precision', 'recall', 'mean_iou': fp64 [C] (NaN where the denominator is 0); 'mean_corloc',
        'mean_any_hit', 'mean_precision', 'mean_recall', 'mean_mean_iou': floats over the classes that have a value (NaN if none has);
        'counters': int64 [10, C] by K.PSEUDO_QUALITY_COUNTERS, 'dropped_rows', 'dropped_gts': ints}} - CPU tensors; one copy."""
        C = self.num_classes
        all_counters = self.counters().numpy()
        out = {}
        for s, stage in enumerate(self.stages):
            c = all_counters[s, :, :C]
            f = c.astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                per = {"corloc": f[1] / f[0], "any_hit": f[2] / f[0], "precision": f[5] / f[4], "recall": f[8] / f[7],
                       "mean_iou": f[9] / float(K.PSEUDO_QUALITY_IOU_SCALE) / (f[4] - f[6])}
            for name, den in (("corloc", c[0]), ("any_hit", c[0]), ("precision", c[4]), ("recall", c[7]), ("mean_iou", c[4] - c[6])):
                per[name] = np.where(den > 0, per[name], np.nan)
            res = {k: torch.from_numpy(v.copy()) for k, v in per.items()}
            for k, v in per.items():
                have = ~np.isnan(v)
                res["mean_" + k] = float(np.mean(v[have])) if have.any() else float("nan")
            res["counters"] = torch.from_numpy(c.copy())
            res["dropped_rows"], res["dropped_gts"] = int(all_counters[s, 4, C]), int(all_counters[s, 7, C])
            out[stage] = res
        return out

    def __str__(self):
        out = self.summarize()
        return "\n".join("Pseudo labels [{}]: CorLoc {:.4f}  precision {:.4f}  recall {:.4f}  mean IoU {:.4f}".format(
            stage, r["mean_corloc"], r["mean_precision"], r["mean_recall"], r["mean_mean_iou"]) for stage, r in out.items())


# ---- proposal recall (csrc/proposal_recall.hip) -------------------------------------------------------------------
def _proposal_tables(who, iou_threshs, ks):
    """The two small tables as the library wants them (fp32 thresholds, int32 cut-offs), checked: ValueError names the argument."""
    limit = K.PROPOSAL_RECALL_MAX_TABLE
    try:
        thr = np.asarray(list(iou_threshs), dtype=np.float32).reshape(-1)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{who}: iou_threshs must be a sequence of numbers") from e
    if not 1 <= thr.size <= limit or not np.all(np.isfinite(thr)) or np.any(thr[1:] <= thr[:-1]):
        raise ValueError(f"{who}: iou_threshs must be 1 to {limit} finite, strictly ascending values (in fp32), got {list(iou_threshs)}")
    kl = list(ks)
    if not 1 <= len(kl) <= limit or any(int(k) != k or not 1 <= int(k) < 2 ** 31 for k in kl) or any(b <= a for a, b in zip(kl, kl[1:])):
        raise ValueError(f"{who}: ks must be 1 to {limit} strictly ascending integers, each at least 1, got {kl}")
    return thr, np.asarray([int(k) for k in kl], dtype=np.int32)


def _class_order_position(p):
    """p fp32 [Q], one class's probabilities of an image's queries -> int64 [Q]: how many queries come before each one in the class's
    order - a NaN before every number, larger values first, equal values (and NaNs among themselves) by lower q.  Three explicit sort
    keys, the query index among them: nothing rests on a sort's tie behaviour."""
    p = p.numpy()
    nan = np.isnan(p)
    order = np.lexsort((np.arange(p.size), -np.where(nan, np.float32(0), p), ~nan))          # the LAST key is the primary one
    pos = np.empty(p.size, np.int64)
    pos[order] = np.arange(p.size)
    return torch.from_numpy(pos)


def _proposal_recall_host(prob, boxes, gboxes, glabels, goff, C, thr, ks, counters):
    """kernels.proposal_recall on CPU tensors, composed of torch / numpy operations per image: box_iou on the corners of both sides (fp32,
    elementwise: one rounding per operation), the class's order as positions, integer counts added into `counters` [2 + T + T * K, C + 1]."""
    from .util import box_ops
    B, Q, Kc = prob.shape
    T, Kn = len(thr), len(ks)
    limit = min(C, Kc)
    thr_t = torch.from_numpy(np.asarray(thr, np.float32))
    ks_t = torch.from_numpy(np.asarray(ks, np.int64))
    for b in range(B):
        g = slice(goff[b], goff[b + 1])
        labels = glabels[g]
        valid = (labels >= 0) & (labels < limit)
        counters[0].index_add_(0, torch.where(valid, labels, torch.full_like(labels, C)), torch.ones_like(labels))
        if not bool(valid.any()):
            continue
        labels = labels[valid]
        iou = box_ops.box_iou(box_ops.box_cxcywh_to_xyxy(gboxes[g][valid]), box_ops.box_cxcywh_to_xyxy(boxes[b]))[0]          # [g, Q]
        best = torch.where(torch.isnan(iou), torch.full_like(iou, float("-inf")), iou).max(dim=1).values
        counted = (best > 0) & torch.isfinite(best)
        q = torch.round(best[counted].clamp(max=1) * float(K.PROPOSAL_RECALL_IOU_SCALE)).to(torch.int64)      # half to even, like llrint
        counters[1].index_add_(0, labels[counted], q)
        for c in torch.unique(labels).tolist():
            rows = labels == c
            pos = _class_order_position(prob[b, :, c])
            one = torch.tensor([c])
            for t in range(T):
                cover = iou[rows] > thr_t[t]                                               # strict; a NaN never covers
                r = torch.where(cover, pos[None, :], torch.full_like(pos, Q)[None, :]).min(dim=1).values       # the position of the lead
                r = r[r < Q]
                counters[2 + t].index_add_(0, one, torch.tensor([r.numel()]))
                hits = (r[:, None] < ks_t[None, :]).sum(dim=0)
                counters[2 + T + t * Kn:2 + T + (t + 1) * Kn, c] += hits
    return counters


class ProposalRecallMeter:
    """Are the sparse proposals of a stage on the objects, or is the pick among them wrong?  Every ground-truth row is scored against ALL
    Q query boxes of its image and stage, counted while training runs: per class and stage the recall-at-k curve under the class's own
    ordering of the queries (k = 1 is exactly PostProcessRefine's pick) and the ceiling with all Q queries.  ceiling - recall@1 is the
    selection gap: a low ceiling is a localisation failure, a high ceiling with a low recall@1 a selection failure.

        m = ProposalRecallMeter(num_classes=21, stages=["s0", "s1", "s2"], iou_threshs=(0.5, 0.75), ks=(1, 10, 100))
        m.update("s0", outputs[0], gts)    # per batch and stage: the sigmoid and one launch on the device, nothing read on the host
        m.merge()                          # once, when the images were split over ranks: an all-reduce of the counters
        out = m.summarize()                # {stage: {'recall' fp64 [T, K, C], 'ceiling' [T, C], 'selection_gap' [T, C], 'mean_best_iou' [C], ...}}
        print(m)                           # one line per stage

    outputs: {'pred_logits' [B, Q, Kc], 'pred_boxes' [B, Q, 4] normalised cxcywh}; the queries are ordered by pred_logits.sigmoid(), bitwise
    the probabilities infer.refine_targets picks on, saturation ties included.  gts: per image {'boxes' [g, 4] normalised cxcywh, 'labels'
    [g]}, the loader's target rows.  num_classes = C: labels lie in [0, min(C, Kc)) and a label is its logit column.

    Rules (the package's own; csrc/proposal_recall.hip).  IoU: box_iou on box_cxcywh_to_xyxy of both rows in fp32, PseudoLabelMeter's.  A
    ground-truth row with a label outside [0, min(C, Kc)) is counted ('dropped_gts') and takes no further part.  Best IoU of a row: the
    maximum over its non-NaN IoUs with the Q queries of its image; capped at 1 and rounded to a multiple of 2^-20 (not finite or not
    positive: 0) it joins an integer sum.  Per threshold the covering set is the queries with IoU > threshold (strict; a NaN never
    covers); a row with a non-empty set counts for the ceiling, and its lead is the set's first query in its class's order: a NaN
    probability before every number, larger values first, equal values and NaNs among themselves by lower query - torch.max's and
    spe_refine_pick's pick comes first.  The row hits at k when fewer than k queries of the image precede the lead.  Per class:
    recall[t][k] = hits / rows, ceiling[t] = rows with a covering query / rows, selection_gap[t] = ceiling[t] - recall[t][0],
    mean_best_iou = the mean best IoU.  A class without ground-truth rows is NaN and takes no part in that stage's mean_* values
    (ClassificationAPMeter's rule).  Every number is a function of the input alone.

    The boxes are scored in the frame the criterion receives them; the meter does not rescale (PseudoLabelMeter's statement).

    The state is int64 [stages, 2 + T + T * K, C + 1] on the device of the first update.  CUDA tensors take spe_proposal_recall (one
    launch per update, the offsets in one pinned upload, at most 1024 queries); CPU tensors take a torch / numpy composition of the same
    rules."""

    def __init__(self, num_classes, stages, iou_threshs=(0.5, 0.75), ks=(1, 10, 100)):
        self.num_classes, self.stages = int(num_classes), [str(s) for s in stages]
        if self.num_classes < 1:
            raise ValueError("ProposalRecallMeter: num_classes must be at least 1")
        if len(set(self.stages)) != len(self.stages) or not self.stages:
            raise ValueError("ProposalRecallMeter: stages must be distinct names, at least one")
        self._thr, self._ks = _proposal_tables("ProposalRecallMeter", iou_threshs, ks)
        self.iou_threshs, self.ks = tuple(float(t) for t in self._thr), tuple(int(k) for k in self._ks)
        self.rows = K.proposal_recall_counters(len(self.iou_threshs), len(self.ks))
        self.reset()

    def reset(self):
        self._counters = None              # int64 [S, 2 + T + T * K, C + 1] on the device of the first update

    def _shape(self):
        return (len(self.stages), len(self.rows), self.num_classes + 1)

    def _state(self, device):
        if self._counters is None:
            self._counters = torch.zeros(self._shape(), dtype=torch.int64, device=device)
        elif self._counters.device != device:
            raise ValueError(f"ProposalRecallMeter: tensors on {device}, earlier updates on {self._counters.device}")
        return self._counters

    @torch.no_grad()
    def update(self, stage, outputs, gts):
        who = "ProposalRecallMeter.update"
        if stage not in self.stages:
            raise ValueError(f"{who}: unknown stage {stage!r}; the meter has {self.stages}")
        for k in ("pred_logits", "pred_boxes"):
            if k not in outputs:
                raise ValueError(f"{who}: outputs have no {k!r}")
        logits, boxes = outputs["pred_logits"].detach(), outputs["pred_boxes"].detach()
        if logits.dim() != 3 or boxes.shape != logits.shape[:2] + (4,):
            raise ValueError(f"{who}: outputs must hold pred_logits [B, Q, Kc] and pred_boxes [B, Q, 4], got {tuple(logits.shape)} and "
                             f"{tuple(boxes.shape)}")
        B, Q, Kc = logits.shape
        gts = list(gts)
        if len(gts) != B:
            raise ValueError(f"{who}: outputs of {B} images, gts of {len(gts)}")
        if B == 0:                                                                      # an empty batch
            return
        if Q < 1 or Kc < 1 or Q > K.PROPOSAL_RECALL_MAX_Q:
            raise ValueError(f"{who}: outputs with 1 to {K.PROPOSAL_RECALL_MAX_Q} queries and at least one class expected, got {tuple(logits.shape)}")
        device = logits.device
        goff = [0]
        for i, r in enumerate(gts):
            for k in ("boxes", "labels"):
                if k not in r:
                    raise ValueError(f"{who}: gts of image {i} have no {k!r}")
            goff.append(goff[-1] + r["labels"].shape[0])
        gboxes = PseudoLabelMeter._cat([r["boxes"] for r in gts], torch.float32, (4,), device)
        glabels = PseudoLabelMeter._cat([r["labels"] for r in gts], torch.int64, (), device)
        if gboxes.shape[0] != goff[-1]:
            raise ValueError(f"{who}: gts hold {goff[-1]} labels and {gboxes.shape[0]} boxes")
        if not (boxes.device == gboxes.device == glabels.device == device):
            raise ValueError(f"{who}: outputs and gts lie on different devices")
        counters = self._state(device)[self.stages.index(stage)]
        prob = logits.to(torch.float32).sigmoid()                                       # fp32 logits: the one ATen launch
        boxes = boxes.to(torch.float32).contiguous()
        if device.type != "cuda":
            _proposal_recall_host(prob, boxes, gboxes, glabels, goff, self.num_classes, self._thr, self._ks, counters)
            return
        host = np.array(goff, np.int32)
        table = K.host_table(host.view(np.uint8), device).view(torch.int32)             # ONE pinned upload
        K.proposal_recall(prob, boxes, gboxes, glabels, table, host, self.num_classes, self._thr, self._ks, counters)

    def merge(self, group=None):
        """All-reduce of the counters: afterwards every rank summarizes the whole run.  A no-op without an initialised process group; a
        rank that saw no batch takes part with zeros."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        if self._counters is None:
            self._state(torch.device("cuda" if dist.get_backend(group) == "nccl" else "cpu"))
        dist.all_reduce(self._counters, op=dist.ReduceOp.SUM, group=group)

    def counters(self):
        """The raw state as a CPU tensor int64 [stages, 2 + T + T * K, C + 1] (zeros before the first update): ONE copy."""
        if self._counters is None:
            return torch.zeros(self._shape(), dtype=torch.int64)
        return self._counters.cpu()

    def summarize(self):
        """-> {stage: {'recall' fp64 [T, K, C], 'ceiling' [T, C], 'selection_gap' [T, C] (ceiling - recall at ks[0]), 'mean_best_iou' [C] - NaN
        for a class without ground-truth rows; 'mean_recall' fp64 [T, K], 'mean_ceiling' [T], 'mean_selection_gap' [T], 'mean_mean_best_iou'
        float: over the classes that have rows (NaN if none has); 'gts' int64 [C], 'counters' int64 [2 + T + T * K, C] by self.rows,
        'dropped_gts' int}} - CPU tensors; one copy."""
        C, T, Kn = self.num_classes, len(self.iou_threshs), len(self.ks)
        all_counters = self.counters().numpy()
        out = {}
        for s, stage in enumerate(self.stages):
            c = all_counters[s, :, :C]
            gts = c[0]
            have = gts > 0
            den = np.where(have, gts, 1).astype(np.float64)

            def per_class(v):
                return np.where(have, v.astype(np.float64) / den, np.nan)

            per = {"recall": per_class(c[2 + T:].reshape(T, Kn, C)), "ceiling": per_class(c[2:2 + T]),
                   "mean_best_iou": per_class(c[1]) / float(K.PROPOSAL_RECALL_IOU_SCALE)}
            per["selection_gap"] = per["ceiling"] - per["recall"][:, 0]
            res = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in per.items()}
            for k, v in per.items():
                mean = np.array([row[have].mean() if have.any() else np.nan for row in v.reshape(-1, C)]).reshape(v.shape[:-1])     # row by row: one summation order
                res["mean_" + k] = float(mean) if mean.ndim == 0 else torch.from_numpy(np.ascontiguousarray(mean))
            res["gts"], res["counters"] = torch.from_numpy(gts.copy()), torch.from_numpy(c.copy())
            res["dropped_gts"] = int(all_counters[s, 0, C])
            out[stage] = res
        return out

    def __str__(self):
        out = self.summarize()
        return "\n".join("Proposals [{}] IoU > {:g}: {}  ceiling {:.4f}".format(
            stage, self.iou_threshs[0], "  ".join("recall@{} {:.4f}".format(k, v) for k, v in zip(self.ks, r["mean_recall"][0].tolist())),
            float(r["mean_ceiling"][0])) for stage, r in out.items())
