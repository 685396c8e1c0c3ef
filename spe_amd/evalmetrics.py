"""PASCAL VOC detection metrics of the SPE evaluation loop: the last step of reference
`engine_loc.evaluate_det_voc` (engine_loc.py:176-197), i.e. `evaluate_detections` -> `voc_eval` (datasets/voc_voc.py:366-437,
datasets/voc_eval.py) for AP / mAP and `evaluate_discovery` -> `dis_eval` (voc_voc.py:454-488, datasets/dis_eval.py) for CorLoc.

The reference writes every detection to per-class text files, parses them and the XML annotations back and walks one global,
score-sorted list per class in Python.  Whether a detection is a true or a false positive depends only on the detections of the same
image and class before it, so here the greedy matching runs per batch, straight after `infer.per_class_nms`
(`spe_voc_match`: one wave per (image, class)), only flags, scores and integer counters are kept, and `summarize()` is one sort and
one launch (`spe_voc_ap`: one workgroup per class).  DESIGN.md section 8g has the decomposition, the tie rule and the argument for the
decimal round trip.

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


class VOCDetectionMeter:
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

    def reset(self):
        self._device = None
        self._n, self._cols = 0, None          # records: capacity-sized tensors, the first _n rows valid
        self._ids = []                         # image ids of every update (images without detections included)
        self._counters = None                  # int32 [3, C]: npos, nimgs, hits
        self._merged = False

    def _append(self, new):
        n = new["flag"].numel()
        if self._cols is None or self._n + n > self._cols["flag"].numel():
            cap = max(2 * (self._n + n), 4096)                                   # geometric growth
            grown = {k: torch.empty((cap,), dtype=v.dtype, device=v.device) for k, v in new.items()}
            if self._cols is not None:
                for k, v in self._cols.items():
                    grown[k][:self._n] = v[:self._n]
            self._cols = grown
        for k, v in new.items():
            self._cols[k][self._n:self._n + n] = v
        self._n += n

    @torch.no_grad()
    def update(self, results, gts):
        if self._merged:
            raise RuntimeError("VOCDetectionMeter: update() after merge(); reset() first")
        if len(results) != len(gts):
            raise ValueError("VOCDetectionMeter.update: one ground-truth dict per result")
        if not results:
            return
        dev, C = results[0]["scores"].device, self.num_classes
        if self._device is None:
            self._device = dev
            self._counters = torch.zeros((3, C), dtype=torch.int32, device=dev)
        elif dev != self._device:
            raise ValueError(f"VOCDetectionMeter: tensors on {dev}, earlier updates on {self._device}")
        nd = [int(r["scores"].shape[0]) for r in results]                       # host lengths: the shapes we are handed
        ng = [int(g["labels"].shape[0]) for g in gts]
        if max(nd) > K.VOC_MAX_DET or max(ng) > K.VOC_MAX_GT:
            raise ValueError(f"at most {K.VOC_MAX_DET} detections and {K.VOC_MAX_GT} ground-truth boxes per image")
        scores = torch.cat([r["scores"].reshape(-1) for r in results]).float()
        labels = torch.cat([r["labels"].reshape(-1) for r in results]).long()
        boxes = torch.cat([r["boxes"].reshape(-1, 4) for r in results]).float()
        gboxes = torch.cat([g["boxes"].reshape(-1, 4) for g in gts]).to(dev, torch.float64).contiguous()
        glabels = torch.cat([g["labels"].reshape(-1) for g in gts]).to(dev, torch.int64)
        gdiff = torch.cat([g["difficult"].reshape(-1) for g in gts]).to(dev).ne(0).to(torch.uint8)
        # what the host knows from the shapes - offsets, the image of every row and its position inside the image - and the image ids
        # go up in ONE copy (from pinned memory, asynchronous on the device path)
        ids = [g["image_id"] for g in gts]
        ids_dev = None
        if any(torch.is_tensor(i) for i in ids):
            ids_dev, ids = torch.stack([torch.as_tensor(i).reshape(()).to(dev, torch.int64) for i in ids]), []
        nimg, ndt = len(nd), sum(nd)
        host = torch.from_numpy(np.concatenate([[0], np.cumsum(nd), [0], np.cumsum(ng), np.repeat(np.arange(nimg), nd)]
                                               + [np.arange(n) for n in nd] + [ids]).astype(np.int64))
        if dev.type == "cuda":
            host = host.pin_memory().to(dev, non_blocking=True)
        det_off, gt_off = host[:nimg + 1].to(torch.int32), host[nimg + 1:2 * nimg + 2].to(torch.int32)
        img, pos = host[2 * nimg + 2:2 * nimg + 2 + ndt], host[2 * nimg + 2 + ndt:2 * nimg + 2 + 2 * ndt].to(torch.int32)
        ids = ids_dev if ids_dev is not None else host[2 * nimg + 2 + 2 * ndt:]
        self._ids.append(ids)
        # (label ascending, score descending) inside every image, equal scores in incoming order; per_class_nms output already
        # is.  Labels outside 1 .. C gather at the two ends of the image.
        cls = torch.where((labels >= 1) & (labels <= C), labels, torch.where(labels < 1, 0, C + 1))
        o1 = torch.sort(scores, descending=True, stable=True).indices
        o2 = torch.sort(img[o1] * (C + 2) + cls[o1], stable=True).indices
        order = o1[o2]
        scores, cls, boxes = scores[order].contiguous(), cls[order].contiguous(), boxes[order].contiguous()
        match = K.voc_match if dev.type == "cuda" else _match_host
        ss, cs = (_SCORE_SCALE, _COORD_SCALE) if self.file_roundtrip else (0.0, 0.0)
        flags, qscores = match(boxes, scores, cls, det_off, gboxes, glabels, gdiff, gt_off, max(nd), max(ng), self.ovthresh, ss, cs,
                               self._counters[0], self._counters[1], self._counters[2])
        self._append({"score": qscores, "flag": flags, "cls": torch.where(cls == 0, C + 1, cls) - 1, "img": ids[img], "ord": pos})

    def merge(self, group=None):
        """Gather the records of every rank and all-reduce the counters: afterwards every rank summarizes the whole run.  A no-op
        without an initialised process group."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        if self._merged:
            raise RuntimeError("VOCDetectionMeter: merge() called twice; reset() first")
        C = self.num_classes
        dev = self._device if self._device is not None else torch.device("cuda" if dist.get_backend(group) == "nccl" else "cpu")
        if self._counters is None:                                              # a rank that saw no image
            self._device, self._counters = dev, torch.zeros((3, C), dtype=torch.int32, device=dev)
        world = dist.get_world_size(group)

        def gather(t):
            n = torch.tensor([t.numel()], dtype=torch.int64, device=dev)
            ns = [torch.zeros_like(n) for _ in range(world)]
            dist.all_gather(ns, n, group=group)
            ns = [int(x) for x in ns]
            pad = torch.zeros((max(max(ns), 1),), dtype=t.dtype, device=dev)
            pad[:t.numel()] = t
            outs = [torch.empty_like(pad) for _ in range(world)]
            dist.all_gather(outs, pad, group=group)
            return torch.cat([o[:k] for o, k in zip(outs, ns)])

        dtypes = {"score": torch.float64, "flag": torch.uint8, "cls": torch.int64, "img": torch.int64, "ord": torch.int32}
        cols = {k: gather(self._cols[k][:self._n] if self._cols is not None else torch.empty((0,), dtype=dt, device=dev))
                for k, dt in dtypes.items()}
        self._ids = [gather(torch.cat(self._ids) if self._ids else torch.empty((0,), dtype=torch.int64, device=dev))]
        self._cols, self._n = cols, cols["flag"].numel()
        dist.all_reduce(self._counters, group=group)
        self._merged = True

    @torch.no_grad()
    def summarize(self, use_07_metric=True, return_curves=False):
        """-> {'ap' [C] (the 11-point metric or the area), 'ap07' [C], 'ap_area' [C], 'map', 'corloc' [C], 'mean_corloc', 'npos' [C],
        'nimgs' [C]}: fp64 / int32 CPU tensors and floats; a class without ground-truth images has corloc NaN and one with detections
        but no non-difficult ground truth has area AP NaN, as in the reference, and the means propagate them (np.mean).
        return_curves adds 'rec', 'prec', 'flags': per class, in curve order."""
        C = self.num_classes
        if self._counters is None:
            raise RuntimeError("VOCDetectionMeter.summarize: nothing accumulated")
        ids = torch.sort(torch.cat(self._ids)).values
        if bool((ids[1:] == ids[:-1]).any()):
            raise ValueError("VOCDetectionMeter: an image id was accumulated twice")
        dev, n = self._device, self._n
        if self._cols is None:
            self._append({"score": torch.empty(0, dtype=torch.float64, device=dev), "flag": torch.empty(0, dtype=torch.uint8, device=dev),
                          "cls": torch.empty(0, dtype=torch.int64, device=dev), "img": torch.empty(0, dtype=torch.int64, device=dev),
                          "ord": torch.empty(0, dtype=torch.int32, device=dev)})
        col = {k: v[:n] for k, v in self._cols.items()}
        # curve order by stable sorts, last key first: class, score descending, image id, position inside the image
        o = torch.sort(col["ord"], stable=True).indices
        o = o[torch.sort(col["img"][o], stable=True).indices]
        o = o[torch.sort(col["score"][o], descending=True, stable=True).indices]
        o = o[torch.sort(col["cls"][o], stable=True).indices]
        flags, cls = col["flag"][o].contiguous(), col["cls"][o].contiguous()
        seg_off = torch.searchsorted(cls, torch.arange(C + 1, device=dev)).to(torch.int32)       # dropped labels (class C) lie behind
        npos = self._counters[0].contiguous()
        ap = K.voc_ap if dev.type == "cuda" else _ap_host
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
