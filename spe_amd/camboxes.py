"""CAM -> pseudo-label boxes, the step before the criterion in the reference training loop (SURVEY.md section 8(f)
rank 1): `engine.get_pseudo_label_multi_boxes` (engine.py:356-398), its single-box form `engine.get_pseudo_label`
(engine.py:312-352) and `engine.get_pseudo_label_multi_boxes_voc` (engine.py:402-444), with `cams_deit.resize_cam` /
`get_bboxes` / `get_multi_bboxes` (cams_deit.py:9-13, 34-96).  The per-pixel work (bilinear resize to image size, min-max,
quantise, threshold) runs on the device for all (image, present class) maps at once.  The borders are then found

  "device" (default)  on the device as well, by labelling instead of border walks (csrc/cambox_labels.hip): one
                      device->host copy of M * (1 + 4 * max_boxes) int32 - counts and boxes, no image;
  "host"              in native host code (csrc/cambox.hip) after one device->host copy of the thresholded uint8 images

(`set_contours`); both give the same boxes in the same order.  The reference runs the whole thing through NumPy + OpenCV
per class on the host.  OpenCV is absent in this environment: the arithmetic is restated from its published algorithms
and pinned only by oracle/cam_oracle.py (same restatement in NumPy) and structural checks against scipy.ndimage in the
tests.
"""
import numpy as np
import torch

from . import kernels as K
from .lib import SpeLibraryError

MAX_BOXES = 256            # per map, both paths (more survivors: status -5)
_CONTOURS = "device"


def set_contours(mode):
    """Where the borders of the thresholded maps are found: "device" or "host"."""
    global _CONTOURS
    if mode not in ("device", "host"):
        raise ValueError(f"set_contours: expected 'device' or 'host', got {mode!r}")
    _CONTOURS = mode


def get_contours():
    return _CONTOURS


def _xyxy_to_cxcywh(x):
    x0, y0, x1, y1 = x[..., 0], x[..., 1], x[..., 2], x[..., 3]
    return torch.stack([(x0 + x1) / 2, (y0 + y1) / 2, (x1 - x0), (y1 - y0)], dim=-1)


def _map_boxes(imgs, area_ratio):
    """Thresholded maps [M, rows, cols] uint8 on the device -> per map an int64 [n, 4] host tensor [x, y, x+w, y+h],
    largest area first."""
    M = imgs.shape[0]
    if _CONTOURS == "host":
        host = imgs.cpu()                                                             # one device->host copy (images)
        return [K.cam_contour_boxes(host[m], area_ratio, MAX_BOXES).to(torch.int64) for m in range(M)]
    packed = K.cam_boxes_device_packed(imgs, area_ratio, MAX_BOXES).cpu()             # one device->host copy (counts + boxes)
    n, boxes = packed[:M].tolist(), packed[M:].view(M, MAX_BOXES, 4)
    if min(n) < 0:
        raise SpeLibraryError(f"spe_cam_boxes_device failed with status {min(n)}")
    return [boxes[m, :n[m]].to(torch.int64) for m in range(M)]


def _pseudo_labels(outputs, samples, present, num_classes, cam_thr, area_ratio, single):
    """The loop shared by the three drivers.  present[b][c] > 0: class c of image b has a map to box.

    Reproduced quirk: the reference passes `size = (H, W)` to `resize_cam`, which hands it to cv2.resize as
    (width, height) - the CAM is resized to W rows x H columns - and then divides the boxes by [W, H, W, H]."""
    tensors = samples.tensors if hasattr(samples, "tensors") else samples
    device = tensors.device
    cams = outputs["cams_cls"]
    B, Kc = cams.shape[0], cams.shape[1]
    H, W = tensors.shape[-2:]
    rows, cols = int(W), int(H)
    sel = [(b, c) for b in range(B) for c in range(min(num_classes, Kc)) if present[b][c] > 0]
    if not sel:
        return [{"boxes": torch.zeros((0, 4), device=device), "labels": torch.zeros((0,), dtype=torch.long, device=device)}
                for _ in range(B)]
    bi = torch.tensor([s[0] for s in sel], device=cams.device)
    ci = torch.tensor([s[1] for s in sel], device=cams.device)
    maps = cams[bi, ci].float().contiguous()
    found = _map_boxes(K.cam_prepare(maps, rows, cols, cam_thr), area_ratio)
    per_img = [([], []) for _ in range(B)]
    for (b, c), bx in zip(sel, found):
        if single:
            bx = bx[:1]             # max(contours, key=contourArea) is the first maximum = the first box of the ordering
        bx = _xyxy_to_cxcywh(bx)                                                      # integer arithmetic -> true division -> float
        per_img[b][0].append(bx)
        per_img[b][1].extend([c + 1] * bx.shape[0])
    scale = torch.tensor([W, H, W, H], dtype=torch.float32)
    out = []
    for b in range(B):
        if per_img[b][0]:
            boxes = torch.cat(per_img[b][0], dim=0).float() / scale
            labels = torch.tensor(per_img[b][1], dtype=torch.long)
        else:                       # no class present: the reference would fail on torch.cat([]); return empty sets
            boxes, labels = torch.zeros((0, 4)), torch.zeros((0,), dtype=torch.long)
        out.append({"boxes": boxes.to(device), "labels": labels.to(device)})
    return out


class PseudoTargets:
    """The stage-0 targets of a batch, flat: `boxes` [T, 4] normalised cxcywh and `labels` [T] (int64, 1-based) on the device of the
    samples, image b owning rows offsets[b] .. offsets[b+1] (host integers); `classes`: per image the sorted class ids (1-based) that
    have a row - what torch.unique of the image's labels holds, known without reading them."""

    def __init__(self, boxes, labels, offsets, classes):
        self.boxes, self.labels, self.offsets, self.classes = boxes, labels, offsets, classes

    def per_image(self):
        """The list the three drivers return: views, one {'boxes', 'labels'} per image."""
        o = self.offsets
        return [{"boxes": self.boxes[o[b]:o[b + 1]], "labels": self.labels[o[b]:o[b + 1]]} for b in range(len(o) - 1)]

    @classmethod
    def from_lists(cls, per_img):
        """Out of the drivers' list (the host composition)."""
        offsets = [0]
        for p in per_img:
            offsets.append(offsets[-1] + p["labels"].shape[0])
        classes = [sorted(set(p["labels"].tolist())) for p in per_img]
        return cls(torch.cat([p["boxes"] for p in per_img]), torch.cat([p["labels"] for p in per_img]), offsets, classes)


@torch.no_grad()
def pseudo_targets(outputs, samples, present, num_classes, cam_thr, area_ratio, single=False):
    """The three drivers' work for host lists `present` (present[b][c] > 0: class c of image b has a map to box) -> PseudoTargets.

    With the "device" contours on device tensors everything is enqueued - prepare, labelling and the assembly of the target rows
    (csrc/train_targets.hip) - and then the M box COUNTS are read: one copy of 4 M bytes, the only synchronising call; offsets, the
    per-image views and the classes follow from them on the host.  The "host" contours and CPU tensors take _pseudo_labels."""
    tensors = samples.tensors if hasattr(samples, "tensors") else samples
    device = tensors.device
    cams = outputs["cams_cls"]
    if _CONTOURS == "host" or not cams.is_cuda:
        return PseudoTargets.from_lists(_pseudo_labels(outputs, samples, present, num_classes, cam_thr, area_ratio, single))
    B, Kc = cams.shape[0], cams.shape[1]
    H, W = tensors.shape[-2:]
    rows, cols = int(W), int(H)                                                       # the (H, W) -> dsize quirk, see _pseudo_labels
    sel = [(b, c) for b in range(B) for c in range(min(num_classes, Kc)) if present[b][c] > 0]
    M = len(sel)
    if not sel:
        return PseudoTargets(torch.zeros((0, 4), device=device), torch.zeros((0,), dtype=torch.long, device=device), [0] * (B + 1),
                             [[] for _ in range(B)])
    table = K.host_table(np.array(sel, np.int32).T.copy().view(np.uint8).reshape(-1), cams.device).view(torch.int32).view(2, M)
    maps = cams[table[0], table[1]].float().contiguous()
    packed = K.cam_boxes_device_packed(K.cam_prepare(maps, rows, cols, cam_thr), area_ratio, MAX_BOXES)
    boxes, labels, _ = K.cam_targets(packed, table[1], MAX_BOXES, single, W, H)
    n = packed[:M].tolist()                                                           # the one device->host copy: 4 M bytes
    if min(n) < 0:
        raise SpeLibraryError(f"spe_cam_boxes_device failed with status {min(n)}")
    offsets, classes, t = [0] * (B + 1), [[] for _ in range(B)], 0
    for (b, c), k in zip(sel, n):
        k = min(k, 1) if single else k
        t += k
        offsets[b + 1] = t
        if k > 0:
            classes[b].append(c + 1)
    for b in range(B):                                                                # an image without a map ends where its predecessor does
        offsets[b + 1] = max(offsets[b + 1], offsets[b])
    return PseudoTargets(boxes[:t].to(device), labels[:t].to(device), offsets, classes)


def present_lists(targets, key):
    """The presence lists of a batch as host lists.  Label tensors on the device are read with ONE stacked copy; tensors on the host
    (what a loader hands over) are not a device read at all."""
    labs = [t[key].detach().reshape(-1) for t in targets]
    if labs and all(l.is_cuda for l in labs) and len({l.shape for l in labs}) == 1:
        return torch.stack(labs).cpu().tolist()
    return [l.cpu().tolist() for l in labs]


@torch.no_grad()
def get_pseudo_label_multi_boxes(outputs, samples, targets, args):
    """Same signature and result as engine.py:356-398: list (one per image) of {'boxes': [n,4] normalised cxcywh,
    'labels': [n] class ids (1-based)} on the device of `samples.tensors`; every border of a present class's thresholded
    map with area >= args.multi_box_ratio * largest gives a box.  The (H, W) -> dsize quirk of the reference is
    reproduced (see _pseudo_labels)."""
    return _pseudo_labels(outputs, samples, present_lists(targets, "img_label"), args.num_classes, args.cam_thr,
                          args.multi_box_ratio, single=False)


@torch.no_grad()
def get_pseudo_label(outputs, samples, targets, args):
    """Same signature and result as engine.py:312-352 (what train_one_epoch uses): ONE box per present class, that of
    the border with the largest area (`max(contours, key=cv2.contourArea)`: the first maximum in discovery order, which is
    the first box of the multi-box ordering; [0, 0, 1, 1] for a map without a border) -> 'boxes' [n, 4] normalised cxcywh,
    'labels' [n] (1-based).  The (H, W) -> dsize quirk is reproduced (see _pseudo_labels).

    An image with no present class raises in the reference (torch.stack of an empty list); here it gets empty tensors."""
    return _pseudo_labels(outputs, samples, present_lists(targets, "img_label"), args.num_classes, args.cam_thr, 1.0, single=True)   # ratio 1: only the
    #                                                     borders that tie for the largest area survive; the first is taken


@torch.no_grad()
def get_pseudo_label_multi_boxes_voc(outputs, samples, targets, args):
    """Same signature and result as engine.py:402-444: as get_pseudo_label_multi_boxes with the presence list read from
    targets[b]['label'] and the area ratio left at get_multi_bboxes' default 0.5 (args.multi_box_ratio is not used there).
    The (H, W) -> dsize quirk is reproduced (see _pseudo_labels)."""
    return _pseudo_labels(outputs, samples, present_lists(targets, "label"), args.num_classes, args.cam_thr, 0.5, single=False)
