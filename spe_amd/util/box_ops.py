"""Box format helpers used by the post-processors (mirror of reference util/box_ops.py:18-31).
The pairwise IoU/GIoU arithmetic of the hot path lives in csrc/loss.hip."""
import torch


def box_cxcywh_to_xyxy(x):
    cx, cy, w, h = x.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], dim=-1)


def box_xyxy_to_cxcywh(x):
    x0, y0, x1, y1 = x.unbind(-1)
    return torch.stack([(x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0], dim=-1)


def box_area(boxes):
    """[n, 4] xyxy -> [n]: width times height, no clamp."""
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])


def box_iou(boxes1, boxes2):
    """[n, 4] and [m, 4] xyxy -> (iou [n, m], union [n, m]) in the reference's operation order (util/box_ops.py:33-46): both areas, the
    larger top-left and the smaller bottom-right corner, the sides clamped at 0, their product, (area1 + area2) - inter, the quotient.
    Degenerate boxes are not refused: a union of 0 gives NaN (0 / 0) and a NaN coordinate gives NaN.  csrc/pseudo_quality.hip restates
    this sequence one rounding per operation."""
    area1, area2 = box_area(boxes1), box_area(boxes2)
    top_left = torch.max(boxes1[:, None, :2], boxes2[None, :, :2])
    bottom_right = torch.min(boxes1[:, None, 2:], boxes2[None, :, 2:])
    sides = (bottom_right - top_left).clamp(min=0)
    inter = sides[..., 0] * sides[..., 1]
    union = area1[:, None] + area2[None, :] - inter
    return inter / union, union
