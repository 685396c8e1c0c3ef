"""Plain numpy restatement of the training-target kernels (csrc/train_targets.hip): the assembly of the stage-0 target rows out of the
packed CAM boxes, and PostProcessRefine's pick.  Every fp32 operation is one numpy fp32 operation: one rounding each."""
import numpy as np

F = np.float32


def cam_targets(counts, boxes, cls0, single, W, H):
    """counts int32 [M] (negative: a status, no rows), boxes int32 [M, max_boxes, 4] as [x0, y0, x1, y1], cls0 int32 [M] ->
    (rows fp32 [T, 4] normalised cxcywh, labels int64 [T], off int32 [M + 1]): per map, in table order, its first counts[m] boxes
    (single: its first box), as spe_amd.camboxes._pseudo_labels builds them - integer sums and differences, true division by 2 in
    fp32, then the division by [W, H, W, H] in fp32."""
    M, max_boxes = boxes.shape[:2]
    n = np.clip(counts, 0, 1 if single else max_boxes).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    keep = np.arange(max_boxes)[None, :] < n[:, None]                       # [M, max_boxes], row-major = table order
    b = boxes[keep].astype(np.int64)
    x0, y0, x1, y1 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    rows = np.stack([(x0 + x1).astype(F) / F(2) / F(W), (y0 + y1).astype(F) / F(2) / F(H), (x1 - x0).astype(F) / F(W), (y1 - y0).astype(F) / F(H)], -1)
    labels = np.repeat(cls0.astype(np.int64) + 1, n)
    return rows.astype(F).reshape(-1, 4), labels, off


def pick_one(col):
    """The best query of one column of probabilities by torch.max's rule: the first NaN if there is one; else the largest value, the
    lowest query among equal values."""
    nan = np.isnan(col)
    if nan.any():
        return int(np.argmax(nan))
    return int(np.argmax(col))                                               # numpy's argmax takes the first maximum


def refine_pick(prob, boxes, classes):
    """prob fp32 [B, Q, Kc], boxes fp32 [B, Q, 4], classes: per image its class ids -> (scores [U] as bits (int32), queries int32 [U],
    boxes fp32 [U, 4] as bits, labels int64 [U], off [B + 1])."""
    scores, queries, rows, labels, off = [], [], [], [], [0]
    for b, cl in enumerate(classes):
        for c in cl:
            q = pick_one(prob[b, :, c])
            scores.append(prob[b, q, c]); queries.append(q); rows.append(boxes[b, q]); labels.append(c)
        off.append(len(labels))
    return (np.asarray(scores, F).view(np.int32), np.asarray(queries, np.int32), np.asarray(rows, F).reshape(-1, 4).view(np.int32),
            np.asarray(labels, np.int64), off)
