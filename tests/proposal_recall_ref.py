"""The rules of spe_proposal_recall (csrc/proposal_recall.hip; include/spe_hip.h) restated in numpy: every fp32
operation of the kernel is one numpy fp32 operation (the IoU is tests/pseudo_quality_ref.py's, the arithmetic both kernels share), every
count a Python integer.  Written as loops over ground-truth rows, thresholds and cut-offs - the shape of the rules, not of the kernel,
and not of the meter's torch / numpy composition either.  The class's order is a key function; nothing rests on a sort's tie rule."""
import numpy as np

import pseudo_quality_ref as P

F = np.float32
IOU_SCALE = 1 << 20


def names(T, K):
    return ["gts", "iou_q"] + [f"ceil[{t}]" for t in range(T)] + [f"hit[{t}][{k}]" for t in range(T) for k in range(K)]


def order_key(p):
    """-> key(q) of the class's order over the probabilities p [Q]: a NaN before every number and NaNs among themselves by lower q; larger
    values first, equal values (+0.0 == -0.0) by lower q."""
    def key(q):
        v = float(p[q])
        return (0, 0.0, q) if v != v else (1, -v, q)        # -(+0.0) == -(-0.0) in the comparison: the index decides
    return key


def positions(p):
    """How many queries come before each query in the class's order -> list [Q]."""
    ordered = sorted(range(len(p)), key=order_key(p))
    pos = [0] * len(p)
    for r, q in enumerate(ordered):
        pos[q] = r
    return pos


def image(prob, boxes, grows, glabels, C, thr, ks, counters):
    """One image - prob [Q, Kc], boxes [Q, 4], its ground-truth rows - added into counters, int64 [2 + T + T * K, C + 1]."""
    Q, Kc = prob.shape
    T, K = len(thr), len(ks)
    limit = min(C, Kc)
    iou = P.iou_matrix(grows, boxes)                           # [g, Q]
    pos = {}
    for g, label in enumerate(glabels):
        c = int(label)
        if not 0 <= c < limit:
            counters[0, C] += 1
            continue
        counters[0, c] += 1
        v = iou[g]
        finite = v[~np.isnan(v)]
        counters[1, c] += P.quantise(finite.max() if finite.size else F(-np.inf))
        if c not in pos:
            pos[c] = positions(prob[:, c])
        for t in range(T):
            with np.errstate(invalid="ignore"):
                cover = [q for q in range(Q) if v[q] > F(thr[t])]      # strict; a NaN compares false
            if not cover:
                continue
            counters[2 + t, c] += 1
            r = min(pos[c][q] for q in cover)                  # the lead is the covering query that comes first; r queries precede it
            for k in range(K):
                if r < int(ks[k]):
                    counters[2 + T + t * K + k, c] += 1
    return counters


def recall(prob, boxes, gboxes, glabels, goff, C, thr, ks, counters=None):
    """The whole batch -> int64 [2 + T + T * K, C + 1]; counters: what the sums start from (a copy is made)."""
    T, K = len(thr), len(ks)
    out = np.zeros((2 + T + T * K, C + 1), np.int64) if counters is None else np.array(counters, np.int64)
    prob, boxes = np.asarray(prob, F), np.asarray(boxes, F)
    gboxes = np.asarray(gboxes, F).reshape(-1, 4)
    for b in range(len(goff) - 1):
        g = slice(goff[b], goff[b + 1])
        image(prob[b], boxes[b], gboxes[g], np.asarray(glabels)[g], C, thr, ks, out)
    return out


def summary(counters, C, T, K):
    """The per-class ratios and their means over the classes with ground-truth rows, fp64."""
    c = np.asarray(counters)[:, :C]
    have = c[0] > 0

    def ratio(row):
        return np.array([float(n) / float(d) if d > 0 else np.nan for n, d in zip(row, c[0])], np.float64)

    def mean(per):
        return float(per[have].mean()) if have.any() else float("nan")
    out = {"recall": np.array([[ratio(c[2 + T + t * K + k]) for k in range(K)] for t in range(T)]),
           "ceiling": np.array([ratio(c[2 + t]) for t in range(T)]),
           "mean_best_iou": np.array([float(n) / float(IOU_SCALE) / float(d) if d > 0 else np.nan for n, d in zip(c[1], c[0])], np.float64)}
    out["selection_gap"] = out["ceiling"] - out["recall"][:, 0]
    out["mean_recall"] = np.array([[mean(out["recall"][t, k]) for k in range(K)] for t in range(T)])
    out["mean_ceiling"] = np.array([mean(out["ceiling"][t]) for t in range(T)])
    out["mean_selection_gap"] = np.array([mean(out["selection_gap"][t]) for t in range(T)])
    out["mean_mean_best_iou"] = mean(out["mean_best_iou"])
    return out
