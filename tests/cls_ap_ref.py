"""The reference's multi-label AP (cams_deit.py:555-574, AveragePrecisionMeter.average_precision) restated in plain Python with the
order written down - what spe_amd.evalmetrics.ClassificationAPMeter and csrc/cls_ap.hip are held against, bit for bit.

The reference sorts with torch.sort(descending=True), which promises no order among equal scores.  Here the order is total: a NaN
score before every number (where torch.sort puts it; pinned by tests/golden/cls_ap_special.pt), then higher score first, scores that
compare equal (+0.0 and -0.0 included) by ascending sample index, NaNs among themselves by index.  Everything after the sort is the
reference's loop, line by line: Python floats, one fp64 division per positive, one fp64 addition per positive, in walk order."""
import math

import numpy as np


def reduce_target(t):
    """What the meter stores of a target: 1 for == 1, 0 for == 0, -1 for anything else (NaN included)."""
    t = float(t)
    return 1 if t == 1 else 0 if t == 0 else -1


def walk_order(scores):
    """Sample indices of one class column in walk order."""
    def key(i):
        s = float(scores[i])
        return (0, 0.0, i) if math.isnan(s) else (1, -s, i)         # -(-0.0) == -(+0.0) as Python compares them
    return sorted(range(len(scores)), key=key)


def average_precision(scores, targets, difficult_examples, order=None):
    """-> (ap as a Python float, NaN without a counted positive; positives; counted samples).  order: walk_order(scores), when the
    caller has it already (it does not depend on difficult_examples)."""
    pos_count = 0.
    total_count = 0.
    precision_at_i = 0.
    for i in (walk_order(scores) if order is None else order):
        label = reduce_target(targets[i])
        if difficult_examples and label == 0:
            continue
        if label == 1:
            pos_count += 1
        total_count += 1
        if label == 1:
            precision_at_i += pos_count / total_count
    if pos_count == 0:
        return float("nan"), 0, int(total_count)
    precision_at_i /= pos_count
    return precision_at_i, int(pos_count), int(total_count)


def evaluate(scores, targets, difficult_examples, orders=None):
    """scores [N, C] (anything numpy reads as fp32), targets [N, C] -> {'ap' fp64 [C], 'npos' int32 [C], 'ncounted' int32 [C], 'map'}.
    orders: walk_orders(scores), to share the sorts between the two settings of difficult_examples."""
    scores = np.asarray(scores, dtype=np.float32).reshape(len(scores), -1)
    targets = np.asarray(targets).reshape(len(targets), -1)
    C = scores.shape[1]
    ap, npos, ncounted = np.zeros(C, np.float64), np.zeros(C, np.int32), np.zeros(C, np.int32)
    for c in range(C):
        ap[c], npos[c], ncounted[c] = average_precision(scores[:, c].tolist(), targets[:, c].tolist(), difficult_examples,
                                                        None if orders is None else orders[c])
    have = npos > 0
    return {"ap": ap, "npos": npos, "ncounted": ncounted, "map": float(np.mean(ap[have])) if have.any() else float("nan")}


def walk_orders(scores):
    scores = np.asarray(scores, dtype=np.float32).reshape(len(scores), -1)
    return [walk_order(scores[:, c].tolist()) for c in range(scores.shape[1])]
