"""The rules of spe_pseudo_quality (csrc/pseudo_quality.hip; include/spe_hip.h) restated in numpy: every fp32
operation of the kernel is one numpy fp32 operation, every count a Python integer.  Written as loops over rows and pairs - the shape of
the rules, not of the kernel, and not of the meter's torch composition either."""
import numpy as np

NAMES = ("pairs", "pairs_lead_hit", "pairs_any_hit", "pairs_empty", "rows", "rows_hit", "rows_orphan", "gts", "gts_covered", "iou_q")
F = np.float32


def corners(rows):
    """box_cxcywh_to_xyxy in fp32: [cx - 0.5 w, cy - 0.5 h, cx + 0.5 w, cy + 0.5 h]."""
    rows = np.asarray(rows, F).reshape(-1, 4)
    cx, cy, w, h = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    with np.errstate(all="ignore"):
        return np.stack([cx - F(0.5) * w, cy - F(0.5) * h, cx + F(0.5) * w, cy + F(0.5) * h], 1).astype(F)


def iou_matrix(rows, grows):
    """box_iou of the corners of both sides -> fp32 [t, g]: areas, max / min (numpy's propagate a NaN, like torch's), the sides clamped
    at 0 (a NaN stays), inter, (area1 + area2) - inter, the division."""
    a, b = corners(rows), corners(grows)
    with np.errstate(all="ignore"):
        area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
        area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        w = np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0])
        h = np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1])
        w, h = np.where(w < 0, F(0), w), np.where(h < 0, F(0), h)
        inter = w * h
        union = (area_a[:, None] + area_b[None, :]) - inter
        out = inter / union
    assert out.dtype == F
    return out


def lead_row(rows, scores):
    """rows: the ascending pseudo rows of one class.  Without scores the first; with scores the first NaN, else the first of the largest."""
    if scores is None:
        return rows[0]
    best = rows[0]
    for t in rows[1:]:
        if np.isnan(scores[best]):
            break
        if np.isnan(scores[t]) or scores[t] > scores[best]:
            best = t
    return best


def quantise(best):
    if not np.isfinite(best) or not best > 0:
        return 0
    return int(np.rint(min(F(best), F(1)) * F(1 << 20)))          # exact product; rint rounds half to even, as llrint does


def image(rows, labels, scores, grows, glabels, C, thr, counters):
    """One image added into counters, int64 [10, C + 1]."""
    thr = F(thr)
    T, G = len(labels), len(glabels)
    iou = iou_matrix(rows, grows)
    cls = [int(l) if 0 <= int(l) < C else -1 for l in labels]
    gcls = [int(l) if 0 <= int(l) < C else -1 for l in glabels]
    hit, covered = [False] * T, [False] * G
    for t in range(T):
        counters[4, C if cls[t] < 0 else cls[t]] += 1
    for g in range(G):
        counters[7, C if gcls[g] < 0 else gcls[g]] += 1
    by_class = {}
    for g in range(G):
        if gcls[g] >= 0:
            by_class.setdefault(gcls[g], []).append(g)
    for t in range(T):
        c = cls[t]
        if c < 0:
            continue
        mine = by_class.get(c)
        if not mine:
            counters[6, c] += 1
            continue
        v = iou[t, mine]
        with np.errstate(invalid="ignore"):
            for g in np.asarray(mine)[v > thr]:                   # a NaN compares false
                covered[g] = True
        v = v[~np.isnan(v)]
        best = v.max() if v.size else F(-np.inf)
        hit[t] = bool(best > thr)
        counters[5, c] += int(hit[t])
        counters[9, c] += quantise(best)
    for g in range(G):
        if covered[g]:
            counters[8, gcls[g]] += 1
    for c in by_class:
        rows_c = [t for t in range(T) if cls[t] == c]
        counters[0, c] += 1
        if not rows_c:
            counters[3, c] += 1
            continue
        counters[1, c] += int(hit[lead_row(rows_c, scores)])
        counters[2, c] += int(any(hit[t] for t in rows_c))
    return counters


def quality(boxes, labels, scores, off, gboxes, glabels, goff, C, thr, counters=None):
    """The whole batch -> int64 [10, C + 1]; counters: what the sums start from (a copy is made)."""
    out = np.zeros((len(NAMES), C + 1), np.int64) if counters is None else np.array(counters, np.int64)
    boxes, gboxes = np.asarray(boxes, F).reshape(-1, 4), np.asarray(gboxes, F).reshape(-1, 4)
    for b in range(len(off) - 1):
        p, g = slice(off[b], off[b + 1]), slice(goff[b], goff[b + 1])
        image(boxes[p], np.asarray(labels)[p], None if scores is None else np.asarray(scores, F)[p], gboxes[g], np.asarray(glabels)[g], C,
              thr, out)
    return out


def summary(counters, C):
    """The per-class ratios and their means over the classes with a denominator, fp64 -> {name: (per class [C], mean)}."""
    c = np.asarray(counters)[:, :C]
    out = {}
    for name, num, den in (("corloc", c[1], c[0]), ("any_hit", c[2], c[0]), ("precision", c[5], c[4]), ("recall", c[8], c[7]),
                           ("mean_iou", c[9] / float(1 << 20), c[4] - c[6])):
        per = np.array([float(n) / float(d) if d > 0 else np.nan for n, d in zip(num, den)], np.float64)
        have = ~np.isnan(per)
        out[name] = (per, float(per[have].mean()) if have.any() else float("nan"))
    return out
