"""Inputs for spe_pseudo_quality and PseudoLabelMeter (csrc/pseudo_quality.hip; tests/pseudo_quality_ref.py restates the rules): the
smallest shapes at which the kernel can go wrong.  One workgroup of 256 threads works on an image, every thread striding over the rows,
and at most 1024 rows of either kind fit its LDS.

  counts_a   B 5, C 21   per-image (pseudo, ground truth) rows (0, 0), (1, 1), (63, 64), (0, 5), (64, 65): an empty image FIRST, an image
                         without pseudo rows in the MIDDLE (its pairs are all empty), one row of each kind, both sides of the wave width
  counts_b   B 2, C 91   (65, 1), (255, 0): one ground-truth row for many pseudo rows; an image without ground truth (every row an orphan)
  counts_c   B 5, C 21   (256, 64), (0, 0), (257, 65), (1, 0), (0, 0): both sides of the workgroup width (the second stride of the row
                         loops), an empty image in the MIDDLE and LAST
  full       B 1, C 91   (1024, 1024): the limit of both sides, every LDS slot in use
  full_thin  B 2, C 21   (1024, 1), (1, 1024): the limit of one side against one row of the other
  one_class  B 2, C 1    every kept label is 0 = C - 1: several rows of both kinds in the one class; labels -1 and 1 = C are dropped
  edges      B 2, C 21   hand-made geometry, see edge_images(): identical boxes (IoU exactly 1), touching boxes (IoU 0), zero-area boxes
                         (union 0: NaN), NaN and infinite coordinates on either side, an IoU of exactly 0.5 out of dyadic coordinates (no
                         hit) beside one just above (a hit), an orphan, a pair without a pseudo row, several ground-truth rows of one class,
                         a class whose lead row misses while a later row hits, labels at 0, at C - 1, below 0 and at C on both sides
  edges_*    the same rows with scores: `equal` (all the same: the lead row is the lowest, which misses), `nan` (a NaN on the hitting
             row: it leads), `best_last` (the hitting row has the largest score), `two_nans` (NaNs on both rows: the first leads)
  *_scored   the random cases once more with scores, equal scores and a NaN among them
  *_preload  counters that already hold values: the kernel accumulates

Random images: the ground truth is drawn uniformly; half of the pseudo rows are a ground-truth row of the image, jittered, under its
label - so hits, near misses and double covers all occur - the others are free.  About one label in sixteen lies outside [0, C).
`plan()` says what every case reaches; tests/test_pseudo_quality_cpu.py checks it against this docstring's list."""
import numpy as np

import pseudo_quality_ref as R

THRESH = 0.5
LIMIT = 1024
PSEUDO_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1024)
GT_COUNTS = (0, 1, 64, 65, 1024)
BATCHES = (1, 2, 5)
CLASSES = (1, 21, 91)
GUARD, GUARD_WORDS = -0x5A5A5A5A5A5A5A5, 32        # what lies around the counters before and after a launch


def _labels(g, n, C, spread):
    """n labels from `spread` classes that include 0 and C - 1; about one in sixteen outside [0, C): -1, -7, C, C + 2."""
    pool = np.unique(np.concatenate([[0, C - 1], g.integers(0, C, max(spread - 2, 0))])).astype(np.int64)
    lab = pool[g.integers(0, len(pool), n)]
    bad = g.random(n) < 1.0 / 16
    lab[bad] = np.array([-1, -7, C, C + 2], np.int64)[g.integers(0, 4, int(bad.sum()))]
    return lab


def random_image(g, t, ng, C, spread=6):
    gb = np.concatenate([g.uniform(0.2, 0.8, (ng, 2)), g.uniform(0.05, 0.4, (ng, 2))], 1).astype(np.float32)
    gl = _labels(g, ng, C, spread)
    pb = np.concatenate([g.uniform(0.2, 0.8, (t, 2)), g.uniform(0.05, 0.4, (t, 2))], 1).astype(np.float32)
    pl = _labels(g, t, C, spread)
    if ng:
        src = g.integers(0, ng, t)
        near = g.random(t) < 0.5
        jitter = (1 + g.uniform(-0.25, 0.25, (t, 4))).astype(np.float32)
        pb[near] = (gb[src] * jitter)[near]
        pl[near] = gl[src][near]
    return pb, pl, gb, gl


def edge_images():
    """-> two images (rows, labels, ground-truth rows, ground-truth labels), C = 21.  Corners of every hand-made box are dyadic."""
    nan, inf = np.nan, np.inf
    d = 2.0 ** -10
    p0 = [((0.5, 0.5, 0.25, 0.25), 3),          # identical to its ground-truth row: IoU exactly 1
          ((nan, 0.5, 0.2, 0.2), 3),            # a NaN coordinate: every IoU NaN, no hit, not an orphan
          ((inf, 0.5, 0.2, 0.2), 3),            # an infinite centre: inf - inf in the area
          ((0.5, 0.5, inf, 0.2), 3),            # an infinite width: union inf, IoU 0
          ((0.625, 0.375, 0.25, 0.25), 4),      # touches its ground-truth row along x = 0.5: IoU 0
          ((0.5, 0.5, 0.0, 0.0), 5),            # zero area on both sides: 0 / 0
          ((0.25, 0.125, 0.5, 0.25), 7),        # half of its ground-truth row: IoU exactly 0.5, no hit
          ((0.25, 0.125 + d / 2, 0.5, 0.25 + d), 8),   # a sliver more: a hit
          ((0.3, 0.3, 0.1, 0.1), 9),            # no ground truth of class 9: an orphan
          ((0.75, 0.75, 0.25, 0.25), 11),       # the second of two ground-truth rows of class 11
          ((0.9, 0.9, 0.1, 0.1), 12),           # the lead row of class 12 misses ...
          ((0.25, 0.75, 0.25, 0.25), 12),       # ... the later row hits
          ((0.5, 0.5, 0.5, 0.5), 0), ((0.5, 0.5, 0.5, 0.5), 20), ((0.5, 0.5, 0.5, 0.5), -1), ((0.5, 0.5, 0.5, 0.5), 21)]
    g0 = [((0.5, 0.5, 0.25, 0.25), 3), ((0.375, 0.375, 0.25, 0.25), 4), ((0.5, 0.5, 0.0, 0.0), 5), ((0.5, nan, 0.2, 0.2), 6),
          ((0.25, 0.25, 0.5, 0.5), 7), ((0.25, 0.25, 0.5, 0.5), 8), ((0.5, 0.5, 0.3, 0.3), 10),          # class 10: a pair without a pseudo row
          ((0.25, 0.25, 0.25, 0.25), 11), ((0.75, 0.75, 0.25, 0.25), 11), ((0.25, 0.75, 0.25, 0.25), 12),
          ((0.5, 0.5, 0.5, 0.5), 0), ((0.5, 0.5, 0.5, 0.5), 20), ((0.5, 0.5, 0.5, 0.5), -3), ((0.5, 0.5, 0.5, 0.5), 21)]
    p1 = [((0.4, 0.4, 0.2, 0.2), 6), ((0.5, 0.5, 0.25, 0.25), 3)]        # class 3 again, another image: no ground truth here, an orphan
    g1 = [((0.4, 0.4, 0.2, 0.2), 6), ((-inf, 0.5, 0.2, 0.2), 6)]

    def arrays(rows):
        return np.array([r for r, _ in rows], np.float32).reshape(-1, 4), np.array([l for _, l in rows], np.int64)
    return [arrays(p0) + arrays(g0), arrays(p1) + arrays(g1)]


def edge_scores(kind):
    """Scores for the rows of edge_images(); the two rows of class 12 are rows 10 (misses) and 11 (hits) of image 0."""
    s = [np.linspace(0.9, 0.1, 16).astype(np.float32), np.float32([0.5, 0.5])]
    if kind == "equal":
        s[0][:] = 0.25
    elif kind == "nan":
        s[0][11] = np.nan
    elif kind == "best_last":
        s[0][10], s[0][11] = 0.125, 0.75
    elif kind == "two_nans":
        s[0][10] = s[0][11] = np.nan
    else:
        raise ValueError(kind)
    return s


class Case:
    """A batch, flat: boxes [T, 4] fp32, labels [T] int64, scores [T] fp32 or None, off [B + 1]; gboxes, glabels, goff; C, thr;
    preload: the counters the launch starts from (int64 [10, C + 1]) or None for zeros."""

    def __init__(self, name, C, images, scores=None, preload=False):
        self.name, self.C, self.thr, self.images = name, C, THRESH, images
        self.boxes = np.concatenate([i[0] for i in images]).astype(np.float32).reshape(-1, 4)
        self.labels = np.concatenate([i[1] for i in images]).astype(np.int64)
        self.gboxes = np.concatenate([i[2] for i in images]).astype(np.float32).reshape(-1, 4)
        self.glabels = np.concatenate([i[3] for i in images]).astype(np.int64)
        self.off = [0] + np.cumsum([len(i[1]) for i in images]).tolist()
        self.goff = [0] + np.cumsum([len(i[3]) for i in images]).tolist()
        self.scores = None if scores is None else np.concatenate(scores).astype(np.float32)
        self.image_scores = scores
        self.preload = None
        if preload:
            self.preload = (np.arange(10 * (C + 1), dtype=np.int64).reshape(10, C + 1) * 1000003 + (1 << 40))
        self._expected = None

    def expected(self):
        """The restatement's counters, computed once and shared."""
        if self._expected is None:
            self._expected = R.quality(self.boxes, self.labels, self.scores, self.off, self.gboxes, self.glabels, self.goff, self.C, self.thr,
                                       self.preload)
            self._expected.setflags(write=False)
        return self._expected

    def per_image(self, torch, device):
        """(pseudo list, gts list) of torch tensors: the form engine.get_refinements_pseudo_label returns and the loader's rows."""
        pseudo, gts = [], []
        for k, (pb, pl, gb, gl) in enumerate(self.images):
            p = {"boxes": torch.from_numpy(np.ascontiguousarray(pb, np.float32).reshape(-1, 4)).to(device), "labels": torch.from_numpy(np.asarray(pl, np.int64)).to(device)}
            if self.image_scores is not None:
                p["scores"] = torch.from_numpy(np.asarray(self.image_scores[k], np.float32)).to(device)
            pseudo.append(p)
            gts.append({"boxes": torch.from_numpy(np.ascontiguousarray(gb, np.float32).reshape(-1, 4)).to(device), "labels": torch.from_numpy(np.asarray(gl, np.int64)).to(device)})
        return pseudo, gts


_SHAPES = (("counts_a", 21, ((0, 0), (1, 1), (63, 64), (0, 5), (64, 65))),
           ("counts_b", 91, ((65, 1), (255, 0))),
           ("counts_c", 21, ((256, 64), (0, 0), (257, 65), (1, 0), (0, 0))),
           ("full", 91, ((1024, 1024),)),
           ("full_thin", 21, ((1024, 1), (1, 1024))),
           ("one_class", 1, ((40, 7), (5, 3))))
_CASES = None


def _random_scores(g, images):
    """Scores in steps of 1/8 (many equal) with a NaN in every image that has three rows or more."""
    out = []
    for im in images:
        s = (g.integers(0, 9, len(im[1])) / 8.0).astype(np.float32)
        if len(s) >= 3:
            s[g.integers(0, len(s))] = np.nan
        out.append(s)
    return out


def cases():
    """The list, built once."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    for k, (name, C, counts) in enumerate(_SHAPES):
        g = np.random.default_rng(100 + k)
        images = [random_image(g, t, ng, C, spread=24 if C == 91 else 6) for t, ng in counts]
        out.append(Case(name, C, images))
        if name in ("counts_a", "counts_c", "one_class", "full_thin"):
            out.append(Case(name + "_scored", C, images, scores=_random_scores(g, images), preload=name == "counts_c"))
    out.append(Case("edges", 21, edge_images()))
    for kind in ("equal", "nan", "best_last", "two_nans"):
        out.append(Case("edges_" + kind, 21, edge_images(), scores=edge_scores(kind)))
    out.append(Case("edges_preload", 21, edge_images(), preload=True))
    out.append(Case("counts_b_preload", 91, out[[c.name for c in out].index("counts_b")].images, preload=True))
    _CASES = out
    return out


def by_name(name):
    return next(c for c in cases() if c.name == name)


def plan():
    """What the case list reaches -> dict of sets / flags, from the inputs and the restatement's own IoUs."""
    seen = {"pseudo_counts": set(), "gt_counts": set(), "B": set(), "C": set(), "empty_at": set(), "labels": set(), "glabels": set(),
            "iou_one": False, "iou_touching": False, "iou_nan_zero_area": False, "nan_coord": set(), "inf_coord": set(),
            "iou_threshold_no_hit": False, "orphans": False, "pairs_empty": False, "gt_same_class": False, "rows_same_class": {False: False, True: False},
            "equal_scores": False, "nan_score": False, "lead_misses_later_hits": {False: False, True: False}, "preload": False}
    for c in cases():
        B = len(c.images)
        seen["B"].add(B)
        seen["C"].add(c.C)
        seen["preload"] |= c.preload is not None
        scored = c.scores is not None
        e = c.expected() - (0 if c.preload is None else c.preload)
        seen["orphans"] |= bool(e[6, :c.C].sum() > 0)
        seen["pairs_empty"] |= bool(e[3, :c.C].sum() > 0)
        seen["lead_misses_later_hits"][scored] |= bool((e[2, :c.C] > e[1, :c.C]).any())
        for b, (pb, pl, gb, gl) in enumerate(c.images):
            seen["pseudo_counts"].add(len(pl))
            seen["gt_counts"].add(len(gl))
            if len(pl) == 0 and len(gl) == 0 and B == 5:
                seen["empty_at"].add("first" if b == 0 else "last" if b == B - 1 else "middle")
            for key, lab in (("labels", pl), ("glabels", gl)):
                for what, hit in (("zero", lab == 0), ("top", lab == c.C - 1), ("below", lab < 0), ("at_C", lab == c.C)):
                    if hit.any():
                        seen[key].add(what)
            kept_g, kept_p = gl[(gl >= 0) & (gl < c.C)], pl[(pl >= 0) & (pl < c.C)]
            seen["gt_same_class"] |= len(np.unique(kept_g)) < len(kept_g)
            seen["rows_same_class"][scored] |= len(np.unique(kept_p)) < len(kept_p)
            for side, rows in (("pseudo", pb), ("gt", gb)):
                if np.isnan(rows).any():
                    seen["nan_coord"].add(side)
                if np.isinf(rows).any():
                    seen["inf_coord"].add(side)
            if scored:
                s = c.image_scores[b]
                for l in np.unique(kept_p):
                    v = s[pl == l]
                    seen["nan_score"] |= bool(np.isnan(v).any() and len(v) > 1)
                    v = v[~np.isnan(v)]
                    seen["equal_scores"] |= bool(len(v) > 1 and (v == v.max()).sum() > 1)
            if c.name == "edges":
                iou = R.iou_matrix(pb, gb)
                same = pl[:, None] == gl[None, :]
                zero_area = (pb[:, 2] * pb[:, 3] == 0)[:, None] & (gb[:, 2] * gb[:, 3] == 0)[None, :]
                seen["iou_one"] |= bool((same & (iou == 1)).any())
                seen["iou_touching"] |= bool((same & (iou == 0) & np.isfinite(pb).all(1)[:, None]).any())
                seen["iou_nan_zero_area"] |= bool((same & zero_area & np.isnan(iou)).any())
                at = same & (iou == np.float32(THRESH))
                seen["iou_threshold_no_hit"] |= bool(at.any()) and e[5, 7] == 0 and e[4, 7] == 1 and e[5, 8] == 1
    return seen
