"""Inputs for spe_proposal_recall and ProposalRecallMeter (csrc/proposal_recall.hip; tests/proposal_recall_ref.py restates the rules): the
smallest shapes at which the kernel can go wrong.  One workgroup of 256 threads works on an image; its four waves stride over the
ground-truth rows, the 64 lanes of a wave over the Q queries (at most 1024: 16 per lane).

  q1          B 2, Q 1     rows (1, 5); T, K = 1, 1; ks (1): one query - it leads whenever it covers
  q63         B 3, Q 63    rows (5, 0, 1): the lane tail; an image WITHOUT rows between two that have some; T, K = 2, 3; ks (1, Q, Q + 5)
  q64         B 1, Q 64    rows (5): a full wave, one image; T, K = 2, 3
  q65         B 2, Q 65    rows (257, 1): the second round of the lanes, more rows than threads; T, K = 8, 8
  q300        B 2, Q 300   rows (5, 257), Kc 21: the flagship shape; T, K = 2, 3; ks (1, 10, 100)
  q300_c10    the same with C = 10 < Kc = 21: labels 10 .. 20 are dropped
  q1024       B 2, Q 1024  rows (5, 1): the limit, every LDS slot and all 16 registers of a lane; T, K = 8, 8; ks up to Q and Q + 5
  ties        Q 65: probabilities in runs of equal values (multiples of 1/4): ties go to the lower query
  zeros       Q 65: +0.0 against -0.0 (equal), a few 0.5
  nans        Q 65: about one probability in eight a NaN, NaNs first among themselves by lower query
  saturated   Q 65: every probability 1.0 (a saturated sigmoid): the class's order is the query order
  wild        Q 65: NaN and infinite coordinates, zero-area boxes (0 / 0) on both sides, queries identical to a ground-truth row
  labels      Q 5, Kc 5, C 8: labels -1, 5 = Kc, 8 = C dropped, 4 = Kc - 1 kept; labels_c3: C 3 < Kc 5, labels 3 and 4 dropped
  hand        B 4, Q 6: hand-made rows, see hand_images(): an IoU of exactly 0.5 and one of exactly 0.75 out of dyadic coordinates that
              must NOT hit, identical boxes, NaN / infinite / zero-area queries, a zero-area ground-truth row, a NaN probability that
              comes first, a class whose ceiling exceeds its recall at k = 1 (the selection gap) while that recall is not 0
  *_preload   counters that already hold values: the kernel adds, it does not store

Random images: ground truth drawn uniformly; half of the queries are a ground-truth row of the image, jittered, so covers and near
misses both occur; about one label in sixteen lies outside [0, min(C, Kc)).  `plan()` says what every case reaches;
tests/test_proposal_recall_cpu.py checks it against this docstring's list."""
import numpy as np

import proposal_recall_ref as R

F = np.float32
LIMIT_Q = 1024
GUARD, GUARD_WORDS = -0x5A5A5A5A5A5A5A5, 32        # what lies around the counters before and after a launch
THR2, THR8 = (0.5, 0.75), (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.75, 0.9)


def _labels(g, n, limit):
    lab = g.integers(0, limit, n).astype(np.int64)
    if limit > 2:
        lab[g.random(n) < 0.5] = limit - 1 if g.random() < 0.5 else 0          # several rows of one class: its order is walked more than once
    bad = g.random(n) < 1.0 / 16
    lab[bad] = np.array([-1, -7, limit, limit + 2], np.int64)[g.integers(0, 4, int(bad.sum()))]
    return lab


def _prob(g, kind, B, Q, Kc):
    p = g.random((B, Q, Kc)).astype(F)
    if kind == "ties":
        p = (np.floor(p * 4) / 4).astype(F)
    elif kind == "zeros":
        p = np.where(g.random(p.shape) < 0.5, F(0.0), F(-0.0)).astype(F)
        p[g.random(p.shape) < 0.1] = F(0.5)
    elif kind == "nans":
        p[g.random(p.shape) < 0.125] = np.nan
    elif kind == "saturated":
        p[:] = F(1.0)
    elif kind != "free":
        raise ValueError(kind)
    return p


def random_batch(g, B, Q, Kc, C, rows, prob="free", wild=False):
    """-> prob [B, Q, Kc], boxes [B, Q, 4], gboxes [G, 4], glabels [G], goff."""
    boxes = np.concatenate([g.uniform(0.2, 0.8, (B, Q, 2)), g.uniform(0.05, 0.4, (B, Q, 2))], 2).astype(F)
    gbs, gls, picks = [], [], []
    for b, ng in enumerate(rows):
        gb = np.concatenate([g.uniform(0.2, 0.8, (ng, 2)), g.uniform(0.05, 0.4, (ng, 2))], 1).astype(F)
        if ng:
            src, near = g.integers(0, ng, Q), g.random(Q) < 0.5
            jitter = (1 + g.uniform(-0.2, 0.2, (Q, 4))).astype(F)
            boxes[b][near] = (gb[src] * jitter)[near]
            if wild:
                boxes[b, 0] = gb[0]                                          # identical to a ground-truth row: IoU exactly 1
        picks.append((src, near) if ng else (np.zeros(Q, np.int64), np.zeros(Q, bool)))
        gbs.append(gb)
        gls.append(_labels(g, ng, min(C, Kc)))
    if wild:
        for b in range(B):
            boxes[b, 3, 0] = np.nan
            boxes[b, 5, 2] = np.inf
            boxes[b, 7, 0] = -np.inf
            boxes[b, 9, 2:] = 0.0                                            # zero area
            boxes[b, Q - 1, 1] = np.nan                                      # in the lane tail
            if len(gbs[b]) > 2:
                gbs[b][1, 2:] = 0.0
                boxes[b, 11] = gbs[b][1]                                     # zero area against the same zero area: 0 / 0
                gbs[b][2, 0] = np.nan
    p = _prob(g, prob, B, Q, Kc)
    if prob == "free":
        for b, (lab, (src, near)) in enumerate(zip(gls, picks)):
            for q in np.nonzero(near)[0]:
                if 0 <= lab[src[q]] < Kc and g.random() < 0.5:
                    p[b, q, lab[src[q]]] = F(0.5 + 0.5 * g.random())         # half of the near queries know their class: the pick often covers
    return p, boxes, np.concatenate(gbs).reshape(-1, 4), np.concatenate(gls), [0] + np.cumsum(rows).tolist()


FILL = (0.0625, 0.0625, 0.0625, 0.0625)            # a query in the corner: overlaps no hand-made ground-truth row
HAND_KS = (1, 2, 6, 11)                            # 1, 2, Q, Q + 5


def hand_images():
    """-> prob [4, 6, 4], boxes [4, 6, 4], gboxes, glabels, goff; C = Kc = 4, thresholds (0.5, 0.75), ks HAND_KS.  Every corner is dyadic."""
    nan, inf = np.nan, np.inf
    big, small = (0.5, 0.5, 0.5, 0.5), (0.5, 0.5, 0.25, 0.25)
    boxes = np.array([
        [(0.5, 0.625, 0.5, 0.25), FILL, FILL, FILL, FILL, FILL],                                     # IoU with `big` exactly 0.5: no hit
        [FILL, FILL, (0.5, 0.5625, 0.5, 0.375), FILL, FILL, FILL],                                   # exactly 0.75: covers at 0.5 only
        [(nan, 0.5, 0.2, 0.2), (0.5, 0.5, inf, 0.2), (0.5, 0.5, 0.0, 0.0), small, FILL, small],      # NaN, infinite, zero area, identical twice
        [small, FILL, FILL, FILL, FILL, FILL]], F)
    prob = np.full((4, 6, 4), 0.125, F)
    prob[1, :, 1] = [0.9, 0.8, 0.7, 0.6, 0.5, 0.4]                  # two queries come before the covering one: r = 2
    prob[2, :, 2] = [0.9, nan, 0.5, 0.5, 0.5, 0.5]                  # order 1 (NaN), 0, 2, 3, 4, 5: the lead of {3, 5} is 3, r = 3
    prob[3, :, 2] = [0.9, 0.5, 0.5, 0.5, 0.5, 0.5]                  # the pick covers: r = 0
    gboxes = np.array([big, big, small, (0.5, 0.5, 0.0, 0.0), small, small, small], F)
    glabels = np.array([1, 1, 2, 0, 2, -1, 4], np.int64)            # image 3 also has a label below 0 and one at C
    return prob, boxes, gboxes, glabels, [0, 1, 2, 4, 7]


def hand_expected():
    """What hand_images() counts, written out: rows gts, iou_q, ceil[0..1], hit[0][0..3], hit[1][0..3]; columns classes 0 .. 3 and dropped."""
    q = R.IOU_SCALE
    return np.array([[1, 2, 2, 0, 2],
                     [0, q // 2 + 3 * q // 4, 2 * q, 0, 0],
                     [0, 1, 2, 0, 0], [0, 0, 2, 0, 0],
                     [0, 0, 1, 0, 0], [0, 0, 1, 0, 0], [0, 1, 2, 0, 0], [0, 1, 2, 0, 0],
                     [0, 0, 1, 0, 0], [0, 0, 1, 0, 0], [0, 0, 2, 0, 0], [0, 0, 2, 0, 0]], np.int64)


class Case:
    """A batch: prob [B, Q, Kc] fp32, boxes [B, Q, 4] fp32, gboxes [G, 4], glabels [G] int64, goff [B + 1]; C, thr, ks; preload: the
    counters the launch starts from (int64 [2 + T + T * K, C + 1]) or None for zeros."""

    def __init__(self, name, C, batch, thr, ks, preload=False, empty=False):
        self.name, self.C, self.thr, self.ks, self.empty = name, C, tuple(thr), tuple(ks), empty
        self.prob, self.boxes, self.gboxes, self.glabels, self.goff = batch
        self.B, self.Q, self.Kc = self.prob.shape
        self.T, self.K = len(self.thr), len(self.ks)
        self.rows = 2 + self.T + self.T * self.K
        self.preload = None
        if preload:
            self.preload = np.random.default_rng(len(name)).integers(-5, 1 << 40, (self.rows, C + 1)).astype(np.int64)
        self._expected = None

    def expected(self):
        """The restatement's counters, computed once and handed out read-only."""
        if self._expected is None:
            self._expected = R.recall(self.prob, self.boxes, self.gboxes, self.glabels, self.goff, self.C, self.thr, self.ks, self.preload)
            self._expected.setflags(write=False)
        return self._expected

    def outputs(self, torch, device):
        """{'pred_logits', 'pred_boxes'} for the meter, which orders by the sigmoid it computes itself: logits on a grid of eighths in
        [-4, 4] - distinct logits have clearly distinct sigmoids and equal ones tie, on any device - a NaN where self.prob has one and 30
        (saturated) where self.prob is 1.  The boxes are the case's."""
        g = np.random.default_rng(sum(map(ord, self.name)))
        logits = (g.integers(-32, 33, self.prob.shape) / 8).astype(F)
        logits[np.isnan(self.prob)] = np.nan
        logits[self.prob == 1] = 30.0
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        return {"pred_logits": up(logits), "pred_boxes": up(self.boxes)}

    def gts(self, torch, device):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        return [{"boxes": up(self.gboxes[a:b]), "labels": up(self.glabels[a:b])} for a, b in zip(self.goff[:-1], self.goff[1:])]


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        g = np.random.default_rng(20240607)
        rb = lambda *a, **k: random_batch(g, *a, **k)
        ks8 = lambda Q: (1, 2, 3, 5, 10, 20, Q, Q + 5)
        _CASES = [
            Case("q1", 3, _q1_batch(g), (0.3,), (1,)),
            Case("q63", 21, rb(3, 63, 21, 21, (5, 0, 1)), THR2, (1, 63, 68)),
            Case("q64", 21, rb(1, 64, 21, 21, (5,)), THR2, (1, 10, 64)),
            Case("q65", 21, rb(2, 65, 21, 21, (257, 1)), THR8, ks8(65)),
            Case("q300", 21, rb(2, 300, 21, 21, (5, 257)), THR2, (1, 10, 100)),
            Case("q300_c10", 10, rb(2, 300, 21, 21, (5, 257)), THR2, (1, 10, 100)),
            Case("q1024", 21, rb(2, 1024, 21, 21, (5, 1)), THR8, ks8(1024)),
            Case("ties", 6, rb(2, 65, 6, 6, (5, 257), prob="ties"), THR2, (1, 2, 3)),
            Case("zeros", 6, rb(2, 65, 6, 6, (5, 257), prob="zeros"), THR2, (1, 2, 3)),
            Case("nans", 6, rb(2, 65, 6, 6, (5, 257), prob="nans"), THR2, (1, 2, 3)),
            Case("saturated", 6, rb(2, 65, 6, 6, (5, 257), prob="saturated"), THR2, (1, 2, 3)),
            Case("wild", 6, rb(2, 65, 6, 6, (5, 257), prob="nans", wild=True), THR2, (1, 10, 65)),
            Case("labels", 8, _label_batch(g, 5, [-1, 5, 8, 4, 0, 4]), THR2, (1, 5, 10)),
            Case("labels_c3", 3, _label_batch(g, 5, [3, 4, 2, 0, -1, 2]), THR2, (1, 5, 10)),
            Case("hand", 4, hand_images(), THR2, HAND_KS),
            Case("no_rows", 4, rb(2, 65, 4, 4, (0, 0)), THR2, (1, 2), empty=True),
            Case("q65_preload", 21, rb(2, 65, 21, 21, (5, 257)), THR8, ks8(65), preload=True),
            Case("hand_preload", 4, hand_images(), THR2, HAND_KS, preload=True),
        ]
    return _CASES


def _label_batch(g, Kc, labels):
    """One image of 5 queries, every ground-truth row identical to query 0 (it covers), under the given labels."""
    prob, boxes, _, _, _ = random_batch(g, 1, 5, Kc, Kc, (0,))
    return prob, boxes, np.repeat(boxes[0, :1], len(labels), 0), np.array(labels, np.int64), [0, len(labels)]


def _q1_batch(g):
    """Two images of ONE query, a little larger than the image's first ground-truth row: it covers that row at least."""
    prob, boxes, gboxes, glabels, goff = random_batch(g, 2, 1, 3, 3, (1, 5))
    boxes[:, 0] = gboxes[[0, 1]] * np.array([1, 1, 1.125, 1.125], F)
    glabels[[0, 1]] = (0, 2)
    return prob, boxes, gboxes, glabels, goff


def by_name(name):
    return next(c for c in cases() if c.name == name)


def plan():
    """What the cases reach -> dict of sets, for the coverage check."""
    cs = cases()
    return {"Q": {c.Q for c in cs}, "rows": {b - a for c in cs for a, b in zip(c.goff[:-1], c.goff[1:])},
            "TK": {(c.T, c.K) for c in cs}, "B": {c.B for c in cs},
            "empty_between": any(any(c.goff[i] < c.goff[i + 1] == c.goff[i + 2] < c.goff[i + 3] for i in range(c.B - 2)) for c in cs),
            "ks_1_Q_Q5": any({1, c.Q, c.Q + 5} <= set(c.ks) for c in cs),
            "C_below_Kc": any(c.C < c.Kc for c in cs), "preload": any(c.preload is not None for c in cs)}
