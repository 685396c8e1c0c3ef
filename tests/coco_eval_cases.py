"""Named shapes of the COCO meter tests (tests/test_coco_meter_cpu.py, tests/test_coco_meter_gpu.py, tools/coco_meter_cost.py), the
seeded builders of their synthetic inputs and the helpers both test files share.  Boxes are integers or half-integers, so the IoUs
the cases turn on are exact in fp64.  An image is the dict tests/coco_eval_ref.py describes."""
import numpy as np
import torch

MAX_DET, MAX_GT = 4096, 512               # per image: accepted; one more: status -2
T, A = 10, 4
DET_COUNTS = (1, 63, 64, 65, 100, 101, 130)        # per (image, category): the wave width, the 100 that are evaluated, beyond
ACC_ND = (0, 1, 255, 256, 257, 513)                # records per category: the 256-wide chunk and its carries


def image(image_id, dets, gts):
    """dets: [(xyxy, score, label)], gts: [(xywh, label, iscrowd, area or None for w * h)]."""
    return {"boxes": np.array([d[0] for d in dets], np.float32).reshape(-1, 4), "scores": np.array([d[1] for d in dets], np.float32),
            "labels": np.array([d[2] for d in dets], np.int64),
            "gt_boxes": np.array([g[0] for g in gts], np.float64).reshape(-1, 4), "gt_labels": np.array([g[1] for g in gts], np.int64),
            "iscrowd": np.array([g[2] for g in gts], np.uint8),
            "area": np.array([g[0][2] * g[0][3] if g[3] is None else g[3] for g in gts], np.float64), "image_id": image_id}


def random_image(rng, image_id, cat_ids, gt_counts, det_counts, frame=400, noise_labels=()):
    """gt_counts[k] boxes and det_counts[k] detections of category cat_ids[k].  Detections are half-integer jitters of the category's
    boxes (a fifth lands exactly on its box, a tenth of the boxes is duplicated: equal IoUs), scores repeat (2 decimals), an eighth of
    the boxes is crowd, the area field is w * h scaled by 0.5 .. 1 (a segment's area), sizes straddle 32^2 and 96^2."""
    dets, gts = [], []
    for k, cid in enumerate(cat_ids):
        g, d = gt_counts[k], det_counts[k]
        side = rng.choice([12, 24, 32, 48, 96, 128], (g, 2))
        xy = rng.integers(0, frame - 130, (g, 2))
        b = np.concatenate([xy, side + rng.integers(0, 9, (g, 2))], 1).astype(np.float64).reshape(-1, 4)
        for q in range(1, g):
            if rng.random() < 0.1:
                b[q] = b[rng.integers(0, q)]
        for q in range(g):
            exact = rng.random() < 0.3
            gts.append((b[q].tolist(), cid, int(rng.random() < 0.125), None if exact else float(np.floor(b[q, 2] * b[q, 3] * rng.uniform(0.5, 1)))))
        if g:
            src = b[rng.integers(0, g, d)]
            jit = rng.integers(-8, 9, (d, 4)) * 0.5 * (rng.random((d, 1)) < 0.8)
            box = src + jit
            box[:, 2:] = np.maximum(box[:, 2:], 1.0)
        else:
            box = np.concatenate([rng.integers(0, frame - 70, (d, 2)), rng.integers(4, 140, (d, 2)) * 0.5], 1).astype(np.float64)
        s = np.round(rng.random(d), 2 if d > 3 else 6)
        dets += [((bx[0], bx[1], bx[0] + bx[2], bx[1] + bx[3]), sc, cid) for bx, sc in zip(box.reshape(-1, 4), s)]
    for lab in noise_labels:                                   # category ids the meter does not know: dropped on both sides
        dets.append(((5., 5., 45., 45.), 0.9, lab)); gts.append(([5., 5., 40., 40.], lab, 0, None))
    order = rng.permutation(len(dets))                          # detections arrive unsorted: update() orders them
    return image(image_id, [dets[o] for o in order], gts)


def _presence():
    """(image, category) pairs with detections and no ground truth, with ground truth and no detections, with neither, with both."""
    return [1, 2, 3, 4], [
        image(7, [((0, 0, 20, 20), .9, 1), ((5, 5, 30, 30), .8, 1), ((0, 0, 40, 40), .7, 4)],
              [([0, 0, 20, 20], 2, 0, None), ([0, 0, 40, 40], 4, 0, None)]),
        image(3, [], [([10, 10, 50, 50], 1, 0, None)]),
        image(5, [((10, 10, 60, 60), .5, 1)], [])]


def _counts():
    """One image, the seven detection counts of DET_COUNTS as seven categories, 3 boxes each."""
    rng = np.random.default_rng(100)
    cats = list(range(11, 18))
    return cats, [random_image(rng, 42, cats, [3] * 7, DET_COUNTS)]


def _equal_iou():
    """Two boxes with the same IoU (90 / 110) to the first detection: the LAST takes it.  The second detection sits on the second box
    (IoU 1) and overlaps the first by 80 / 120: with the second box gone it is matched up to t = 0.65 and not at 0.7 .. 0.8."""
    return [1], [image(1, [((1, 0, 11, 10), .9, 1), ((2, 0, 12, 10), .8, 1)], [([0, 0, 10, 10], 1, 0, None), ([2, 0, 10, 10], 1, 0, None)])]


def _keep_nonignored():
    """IoU 0.6 with a plain box, 1.0 (60 / its own area) with the crowd box that arrives before it: the plain box is visited first and
    the walk stops at the ignored group, so up to t = 0.55 the detection is a true positive; from 0.65 on it goes to the crowd."""
    return [1], [image(1, [((0, 0, 10, 6), .9, 1)], [([0, 0, 10, 9], 1, 1, None), ([0, 0, 10, 10], 1, 0, None)])]


def _crowd3():
    """Three detections inside one crowd box: IoU = intersection / detection area = 1, all matched, all ignored; a fourth outside."""
    return [1], [image(1, [((10, 10, 30, 30), .9, 1), ((40, 40, 70, 70), .8, 1), ((5, 50, 25, 90), .7, 1), ((200, 200, 240, 240), .6, 1)],
                       [([0, 0, 100, 100], 1, 1, None)])]


def _area_edges():
    """Area fields of exactly 32^2 and 96^2: small AND medium, medium AND large (the bounds are inclusive on both sides)."""
    return [1], [image(1, [((0, 0, 32, 32), .9, 1), ((100, 100, 196, 196), .8, 1)],
                       [([0, 0, 32, 32], 1, 0, 32. ** 2), ([100, 100, 96, 96], 1, 0, 96. ** 2)])]


def _det_outside():
    """An unmatched 200 x 200 detection is ignored in 'small' and 'medium' and a false positive in 'all' and 'large'."""
    return [1], [image(1, [((0, 0, 200, 200), .9, 1), ((300, 300, 320, 320), .8, 1)], [([300, 300, 20, 20], 1, 0, None)])]


def _equal_scores():
    """Equal scores: the incoming order decides who meets the box first."""
    return [1], [image(1, [((0, 0, 10, 8), .5, 1), ((0, 0, 10, 10), .5, 1), ((0, 0, 10, 9), .5, 1)], [([0, 0, 10, 10], 1, 0, None)])]


def _free_at_075():
    """The first detection (IoU 0.6) takes the box at t <= 0.6; at t >= 0.65 the box is still free for the second (IoU 0.9)."""
    return [1], [image(1, [((0, 0, 10, 6), .9, 1), ((0, 0, 10, 9), .8, 1)], [([0, 0, 10, 10], 1, 0, None)])]


def _half_iou():
    """IoU exactly 0.5: matched at t = 0.5 (the test is iou < t), unmatched from 0.55 on."""
    return [1], [image(1, [((0, 0, 10, 5), .9, 1)], [([0, 0, 10, 10], 1, 0, None)])]


def _random(seed, nimg, cats, per_gt, per_det, noise=()):
    def build():
        rng = np.random.default_rng(seed)
        ims = []
        for i in range(nimg):
            gc = rng.integers(0, per_gt + 1, len(cats)) * (rng.random(len(cats)) < 0.7)
            dc = rng.integers(0, per_det + 1, len(cats)) * (rng.random(len(cats)) < 0.7)
            ims.append(random_image(rng, 1000 - 37 * i, cats, gc, dc, noise_labels=noise))
        return cats, ims
    return build


CASES = {"presence": _presence, "counts": _counts, "equal_iou": _equal_iou, "keep_nonignored": _keep_nonignored, "crowd3": _crowd3,
         "area_edges": _area_edges, "det_outside": _det_outside, "equal_scores": _equal_scores, "free_at_075": _free_at_075,
         "half_iou": _half_iou,
         "random_small": _random(1, 6, [1, 3, 7, 90], 4, 12, noise=(2, 91)),      # ids with gaps, unknown ids on both sides
         "random_dense": _random(2, 4, [5, 6], 12, 40)}                           # many boxes per category: long walks, duplicates


def case(name):
    return CASES[name]()


def big_image(n_det, n_gt):
    rng = np.random.default_rng([n_det, n_gt])
    return random_image(rng, 1, [1], [n_gt], [n_det])


def synthetic_run(seed, nimg, cats, dets_per_image=100, gts_per_image=7):
    """A whole evaluation run at dataset size (tools/coco_meter_cost.py): per image `dets_per_image` detections over a few categories."""
    rng = np.random.default_rng([seed, nimg, len(cats)])
    out = []
    for i in range(nimg):
        gc, dc = np.zeros(len(cats), int), np.zeros(len(cats), int)
        for c in rng.integers(0, len(cats), gts_per_image):
            gc[c] += 1
        for c in rng.choice(np.concatenate([np.nonzero(gc)[0], rng.integers(0, len(cats), 2)]), dets_per_image):
            dc[c] += 1
        out.append(random_image(rng, i, cats, gc, dc))
    return out


# ---- record streams for spe_coco_accumulate -------------------------------------------------------------------------------------
# category -> (records, kind, npig per area range).  Synthetic per-image evaluations in the form tests/coco_eval_ref.accumulate takes.
ACC_TABLE = ((0, "random", (3, 3, 3, 3)), (1, "random", (2, 1, 0, 5)), (255, "random", None), (256, "random", None),
             (257, "random", None), (513, "late_max", None), (130, "random", (0, 0, 0, 0)), (10, "quarter", (4, 4, 4, 4)))


def acc_evals(seed=0):
    """-> (evals, n_images, K).  Images hold up to 100 detections (ranks 0 .. 99), so the rank filters of maxDets 1 and 10 bite; scores
    repeat (ties are broken by image, then rank); matched and ignore bits are random except
      late_max, area range 0: the best-scoring record is a false positive and every other one a true positive - precision grows to the
                very end, so the envelope has to carry its maximum back across two chunk boundaries;
      quarter:  npig = 4 and a fixed fp, tp, ignored, fp, fp, fp, fp, ignored ... run - recall is 0.25 = recThrs[25] exactly from the
                second record on and never grows: precision is 1/2 up to recThrs[25] and 0 behind it.
    npig None: the true positives of the category at the loosest setting + 3 (recall stays below 1: the tail of precision is 0)."""
    rng = np.random.default_rng([seed, 55])
    evals, n_images = {}, 7
    for k, (nd, kind, npig) in enumerate(ACC_TABLE):
        sizes = [min(100, nd - 100 * i) for i in range(n_images) if nd - 100 * i > 0]
        sizes += [0] * (n_images - len(sizes))
        scores = [np.sort(np.round(rng.random(D), 2).astype(np.float32).astype(np.float64))[::-1] for D in sizes]
        if kind == "late_max":
            scores[2][0] = 2.0                                  # the single best record: image 2, rank 0
        for a in range(A):
            tot_tp = 0
            for i, D in enumerate(sizes):
                dtm, dig = rng.random((T, D)) < 0.5, rng.random((T, D)) < 0.2
                if kind == "late_max" and a == 0:
                    dtm[:], dig[:] = True, False
                    if i == 2:
                        dtm[:, 0] = False
                if kind == "quarter":
                    pat = np.arange(D) % 5
                    dtm[:], dig[:] = np.arange(D) == 1, pat == 2
                tot_tp += int((dtm & ~dig).sum(1).max()) if D else 0
                evals[(k, a, i)] = {"dtScores": scores[i], "dtMatches": dtm, "dtIgnore": dig, "gtIgnore": np.ones(2, bool)}
            n = tot_tp + 3 if npig is None else npig[a]
            evals[(k, a, 0)]["gtIgnore"] = np.concatenate([np.zeros(n, bool), np.ones(2, bool)])
    return evals, n_images, len(ACC_TABLE)


def acc_records(evals, n_images, K):
    """The same evaluations as the records spe_coco_accumulate takes: (words int32 [n,4], rank int32 [n], scores fp32 [n], seg_off int32
    [K+1], npig int32 [K,4]), per category in curve order (score descending, image ascending, rank)."""
    words, rank, score, seg, npig = [], [], [], [0], np.zeros((K, A), np.int32)
    for k in range(K):
        w, r, s, im = [], [], [], []
        for i in range(n_images):
            D = evals[(k, 0, i)]["dtScores"].size
            ws = np.zeros((D, A), np.int64)
            for a in range(A):
                e = evals[(k, a, i)]
                npig[k, a] += int((~e["gtIgnore"]).sum())
                for t in range(T):
                    ws[:, a] |= (e["dtMatches"][t].astype(np.int64) << t) | (e["dtIgnore"][t].astype(np.int64) << (T + t))
            w.append(ws.astype(np.int32)); r.append(np.arange(D, dtype=np.int32)); s.append(evals[(k, 0, i)]["dtScores"].astype(np.float32))
            im.append(np.full(D, i))
        w, r, s, im = np.concatenate(w), np.concatenate(r), np.concatenate(s), np.concatenate(im)
        o = np.lexsort((r, im, -s.astype(np.float64)))
        words.append(w[o]); rank.append(r[o]); score.append(s[o]); seg.append(seg[-1] + r.size)
    return np.concatenate(words), np.concatenate(rank), np.concatenate(score), np.array(seg, np.int32), npig


# ---- shared by the CPU and the GPU tests ------------------------------------------------------------------------------------------
def split(images, device="cpu"):
    """image dicts -> (results, gts) as the meter takes them."""
    t = lambda v: torch.as_tensor(v).to(device)
    res = [{"boxes": t(im["boxes"]), "scores": t(im["scores"]), "labels": t(im["labels"])} for im in images]
    gts = [{"boxes": t(im["gt_boxes"]), "labels": t(im["gt_labels"]), "iscrowd": t(im["iscrowd"]), "area": t(im["area"]),
            "image_id": im["image_id"]} for im in images]
    return res, gts


def run_meter(images, cat_ids, batches=None, device="cpu"):
    from spe_amd.evalmetrics import COCODetectionMeter
    m = COCODetectionMeter(cat_ids)
    for b in (batches if batches is not None else [list(range(len(images)))]):
        m.update(*split([images[i] for i in b], device))
    return m


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b)


def check_against(out, ref):
    """out: summarize(return_records=True) of the meter; ref: coco_eval_ref.evaluate.  Everything exactly."""
    for k in ("cat", "img", "rank", "score", "words"):
        assert same(out["records"][k], ref["records"][k]), k
    assert same(out["npig"], ref["npig"])
    for k in ("precision", "recall", "scores"):
        assert same(out["eval"][k], ref[k]), k
    assert same(out["stats"], ref["stats"]), (out["stats"], ref["stats"])
