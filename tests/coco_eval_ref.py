"""The published COCOeval algorithm for iouType 'bbox', useCats = 1, restated in plain numpy and Python loops, one (image, category,
area range) at a time, as the reference drives it (datasets/coco_eval.py: CocoEvaluator.update / accumulate / summarize).  It shares
no code with spe_amd/ and is what the COCO meter's tests hold the meter to.  pycocotools itself is not available where this project
is developed, so parity with it is unpinned; this file follows its evaluateImg / accumulate / summarize
statement by statement.

An image is a dict of numpy arrays: 'boxes' [n,4] fp32 xyxy, 'scores' [n] fp32, 'labels' [n] category ids (detections);
'gt_boxes' [g,4] fp64 xywh, 'gt_labels' [g], 'iscrowd' [g], 'area' [g] fp64 (the annotation's own field), 'image_id'."""
import numpy as np


def params():
    return {"iouThrs": np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True),
            "recThrs": np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True),
            "maxDets": [1, 10, 100],
            "areaRng": [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]}


def to_xywh(boxes):
    """convert_to_xywh on the fp32 tensor, then .tolist(): the widths are fp32 differences, widened afterwards."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    return np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1).astype(np.float64)


def iou(d, g, crowd):
    """maskApi bbIou of one detection and one ground-truth box, both xywh doubles."""
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = d[2] * d[3] if crowd else d[2] * d[3] + g[2] * g[3] - i
    return i / u


def evaluate_img(im, cat_id, a_rng, max_det, iou_thrs):
    """COCOeval.evaluateImg -> None, or {'dt': indices into the image's detections (score order, truncated), 'dtScores',
    'dtMatches' [T,D] bool, 'dtIgnore' [T,D] bool, 'gtIgnore' [G] bool (visiting order)}."""
    gidx = [j for j in range(len(im["gt_labels"])) if int(im["gt_labels"][j]) == cat_id]
    didx = [i for i in range(len(im["labels"])) if int(im["labels"][i]) == cat_id]
    if len(gidx) == 0 and len(didx) == 0:
        return None
    g_ig = [bool(im["iscrowd"][j]) or float(im["area"][j]) < a_rng[0] or float(im["area"][j]) > a_rng[1] for j in gidx]
    gorder = np.argsort(np.array(g_ig, dtype=np.int64), kind="mergesort") if gidx else []
    gidx = [gidx[o] for o in gorder]
    g_ig = [g_ig[o] for o in gorder]
    dorder = np.argsort(-np.asarray(im["scores"], np.float32)[didx].astype(np.float64), kind="mergesort") if didx else []
    didx = [didx[o] for o in dorder[:max_det]]
    dbox = to_xywh(im["boxes"])
    gbox = np.asarray(im["gt_boxes"], np.float64).reshape(-1, 4)
    crowd = [bool(im["iscrowd"][j]) for j in gidx]
    ious = [[iou(dbox[i], gbox[j], c) for j, c in zip(gidx, crowd)] for i in didx]
    T, D, G = len(iou_thrs), len(didx), len(gidx)
    gtm = np.zeros((T, G), bool)
    dtm = np.zeros((T, D), bool)
    dt_ig = np.zeros((T, D), bool)
    for tind, t in enumerate(iou_thrs):
        for dind in range(D):
            best = min(t, 1 - 1e-10)
            m = -1
            for gind in range(G):
                if gtm[tind, gind] and not crowd[gind]:
                    continue
                if m > -1 and not g_ig[m] and g_ig[gind]:
                    break
                if ious[dind][gind] < best:
                    continue
                best = ious[dind][gind]
                m = gind
            if m == -1:
                continue
            dt_ig[tind, dind] = g_ig[m]
            dtm[tind, dind] = True
            gtm[tind, m] = True
    d_area = np.array([dbox[i][2] * dbox[i][3] for i in didx], np.float64)
    out = np.array([ar < a_rng[0] or ar > a_rng[1] for ar in d_area], bool).reshape(1, D)
    dt_ig = np.logical_or(dt_ig, np.logical_and(~dtm, np.repeat(out, T, 0)))
    return {"dt": didx, "dtScores": np.asarray(im["scores"], np.float32)[didx].astype(np.float64), "dtMatches": dtm, "dtIgnore": dt_ig,
            "gtIgnore": np.array(g_ig, bool)}


def words_of(dtm, dt_ig):
    """[T,D] bool x 2 -> the flag word per detection: matched bits in the low T bits, ignore bits in the next T."""
    T = dtm.shape[0]
    w = np.zeros(dtm.shape[1], np.int64)
    for t in range(T):
        w |= dtm[t].astype(np.int64) << t
        w |= dt_ig[t].astype(np.int64) << (T + t)
    return w.astype(np.int32)


def match_image(im, cat_ids, P=None):
    """What the match step leaves per detection of one image, in the image's incoming order: rank [n] (position inside its (image,
    category) by descending score, -1 when not evaluated), words [n, A]; and the image's npig [K, A]."""
    P = P or params()
    n, K, A = len(im["labels"]), len(cat_ids), len(P["areaRng"])
    rank, words, npig = np.full(n, -1, np.int32), np.zeros((n, A), np.int32), np.zeros((K, A), np.int32)
    for k, cid in enumerate(cat_ids):
        for a, rng in enumerate(P["areaRng"]):
            e = evaluate_img(im, cid, rng, P["maxDets"][-1], P["iouThrs"])
            if e is None:
                continue
            npig[k, a] = int(np.count_nonzero(~e["gtIgnore"]))
            if e["dt"]:
                rank[e["dt"]] = np.arange(len(e["dt"]))
                words[e["dt"], a] = words_of(e["dtMatches"], e["dtIgnore"])
    return rank, words, npig


def accumulate(evals, n_images, K, P):
    """COCOeval.accumulate.  evals[(k, a, i)]: evaluate_img of image i (the i-th in ascending image id) -> precision [T,R,K,A,M],
    recall [T,K,A,M], scores [T,R,K,A,M]."""
    T, R, A, M = len(P["iouThrs"]), len(P["recThrs"]), len(P["areaRng"]), len(P["maxDets"])
    precision, recall, scores = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))
    for k in range(K):
        for a in range(A):
            for m, max_det in enumerate(P["maxDets"]):
                E = [evals.get((k, a, i)) for i in range(n_images)]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                dt_scores = np.concatenate([e["dtScores"][0:max_det] for e in E])
                inds = np.argsort(-dt_scores, kind="mergesort")
                dt_sorted = dt_scores[inds]
                dtm = np.concatenate([e["dtMatches"][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dtIgnore"][:, 0:max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp, fp = np.array(tp), np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q, ss = np.zeros((R,)), np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr, q = pr.tolist(), q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds_r = np.searchsorted(rc, P["recThrs"], side="left")
                    try:
                        for ri, pi in enumerate(inds_r):
                            q[ri] = pr[pi]
                            ss[ri] = dt_sorted[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
                    scores[t, :, k, a, m] = np.array(ss)
    return precision, recall, scores


def summarize(precision, recall, P):
    """COCOeval.summarize for 'bbox' -> stats [12]."""
    def one(ap, iou_thr=None, area=0, max_dets=100):
        m = P["maxDets"].index(max_dets)
        s = precision[:, :, :, area, m] if ap else recall[:, :, area, m]
        if iou_thr is not None:
            s = s[np.where(iou_thr == P["iouThrs"])[0]]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
    last = P["maxDets"][2]
    return np.array([one(1, max_dets=last), one(1, .5, max_dets=last), one(1, .75, max_dets=last), one(1, area=1, max_dets=last),
                     one(1, area=2, max_dets=last), one(1, area=3, max_dets=last), one(0, max_dets=P["maxDets"][0]),
                     one(0, max_dets=P["maxDets"][1]), one(0, max_dets=last), one(0, area=1, max_dets=last),
                     one(0, area=2, max_dets=last), one(0, area=3, max_dets=last)], np.float64)


def evaluate(images, cat_ids, P=None):
    """The whole evaluation -> {'precision', 'recall', 'scores', 'stats', 'npig' [K,A], 'records'}.  records: what the evaluated
    detections carry, per category in curve order (score descending, image id ascending, rank) - 'cat' (index), 'img', 'rank',
    'score' (fp32), 'words' [n,A]."""
    P = P or params()
    cat_ids = sorted(int(c) for c in cat_ids)
    K, A = len(cat_ids), len(P["areaRng"])
    images = sorted(images, key=lambda im: int(im["image_id"]))
    ids = [int(im["image_id"]) for im in images]
    assert len(set(ids)) == len(ids)
    evals, npig = {}, np.zeros((K, A), np.int32)
    rec = {k: [] for k in ("cat", "img", "rank", "score", "words")}
    for i, im in enumerate(images):
        for k, cid in enumerate(cat_ids):
            per_a = []
            for a, rng in enumerate(P["areaRng"]):
                e = evaluate_img(im, cid, rng, P["maxDets"][-1], P["iouThrs"])
                if e is None:
                    continue
                evals[(k, a, i)] = e
                npig[k, a] += int(np.count_nonzero(~e["gtIgnore"]))
                per_a.append(e)
            if per_a and per_a[0]["dt"]:
                D = len(per_a[0]["dt"])
                rec["cat"].append(np.full(D, k, np.int64)); rec["img"].append(np.full(D, ids[i], np.int64))
                rec["rank"].append(np.arange(D, dtype=np.int32))
                rec["score"].append(np.asarray(im["scores"], np.float32)[per_a[0]["dt"]])
                rec["words"].append(np.stack([words_of(e["dtMatches"], e["dtIgnore"]) for e in per_a], 1))
    empty = {"cat": np.zeros(0, np.int64), "img": np.zeros(0, np.int64), "rank": np.zeros(0, np.int32), "score": np.zeros(0, np.float32),
             "words": np.zeros((0, A), np.int32)}
    rec = {k: (np.concatenate(v) if v else empty[k]) for k, v in rec.items()}
    o = np.lexsort((rec["rank"], rec["img"], -rec["score"].astype(np.float64), rec["cat"]))
    rec = {k: v[o] for k, v in rec.items()}
    precision, recall, scores = accumulate(evals, len(images), K, P)
    return {"precision": precision, "recall": recall, "scores": scores, "stats": summarize(precision, recall, P), "npig": npig,
            "records": rec}
