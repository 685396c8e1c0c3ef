"""Named shapes of the VOC meter tests (tests/test_voc_meter_cpu.py, tests/test_voc_meter_gpu.py, tools/gen_voc_eval_golden.py,
tools/voc_meter_cost.py) and the seeded builders of their synthetic inputs, plus the helpers both test files share."""
import os

import numpy as np
import torch

GOLDENS = ("voc_eval_small", "voc_eval_edges")

# spe_voc_match: ground truth and detections per (image, class) segment around the wave width (64), with several lane strides (130,
# 300) and the empty / single cases; every pairing appears in MATCH_CASES.  Class c of image i takes entry (i * C + c) of the cycle.
GT_PER_SEG = (0, 1, 63, 64, 65, 130)
DET_PER_SEG = (0, 1, 2, 64, 65, 300)
# name -> (images, classes, offset into the gt cycle, offset into the det cycle)
MATCH_CASES = {
    "one_image": (1, 6, 0, 0),            # gt count = det count position by position
    "two_images_shifted": (2, 6, 0, 1),   # 12 segments: every gt count meets two more det counts
    "three_images": (3, 6, 2, 5),         # 18 segments, three more pairings per gt count
    "one_class": (2, 1, 5, 5),            # C = 1: the first and the last wave of an image are the same wave
}
MAX_DET, MAX_GT = 4096, 1024              # per image: accepted; one more: status -2

# spe_voc_ap: detections per class, 20 classes in one launch (the chunk is 256 wide: 255 / 256 / 257, 1023 / 1025, many chunks)
AP_ND = (0, 1, 255, 256, 257, 1023, 1025, 5000)
AP_STREAMS = ("tp", "fp", "ignored", "random")
AP_CLASSES = 20


def make_image(rng, image_id, gt_counts, det_counts, frame=500, integer_dets=False, label_noise=True):
    """One image with gt_counts[c] ground-truth boxes and det_counts[c] detections of class c + 1, detections ordered like
    per_class_nms output (label ascending, score descending).  Detections are jittered copies of the class's ground truth (or free
    boxes), a tenth of the ground truth is duplicated (identical boxes: equal overlaps), a fifth is difficult, scores repeat now and
    then (equal scores), and with label_noise a few detections carry labels outside 1 .. C."""
    C = len(gt_counts)
    gb, gl, gd, db, ds, dl = [], [], [], [], [], []
    for c in range(C):
        g = gt_counts[c]
        x0, y0 = rng.integers(1, frame - 60, g), rng.integers(1, frame - 60, g)
        b = np.stack([x0, y0, x0 + rng.integers(8, 60, g), y0 + rng.integers(8, 60, g)], 1).astype(np.int64).reshape(-1, 4)
        for k in range(1, g):
            if rng.random() < 0.1:
                b[k] = b[rng.integers(0, k)]
        gb.append(b); gl.append(np.full(g, c + 1)); gd.append(rng.random(g) < 0.2)
        d = det_counts[c]
        if g:
            src = b[rng.integers(0, g, d)].astype(np.float64)
            jit = rng.normal(0, 4, (d, 4)) * (rng.random((d, 1)) < 0.8)         # a fifth lands exactly on its ground truth
            box = src + jit
        else:
            p = rng.uniform(0, frame - 60, (d, 2))
            box = np.concatenate([p, p + rng.uniform(5, 60, (d, 2))], 1)
        box = box - 1.0                                                         # detections live in 0-based pixels
        if integer_dets:
            box = np.rint(box)
        s = np.sort(np.round(rng.random(d), 2 if d > 3 else 6).astype(np.float32))[::-1]     # 2 decimals: repeated scores
        db.append(box.astype(np.float32).reshape(-1, 4)); ds.append(s); dl.append(np.full(d, c + 1))
    if label_noise:                                                             # dropped labels: 0 in front, C + 1 and C + 7 behind
        for lab in (0, C + 1, C + 7):
            p = rng.uniform(0, frame - 60, (2, 2))
            where = 0 if lab == 0 else len(db)
            db.insert(where, np.concatenate([p, p + 20], 1).astype(np.float32)); ds.insert(where, np.array([0.9, 0.3], np.float32))
            dl.insert(where, np.full(2, lab))
    cat = np.concatenate
    return {"boxes": cat(db).reshape(-1, 4), "scores": cat(ds).astype(np.float32), "labels": cat(dl).astype(np.int64),
            "gt_boxes": cat(gb).reshape(-1, 4), "gt_labels": cat(gl).astype(np.int64), "difficult": cat(gd).astype(bool),
            "image_id": image_id}


def match_case(name, seed=0, **kw):
    nimg, C, go, do = MATCH_CASES[name]
    rng = np.random.default_rng([seed, nimg, C, go, do])
    return C, [make_image(rng, 100 + 7 * i, [GT_PER_SEG[(go + i * C + c) % 6] for c in range(C)],
                          [DET_PER_SEG[(do + i * C + c) % 6] for c in range(C)], **kw) for i in range(nimg)]


# (detections, stream, npos) of the 20 classes: every nd, every stream and every npos kind, the long and the chunk-edge segments with
# the streams whose curve moves (random, all tp)
AP_TABLE = ((0, "random", "many"), (1, "tp", "one"), (255, "random", "many"), (256, "tp", "zero"), (257, "random", "one"),
            (1023, "random", "many"), (1025, "fp", "zero"), (5000, "random", "many"), (0, "tp", "zero"), (1, "fp", "one"),
            (255, "ignored", "many"), (256, "random", "many"), (257, "tp", "many"), (1023, "tp", "one"), (1025, "random", "many"),
            (5000, "tp", "many"), (1, "ignored", "zero"), (5000, "random", "zero"), (1025, "ignored", "one"), (5000, "fp", "many"))


def ap_streams(seed=0):
    """-> (flags uint8 [nd total] sorted per class, seg_off int32 [21], npos int32 [20]) of AP_TABLE.  Where npos > 0 the true
    positives stay <= npos (as the matcher guarantees; the area bound of the tests needs partial sums <= 1), except the all-tp stream
    with npos = 1, whose terms are whole numbers and add exactly."""
    rng = np.random.default_rng([seed, 77])
    flags, npos = [], []
    for nd, kind, objects in AP_TABLE:
        f = {"tp": np.ones(nd), "fp": np.full(nd, 2), "ignored": np.zeros(nd), "random": rng.integers(0, 3, nd)}[kind].astype(np.uint8)
        if objects == "one" and kind == "random":
            f[np.nonzero(f == 1)[0][1:]] = 2                                    # one object: at most one true positive
        flags.append(f); npos.append({"zero": 0, "one": 1, "many": int((f == 1).sum()) + 3}[objects])
    seg = np.concatenate(([0], np.cumsum([f.size for f in flags]))).astype(np.int32)
    return np.concatenate(flags), seg, np.array(npos, np.int32)


def synthetic_run(seed, nimg, C, dets_per_image=100, gts_per_image=3):
    """A whole evaluation run at dataset size (tools/voc_meter_cost.py): per image `dets_per_image` detections over a few classes."""
    rng = np.random.default_rng([seed, nimg, C])
    out = []
    for i in range(nimg):
        gc, dc = np.zeros(C, int), np.zeros(C, int)
        for c in rng.integers(0, C, gts_per_image):
            gc[c] += 1
        for c in rng.choice(np.concatenate([np.nonzero(gc)[0], rng.integers(0, C, 2)]), dets_per_image):
            dc[c] += 1
        out.append(make_image(rng, i, gc, dc, label_noise=False))
    return out


# ---- shared by the CPU and the GPU tests -------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    return torch.load(os.path.join(GOLDEN, name + ".pt"), weights_only=False)


def as_numpy(images):
    return [{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in im.items()} for im in images]


def split(images, device="cpu"):
    """image dicts (tensors or arrays) -> (results, gts) as the meter takes them."""
    t = lambda v: torch.as_tensor(v).to(device)
    res = [{"boxes": t(im["boxes"]), "scores": t(im["scores"]), "labels": t(im["labels"])} for im in images]
    gts = [{"boxes": t(im["gt_boxes"]), "labels": t(im["gt_labels"]), "difficult": t(im["difficult"]), "image_id": im["image_id"]}
           for im in images]
    return res, gts


def run_meter(images, C, batches=None, device="cpu", **kw):
    from spe_amd.evalmetrics import VOCDetectionMeter
    m = VOCDetectionMeter(num_classes=C, **kw)
    for b in (batches if batches is not None else [list(range(len(images)))]):
        m.update(*split([images[i] for i in b], device))
    return m


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def check_against(out, want, C):
    """out: summarize(return_curves=True); want: dict with per-class flags (optional), rec, prec, ap07, ap_area, corloc."""
    for c in range(C):
        if "flags" in want:
            assert same(out["flags"][c], want["flags"][c]), c
        assert same(out["rec"][c], want["rec"][c]) and same(out["prec"][c], want["prec"][c]), c
        assert same(out["ap07"][c], want["ap07"][c]), (c, float(out["ap07"][c]), float(want["ap07"][c]))
        a, b, nd = float(out["ap_area"][c]), float(want["ap_area"][c]), len(out["rec"][c])
        assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= nd * 2.0 ** -52, (c, a, b, nd)
        assert same(out["corloc"][c], want["corloc"][c]), c
