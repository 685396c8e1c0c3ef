"""Golden vectors of the REFERENCE's PASCAL VOC evaluator (datasets/voc_eval.py: voc_eval / voc_ap, datasets/dis_eval.py: dis_eval),
written by running the reference's own functions in the build container (imported by path from the reference checkout,
tools/ref_harness.REF, with `np.bool = bool` set first - the alias voc_eval.py:128 needs left numpy in 1.24):

    python tools/gen_voc_eval_golden.py

Synthetic XML annotations, an image-set file and per-class result files in the format of `_write_voc_results_file`
(datasets/voc_voc.py:366-386: image name, score to 3 decimals, the four coordinates + 1 to 1 decimal, from the fp32 rows) go to a temporary directory;
CorLoc is evaluated like engine_loc.py:187-194 does, from files that hold the top-scoring box per (class, image) only.

-> tests/golden/voc_eval_small.pt, tests/golden/voc_eval_edges.pt (data only): the fp32 detections, the ground truth with difficult flags
and image ids, and per class the reference's rec, prec, both APs and CorLoc.

Before anything is recorded the generator asserts that the reference is unambiguous on these inputs (np.argsort(-confidence) is an
unstable sort and np.argmax needs distinct maxima to be a rule): inside a class all file scores are distinct, and no positive overlap
lies within 1e-9 of the threshold or of another ground truth's overlap unless the two ground-truth boxes are identical.  It also asserts
that tests/voc_eval_ref.py reproduces the recorded rec and prec bitwise.  Deterministic: the files regenerate bit for bit."""
import importlib.util
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voc_eval_ref as R  # noqa: E402
from tools.ref_harness import REF  # noqa: E402

OVTHRESH = 0.5


def load_reference():
    if not hasattr(np, "bool"):
        np.bool = bool                                       # voc_eval.py:128
    mods = []
    for name in ("voc_eval", "dis_eval"):
        spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(REF, "datasets", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        mods.append(m)
    return mods


def _sorted_like_nms(im):
    """(label ascending, score descending) - the order per_class_nms returns."""
    o = np.argsort(-im["scores"].astype(np.float64), kind="stable")
    o = o[np.argsort(im["labels"][o], kind="stable")]
    for k in ("boxes", "scores", "labels"):
        im[k] = im[k][o]
    return im


def small_case():
    rng = np.random.default_rng(20250)
    C, images = 4, []
    ticket = [list(rng.permutation(np.arange(1, 1000))) for _ in range(C)]      # distinct file scores per class
    for i in range(40):
        g = int(rng.integers(0, 4))
        x0, y0 = rng.integers(1, 300, g), rng.integers(1, 200, g)
        gb = np.stack([x0, y0, x0 + rng.integers(20, 150, g), y0 + rng.integers(20, 120, g)], 1).reshape(-1, 4).astype(np.int64)
        gl = rng.integers(1, C + 1, g)
        gl[gl == 3] = 4 if i % 2 else 2                      # class 3: no ground truth at all
        gd = rng.random(g) < 0.2
        gd[gl == 2] = True                                   # class 2: only difficult ground truth
        boxes, labels = [], []
        for k in range(g):
            for _ in range(int(rng.integers(0, 3))):
                boxes.append(gb[k] - 1.0 + rng.normal(0, 6, 4)); labels.append(gl[k] if rng.random() < 0.85 else rng.integers(1, C + 1))
        for _ in range(int(rng.integers(0, 4))):
            p = rng.uniform(0, 300, 2)
            boxes.append(np.concatenate([p, p + rng.uniform(15, 140, 2)])); labels.append(rng.integers(1, C + 1))
        labels = np.array(labels, np.int64).reshape(-1)
        scores = np.array([(ticket[l - 1].pop() + rng.uniform(-0.3, 0.3)) / 1000. for l in labels], np.float32)
        images.append(_sorted_like_nms({"boxes": np.array(boxes, np.float32).reshape(-1, 4), "scores": scores, "labels": labels,
                                        "gt_boxes": gb, "gt_labels": gl.astype(np.int64), "difficult": gd, "image_id": 1000 + 3 * i}))
    return C, images


def edges_case():
    """class 1: ground truth, no detections; 2: neither; 3: only difficult ground truth; 4: two identical ground-truth boxes hit by two
    detections (the second is a false positive); 5: a duplicate detection on a matched box; 6: a detection on a difficult box followed
    by another on it."""
    f = lambda *rows: np.array(rows, np.float32).reshape(-1, 4)
    imgs = [
        {"image_id": 1, "gt_boxes": [[10, 10, 50, 50], [100, 100, 160, 160]], "gt_labels": [1, 3], "difficult": [0, 1],
         "boxes": f([99, 99, 159, 159], [300, 300, 340, 340]), "scores": [0.9, 0.8], "labels": [3, 3]},
        {"image_id": 2, "gt_boxes": [[20, 20, 80, 80], [20, 20, 80, 80]], "gt_labels": [4, 4], "difficult": [0, 0],
         "boxes": f([30, 40, 90, 100], [19, 19, 79, 79], [20, 20, 79, 80]), "scores": [0.85, 0.95, 0.7], "labels": [3, 4, 4]},
        {"image_id": 3, "gt_boxes": [[50, 60, 150, 200], [200, 50, 260, 120], [300, 300, 380, 390]], "gt_labels": [5, 6, 6],
         "difficult": [0, 1, 0],
         "boxes": f([49, 59, 149, 199], [49, 59, 149, 199], [199, 49, 259, 119], [201, 51, 259, 119], [298, 301, 377, 392]),
         "scores": [0.9, 0.6, 0.88, 0.5, 0.4], "labels": [5, 5, 6, 6, 6]},
        {"image_id": 4, "gt_boxes": [[10, 10, 100, 100]], "gt_labels": [5], "difficult": [0],
         "boxes": f([14, 12, 104, 99], [200, 200, 250, 260]), "scores": [0.75, 0.65], "labels": [5, 6]},
    ]
    for im in imgs:
        im["gt_boxes"] = np.array(im["gt_boxes"], np.int64).reshape(-1, 4)
        im["gt_labels"], im["difficult"] = np.array(im["gt_labels"], np.int64), np.array(im["difficult"], bool)
        im["scores"], im["labels"] = np.array(im["scores"], np.float32), np.array(im["labels"], np.int64)
        _sorted_like_nms(im)
    return 6, imgs


def assert_unambiguous(C, images):
    file_scores = [[] for _ in range(C)]
    for im in images:
        qs, bx = R.quantise(im["scores"], im["boxes"], True)
        for j, l in enumerate(im["labels"]):
            file_scores[l - 1].append("%.3f" % im["scores"][j])
            assert float("%.3f" % im["scores"][j]) == qs[j], "rint / 1000 is not what '{:.3f}' prints"
            g = np.nonzero(im["gt_labels"] == l)[0]
            if not g.size:
                continue
            ov = R.overlaps(bx[j], im["gt_boxes"][g].astype(np.float64))
            assert np.all(np.abs(ov[ov > 0] - OVTHRESH) > 1e-9), "an overlap sits on the threshold"
            for a in range(g.size):
                for b in range(a + 1, g.size):
                    same = np.array_equal(im["gt_boxes"][g[a]], im["gt_boxes"][g[b]])
                    assert same or ov[a] <= 0 or ov[b] <= 0 or abs(ov[a] - ov[b]) > 1e-9, "two ground truths tie"
    for c in range(C):
        assert len(set(file_scores[c])) == len(file_scores[c]) <= 1000, f"class {c + 1}: repeated file score"


def run_reference(C, images, voc_eval, dis_eval, tmp):
    names = ["cls%d" % (c + 1) for c in range(C)]
    images = sorted(images, key=lambda im: im["image_id"])                     # the image-set order: ascending ids
    os.makedirs(os.path.join(tmp, "anno"))
    with open(os.path.join(tmp, "set.txt"), "w") as f:
        f.writelines("%06d\n" % im["image_id"] for im in images)
    for im in images:
        objs = "".join(
            "<object><name>%s</name><pose>Unspecified</pose><truncated>0</truncated><difficult>%d</difficult>"
            "<bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>"
            % ((names[l - 1], int(d)) + tuple(int(v) for v in b)) for b, l, d in zip(im["gt_boxes"], im["gt_labels"], im["difficult"]))
        with open(os.path.join(tmp, "anno", "%06d.xml" % im["image_id"]), "w") as f:
            f.write("<annotation>%s</annotation>" % objs)
    for kind in ("det", "top"):                                                # all survivors / the top-scoring one per (class, image)
        for c in range(C):
            with open(os.path.join(tmp, "%s_%s.txt" % (kind, names[c])), "w") as f:
                for im in images:
                    rows = np.nonzero(im["labels"] == c + 1)[0]
                    if kind == "top" and rows.size:
                        best = rows[0]
                        for j in rows[1:]:
                            if im["scores"][best] < im["scores"][j]:            # engine_loc.py:193: strict, the first wins
                                best = j
                        rows = np.array([best])
                    dets = np.hstack((im["boxes"], im["scores"].reshape(-1, 1)))[rows]       # fp32 rows, as engine_loc.py:186 builds
                    for k in range(dets.shape[0]):
                        f.write("%s %.3f %.1f %.1f %.1f %.1f\n" % (("%06d" % im["image_id"], dets[k, -1]) + tuple(dets[k, :4] + 1)))
    anno, imset = os.path.join(tmp, "anno", "{:s}.xml"), os.path.join(tmp, "set.txt")
    out = {k: [] for k in ("rec", "prec", "ap07", "ap_area", "corloc")}
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in range(C):
            det = [os.path.join(tmp, "det_{:s}.txt")]
            rec, prec, a07 = voc_eval(det, anno, imset, names[c], os.path.join(tmp, "cache"), ovthresh=OVTHRESH, use_07_metric=True)
            rec2, prec2, area = voc_eval(det, anno, imset, names[c], os.path.join(tmp, "cache"), ovthresh=OVTHRESH, use_07_metric=False)
            assert np.array_equal(rec, rec2, equal_nan=True) and np.array_equal(prec, prec2)
            cl = dis_eval([os.path.join(tmp, "top_{:s}.txt")], [anno], [imset], names[c], [os.path.join(tmp, "cache_dis")],
                          ovthresh=OVTHRESH)
            out["rec"].append(torch.from_numpy(np.asarray(rec, np.float64).reshape(-1)))
            out["prec"].append(torch.from_numpy(np.asarray(prec, np.float64).reshape(-1)))
            out["ap07"].append(float(a07)); out["ap_area"].append(float(area)); out["corloc"].append(float(cl))
    return out


def main():
    voc_mod, dis_mod = load_reference()
    for name, (C, images) in (("voc_eval_small", small_case()), ("voc_eval_edges", edges_case())):
        assert_unambiguous(C, images)
        with tempfile.TemporaryDirectory() as tmp:
            ref = run_reference(C, images, voc_mod.voc_eval, dis_mod.dis_eval, tmp)
        ours = R.evaluate(images, C, OVTHRESH, True)
        for c in range(C):                                                      # the restatement must be the reference, bit for bit
            assert np.array_equal(ours["rec"][c], ref["rec"][c].numpy(), equal_nan=True), (name, c)
            assert np.array_equal(ours["prec"][c], ref["prec"][c].numpy()), (name, c)
            assert ours["ap07"][c] == ref["ap07"][c], (name, c)
            assert ours["ap_area"][c] == ref["ap_area"][c] or (np.isnan(ours["ap_area"][c]) and np.isnan(ref["ap_area"][c])), (name, c)
            assert ours["corloc"][c] == ref["corloc"][c] or (np.isnan(ours["corloc"][c]) and np.isnan(ref["corloc"][c])), (name, c)
        t = torch.from_numpy
        rec = {"num_classes": C, "ovthresh": OVTHRESH,
               "images": [{"boxes": t(im["boxes"]), "scores": t(im["scores"]), "labels": t(im["labels"]), "gt_boxes": t(im["gt_boxes"]),
                           "gt_labels": t(im["gt_labels"]), "difficult": t(im["difficult"]), "image_id": int(im["image_id"])} for im in images],
               "rec": ref["rec"], "prec": ref["prec"], "ap07": torch.tensor(ref["ap07"], dtype=torch.float64),
               "ap_area": torch.tensor(ref["ap_area"], dtype=torch.float64), "corloc": torch.tensor(ref["corloc"], dtype=torch.float64)}
        path = os.path.join(ROOT, "tests", "golden", name + ".pt")
        torch.save(rec, path)
        nd = sum(im["scores"].size for im in images)
        print("wrote", path, os.path.getsize(path), "bytes;", len(images), "images,", nd, "detections; ap07", ref["ap07"], "area", ref["ap_area"],
              "corloc", ref["corloc"])


if __name__ == "__main__":
    main()
