"""Measured cost of the COCO meter (spe_amd.evalmetrics.COCODetectionMeter) on the GPU -> profiles/coco_meter.txt.

    python tools/coco_meter_cost.py [out.txt] [--step-ms MS]

Three times, each a host clock around work that ends in a device synchronise (median, 10th .. 90th percentile):
  update()      for a batch of 2 images x 300 detections (PostProcess' top 300, through per_class_nms), 80 categories, next to the
                per_class_nms call that precedes it in the evaluation loop, alternating on the same inputs; with --step-ms (the step
                time bench.py reports) also as a share of the step;
  summarize()   at COCO val2017 size: 5000 images, 80 categories, up to 100 detections per image, synthetic
                (tests/coco_eval_cases.synthetic_run);
  the numpy restatement (tests/coco_eval_ref.evaluate) on the host for the same 5000 images, once - what a per-image Python evaluator
                costs (pycocotools does the matching in C and is faster than that; it is not installed here).
The meter's tables are compared with the restatement's, exactly, before anything is written.  --device cpu is a dry run of the script."""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def quantiles(ms):
    ms = sorted(ms)
    q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]
    return "%.3f ms (p10 %.3f, p90 %.3f, n = %d)" % (statistics.median(ms), q(0.1), q(0.9), len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "coco_meter.txt"))
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--dets", type=int, default=100, help="NMS survivors per image of the dataset-size run")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--step-ms", type=float, default=None, help="step time of bench.py, to state update() as a share of it")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    import numpy as np
    import torch
    import coco_eval_cases as cases
    import coco_eval_ref as R
    from spe_amd.evalmetrics import COCODetectionMeter
    dev = torch.device(a.device)
    if dev.type == "cuda" and not torch.cuda.is_available():
        raise SystemExit("coco_meter_cost: needs the GPU (a CPU timing says nothing about it)")
    sync = torch.cuda.synchronize if dev.type == "cuda" else (lambda: None)
    cats = list(range(1, 81))

    # ---- update(): 2 x 300 detections over a handful of categories per image
    rng = np.random.default_rng(7)
    batch = [cases.random_image(rng, i, cats, np.bincount(rng.integers(0, 80, 7), minlength=80),
                                np.bincount(rng.integers(0, 6, 300), minlength=80)) for i in range(2)]
    raw, gts = cases.split(batch, dev)
    t_nms, t_upd, kept = [], [], 0
    for it in range(a.warmup + a.steps):
        sync()
        t0 = time.perf_counter()
        if dev.type == "cuda":
            from spe_amd import infer
            res = infer.per_class_nms(raw, 0.5)
        else:
            res = raw
        sync()
        t1 = time.perf_counter()
        if it == 0:
            m = COCODetectionMeter(cats)
        for i, g in enumerate(gts):
            g["image_id"] = 2 * it + i
        t2 = time.perf_counter()
        m.update(res, gts)
        sync()
        t3 = time.perf_counter()
        if it >= a.warmup:
            t_nms.append((t1 - t0) * 1e3); t_upd.append((t3 - t2) * 1e3)
        kept = sum(r["scores"].numel() for r in res)

    # ---- summarize() at dataset size, and the numpy restatement on the same images
    images = cases.synthetic_run(11, a.images, cats, dets_per_image=a.dets)
    m = COCODetectionMeter(cats)
    sync()
    t0 = time.perf_counter()
    for i in range(0, len(images), 2):
        m.update(*cases.split(images[i:i + 2], dev))
    sync()
    t_feed = (time.perf_counter() - t0) * 1e3
    t_sum = []
    for it in range(3 + 20):
        sync()
        t0 = time.perf_counter()
        out = m.summarize()
        sync()
        if it >= 3:
            t_sum.append((time.perf_counter() - t0) * 1e3)
    print("meter done; the restatement on the host takes a while", flush=True)
    t0 = time.perf_counter()
    ref = R.evaluate(images, cats)
    t_ref = (time.perf_counter() - t0) * 1e3
    nd = sum(im["scores"].size for im in images)
    for k in ("precision", "recall", "scores"):
        assert np.array_equal(out["eval"][k], ref[k]), k
    assert np.array_equal(out["stats"], ref["stats"]) and np.array_equal(out["npig"], ref["npig"])

    med = statistics.median(t_upd)
    share = f"; {100 * med / a.step_ms:.2f} % of the {a.step_ms:.1f} ms step bench.py reports" if a.step_ms else ""
    where = "on the MI355X" if dev.type == "cuda" else "DRY RUN ON THE CPU PATH (says nothing about the device)"
    lines = [
        f"COCO meter cost {where} (tools/coco_meter_cost.py; host clock around work ending in a device synchronise)", "",
        f"update(), batch of 2 x 300 detections ({kept} NMS survivors), 80 categories:   {quantiles(t_upd)}{share}",
        f"per_class_nms on the same batch (the call before it):                  {quantiles(t_nms)}",
        f"summarize(), {len(images)} images, 80 categories, {nd} detections:            {quantiles(t_sum)}",
        f"    (feeding them: {len(images) // 2} update() calls of 2 images, {t_feed:.0f} ms in all, inputs uploaded from the host included)",
        f"numpy restatement on the host, same images (tests/coco_eval_ref.evaluate), once:     {t_ref:.0f} ms",
        "    stats " + " ".join("%.4f" % s for s in out["stats"]),
        "    precision, recall, scores, npig and the twelve stats equal to the restatement exactly (np.array_equal)", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
