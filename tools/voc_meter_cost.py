"""Measured cost of the VOC meter (spe_amd.evalmetrics.VOCDetectionMeter) on the GPU -> profiles/voc_meter.txt.

    python tools/voc_meter_cost.py [out.txt]

Three times, each a host clock around work that ends in a device synchronise (median, 10th .. 90th percentile):
  update()      for a batch of 2 images x 300 detections (PostProcess' top 300, through per_class_nms), next to the per_class_nms
                call that precedes it in the evaluation loop, alternating on the same inputs;
  summarize()   at VOC07-test size: 4952 images, 20 classes, synthetic detections (tests/voc_eval_cases.synthetic_run);
  the numpy restatement (tests/voc_eval_ref.evaluate) on the host for the same 4952 images, once - what a per-image Python evaluator
                costs; the reference's own file round trip is slower still and is not timed.
The meter's APs are compared with the restatement's before anything is written."""
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
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "voc_meter.txt"))
    ap.add_argument("--images", type=int, default=4952)
    ap.add_argument("--dets", type=int, default=100, help="NMS survivors per image of the dataset-size run")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch
    import voc_eval_cases as cases
    import voc_eval_ref as R
    from spe_amd import infer
    from spe_amd.evalmetrics import VOCDetectionMeter
    if not torch.cuda.is_available():
        raise SystemExit("voc_meter_cost: needs the GPU (a CPU timing says nothing about it)")
    dev, C = torch.device("cuda:0"), 20

    # ---- update(): 2 x 300 detections
    rng = np.random.default_rng(7)
    batch = [cases.make_image(rng, i, np.bincount(rng.integers(0, C, 3), minlength=C), np.bincount(rng.integers(0, 4, 300), minlength=C),
                              label_noise=False) for i in range(2)]
    raw, gts = cases.split(batch, dev)
    t_nms, t_upd, kept = [], [], 0
    for it in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = infer.per_class_nms(raw, 0.5)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if it == 0:
            m = VOCDetectionMeter(C)
        for i, g in enumerate(gts):
            g["image_id"] = 2 * it + i
        t2 = time.perf_counter()
        m.update(res, gts)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if it >= a.warmup:
            t_nms.append((t1 - t0) * 1e3); t_upd.append((t3 - t2) * 1e3)
        kept = sum(r["scores"].numel() for r in res)

    # ---- summarize() at dataset size, and the numpy restatement on the same images
    images = cases.synthetic_run(11, a.images, C, dets_per_image=a.dets)
    m = VOCDetectionMeter(C)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(0, len(images), 2):
        m.update(*cases.split(images[i:i + 2], dev))
    torch.cuda.synchronize()
    t_feed = (time.perf_counter() - t0) * 1e3
    t_sum = []
    for it in range(3 + 20):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.summarize()
        torch.cuda.synchronize()
        if it >= 3:
            t_sum.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    ref = R.evaluate(images, C)
    t_ref = (time.perf_counter() - t0) * 1e3
    nd = sum(im["scores"].size for im in images)
    assert np.array_equal(out["ap07"].numpy(), ref["ap07"]) and np.array_equal(out["corloc"].numpy(), ref["corloc"], equal_nan=True)
    assert np.nanmax(np.abs(out["ap_area"].numpy() - ref["ap_area"])) <= nd * 2.0 ** -52

    lines = [
        "VOC meter cost on the MI355X (tools/voc_meter_cost.py; host clock around work ending in a device synchronise)", "",
        f"update(), batch of 2 x 300 detections ({kept} NMS survivors), {C} classes:   {quantiles(t_upd)}",
        f"per_class_nms on the same batch (the call before it):                {quantiles(t_nms)}",
        f"summarize(), {len(images)} images, {C} classes, {nd} detections:          {quantiles(t_sum)}",
        f"    (feeding them: {len(images) // 2} update() calls of 2 images, {t_feed:.0f} ms in all, inputs uploaded from the host included)",
        f"numpy restatement on the host, same images (tests/voc_eval_ref.evaluate), once:   {t_ref:.0f} ms",
        f"    mAP07 {out['map']:.6f} / mean CorLoc {out['mean_corloc']:.6f}: AP07 and CorLoc equal to the restatement bitwise, area AP within nd * 2^-52", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
