"""Measured cost of the classification-AP meter (spe_amd.evalmetrics.ClassificationAPMeter) on the GPU -> profiles/cls_ap_meter.txt.

    python tools/cls_ap_cost.py [out.txt]

At two evaluation sizes - (N 4952, C 20): VOC07 test, and (N 5000, C 90): COCO val - with synthetic logits and ~7 % positives:
  add()         per batch of 2 images, a host clock around the call ending in a device synchronise (median, 10th .. 90th percentile),
                and the host time of the call alone (what the evaluation loop waits for: add() never synchronises);
  summarize()   the same clock around the one call and one copy, and the two kernels of spe_cls_ap by device events;
  the CPU path  of this package on the same samples: a device -> host copy of the [N, C] logits and labels, then the meter on CPU
                tensors (a stable sort and a sequential sum per class in numpy).  It stands in for the reference's meter, which needs a
                host copy per batch and walks every class in a Python loop; the reference itself is not timed here.
The device result is compared with the CPU path's, bit for bit, before anything is written.  No threshold: this records costs."""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def quantiles(ms):
    ms = sorted(ms)
    q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]
    return "%.3f ms (p10 %.3f, p90 %.3f, n = %d)" % (statistics.median(ms), q(0.1), q(0.9), len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "cls_ap_meter.txt"))
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    from spe_amd import kernels as K
    from spe_amd.evalmetrics import ClassificationAPMeter
    if not torch.cuda.is_available():
        raise SystemExit("cls_ap_cost: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    lines = ["Classification-AP meter cost on the MI355X (tools/cls_ap_cost.py; host clock around work ending in a device synchronise "
             "unless stated)", ""]
    for N, C in ((4952, 20), (5000, 90)):
        g = torch.Generator().manual_seed(N + C)
        logits = torch.randn(N, C, generator=g).to(dev)
        labels = (torch.rand(N, C, generator=g) < 0.07).float().to(dev)
        m = ClassificationAPMeter()
        t_add, t_host = [], []
        for i in range(0, N, a.batch):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.add(logits[i:i + a.batch], labels[i:i + a.batch])
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if i >= 20 * a.batch:
                t_add.append((t2 - t0) * 1e3); t_host.append((t1 - t0) * 1e3)
        t_sum, t_dev = [], []
        for it in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = m.summarize()
            t1 = time.perf_counter()
            e0.record()
            K.cls_ap(m._scores, m._targets, m._n, m.difficult_examples)
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                t_sum.append((t1 - t0) * 1e3); t_dev.append(e0.elapsed_time(e1))
        t_cpu = []
        for it in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = ClassificationAPMeter()
            h.add(logits.cpu(), labels.cpu())
            ref = h.summarize()
            t_cpu.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(out["ap"].numpy().view(np.int64), ref["ap"].numpy().view(np.int64)) and out["map"] == ref["map"]
        assert torch.equal(out["npos"], ref["npos"]) and torch.equal(out["ncounted"], ref["ncounted"])
        lines += [
            f"N = {N} samples, C = {C} classes, {int(out['npos'].sum())} positives, added in batches of {a.batch}:",
            f"  add(), call to device idle:                      {quantiles(t_add)}",
            f"  add(), host time of the call alone:              {quantiles(t_host)}",
            f"  summarize(), one call + one copy to the host:    {quantiles(t_sum)}",
            f"  spe_cls_ap alone (both kernels, device events):  {quantiles(t_dev)}",
            f"  CPU path: one copy of logits + labels to the host, add, summarize (numpy sort + loop per class): {quantiles(t_cpu)}",
            f"  mAP {out['map']:.6f}: AP per class equal to the CPU path bitwise", ""]
    lines += ["Not measured: the reference's own AveragePrecisionMeter (it is not importable where the GPU is; it copies every batch to the host",
              "and walks each class in a Python loop, slower than the numpy path above); sizes beyond N = 5000 - the ranking kernel does",
              "N comparisons per (class, sample), so its time grows with N^2 per class.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
