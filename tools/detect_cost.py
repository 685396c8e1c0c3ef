"""Measured cost of the detection head (spe_amd.infer.detect: one HIP launch, csrc/detect.hip) next to the composition it stands for
(PostProcess -> spe_amd.infer.per_class_nms) on the GPU -> profiles/detect_fused.txt.

    python tools/detect_cost.py [out.txt] [--bench bench_line.json]

Per shape, B = 2: `infer.detect(outputs, sizes, k).padded()` (what the evaluation loops hand to a meter) against
`per_class_nms(PostProcess()(outputs, sizes, k))`, alternating on the same inputs in one process; a host clock around work that ends in
a device synchronise, median and 10th .. 90th percentile (tools/voc_meter_cost.py's method).  Shapes (Q, Kc, k): (300, 21, 300) the VOC
loop, (300, 91, 100) the COCO loop, (600, 21, 300) the VOC loop with the flip augmentation.  Besides, for one call of either: the
device kernels and copies of a torch.profiler trace, and the synchronising torch calls torch.cuda.set_sync_debug_mode('warn')
reports.  The two results are compared before anything is written.  --bench: a bench.py result line to quote."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = (("VOC loop", 300, 21, 300), ("COCO loop", 300, 91, 100), ("VOC loop, flip", 600, 21, 300))


def quantiles(ms):
    ms = sorted(ms)
    q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]
    return "%.3f ms (p10 %.3f, p90 %.3f, n = %d)" % (statistics.median(ms), q(0.1), q(0.9), len(ms))


def trace(fn):
    """-> (device kernels, device copies, synchronising torch calls) of one call; None where a count could not be taken."""
    import torch
    kernels = copies = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
        copies = sum(1 for e in dev if "memcpy" in e.name.lower())
        kernels = sum(1 for e in dev if "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    except Exception as e:                                    # a profiler that does not start must not cost the timings
        print("detect_cost: no profiler trace (%s)" % e, file=sys.stderr)
    torch.cuda.set_sync_debug_mode("warn")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        fn()
    torch.cuda.set_sync_debug_mode("default")
    return kernels, copies, sum(1 for x in w if "synchroniz" in str(x.message).lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "detect_fused.txt"))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--bench", default=None)
    a = ap.parse_args()
    import torch
    from spe_amd import infer
    from spe_amd.models.conditional_detr import PostProcess
    if not torch.cuda.is_available():
        raise SystemExit("detect_cost: needs the GPU (a CPU timing says nothing about it)")
    dev, B, pp = torch.device("cuda:0"), 2, PostProcess()
    lines = ["Detection head cost on the MI355X (tools/detect_cost.py; host clock around work ending in a device synchronise; B = 2;",
             "fused = infer.detect(...).padded(): spe_detect + one sigmoid; composed = per_class_nms(PostProcess(...)); alternating, same inputs)", ""]
    verdicts = []
    for name, Q, Kc, k in SHAPES:
        g = torch.Generator().manual_seed(Q * Kc + k)
        N = Q * Kc
        logits = torch.stack([torch.linspace(-12, 3, N)[torch.randperm(N, generator=g)] for _ in range(B)]).reshape(B, Q, Kc)
        centres = torch.rand(B, 6, 2, generator=g) * 0.6 + 0.2
        pick = torch.randint(0, 6, (B, Q), generator=g)
        boxes = torch.cat([torch.gather(centres, 1, pick[..., None].expand(-1, -1, 2)) + 0.02 * torch.randn(B, Q, 2, generator=g),
                           0.25 * (1 + 0.08 * torch.randn(B, Q, 2, generator=g))], -1)
        outputs = {"pred_logits": logits.to(dev), "pred_boxes": boxes.to(dev)}
        sizes = torch.tensor([[480., 640.], [375., 500.]], device=dev)
        fused = lambda: infer.detect(outputs, sizes, k, 0.5).padded()
        composed = lambda: infer.per_class_nms(pp(outputs, sizes, k), 0.5)
        got, want = infer.detect(outputs, sizes, k, 0.5).results(), composed()
        for x, y in zip(got, want):
            assert all(torch.equal(x[key], y[key]) for key in ("scores", "labels", "boxes")), "the two paths disagree"
        t_f, t_c = [], []
        for it in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fused()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            composed()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if it >= a.warmup:
                t_f.append((t1 - t0) * 1e3); t_c.append((t2 - t1) * 1e3)
        kf, cf, sf = trace(fused)
        kc, cc, sc = trace(composed)
        show = lambda v: "n/a" if v is None else str(v)
        mf, mc = statistics.median(t_f), statistics.median(t_c)
        verdicts.append(mf <= mc)
        lines += [f"{name}: Q = {Q}, Kc = {Kc}, k = {k} ({sum(r['scores'].numel() for r in want)} NMS survivors)",
                  f"    fused      {quantiles(t_f)}   device kernels {show(kf)}, device copies {show(cf)}, synchronising torch calls {show(sf)}",
                  f"    composed   {quantiles(t_c)}   device kernels {show(kc)}, device copies {show(cc)}, synchronising torch calls {show(sc)}",
                  f"    fused / composed (medians): {mf / mc:.3f}", ""]
    lines += ["The fused median is not above the composed median at every shape." if all(verdicts) else
              "THE FUSED MEDIAN IS ABOVE THE COMPOSED MEDIAN at: " + ", ".join(s[0] for s, v in zip(SHAPES, verdicts) if not v) + ".", ""]
    if a.bench and os.path.exists(a.bench):
        for ln in open(a.bench):
            if ln.startswith("{"):
                r = json.loads(ln)
                keep = {k: v for k, v in r.items() if not isinstance(v, (dict, list)) and not (isinstance(v, str) and len(v) > 80)}
                lines += ["bench.py --gpus 1 --steps 20 --warmup 5 after the change (the training hot path is untouched; the parent was not run beside it):",
                          "    " + json.dumps(keep), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
