"""Measured cost of the stretch between the forward and the criterion of the refine training loops - the stage-0 targets out of the class
maps and the stage k+1 targets out of every stage's detections - on the GPU -> profiles/train_targets.txt.

    python tools/train_targets_cost.py [out.txt] [--bench-before line.json] [--bench-after line.json]

cfg2: B = 2 at 800 x 1333, 6 present maps, Q = 300, Kc = 21, two refinement stages.  Two forms of the stretch, alternating on the same
outputs in one process:

  before   the composition the loop had: get_pseudo_label_multi_boxes on the moved targets (label reads, the packed counts + boxes copy,
           the boxes built on host tensors and sent back), PostProcessRefine on ATen (REFINE_KERNEL = False) without 'labels_unique'
  new      camboxes.pseudo_targets (spe_cam_targets, the counts read), 'labels_unique' from its classes, PostProcessRefine's one launch

A host clock around work that ends in a device synchronise (tools/detect_cost.py's method), three runs of --steps alternations each, the
median of every run.  Besides, for one call of either: the device kernels and copies of a torch.profiler trace (copies by direction), and
the synchronising torch calls torch.cuda.set_sync_debug_mode('warn') reports.  The two target lists are compared before anything is
written."""
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

B, H, W, Q, KC, CLASSES, STAGES, RUNS = 2, 800, 1333, 300, 21, 20, 2, 3
PRESENT = ((1, 6, 14), (0, 7, 11))                       # 6 maps


def trace(fn):
    """-> (device kernels, {copy direction: count}, synchronising torch calls) of one call; None where a count could not be taken."""
    import torch
    kernels = copies = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
        copies = {}
        for e in dev:
            n = e.name.lower()
            if "memcpy" in n:
                d = "device-to-host" if "dtoh" in n else "host-to-device" if "htod" in n else "device-to-device" if "dtod" in n else e.name
                copies[d] = copies.get(d, 0) + 1
        kernels = sum(1 for e in dev if "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    except Exception as e:                                    # a profiler that does not start must not cost the timings
        print("train_targets_cost: no profiler trace (%s)" % e, file=sys.stderr)
    torch.cuda.set_sync_debug_mode("warn")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        fn()
    torch.cuda.set_sync_debug_mode("default")
    return kernels, copies, sum(1 for x in w if "synchroniz" in str(x.message).lower())


def bench_line(path):
    if path and os.path.exists(path):
        for ln in open(path):
            if ln.startswith("{"):
                r = json.loads(ln)
                return json.dumps({k: v for k, v in r.items() if not isinstance(v, (dict, list)) and not (isinstance(v, str) and len(v) > 80)})
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "train_targets.txt"))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--bench-before", action="append", default=[])
    ap.add_argument("--bench-after", action="append", default=[])
    a = ap.parse_args()
    import torch
    import train_targets_cases as C
    from spe_amd import camboxes, engine, infer
    from spe_amd.models import conditional_detr as cd
    from spe_amd.util.misc import NestedTensor
    if not torch.cuda.is_available():
        raise SystemExit("train_targets_cost: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(9)
    outputs = {k: {"pred_logits": (torch.randn(B, Q, KC, generator=g) * 3).to(dev), "pred_boxes": torch.rand(B, Q, 4, generator=g).to(dev)}
               for k in range(STAGES + 1)}
    outputs[0]["cams_cls"] = C.cam_maps(B, CLASSES, 50, 84).to(dev)
    samples = NestedTensor(torch.zeros(B, 3, H, W, device=dev), None)
    host_targets = []
    for b in range(B):
        lab = torch.zeros(CLASSES, dtype=torch.int64)
        lab[list(PRESENT[b])] = 1
        host_targets.append({"img_label": lab, "orig_size": torch.tensor([H, W])})
    args = argparse.Namespace(num_classes=CLASSES, cam_thr=0.2, multi_box_ratio=0.5, num_refines=STAGES)
    post = {"bbox": cd.PostProcessRefine()}

    def before():
        cd.REFINE_KERNEL = False
        targets = [dict(t) for t in moved]
        for t, p in zip(targets, camboxes.get_pseudo_label_multi_boxes(outputs[0], samples, targets, args)):
            t.update(p)
        return targets, engine.get_refinements_pseudo_label(outputs, samples, targets, args, post)

    def new():
        cd.REFINE_KERNEL = True
        present = camboxes.present_lists(host_targets, "img_label")
        targets = [dict(t) for t in moved]
        pseudo = camboxes.pseudo_targets(outputs[0], samples, present, args.num_classes, args.cam_thr, args.multi_box_ratio)
        uniq = infer.ClassTable([[c for c in cl if c < KC] for cl in pseudo.classes], dev).per_image()
        for t, p, u in zip(targets, pseudo.per_image(), uniq):
            t.update(p)
            t["labels_unique"] = u
        return targets, engine.get_refinements_pseudo_label(outputs, samples, targets, args, post)

    moved = [{k: v.to(dev) for k, v in t.items()} for t in host_targets]          # the loop moves the targets before the forward: not timed
    (t0, r0), (t1, r1) = before(), new()
    for x, y in zip(t0, t1):
        assert torch.equal(x["boxes"], y["boxes"]) and torch.equal(x["labels"], y["labels"]), "the stage-0 targets disagree"
    for rf in r0:
        for x, y in zip(r0[rf], r1[rf]):
            assert all(torch.equal(x[k].view(torch.int32) if x[k].dtype == torch.float32 else x[k],
                                   y[k].view(torch.int32) if y[k].dtype == torch.float32 else y[k]) for k in ("scores", "labels", "boxes")), "the stage targets disagree"
    rows = sum(t["boxes"].shape[0] for t in t1)
    med = {"before": [], "new": []}
    for _ in range(RUNS):
        t_b, t_n = [], []
        for it in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            s0 = time.perf_counter()
            before()
            torch.cuda.synchronize()
            s1 = time.perf_counter()
            new()
            torch.cuda.synchronize()
            s2 = time.perf_counter()
            if it >= a.warmup:
                t_b.append((s1 - s0) * 1e3); t_n.append((s2 - s1) * 1e3)
        med["before"].append(statistics.median(t_b)); med["new"].append(statistics.median(t_n))
    show = lambda v: "n/a" if v is None else str(v)
    lines = ["Training targets between the forward and the criterion on the MI355X (tools/train_targets_cost.py; host clock around work ending",
             f"in a device synchronise; cfg2: B = {B} at {H} x {W}, {sum(map(len, PRESENT))} maps -> {rows} stage-0 rows, Q = {Q}, Kc = {KC}, {STAGES} refinement stages;",
             f"before / new alternating on the same outputs, {RUNS} runs of {a.steps} alternations, the median of every run)", ""]
    for name, fn in (("before", before), ("new", new)):
        k, c, s = trace(fn)
        lines.append(f"    {name:<7} medians " + ", ".join("%.3f" % m for m in med[name]) + f" ms   device kernels {show(k)}, copies {show(c)}, synchronising torch calls {show(s)}")
    faster = max(med["new"]) < min(med["before"])
    lines += ["", ("Every run's median of the new path lies below every run's median of the composition before: faster beyond the run-to-run spread."
                   if faster else "THE NEW PATH IS NOT FASTER BEYOND THE RUN-TO-RUN SPREAD of three runs each."), ""]
    for title, paths in (("before (the parent commit)", a.bench_before), ("after", a.bench_after)):
        got = [l for l in (bench_line(p) for p in paths) if l]
        if got:
            lines += [f"bench.py --gpus 1 --steps 20 --warmup 5, {title}:"] + ["    " + l for l in got] + [""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
