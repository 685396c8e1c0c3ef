"""Measured cost of scoring the pseudo labels while training runs (evalmetrics.PseudoLabelMeter, spe_pseudo_quality) on the GPU
-> profiles/pseudo_quality.txt.

    python tools/pseudo_quality_cost.py [out.txt] [--bench-before line.json] [--bench-after line.json]

cfg2: B = 2 at 800 x 1333, 6 present maps, Q = 300, Kc = 21, two refinement stages, 3 ground-truth rows per image.  The target section of
engine._train_one_epoch - from the model's outputs to both target lists - in two forms, alternating on the same outputs in one process:

  plain   camboxes.pseudo_targets, 'labels_unique', PostProcessRefine's picks: what the loop does without a meter
  meter   the same, the loader's rows kept aside before the pseudo labels replace them, then one update per stage: 'cam', 'rf_1', 'rf_2'

A host clock around work that ends in a device synchronise (tools/train_targets_cost.py's method), three runs of --steps alternations
each, the median of every run.  Besides, for one call of either: the launches per entry point of the library, the device kernels and
copies of a torch.profiler trace, and the synchronising torch calls torch.cuda.set_sync_debug_mode('warn') reports.  The meter's
counters are compared with the CPU meter on the same rows before anything is written."""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

B, H, W, Q, KC, CLASSES, STAGES, RUNS, GT_ROWS = 2, 800, 1333, 300, 21, 20, 2, 3, 3
PRESENT = ((1, 6, 14), (0, 7, 11))                       # 6 maps
NAMES = ["cam"] + [f"rf_{k}" for k in range(1, STAGES + 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "pseudo_quality.txt"))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--bench-before", action="append", default=[])
    ap.add_argument("--bench-after", action="append", default=[])
    a = ap.parse_args()
    import torch
    import train_targets_cases as C
    from train_targets_cost import bench_line, trace
    from spe_amd import camboxes, engine, infer, lib
    from spe_amd.evalmetrics import PseudoLabelMeter
    from spe_amd.models import conditional_detr as cd
    from spe_amd.util.misc import NestedTensor
    if not torch.cuda.is_available():
        raise SystemExit("pseudo_quality_cost: needs the GPU (a CPU timing says nothing about it)")
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
        boxes = torch.cat([0.3 + 0.4 * torch.rand(GT_ROWS, 2, generator=g), 0.2 + 0.5 * torch.rand(GT_ROWS, 2, generator=g)], dim=1)
        host_targets.append({"img_label": lab, "orig_size": torch.tensor([H, W]), "boxes": boxes,
                             "labels": torch.tensor([c + 1 for c in PRESENT[b]][:GT_ROWS])})
    args = argparse.Namespace(num_classes=CLASSES, cam_thr=0.2, multi_box_ratio=0.5, num_refines=STAGES)
    post = {"bbox": cd.PostProcessRefine()}
    moved = [{k: v.to(dev) for k, v in t.items()} for t in host_targets]          # the loop moves the targets before the forward: not timed
    meter = PseudoLabelMeter(KC, NAMES)

    def section(m):
        present = camboxes.present_lists(host_targets, "img_label")
        targets = [dict(t) for t in moved]
        pseudo = camboxes.pseudo_targets(outputs[0], samples, present, args.num_classes, args.cam_thr, args.multi_box_ratio)
        uniq = infer.ClassTable([[c for c in cl if c < KC] for cl in pseudo.classes], dev).per_image()
        if m is not None:
            gt = [{"boxes": t["boxes"], "labels": t["labels"]} for t in targets]
        for t, p, u in zip(targets, pseudo.per_image(), uniq):
            t.update(p)
            t["labels_unique"] = u
        refine = engine.get_refinements_pseudo_label(outputs, samples, targets, args, post)
        if m is not None:
            m.update("cam", pseudo, gt)
            for rf, rows in refine.items():
                m.update(f"rf_{rf}", rows, gt)
        return pseudo, refine

    plain, with_meter = (lambda: section(None)), (lambda: section(meter))
    pseudo, refine = with_meter()
    cpu = PseudoLabelMeter(KC, NAMES)
    gt = [{"boxes": t["boxes"], "labels": t["labels"]} for t in host_targets]
    cpu.update("cam", [{k: v.cpu() for k, v in p.items()} for p in pseudo.per_image()], gt)
    for rf, rows in refine.items():
        cpu.update(f"rf_{rf}", [{k: r[k].cpu() for k in ("boxes", "labels", "scores")} for r in rows], gt)
    assert torch.equal(meter.counters(), cpu.counters()), "the device meter and the CPU meter disagree"
    rows0 = pseudo.boxes.shape[0]
    med = {"plain": [], "meter": []}
    for _ in range(RUNS):
        t_p, t_m = [], []
        for it in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            s0 = time.perf_counter()
            plain()
            torch.cuda.synchronize()
            s1 = time.perf_counter()
            with_meter()
            torch.cuda.synchronize()
            s2 = time.perf_counter()
            if it >= a.warmup:
                t_p.append((s1 - s0) * 1e3); t_m.append((s2 - s1) * 1e3)
        med["plain"].append(statistics.median(t_p)); med["meter"].append(statistics.median(t_m))
    show = lambda v: "n/a" if v is None else str(v)
    lines = ["Scoring the pseudo labels inside the training loop's target section on the MI355X (tools/pseudo_quality_cost.py; host clock around",
             f"work ending in a device synchronise; cfg2: B = {B} at {H} x {W}, {sum(map(len, PRESENT))} maps -> {rows0} stage-0 rows, Q = {Q}, Kc = {KC}, {STAGES} refinement",
             f"stages, {GT_ROWS} ground-truth rows per image; plain / meter alternating on the same outputs, {RUNS} runs of {a.steps} alternations, the median of every run)", ""]
    for name, fn in (("plain", plain), ("meter", with_meter)):
        lib.count_launches(True)
        fn()
        launches = lib.count_launches(False)
        k, c, s = trace(fn)
        lines.append(f"    {name:<6} medians " + ", ".join("%.3f" % m for m in med[name]) + f" ms   device kernels {show(k)}, copies {show(c)}, synchronising torch calls {show(s)}")
        lines.append(f"           library launches {dict(sorted(launches.items()))}")
    diff = [m - p for m, p in zip(med["meter"], med["plain"])]
    lines += ["", "meter - plain per run: " + ", ".join("%+.3f" % d for d in diff) + f" ms for {len(NAMES)} updates", ""]
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
