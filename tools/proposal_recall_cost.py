"""Measured cost of scoring every stage's query boxes while training runs (evalmetrics.ProposalRecallMeter, spe_proposal_recall) on the
GPU -> profiles/proposal_recall.txt.

    python tools/proposal_recall_cost.py [out.txt] [--bench-before line.json] [--bench-after line.json]

cfg2: B = 2 at 800 x 1333, 6 present maps, Q = 300, Kc = 21, two refinement stages, 3 ground-truth rows per image.  The target section of
engine._train_one_epoch - from the model's outputs to both target lists - in two forms, alternating on the same outputs in one process:

  plain   camboxes.pseudo_targets, 'labels_unique', PostProcessRefine's picks: what the loop does without a meter
  meter   the same, the loader's rows kept aside before the pseudo labels replace them, then one update per stage: 's0', 's1', 's2'

A host clock around work that ends in a device synchronise (tools/pseudo_quality_cost.py's method), three runs of --steps alternations
each, the median of every run.  Besides, for one call of either: the launches per entry point of the library, the device kernels and
copies of a torch.profiler trace, and the synchronising torch calls torch.cuda.set_sync_debug_mode('warn') reports; and the update
alone, and its kernel alone between two events.  The meter's counters are compared with the CPU meter's host composition over the
device's probabilities before anything is written."""
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
NAMES = [f"s{k}" for k in range(STAGES + 1)]
PSEUDO_UPDATE_MS = 0.076                                 # PseudoLabelMeter's update on the same box (profiles/pseudo_quality.txt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "proposal_recall.txt"))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--bench-before", action="append", default=[])
    ap.add_argument("--bench-after", action="append", default=[])
    a = ap.parse_args()
    import torch
    import proposal_recall_loops as PL
    import train_targets_cases as C
    from train_targets_cost import bench_line, trace
    from spe_amd import camboxes, engine, infer, lib
    from spe_amd.evalmetrics import ProposalRecallMeter
    from spe_amd.models import conditional_detr as cd
    from spe_amd.util.misc import NestedTensor
    if not torch.cuda.is_available():
        raise SystemExit("proposal_recall_cost: needs the GPU (a CPU timing says nothing about it)")
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
    make = lambda: ProposalRecallMeter(KC, NAMES)
    meter = make()

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
            for rf, out in outputs.items():
                m.update(f"s{rf}", out, gt)
        return pseudo, refine

    plain, with_meter = (lambda: section(None)), (lambda: section(meter))
    with_meter()
    gt_dev = [{"boxes": t["boxes"], "labels": t["labels"]} for t in moved]
    hand = PL.fed_by_hand(make(), ((f"s{rf}", out, gt_dev) for rf, out in outputs.items()))
    assert torch.equal(meter.counters(), hand.counters()), "the device meter and the host composition disagree"
    med = {"plain": [], "meter": [], "update": []}
    for _ in range(RUNS):
        t_p, t_m, t_u = [], [], []
        for it in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            s0 = time.perf_counter()
            plain()
            torch.cuda.synchronize()
            s1 = time.perf_counter()
            with_meter()
            torch.cuda.synchronize()
            s2 = time.perf_counter()
            meter.update("s1", outputs[1], gt_dev)
            torch.cuda.synchronize()
            s3 = time.perf_counter()
            if it >= a.warmup:
                t_p.append((s1 - s0) * 1e3); t_m.append((s2 - s1) * 1e3); t_u.append((s3 - s2) * 1e3)
        for k, v in (("plain", t_p), ("meter", t_m), ("update", t_u)):
            med[k].append(statistics.median(v))
    # the kernel alone, between two events on the stream
    from spe_amd import kernels as K
    import numpy as np
    prob = outputs[1]["pred_logits"].sigmoid()
    gboxes, glabels = torch.cat([t["boxes"] for t in gt_dev]).float().contiguous(), torch.cat([t["labels"] for t in gt_dev])
    host = np.arange(0, (B + 1) * GT_ROWS, GT_ROWS, dtype=np.int32)
    goff = torch.from_numpy(host).to(dev)
    scratch = torch.zeros_like(meter._counters[0])
    ev = []
    for it in range(a.warmup + a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        K.proposal_recall(prob, outputs[1]["pred_boxes"], gboxes, glabels, goff, host, KC, meter._thr, meter._ks, scratch)
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    kernel_us = statistics.median(e0.elapsed_time(e1) for e0, e1 in ev[a.warmup:]) * 1e3
    show = lambda v: "n/a" if v is None else str(v)
    lines = ["Scoring every stage's query boxes inside the training loop's target section on the MI355X (tools/proposal_recall_cost.py; host clock",
             f"around work ending in a device synchronise; cfg2: B = {B} at {H} x {W}, {sum(map(len, PRESENT))} maps, Q = {Q}, Kc = {KC}, {STAGES} refinement stages,",
             f"{GT_ROWS} ground-truth rows per image, thresholds {meter.iou_threshs}, ks {meter.ks}; plain / meter alternating on the same outputs, {RUNS} runs of",
             f"{a.steps} alternations, the median of every run)", ""]
    for name, fn in (("plain", plain), ("meter", with_meter)):
        lib.count_launches(True)
        fn()
        launches = lib.count_launches(False)
        k, c, s = trace(fn)
        lines.append(f"    {name:<6} medians " + ", ".join("%.3f" % m for m in med[name]) + f" ms   device kernels {show(k)}, copies {show(c)}, synchronising torch calls {show(s)}")
        lines.append(f"           library launches {dict(sorted(launches.items()))}")
    diff = [m - p for m, p in zip(med["meter"], med["plain"])]
    lines += ["", "meter - plain per run: " + ", ".join("%+.3f" % d for d in diff) + f" ms for {len(NAMES)} updates",
              "one update alone (host clock to a synchronise): " + ", ".join("%.3f" % m for m in med["update"]) +
              f" ms; PseudoLabelMeter's update: {PSEUDO_UPDATE_MS} ms (profiles/pseudo_quality.txt)",
              "spe_proposal_recall alone between two events (launch included): %.1f us" % kernel_us, ""]
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
