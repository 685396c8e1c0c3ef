"""Measured cost of gradient accumulation (GradAllReducer(accum_steps=K)) at cfg2 -> profiles/grad_accum.txt.

    python tools/grad_accum_cost.py --accum 4                         # one measurement: ms per backward + finish(), JSON line
    python tools/grad_accum_cost.py --compare PARENT_TREE [out.txt]   # the two comparisons below

One measurement: the bench.py step (TSCAM_cait_S24, 2 x 800 x 1333, bf16s) with device events around `total.backward();
reducer.finish()` of every micro-step; forward and optimizer step run untimed in between.  `--steps` optimizer steps are timed after
`--warmup`; the figure is the median over all timed micro-steps, the spread their 10th .. 90th percentile.

--compare runs every measurement in a fresh child process, with `--root` choosing the tree whose spe_amd is imported:
  (a) accum_steps = 1 in this tree against PARENT_TREE (a built checkout of the parent commit), alternating, `--rounds` times each:
      that code path is meant to be unchanged, so this tree has to sit inside the parent's own run-to-run spread;
  (b) accum_steps = 4 in this tree: extra ms per micro-step over (a), next to the estimate from the bytes the merge pass moves.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
HBM_GBS = 6300.0            # achievable HBM bandwidth of one MI355X


def measure(a):
    root = os.path.abspath(a.root) if a.root else os.path.dirname(HERE)
    sys.path.insert(0, root)
    import torch
    import bench
    from spe_amd import kernels as K
    from spe_amd.dp import GradAllReducer
    from spe_amd.optim import FlatAdamW
    from spe_amd.models import build_model
    from spe_amd.util.misc import NestedTensor
    dev = torch.device("cuda:0")
    K.set_precision("bf16s")
    K.manual_seed(1234)
    torch.manual_seed(0)
    model, crit, crit_r, pp, rpp = build_model(bench.model_args())
    model.to(dev).train(); crit.to(dev).train(); crit_r.to(dev).train()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    kw = {"accum_steps": a.accum} if a.accum > 1 else {}       # accum_steps = 1: the constructor call a parent tree understands
    reducer = GradAllReducer([p for _, p in named], flatten_params=True, **kw)
    groups = [{"params": [p for n, p in named if "backbone" not in n], "lr": 1e-4},
              {"params": [p for n, p in named if "backbone" in n], "lr": 1e-5}]
    opt = FlatAdamW(groups, reducer, lr=1e-4, weight_decay=1e-4, max_grad_norm=0.1)
    batches = []
    for k in range(a.accum):
        img, mask, tg = bench.synth_batch(1234 + k, dev)
        batches.append((NestedTensor(img, mask), tg))
    events = []

    def step(timed):
        for samples, tg in batches:
            reducer.reset()
            out = model(samples)
            l0 = crit(out[0], tg)
            with torch.no_grad():
                ps = bench.pseudo_labels(rpp, out[0], tg)
            l1 = crit_r(out[1], ps)
            total = bench.weighted_total(l0, l1, crit.weight_dict)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            total.backward()
            reducer.finish()
            e1.record()
            if timed:
                events.append((e0, e1))
        opt.step()

    for _ in range(a.warmup):
        step(False)
    torch.cuda.synchronize()
    for _ in range(a.steps):
        step(True)
    torch.cuda.synchronize()
    ms = sorted(x.elapsed_time(y) for x, y in events)
    q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]
    nbytes = sum(b["flat"].numel() * 4 for b in reducer.buckets)
    print(json.dumps({"root": root, "accum_steps": a.accum, "micro_steps_timed": len(ms), "ms_median": statistics.median(ms),
                      "ms_p10": q(0.1), "ms_p90": q(0.9), "bucket_bytes": nbytes}))


def child(root, accum, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--accum", str(accum), "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--root", root]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=240, cwd=root)
    if r.returncode != 0:                   # no further GPU work after a child that did not end cleanly
        raise SystemExit(f"{' '.join(cmd)} ended with status {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def compare(a):
    here, parent = os.path.dirname(HERE), os.path.abspath(a.compare)
    base, mine = [], []
    for _ in range(a.rounds):
        base.append(child(parent, 1, a))
        mine.append(child(here, 1, a))
    acc = [child(here, 4, a) for _ in range(3)]
    med = lambda rs: [r["ms_median"] for r in rs]
    fmt = lambda xs: ", ".join(f"{x:.3f}" for x in xs)
    nbytes = acc[0]["bucket_bytes"]
    # a non-final micro-step reads the bucket (micro-step 0) or the bucket and the running sum, and writes the running sum; the final
    # one reads both and writes the bucket: 3 bucket-sized streams at most
    est = 3 * nbytes / (HBM_GBS * 1e9) * 1e3
    m1, m4 = statistics.median(med(mine)), statistics.median(med(acc))
    lines = [
        "# gradient accumulation: measured cost at cfg2 on one MI355X (tools/grad_accum_cost.py --compare)",
        f"# TSCAM_cait_S24, 2 x 800 x 1333, bf16s; ms per `backward(); finish()`, device events, {a.warmup} warm-up + {a.steps} timed optimizer",
        "# steps per process, median over the timed micro-steps; one fresh process per figure",
        "",
        f"(a) accum_steps = 1, parent commit and this tree alternating, {a.rounds} processes each",
        f"    parent     medians: {fmt(med(base))}   min {min(med(base)):.3f}  max {max(med(base)):.3f}  median {statistics.median(med(base)):.3f}",
        f"    this tree  medians: {fmt(med(mine))}   min {min(med(mine)):.3f}  max {max(med(mine)):.3f}  median {m1:.3f}",
        f"    within one process (p10 .. p90): parent {base[0]['ms_p10']:.3f} .. {base[0]['ms_p90']:.3f}, this tree {mine[0]['ms_p10']:.3f} .. {mine[0]['ms_p90']:.3f}",
        f"    this tree's median inside the parent's run-to-run range: {'yes' if min(med(base)) <= m1 <= max(med(base)) else 'NO'}",
        "",
        f"(b) accum_steps = 4, this tree, 3 processes ({acc[0]['micro_steps_timed']} micro-steps each)",
        f"    medians: {fmt(med(acc))}   median {m4:.3f}   (p10 .. p90 of the first: {acc[0]['ms_p10']:.3f} .. {acc[0]['ms_p90']:.3f})",
        f"    extra per micro-step over accum_steps = 1: {m4 - m1:+.3f} ms",
        f"    estimate from bytes: buckets {nbytes / 1e6:.0f} MB, 3 streams per merge pass = {3 * nbytes / 1e9:.2f} GB at {HBM_GBS / 1e3:.1f} TB/s = {est:.3f} ms",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--accum", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--root", default=None, help="tree whose spe_amd / bench are imported (default: this one)")
    ap.add_argument("--compare", default=None, metavar="PARENT_TREE")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("out", nargs="?", default=None)
    a = ap.parse_args()
    if a.compare:
        compare(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
