"""Measured cost of the guarded optimizer step (FlatAdamW(..., skip_nonfinite=True)) at cfg2's parameter count -> profiles/adamw_guard.txt.

    python tools/adamw_guard_cost.py                                   # one process: unguarded and guarded alternating, JSON line
    python tools/adamw_guard_cost.py --compare PARENT_TREE [out.txt]   # the file: that, the parent's unguarded step, two bench lines

One measurement: parameters with the shapes of the bench.py model (TSCAM_cait_S24, cfg2; built on the host for its shapes only) in
flat buckets on the device, one GradAllReducer + FlatAdamW(max_grad_norm=0.1) per variant, the buckets filled with random gradients.
Device events around `--inner` consecutive optimizer.step() calls give ms per step; the variants alternate `--rounds` times inside
ONE process after `--warmup` rounds.  The figure is the median over the rounds, the spread their 10th .. 90th percentile.

--compare adds, each in a fresh child process with `--root` choosing the tree whose spe_amd is imported: the unguarded step of
PARENT_TREE (a built checkout of the parent commit - the yardstick) next to this tree's, alternating, and
`python bench.py --steps 20 --warmup 5` in both trees (the benchmark uses the unguarded path).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LAUNCH_US = 1.7             # a dependent boundary between two streaming kernels on one stream (the estimate's one constant)


def measure(a):
    root = os.path.abspath(a.root) if a.root else os.path.dirname(HERE)
    sys.path.insert(0, root)
    import torch
    import bench
    from spe_amd.dp import GradAllReducer
    from spe_amd.optim import FlatAdamW
    from spe_amd.models import build_model
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    margs = bench.model_args()
    margs.device = "cpu"
    model = build_model(margs)[0]
    named = [(n, tuple(p.shape)) for n, p in model.named_parameters() if p.requires_grad]
    del model
    variants = ["unguarded"] if a.only_unguarded else ["unguarded", "guarded"]
    opts = {}
    for v in variants:
        g = torch.Generator().manual_seed(1)
        ps = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.02).to(dev)) for _, s in named]
        red = GradAllReducer(ps, flatten_params=True)
        groups = [{"params": [p for (n, _), p in zip(named, ps) if "backbone" not in n], "lr": 1e-4},
                  {"params": [p for (n, _), p in zip(named, ps) if "backbone" in n], "lr": 1e-5}]
        kw = {"skip_nonfinite": True} if v == "guarded" else {}      # unguarded: the constructor call a parent tree understands
        opt = FlatAdamW(groups, red, lr=1e-4, weight_decay=1e-4, max_grad_norm=0.1, write_clipped_grads=False, **kw)
        for b in red.buckets:
            b["flat"].normal_(0.0, 0.01, generator=None)
        opts[v] = (opt, red)
    times = {v: [] for v in variants}
    for r in range(a.warmup + a.rounds):
        for v in variants:
            opt = opts[v][0]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                opt.step()
            e1.record()
            if r >= a.warmup:
                times[v].append((e0, e1))
    torch.cuda.synchronize()
    red = opts[variants[0]][1]
    out = {"root": root, "inner": a.inner, "rounds": a.rounds, "buckets": len(red.buckets),
           "elements": sum(b["flat"].numel() for b in red.buckets)}
    for v in variants:
        ms = sorted(x.elapsed_time(y) / a.inner for x, y in times[v])
        q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]
        out[v] = {"ms_median": statistics.median(ms), "ms_min": ms[0], "ms_p10": q(0.1), "ms_p90": q(0.9)}
    if "guarded" in opts:
        o = opts["guarded"][0]
        out["guarded_counts"] = [o.applied_steps(), o.skipped_steps()]
    print(json.dumps(out))


def child(cmd, cwd, timeout):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=timeout, cwd=cwd)
    if r.returncode != 0:                   # no further GPU work after a child that did not end cleanly
        raise SystemExit(f"{' '.join(cmd)} ended with status {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def compare(a):
    here, parent = os.path.dirname(HERE), os.path.abspath(a.compare)
    me = [sys.executable, os.path.abspath(__file__), "--inner", str(a.inner), "--rounds", str(a.rounds), "--warmup", str(a.warmup)]
    both = [child(me + ["--root", here], here, 300) for _ in range(2)]
    base, mine = [], []
    for _ in range(2):
        base.append(child(me + ["--root", parent, "--only-unguarded"], parent, 300))
        mine.append(child(me + ["--root", here, "--only-unguarded"], here, 300))
    bench_cmd = [sys.executable, "bench.py", "--steps", "20", "--warmup", "5", "--no-cpu-baseline"]
    bp = [child(bench_cmd, parent, 600)]
    bm = [child(bench_cmd, here, 600)]
    bp.append(child(bench_cmd, parent, 600))
    bm.append(child(bench_cmd, here, 600))
    f = lambda d: f"median {d['ms_median']:.4f}  min {d['ms_min']:.4f}  p10 .. p90 {d['ms_p10']:.4f} .. {d['ms_p90']:.4f}"
    nb = both[0]["buckets"]
    lines = [
        "# guarded optimizer step: measured cost at cfg2's parameter count on one MI355X (tools/adamw_guard_cost.py --compare)",
        f"# {both[0]['elements']} fp32 elements in {nb} bucket(s); ms per optimizer.step(), device events around {a.inner} consecutive steps,",
        f"# {a.warmup} warm-up + {a.rounds} timed rounds per variant",
        "",
        "(a) unguarded and guarded alternating inside one process (two processes)",
    ]
    for i, r in enumerate(both):
        lines += [f"    process {i}  unguarded  {f(r['unguarded'])}",
                  f"    process {i}  guarded    {f(r['guarded'])}   (applied, skipped) = {tuple(r['guarded_counts'])}",
                  f"    process {i}  guarded - unguarded (medians): {r['guarded']['ms_median'] - r['unguarded']['ms_median']:+.4f} ms"]
    lines += ["", "(b) the unguarded step alone: parent commit and this tree, alternating processes"]
    for i, (p, m) in enumerate(zip(base, mine)):
        lines += [f"    parent     {i}  {f(p['unguarded'])}", f"    this tree  {i}  {f(m['unguarded'])}"]
    lines += ["", "(c) python bench.py --steps 20 --warmup 5 (unguarded path), parent commit and this tree, alternating"]
    for i, (p, m) in enumerate(zip(bp, bm)):
        lines += [f"    parent     {i}  {p['value']:.3f} {p['unit']}", f"    this tree  {i}  {m['value']:.3f} {m['unit']}"]
    lines += ["", f"Expected difference of (a): + one one-workgroup launch (~{LAUNCH_US} us of dependent boundary) and, with the clip on in both, no",
              f"    extra norm pass; - the {nb} x up to 2048 per-workgroup reductions of the partials in the update's prologue."]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--root", default=None, help="tree whose spe_amd / bench are imported (default: this one)")
    ap.add_argument("--only-unguarded", action="store_true")
    ap.add_argument("--compare", default=None, metavar="PARENT_TREE")
    ap.add_argument("out", nargs="?", default=None)
    a = ap.parse_args()
    if a.compare:
        compare(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
