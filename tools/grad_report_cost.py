"""Measured cost of the gradient report of FlatAdamW (skip_report=..., grad_stats()) at cfg2's parameter layout -> profiles/grad_report.txt.

    python tools/grad_report_cost.py                                   # one process: the variants alternating, one JSON line
    python tools/grad_report_cost.py --only-off                        # the guarded step without the report alone (what a parent tree understands)
    python tools/grad_report_cost.py --compare PARENT_TREE [out.txt]   # the file: (a) parent against this tree, (b) the gated launches, (c) grad_stats()

The set-up is that of tools/adamw_ema_cost.py: parameters with the shapes of the bench.py model (TSCAM_cait_S24, cfg2; built on the host
for its shapes only) in flat buckets on the device, one GradAllReducer + FlatAdamW(max_grad_norm=0.1, skip_nonfinite=True) per variant,
the buckets filled with random (finite) gradients, so every step is applied and the report's launches take their gated exit.  Device
events around `--inner` consecutive calls give ms per call; the variants alternate `--rounds` times inside ONE process after `--warmup`
rounds.  Median over the rounds, spread = their 10th .. 90th percentile.  The launches of one step are counted per entry point.

--compare runs every part in a fresh child process, `--root` choosing the tree whose spe_amd is imported: PARENT_TREE is a built
checkout of the parent commit."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12            # bytes / s: the data sheet's peak and the measured rate of a float4 copy on this chip
VARIANTS = {"guarded": {}, "guarded+report": {"skip_report": "first"}}


def _root(a):
    root = os.path.abspath(a.root) if a.root else os.path.dirname(HERE)
    sys.path.insert(0, root)
    return root


def _stats(ms):
    ms = sorted(ms)
    q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]
    return {"ms_median": statistics.median(ms), "ms_min": ms[0], "ms_p10": q(0.1), "ms_p90": q(0.9)}


def measure(a):
    root = _root(a)
    import torch
    import bench
    from spe_amd import lib
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
    variants = ["guarded"] if a.only_off else list(VARIANTS)
    opts = {}
    for v in variants:
        g = torch.Generator().manual_seed(1)
        ps = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.02).to(dev)) for _, s in named]
        red = GradAllReducer(ps, flatten_params=True)
        groups = [{"params": [p for (n, _), p in zip(named, ps) if "backbone" not in n], "lr": 1e-4},
                  {"params": [p for (n, _), p in zip(named, ps) if "backbone" in n], "lr": 1e-5}]
        opt = FlatAdamW(groups, red, lr=1e-4, weight_decay=1e-4, max_grad_norm=0.1, write_clipped_grads=False, skip_nonfinite=True,
                        **VARIANTS[v])
        for b in red.buckets:
            b["flat"].normal_(0.0, 0.01, generator=None)
        opts[v] = (opt, red)
    calls = {v: opts[v][0].step for v in variants}
    if not a.only_off:
        calls["grad_stats"] = lambda: opts["guarded"][0].grad_stats(raw=True)
    torch.cuda.synchronize()
    times = {v: [] for v in calls}
    for r in range(a.warmup + a.rounds):
        for v, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                f()
            e1.record()
            if r >= a.warmup:
                times[v].append((e0, e1))
    torch.cuda.synchronize()
    red = opts[variants[0]][1]
    elements = sum(b["flat"].numel() for b in red.buckets)
    out = {"root": root, "inner": a.inner, "rounds": a.rounds, "buckets": len(red.buckets), "elements": elements,
           "parameters": len(named), "largest_parameter": max(p.numel() for b in red.buckets for p, _ in b["offsets"])}
    for v, f in calls.items():
        out[v] = _stats([x.elapsed_time(y) / a.inner for x, y in times[v]])
        lib.count_launches(True)
        f()
        out[v]["launches"] = lib.count_launches(False)
    torch.cuda.synchronize()
    if not a.only_off:
        assert opts["guarded+report"][0].skipped_steps() == 0 and opts["guarded+report"][0].skip_report() is None
        out["grad_stats"]["bytes"] = 8 * elements
    print(json.dumps(out))


def child(cmd, cwd, timeout):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=timeout, cwd=cwd)
    if r.returncode != 0:                   # no further GPU work after a child that did not end cleanly
        raise SystemExit(f"{' '.join(cmd)} ended with status {r.returncode}")
    last = r.stdout.strip().splitlines()[-1]
    print(f"done: {' '.join(cmd[1:])} (in {cwd})\n    {last}", file=sys.stderr, flush=True)
    return json.loads(last)


def compare(a):
    here, parent = os.path.dirname(HERE), os.path.abspath(a.compare)
    me = [sys.executable, os.path.abspath(__file__), "--inner", str(a.inner), "--rounds", str(a.rounds), "--warmup", str(a.warmup)]
    base, mine = [], []
    for _ in range(2):
        base.append(child(me + ["--root", parent, "--only-off"], parent, 300))
        mine.append(child(me + ["--root", here, "--only-off"], here, 300))
    both = [child(me + ["--root", here], here, 300) for _ in range(2)]
    f = lambda d: f"median {d['ms_median']:.4f}  min {d['ms_min']:.4f}  p10 .. p90 {d['ms_p10']:.4f} .. {d['ms_p90']:.4f}"
    b0 = both[0]
    lines = [
        "# gradient report of FlatAdamW: measured cost at cfg2's parameter layout on one MI355X (tools/grad_report_cost.py --compare)",
        f"# {b0['elements']} fp32 elements, {b0['parameters']} parameters (the largest {b0['largest_parameter']} elements) in {b0['buckets']} bucket(s);",
        f"# ms per call, device events around {a.inner} consecutive calls, {a.warmup} warm-up + {a.rounds} timed rounds per variant; finite gradients",
        "",
        "(a) the guarded step with skip_report off: parent commit and this tree, alternating processes",
    ]
    for i, (p, m) in enumerate(zip(base, mine)):
        lines += [f"    parent     {i}  {f(p['guarded'])}", f"    this tree  {i}  {f(m['guarded'])}"]
    same = base[0]["guarded"]["launches"] == mine[0]["guarded"]["launches"]
    lines += [f"    launches of one step, parent:    {json.dumps(base[0]['guarded']['launches'], sort_keys=True)}",
              f"    launches of one step, this tree: {json.dumps(mine[0]['guarded']['launches'], sort_keys=True)}",
              f"    {'THE SAME LAUNCHES' if same else 'DIFFERENT LAUNCHES'}",
              "", "(b) skip_report off and skip_report='first' on clean gradients (every report launch takes its gated exit), alternating inside one",
              "    process (two processes)"]
    for i, r in enumerate(both):
        for v in VARIANTS:
            lines.append(f"    process {i}  {v:<15} {f(r[v])}")
        d = r["guarded+report"]["ms_median"] - r["guarded"]["ms_median"]
        lines.append(f"    process {i}  report on - report off (medians): {d:+.4f} ms  ({100 * d / r['guarded']['ms_median']:+.1f} %)")
    lines += [f"    launches of one step with the report: {json.dumps(b0['guarded+report']['launches'], sort_keys=True)}",
              "    yardstick: the weight-EMA stream, +0.09 ms on the 0.53 ms step (profiles/adamw_ema.txt)",
              "", "(c) one grad_stats(raw=True) call: one unconditional spe_grad_report per bucket over gradients and parameters"]
    for i, r in enumerate(both):
        s = r["grad_stats"]
        t = s["ms_median"] * 1e-3
        lines += [f"    process {i}  {f(s)}",
                  f"    process {i}  {s['bytes']} bytes read once: {s['bytes'] / t / 1e12:.2f} TB/s = {100 * s['bytes'] / t / HBM_COPY:.0f} % of the measured copy rate "
                  f"({HBM_COPY / 1e12:.2f} TB/s: {1e3 * s['bytes'] / HBM_COPY:.3f} ms), {100 * s['bytes'] / t / HBM_SPEC:.0f} % of the {HBM_SPEC / 1e12:.1f} TB/s data-sheet peak"]
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
    ap.add_argument("--only-off", action="store_true", help="the guarded step without the report alone (what a parent tree understands)")
    ap.add_argument("--compare", default=None, metavar="PARENT_TREE")
    ap.add_argument("out", nargs="?", default=None)
    a = ap.parse_args()
    if a.compare:
        compare(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
