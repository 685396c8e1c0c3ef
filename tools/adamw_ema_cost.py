"""Measured cost of the weight EMA inside the optimizer step (FlatAdamW(..., ema_decay=d)) at cfg2's parameter count -> profiles/adamw_ema.txt.

    python tools/adamw_ema_cost.py                                   # one process: EMA off / on, unguarded / guarded alternating, JSON line
    python tools/adamw_ema_cost.py --bits                            # sha256 of the EMA-off entries' results over the edge sizes, JSON line
    python tools/adamw_ema_cost.py --compare PARENT_TREE [out.txt]   # the file: (a) that, (b) the parent's EMA-off step and bits, (c) bench lines

The measurement is that of tools/adamw_guard_cost.py: parameters with the shapes of the bench.py model (TSCAM_cait_S24, cfg2; built on
the host for its shapes only) in flat buckets on the device, one GradAllReducer + FlatAdamW(max_grad_norm=0.1) per variant, the buckets
filled with random gradients.  Device events around `--inner` consecutive optimizer.step() calls give ms per step; the variants
alternate `--rounds` times inside ONE process after `--warmup` rounds.  Median over the rounds, spread = their 10th .. 90th percentile.

--compare runs every part in a fresh child process, `--root` choosing the tree whose spe_amd is imported: PARENT_TREE is a built
checkout of the parent commit - the yardstick for the EMA-off step (b) and for `python bench.py --steps 20 --warmup 5` (c; the
benchmark does not enable the EMA).
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [1, 3, 4, 5, 255, 256, 1023, 1024, 1025, 2048 * 1024 + 7]
VARIANTS = {"unguarded": {}, "unguarded+ema": {"ema_decay": 0.9998}, "guarded": {"skip_nonfinite": True},
            "guarded+ema": {"skip_nonfinite": True, "ema_decay": 0.9998}}


def _root(a):
    root = os.path.abspath(a.root) if a.root else os.path.dirname(HERE)
    sys.path.insert(0, root)
    return root


def measure(a):
    root = _root(a)
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
    variants = ["unguarded"] if a.only_off else list(VARIANTS)
    opts = {}
    for v in variants:
        g = torch.Generator().manual_seed(1)
        ps = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.02).to(dev)) for _, s in named]
        red = GradAllReducer(ps, flatten_params=True)
        groups = [{"params": [p for (n, _), p in zip(named, ps) if "backbone" not in n], "lr": 1e-4},
                  {"params": [p for (n, _), p in zip(named, ps) if "backbone" in n], "lr": 1e-5}]
        opt = FlatAdamW(groups, red, lr=1e-4, weight_decay=1e-4, max_grad_norm=0.1, write_clipped_grads=False, **VARIANTS[v])
        for b in red.buckets:
            b["flat"].normal_(0.0, 0.01, generator=None)
        opts[v] = (opt, red)
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
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
           "elements": sum(b["flat"].numel() for b in red.buckets), "allocated_bytes": mem}
    for v in variants:
        ms = sorted(x.elapsed_time(y) / a.inner for x, y in times[v])
        q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]
        out[v] = {"ms_median": statistics.median(ms), "ms_min": ms[0], "ms_p10": q(0.1), "ms_p90": q(0.9)}
        if "ema" in v:
            out[v]["ema_bytes"] = sum(e["ema"].numel() * 4 for e in opts[v][0]._buckets)
    print(json.dumps(out))


def bits(a):
    """sha256 over p, g, m, v after spe_adamw_flat and after spe_adamw_gate + spe_adamw_flat_guarded, at every edge size, clipped and
    unclipped, three segments: two trees whose lines agree compute the same bits."""
    root = _root(a)
    import torch
    from spe_amd import kernels as K, lib
    dev = torch.device("cuda:0")
    h = hashlib.sha256()
    for n in SIZES:
        for max_norm in (0.1, 0.0):
            for guarded in (False, True):
                gen = torch.Generator().manual_seed(n)
                p, g, m, v = (torch.randn(n, generator=gen).to(dev) for _ in range(4))
                v = v.abs()
                partials = torch.zeros(256, device=dev)
                seg = torch.tensor([n // 3, 2 * n // 3, n], dtype=torch.int64, device=dev)
                lr, wd = torch.tensor([1e-2, 3e-3, 1e-3], device=dev), torch.tensor([1e-2, 0.0, 1e-4], device=dev)
                lib.call("spe_sqnorm_partials", g.data_ptr(), n, partials.data_ptr(), 256, K._st())
                if guarded:
                    guard = torch.zeros(K.ADAMW_GUARD_WORDS, dtype=torch.int32, device=dev)
                    guard[0] = 2
                    K.adamw_gate(guard, partials, max_norm, 0.5, 0.9, 0.999)
                    K.adamw_flat_guarded(p, g, m, v, seg, lr, wd, 0.9, 0.999, 1e-8, guard, True)
                else:
                    K.adamw_flat(p, g, m, v, seg, lr, wd, 0.9, 0.999, 1e-8, 1 - 0.9 ** 3, 1 - 0.999 ** 3, partials, max_norm, True, grad_scale=0.5)
                for t in (p, g, m, v):
                    h.update(t.cpu().numpy().tobytes())
    print(json.dumps({"root": root, "sha256": h.hexdigest()}))


def child(cmd, cwd, timeout):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=timeout, cwd=cwd)
    if r.returncode != 0:                   # no further GPU work after a child that did not end cleanly
        raise SystemExit(f"{' '.join(cmd)} ended with status {r.returncode}")
    last = r.stdout.strip().splitlines()[-1]
    print(f"done: {' '.join(cmd[1:])} (in {cwd})\n    {last}", file=sys.stderr, flush=True)       # progress, and the figures should a later child fail
    return json.loads(last)


def compare(a):
    here, parent = os.path.dirname(HERE), os.path.abspath(a.compare)
    me = [sys.executable, os.path.abspath(__file__), "--inner", str(a.inner), "--rounds", str(a.rounds), "--warmup", str(a.warmup)]
    both = [child(me + ["--root", here], here, 300) for _ in range(2)]
    base, mine = [], []
    for _ in range(2):
        base.append(child(me + ["--root", parent, "--only-off"], parent, 300))
        mine.append(child(me + ["--root", here, "--only-off"], here, 300))
    hp, hm = child(me + ["--root", parent, "--bits"], parent, 300), child(me + ["--root", here, "--bits"], here, 300)
    bench_cmd = [sys.executable, "bench.py", "--steps", "20", "--warmup", "5", "--no-cpu-baseline"]
    bp, bm = [], []
    for _ in range(2):
        bp.append(child(bench_cmd, parent, 600))
        bm.append(child(bench_cmd, here, 600))
    f = lambda d: f"median {d['ms_median']:.4f}  min {d['ms_min']:.4f}  p10 .. p90 {d['ms_p10']:.4f} .. {d['ms_p90']:.4f}"
    nb, ne = both[0]["buckets"], both[0]["elements"]
    lines = [
        "# weight EMA inside the optimizer step: measured cost at cfg2's parameter count on one MI355X (tools/adamw_ema_cost.py --compare)",
        f"# {ne} fp32 elements in {nb} bucket(s); ms per optimizer.step(), device events around {a.inner} consecutive steps,",
        f"# {a.warmup} warm-up + {a.rounds} timed rounds per variant",
        "",
        "(a) EMA off and EMA on (ema_decay=0.9998, warm-up on), unguarded and guarded, alternating inside one process (two processes)",
    ]
    for i, r in enumerate(both):
        for v in VARIANTS:
            lines.append(f"    process {i}  {v:<14} {f(r[v])}")
        for v in ("unguarded", "guarded"):
            d = r[v + "+ema"]["ms_median"] - r[v]["ms_median"]
            lines.append(f"    process {i}  {v}: EMA on - EMA off (medians): {d:+.4f} ms  ({100 * d / r[v]['ms_median']:+.1f} %)")
    eb = both[0]["unguarded+ema"]["ema_bytes"]
    lines += [f"    EMA buffers: {eb} bytes ({eb / 1e6:.1f} MB) beside {4 * eb} bytes of parameters, gradients and both moments",
              "", "(b) the EMA-off unguarded step alone: parent commit and this tree, alternating processes"]
    for i, (p, m) in enumerate(zip(base, mine)):
        lines += [f"    parent     {i}  {f(p['unguarded'])}", f"    this tree  {i}  {f(m['unguarded'])}"]
    lines += [f"    results of spe_adamw_flat and spe_adamw_gate + spe_adamw_flat_guarded on n = {', '.join(str(n) for n in SIZES)}",
              "    (clipped and unclipped, three segments), sha256 over p, g, m, v:",
              f"    parent     {hp['sha256']}", f"    this tree  {hm['sha256']}",
              f"    {'IDENTICAL' if hp['sha256'] == hm['sha256'] else 'DIFFERENT'}"]
    lines += ["", "(c) python bench.py --steps 20 --warmup 5 (EMA off), parent commit and this tree, alternating"]
    for i, (p, m) in enumerate(zip(bp, bm)):
        lines += [f"    parent     {i}  {p['value']:.3f} {p['unit']}", f"    this tree  {i}  {m['value']:.3f} {m['unit']}"]
    lines += ["", "Expected difference of (a), by traffic: the update moves 28 B per element (p, m, v read and written, g read), the EMA adds 8 B:",
              f"    + {100 * 8 / 28:.0f} % of the update launches."]
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
    ap.add_argument("--only-off", action="store_true", help="the unguarded EMA-off variant alone (what a parent tree understands)")
    ap.add_argument("--bits", action="store_true")
    ap.add_argument("--compare", default=None, metavar="PARENT_TREE")
    ap.add_argument("out", nargs="?", default=None)
    a = ap.parse_args()
    if a.compare:
        compare(a)
    elif a.bits:
        bits(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
