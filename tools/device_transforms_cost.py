"""Measured cost of the input transforms on the device (spe_amd.transforms.collate_fn and its kernels) against the same work
through Pillow + torch on the host -> profiles/device_transforms.txt.

    python tools/device_transforms_cost.py [out.txt]

B = 2 at the workload's own sizes.  "plain": 375 x 500 -> 800 x 1066 and 480 x 640 -> 800 x 1066, one resize each.  "chained":
both images through the second arm of RandomSelect, 375 x 500 -> 600 x 800 -> crop 560 x 720 -> 800 x 1028 and 480 x 640 ->
600 x 800 -> crop 560 x 720 -> 800 x 1028, under a flip.  The uint8 sources are already on the device (a loader's copy of 0.56 /
0.92 MB overlaps the step); the draws are fixed so that every repetition does the same work.

Device: the whole collate_fn call between two device events around synchronised work (host planning, the descriptor upload and
the allocations included), `--steps` calls after `--warmup`, median and 10th .. 90th percentile, and the host clock around the
same calls as a cross-check; in a second pass of the same
length, each entry point between events of its own (spe_amd.kernels.enable_timing), the launches of one call added up (an event
pair around an empty launch costs a few microseconds itself: the tables launch shows that floor).  The bytes each kernel must
move are computed from the shapes; its share of the HBM bound is those bytes / 6.3 TB/s (the achievable rate, 8 TB/s spec) over its time.
Host: Image.resize + crop + transpose, to_tensor + normalize in torch CPU fp32, the padding collate and the .to(device) of the
batch, wall clock ending in a device synchronise - when Pillow is importable where this runs; else "not measured here"."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
STEP_MS = 47.0              # the cfg2 training step this is held against
HBM_BPS = 6.3e12
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
# per image: source (h, w), then flip and the ops in order
PLAIN = [((375, 500), False, [("resize", 800, 1066)]), ((480, 640), False, [("resize", 800, 1066)])]
CHAINED = [((375, 500), True, [("resize", 600, 800), ("crop", 20, 40, 560, 720), ("resize", 800, 1028)]),
           ((480, 640), True, [("resize", 600, 800), ("crop", 20, 40, 560, 720), ("resize", 800, 1028)])]


def quantiles(ms):
    ms = sorted(ms)
    q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]
    return {"median": statistics.median(ms), "p10": q(0.1), "p90": q(0.9), "n": len(ms)}


def kernel_bytes(stage_lists):
    """Bytes each launch must move, from the shapes: {entry point: bytes summed over its launches in one collate_fn call}."""
    from spe_amd.kernels import RESAMPLE_DESC
    depth = max(len(s) for s in stage_lists)
    rounds = [[s[len(s) - depth + r] for s in stage_lists if len(s) - depth + r >= 0] for r in range(depth)]
    b = {"spe_resample_tables": 0, "spe_resample_h": 0, "spe_resample_v": 0}
    Hm, Wm = max(s[-1][5] for s in stage_lists), max(s[-1][6] for s in stage_lists)
    for r, jobs in enumerate(rounds):
        for (x0, y0, cw, ch, flip, oh, ow) in jobs:
            kx, ky = 2 * -(-max(cw, ow) // ow) + 1, 2 * -(-max(ch, oh) // oh) + 1
            tab = 4 * (ow * (2 + kx) + oh * (2 + ky))
            tmp = 3 * ch * ((ow + 3) & ~3)
            b["spe_resample_tables"] += tab + 8 * RESAMPLE_DESC
            b["spe_resample_h"] += 3 * cw * ch + tmp + tab
            b["spe_resample_v"] += tmp + tab + (3 * oh * ow if r < depth - 1 else 0)
        if r == depth - 1:
            b["spe_resample_v"] += len(jobs) * (12 * Hm * Wm + Hm * Wm) + 3072
    return b


def build(sample_specs, dev, seed):
    import torch
    from spe_amd import transforms as T
    g = torch.Generator().manual_seed(seed)
    srcs = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g) for (h, w), _, _ in sample_specs]
    dsrcs = [s.to(dev) for s in srcs]
    norm = T.Compose([T.ToTensor(), T.Normalize(MEAN, STD)])

    def samples():
        out = []
        for d, (_, flip, ops) in zip(dsrcs, sample_specs):
            im = T.DeviceImage(d)
            im = im.hflip() if flip else im
            for op in ops:
                im = im.resize(op[1], op[2]) if op[0] == "resize" else im.crop(*op[1:])
            out.append(norm(im, None))
        return out
    return srcs, samples


def host_path(srcs, sample_specs, dev):
    """The reference's way: Pillow per image, to_tensor + normalize, zero-padded batch, copy to the device."""
    import numpy as np
    import torch
    from PIL import Image
    mean, std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
    ts = []
    for s, (_, flip, ops) in zip(srcs, sample_specs):
        im = Image.fromarray(s.numpy())
        im = im.transpose(Image.FLIP_LEFT_RIGHT) if flip else im
        for op in ops:
            im = im.resize((op[2], op[1]), Image.BILINEAR) if op[0] == "resize" else im.crop((op[2], op[1], op[2] + op[4], op[1] + op[3]))
        t = torch.from_numpy(np.array(im, np.uint8, copy=True)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        ts.append(t.sub_(mean).div_(std))
    H, W = max(t.shape[1] for t in ts), max(t.shape[2] for t in ts)
    tensor = torch.zeros((len(ts), 3, H, W))
    mask = torch.ones((len(ts), H, W), dtype=torch.bool)
    for t, p, m in zip(ts, tensor, mask):
        p[:, :t.shape[1], :t.shape[2]].copy_(t)
        m[:t.shape[1], :t.shape[2]] = False
    return tensor.to(dev), mask.to(dev)


def measure(a, name, sample_specs):
    import torch
    from spe_amd import kernels as K, transforms as T
    dev = torch.device("cuda:0")
    srcs, samples = build(sample_specs, dev, 77)
    call, wall = [], []
    for it in range(a.warmup + a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        nt, _ = T.collate_fn(samples())
        e1.record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            call.append(e0.elapsed_time(e1))
            wall.append((time.perf_counter() - t0) * 1e3)
    names = ["spe_resample_tables", "spe_resample_h", "spe_resample_v"]
    K.enable_timing(names)
    for it in range(a.steps):
        T.collate_fn(samples())
    torch.cuda.synchronize()
    launches = {n: len(ev) // a.steps for n, ev in K._TIMED.items()}
    per = {}
    for n, ev in K._TIMED.items():              # per call: the launches of one collate_fn call added up
        ms = [x.elapsed_time(y) for x, y in ev]
        per[n] = quantiles([sum(ms[i:i + launches[n]]) for i in range(0, len(ms), launches[n])])
    K.enable_timing([])
    stage_lists = [T.plan_stages(s[0].image) for s in samples()]
    res = {"name": name, "shape": list(nt.tensors.shape), "call_ms": quantiles(call), "call_wall_ms": quantiles(wall), "kernel_ms": per, "launches": launches,
           "kernel_bytes": kernel_bytes(stage_lists), "host_ms": None, "host_equal": None}
    try:
        import PIL  # noqa: F401
    except ImportError:
        return res
    if a.host_steps <= 0:
        return res
    wall = []                                   # the host path, from here on
    for it in range(3 + a.host_steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ht, hm = host_path(srcs, sample_specs, dev)
        torch.cuda.synchronize()
        if it >= 3:
            wall.append((time.perf_counter() - t0) * 1e3)
    res["host_ms"] = quantiles(wall)
    res["host_equal"] = bool(torch.equal(ht, nt.tensors) and torch.equal(hm, nt.mask))
    res["host_threads"] = torch.get_num_threads()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-steps", type=int, default=20)
    ap.add_argument("out", nargs="?", default=None)
    a = ap.parse_args()
    res = [measure(a, "plain", PLAIN), measure(a, "chained", CHAINED)]
    f = lambda q: f"{q['median']:.3f} ms (p10 .. p90: {q['p10']:.3f} .. {q['p90']:.3f}, n = {q['n']})"
    lines = ["# Input transforms on one MI355X: spe_amd.transforms.collate_fn, B = 2, against Pillow + torch on the host",
             f"# (tools/device_transforms_cost.py; device events around synchronised work, {a.warmup} warm-up + {a.steps} timed calls;",
             f"# per-kernel times per call from a second pass with events around every entry point; HBM bound at {HBM_BPS / 1e12:.1f} TB/s)", ""]
    for r in res:
        lines += [f"{r['name']}: batch {r['shape']}",
                  f"    collate_fn, whole call: {f(r['call_ms'])} = {100 * r['call_ms']['median'] / STEP_MS:.2f} % of a {STEP_MS:.0f} ms step",
                  f"        the same calls by the host clock, building the lazy images and the final synchronise included: {f(r['call_wall_ms'])}"]
        for n, q in r["kernel_ms"].items():
            by, ln = r["kernel_bytes"][n], r["launches"][n]
            bound_ms = by / HBM_BPS * 1e3
            lines.append(f"    {n:20s} {ln} launch(es) per call, together {f(q)}; must move {by / 1e6:.2f} MB per call = "
                         f"{bound_ms * 1e3:.1f} us at the HBM bound = {100 * bound_ms / q['median']:.1f} % of its time")
        if r["host_ms"] is None:
            lines.append("    host path: Pillow is not importable on this machine - not measured here")
        else:
            lines += [f"    host path (Pillow + torch CPU, {r['host_threads']} torch threads, one process, copy to the device included): {f(r['host_ms'])}"
                      f" = {100 * r['host_ms']['median'] / STEP_MS:.0f} % of a {STEP_MS:.0f} ms step; output equal to the device path: "
                      f"{'yes' if r['host_equal'] else 'NO'}",
                      f"    device path {'faster' if r['call_ms']['median'] < r['host_ms']['median'] else 'NOT faster'}: "
                      f"{r['host_ms']['median'] / r['call_ms']['median']:.1f} x"]
        lines.append("")
    text = "\n".join(lines)
    print(text, file=sys.stderr)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
