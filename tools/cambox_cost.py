"""Measured cost of the CAM -> pseudo-box step (spe_amd.camboxes.get_pseudo_label_multi_boxes) with the borders found on the
host and on the device -> profiles/cambox_labels.txt.

    python tools/cambox_cost.py [out.txt]

Both contour paths are timed in this one process, alternating, on the same inputs: wall time of the whole call with a device
synchronise at both ends (the call ends in host work, so device events alone would miss most of the host path), `--steps` calls
after `--warmup`; the figure is the median, the spread the 10th .. 90th percentile.  Next to it, with device events, the two device
parts on their own: spe_cam_prepare, and the eight launches of spe_cam_boxes_device.  Shapes: the benchmark's (cfg2) B = 2 at
800 x 1333 with three present classes per image, and the launch scripts' B = 1 at 512 x 512 with two; class maps on the 16-pixel
patch grid, made of bumps plus noise."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
STEP_MS = 47.0              # the cfg2 training step this is held against


def make_inputs(B, H, W, present, Kc, dev, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    h, w = H // 16, W // 16
    yy, xx = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    cams = torch.zeros(B, Kc, h, w)
    for b in range(B):
        for c in range(Kc):
            for _ in range(3):
                cy, cx = torch.rand(2, generator=g) * torch.tensor([h - 1.0, w - 1.0])
                s = 2.0 + 6.0 * torch.rand(1, generator=g)
                cams[b, c] += torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s ** 2))
    cams += 0.05 * torch.randn(cams.shape, generator=g)
    labels = torch.zeros(B, Kc, dtype=torch.int64)
    for b in range(B):
        labels[b, torch.randperm(Kc, generator=g)[:present]] = 1
    targets = [{"img_label": labels[b].to(dev)} for b in range(B)]
    return {"cams_cls": cams.to(dev)}, torch.zeros(B, 3, H, W, device=dev), targets


def quantiles(ms):
    ms = sorted(ms)
    q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]
    return {"median": statistics.median(ms), "p10": q(0.1), "p90": q(0.9)}


def measure(a, B, H, W, present):
    import torch
    from spe_amd import camboxes, kernels as K
    dev = torch.device("cuda:0")
    Kc = 20
    args = argparse.Namespace(num_classes=Kc, cam_thr=0.2, multi_box_ratio=0.5)
    outputs, samples, targets = make_inputs(B, H, W, present, Kc, dev, 1234)
    wall = {"host": [], "device": []}
    results = {}
    for it in range(a.warmup + a.steps):
        for mode in ("host", "device"):
            camboxes.set_contours(mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results[mode] = camboxes.get_pseudo_label_multi_boxes(outputs, samples, targets, args)
            torch.cuda.synchronize()
            if it >= a.warmup:
                wall[mode].append((time.perf_counter() - t0) * 1e3)
    camboxes.set_contours("device")
    same = all(torch.equal(x["boxes"], y["boxes"]) and torch.equal(x["labels"], y["labels"])
               for x, y in zip(results["host"], results["device"]))
    # the device parts alone, by device events
    sel = [(b, c) for b in range(B) for c in range(Kc) if int(targets[b]["img_label"][c]) > 0]
    maps = outputs["cams_cls"][[s[0] for s in sel], [s[1] for s in sel]].float().contiguous()
    prep, lab = [], []
    for it in range(a.warmup + a.steps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        imgs = K.cam_prepare(maps, W, H, args.cam_thr)
        e[1].record()
        K.cam_boxes_device_packed(imgs, args.multi_box_ratio, camboxes.MAX_BOXES)
        e[2].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            prep.append(e[0].elapsed_time(e[1])); lab.append(e[1].elapsed_time(e[2]))
    return {"B": B, "H": H, "W": W, "maps": len(sel), "boxes": sum(int(x["boxes"].shape[0]) for x in results["device"]),
            "paths_equal": same, "host_ms": quantiles(wall["host"]), "device_ms": quantiles(wall["device"]),
            "cam_prepare_ms": quantiles(prep), "cam_boxes_device_ms": quantiles(lab),
            "workspace_mb": K.cam_boxes_workspace_bytes(len(sel), W, H) / 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("out", nargs="?", default=None)
    a = ap.parse_args()
    res = [measure(a, 2, 800, 1333, 3), measure(a, 1, 512, 512, 2)]
    f = lambda q: f"{q['median']:.3f} ms (p10 .. p90: {q['p10']:.3f} .. {q['p90']:.3f})"
    lines = ["# CAM -> pseudo boxes: get_pseudo_label_multi_boxes on one MI355X, borders found on the host against on the device",
             f"# (tools/cambox_cost.py; wall time of the whole call, synchronised at both ends, {a.warmup} warm-up + {a.steps} timed calls per path,",
             "# both paths alternating in one process; device parts by device events)", ""]
    for r in res:
        faster = r["device_ms"]["median"] < r["host_ms"]["median"]
        lines += [f"B = {r['B']}, {r['H']} x {r['W']}, {r['maps']} present-class maps, {r['boxes']} boxes, both paths equal: {'yes' if r['paths_equal'] else 'NO'}",
                  f"    host   contours, whole call: {f(r['host_ms'])} = {100 * r['host_ms']['median'] / STEP_MS:.1f} % of a {STEP_MS:.0f} ms step",
                  f"    device contours, whole call: {f(r['device_ms'])} = {100 * r['device_ms']['median'] / STEP_MS:.1f} % of a {STEP_MS:.0f} ms step",
                  f"    device path {'faster' if faster else 'NOT faster'}: {r['host_ms']['median'] / r['device_ms']['median']:.2f} x",
                  f"    device parts alone: spe_cam_prepare {f(r['cam_prepare_ms'])}; spe_cam_boxes_device (8 launches) {f(r['cam_boxes_device_ms'])}",
                  f"    workspace of spe_cam_boxes_device: {r['workspace_mb']:.1f} MB", ""]
    text = "\n".join(lines)
    print(text, file=sys.stderr)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
