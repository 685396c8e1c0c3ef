"""Measured cost of the woct0head backbones' additions (csrc/conv_head.hip, csrc/attn_pmean.hip) -> profiles/woct0_cost.txt.

    python tools/woct0_cost.py [out.txt]

  - conv class head forward / backward (map + pooled logits; dx + dW + db) at the XXS launch shape and at cfg2's token count;
  - the attention-probability accumulation per block (fused path) at N = 1024 and N = 4150;
  - one training step (forward, both criteria, backward; no optimiser) of TSCAM_cait_XXS36_Two_Branch_conv_cls_attn_woct0head against
    TSCAM_cait_XXS36_Two_Branch at 512 x 512 with script_voc's decoder settings (3 encoder / 6 decoder layers, 300 queries, layer_to_det 24).
Timings: CUDA events around N back-to-back repetitions after warm-up, median of 5 such windows.
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps=20, windows=5, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / reps)
    return statistics.median(out)


def conv_cost(dev, B, C, Kc, h, w):
    from spe_amd import kernels as K
    x = torch.randn(B, h * w, C, device=dev)
    W = torch.randn(Kc, C, 3, 3, device=dev) * 0.05
    b = torch.randn(Kc, device=dev)
    dl = torch.randn(B, Kc, device=dev)
    f = timed(lambda: K.conv_head_fwd(x, W, b, h, w))
    g = timed(lambda: K.conv_head_bwd(x, W, None, dl, h, w))
    return f, g


def pmean_cost(dev, B, H, N, dh):
    from spe_amd import kernels as K
    C = H * dh
    qkv = torch.randn(B, N, 3 * C, device=dev)
    Wl = torch.eye(H, device=dev) + 0.3 * torch.randn(H, H, device=dev)
    bl = 0.1 * torch.randn(H, device=dev)
    q, k = qkv.view(B, N, 3, H, dh)[:, :, 0], qkv.view(B, N, 3, H, dh)[:, :, 1]
    Qf, Kf = K.attn_pack_multi([(q, dh ** -0.5 * K.LOG2E, 32 + K.F16), (k, 1.0, 32 + K.F16)])
    _, _, c0 = K.talking_row_constants(Qf, Kf, Wl, bl, B, H, N, dh)
    M = torch.zeros(B, N, N, device=dev)
    return timed(lambda: K.attn_pmean(Qf, Kf, Wl, c0, M, 1.0 / H, B, H, N, dh))


def step_cost(dev, backbone):
    import bench
    from spe_amd.models import build_model
    from spe_amd.util.misc import NestedTensor
    args = bench.model_args(backbone=backbone, enc_layers=3, dec_layers=6, num_queries=300, dataset="voc", layer_to_det=24, dropout=0.0)
    args.focal_gamma = 0.5
    torch.manual_seed(0)
    model, crit, crit_r, pp, rpp = build_model(args)
    model.to(dev).train(); crit.to(dev).train(); crit_r.to(dev).train()
    imgs, mask, tg = bench.synth_batch(5, dev, batch=1, H=512, W=512, K=20, n_tgt=4)
    samples = NestedTensor(imgs, mask)

    def step():
        model.zero_grad(set_to_none=True)
        out = model(samples)
        l0 = crit(out[0], tg)
        with torch.no_grad():
            ps = bench.pseudo_labels(rpp, out[0], tg)
        l1 = crit_r(out[1], ps)
        bench.weighted_total(l0, l1, crit.weight_dict).backward()
    return timed(step, reps=3, windows=5, warm=2)


def main():
    from spe_amd import kernels as K
    dev = torch.device("cuda:0")
    K.set_precision("bf16s")
    lines = ["# woct0head backbones: measured cost on one MI355X (tools/woct0_cost.py; CUDA events, median of 5 windows)"]
    for shp in ((1, 192, 20, 32, 32), (2, 192, 20, 50, 83), (2, 384, 90, 50, 83)):
        f, g = conv_cost(dev, *shp)
        lines.append(f"conv head (B, C, K, h x w) = {shp[:3]} {shp[3]}x{shp[4]}: forward {f:.1f} us, backward (dx + dW + db) {g:.1f} us")
    for shp in ((1, 4, 1024, 48), (2, 4, 1024, 48), (2, 4, 4150, 48), (2, 8, 4150, 48)):
        t = pmean_cost(dev, *shp)
        lines.append(f"attention-probability accumulation per block (B, H, N, dh) = {shp}: {t:.1f} us")
    base = step_cost(dev, "TSCAM_cait_XXS36_Two_Branch")
    woct = step_cost(dev, "TSCAM_cait_XXS36_Two_Branch_conv_cls_attn_woct0head")
    lines.append(f"training step, 1 x 512 x 512, script_voc decoder (3 enc / 6 dec, 300 queries, layer_to_det 24), bf16s: "
                 f"TSCAM_cait_XXS36_Two_Branch {base / 1000:.2f} ms, ..._conv_cls_attn_woct0head {woct / 1000:.2f} ms ({(woct / base - 1) * 100:+.1f} %)")
    text = "\n".join(lines) + "\n"
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
