"""Measured cost of the learned position embedding (csrc/pos_learned.hip) -> profiles/pos_learned.txt.

    python tools/pos_learned_cost.py [out.txt]

  - spe_pos_learned_fwd, spe_pos_learned_bwd and, beside them, spe_pos_sine at (B, h, w, d) = 2 x 32 x 32 x 384 and 2 x 50 x 50 x 384;
  - one training step (forward, both criteria, backward; no optimiser) of the n1024 case of tests/pos_learned_cases.py with
    position_embedding = sine and = learned, alternating.
Timings: CUDA events around N back-to-back repetitions after warm-up, median of 5 such windows.
"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from woct0_cost import timed  # noqa: E402


def kernel_cost(dev, B, h, w, npf):
    from spe_amd import kernels as K
    col, row = torch.randn(50, npf, device=dev), torch.randn(50, npf, device=dev)
    g = torch.randn(B, h * w, 2 * npf, device=dev)
    dc, dr = torch.empty(50, npf, device=dev), torch.empty(50, npf, device=dev)
    mask = torch.zeros(B, h, w, dtype=torch.bool, device=dev)
    k = torch.arange(npf, dtype=torch.float32, device=dev)
    dim_t = 10000 ** (2 * torch.div(k, 2, rounding_mode="floor") / npf)
    f = timed(lambda: K.pos_learned_fwd(col, row, B, h, w), reps=50)
    b = timed(lambda: K.pos_learned_bwd(g, B, h, w, npf, dcol_out=dc, drow_out=dr), reps=50)
    s = timed(lambda: K.pos_sine(mask, dim_t, npf, 2 * math.pi, 1e-6, True), reps=50)
    return f, b, s


def step_cost(dev, position_embedding):
    import pos_learned_cases as pc
    from spe_amd.models import build_model
    from spe_amd.util.misc import NestedTensor, nested_tensor_from_tensor_list
    import cfg_cases as cc
    c = pc.CASES["n1024"]
    pc.register_product_backbones()
    torch.manual_seed(c["seed"])
    model, crit, crit_r, pp, rpp = build_model(pc.make_args("n1024", position_embedding))
    g = torch.Generator().manual_seed(c["seed"] + 1)
    cc.randomise(model, g, c["gamma"])
    nt = nested_tensor_from_tensor_list([torch.randn(3, hh, ww, generator=g) for hh, ww in c["sizes_hw"]])
    targets = cc.make_targets(g, c["K"], c["n_tgt"], c["sizes_hw"])
    model.to(dev).train(); crit.to(dev).eval(); crit_r.to(dev).eval()
    tg = [{k: v.to(dev) for k, v in t.items()} for t in targets]
    samples = NestedTensor(nt.tensors.to(dev), nt.mask.to(dev))
    wd = crit.weight_dict

    def step():
        model.zero_grad(set_to_none=True)
        out = model(samples)
        l0, l1 = crit(out[0], tg), crit_r(out[1], [dict(t, scores=torch.ones_like(t["labels"], dtype=torch.float32)) for t in tg])
        (sum(l0[k] * wd[k] for k in l0 if k in wd) + sum(l1[k] * wd[k] for k in l1 if k in wd)).backward()
    return timed(step, reps=5, windows=5, warm=3)


def main():
    from spe_amd import kernels as K
    dev = torch.device("cuda:0")
    K.set_precision("bf16s")
    lines = ["# learned position embedding: measured cost on one MI355X (tools/pos_learned_cost.py; CUDA events, median of 5 windows of 50 launches)"]
    for shp in ((2, 32, 32, 192), (2, 50, 50, 192)):
        f, b, s = kernel_cost(dev, *shp)
        mb = shp[0] * shp[1] * shp[2] * 2 * shp[3] * 4 / 1e6
        lines.append(f"(B, h, w, d) = {shp[:3]} x {2 * shp[3]} ({mb:.1f} MB): spe_pos_learned_fwd {f:.1f} us, spe_pos_learned_bwd {b:.1f} us, "
                     f"spe_pos_sine {s:.1f} us (mask conversion and output allocation included in all three)")
    # alternating, twice: the first model of a process also pays for code loading and a cold allocator
    runs = [(pe, step_cost(dev, pe)) for pe in ("sine", "learned", "sine", "learned")]
    lines.append("training step, n1024 case (2 x 512 x 512, width 192, depth 2, 1 enc / 2 dec, 20 queries), bf16s, in the order run: "
                 + ", ".join(f"{pe} {t / 1000:.2f} ms" for pe, t in runs))
    text = "\n".join(lines) + "\n"
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
