"""Parity cases of the woct0head TSCAM backbones (reference models/cait.py:834-1332; spe_amd.models.cait._TSCAMConvHead).

Like tests/cfg_cases.py: every case is determined by seeds - `build_case(name)` constructs the product's detector on the CPU, randomises it
with cfg_cases.randomise and returns it with the images and targets.  tools/gen_woct0_golden.py loads that state dict strictly into the
REFERENCE class, runs one iteration there and writes tests/golden/woct0_<case>.pt (data only); tests/test_woct0head_cpu.py and
tests/test_woct0head_gpu.py compare against it.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfg_cases as cc  # noqa: E402

VARIANTS = {"v1": "TSCAM_cait_two_branch_conv_cls_attn_woct0head", "v2": "TSCAM_cait_two_branch_conv_cls_attn_woct0head_v2",
            "v3": "TSCAM_cait_two_branch_conv_cls_attn_woct0head_v3"}

# tiny: C = 32, 4 heads, depth 4, detection branch from block 3, two images (the second padded); n1024: the launch scripts' token count
# (512 x 512 -> N = 1024) at XXS widths (C = 192, 4 heads of 48), 2 blocks - the fused attention kernels and the fused accumulation run there.
_TINY = dict(width=32, depth=4, heads=4, init_scale=1e-5, layer_to_det=3, enc=1, dec=2, Q=10, dataset="voc", K=20, img_size=64,
             sizes_hw=[(64, 96), (48, 80)], n_tgt=[3, 2], gamma=0.25)
CASES = {
    "tiny_v1": dict(_TINY, variant="v1", backbone="woct0_tiny_v1", seed=811),
    "tiny_v2": dict(_TINY, variant="v2", backbone="woct0_tiny_v2", seed=812),
    "tiny_v3": dict(_TINY, variant="v3", backbone="woct0_tiny_v3", seed=813),
    "n1024_v1": dict(variant="v1", backbone="woct0_n1024_v1", width=192, depth=2, heads=4, init_scale=1e-5, layer_to_det=1, enc=1, dec=2, Q=20,
                     dataset="voc", K=20, img_size=384, sizes_hw=[(512, 512), (480, 448)], n_tgt=[4, 3], seed=821, gamma=0.25),
}


def register_product_backbones():
    from spe_amd.models import cait
    for c in CASES.values():
        if c["backbone"] in cait._REGISTRY:
            continue

        def fac(pretrained=False, _c=c, **kw):
            cls = getattr(cait, VARIANTS[_c["variant"]])
            return cait._make(cls, _c["width"], _c["depth"], _c["heads"], _c["init_scale"], False, img_size=_c["img_size"], **kw)
        fac.__name__ = c["backbone"]
        cait.register_model(fac)


def make_args(name):
    return cc.make_args(CASES[name])


def build_case(name):
    """-> (args, (model, crit, crit_r, pp, rpp) on the CPU carrying the case's weights, padded images, mask, targets)."""
    from spe_amd.models import build_model
    from spe_amd.util.misc import nested_tensor_from_tensor_list
    c = CASES[name]
    register_product_backbones()
    args = make_args(name)
    torch.manual_seed(c["seed"])
    model, crit, crit_r, pp, rpp = build_model(args)
    g = torch.Generator().manual_seed(c["seed"] + 1)
    cc.randomise(model, g, c["gamma"])
    imgs = [torch.randn(3, h, w, generator=g) for h, w in c["sizes_hw"]]
    nt = nested_tensor_from_tensor_list(imgs)
    targets = cc.make_targets(g, c["K"], c["n_tgt"], c["sizes_hw"])
    return args, (model, crit, crit_r, pp, rpp), nt.tensors, nt.mask, targets
