"""Parity cases of the learned position embedding (reference models/position_encoding.py:60-85, --position_embedding learned / v3;
spe_amd.models.position_encoding.PositionEmbeddingLearned).

Like tests/woct0_cases.py: every case is determined by seeds - `build_case(name)` constructs the product's detector on the CPU with the args of
cfg_cases.make_args and position_embedding = "learned" set afterwards, randomises it with cfg_cases.randomise and draws the two tables from the
same generator (randn: a row / column or channel-order mix-up cannot hide behind the reference's uniform [0, 1) initialisation).
tools/gen_pos_learned_golden.py loads that state dict strictly into the REFERENCE, runs one iteration there and writes
tests/golden/pos_learned_<case>.pt (data only); tests/test_pos_learned_cpu.py and tests/test_pos_learned_gpu.py compare against it.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfg_cases as cc  # noqa: E402

TABLES = ("backbone.1.row_embed.weight", "backbone.1.col_embed.weight")

# Two images each, the second padded.
# tiny : a 4 x 6 grid (h != w), NO encoder layer: pos is consumed by the decoder's small-row path alone.
# n1024: the launch scripts' 32 x 32 grid (S = 1024 >= the row bound of ops.memory_side_kv_ok), one encoder layer: the fp16 fragment path of
#        the decoder's memory side and the flash encoder both send a gradient into pos.
CASES = {
    "tiny": dict(backbone="pos_learned_tiny", width=32, depth=4, heads=4, init_scale=1e-5, layer_to_det=3, enc=0, dec=2, Q=10, dataset="voc",
                 K=20, sizes_hw=[(64, 96), (48, 80)], n_tgt=[3, 2], seed=911, gamma=0.25),
    "n1024": dict(backbone="pos_learned_n1024", width=192, depth=2, heads=4, init_scale=1e-5, layer_to_det=1, enc=1, dec=2, Q=20,
                  dataset="voc", K=20, sizes_hw=[(512, 512), (480, 448)], n_tgt=[4, 3], seed=921, gamma=0.25),
}


def register_product_backbones():
    from spe_amd.models import cait
    for c in CASES.values():
        if c["backbone"] in cait._REGISTRY:
            continue

        def fac(pretrained=False, _c=c, **kw):
            return cait._make(cait.TSCAM_cait, _c["width"], _c["depth"], _c["heads"], _c["init_scale"], False, **kw)
        fac.__name__ = c["backbone"]
        cait.register_model(fac)


def make_args(name, position_embedding="learned"):
    args = cc.make_args(CASES[name])
    args.position_embedding = position_embedding
    return args


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
    sd = model.state_dict()
    with torch.no_grad():
        for k in TABLES:
            sd[k].copy_(torch.randn(sd[k].shape, generator=g))
    imgs = [torch.randn(3, h, w, generator=g) for h, w in c["sizes_hw"]]
    nt = nested_tensor_from_tensor_list(imgs)
    targets = cc.make_targets(g, c["K"], c["n_tgt"], c["sizes_hw"])
    return args, (model, crit, crit_r, pp, rpp), nt.tensors, nt.mask, targets
