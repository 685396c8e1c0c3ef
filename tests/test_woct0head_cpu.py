"""The woct0head TSCAM backbones on the CPU (construction only, no kernel runs): the four factories the reference's --backbone flag reaches
are registered, and every woct0head model has exactly the reference's parameter names and shapes (tests/golden/woct0_*.pt, written by
tools/gen_woct0_golden.py from the reference classes) and strict-loads them."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import woct0_cases as wc  # noqa: E402

GOLD = os.path.join(HERE, "golden")
FACTORIES = ["TSCAM_cait_XXS36_Two_Branch_conv_cls_attn_woct0head", "TSCAM_cait_XXS36_Two_Branch_conv_cls_attn_woct0head_v2",
             "TSCAM_cait_XXS36_Two_Branch_conv_cls_attn_woct0head_v3", "TSCAM_cait_XXS24_224"]


@pytest.mark.parametrize("name", FACTORIES)
def test_factory_is_registered(name):
    from spe_amd.models.cait import create_model
    model, C = create_model(name, num_classes=20, layer_to_det=35 if "XXS36" in name else 23)
    assert C == 192
    sd = model.state_dict()
    assert sd["patch_embed.proj.weight"].shape == (192, 3, 16, 16)
    if "woct0head" in name:
        K1 = 21 if name.endswith("woct0head") else 20
        assert sd["extra_cls_token"].shape == (1, K1, 192)
        assert sd["conv_head.weight"].shape == (20, 192, 3, 3) and sd["conv_head.bias"].shape == (20,)
        assert "cls_head_multi_cls.weight" not in sd
        assert len(model.blocks) == 36 and len(model.blocks_det) == 1
    else:
        assert sd["pos_embed"].shape == (1, 14 * 14, 192) and len(model.blocks) == 24


@pytest.mark.parametrize("case", sorted(wc.CASES))
def test_parameter_names_and_shapes_match_reference(case):
    from spe_amd.models import build_model
    blob = torch.load(os.path.join(GOLD, f"woct0_{case}.pt"), weights_only=False)
    wc.register_product_backbones()
    model = build_model(wc.make_args(case))[0]
    own = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert own == blob["param_shapes"], set(own.items()) ^ set(blob["param_shapes"].items())
    model.load_state_dict({k: torch.zeros(s) for k, s in blob["param_shapes"].items()}, strict=True)
    q = model.backbone[0].body.blocks_token_only[0].attn.num_queries
    assert q == (20 if wc.CASES[case]["variant"] == "v2" else 21)


@pytest.mark.parametrize("case", sorted(wc.CASES))
def test_seeded_weights_match_fixture(case):
    _, (model, *_), *_ = wc.build_case(case)
    blob = torch.load(os.path.join(GOLD, f"woct0_{case}.pt"), weights_only=False)
    chk = float(sum(v.detach().double().abs().sum() for v in model.state_dict().values() if v.is_floating_point()))
    assert abs(chk - blob["sd_checksum"]) <= 1e-9 * blob["sd_checksum"]
