"""Host logic of the COCO training loop (spe_amd.engine.train_one_epoch_refine_coco): its epoch curriculum against the restated lines
of the reference (engine.py:573-581), on the weight dict a built model really has."""
import argparse
import copy
import os
import time

import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _reference_lines(weight_dict, epoch, header):
    """engine.py:573-581, restated: `header` there is the log header of the epoch, not the 'ref' prefix."""
    if epoch < 1:
        for k in weight_dict:
            if not 'img_label' in k:
                weight_dict[k] = 0.0

    if epoch < 1:
        for k in weight_dict:
            if header in k:
                weight_dict[k] = 0.0
    return weight_dict


def test_apply_curriculum_coco_matches_the_reference_lines():
    from spe_amd import engine
    from spe_amd.models import build_model
    blob = torch.load(os.path.join(GOLD, "e2e_single.pt"), weights_only=False)
    args = argparse.Namespace(**blob["args"])
    args.device, args.num_refines = "cpu", 1
    criterion = build_model(args)[1]
    full = engine.get_refine_weight_dict(copy.deepcopy(criterion.weight_dict), args.num_refines, header=engine.RF_HEADER)
    assert any("img_label" in k for k in full) and any(k.startswith("ref_1_") and "img_label" not in k for k in full)
    assert all(w != 0.0 for w in full.values())
    for epoch in (0, 1, 7):
        header = f"[{time.strftime('%Y-%m-%d-%H:%M:%S', time.localtime())}] => Epoch: [{epoch}]"
        want = _reference_lines(dict(full), epoch, header)
        got = dict(full)
        assert engine.apply_curriculum_coco(got, epoch) is got
        assert got == want and list(got) == list(full), epoch
        assert engine.apply_curriculum_coco(dict(got), epoch) == want                       # applied every step: idempotent
        if epoch < 1:
            assert {k for k, w in got.items() if w != 0.0} == {k for k in full if "img_label" in k}
        else:
            assert got == full
    assert engine.train_one_epoch_refine_coco.__code__.co_varnames[:10] == engine.train_one_epoch_refine.__code__.co_varnames[:10]
