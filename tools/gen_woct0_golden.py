"""Golden vectors of the REFERENCE's woct0head backbones (reference models/cait.py:834-1332; case table: tests/woct0_cases.py).

    python tools/gen_woct0_golden.py [case ...]        # needs the reference checkout (tools/ref_harness.py)

For every case the product's seeded and randomised detector state dict is loaded - strict=True - into the reference's ConditionalDETR_Refine
built around the reference class of the case's variant; one iteration runs there: forward, SetCriterion, PostProcessRefine pseudo labels,
SetCriterionRefine, weighted total and backward (all drop rates 0, so the train-mode forward is the eval-mode one; criteria in eval mode = no
jitter).  tests/golden/woct0_<case>.pt receives data only: outputs (cams_cls_patch included), loss keys, pseudo labels, every parameter
gradient as (norm, 64 samples), the reference's parameter names and shapes, and a checksum of the weights (rebuilt from the seed, never
stored).
"""
import contextlib
import copy
import io
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfg_cases as cc  # noqa: E402
import gen_config_golden as gcg  # noqa: E402
import ref_harness as rh  # noqa: E402
import woct0_cases as wc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def register_reference_backbones():
    rh.install_shims()
    from functools import partial
    import models.cait as rc
    from timm.models.registry import register_model
    from torch import nn
    for c in wc.CASES.values():
        def fac(pretrained=False, _c=c, **kwargs):
            cls = getattr(rc, wc.VARIANTS[_c["variant"]])
            m = cls(img_size=_c["img_size"], patch_size=16, embed_dim=_c["width"], depth=_c["depth"], num_heads=_c["heads"], mlp_ratio=4,
                    qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), init_scale=_c["init_scale"], depth_token_only=2, **kwargs)
            return m, _c["width"]
        fac.__name__ = c["backbone"]
        register_model(fac)


def out_record(o):
    r = gcg.out_record({k: v for k, v in o.items() if k != "cams_cls_patch"})
    if "cams_cls_patch" in o:
        r["cams_cls_patch"] = gcg.keep(o["cams_cls_patch"])
    return r


def run_case(name):
    from models import build_model as ref_build
    import util.misc as um
    torch.use_deterministic_algorithms(True)
    args, (pmodel, *_), tensors, mask, targets = wc.build_case(name)
    sd = {k: v.detach().clone() for k, v in pmodel.state_dict().items()}
    del pmodel
    with contextlib.redirect_stdout(io.StringIO()):
        model, crit, crit_r, pp, rpp = ref_build(copy.deepcopy(args))
    model.load_state_dict(sd, strict=True)                   # identical keys and shapes: the boundary contract
    model.train(); crit.eval(); crit_r.eval()
    out = model(um.NestedTensor(tensors, mask))
    l0 = crit(out[0], targets)
    orig = torch.stack([t["orig_size"] for t in targets])
    with torch.no_grad():
        pr = rpp["bbox"](out[0], orig, targets)
        pseudo = []
        for t, r in zip(targets, pr):
            p = copy.deepcopy(t)
            p.update({"labels": r["labels"].clone(), "boxes": r["boxes"].clone(), "scores": r["scores"].clone()})
            pseudo.append(p)
    l1 = crit_r(out[1], pseudo)
    wd = crit.weight_dict
    total = sum(l0[k] * wd[k] for k in l0 if k in wd) + sum(l1[k] * wd[k] for k in l1 if k in wd)
    total.backward()
    grads = {n: (cc.sample(p.grad) if p.grad is not None else None) for n, p in model.named_parameters()}
    blob = {"case": name, "dims": wc.CASES[name], "out0": out_record(out[0]), "out1": out_record(out[1]),
            "loss0": {k: v.detach().clone() for k, v in l0.items()}, "loss1": {k: v.detach().clone() for k, v in l1.items()},
            "pseudo": pseudo, "total": total.detach().clone(), "grads": grads, "weight_dict": dict(wd),
            "param_shapes": {k: tuple(v.shape) for k, v in model.state_dict().items()},
            "sd_checksum": float(sum(v.double().abs().sum() for v in sd.values() if v.is_floating_point()))}
    path = os.path.join(OUT, f"woct0_{name}.pt")
    torch.save(blob, path)
    print(name, "total", float(total.detach()), "bytes", os.path.getsize(path))


def main():
    register_reference_backbones()
    for n in sys.argv[1:] or list(wc.CASES):
        run_case(n)


if __name__ == "__main__":
    main()
