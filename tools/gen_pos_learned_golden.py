"""Golden vectors of the REFERENCE with --position_embedding learned (reference models/position_encoding.py:60-85; case table:
tests/pos_learned_cases.py).

    python tools/gen_pos_learned_golden.py [case ...]        # needs the reference checkout (tools/ref_harness.py)

For every case the product's seeded and randomised detector state dict - the two position tables drawn with randn - is loaded, strict=True, into
the reference's ConditionalDETR_Refine; one iteration runs there: forward, SetCriterion, PostProcessRefine pseudo labels, SetCriterionRefine,
weighted total and backward (all drop rates 0; criteria in eval mode = no jitter).  tests/golden/pos_learned_<case>.pt receives data only:
outputs, loss keys, pseudo labels, every parameter gradient as (norm, 64 samples), the reference's parameter names and shapes, the Hungarian
assignments of both criteria (one list of per-image index pairs per matcher call: the main output, then every auxiliary one), a checksum of the
weights (rebuilt from the seed, never stored) and - for the tiny case - the raw `pos` tensor the reference's embedding module returned.
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
import pos_learned_cases as pc  # noqa: E402
import ref_harness as rh  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
KEEP_POS = ("tiny",)


def register_reference_backbones():
    rh.install_shims()
    from functools import partial
    import models.cait as rc
    from timm.models.registry import register_model
    from torch import nn
    for c in pc.CASES.values():
        def fac(pretrained=False, _c=c, **kwargs):
            m = rc.TSCAM_cait(img_size=384, patch_size=16, embed_dim=_c["width"], depth=_c["depth"], num_heads=_c["heads"], mlp_ratio=4,
                              qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), init_scale=_c["init_scale"], depth_token_only=2,
                              **kwargs)
            return m, _c["width"]
        fac.__name__ = c["backbone"]
        register_model(fac)


def record_matcher(crit):
    """-> the list that receives, per matcher call, the per-image (query, target) index pairs"""
    inner, calls = crit.matcher.forward, []

    def fwd(outputs, tg):
        res = inner(outputs, tg)
        calls.append([(i.clone(), j.clone()) for i, j in res])
        return res
    crit.matcher.forward = fwd
    return calls


def run_case(name):
    from models import build_model as ref_build
    import util.misc as um
    torch.use_deterministic_algorithms(True)
    args, (pmodel, *_), tensors, mask, targets = pc.build_case(name)
    sd = {k: v.detach().clone() for k, v in pmodel.state_dict().items()}
    del pmodel
    with contextlib.redirect_stdout(io.StringIO()):
        model, crit, crit_r, pp, rpp = ref_build(copy.deepcopy(args))
    model.load_state_dict(sd, strict=True)                   # identical keys and shapes: the boundary contract
    model.train(); crit.eval(); crit_r.eval()
    idx0, idx1 = record_matcher(crit), record_matcher(crit_r)
    seen = []
    hook = model.backbone[1].register_forward_hook(lambda m, i, o: seen.append(o.detach().clone()))
    out = model(um.NestedTensor(tensors, mask))
    hook.remove()
    l0 = crit(out[0], targets)
    orig = torch.stack([t["orig_size"] for t in targets])
    with torch.no_grad():
        pr = rpp["bbox"](out[0], orig, targets)
        pseudo = []
        for t, r in zip(targets, pr):
            p = copy.deepcopy(t)
            p.update({"labels": r["labels"].clone(), "boxes": r["boxes"].clone(), "scores": r["scores"].clone()})
            pseudo.append(p)
    # conditioning of the case (as tools/gen_config_golden.py): the relative top-2 gap over the queries behind every pseudo label
    prob = out[0]["pred_logits"].detach().sigmoid()
    margins = [[float((lambda top: (top[0] - top[1]) / top[0])(prob[b, :, c_].topk(2).values)) for c_ in torch.unique(t["labels"]).tolist()]
               for b, t in enumerate(targets)]
    l1 = crit_r(out[1], pseudo)
    wd = crit.weight_dict
    total = sum(l0[k] * wd[k] for k in l0 if k in wd) + sum(l1[k] * wd[k] for k in l1 if k in wd)
    total.backward()
    grads = {n: (cc.sample(p.grad) if p.grad is not None else None) for n, p in model.named_parameters()}
    assert len(seen) == 1 and all(grads[k] is not None and grads[k][0] > 0 for k in pc.TABLES)
    blob = {"case": name, "dims": pc.CASES[name], "out0": gcg.out_record(out[0]), "out1": gcg.out_record(out[1]),
            "loss0": {k: v.detach().clone() for k, v in l0.items()}, "loss1": {k: v.detach().clone() for k, v in l1.items()},
            "pseudo": pseudo, "pseudo_margins": margins, "total": total.detach().clone(), "grads": grads, "weight_dict": dict(wd),
            "indices0": idx0, "indices1": idx1,
            "param_shapes": {k: tuple(v.shape) for k, v in model.state_dict().items()},
            "sd_checksum": float(sum(v.double().abs().sum() for v in sd.values() if v.is_floating_point()))}
    if name in KEEP_POS:
        blob["pos"] = seen[0]
    path = os.path.join(OUT, f"pos_learned_{name}.pt")
    torch.save(blob, path)
    print(name, "total", float(total.detach()), "pos", tuple(seen[0].shape), "matcher calls", len(idx0), len(idx1), "min pseudo margin", min(min(m) for m in margins), "bytes", os.path.getsize(path))


def main():
    register_reference_backbones()
    for n in sys.argv[1:] or list(pc.CASES):
        run_case(n)


if __name__ == "__main__":
    main()
