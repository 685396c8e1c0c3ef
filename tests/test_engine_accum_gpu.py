"""The public training loops (spe_amd.engine) with gradient accumulation, with the guarded optimizer and with the COCO curriculum,
against the same loops written out by hand on the e2e_single.pt harness (the one of test_steplog_gpu.py, restated here)."""
import argparse
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_NORM = 0.1


@pytest.fixture(scope="module")
def blob():
    return torch.load(os.path.join(GOLD, "e2e_single.pt"), weights_only=False)


def _to_dev(targets, dev):
    return [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in t.items()} for t in targets]


def _setup(blob, dev, accum_steps=1, guarded=False):
    from spe_amd import kernels as Kn
    from spe_amd.dp import GradAllReducer
    from spe_amd.models import build_model
    from spe_amd.optim import FlatAdamW
    torch.manual_seed(11)
    Kn.manual_seed(11)
    args = argparse.Namespace(**blob["args"])
    args.device, args.num_classes, args.cam_thr, args.multi_box_ratio = "cuda", 20, 0.2, 0.5
    model, crit, crit_r, pp, rpp = build_model(args)
    model.load_state_dict(blob["state_dict"], strict=True)
    model, crit, crit_r = model.to(dev), crit.to(dev), crit_r.to(dev)
    named_p = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    groups = [{"params": [p for n, p in named_p if "backbone" not in n], "lr": 2e-3},
              {"params": [p for n, p in named_p if "backbone" in n], "lr": 5e-4}]
    red = GradAllReducer([p for _, p in named_p], bucket_bytes=1 << 16, flatten_params=True, accum_steps=accum_steps)
    kw = {"skip_nonfinite": True} if guarded else {}
    opt = FlatAdamW(groups, red, weight_decay=1e-2, max_grad_norm=MAX_NORM, **kw)
    return args, model, crit, crit_r, rpp, opt, red, named_p


def _loader(blob, n=4):
    from spe_amd.util.misc import NestedTensor
    g = torch.Generator().manual_seed(3)
    return [(NestedTensor(blob["tensors"] + 0.1 * i * torch.randn(blob["tensors"].shape, generator=g), blob["mask"]),
             [dict(t) for t in blob["targets"]]) for i in range(n)]


def _weighted_total(loss_dict, wd, dev):
    terms = [loss_dict[k] for k in loss_dict if k in wd]                 # bench.py's weighted_total: one stack, one product, one sum
    w = torch.tensor([float(wd[k]) for k in loss_dict if k in wd], dtype=torch.float32).to(dev)
    return (torch.stack(terms) * w).sum()


def _public(blob, dev, loader, epoch, accum_steps=1, guarded=False, loop="train_one_epoch_refine", wrap=None):
    """The public loop -> (parameters, optimizer, reducer); the reducer's hooks are removed, its counters stay readable."""
    from spe_amd import engine
    args, model, crit, crit_r, rpp, opt, red, named_p = _setup(blob, dev, accum_steps, guarded)
    if wrap is not None:
        wrap(red)
    getattr(engine, loop)(model, crit, loader, opt, dev, epoch, MAX_NORM, args, rpp, crit_r)
    red.remove()
    return {n: p.detach().clone() for n, p in named_p}, opt, red


def _by_hand(blob, dev, loader, epoch, accum_steps=1, curriculum="apply_curriculum"):
    """The same components in a hand-written cycle loop: the update follows the backward that completes a cycle."""
    from spe_amd import camboxes, engine
    args, model, crit, crit_r, rpp, opt, red, named_p = _setup(blob, dev, accum_steps)
    model.train(); crit.train(); crit_r.train()
    wd = engine.get_refine_weight_dict(dict(crit.weight_dict), args.num_refines, header="ref")
    updates = 0
    for i, (samples, targets) in enumerate(loader):
        samples, targets = samples.to(dev), _to_dev(targets, dev)
        outputs = model(samples)
        for t, p in zip(targets, camboxes.get_pseudo_label_multi_boxes(outputs[0], samples, targets, args)):
            t.update(p)
        pseudo = engine.get_refinements_pseudo_label(outputs, samples, targets, args, rpp)
        loss_dict = crit(outputs[0], targets)
        for k, v in crit_r(outputs[1], pseudo[1]).items():
            loss_dict[f"ref_1_{k}"] = v
        getattr(engine, curriculum)(wd, epoch)
        total = _weighted_total(loss_dict, wd, dev)
        opt.zero_grad()
        total.backward()
        red.finish()
        if (i + 1) % accum_steps == 0:
            opt.step()
            updates += 1
    red.remove()
    return {n: p.detach().clone() for n, p in named_p}, updates, wd


def _same(a, b):
    bad = [n for n in a if not torch.equal(a[n], b[n])]
    assert not bad, (bad[:10], len(bad))


def test_accumulating_loop_equals_the_cycle_loop_by_hand(dev, blob, capsys):
    got, opt, red = _public(blob, dev, _loader(blob), 15, accum_steps=2)
    out = capsys.readouterr().out
    want, updates, _ = _by_hand(blob, dev, _loader(blob), 15, accum_steps=2)
    assert updates == 2 and opt._step == 2 and red.micro == 0
    _same(got, want)
    one, _, _ = _by_hand(blob, dev, _loader(blob, 2), 15, accum_steps=2)
    assert any(not torch.equal(got[n], one[n]) for n in got)              # the second update moved something
    assert "Dropped" not in out and "skipped" not in out


def test_leftover_micro_batch_is_dropped(dev, blob, capsys):
    """Three batches at accum_steps = 2: one update, the third batch's gradient is dropped with one line.  Without the accumulating
    loop the first iteration raises RuntimeError (FlatAdamW.step() inside an accumulation cycle)."""
    got, opt, red = _public(blob, dev, _loader(blob, 3), 15, accum_steps=2)
    lines = capsys.readouterr().out.splitlines()
    want, updates, _ = _by_hand(blob, dev, _loader(blob, 2), 15, accum_steps=2)
    assert updates == 1 and opt._step == 1 and red.micro == 0
    _same(got, want)
    drop = [l for l in lines if l.startswith("Dropped")]
    assert len(drop) == 1 and "1 micro-batch" in drop[0]
    assert lines[-1].startswith("Averaged stats: ") and lines.index(drop[0]) == len(lines) - 2


def test_guarded_loop_survives_a_poisoned_bucket(dev, blob, capsys):
    calls = []

    def wrap(red):
        finish = red.finish

        def poisoned_finish():
            finish()
            calls.append(1)
            if len(calls) == 2:                              # the second iteration's reduced gradient
                red.buckets[0]["flat"][3] = float("inf")
        red.finish = poisoned_finish
    got, opt, red = _public(blob, dev, _loader(blob), 15, guarded=True, wrap=wrap)
    lines = capsys.readouterr().out.splitlines()
    assert len(calls) == 4
    assert all(bool(torch.isfinite(p).all()) for p in got.values())
    assert (opt.applied_steps(), opt.skipped_steps(), opt.first_skipped()) == (3, 1, 2)
    told = [l for l in lines if "skipped" in l]
    assert len(told) == 1 and "1 so far" in told[0] and "step 2" in told[0]
    assert lines[-1].startswith("Averaged stats: ")


@pytest.mark.parametrize("epoch", [0, 1])
def test_coco_loop_equals_the_loop_with_its_curriculum_by_hand(dev, blob, epoch):
    got, opt, _ = _public(blob, dev, _loader(blob, 2), epoch, loop="train_one_epoch_refine_coco")
    want, updates, wd = _by_hand(blob, dev, _loader(blob, 2), epoch, curriculum="apply_curriculum_coco")
    assert updates == 2 and opt._step == 2
    _same(got, want)
    nonzero = {k for k, w in wd.items() if w != 0.0}
    assert nonzero and (all("img_label" in k for k in nonzero) if epoch < 1 else any("ref" in k for k in nonzero))
