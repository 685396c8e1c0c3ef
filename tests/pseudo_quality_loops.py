"""The refine training loop on the stub of tests/train_targets_cases.py with a PseudoLabelMeter: batches whose host targets carry the
loader's ground-truth rows, criteria that keep the rows they were given, and the restatement's counters for what they kept."""
import numpy as np
import torch

import pseudo_quality_ref as R
import train_targets_cases as T

STAGES = ["cam"] + [f"rf_{k}" for k in range(1, T.STUB_STAGES)]
NUM_CLASSES = T.STUB_KC + 1                            # the stub's logits: labels 1 .. STUB_KC, 0 unused


def gt_batches(steps=3, seed=9):
    """T.stub_batches with 'boxes' / 'labels' in every host target: one to four large ground-truth rows per image, labels 1 .. STUB_KC
    and now and then STUB_KC + 1 = C (dropped); image 0 of the last batch has none."""
    g = torch.Generator().manual_seed(seed)
    batches = T.stub_batches(steps)
    for s, (_, targets) in enumerate(batches):
        for b, t in enumerate(targets):
            n = 0 if (s == steps - 1 and b == 0) else int(torch.randint(1, 5, (1,), generator=g))
            t["boxes"] = torch.cat([0.3 + 0.4 * torch.rand(n, 2, generator=g), 0.4 + 0.5 * torch.rand(n, 2, generator=g)], dim=1)
            t["labels"] = torch.randint(1, T.STUB_KC + 2, (n,), generator=g)
    return batches


class KeepingCriterion(T.StubCriterion):
    """StubCriterion that also keeps the rows of every call, as host arrays."""

    def __init__(self):
        super().__init__()
        self.rows = []

    def __call__(self, outputs, targets):
        self.rows.append([{k: t[k].detach().cpu().numpy().copy() for k in ("boxes", "labels", "scores") if k in t} for t in targets])
        return super().__call__(outputs, targets)


def run_epochs(device, meter_factory=None, epochs=2, steps=3, lr=0.05):
    """`epochs` of engine.train_one_epoch_refine over gt_batches; meter_factory: None or a callable giving the epoch's meter.  lr = 0:
    the parameters stay, so the rows of every step are the same on any device.
    -> (stats of the last epoch, the parameters, the last meter, the two criteria, the batches)."""
    from spe_amd import engine
    from spe_amd.models.conditional_detr import PostProcessRefine
    batches = gt_batches(steps)
    model = T.StubModel(batches).to(device)
    crit, crit_r = KeepingCriterion(), KeepingCriterion()
    opt = torch.optim.SGD(model.parameters(), lr=lr)
    meter = None
    for e in range(epochs):
        kw = {}
        if meter_factory is not None:
            meter = meter_factory()
            kw["pseudo_meter"] = meter
        stats = engine.train_one_epoch_refine(model, crit, T.stub_loader(batches), opt, device, T.STUB_EPOCH + e, 0.1, T.stub_args(),
                                              {"bbox": PostProcessRefine()}, crit_r, **kw)
    return stats, model.p.detach().cpu().clone(), meter, crit, crit_r, batches


def expected_counters(crit, crit_r, batches, epochs=2, thr=0.5):
    """The restatement over what the criteria were given in the LAST epoch -> int64 [stages, 10, C + 1]."""
    steps, nrf = len(batches), T.STUB_STAGES - 1
    out = np.zeros((len(STAGES), 10, NUM_CLASSES + 1), np.int64)
    for s in range(steps):
        gts = batches[s][1]
        calls = [crit.rows[(epochs - 1) * steps + s]] + [crit_r.rows[((epochs - 1) * steps + s) * nrf + k] for k in range(nrf)]
        for stage, rows in enumerate(calls):
            for p, t in zip(rows, gts):
                R.image(p["boxes"], p["labels"], p.get("scores"), t["boxes"].numpy(), t["labels"].numpy(), NUM_CLASSES, thr, out[stage])
    return out
