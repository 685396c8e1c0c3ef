"""The training and evaluation loops with a ProposalRecallMeter: the stub model of tests/train_targets_cases.py with the ground-truth rows
of tests/pseudo_quality_loops.py, recording what it returned, and the canned VOC run of tests/detect_loops.py - plus a meter fed by hand
with what the loops saw."""
import torch

import detect_loops as D
import pseudo_quality_loops as L
import train_targets_cases as T

STAGES = [f"s{k}" for k in range(T.STUB_STAGES)]
NUM_CLASSES = T.STUB_KC + 1                            # the stub's logit columns; the loader's label STUB_KC + 1 is dropped
KS = (1, 5, 70, 75)                                    # 1, Q = STUB_Q and Q + 5
THRESHS = (0.25, 0.5)


def meter_factory():
    from spe_amd.evalmetrics import ProposalRecallMeter
    return ProposalRecallMeter(NUM_CLASSES, STAGES, iou_threshs=THRESHS, ks=KS)


class RecordingModel(T.StubModel):
    """StubModel that keeps every output it returned: per call {stage: {'pred_logits', 'pred_boxes'}}, detached, on the device."""

    def __init__(self, batches):
        super().__init__(batches)
        self.recorded = []

    def forward(self, samples):
        out = super().forward(samples)
        self.recorded.append({k: {n: v[n].detach().clone() for n in ("pred_logits", "pred_boxes")} for k, v in out.items()})
        return out


def run_epochs(device, proposal=None, pseudo=None, epochs=2, steps=3, lr=0.05):
    """`epochs` of engine.train_one_epoch_refine over L.gt_batches; proposal / pseudo: None or a callable giving the epoch's meter.
    -> (stats of the last epoch, the parameters, the last proposal meter, what the model returned, the batches)."""
    from spe_amd import engine
    from spe_amd.models.conditional_detr import PostProcessRefine
    batches = L.gt_batches(steps)
    model = RecordingModel(batches).to(device)
    crit, crit_r = T.StubCriterion(), T.StubCriterion()
    opt = torch.optim.SGD(model.parameters(), lr=lr)
    meter = None
    for e in range(epochs):
        kw = {}
        if proposal is not None:
            meter = kw["proposal_meter"] = proposal()
        if pseudo is not None:
            kw["pseudo_meter"] = pseudo()
        stats = engine.train_one_epoch_refine(model, crit, T.stub_loader(batches), opt, device, T.STUB_EPOCH + e, 0.1, T.stub_args(),
                                              {"bbox": PostProcessRefine()}, crit_r, **kw)
    return stats, model.p.detach().cpu().clone(), meter, model.recorded, batches


def fed_by_hand(meter, updates):
    """updates: (stage, outputs, gts) - feeds a CPU meter's state through the host composition with the probabilities computed WHERE the
    outputs lie: a device's sigmoid and the host's need not round alike, and an order is only comparable over the same values."""
    from spe_amd import evalmetrics
    state = meter._state(torch.device("cpu"))
    for stage, outputs, gts in updates:
        prob = outputs["pred_logits"].float().sigmoid().cpu()
        goff = [0]
        for t in gts:
            goff.append(goff[-1] + t["labels"].shape[0])
        evalmetrics._proposal_recall_host(prob, outputs["pred_boxes"].float().cpu(), torch.cat([t["boxes"].float().cpu() for t in gts]).reshape(-1, 4),
                                          torch.cat([t["labels"].long().cpu() for t in gts]), goff, meter.num_classes, meter._thr, meter._ks,
                                          state[meter.stages.index(stage)])
    return meter


def last_epoch_updates(recorded, batches, epochs=2):
    steps = len(batches)
    for s in range(steps):
        for k, out in recorded[(epochs - 1) * steps + s].items():
            yield f"s{k}", out, batches[s][1]


def stat_keys():
    return [f"prop_{s}_{n}" for s in STAGES for n in [f"recall_at_{k}" for k in KS] + ["ceiling", "mean_best_iou"]]


# ---- evaluate_det_voc ----------------------------------------------------------------------------------------------------------------
def voc_updates(images, canned, batch, flip, device):
    """What the evaluation loop gives the meter: the (flip-merged) canned outputs and base_ds's rows, divided by the frame, as cxcywh."""
    from spe_amd.util.box_ops import box_xyxy_to_cxcywh
    scale = torch.tensor([D.FRAME, D.FRAME]).to(torch.float32).repeat(2)
    for i, out in zip(range(0, len(images), batch), canned):
        out = D.flip_merged(out) if flip else out
        gts = [{"boxes": box_xyxy_to_cxcywh(torch.as_tensor(im["gt_boxes"]).to(torch.float32).reshape(-1, 4) / scale),
                "labels": torch.as_tensor(im["gt_labels"]).to(torch.int64).reshape(-1)} for im in images[i:i + batch]]
        yield "det", {k: v.to(device) for k, v in out.items()}, gts
