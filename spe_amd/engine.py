"""The refine training loop as a public entry (reference engine.py:93-174), built from the device-side pieces of this package: CAM
pseudo boxes (spe_amd.camboxes), the refine post-processor for the stage-k+1 targets, both criteria, and the step ledger
(spe_amd.steplog) in place of the reference's per-key loss arithmetic, its `.item()` before the backward and its ~95 `.item()` calls
after the optimizer step.  Signature, log lines and return value are the reference's.

Difference: a weighted total that is not finite stops the run at the next log line or at the end of the epoch
(FloatingPointError from the ledger), not before the optimizer step of that iteration; up to print_freq steps of compute are wasted,
the weights are lost either way (the reference exits without saving)."""
import copy
import time

import torch

from . import camboxes
from .steplog import StepLedger

PRINT_FREQ = 100
RF_HEADER = "ref"


def get_refine_weight_dict(weight_dict, num_refinements, header="rf"):
    """engine.py:260-268: every weight once more under '<header>_<rf>_<key>' per refinement stage (in place, and returned)."""
    base = list(weight_dict.items())
    for rf in range(1, num_refinements + 1):
        for key, w in base:
            weight_dict[f"{header}_{rf}_{key}"] = w
    return weight_dict


def apply_curriculum(weight_dict, epoch, rf_header=RF_HEADER):
    """engine.py:134-142: before epoch 7 only the image-label / drloc keys keep their weight; before epoch 15 the refine keys are 0."""
    if epoch < 7:
        for k in weight_dict:
            if not ("img_label" in k or "drloc" in k):
                weight_dict[k] = 0.0
    if epoch < 15:
        for k in weight_dict:
            if rf_header in k:
                weight_dict[k] = 0.0
    return weight_dict


@torch.no_grad()
def output_to_pseudo_label(outputs, samples, targets, args, postprocessors):
    """engine.py:294-308: the refine post-processor's detections of one stage become the next stage's targets."""
    orig_target_sizes = torch.stack([t["orig_size"] for t in targets], dim=0)
    results = postprocessors["bbox"](outputs, orig_target_sizes, targets)
    pseudo = []
    for t, r in zip(targets, results):
        p = dict(t)
        p.update({"labels": r["labels"].detach(), "boxes": r["boxes"].detach(), "scores": r["scores"].detach()})
        pseudo.append(p)
    return pseudo


@torch.no_grad()
def get_refinements_pseudo_label(outputs, samples, targets, args, postprocessors):
    """engine.py:271-280: {stage k + 1: targets made from stage k}."""
    targets_refine = {}
    for k, v in outputs.items():
        if k == args.num_refines:
            break
        targets_refine[k + 1] = output_to_pseudo_label(v, samples, targets, args, postprocessors)
    return targets_refine


def train_one_epoch_refine(model, criterion, data_loader, optimizer, device, epoch, max_norm=0, args=None, postprocessors=None,
                           criterion_refine=None):
    from .optim import FlatAdamW
    model.train()
    criterion.train()
    criterion_refine.train()
    ledger = StepLedger(windows={"lr": 1, "class_error": 1}, fmts={"lr": "{value:.6f}", "class_error": "{value:.2f}"}, delimiter="  ")
    header = f"[{time.strftime('%Y-%m-%d-%H:%M:%S', time.localtime())}] => Epoch: [{epoch}]"
    weight_dict = get_refine_weight_dict(copy.deepcopy(criterion.weight_dict), args.num_refines, header=RF_HEADER)
    flat = isinstance(optimizer, FlatAdamW)
    if flat:
        optimizer.max_grad_norm = max_norm if max_norm > 0 else None     # the clip rides on the update launch
    for samples, targets in ledger.log_every(data_loader, PRINT_FREQ, header):
        samples = samples.to(device)
        targets = [{k: v.to(device) for k, v in t.items()} for t in targets]
        outputs = model(samples)
        pseudo_label = camboxes.get_pseudo_label_multi_boxes(outputs[0], samples, targets, args)
        for t, p in zip(targets, pseudo_label):
            t.update(p)
        pseudo_label_refine = get_refinements_pseudo_label(outputs, samples, targets, args, postprocessors)
        loss_dict = criterion(outputs[0], targets)
        for rf, out in outputs.items():
            if rf == 0:
                continue
            for k, v in criterion_refine(out, pseudo_label_refine[rf]).items():
                loss_dict[f"{RF_HEADER}_{rf}_{k}"] = v
        apply_curriculum(weight_dict, epoch)

        losses = ledger.record(loss_dict, weight_dict, lr=optimizer.param_groups[0]["lr"])
        optimizer.zero_grad()
        losses.backward()
        if flat:
            optimizer.reducer.finish()
        elif max_norm > 0:
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
        optimizer.step()

    stats = ledger.global_avg()                  # synchronised between the ranks; raises if a step's total was not finite
    print("Averaged stats:", ledger)
    return stats
