"""The refine training loops as public entries (reference engine.py:93-174 and its COCO twin :534-613), built from the device-side pieces of this package: CAM
pseudo boxes (spe_amd.camboxes), the refine post-processor for the stage-k+1 targets, both criteria, and the step ledger
(spe_amd.steplog) in place of the reference's per-key loss arithmetic, its `.item()` before the backward and its ~95 `.item()` calls
after the optimizer step.  Signature, log lines and return value are the reference's.

Difference: a weighted total that is not finite stops the run at the next log line or at the end of the epoch
(FloatingPointError from the ledger), not before the optimizer step of that iteration; up to print_freq steps of compute are wasted,
the weights are lost either way (the reference exits without saving).  FlatAdamW(..., skip_nonfinite=True) closes the hole from the
other side: an update whose reduced GRADIENT is not finite is skipped on the device, so the weights in memory survive; a non-finite
loss with finite gradients is still applied and still stops at the ledger's check.

The evaluation loops `evaluate_det_voc` (reference engine_loc.py:127-201) and `evaluate_refinements` (engine.py:617-724) follow: the
detection head (spe_amd.infer.detect) between the forward and a detection meter (spe_amd.evalmetrics), DESIGN.md section 8k;
`evaluate_det_voc` also feeds a caller's ClassificationAPMeter with the image-level logits."""
import copy
import time

import torch

from . import camboxes, infer
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


def format_skip_report(report, limit=5):
    """One line from FlatAdamW.skip_report(): the attempt and up to `limit` parameters behind the skipped step - `name[index] nan=N inf=M`
    for a parameter with non-finite elements (the index of the first), `name |g|max=X (square overflows fp32)` for one whose finite
    elements overflow its own squared norm; without any culprit, the rows of largest |g| (only the total norm overflowed).  Pure host
    code: no device access."""
    def index(row):
        return "[" + ", ".join(str(i) for i in row["first_bad"]) + "]" if row["first_bad"] is not None else ""

    def tail(rows):
        return f" (+{len(rows) - limit} more)" if len(rows) > limit else ""

    head = f"Skipped step {report['attempt']}: "
    culprits = report["culprits"]
    if culprits:
        parts = [f"{r['name']}{index(r)} nan={r['nan']} inf={r['inf']}" if r["nan"] + r["inf"] > 0
                 else f"{r['name']} |g|max={r['grad_absmax']:.4g} (square overflows fp32)" for r in culprits[:limit]]
        return head + "; ".join(parts) + tail(culprits)
    largest = report["largest"]
    parts = [f"{r['name']} |g|max={r['grad_absmax']:.4g}" for r in largest[:limit]]
    return head + "no single parameter is non-finite, only the total squared norm overflows fp32; largest gradients: " + "; ".join(parts) + tail(largest)


def apply_curriculum_coco(weight_dict, epoch):
    """engine.py:573-581, the COCO loop's curriculum: before epoch 1 only the image-label keys keep their weight.  The reference's
    second block (:578-581) zeroes the keys that contain `header` - there the LOG header string '[<time>] => Epoch: [<n>]', not
    'ref': it matches no key and changes nothing, so it is restated here as nothing."""
    if epoch < 1:
        for k in weight_dict:
            if "img_label" not in k:
                weight_dict[k] = 0.0
    return weight_dict


def _train_one_epoch(curriculum, model, criterion, data_loader, optimizer, device, epoch, max_norm, args, postprocessors, criterion_refine,
                     pseudo_meter=None, proposal_meter=None):
    """The loop of both public entries; `curriculum(weight_dict, epoch)` is what differs between them.

    pseudo_meter: an evalmetrics.PseudoLabelMeter with the stages 'cam', 'rf_1' .. 'rf_<num_refines>' (DESIGN.md section 8o).  Every
    batch scores the stage-0 targets and the targets of every refine stage against the loader's own 'boxes' / 'labels' (kept before the
    pseudo labels replace them; a target without them raises ValueError): one launch per (step, stage), no host read.  After the loop the
    meter is merged between the ranks and printed, and its four means per stage join the returned statistics as
    pseudo_<stage>_corloc / _precision / _recall / _mean_iou.  The rows are scored in the frame the criterion receives them: CAM rows
    normalised by the padded canvas (with the (H, W) -> dsize transposition of camboxes._pseudo_labels), ground truth by the image's own
    size - on fixed square inputs the same frame, elsewhere the mismatch the criterion trains on.  None: nothing of it.

    proposal_meter: an evalmetrics.ProposalRecallMeter with the stages 's0' .. 's<num_refines>' (DESIGN.md section 8p).  Every batch scores
    ALL query boxes of every stage of `outputs`, 0 included, against the same ground-truth rows: the sigmoid and one launch per (step,
    stage), no host read.  After the loop the meter is merged and printed, and the statistics gain prop_s<rf>_recall_at_<k> for every k
    of the meter, prop_s<rf>_ceiling (both at the meter's first threshold, means over the classes with rows) and
    prop_s<rf>_mean_best_iou.  None: nothing of it.

    Gradient accumulation: with a FlatAdamW whose reducer has accum_steps > 1 every iteration still does zero_grad / backward /
    finish() and is recorded in the ledger, optimizer.step() runs when finish() completed a cycle, and the micro-batches of a cycle
    left open at the end of the epoch are dropped (one printed line).  With accum_steps = 1 every finish() completes a cycle."""
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
        present = camboxes.present_lists(targets, "img_label")         # the loader's HOST tensors, before they move: a read, no synchronisation
        samples = samples.to(device)
        targets = [{k: v.to(device) for k, v in t.items()} for t in targets]
        outputs = model(samples)
        # get_pseudo_label_multi_boxes with the target rows assembled on the device: the box counts are the one read between the forward
        # and the criterion.  The class lists follow from the counts, so PostProcessRefine gets its
        # `labels_unique` without torch.unique and picks the stage k+1 targets in one launch per stage.
        pseudo = camboxes.pseudo_targets(outputs[0], samples, present, args.num_classes, args.cam_thr, args.multi_box_ratio)
        logits = outputs[0]["pred_logits"]
        uniq = infer.ClassTable([[c for c in cl if c < logits.shape[2]] for cl in pseudo.classes], logits.device).per_image()
        if pseudo_meter is not None or proposal_meter is not None:
            for key in ("boxes", "labels"):
                if any(key not in t for t in targets):
                    raise ValueError(f"pseudo_meter: the loader's targets carry no {key!r} to score the pseudo labels against")
            gt = [{"boxes": t["boxes"], "labels": t["labels"]} for t in targets]
        for t, p, u in zip(targets, pseudo.per_image(), uniq):
            t.update(p)
            t["labels_unique"] = u
        pseudo_label_refine = get_refinements_pseudo_label(outputs, samples, targets, args, postprocessors)
        if pseudo_meter is not None:
            pseudo_meter.update("cam", pseudo, gt)
            for rf, rows in pseudo_label_refine.items():
                pseudo_meter.update(f"rf_{rf}", rows, gt)
        if proposal_meter is not None:
            for rf, out in outputs.items():
                proposal_meter.update(f"s{rf}", out, gt)
        loss_dict = criterion(outputs[0], targets)
        for rf, out in outputs.items():
            if rf == 0:
                continue
            for k, v in criterion_refine(out, pseudo_label_refine[rf]).items():
                loss_dict[f"{RF_HEADER}_{rf}_{k}"] = v
        curriculum(weight_dict, epoch)

        losses = ledger.record(loss_dict, weight_dict, lr=optimizer.param_groups[0]["lr"])
        optimizer.zero_grad()
        losses.backward()
        if flat:
            optimizer.reducer.finish()
            if optimizer.reducer.micro != 0:             # inside an accumulation cycle: the update waits for its last micro-step
                continue
        elif max_norm > 0:
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
        optimizer.step()

    if flat and optimizer.reducer.micro != 0:
        left = optimizer.reducer.micro
        optimizer.reducer.restart_cycle()
        print(f"Dropped the last {left} micro-batch(es) of the epoch: an incomplete accumulation cycle of {optimizer.reducer.accum_steps}")
    if flat and optimizer.skip_nonfinite and optimizer.skipped_steps() > 0:
        print(f"Optimizer steps skipped on a non-finite gradient: {optimizer.skipped_steps()} so far, the first at step {optimizer.first_skipped()}")
        if optimizer.skip_report_mode is not None:
            report = optimizer.skip_report(model)
            if report is not None:
                print(format_skip_report(report))
    stats = ledger.global_avg()                 # synchronised between the ranks; raises if a step's total was not finite
    print("Averaged stats:", ledger)
    if pseudo_meter is not None:
        pseudo_meter.merge()
        print(pseudo_meter)
        for stage, r in pseudo_meter.summarize().items():
            for k in ("corloc", "precision", "recall"):
                stats[f"pseudo_{stage}_{k}"] = r["mean_" + k]
            stats[f"pseudo_{stage}_mean_iou"] = r["mean_mean_iou"]
    if proposal_meter is not None:
        proposal_meter.merge()
        print(proposal_meter)
        for stage, r in proposal_meter.summarize().items():
            for k, v in zip(proposal_meter.ks, r["mean_recall"][0].tolist()):
                stats[f"prop_{stage}_recall_at_{k}"] = v
            stats[f"prop_{stage}_ceiling"] = float(r["mean_ceiling"][0])
            stats[f"prop_{stage}_mean_best_iou"] = r["mean_mean_best_iou"]
    return stats


def train_one_epoch_refine(model, criterion, data_loader, optimizer, device, epoch, max_norm=0, args=None, postprocessors=None,
                           criterion_refine=None, proposal_meter=None, pseudo_meter=None):
    """engine.py:93-174 (the VOC loop).  pseudo_meter, proposal_meter: see _train_one_epoch."""
    return _train_one_epoch(apply_curriculum, model, criterion, data_loader, optimizer, device, epoch, max_norm, args, postprocessors,
                            criterion_refine, pseudo_meter=pseudo_meter, proposal_meter=proposal_meter)


def train_one_epoch_refine_coco(model, criterion, data_loader, optimizer, device, epoch, max_norm=0, args=None, postprocessors=None,
                                criterion_refine=None, proposal_meter=None, pseudo_meter=None):
    """engine.py:534-613 (the loop main_coco.py:356 calls): the same body with the COCO curriculum.  pseudo_meter, proposal_meter: see _train_one_epoch."""
    return _train_one_epoch(apply_curriculum_coco, model, criterion, data_loader, optimizer, device, epoch, max_norm, args, postprocessors,
                            criterion_refine, pseudo_meter=pseudo_meter, proposal_meter=proposal_meter)


# ---- evaluation loops (reference engine_loc.py:127-201, engine.py:617-724) -----------------------------------
# One forward, one detection-head launch (infer.detect) and one meter update per batch; nothing on a device tensor is read on the host
# inside the batch loop.  The image id that looks the ground truth up is read from the loader's HOST tensor before the targets move
# to the device; the meters get the id as a 0-d device tensor.
def _host_id(t, key):
    return int(t[key])                            # the loader's tensors live on the host: a read, not a synchronisation


def _lookup(base_ds):
    if base_ds is None:
        raise ValueError("base_ds: a mapping or a callable from image id to the ground-truth dict of the meter (evalmetrics.py)")
    return base_ds if callable(base_ds) else base_ds.__getitem__


def _coco_cat_ids(base_ds):
    """The category ids of the run: base_ds.getCatIds() (the COCO API's name) or base_ds.cat_ids, else every label of a mapping."""
    if hasattr(base_ds, "getCatIds"):
        return list(base_ds.getCatIds())
    if hasattr(base_ds, "cat_ids"):
        return list(base_ds.cat_ids)
    if hasattr(base_ds, "values"):
        return sorted({int(c) for g in base_ds.values() for c in torch.as_tensor(g["labels"]).reshape(-1).tolist()})
    raise ValueError("evaluate_refinements: a callable base_ds needs .cat_ids (or .getCatIds())")


@torch.no_grad()
def evaluate_det_voc(model, criterion, postprocessors, data_loader, base_ds, device, output_dir, cache_dir, with_flip=False, *kargs,
                     cls_meter=None, cls_key="x_logits", proposal_meter=None, **kwargs):
    """engine_loc.py:127-201 with the VOC meter in place of the result files: top 300, per-class NMS at 0.5, AP (VOC07 11-point unless
    use_07_metric=False is passed) and CorLoc, printed in the lines of datasets/voc_voc.py:_eval_discovery and _do_python_eval (without
    the closing banner about the MATLAB code).  base_ds: image id (t['idx']) -> {'boxes' [g,4] annotation frame, 'labels' [g],
    'difficult' [g]}.  The class names come from data_loader.dataset.classes when it has them ('__background__' skipped), the class
    count from there or from num_classes= (20).  Writes no files; returns the meter's summary (the reference returns None).
    cls_meter: an evalmetrics.ClassificationAPMeter (the reference's AveragePrecisionMeter, cams_deit.py:493-574) that is fed the raw
    image-level logits outputs[cls_key] - with_flip: of the merged output - against the stacked t['label'] of every batch; after the
    detection lines its per-class AP and the mean are printed and returned as 'cls_ap' (fp64 [C]) and 'cls_map'.  None: nothing of it.
    proposal_meter: an evalmetrics.ProposalRecallMeter with a stage 'det' (DESIGN.md section 8p): every batch scores all query boxes of
    the (with_flip: merged) outputs against base_ds's rows - the boxes divided by the image's [w, h, w, h] and turned into cxcywh on the
    device, the labels as they are (a label is its logit column).  Merged and printed after the loop, its summary returned as
    'proposals'.  None: nothing of it."""
    from .evalmetrics import VOCDetectionMeter
    from .util.box_ops import box_xyxy_to_cxcywh
    from .util.misc import NestedTensor
    model.eval()
    criterion.eval()
    ledger = StepLedger(delimiter="  ")
    header = f"[{time.strftime('%Y-%m-%d-%H:%M:%S', time.localtime())}] => Test:"
    names = [c for c in getattr(getattr(data_loader, "dataset", None), "classes", ()) if c != "__background__"]
    C = len(names) or int(kwargs.get("num_classes", 20))
    names = names or [f"class{c + 1}" for c in range(C)]
    use_07_metric = bool(kwargs.get("use_07_metric", True))
    meter = VOCDetectionMeter(num_classes=C, ovthresh=0.5, file_roundtrip=True)
    gt_of = _lookup(base_ds)
    if proposal_meter is not None and "det" not in proposal_meter.stages:
        raise ValueError(f"proposal_meter: the evaluation loop updates the stage 'det'; the meter has {proposal_meter.stages}")
    for samples, targets in ledger.log_every(data_loader, 256, header):
        ids = [_host_id(t, "idx") for t in targets]
        samples = samples.to(device)
        batch_size = samples.tensors.shape[0]
        targets = [{k: v.to(device) for k, v in t.items()} for t in targets]
        if with_flip:
            coupled = NestedTensor(torch.cat((samples.tensors, samples.tensors.flip(-1)), dim=0),
                                   None if samples.mask is None else torch.cat((samples.mask, samples.mask.flip(-1)), dim=0))
            outputs = infer.decouple_output(model(coupled)[0], bs=batch_size)
        else:
            outputs = model(samples)[0]
        sizes = torch.stack([t["image_size"].flip(0) for t in targets], dim=0)
        det = infer.detect(outputs, sizes, 300, 0.5)
        meter.update(det.padded(), [{**gt_of(i), "image_id": t["idx"].reshape(())} for i, t in zip(ids, targets)])
        if proposal_meter is not None:
            rows = []
            for i, t in zip(ids, targets):
                g = gt_of(i)
                xyxy = torch.as_tensor(g["boxes"]).to(device=device, dtype=torch.float32).reshape(-1, 4)
                rows.append({"boxes": box_xyxy_to_cxcywh(xyxy / t["image_size"].to(torch.float32).repeat(2)),
                             "labels": torch.as_tensor(g["labels"]).to(device=device, dtype=torch.int64).reshape(-1)})
            proposal_meter.update("det", outputs, rows)
        if cls_meter is not None:
            cls_meter.add(outputs[cls_key], torch.stack([t["label"] for t in targets]))      # logits, not sigmoids: no saturation ties
    meter.merge()
    out = meter.summarize(use_07_metric=use_07_metric)
    for what, per_class, mean in (("CorLoc", out["corloc"].tolist(), out["mean_corloc"]), ("AP", out["ap"].tolist(), out["map"])):
        if what == "AP":
            print("VOC07 metric? " + ("Yes" if use_07_metric else "No"))
        for name, v in zip(names, per_class):
            print("{} for {} = {:.4f}".format(what, name, v))
        print("Mean {} = {:.4f}".format(what, mean))
        print("~~~~~~~~")
        print("Results:")
        for v in per_class:
            print("{:.3f}".format(v))
        print("{:.3f}".format(mean))
        print("~~~~~~~~")
    if cls_meter is not None:
        cls_meter.merge()
        cls = cls_meter.summarize()
        cls_names = names if len(names) == cls["ap"].numel() else [f"class{c + 1}" for c in range(cls["ap"].numel())]
        for name, v in zip(cls_names, cls["ap"].tolist()):
            print("AP (cls) for {} = {:.4f}".format(name, v))
        print("Mean AP (cls) = {:.4f}".format(cls["map"]))
        out["cls_ap"], out["cls_map"] = cls["ap"], cls["map"]
    if proposal_meter is not None:
        proposal_meter.merge()
        print(proposal_meter)
        out["proposals"] = proposal_meter.summarize()["det"]
    return out


_COCO_LINES = (("Precision", "AP", "0.50:0.95", "all", 100), ("Precision", "AP", "0.50", "all", 100), ("Precision", "AP", "0.75", "all", 100),
               ("Precision", "AP", "0.50:0.95", "small", 100), ("Precision", "AP", "0.50:0.95", "medium", 100),
               ("Precision", "AP", "0.50:0.95", "large", 100), ("Recall", "AR", "0.50:0.95", "all", 1), ("Recall", "AR", "0.50:0.95", "all", 10),
               ("Recall", "AR", "0.50:0.95", "all", 100), ("Recall", "AR", "0.50:0.95", "small", 100),
               ("Recall", "AR", "0.50:0.95", "medium", 100), ("Recall", "AR", "0.50:0.95", "large", 100))


@torch.no_grad()
def evaluate_refinements(model, criterion, postprocessors, data_loader, base_ds, device, output_dir, refine_stage=0):
    """engine.py:617-724 for 'bbox': the last auxiliary output of refinement stage `refine_stage`, its losses in the step ledger (scaled,
    `_unscaled`, class_error with window 1), top 100, per-class NMS at 0.5, the COCO meter.  base_ds: image id (t['image_id']) ->
    {'boxes' [g,4] xywh, 'labels' [g], 'iscrowd' [g], 'area' [g]}; the category ids are base_ds.getCatIds() / base_ds.cat_ids, or every
    label of a mapping.  -> (stats, meter): the global averages of the ledger plus stats['coco_eval_bbox'], COCOeval's twelve numbers."""
    from .evalmetrics import COCODetectionMeter
    for k in ("segm", "panoptic"):
        if k in postprocessors:
            raise NotImplementedError(f"evaluate_refinements: the {k!r} post-processor is outside this package (DESIGN.md section 7)")
    model.eval()
    criterion.eval()
    ledger = StepLedger(windows={"class_error": 1}, fmts={"class_error": "{value:.2f}"}, delimiter="  ")
    meter = COCODetectionMeter(_coco_cat_ids(base_ds))
    gt_of = _lookup(base_ds)
    for samples, targets in ledger.log_every(data_loader, 10, "Test:"):
        ids = [_host_id(t, "image_id") for t in targets]
        samples = samples.to(device)
        targets = [{k: v.to(device) for k, v in t.items()} for t in targets]
        outputs = model(samples)[refine_stage]["aux_outputs"][-1]
        loss_criterion = copy.deepcopy(criterion.losses)
        criterion.losses = ["labels", "boxes", "cardinality"]
        try:
            loss_dict = criterion(outputs, targets)
        finally:
            criterion.losses = loss_criterion
        ledger.record(loss_dict, criterion.weight_dict)
        orig_target_sizes = torch.stack([t["orig_size"] for t in targets], dim=0)
        det = infer.detect(outputs, orig_target_sizes, 100, 0.5)
        meter.update(det.padded(), [{**gt_of(i), "image_id": t["image_id"].reshape(())} for i, t in zip(ids, targets)])
    stats = ledger.global_avg()                  # synchronised between the ranks
    print("Averaged stats:", ledger)
    meter.merge()
    numbers = meter.summarize()["stats"]
    for (title, short, iou, area, dets), v in zip(_COCO_LINES, numbers):
        print(" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format("Average " + title, f"({short})", iou, area, dets, v))
    stats["coco_eval_bbox"] = numbers.tolist()
    return stats, meter
