"""Shapes and inputs for the training-target kernels (csrc/train_targets.hip; tests/train_targets_ref.py restates them): the smallest
sizes at which the scan, the row assembly and the pick can go wrong.

spe_cam_targets scans the M maps in chunks of 256 with a carry, so M runs over 1, 2 and both sides of the first two chunk edges;
max_boxes over 1, a small value and the drivers' 256.  spe_refine_pick gives one wave of 64 lanes to an (image, class) pair, so Q runs
over 1, both sides of 64, a few strides (300) and many (1025)."""
import numpy as np
import torch

CHUNK = 256                                        # TT_THREADS of csrc/train_targets.hip: maps per scan step
CAM_MS = (1, 2, 255, 256, 257, 513)
CAM_MAX_BOXES = (1, 4, 256)
CAM_SIZES = ((1333, 800), (7, 3))                  # (W, H)
CAM_COUNTS = ("zero", "full", "edges", "status")
GUARD_F, GUARD_L, GUARD_ROWS = -7.25, -77, 16      # what the rows behind T hold before and after a launch


def cam_counts(kind, M, max_boxes, seed=0):
    """int32 [M]: all 0, all max_boxes, random with zeros on both sides of every chunk edge, random with one status in the middle."""
    g = np.random.default_rng(1000 * M + max_boxes + seed)
    if kind == "zero":
        return np.zeros(M, np.int32)
    if kind == "full":
        return np.full(M, max_boxes, np.int32)
    n = g.integers(0, max_boxes + 1, M).astype(np.int32)
    if kind == "edges":
        n[0] = n[-1] = 0
        for e in range(CHUNK, M + 1, CHUNK):
            n[e - 1] = 0
            if e < M:
                n[e] = 0
        return n
    assert kind == "status"
    n[M // 2] = -5
    return n


def cam_boxes(M, max_boxes, W, H, seed=0):
    """int32 [M, max_boxes, 4] as [x0, y0, x1, y1] with x0 < x1 <= W, y0 < y1 <= H, uniformly drawn: about half of the sums x0 + x1
    and y0 + y1 are odd, so that the halving and the division both round."""
    g = np.random.default_rng(7 * M + max_boxes + W + seed)
    x0 = g.integers(0, W, (M, max_boxes))
    y0 = g.integers(0, H, (M, max_boxes))
    x1 = x0 + 1 + g.integers(0, W, (M, max_boxes)) % (W - x0)
    y1 = y0 + 1 + g.integers(0, H, (M, max_boxes)) % (H - y0)
    return np.stack([x0, y0, x1, y1], -1).astype(np.int32)


def cam_classes(M, seed=0):
    """int32 [M]: the 0-based class of every map, ascending inside runs the way an image-major table is."""
    g = np.random.default_rng(31 * M + seed)
    return np.sort(g.integers(0, 90, M)).astype(np.int32)


def cam_packed(counts, boxes):
    return np.concatenate([counts.reshape(-1), boxes.reshape(-1)]).astype(np.int32)


# ---- the pick ------------------------------------------------------------------------------------------------------------------------
PICK_SHAPES = ((1, 1, 1), (2, 63, 21), (2, 64, 21), (2, 65, 21), (3, 300, 91), (1, 1025, 2))
PICK_TABLES = ("empty_one", "all", "first", "last")
PICK_INPUTS = ("free", "ties", "nan1", "nans", "inf")
TIE_FREE = ("free",)                               # the inputs whose best probability is unique in every column


def pick_logits(kind, B, Q, Kc, seed=0):
    """fp32 [B, Q, Kc].  Every column is a permutation of Q evenly spaced logits in [-4, 4]: neighbouring probabilities differ by at
    least 1e-4, whatever sigmoid computes them.  On top of that
      ties   up to five queries per column with DIFFERENT logits >= 20: all of them are probability 1.0 in fp32
      nan1   one NaN in every second column;  nans  three NaNs in every column (where Q allows)
      inf    +inf at up to three queries of the even columns (ties at 1.0), the odd columns -inf everywhere (every query ties at 0.0)"""
    g = np.random.default_rng(100 * Q + Kc + seed)
    grid = np.linspace(-4.0, 4.0, Q, dtype=np.float32) if Q > 1 else np.float32([0.3])
    x = np.stack([np.stack([g.permutation(grid) for _ in range(Kc)], 1) for _ in range(B)]).astype(np.float32)
    for b in range(B):
        for c in range(Kc):
            q = np.sort(g.choice(Q, min(Q, 5), replace=False))
            if kind == "ties":
                x[b, q, c] = np.float32(20.0) + np.arange(len(q), dtype=np.float32) * np.float32(3.5)     # the lowest query has the lowest logit
            elif kind == "nan1" and c % 2 == 0:
                x[b, q[-1], c] = np.nan
            elif kind == "nans":
                x[b, q[-3:], c] = np.nan
            elif kind == "inf":
                if c % 2 == 0:
                    x[b, q[-3:], c] = np.inf
                else:
                    x[b, :, c] = -np.inf
    return torch.from_numpy(x)


def pick_boxes(B, Q, seed=0):
    g = torch.Generator().manual_seed(17 * Q + B + seed)
    return torch.rand(B, Q, 4, generator=g)


def pick_classes(kind, B, Kc, seed=0):
    """Per image the sorted class ids: image 0 empty and the others a random subset / all Kc / the first only / the last only."""
    g = np.random.default_rng(13 * Kc + B + seed)
    if kind == "all":
        return [list(range(Kc)) for _ in range(B)]
    if kind == "first":
        return [[0] for _ in range(B)]
    if kind == "last":
        return [[Kc - 1] for _ in range(B)]
    assert kind == "empty_one"
    return [[] if b == 0 else sorted(g.choice(Kc, max(1, Kc // 3), replace=False).tolist()) for b in range(B)]


# ---- the drivers and the loop --------------------------------------------------------------------------------------------------------
def cam_maps(B, Kc, h, w, seed=12):
    """Smooth class maps [B, Kc, h, w] (two bumps and a little noise each): several borders per map at a threshold of 20 %."""
    g = torch.Generator().manual_seed(seed)
    cams = torch.zeros(B, Kc, h, w)
    yy, xx = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    for b in range(B):
        for c in range(Kc):
            for _ in range(2):
                cy, cx = torch.rand(2, generator=g) * torch.tensor([h - 1.0, w - 1.0])
                cams[b, c] += torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * (1.0 + 2 * torch.rand(1, generator=g)) ** 2))
    return cams + 0.05 * torch.randn(cams.shape, generator=g)


STUB_B, STUB_KC, STUB_Q, STUB_H, STUB_W, STUB_STAGES = 2, 5, 70, 72, 104, 3


def stub_batches(steps=3, seed=5):
    """-> list of (canned, targets): what StubModel returns for a batch (per stage logits and boxes, the class maps under stage 0) and
    the loader's HOST targets.  Image 1 of the second batch has no present class."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in range(steps):
        canned = {"cams_cls": cam_maps(STUB_B, STUB_KC, 9, 13, seed=seed + s),
                  "stages": [(torch.randn(STUB_B, STUB_Q, STUB_KC + 1, generator=g) * 3, torch.rand(STUB_B, STUB_Q, 4, generator=g))
                             for _ in range(STUB_STAGES)]}
        canned["stages"][0][0][0, 3:9, 2] = 30.0                                    # saturated ties in a class that is picked
        present = (torch.rand(STUB_B, STUB_KC, generator=g) < 0.6).long()
        present[0, 1] = 1
        if s == 1:
            present[1] = 0
        targets = [{"img_label": present[b].clone(), "orig_size": torch.tensor([STUB_H, STUB_W])} for b in range(STUB_B)]
        out.append((canned, targets))
    return out


class StubModel(torch.nn.Module):
    """Returns the canned outputs batch by batch, scaled by two parameters, so that an optimizer step changes what the next step's
    targets are picked from: {stage: {'pred_logits', 'pred_boxes'}}, the class maps under stage 0."""

    def __init__(self, batches):
        super().__init__()
        self.batches, self.calls = batches, 0
        self.p = torch.nn.Parameter(torch.tensor([1.0, 0.75]))

    def forward(self, samples):
        canned = self.batches[self.calls % len(self.batches)][0]
        self.calls += 1
        dev = samples.tensors.device
        out = {k: {"pred_logits": lg.to(dev) * self.p[0], "pred_boxes": bx.to(dev) * self.p[1]} for k, (lg, bx) in enumerate(canned["stages"])}
        out[0]["cams_cls"] = canned["cams_cls"].to(dev)
        return out


class StubCriterion:
    """Losses that are plain functions of the output AND of the targets' boxes, labels and scores: a changed target changes them."""

    def __init__(self):
        self.weight_dict = {"loss_ce": 2.0, "loss_bbox": 5.0, "loss_giou": 2.0}
        self.seen = []

    def train(self):
        pass

    def __call__(self, outputs, targets):
        self.seen.append([sorted(t) for t in targets])
        lg, bx = outputs["pred_logits"], outputs["pred_boxes"]
        tb, tl = torch.cat([t["boxes"] for t in targets]), torch.cat([t["labels"] for t in targets])
        n = float(max(tb.shape[0], 1))
        ce = lg.sigmoid().mean() * (1 + tl.float().sum() / (10 * n))
        if "scores" in targets[0]:
            ce = ce * (1 + torch.cat([t["scores"] for t in targets]).sum() / n)
        d = bx.mean() - tb.sum() / (4 * n)
        return {"loss_ce": ce, "class_error": ce * 100, "loss_bbox": d * d + 0.25, "loss_giou": (bx * bx).mean() * (1 + tb[:, 2:].sum() / n)}


def stub_loader(batches):
    from spe_amd.util.misc import NestedTensor
    return [(NestedTensor(torch.zeros(STUB_B, 3, STUB_H, STUB_W), torch.zeros(STUB_B, STUB_H, STUB_W, dtype=torch.bool)),
             [dict(t) for t in targets]) for _, targets in batches]


def stub_args():
    import argparse
    return argparse.Namespace(num_classes=STUB_KC, cam_thr=0.2, multi_box_ratio=0.5, num_refines=STUB_STAGES - 1)


STUB_EPOCH = 15                                    # past the curriculum: every weight counts


def run_stub_epochs(device, epochs=2, steps=3):
    """`epochs` of engine.train_one_epoch_refine on the stub -> (stats of the last epoch, the parameters, what the criteria saw)."""
    from spe_amd import engine
    from spe_amd.models.conditional_detr import PostProcessRefine
    batches = stub_batches(steps)
    model = StubModel(batches).to(device)
    crit, crit_r = StubCriterion(), StubCriterion()
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    for e in range(epochs):
        stats = engine.train_one_epoch_refine(model, crit, stub_loader(batches), opt, device, STUB_EPOCH + e, 0.1, stub_args(),
                                              {"bbox": PostProcessRefine()}, crit_r)
    return stats, model.p.detach().cpu().clone(), crit.seen, crit_r.seen


def run_parent_epochs(device, epochs=2, steps=3):
    """The same epochs with the body the loop had before the targets moved to the device: get_pseudo_label_multi_boxes on the moved
    targets, PostProcessRefine without 'labels_unique'."""
    import copy
    from spe_amd import camboxes, engine
    from spe_amd.models.conditional_detr import PostProcessRefine
    from spe_amd.steplog import StepLedger
    batches = stub_batches(steps)
    model = StubModel(batches).to(device)
    crit, crit_r, args, post = StubCriterion(), StubCriterion(), stub_args(), {"bbox": PostProcessRefine()}
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    for e in range(epochs):
        ledger = StepLedger(windows={"lr": 1, "class_error": 1}, fmts={"lr": "{value:.6f}", "class_error": "{value:.2f}"}, delimiter="  ")
        wd = engine.get_refine_weight_dict(copy.deepcopy(crit.weight_dict), args.num_refines, header=engine.RF_HEADER)
        for samples, targets in stub_loader(batches):
            samples = samples.to(device)
            targets = [{k: v.to(device) for k, v in t.items()} for t in targets]
            outputs = model(samples)
            for t, p in zip(targets, camboxes.get_pseudo_label_multi_boxes(outputs[0], samples, targets, args)):
                t.update(p)
            refine = engine.get_refinements_pseudo_label(outputs, samples, targets, args, post)
            loss_dict = crit(outputs[0], targets)
            for rf, out in outputs.items():
                if rf:
                    for k, v in crit_r(out, refine[rf]).items():
                        loss_dict[f"{engine.RF_HEADER}_{rf}_{k}"] = v
            engine.apply_curriculum(wd, STUB_EPOCH + e)
            losses = ledger.record(loss_dict, wd, lr=opt.param_groups[0]["lr"])
            opt.zero_grad()
            losses.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 0.1)
            opt.step()
        stats = ledger.global_avg()
    return stats, model.p.detach().cpu().clone()
