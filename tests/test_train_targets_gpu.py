"""The training-target kernels (csrc/train_targets.hip) on the device.

spe_cam_targets against the numpy restatement (tests/train_targets_ref.py) with torch.equal, on buffers that carry a guard pattern
behind the last row; spe_refine_pick bit for bit - NaN included - against the ATen composition of PostProcessRefine on the same device
(REFINE_KERNEL = False) and against the restatement of torch.max's rule; the drivers against the "host" contours; the stretch from the
model's outputs to both target lists under torch's sync debug mode; the training loop with the kernels on and off."""
import argparse

import numpy as np
import pytest
import torch

import cambox_cases
import train_targets_cases as C
import train_targets_ref as R

pytestmark = pytest.mark.gpu


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32).numpy() if t.dtype == torch.float32 else t.numpy()


# ---- spe_cam_targets -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_boxes", C.CAM_MAX_BOXES)
@pytest.mark.parametrize("M", C.CAM_MS)
def test_cam_targets_equal_the_restatement(dev, M, max_boxes):
    from spe_amd import kernels as K
    cls0 = C.cam_classes(M)
    cls_d = torch.from_numpy(cls0).to(dev)
    for W, H in C.CAM_SIZES:
        boxes = C.cam_boxes(M, max_boxes, W, H)
        for kind in C.CAM_COUNTS:
            counts = C.cam_counts(kind, M, max_boxes)
            packed = torch.from_numpy(C.cam_packed(counts, boxes)).to(dev)
            for single in (False, True):
                rows, labels, off = R.cam_targets(counts, boxes, cls0, single, W, H)
                T, cap = rows.shape[0], M * (1 if single else max_boxes)
                out = (torch.full((cap + C.GUARD_ROWS, 4), C.GUARD_F, device=dev), torch.full((cap + C.GUARD_ROWS,), C.GUARD_L, device=dev),
                       torch.full((M + 1 + C.GUARD_ROWS,), C.GUARD_L, device=dev, dtype=torch.int32))
                b, l, o = K.cam_targets(packed, cls_d, max_boxes, single, W, H, cap=cap, out=out)
                where = (M, max_boxes, W, H, kind, single)
                assert torch.equal(b[:T].cpu(), torch.from_numpy(rows)), where
                assert torch.equal(l[:T].cpu(), torch.from_numpy(labels)) and torch.equal(o[:M + 1].cpu(), torch.from_numpy(off)), where
                assert bool((b[T:] == C.GUARD_F).all()) and bool((l[T:] == C.GUARD_L).all()) and bool((o[M + 1:] == C.GUARD_L).all()), where
                assert torch.equal(packed[:M].cpu(), torch.from_numpy(counts)), where          # a status stays where it is
                if kind == "status":
                    assert (counts < 0).sum() == 1 and off[M // 2] == off[M // 2 + 1]


def test_cam_targets_no_map_and_wrapper_checks(dev):
    from spe_amd import kernels as K, lib
    none = torch.zeros((0,), dtype=torch.int32, device=dev)
    b, l, o = K.cam_targets(none, none, 256, False, 100, 50)
    assert b.shape == (0, 4) and l.shape == (0,) and o.tolist() == [0]
    packed = torch.zeros((2 * (1 + 4 * 4),), dtype=torch.int32, device=dev)
    cls = torch.zeros((2,), dtype=torch.int32, device=dev)
    with pytest.raises(lib.SpeLibraryError, match="status -3"):
        K.cam_targets(packed, cls, 4, False, 100, 50, cap=7)
    with pytest.raises(ValueError):
        K.cam_targets(packed[:-1], cls, 4, False, 100, 50)
    with pytest.raises(lib.SpeLibraryError):
        K.cam_targets(packed.cpu(), cls.cpu(), 4, False, 100, 50)


# ---- spe_refine_pick -------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def detr():
    from spe_amd.models import conditional_detr as cd
    assert cd.REFINE_KERNEL is True                     # the default
    yield cd
    cd.REFINE_KERNEL = True


@pytest.mark.parametrize("kind", C.PICK_INPUTS)
@pytest.mark.parametrize("B,Q,Kc", C.PICK_SHAPES)
def test_refine_pick_equals_aten_and_the_rule(dev, detr, B, Q, Kc, kind):
    """The yardstick is PostProcessRefine's ATen composition on the same device; the rule is torch.max's as train_targets_ref states it,
    applied to the probabilities the device computed."""
    from spe_amd import infer, lib
    logits, boxes = C.pick_logits(kind, B, Q, Kc).to(dev), C.pick_boxes(B, Q).to(dev)
    out = {"pred_logits": logits, "pred_boxes": boxes}
    sizes = torch.tensor([[480, 640]] * B, device=dev)
    prob = logits.sigmoid().cpu().numpy()
    for table in C.PICK_TABLES:
        classes = C.pick_classes(table, B, Kc)
        targets = [{"labels_unique": torch.tensor(cl, dtype=torch.int64, device=dev)} for cl in classes]
        detr.REFINE_KERNEL = False
        want = detr.PostProcessRefine()(out, sizes, targets)
        detr.REFINE_KERNEL = True
        lib.count_launches(True)
        got = detr.PostProcessRefine()(out, sizes, targets)
        counts = lib.count_launches(False)
        flat = infer.refine_targets(out, classes)
        assert counts == {"spe_refine_pick": 1}, counts
        scores, queries, rows, labels, off = R.refine_pick(prob, boxes.cpu().numpy(), classes)
        assert flat["offsets"] == off and np.array_equal(_bits(flat["queries"]), queries) and np.array_equal(_bits(flat["labels"]), labels)
        assert np.array_equal(_bits(flat["scores"]), scores) and np.array_equal(_bits(flat["boxes"]).reshape(-1, 4), rows), (table, "rule")
        for b in range(B):
            for k in ("scores", "labels", "boxes"):
                assert got[b][k].dtype == want[b][k].dtype and got[b][k].shape == want[b][k].shape, (table, b, k)
                assert np.array_equal(_bits(got[b][k]), _bits(want[b][k])), (table, b, k, "ATen")
                assert np.array_equal(_bits(got[b][k]), _bits(flat[k][off[b]:off[b + 1]])), (table, b, k)


def test_refine_pick_refuses_a_class_outside_the_logits(dev):
    from spe_amd import infer, lib
    out = {"pred_logits": C.pick_logits("free", 2, 65, 21).to(dev), "pred_boxes": C.pick_boxes(2, 65).to(dev)}
    for bad in ([[0], [21]], [[-1], [3]]):
        with pytest.raises(lib.SpeLibraryError, match="status -3"):
            infer.refine_targets(out, bad)
    with pytest.raises(ValueError):
        infer.refine_targets(out, [[0]])


# ---- the drivers -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def contours():
    from spe_amd import camboxes
    assert camboxes.get_contours() == "device"          # the default
    yield camboxes
    camboxes.set_contours("device")


def _canvas(images, rows, cols):
    """The named images of cambox_cases side by side as class maps [1, n, rows, cols] of 0 / 1: prepared at their own size they threshold
    to themselves."""
    maps = torch.zeros(1, len(images), rows, cols)
    for i, im in enumerate(images):
        maps[0, i, :im.shape[0], :im.shape[1]] = torch.from_numpy((im > 0).astype(np.float32))
    return maps


@pytest.mark.parametrize("single", [False, True])
def test_drivers_on_the_cambox_cases_equal_the_host_contours(dev, contours, single):
    from spe_amd.util.misc import NestedTensor
    imgs = [im for _, im in cambox_cases.small_cases() if im.shape[0] <= 72 and im.shape[1] <= 136]
    assert len(imgs) >= 20
    rows, cols = 72, 136
    out = {"cams_cls": _canvas(imgs, rows, cols).to(dev)}
    samples = NestedTensor(torch.zeros(1, 3, cols, rows, device=dev), None)              # H = cols, W = rows: the (H, W) -> dsize quirk
    n = len(imgs)
    present = [[1] * n]
    present[0][5] = 0
    targets = [{"img_label": torch.tensor(present[0], device=dev)}]
    args = argparse.Namespace(num_classes=n, cam_thr=0.2, multi_box_ratio=0.25)
    fn = contours.get_pseudo_label if single else contours.get_pseudo_label_multi_boxes
    ratio = 1.0 if single else 0.25
    contours.set_contours("host")
    want = fn(out, samples, targets, args)
    want_pt = contours.pseudo_targets(out, samples, present, n, 0.2, ratio, single=single)
    contours.set_contours("device")
    got = fn(out, samples, targets, args)
    pt = contours.pseudo_targets(out, samples, present, n, 0.2, ratio, single=single)
    assert want[0]["boxes"].shape[0] == n - 1 if single else want[0]["boxes"].shape[0] >= n + 10
    for a in (got, pt.per_image(), want_pt.per_image()):
        assert len(a) == 1 and torch.equal(a[0]["boxes"], want[0]["boxes"]) and torch.equal(a[0]["labels"], want[0]["labels"])
        assert a[0]["boxes"].dtype == torch.float32 and a[0]["labels"].dtype == torch.int64 and a[0]["boxes"].is_cuda
    assert pt.classes == want_pt.classes == [[c + 1 for c in range(n) if c != 5]] and pt.offsets == want_pt.offsets


def test_pseudo_targets_over_images_without_maps(dev, contours):
    from spe_amd.util.misc import NestedTensor
    cams = C.cam_maps(3, 5, 9, 13).to(dev)
    samples = NestedTensor(torch.zeros(3, 3, C.STUB_H, C.STUB_W, device=dev), None)
    present = [[0] * 5, [1, 0, 1, 0, 1], [0] * 5]
    pt = contours.pseudo_targets({"cams_cls": cams}, samples, present, 5, 0.2, 0.5)
    contours.set_contours("host")
    want = contours.pseudo_targets({"cams_cls": cams}, samples, present, 5, 0.2, 0.5)
    assert pt.offsets == want.offsets and pt.offsets[1] == 0 and pt.offsets[2] == pt.offsets[3] and pt.classes == want.classes == [[], [1, 3, 5], []]
    assert torch.equal(pt.boxes, want.boxes) and torch.equal(pt.labels, want.labels)
    contours.set_contours("device")
    empty = contours.pseudo_targets({"cams_cls": cams}, samples, [[0] * 5] * 3, 5, 0.2, 0.5)
    assert empty.boxes.shape == (0, 4) and empty.offsets == [0, 0, 0, 0] and len(empty.per_image()) == 3


def test_overflow_raises_with_the_drivers_text(dev, contours, monkeypatch):
    from spe_amd.lib import SpeLibraryError
    from spe_amd.util.misc import NestedTensor
    monkeypatch.setattr(contours, "MAX_BOXES", 8)
    chk = dict(cambox_cases.small_cases())["checkerboard"]
    out = {"cams_cls": _canvas([chk], *chk.shape).to(dev)}
    samples = NestedTensor(torch.zeros(1, 3, chk.shape[1], chk.shape[0], device=dev), None)
    with pytest.raises(SpeLibraryError, match="status -5"):
        contours.pseudo_targets(out, samples, [[1]], 1, 0.2, 0.0)


# ---- the stretch from the outputs to both target lists ---------------------------------------------------------------------------------
def _stretch(camboxes, engine, infer, outputs, samples, targets, present, args, post, labels_unique=True):
    """What engine._train_one_epoch does between the forward and the criterion."""
    if labels_unique:
        pseudo = camboxes.pseudo_targets(outputs[0], samples, present, args.num_classes, args.cam_thr, args.multi_box_ratio)
        logits = outputs[0]["pred_logits"]
        uniq = infer.ClassTable([[c for c in cl if c < logits.shape[2]] for cl in pseudo.classes], logits.device).per_image()
        for t, p, u in zip(targets, pseudo.per_image(), uniq):
            t.update(p)
            t["labels_unique"] = u
    else:
        for t, p in zip(targets, camboxes.get_pseudo_label_multi_boxes(outputs[0], samples, targets, args)):
            t.update(p)
    return engine.get_refinements_pseudo_label(outputs, samples, targets, args, post)


def test_one_read_between_the_forward_and_the_criterion(dev, contours, detr, monkeypatch):
    """Under torch's sync debug mode every synchronising call raises.  The one read the stretch is allowed - the M box counts, 4 M
    bytes - is let through by name and counted; the composition the loop had before raises inside the same guard."""
    from spe_amd import engine, infer, lib
    batches = C.stub_batches(3)
    model, args, post = C.StubModel(batches).to(dev), C.stub_args(), {"bbox": detr.PostProcessRefine()}

    def batch(i):
        samples, host_targets = C.stub_loader(batches)[i]
        present = contours.present_lists(host_targets, "img_label")
        samples = samples.to(dev)
        targets = [{k: v.to(dev) for k, v in t.items()} for t in host_targets]
        with torch.no_grad():
            outputs = model(samples)
        return outputs, samples, targets, present

    _stretch(contours, engine, infer, *batch(0), args, post)                             # first call: allocations, library load
    reads, real = [], torch.Tensor.tolist

    def counted(self):
        if not self.is_cuda:
            return real(self)
        reads.append((self.dtype, self.numel()))
        torch.cuda.set_sync_debug_mode("default")
        try:
            return real(self)
        finally:
            torch.cuda.set_sync_debug_mode("error")
    monkeypatch.setattr(torch.Tensor, "tolist", counted)
    outputs, samples, targets, present = batch(1)
    M = sum(sum(1 for v in p if v > 0) for p in present)
    plain = [dict(t) for t in targets]
    torch.cuda.synchronize()
    lib.count_launches(True)
    torch.cuda.set_sync_debug_mode("error")
    try:
        refine = _stretch(contours, engine, infer, outputs, samples, targets, present, args, post)
        counts, seen = lib.count_launches(False), list(reads)
        with pytest.raises(RuntimeError):
            detr.REFINE_KERNEL = False
            _stretch(contours, engine, infer, outputs, samples, plain, present, args, post, labels_unique=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        lib.count_launches(False)
    assert seen == [(torch.int32, M)] and M >= 2, seen                                  # the counts, and nothing else
    assert counts["spe_cam_targets"] == 1 and counts["spe_refine_pick"] == C.STUB_STAGES - 1 == len(refine), counts
    monkeypatch.undo()
    # the same targets as the composition without the kernels gives
    detr.REFINE_KERNEL = False
    want = _stretch(contours, engine, infer, outputs, samples, [dict(t) for t in plain], present, args, post, labels_unique=False)
    for rf in refine:
        for a, b in zip(refine[rf], want[rf]):
            for k in ("boxes", "labels", "scores"):
                assert np.array_equal(_bits(a[k]), _bits(b[k])), (rf, k)


# ---- the loop --------------------------------------------------------------------------------------------------------------------------
def test_loop_with_kernels_on_and_off_and_twice(dev, contours, detr, capsys):
    on = C.run_stub_epochs(dev)
    again = C.run_stub_epochs(dev)
    detr.REFINE_KERNEL = False
    contours.set_contours("host")
    off = C.run_stub_epochs(dev)
    contours.set_contours("device")
    parent = C.run_parent_epochs(dev)
    capsys.readouterr()
    for other in (again, off, parent):
        assert list(on[0]) == list(other[0]) and len(on[0]) > 20
        for k in on[0]:
            assert np.float64(on[0][k]).view(np.int64) == np.float64(other[0][k]).view(np.int64), (k, on[0][k], other[0][k])
        assert torch.equal(on[1], other[1])
    assert not torch.equal(on[1], torch.tensor([1.0, 0.75])) and all("labels_unique" in keys for step in on[2] + on[3] for keys in step)
