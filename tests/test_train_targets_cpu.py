"""Host side of the training targets: spe_amd.infer.refine_targets and PostProcessRefine on CPU tensors against
the numpy restatement (tests/train_targets_ref.py), the restatement of the row assembly against the drivers' own host arithmetic, the
argument checks of the two entry points (host returns: nothing is launched), and the training loop on a stub model with CPU tensors."""
import numpy as np
import pytest
import torch

import train_targets_cases as C
import train_targets_ref as R


def _bits(t):
    return t.contiguous().view(torch.int32).numpy() if t.dtype == torch.float32 else t.numpy()


@pytest.mark.parametrize("kind", C.PICK_INPUTS)
@pytest.mark.parametrize("B,Q,Kc", C.PICK_SHAPES)
def test_refine_targets_host_equals_restatement(B, Q, Kc, kind):
    from spe_amd import infer
    logits, boxes = C.pick_logits(kind, B, Q, Kc), C.pick_boxes(B, Q)
    prob = logits.sigmoid().numpy()
    for table in C.PICK_TABLES:
        classes = C.pick_classes(table, B, Kc)
        got = infer.refine_targets({"pred_logits": logits, "pred_boxes": boxes}, classes)
        scores, queries, rows, labels, off = R.refine_pick(prob, boxes.numpy(), classes)
        assert got["offsets"] == off and got["labels"].dtype == torch.int64 and got["queries"].dtype == torch.int32
        assert np.array_equal(_bits(got["scores"]), scores) and np.array_equal(got["queries"].numpy(), queries)
        assert np.array_equal(_bits(got["boxes"]).reshape(-1, 4), rows) and np.array_equal(got["labels"].numpy(), labels)


def test_the_inputs_hold_what_they_are_named_for():
    """ties: several queries share the best probability with different logits; free: none do; nan: a NaN wins a column."""
    for B, Q, Kc in C.PICK_SHAPES:
        for kind in C.PICK_INPUTS:
            x = C.pick_logits(kind, B, Q, Kc)
            p = x.sigmoid()
            top = p.max(dim=1, keepdim=True).values
            shared = ((p == top).sum(1) > 1)
            if kind in C.TIE_FREE:
                assert not shared.any() and not torch.isnan(p).any()
            elif kind == "ties" and Q >= 2:
                assert shared.all()
                q = (p == top).float().argmax(1)
                assert (x.gather(1, q[:, None]).squeeze(1) < x.max(1).values).any() or Q < 3      # a pick by logit would differ
            elif kind in ("nan1", "nans"):
                assert torch.isnan(top).any()
            elif kind == "inf" and Q >= 2 and Kc >= 2:
                assert shared.all() and (top == 0).any() and (top == 1).any()


def test_postprocess_refine_with_and_without_labels_unique():
    from spe_amd.models.conditional_detr import PostProcessRefine
    B, Q, Kc = 3, 300, 91
    logits, boxes = C.pick_logits("ties", B, Q, Kc), C.pick_boxes(B, Q)
    classes = C.pick_classes("empty_one", B, Kc)
    g = torch.Generator().manual_seed(3)
    targets = []
    for cl in classes:                                                       # labels with repeats, out of order, and ids >= Kc that are dropped
        lab = torch.tensor(cl + cl[:2] + [Kc, Kc + 7], dtype=torch.int64)
        targets.append({"labels": lab[torch.randperm(lab.numel(), generator=g)]})
    sizes = torch.tensor([[480, 640]] * B)
    out = {"pred_logits": logits, "pred_boxes": boxes}
    plain = PostProcessRefine()(out, sizes, targets)
    with_u = PostProcessRefine()(out, sizes, [{**t, "labels_unique": torch.tensor(cl, dtype=torch.int64)} for t, cl in zip(targets, classes)])
    for a, b, cl in zip(plain, with_u, classes):
        assert a["labels"].tolist() == cl
        for k in ("scores", "labels", "boxes"):
            assert a[k].dtype == b[k].dtype and np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_class_table_views_know_their_table():
    from spe_amd import infer
    t = infer.ClassTable([[1, 4], [], [2]], "cpu")
    views = t.per_image()
    assert [v.tolist() for v in views] == [[1, 4], [], [2]] and t.off == [0, 2, 2, 3]
    assert infer.ClassTable.of(views, "cpu") is t
    assert infer.ClassTable.of(views[:2], "cpu") is not t                    # another batch: a table of its own
    other = infer.ClassTable.of([torch.tensor([5]), torch.tensor([], dtype=torch.int64)], "cpu")
    assert other.lists == [[5], []] and other.off == [0, 1, 1]


def test_row_restatement_equals_the_drivers_host_arithmetic():
    """tests/train_targets_ref.cam_targets against the torch operations of spe_amd.camboxes._pseudo_labels, on every (W, H) of the cases."""
    from spe_amd import camboxes
    for W, H in C.CAM_SIZES:
        M, mb = 257, 4
        counts, boxes, cls0 = C.cam_counts("edges", M, mb), C.cam_boxes(M, mb, W, H), C.cam_classes(M)
        rows, labels, off = R.cam_targets(counts, boxes, cls0, False, W, H)
        scale = torch.tensor([W, H, W, H], dtype=torch.float32)
        want = torch.cat([camboxes._xyxy_to_cxcywh(torch.from_numpy(boxes[m, :counts[m]]).to(torch.int64)) for m in range(M)]).float() / scale
        assert torch.equal(torch.from_numpy(rows), want) and off[-1] == want.shape[0] == labels.shape[0]
        assert (np.float32(boxes[..., 0] + boxes[..., 2]) / np.float32(2) != np.floor(np.float32(boxes[..., 0] + boxes[..., 2]) / np.float32(2))).any()
        single = R.cam_targets(counts, boxes, cls0, True, W, H)
        assert single[2][-1] == int((counts > 0).sum()) and np.array_equal(single[1], (cls0[counts > 0] + 1).astype(np.int64))


def test_entry_points_refuse_on_the_host():
    """The launchers look at sizes and host tables before anything is launched: status -2 for a limit, -3 for arguments."""
    import ctypes
    from spe_amd import lib
    L = lib.load()
    one = ctypes.c_void_p(256)                                               # a non-NULL, aligned address that is never touched
    ct = lambda *a: L.spe_cam_targets(one, one, *a, one, one, one, None)
    assert ct(65536, 4, 0, 100, 100, 1 << 30) == -2 and ct(4, 2049, 0, 100, 100, 1 << 30) == -2
    assert ct(4, 4, 0, 100, 100, 15) == -3 and ct(4, 4, 1, 100, 100, 3) == -3              # cap below the worst case
    assert ct(-1, 4, 0, 100, 100, 16) == -3 and ct(4, 0, 0, 100, 100, 16) == -3 and ct(4, 4, 0, 0, 100, 16) == -3 and ct(4, 4, 0, 100, 0, 16) == -3
    assert L.spe_cam_targets(one, one, 4, 4, 0, 100, 100, 16, ctypes.c_void_p(260), one, one, None) == -3      # misaligned rows
    assert L.spe_cam_targets(None, one, 4, 4, 0, 100, 100, 16, one, one, one, None) == -3
    assert L.spe_cam_targets(None, None, 0, 4, 0, 100, 100, 0, None, None, None, None) == -3          # even without a map: off[0] is written

    def rp(cls, off, B, Q, Kc):
        hc, ho = np.asarray(cls, np.int32), np.asarray(off, np.int32)
        return L.spe_refine_pick(one, one, one, one, hc.ctypes.data, ho.ctypes.data, B, Q, Kc, len(cls), one, one, one, None)
    assert rp([0, 5], [0, 1, 2], 2, 10, 5) == -3 and rp([-1], [0, 1], 1, 10, 5) == -3      # class ids outside [0, Kc)
    assert rp([0, 1], [0, 2, 1], 2, 10, 5) == -3 and rp([0, 1], [1, 1, 2], 2, 10, 5) == -3 and rp([0, 1], [0, 1, 1], 2, 10, 5) == -3
    assert rp([0], [0, 1], 1, 0, 5) == -3 and rp([0], [0, 1], 1, 10, 0) == -3
    assert rp([], [0, 0, 0], 2, 10, 5) == 0                                                # U = 0: valid, nothing to do
    assert L.spe_abi_version() == 7


@pytest.fixture
def host_contours(monkeypatch):
    """The "host" contours with a stand-in for the device's prepare step: CPU tensors have no resize kernel; what the maps become is
    not the subject here, only that both loops see the same."""
    from spe_amd import camboxes

    def prepare(maps, rows, cols, cam_thr):
        big = torch.nn.functional.interpolate(maps[:, None], size=(rows, cols), mode="bilinear", align_corners=False)[:, 0]
        lo, hi = big.amin((1, 2), keepdim=True), big.amax((1, 2), keepdim=True)
        q = ((big - lo) / (hi - lo) * 255).to(torch.uint8)
        return torch.where(q > int(cam_thr * 255), q, torch.zeros_like(q))
    monkeypatch.setattr(camboxes.K, "cam_prepare", prepare)
    camboxes.set_contours("host")
    yield camboxes
    camboxes.set_contours("device")


def test_loop_attaches_labels_unique_and_keeps_its_statistics(host_contours, capsys):
    cpu = torch.device("cpu")
    stats, params, seen, seen_r = C.run_stub_epochs(cpu)
    want_stats, want_params = C.run_parent_epochs(cpu)
    capsys.readouterr()
    assert all("labels_unique" in keys for step in seen + seen_r for keys in step)
    assert all("scores" in keys for step in seen_r for keys in step) and len(seen_r) == 2 * 3 * (C.STUB_STAGES - 1)
    assert list(stats) == list(want_stats) and len(stats) > 20
    for k in stats:
        assert np.float64(stats[k]).view(np.int64) == np.float64(want_stats[k]).view(np.int64), (k, stats[k], want_stats[k])
    assert torch.equal(params, want_params) and not torch.equal(params, torch.tensor([1.0, 0.75]))


def test_pseudo_targets_host_path_equals_the_driver(host_contours):
    import argparse
    from spe_amd.util.misc import NestedTensor
    cams = C.cam_maps(2, 5, 9, 13)
    present = [[1, 0, 0, 1, 0], [0, 0, 0, 0, 0]]
    samples = NestedTensor(torch.zeros(2, 3, C.STUB_H, C.STUB_W), None)
    targets = [{"img_label": torch.tensor(p)} for p in present]
    for single, fn in ((False, host_contours.get_pseudo_label_multi_boxes), (True, host_contours.get_pseudo_label)):
        args = argparse.Namespace(num_classes=5, cam_thr=0.2, multi_box_ratio=0.5)
        pt = host_contours.pseudo_targets({"cams_cls": cams}, samples, present, 5, 0.2, 1.0 if single else 0.5, single=single)
        want = fn({"cams_cls": cams}, samples, targets, args)
        assert pt.classes == [[1, 4], []] and pt.offsets[0] == 0 and pt.offsets[-1] == pt.boxes.shape[0]
        for a, b in zip(pt.per_image(), want):
            assert torch.equal(a["boxes"], b["boxes"]) and torch.equal(a["labels"], b["labels"])
