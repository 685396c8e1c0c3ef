"""The CAM pseudo boxes found on the device (csrc/cambox_labels.hip, spe_cam_boxes_device): exact equality with the border walks
it replaces - oracle/cam_oracle.py on the small cases of tests/cambox_cases.py, the native host walk (csrc/cambox.hip) on the
full-size map - at area ratios 0, 0.5 and 1; batching, reproducibility, the overflow status, and the three drivers of
spe_amd/camboxes.py on both contour paths."""
import argparse
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cambox_cases as cc  # noqa: E402
from oracle import cam_oracle as CO  # noqa: E402

pytestmark = pytest.mark.gpu
SMALL = cc.small_cases()
BY_NAME = dict(SMALL)
GUARD, FILL = 64, -7777


@functools.lru_cache(maxsize=None)
def _walked(name, ratio):
    """the reference of a small case, computed once and shared"""
    return CO.multi_bboxes_from_image(BY_NAME[name], ratio)


@functools.lru_cache(maxsize=None)
def _full():
    from spe_amd import kernels as K
    name, img = cc.full_size_case()
    t = torch.from_numpy(img)
    return img, {r: K.cam_contour_boxes(t, r, max_boxes=8192).tolist() for r in cc.RATIOS}


def _raw(dev, imgs, ratio, max_boxes):
    """spe_cam_boxes_device on buffers this test owns, pre-filled, with a guard band behind boxes[M][max_boxes] ->
    (nboxes [M], boxes [M, max_boxes, 4], guard) on the host"""
    from spe_amd import kernels as K, lib
    t = torch.from_numpy(np.stack(imgs)).to(dev)
    M, rows, cols = t.shape
    boxes = torch.full((M * max_boxes * 4 + GUARD,), FILL, device=dev, dtype=torch.int32)
    nb = torch.full((M + GUARD,), FILL, device=dev, dtype=torch.int32)
    nbytes = K.cam_boxes_workspace_bytes(M, rows, cols)
    assert nbytes == M * (7 * (((rows + 2) * (cols + 2) + 3) // 4 * 4) + 4 + 6 * 2048) * 4          # the formula of include/spe_hip.h
    ws = torch.empty((nbytes // 4,), device=dev, dtype=torch.int32)
    lib.call("spe_cam_boxes_device", t.data_ptr(), M, rows, cols, float(ratio), ws.data_ptr(), nbytes, boxes.data_ptr(),
             nb.data_ptr(), max_boxes, torch.cuda.current_stream().cuda_stream)
    boxes, nb = boxes.cpu(), nb.cpu()
    assert (nb[M:] == FILL).all()
    return nb[:M], boxes[:M * max_boxes * 4].view(M, max_boxes, 4), boxes[M * max_boxes * 4:]


def _device_boxes(dev, imgs, ratio, max_boxes=2048):
    from spe_amd import kernels as K
    t = torch.from_numpy(np.stack(imgs)).to(dev)
    boxes, nb = K.cam_boxes_device(t, ratio, max_boxes)
    assert boxes.is_cuda and nb.is_cuda and boxes.shape == (len(imgs), max_boxes, 4) and boxes.dtype == nb.dtype == torch.int32
    boxes, nb = boxes.cpu(), nb.cpu()
    assert (nb > 0).all(), nb
    return [boxes[m, :int(nb[m])].tolist() for m in range(len(imgs))]


@pytest.mark.parametrize("name", [n for n, _ in SMALL])
def test_boxes_equal_the_border_walk(dev, name):
    for ratio in cc.RATIOS:
        assert _device_boxes(dev, [BY_NAME[name]], ratio) == [_walked(name, ratio)], ratio


def test_full_size_equals_the_native_walk(dev):
    img, want = _full()
    for ratio in cc.RATIOS:
        assert len(want[ratio]) <= 2048
        assert _device_boxes(dev, [img], ratio) == [want[ratio]], ratio


def test_batched_maps_equal_single_maps(dev):
    """all cases of one size in one call: no map leaks into another"""
    groups = {}
    for n, im in SMALL:
        groups.setdefault(im.shape, []).append(n)
    groups = {s: ns for s, ns in groups.items() if len(ns) > 1}
    assert (37, 71) in groups and (5, 7) in groups
    for shape, names in groups.items():
        names = names + names[:1]                      # and the same map twice
        for ratio in cc.RATIOS:
            assert _device_boxes(dev, [BY_NAME[n] for n in names], ratio) == [_walked(n, ratio) for n in names], (shape, ratio)
    img, want = _full()                                 # full size: three maps, the middle one empty
    got = _device_boxes(dev, [img, np.zeros_like(img), img[::-1].copy()], 0.5)
    assert got[0] == want[0.5] and got[1] == [[0, 0, 1, 1]]
    assert got[2] == _device_boxes(dev, [img[::-1].copy()], 0.5)[0]


def test_two_runs_are_bitwise_equal(dev):
    img, _ = _full()
    for imgs, ratio in (([img, img.T.copy().reshape(img.shape)], 0.0), ([BY_NAME[f"noise{d}"] for d in (20, 50, 80, 95)], 0.0),
                        ([BY_NAME["comb"]], 0.5)):
        a, b = _raw(dev, imgs, ratio, 2048), _raw(dev, imgs, ratio, 2048)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert (a[0] > 0).all()


def test_overflow_is_status_minus_5_and_stays_inside_the_buffers(dev):
    chk = BY_NAME["checkerboard"]
    n_all = len(_walked("checkerboard", 0.0))
    assert n_all > 8
    nb, boxes, guard = _raw(dev, [chk, np.zeros_like(chk), chk], 0.0, 8)
    assert nb.tolist() == [-5, 1, -5]
    assert (guard == FILL).all()
    assert (boxes[0] == FILL).all() and (boxes[2] == FILL).all()                    # an overflowing map writes no row
    assert boxes[1, 0].tolist() == [0, 0, 1, 1] and (boxes[1, 1:] == FILL).all()
    nb, boxes, guard = _raw(dev, [chk], 0.0, n_all)                                 # exactly full: fine
    assert nb.tolist() == [n_all] and boxes[0].tolist() == _walked("checkerboard", 0.0) and (guard == FILL).all()
    nb, boxes, guard = _raw(dev, [chk], 0.0, n_all - 1)                             # one short
    assert nb.tolist() == [-5] and (boxes == FILL).all() and (guard == FILL).all()


def test_bad_arguments_are_refused(dev):
    from spe_amd import kernels as K, lib
    t = torch.zeros((1, 4, 4), dtype=torch.uint8, device=dev)
    for mb in (0, 2049):
        with pytest.raises(lib.SpeLibraryError, match="status -2"):
            K.cam_boxes_device(t, 0.5, mb)
    ws = torch.empty((16,), device=dev, dtype=torch.int32)
    out = torch.empty((64,), device=dev, dtype=torch.int32)
    with pytest.raises(lib.SpeLibraryError, match="status -4"):
        lib.call("spe_cam_boxes_device", t.data_ptr(), 1, 4, 4, 0.5, ws.data_ptr(), 64, out.data_ptr(), out.data_ptr(), 4,
                 torch.cuda.current_stream().cuda_stream)
    with pytest.raises(lib.SpeLibraryError):
        K.cam_boxes_device(t.cpu(), 0.5)
    boxes, nb = K.cam_boxes_device(t[:0], 0.5)
    assert boxes.shape == (0, 256, 4) and nb.shape == (0,)


# ------------------------------------------------------------------------------------------------ drivers
@pytest.fixture
def contours():
    from spe_amd import camboxes
    assert camboxes.get_contours() == "device"          # the default
    yield camboxes
    camboxes.set_contours("device")


def _driver_inputs(dev):
    """the inputs of tests/test_kernels_gpu.py::test_cam_to_boxes_vs_oracle"""
    g = torch.Generator().manual_seed(12)
    B, Kc, h, w, H, W = 2, 5, 9, 13, 144, 208
    cams = torch.zeros(B, Kc, h, w)
    for b in range(B):
        for c in range(Kc):
            for _ in range(2):
                cy, cx = torch.rand(2, generator=g) * torch.tensor([h - 1.0, w - 1.0])
                yy, xx = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
                cams[b, c] += torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * (1.0 + 2 * torch.rand(1, generator=g)) ** 2))
    cams += 0.05 * torch.randn(cams.shape, generator=g)
    labels = torch.zeros(B, Kc, dtype=torch.int64); labels[0, [0, 3]] = 1; labels[1, [1, 2, 4]] = 1
    targets = [{"img_label": labels[b].to(dev), "label": labels[b].to(dev)} for b in range(B)]
    args = argparse.Namespace(num_classes=Kc, cam_thr=0.2, multi_box_ratio=0.5)
    return cams, labels, targets, args, torch.zeros(B, 3, H, W, device=dev)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x["boxes"], y["boxes"]) and torch.equal(x["labels"], y["labels"])
        assert x["boxes"].dtype == torch.float32 and x["labels"].dtype == torch.int64 and x["boxes"].is_cuda


def test_device_and_host_contours_give_equal_pseudo_labels(dev, contours):
    cams, labels, targets, args, samples = _driver_inputs(dev)
    out = {"cams_cls": cams.to(dev)}
    for fn in (contours.get_pseudo_label_multi_boxes, contours.get_pseudo_label, contours.get_pseudo_label_multi_boxes_voc):
        contours.set_contours("device")
        a = fn(out, samples, targets, args)
        contours.set_contours("host")
        b = fn(out, samples, targets, args)
        _same(a, b)
        assert sum(x["boxes"].shape[0] for x in a) >= 5
    with pytest.raises(ValueError):
        contours.set_contours("cv2")


def test_single_box_and_voc_drivers_vs_the_reference_loops(dev, contours):
    """engine.py:312-352 and :402-444 restated on the oracle functions, from the thresholded images the device produced (which
    isolates the box logic, as in test_cam_to_boxes_vs_oracle)"""
    from spe_amd import kernels as K
    cams, labels, targets, args, samples = _driver_inputs(dev)
    args.multi_box_ratio = 0.05                         # neither driver reads it
    B, Kc, h, w = cams.shape
    H, W = samples.shape[-2:]
    imgs = K.cam_prepare(cams.view(-1, h, w).to(dev), W, H, args.cam_thr).cpu().numpy()
    scale = torch.tensor([W, H, W, H], dtype=torch.float32)
    single = contours.get_pseudo_label({"cams_cls": cams.to(dev)}, samples, targets, args)
    voc = contours.get_pseudo_label_multi_boxes_voc({"cams_cls": cams.to(dev)}, samples, targets, args)
    for b in range(B):
        sb, sl, vb, vl = [], [], [], []
        for c in range(Kc):
            if labels[b, c] > 0:
                bs = CO.find_borders(imgs[b * Kc + c])
                if bs:                                                  # get_bboxes: max(contours, key=contourArea), first maximum
                    _, x0, y0, x1, y1 = max(bs, key=lambda t: t[0])
                    box = torch.tensor([x0, y0, x1 + 1, y1 + 1])
                else:
                    box = torch.tensor([0, 0, 1, 1])
                x0, y0, x1, y1 = box
                sb.append(torch.stack([(x0 + x1) / 2, (y0 + y1) / 2, (x1 - x0), (y1 - y0)], dim=-1)); sl.append(c + 1)
                mb = torch.tensor(CO.multi_bboxes_from_image(imgs[b * Kc + c], 0.5))   # get_multi_bboxes' default ratio
                x0, y0, x1, y1 = mb[..., 0], mb[..., 1], mb[..., 2], mb[..., 3]
                vb.append(torch.stack([(x0 + x1) / 2, (y0 + y1) / 2, (x1 - x0), (y1 - y0)], dim=-1)); vl += [c + 1] * mb.shape[0]
        assert torch.equal(single[b]["boxes"].cpu(), torch.stack(sb) / scale) and single[b]["labels"].tolist() == sl
        assert torch.equal(voc[b]["boxes"].cpu(), torch.cat(vb, 0) / scale) and voc[b]["labels"].tolist() == vl
        assert single[b]["boxes"].shape == (len(sl), 4)
    none = [{"img_label": torch.zeros(Kc, dtype=torch.int64, device=dev)} for _ in range(B)]
    empty = contours.get_pseudo_label({"cams_cls": cams.to(dev)}, samples, none, args)   # the reference raises here
    assert all(e["boxes"].shape == (0, 4) and e["labels"].shape == (0,) for e in empty)


def test_no_image_crosses_to_the_host_on_the_device_path(dev, contours, monkeypatch):
    cams, labels, targets, args, samples = _driver_inputs(dev)
    H, W = samples.shape[-2:]
    M = int(labels.sum())
    seen = []
    real = torch.Tensor.cpu

    def spy(self, *a, **k):
        if self.is_cuda:
            seen.append((self.dtype, tuple(self.shape)))
        return real(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "cpu", spy)
    contours.get_pseudo_label_multi_boxes({"cams_cls": cams.to(dev)}, samples, targets, args)
    big = [s for s in seen if int(np.prod(s[1])) >= 64]
    assert big == [(torch.int32, (M * (1 + 4 * contours.MAX_BOXES),))], seen      # counts and boxes in one piece, nothing else
    assert all(dt != torch.uint8 for dt, _ in seen)
    seen.clear()
    contours.set_contours("host")                       # the spy does see an image copy where there is one
    contours.get_pseudo_label_multi_boxes({"cams_cls": cams.to(dev)}, samples, targets, args)
    assert (torch.uint8, (M, W, H)) in seen


def test_overflow_raises_with_the_host_paths_text(dev, contours, monkeypatch):
    monkeypatch.setattr(contours, "MAX_BOXES", 8)
    from spe_amd.lib import SpeLibraryError
    t = torch.from_numpy(np.stack([BY_NAME["all_zero"], BY_NAME["all_ones"]])).to(dev)
    assert [b.tolist() for b in contours._map_boxes(t, 0.0)] == [[[0, 0, 1, 1]], [[0, 0, 7, 5]]]
    t = torch.from_numpy(BY_NAME["checkerboard"][None]).to(dev)
    for mode in ("device", "host"):
        contours.set_contours(mode)
        with pytest.raises(SpeLibraryError, match="status -5"):
            contours._map_boxes(t, 0.0)
