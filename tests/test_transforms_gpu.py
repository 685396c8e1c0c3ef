"""The input-transform kernels (csrc/img_resample.hip) against the numpy restatement (tests/resample_ref.py), and the whole
spe_amd.transforms pipeline + collate_fn against the recorded outputs of the reference (tests/golden/transforms_*.pt).
Everything is integer arithmetic and table lookups after fp64 coefficients in a fixed order, so every comparison is torch.equal."""
import functools
import math

import numpy as np
import pytest
import torch

import resample_cases as cases
import resample_ref as R
from resample_cases import NAMES, load, run_pipeline

pytestmark = pytest.mark.gpu

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
SINGLE = {c[0]: c for c in cases.SINGLE}
BATCHES = dict(cases.BATCHES)


@functools.lru_cache(maxsize=None)
def single_ref(name):
    """(source, box, flip, (oh, ow), restated uint8 output): computed once per case, shared, never written to."""
    _, (h, w), box, flip, out, kind = SINGLE[name]
    box = box or (0, 0, w, h)
    src = cases.fill(kind, h, w, 1 + sorted(SINGLE).index(name))
    return src, box, flip, out, R.run_stages(src, [tuple(box) + (flip,) + tuple(out)])


@functools.lru_cache(maxsize=None)
def batch_ref(name):
    srcs = [cases.fill("rand", h, w, 100 + i) for i, ((h, w), _) in enumerate(BATCHES[name])]
    outs = [R.resize(s, oh, ow) for s, (_, (oh, ow)) in zip(srcs, BATCHES[name])]
    return srcs, outs, R.collate(outs, R.norm_table(MEAN, STD))


def final(dev, jobs, lut, fill=float("nan"), slack=0):
    """The final epilogue into buffers pre-filled with NaN / False, `slack` elements longer than the batch needs."""
    from spe_amd import kernels as K
    B, H, W = len(jobs), max(j[3][0] for j in jobs), max(j[3][1] for j in jobs)
    tb = torch.full((B * 3 * H * W + slack,), fill, device=dev)
    mb = torch.zeros((B * H * W + slack,), device=dev, dtype=torch.bool)
    K.resample_batch(jobs, lut=lut.to(dev), out=tb[:B * 3 * H * W].view(B, 3, H, W), mask=mb[:B * H * W].view(B, H, W))
    return tb, mb, (B, H, W)


@pytest.mark.parametrize("name", sorted(SINGLE))
def test_single_image_both_epilogues(dev, name):
    from spe_amd import kernels as K
    src, box, flip, out, want = single_ref(name)
    job = (torch.from_numpy(src).to(dev), box, flip, out)
    got = K.resample_batch([job])[0]
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    lut = R.norm_table(MEAN, STD)
    tb, mb, (B, H, W) = final(dev, [job], lut, slack=8)
    wt, wm = R.collate([want], lut)
    assert torch.equal(tb[:-8].view(B, 3, H, W).cpu(), wt) and not mb.any()
    assert torch.isnan(tb[-8:]).all()


def test_coefficient_tables(dev):
    """The fp64 tables themselves, read back: first tap, tap count and every 22-bit coefficient, both axes."""
    from spe_amd import kernels as K
    pairs = [((20, 30), (45, 70)), ((50, 45), (30, 27)), ((70, 52), (27, 20)), ((64, 48), (16, 12)), ((64, 8), (2, 8)), ((1, 9), (5, 3)),
             ((37, 41), (11, 13)), ((33, 40), (33, 40))]
    d = torch.zeros((len(pairs), 16), dtype=torch.int64)
    for i, ((h, w), (oh, ow)) in enumerate(pairs):
        d[i, :11] = torch.tensor([4096, w, h, 0, 0, w, h, 0, ow, oh, 0])
    tot = torch.zeros(5, dtype=torch.int64)
    K._call("spe_resample_plan", d.data_ptr(), len(pairs), tot.data_ptr())
    tables = torch.full((int(tot[1]) + 16,), -77, device=dev, dtype=torch.int32)
    K._call("spe_resample_tables", d.data_ptr(), d.to(dev).data_ptr(), len(pairs), tables.data_ptr(), K._st())
    t = tables.cpu().numpy()
    assert (t[-16:] == -77).all()
    for i, ((h, w), (oh, ow)) in enumerate(pairs):
        for off, inS, outS in ((int(d[i, 12]), w, ow), (int(d[i, 13]), h, oh)):
            ks, xmin, cnt, k = R.coeffs(inS, outS)
            assert np.array_equal(t[off:off + outS], xmin) and np.array_equal(t[off + outS:off + 2 * outS], cnt)
            assert np.array_equal(t[off + 2 * outS:off + 2 * outS + outS * ks].reshape(outS, ks), k)


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_padded_batch_owns_every_element(dev, name):
    """Images that differ in both dimensions, every Wmax mod 4: values, 0.0 / True on all padding, nothing beyond the views."""
    srcs, outs, (wt, wm) = batch_ref(name)
    jobs = [(torch.from_numpy(s).to(dev), (0, 0, s.shape[1], s.shape[0]), False, o.shape[:2]) for s, o in zip(srcs, outs)]
    tb, mb, (B, H, W) = final(dev, jobs, R.norm_table(MEAN, STD), slack=13)
    assert W % 4 == int(name[4:]) % 4
    got_t, got_m = tb[:-13].view(B, 3, H, W).cpu(), mb[:-13].view(B, H, W).cpu()
    assert torch.equal(got_m, wm) and torch.equal(got_t, wt)
    for b, o in enumerate(outs):
        h, w = o.shape[:2]
        assert (got_t[b, :, h:, :] == 0).all() and (got_t[b, :, :, w:] == 0).all()
        assert got_m[b, h:, :].all() and got_m[b, :, w:].all() and not got_m[b, :h, :w].any()
    assert torch.isnan(tb[-13:]).all() and not mb[-13:].any()


def test_mixed_stages_in_one_launch(dev):
    """One batch whose images take a crop under a flip, a downscale and an upscale, through the uint8 epilogue."""
    from spe_amd import kernels as K
    names = ["crop_flip", "down_7taps", "up_3taps", "src_w1", "ow_257"]
    refs = [single_ref(n) for n in names]
    got = K.resample_batch([(torch.from_numpy(r[0]).to(dev), r[1], r[2], r[3]) for r in refs])
    for g, r, n in zip(got, refs, names):
        assert torch.equal(g.cpu(), torch.from_numpy(r[4])), n


def test_chained_resize_crop_resize_and_out_buffers(dev):
    """resize -> crop -> resize next to a single resize, B = 2, into caller-owned buffers; then the same call again, bit for bit."""
    from spe_amd import transforms as T
    a, b = cases.fill("rand", 37, 50, 21), cases.fill("rand", 48, 33, 22)
    tf = T.Compose([T.ToTensor(), T.Normalize(MEAN, STD)])

    def samples():
        ia = T.DeviceImage(torch.from_numpy(a), device=dev).hflip().resize(45, 60).crop(4, 6, 30, 41).resize(59, 80)
        ib = T.DeviceImage(torch.from_numpy(b).to(dev)).resize(64, 44)
        return [tf(ia, None), tf(ib, None)]
    wa = R.resize(R.resize(a[:, ::-1], 45, 60)[4:34, 6:47], 59, 80)
    wt, wm = R.collate([wa, R.resize(b, 64, 44)], R.norm_table(MEAN, STD))
    n = wt.numel()
    tb = torch.full((n + 100,), float("nan"), device=dev)
    mb = torch.zeros((wm.numel() + 100,), device=dev, dtype=torch.bool)
    nt, _ = T.collate_fn(samples(), out=(tb, mb))
    assert nt.tensors.data_ptr() == tb.data_ptr() and nt.mask.data_ptr() == mb.data_ptr()
    assert torch.equal(nt.tensors.cpu(), wt) and torch.equal(nt.mask.cpu(), wm)
    assert torch.isnan(tb[n:]).all() and not mb[wm.numel():].any()
    again, _ = T.collate_fn(samples())
    assert torch.equal(again.tensors, nt.tensors) and torch.equal(again.mask, nt.mask)
    with pytest.raises(ValueError):
        T.collate_fn(samples(), out=(tb[:n - 1], mb))


def test_batch_of_one_and_plain_totensor(dev):
    from spe_amd import transforms as T
    a = cases.fill("rand", 19, 26, 23)
    img = T.DeviceImage(torch.from_numpy(a), device=dev)
    nt, tg = T.collate_fn([T.ToTensor()(img.crop(2, 3, 11, 13), {"labels": torch.tensor([1])})])
    wt, wm = R.collate([a[2:13, 3:16]], R.norm_table())
    assert torch.equal(nt.tensors.cpu(), wt) and torch.equal(nt.mask.cpu(), wm) and tg[0]["labels"].tolist() == [1]


@pytest.mark.parametrize("name", NAMES)
def test_pipeline_equals_reference(dev, name):
    """make_transforms + collate_fn from the fixture's seeds: the reference's batch, mask and targets."""
    from spe_amd import transforms as T
    g = load(name)
    nt, targets = T.collate_fn(run_pipeline(g, device=dev))
    assert torch.equal(nt.tensors.cpu(), g["tensors"]) and torch.equal(nt.mask.cpu(), g["mask"])
    for tgt, want in zip(targets, g["targets_out"]):
        assert set(tgt) == set(want) and all(torch.equal(tgt[k], want[k]) for k in want)


@pytest.mark.parametrize("case", cases.BAD, ids=[c[0] for c in cases.BAD])
def test_bad_jobs_raise(dev, case):
    from spe_amd import kernels as K, lib
    _, (h, w), box, out, status = case
    with pytest.raises(lib.SpeLibraryError, match=f"status {status}"):
        K.resample_batch([(torch.zeros((h, w, 3), dtype=torch.uint8, device=dev), box, False, out)])
    torch.cuda.synchronize()


def test_tap_limit_itself(dev):
    from spe_amd import kernels as K
    (h, w), (oh, ow) = cases.TAP_LIMIT_OK
    a = cases.fill("rand", h, w, 31)
    assert math.ceil(h / oh) * 2 + 1 == K.RESAMPLE_MAX_TAPS
    got = K.resample_batch([(torch.from_numpy(a).to(dev), (0, 0, w, h), False, (oh, ow))])[0]
    assert torch.equal(got.cpu(), torch.from_numpy(R.resize(a, oh, ow)))
