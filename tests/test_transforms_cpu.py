"""The input transforms without a GPU: the numpy restatement (tests/resample_ref.py) against the recorded outputs of the
reference's pipeline (tests/golden/transforms_*.pt) and against Pillow itself; the host side of spe_amd.transforms - targets, drawn
sizes and boxes, batch shape, generator states - against the same recordings; the refusals.  Every comparison is exact."""
import random

import numpy as np
import pytest
import torch

import resample_cases as cases
import resample_ref as R

from resample_cases import NAMES, load, run_pipeline


def replay(img, trace):
    """The reference's recorded draws, one materialised step at a time."""
    for t in trace:
        if t[0] == "hflip":
            img = img[:, ::-1]
        elif t[0] == "crop":
            img = img[t[1]:t[1] + t[3], t[2]:t[2] + t[4]]
        else:
            img = R.resize(img, t[1], t[2])
    return img


def test_fixture_covers_every_branch():
    assert len(NAMES) >= 3
    seen = set()
    for n in NAMES:
        g = load(n)
        for tr in g["trace"]:
            names = [t[0] for t in tr]
            seen.add("flip" if "hflip" in names else "noflip")
            seen.add("arm2" if "crop" in names else "arm1")
            seen |= {"crop_equal" for t in tr if t[0] == "crop" and t[5]} | {"crop_drops" for t in tr if t[0] == "crop" and t[6]}
            seen |= {"clamp" for t in tr if t[0] == "resize" and t[3]}
        hw = [tuple(t["size"].tolist()) for t in g["targets_out"]]
        if len({h for h, _ in hw}) > 1 and len({w for _, w in hw}) > 1:
            seen.add("pad_both")
    assert seen == {"flip", "noflip", "arm1", "arm2", "crop_equal", "crop_drops", "clamp", "pad_both"}


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_reference(name):
    g = load(name)
    outs = [replay(im.numpy(), tr) for im, tr in zip(g["images"], g["trace"])]
    t, m = R.collate(outs, R.norm_table(g["mean"], g["std"]))
    assert torch.equal(t, g["tensors"]) and torch.equal(m, g["mask"])


@pytest.mark.parametrize("name", NAMES)
def test_pipeline_host_side_equals_reference(name):
    """Targets, the drawn sizes and boxes (as the planned stages, executed by the restatement), the batch shape, the RNG states."""
    from spe_amd import transforms as T
    g = load(name)
    samples = run_pipeline(g)
    after = (random.getstate(), torch.get_rng_state())
    assert after[0] == g["random_state"] and torch.equal(after[1], g["torch_state"])
    for (_, tgt), want in zip(samples, g["targets_out"]):
        assert set(tgt) == set(want)
        for k in want:
            assert tgt[k].dtype == want[k].dtype and torch.equal(tgt[k], want[k]), k
    pend = [s[0] for s in samples]
    assert T.batch_shape(pend) == tuple(g["tensors"].shape)
    outs = []
    for p, im, tr in zip(pend, g["images"], g["trace"]):
        stages = T.plan_stages(p.image)
        sizes = [(t[1], t[2]) for t in tr if t[0] == "resize"]
        assert [s[5:7] for s in stages][:len(sizes)] == sizes and len(stages) == len(sizes)
        outs.append(R.run_stages(im.numpy(), stages))
    t, m = R.collate(outs, T.norm_table(pend[0].mean, pend[0].std, "cpu"))
    assert torch.equal(t, g["tensors"]) and torch.equal(m, g["mask"])


def test_size_rule():
    from spe_amd.transforms import get_size_with_aspect_ratio as f
    assert f((500, 375), 800, 1333) == (800, 1066)
    assert f((640, 480), 800, 1333) == (800, 1066)
    assert f((64, 24), 60, 100) == (38, 101)               # the clamp, then int(size * w / h) past max_size, as the reference has it
    assert f((375, 500), 375, None) == (500, 375)
    assert f((1000, 300), 800, 1333) == (400, 1333)


def test_lazy_image_views():
    """Crop under a flip, flip after a crop, a crop after the last resize: the index map equals the materialised steps."""
    from spe_amd import transforms as T
    a = cases.fill("rand", 23, 31, 5)
    im = T.DeviceImage(torch.from_numpy(a), device=None)
    assert im.size == (31, 23) and im.width == 31 and im.height == 23
    got = im.hflip().crop(3, 4, 10, 12).hflip().crop(1, 2, 7, 8).hflip()
    want = a[:, ::-1][3:13, 4:16][:, ::-1][1:8, 2:10][:, ::-1]
    st = T.plan_stages(got)
    assert len(st) == 1 and np.array_equal(R.run_stages(a, st), want)
    got = im.resize(30, 40).crop(2, 3, 20, 25)
    assert got.size == (25, 20)
    assert np.array_equal(R.run_stages(a, T.plan_stages(got)), R.resize(a, 30, 40)[2:22, 3:28])
    assert len(T.plan_stages(im.resize(30, 40))) == 1


def test_restatement_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    for name, (h, w), box, flip, (oh, ow), kind in cases.SINGLE:
        a = cases.fill(kind, h, w, 11)
        v = np.ascontiguousarray(R.view(a, box or (0, 0, w, h), flip))
        want = np.asarray(Image.fromarray(v).resize((ow, oh), Image.BILINEAR))
        assert np.array_equal(R.resize(v, oh, ow), want), name
    a = cases.fill("rand", 375, 500, 3)
    assert np.array_equal(R.resize(a, 800, 1066), np.asarray(Image.fromarray(a).resize((1066, 800), Image.BILINEAR)))


def test_errors():
    from spe_amd import lib, transforms as T
    img = T.DeviceImage(torch.zeros((8, 9, 3), dtype=torch.uint8), device=None)
    tgt = {"boxes": torch.tensor([[1., 1., 4., 4.]]), "labels": torch.tensor([1]), "area": torch.tensor([9.]),
           "iscrowd": torch.tensor([0])}
    t, tg = T.ToTensor()(img, tgt)
    for tf in (T.RandomHorizontalFlip(1.0), T.Resize(4, 8), T.RandomResize([4]), T.RandomCrop((2, 2)), T.RandomSizeCrop(2, 3),
               T.CenterCrop((2, 2)), T.ToTensor()):
        with pytest.raises(TypeError):
            tf(t, tg)
    with pytest.raises(TypeError):
        T.Normalize([0, 0, 0], [1, 1, 1])(img, tgt)
    with pytest.raises(TypeError):
        T.DeviceImage(torch.zeros((3, 8, 9), dtype=torch.float32), device=None)
    masks = dict(tgt, masks=torch.zeros((1, 8, 9), dtype=torch.bool))
    for tf in (T.RandomHorizontalFlip(1.0), T.Resize(4, 8), T.CenterCrop((2, 2))):
        with pytest.raises(NotImplementedError):
            tf(img, masks)
    assert not hasattr(T, "RandomPad") and not hasattr(T, "RandomErasing")
    with pytest.raises(ValueError):
        T.make_transforms("test")
    # a host tensor reaching the kernels fails loudly
    sample = T.make_transforms("val", max_size=100)(img, tgt)
    with pytest.raises(lib.SpeLibraryError):
        T.collate_fn([sample])


def _desc(src_hw, box, out_hw):
    d = torch.zeros((1, 16), dtype=torch.int64)
    d[0, :11] = torch.tensor([4096, src_hw[1], src_hw[0], box[0], box[1], box[2], box[3], 0, out_hw[1], out_hw[0], 4096])
    return d


@pytest.mark.parametrize("case", cases.BAD, ids=[c[0] for c in cases.BAD])
def test_bad_descriptors_are_refused_before_any_launch(case):
    """Status codes of the host-side validation; with a bad descriptor no entry point reaches its launch (there is no GPU here)."""
    from spe_amd import kernels as K, lib
    _, src, box, out, status = case
    d, tot = _desc(src, box, out), torch.zeros(5, dtype=torch.int64)
    l = lib.load()
    assert l.spe_resample_plan(d.data_ptr(), 1, tot.data_ptr()) == status
    assert l.spe_resample_tables(d.data_ptr(), None, 1, None, None) == status
    assert l.spe_resample_h(d.data_ptr(), None, 1, None, None, None) == status
    assert l.spe_resample_v(d.data_ptr(), None, 1, None, None, None, None, None, 0, 0, None) == status
    assert status != -5 or K.RESAMPLE_MAX_TAPS == 65


def test_plan_offsets_and_tap_limit():
    from spe_amd import kernels as K, lib
    (sh, sw), (oh, ow) = cases.TAP_LIMIT_OK
    d = torch.cat([_desc((sh, sw), (0, 0, sw, sh), (oh, ow)), _desc((20, 30), (1, 2, 10, 8), (5, 7))])
    tot = torch.zeros(5, dtype=torch.int64)
    assert lib.load().spe_resample_plan(d.data_ptr(), 2, tot.data_ptr()) == 0
    ky, kx = R.coeffs(sh, oh)[0], R.coeffs(sw, ow)[0]
    assert ky == K.RESAMPLE_MAX_TAPS and d[0, 11:].tolist() == [0, 0, ow * (2 + kx), kx, ky]
    tmp0, tab0 = 3 * sh * 8, ow * (2 + kx) + oh * (2 + ky)
    assert d[1, 11:].tolist() == [tmp0, tab0, tab0 + 7 * 7, 5, 5]
    assert tot.tolist() == [tmp0 + 3 * 8 * 8 + 16, tab0 + 7 * 7 + 5 * 7, 8, 5, sh]
    # a launcher refuses descriptors that were not planned
    d[1, 11] += 4
    assert lib.load().spe_resample_h(d.data_ptr(), None, 2, None, None, None) == -2
