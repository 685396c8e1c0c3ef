"""The device half of the JPEG decoder (csrc/jpeg_decode.hip) behind spe_amd.jpeg: against Pillow's recorded decodes
(tests/golden/jpeg_small.pt, jpeg_voc.pt) and the numpy restatement (tests/jpeg_ref.py).  Integer arithmetic throughout: every
comparison is torch.equal."""
import functools
import hashlib

import numpy as np
import pytest
import torch

import jpeg_cases as C
import jpeg_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def small():
    """{name: (file bytes, Pillow's RGB)}: loaded once, shared, never written to."""
    return {k: (v["data"].numpy().tobytes(), v["rgb"]) for k, v in C.load("jpeg_small").items()}


@functools.lru_cache(maxsize=None)
def coefficients():
    from spe_amd import jpeg as J
    return {k: J.entropy_decode(d) for k, (d, _) in small().items()}


@pytest.mark.parametrize("name", C.SMALL_NAMES)
def test_case_equals_pillow(dev, name):
    from spe_amd import jpeg as J
    got = J.reconstruct([coefficients()[name]], dev)[0]
    want = small()[name][1]
    assert got.dtype == torch.uint8 and got.is_contiguous() and got.shape == want.shape
    assert torch.equal(got.cpu(), want)


def test_all_cases_in_one_batch(dev):
    """Mixed sizes, all three samplings and grayscale images in one launch pair; and the whole thing twice, bitwise equal."""
    from spe_amd import jpeg as J
    from spe_amd import lib
    names = C.SMALL_NAMES
    lib.count_launches(True)
    got = J.reconstruct([coefficients()[n] for n in names], dev)
    counts = lib.count_launches(False)
    assert {k: v for k, v in counts.items() if "jpeg" in k or "resample" in k} == {"spe_jpeg_reconstruct": 1}
    for n, g in zip(names, got):
        assert torch.equal(g.cpu(), small()[n][1]), n
    again = J.decode_batch([small()[n][0] for n in names], dev)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


def test_guard_bytes_keep_their_fill(dev):
    """Every image at its own byte offset inside one buffer (all four alignments occur), 5 .. 8 guard bytes before and after."""
    from spe_amd import kernels as K
    names = C.SMALL_NAMES
    cs = [coefficients()[n] for n in names]
    sizes = [c.info.width * c.info.height * 3 for c in cs]
    starts, p = [], 0
    for i, s in enumerate(sizes):
        p += 5 + i % 4
        starts.append(p)
        p += s
    buf = torch.full((p + 8,), 0xA5, device=dev, dtype=torch.uint8)
    assert {(buf.data_ptr() + s) % 4 for s in starts} == {0, 1, 2, 3}
    packed = torch.cat([c.record for c in cs]).to(dev)
    offs = np.cumsum([0] + [c.record.numel() for c in cs])[:-1]
    K.jpeg_reconstruct([c.info.frame + (int(o),) for c, o in zip(cs, offs)], packed, dsts=[buf[s:s + n] for s, n in zip(starts, sizes)])
    host = buf.cpu()
    inside = torch.zeros_like(host, dtype=torch.bool)
    for n, s, size in zip(names, starts, sizes):
        assert torch.equal(host[s:s + size], small()[n][1].reshape(-1)), n
        inside[s:s + size] = True
    assert (host[~inside] == 0xA5).all()


def test_voc_sized_file(dev):
    from spe_amd import jpeg as J
    g = C.load("jpeg_voc")
    data = g["data"].numpy().tobytes()
    co = J.entropy_decode(data)
    got = J.reconstruct([co], dev)[0].cpu()
    info = R.parse(data)
    want = R.back(info, [co.component(c).numpy() for c in range(3)])           # the restatement's back half on the same coefficients
    assert torch.equal(got, torch.from_numpy(want))
    assert hashlib.sha256(got.numpy().tobytes()).digest() == g["sha256"].numpy().tobytes()


def test_pipeline_from_file_bytes(dev):
    """decode_jpeg -> Resize -> ToTensor -> Normalize -> collate_fn equals the same pipeline fed with Pillow's RGB."""
    from spe_amd import transforms as T
    names = ["37x45_420_noise", "40x48_422_white", "31x64_444_smooth", "17x33_gray_noise"]
    tf = T.Compose([T.Resize(24, max_size=40), T.ToTensor(), T.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])])
    imgs = T.decode_jpeg([small()[n][0] for n in names], device=dev)
    assert [im.size for im in imgs] == [(small()[n][1].shape[1], small()[n][1].shape[0]) for n in names]
    got, _ = T.collate_fn([tf(im, None) for im in imgs])
    want, _ = T.collate_fn([tf(T.DeviceImage(small()[n][1], device=dev), None) for n in names])
    assert torch.equal(got.tensors, want.tensors) and torch.equal(got.mask, want.mask)


def test_bad_descriptor_launches_nothing(dev):
    from spe_amd import kernels as K
    from spe_amd import lib
    cs = [coefficients()[n] for n in ("17x33_420_noise", "16x16_422_smooth")]
    packed = torch.cat([c.record for c in cs]).to(dev)
    offs = [0, cs[0].record.numel()]
    nb = [c.info.nblocks for c in cs]
    dsts = [torch.full((c.info.height, c.info.width, 3), 0x5A, device=dev, dtype=torch.uint8) for c in cs]
    planes = torch.full((64 * sum(nb),), 0x5A, device=dev, dtype=torch.uint8)
    good = torch.zeros((2, 16), dtype=torch.int64)
    for i, c in enumerate(cs):
        good[i, :10] = torch.tensor(c.info.frame + (offs[i], 64 * sum(nb[:i]), dsts[i].data_ptr()))
    fn = lib.load().spe_jpeg_reconstruct

    def call(desc, n=2, coef_elems=packed.numel(), planes_bytes=planes.numel(), coef_ptr=packed.data_ptr()):
        return fn(desc.data_ptr(), desc.to(dev).data_ptr(), n, coef_ptr, coef_elems, planes.data_ptr(), planes_bytes, K._st())
    edits = {"W = 0": (0, 0, 0), "W above the limit": (0, 0, 32769), "two components": (1, 2, 2), "sampling 1x2": (0, 3, 1),
             "sampling 3x1": (0, 3, 3), "grey with 2x1": None, "MCUs across too few": (0, 5, 1), "MCUs down too many": (1, 6, 3),
             "record misaligned": (1, 7, offs[1] + 4), "record overlaps the one before": (1, 7, offs[1] - 8),
             "record past the buffer": (1, 7, offs[1] + 8), "planes misaligned": (1, 8, 64 * nb[0] + 8),
             "planes overlap": (1, 8, 64 * nb[0] - 16), "planes past the buffer": (1, 8, 64 * nb[0] + 16), "no destination": (0, 9, 0)}
    for what, e in edits.items():
        d = good.clone()
        if e is None:
            d[1, 2] = 1
        else:
            d[e[0], e[1]] = e[2]
        assert call(d) == -2, what
    assert call(good, n=0) == -2 and call(good, n=65536) == -2
    assert call(good, coef_elems=packed.numel() - 1) == -2 and call(good, planes_bytes=planes.numel() - 1) == -2
    assert call(good, coef_ptr=packed.data_ptr() + 2) == -2
    torch.cuda.synchronize()
    assert all((t == 0x5A).all() for t in dsts + [planes])
    assert call(good) == 0                                                       # and the table they were derived from is fine
    want = [small()[n][1] for n in ("17x33_420_noise", "16x16_422_smooth")]
    assert all(torch.equal(t.cpu(), w) for t, w in zip(dsts, want))
