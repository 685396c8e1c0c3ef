"""Baseline JPEG decoding without a GPU: the numpy restatement (tests/jpeg_ref.py) against Pillow's recorded decodes and, where Pillow
imports, against Pillow itself on the full grid; the C host pass (csrc/jpeg_entropy.h) against the restatement's front half; every
refusal; decode_batch's fallback; two threads at once.  All comparisons are exact."""
import functools
import hashlib
import threading

import numpy as np
import pytest
import torch

import jpeg_cases as C
import jpeg_ref as R

UNSUPPORTED, CORRUPT = -7, -8


@functools.lru_cache(maxsize=None)
def small():
    return C.load("jpeg_small")


@functools.lru_cache(maxsize=None)
def voc():
    return C.load("jpeg_voc")


def file_of(name):
    return bytes(small()[name]["data"].numpy().tobytes())


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_goldens_hold_every_case():
    assert sorted(small()) == sorted(C.SMALL_NAMES) and len(set(C.SMALL_NAMES)) == len(C.SMALL)
    assert {c[0] for c in C.SMALL} == set(C.SIZES) and {c[1] for c in C.SMALL} == set(C.ENCODINGS)
    assert {c[2] for c in C.SMALL} == set(C.CONTENTS)
    for size in C.CHROMA_EDGES:
        assert {e[:3] for s, e, _ in C.SMALL if s == size} >= {"422", "420"}
    assert {(3 * w) % 4 for _, w in C.SIZES} == {0, 1, 2, 3}


@pytest.mark.parametrize("name", C.SMALL_NAMES)
def test_restatement_equals_golden(name):
    g = small()[name]
    assert torch.equal(torch.from_numpy(R.decode(file_of(name))), g["rgb"])


def test_restatement_equals_golden_voc():
    g = voc()
    rgb = R.decode(g["data"].numpy().tobytes())
    assert rgb.shape == (375, 500, 3)
    assert hashlib.sha256(np.ascontiguousarray(rgb).tobytes()).digest() == g["sha256"].numpy().tobytes()


def test_restatement_equals_pillow_on_the_grid():
    pytest.importorskip("PIL")
    bad = []
    for case in C.GRID:
        data = C.make(*case)
        if not np.array_equal(R.decode(data), C.pillow_rgb(data)):
            bad.append(C.name(*case))
    assert not bad, bad
    # the recorded files are what this Pillow writes, too (restart intervals included)
    assert all(C.make(*case) == file_of(C.name(*case)) for case in C.SMALL)


# ---- the C host pass against the restatement's front half -----------------------------------------------------------------------------
def check_front(data):
    from spe_amd import jpeg as J
    info, coefs = R.front(data)
    pi = J.probe(data)
    assert (pi.width, pi.height, pi.ncomp, pi.restart_interval, pi.mcux, pi.mcuy) == \
        (info["width"], info["height"], info["ncomp"], info["restart"], info["mcux"], info["mcuy"])
    assert pi.sampling == list(zip(info["h"], info["v"])) and pi.blocks == list(zip(info["bw"], info["bh"]))
    assert pi.nblocks == sum(w * h for w, h in pi.blocks)
    assert torch.equal(pi.qt, torch.from_numpy(np.stack(info["qt"]).astype(np.int32)))
    co = J.entropy_decode(data)
    assert co.record.dtype == torch.int16 and co.record.numel() == 192 + 64 * pi.nblocks
    assert torch.equal(co.record[:64 * pi.ncomp].view(-1, 64).int(), pi.qt) and not co.record[64 * pi.ncomp:192].any()
    for c in range(pi.ncomp):
        assert torch.equal(co.component(c), torch.from_numpy(coefs[c])), c
    return co


@pytest.mark.parametrize("name", C.SMALL_NAMES)
def test_host_pass_equals_restatement(name):
    check_front(file_of(name))


def test_host_pass_equals_restatement_voc():
    check_front(voc()["data"].numpy().tobytes())


def test_restart_intervals_are_really_there():
    from spe_amd import jpeg as J
    assert J.probe(file_of("17x33_420_r1_noise")).restart_interval == 1
    pi = J.probe(file_of("37x45_422_r5_noise"))
    assert pi.restart_interval == 5 and pi.mcux % 5 != 0


def test_out_buffer_is_reused_and_fully_written():
    from spe_amd import jpeg as J
    data = file_of("37x45_420_opt_q30_smooth")           # low quality: most coefficients lie past an end of block
    want = J.entropy_decode(data)
    buf = torch.full((want.record.numel() + 7,), 12345, dtype=torch.int16)
    got = J.entropy_decode(data, out=buf)
    assert got.record.data_ptr() == buf.data_ptr() and torch.equal(got.record, want.record) and (buf[-7:] == 12345).all()
    with pytest.raises(ValueError):
        J.entropy_decode(data, out=buf[:100])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def segments(d):
    """[(marker, start of the FF, end)] up to and including SOS; the scan data follow the last end."""
    out, p = [], 2
    while True:
        m, L = d[p + 1], (d[p + 2] << 8) | d[p + 3]
        out.append((m, p, p + 2 + L))
        p += 2 + L
        if m == 0xDA:
            return out


def seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def rebuild(d, edit=None, drop=(), insert=b"", scan=None):
    """The file with edit(marker, payload) -> payload applied to every segment, the markers in `drop` left out, `insert` put behind
    SOI and the entropy-coded data replaced by `scan`."""
    segs = segments(d)
    out = bytearray(d[:2]) + insert
    for m, a, b in segs:
        if m in drop:
            continue
        pay = d[a + 4:b]
        if edit:
            r = edit(m, bytearray(pay))
            if isinstance(r, tuple):
                m, pay = r
            elif r is not None:
                pay = r
        out += seg(m, pay)
    return bytes(out) + (d[segs[-1][2]:] if scan is None else scan)


def sof(fn):
    return lambda m, p: fn(p) if m == 0xC0 else None


def set_byte(i, v):
    def f(p):
        p[i] = v
        return p
    return f


def adobe(transform):
    return seg(0xEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, transform]))


def rgb_ids(m, p):
    if m == 0xC0:
        p[6], p[9], p[12] = b"RGB"
    if m == 0xDA:
        p[1], p[3], p[5] = b"RGB"
    return p


def one_code_tables(ac_symbol):
    """DC and AC table 0 with the single one-bit code 0 -> DC category 0 / ac_symbol."""
    def f(m, p):
        if m == 0xC4:
            return bytes([0x00, 1] + [0] * 15 + [0]) + bytes([0x10, 1] + [0] * 15 + [ac_symbol])
    return f


def refusals():
    c3, c1 = file_of("16x16_444_q100_black"), file_of("8x8_gray_smooth")
    r1 = file_of("17x33_420_r1_noise")
    four = bytes([8, 0, 16, 0, 16, 4, 1, 0x11, 0, 2, 0x11, 0, 3, 0x11, 0, 4, 0x11, 0])
    first_rst = r1.index(b"\xff\xd0", segments(r1)[-1][2])
    marker = lambda new: (lambda m, p: (new, p) if m == 0xC0 else None)       # noqa: E731
    cases = {
        "progressive": (UNSUPPORTED, rebuild(c3, marker(0xC2))),
        "extended": (UNSUPPORTED, rebuild(c3, marker(0xC1))),
        "lossless": (UNSUPPORTED, rebuild(c3, marker(0xC3))),
        "arithmetic": (UNSUPPORTED, rebuild(c3, marker(0xC9))),
        "12-bit samples": (UNSUPPORTED, rebuild(c3, sof(set_byte(0, 12)))),
        "16-bit tables": (UNSUPPORTED, rebuild(c3, lambda m, p: set_byte(0, 0x10)(p) if m == 0xDB else None)),
        "four components": (UNSUPPORTED, rebuild(c3, sof(lambda p: four))),
        "4:4:0": (UNSUPPORTED, rebuild(c3, sof(set_byte(7, 0x12)))),
        "4:1:1": (UNSUPPORTED, rebuild(c3, sof(set_byte(7, 0x41)))),
        "chroma 2x2": (UNSUPPORTED, rebuild(c3, sof(set_byte(10, 0x22)))),
        "several scans": (UNSUPPORTED, rebuild(c3, lambda m, p: bytes([1, 1, 0, 0, 63, 0]) if m == 0xDA else None)),
        "adobe transform 0": (UNSUPPORTED, rebuild(c3, insert=adobe(0))),
        "adobe transform 2": (UNSUPPORTED, rebuild(c3, insert=adobe(2))),
        "ids RGB": (UNSUPPORTED, rebuild(c3, rgb_ids, drop=(0xE0,))),
        "no SOI": (CORRUPT, b"\x00\x01" + c3[2:]),
        "bad marker": (CORRUPT, rebuild(c3, lambda m, p: (0x02, p) if m == 0xDB else None)),
        "stray byte for a marker": (CORRUPT, c3[:2] + b"\x00" + c3[2:]),
        "segment length 1": (CORRUPT, c3[:4] + b"\x00\x01" + c3[6:]),
        "table segment cut short": (CORRUPT, rebuild(c3, lambda m, p: p[:40] if m == 0xDB else None)),
        "no quantisation table": (CORRUPT, rebuild(c3, drop=(0xDB,))),
        "no Huffman table": (CORRUPT, rebuild(c3, drop=(0xC4,))),
        "undefined code": (CORRUPT, rebuild(c1, one_code_tables(0x00), scan=b"\x80\x00\x00\x00")),
        "run past 63": (CORRUPT, rebuild(c1, one_code_tables(0xF1), scan=b"\x00" * 8)),
        "wrong restart marker": (CORRUPT, r1[:first_rst + 1] + b"\xd1" + r1[first_rst + 2:]),
        "bytes in front of a restart marker": (CORRUPT, r1[:first_rst] + b"\x12\x34" + r1[first_rst:]),
        "scan data end early": (CORRUPT, c3[:-6]),
        "frame the data cannot fill": (CORRUPT, rebuild(c3, sof(lambda p: p[:1] + b"\xff\xff\xff\xff" + p[5:]))),
    }
    return cases


REFUSALS = ["progressive", "extended", "lossless", "arithmetic", "12-bit samples", "16-bit tables", "four components", "4:4:0", "4:1:1",
            "chroma 2x2", "several scans", "adobe transform 0", "adobe transform 2", "ids RGB", "no SOI", "bad marker",
            "stray byte for a marker", "segment length 1", "table segment cut short", "no quantisation table", "no Huffman table",
            "undefined code", "run past 63", "wrong restart marker", "bytes in front of a restart marker", "scan data end early",
            "frame the data cannot fill"]


def status_of(data):
    """(status, reason) of probe followed by entropy, as the library reports them."""
    from spe_amd import kernels as K
    rc, info = K.jpeg_probe(data)
    if rc:
        return rc, int(info[24])
    return K.jpeg_entropy(data, torch.zeros((int(info[23]) * 64,), dtype=torch.int16))


@pytest.mark.parametrize("what", REFUSALS)
def test_refusal(what):
    from spe_amd import jpeg as J
    assert sorted(refusals()) == sorted(REFUSALS)
    want, data = refusals()[what]
    rc, reason = status_of(data)
    assert rc == want and reason in J.REASONS, (rc, reason)
    exc = J.JpegUnsupported if want == UNSUPPORTED else J.JpegCorrupt
    with pytest.raises(exc) as e:
        J.entropy_decode(data)
    assert isinstance(e.value, ValueError) and e.value.reason == J.REASONS[reason]
    with pytest.raises(exc) as e:
        J.decode_batch([data], device="cpu", threads=1)
    assert e.value.index == 0


def test_made_up_size_is_refused_by_probe():
    """65535 x 65535 in a 1 KB file: probe says so, nobody allocates the 12 GB of coefficients."""
    from spe_amd import jpeg as J
    from spe_amd import kernels as K
    rc, info = K.jpeg_probe(refusals()["frame the data cannot fill"][1])
    assert rc == CORRUPT and J.REASONS[int(info[24])] == "truncated data" and int(info[23]) == 0


def test_accepted_variants():
    """What must NOT be refused: Adobe transform 1, comments and application segments, fill bytes, a missing EOI."""
    from spe_amd import jpeg as J
    c3 = file_of("17x33_420_noise")
    want = J.entropy_decode(c3).record
    assert c3[-2:] == b"\xff\xd9"
    for data in (rebuild(c3, insert=adobe(1)), rebuild(c3, insert=seg(0xFE, b"hello") + seg(0xE5, b"\xff\xd8\xff\xc2")),
                 c3[:2] + b"\xff\xff" + c3[2:], c3[:-2], c3[:-1]):
        assert torch.equal(J.entropy_decode(data).record, want)


def test_every_prefix_is_corrupt():
    data = file_of("17x33_420_r1_noise")
    for k in range(len(data) - 2):
        rc, _ = status_of(data[:k])
        assert rc == CORRUPT, k


def test_coefficient_buffer_too_small():
    from spe_amd import kernels as K
    data = file_of("8x8_444_noise")
    buf = torch.full((3 * 64,), 77, dtype=torch.int16)
    assert K.jpeg_entropy(data, buf[:3 * 64 - 1])[0] == -2 and (buf == 77).all()
    assert K.jpeg_entropy(data, buf)[0] == 0


# ---- the batch front end ---------------------------------------------------------------------------------------------------------------
def test_decode_batch_fallback_and_index():
    from spe_amd import jpeg as J
    prog = refusals()["progressive"][1]
    bad = refusals()["run past 63"][1]
    seen = []

    def fallback(d):
        seen.append(d)
        return torch.full((2, 3, 3), len(seen), dtype=torch.uint8)
    out = J.decode_batch([prog, prog], device="cpu", fallback=fallback)
    assert seen == [prog, prog] and [int(t[0, 0, 0]) for t in out] == [1, 2]
    with pytest.raises(J.JpegUnsupported) as e:
        J.decode_batch([prog], device="cpu")
    assert e.value.index == 0 and "progressive" in str(e.value)
    with pytest.raises(J.JpegCorrupt) as e:                  # a corrupt file is never handed to the fallback
        J.decode_batch([prog, bad], device="cpu", fallback=fallback)
    assert e.value.index == 1
    with pytest.raises(TypeError):
        J.decode_batch([prog], device="cpu", fallback=lambda d: torch.zeros(2, 2))


def test_supported_files_need_the_device():
    from spe_amd import jpeg as J
    from spe_amd.lib import SpeLibraryError
    with pytest.raises(SpeLibraryError):
        J.decode_batch([file_of("8x8_444_noise")], device="cpu")


def test_two_threads_decode_at_once():
    from spe_amd import jpeg as J
    datas = [voc()["data"].numpy().tobytes(), file_of("37x45_422_r5_noise")]
    want = [J.entropy_decode(d).record.clone() for d in datas]
    got = {}

    def work(t):
        got[t] = [J.entropy_decode(datas[(t + i) % 2]).record.clone() for i in range(6)]
    ths = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    for t in range(2):
        assert all(torch.equal(r, want[(t + i) % 2]) for i, r in enumerate(got[t]))
