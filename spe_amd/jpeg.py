"""Baseline JPEG decoding in front of the device transforms.

The serial part of a JPEG file - markers and Huffman codes - is decoded on the host by plain C++ (csrc/jpeg_entropy.h) into quantised
coefficients in pinned memory; everything that touches a pixel (dequantisation, inverse DCT, chroma upsampling, YCbCr -> RGB) runs on
the device in two launches for the whole batch (csrc/jpeg_decode.hip) and writes the uint8 [H,W,3] tensors spe_amd.transforms takes,
equal to Pillow's decode (libjpeg-turbo: islow IDCT, fancy upsampling) bit for bit.

Accepted: baseline (SOF0) files with 8-bit samples, one component or three with 4:4:4, 4:2:2 or 4:2:0 sampling, in one scan, with or
without restart markers.  Everything else is refused by the host pass: JpegUnsupported for valid files of other forms (progressive,
arithmetic, 12-bit, CMYK, 4:4:0 / 4:1:1 ...), JpegCorrupt for files that cannot be decoded.  decode_batch(fallback=...) hands the
unsupported ones to a decoder of the caller's choice."""
from concurrent.futures import ThreadPoolExecutor

import torch

from . import kernels as K

REASONS = {
    1: "progressive (SOF2)", 2: "extended, lossless or arithmetic coding", 3: "12-bit samples", 4: "16-bit quantisation tables",
    5: "two or four components", 6: "sampling factors other than 4:4:4, 4:2:2, 4:2:0", 7: "more than one scan",
    8: "Adobe APP14 marker with a colour transform other than YCbCr", 9: "component ids R, G, B", 10: "height given by a DNL segment",
    32: "truncated data", 33: "bad marker", 34: "bad segment length", 35: "missing quantisation or Huffman table",
    36: "undefined Huffman code", 37: "run past coefficient 63", 38: "wrong restart marker", 39: "bad header field",
    64: "coefficient buffer too small",
}


class JpegError(ValueError):
    """index: the image's position in the batch (None outside one); reason: the text of REASONS."""

    def __init__(self, reason, index=None):
        self.reason, self.index = reason, index
        super().__init__(f"{self.KIND} JPEG{'' if index is None else f' (image {index})'}: {reason}")


class JpegUnsupported(JpegError):
    KIND = "unsupported"


class JpegCorrupt(JpegError):
    KIND = "corrupt"


def _raise(status, reason, index=None):
    text = REASONS.get(reason, f"reason {reason}")
    if status == K.JPEG_UNSUPPORTED:
        raise JpegUnsupported(text, index)
    if status == K.JPEG_CORRUPT:
        raise JpegCorrupt(text, index)
    raise ValueError(f"JPEG decoding failed with status {status}: {text}")


class JpegInfo:
    """What the markers say.  sampling: (h, v) per component; blocks: (across, down) per component, the grid padded to whole MCUs;
    qt: int32 [ncomp, 64], natural order."""

    def __init__(self, raw):
        r = raw.tolist()
        self.width, self.height, self.ncomp, self.restart_interval, self.mcux, self.mcuy = r[0], r[1], r[2], r[5], r[6], r[7]
        nc = self.ncomp
        self.sampling = [(r[8 + c], r[11 + c]) for c in range(nc)]
        self.blocks = [(r[14 + c], r[17 + c]) for c in range(nc)]
        self.nblocks = r[23]
        self.qt = raw[32:32 + 64 * nc].view(nc, 64).clone()

    @property
    def frame(self):
        """(W, H, ncomp, hs, vs, mcux, mcuy) as kernels.jpeg_reconstruct takes it."""
        return (self.width, self.height, self.ncomp) + self.sampling[0] + (self.mcux, self.mcuy)

    def __repr__(self):
        return f"JpegInfo({self.width}x{self.height}, sampling {self.sampling}, restart {self.restart_interval}, {self.nblocks} blocks)"


class JpegCoefficients:
    """One image after the host pass.  record: int16 [192 + nblocks * 64] in pinned host memory (pageable where there is no device) -
    the three quantisation tables, then every block's 64 quantised coefficients in natural order, the components one after the
    other in raster order over their padded block grids: exactly what is uploaded."""

    def __init__(self, info, record):
        self.info, self.record = info, record

    @property
    def coef(self):
        return self.record[K.JPEG_QT:K.JPEG_QT + self.info.nblocks * 64].view(-1, 64)

    def component(self, c):
        """int16 [blocks down, blocks across, 64] of component c."""
        start = sum(w * h for w, h in self.info.blocks[:c])
        w, h = self.info.blocks[c]
        return self.coef[start:start + w * h].view(h, w, 64)


def probe(data):
    """bytes -> JpegInfo.  Host only."""
    data = bytes(data)
    status, raw = K.jpeg_probe(data)
    if status:
        _raise(status, int(raw[24]))
    return JpegInfo(raw)


def record_elems(info):
    return K.JPEG_QT + info.nblocks * 64


def entropy_decode(data, out=None):
    """bytes -> JpegCoefficients.  Host only; the Huffman pass runs with the GIL released.  out: an int16 host tensor of at least
    record_elems(probe(data)) elements to decode into (a loader reuses its pinned buffers); default: a fresh pinned one."""
    data = bytes(data)
    info = probe(data)
    need = record_elems(info)
    if out is None:
        out = torch.empty((need,), dtype=torch.int16, pin_memory=torch.cuda.is_available())
    elif out.is_cuda or out.dtype != torch.int16 or not out.is_contiguous() or out.numel() < need:
        raise ValueError(f"entropy_decode: out needs a contiguous int16 host tensor of at least {need} elements")
    record = out.view(-1)[:need]
    record[:K.JPEG_QT] = 0
    record[:64 * info.ncomp] = info.qt.reshape(-1).to(torch.int16)
    status, reason = K.jpeg_entropy(data, record[K.JPEG_QT:])
    if status:
        _raise(status, reason)
    return JpegCoefficients(info, record)


def reconstruct(coeffs_list, device="cuda"):
    """[JpegCoefficients, ...] -> uint8 [H,W,3] device tensors: one non-blocking upload per image into one packed buffer, then the
    two launches."""
    device = torch.device(device)
    if device.type != "cuda":
        from .lib import SpeLibraryError
        raise SpeLibraryError("spe_amd kernels run on the GPU only; there is no CPU fallback")
    for c in coeffs_list:
        if c.info.width > K.JPEG_MAX_SIDE or c.info.height > K.JPEG_MAX_SIDE:
            raise JpegUnsupported(f"a side above {K.JPEG_MAX_SIDE}")
    offs, total = [], 0
    for c in coeffs_list:
        offs.append(total)
        total += c.record.numel()                      # 192 + 64 * blocks: every record starts 16-byte aligned
    packed = torch.empty((total,), device=device, dtype=torch.int16)
    for c, o in zip(coeffs_list, offs):
        packed[o:o + c.record.numel()].copy_(c.record, non_blocking=True)
    with torch.cuda.device(device):
        return K.jpeg_reconstruct([c.info.frame + (o,) for c, o in zip(coeffs_list, offs)], packed)


_POOLS = {}


def _pool(threads):
    """One pool per size, kept: starting threads costs more than decoding a file."""
    ex = _POOLS.get(threads)
    if ex is None:
        ex = _POOLS[threads] = ThreadPoolExecutor(max_workers=threads, thread_name_prefix="spe_jpeg")
    return ex


def decode_batch(datas, device="cuda", threads=4, fallback=None):
    """[bytes, ...] -> uint8 [H,W,3] device tensors.  The host pass of every file runs on a pool of `threads` threads, then
    reconstruct.  A refused file raises JpegUnsupported / JpegCorrupt with its index; with fallback (bytes -> uint8 [H,W,3] tensor)
    an unsupported one is decoded by it instead."""
    datas = [bytes(d) for d in datas]

    def host(d):
        try:
            return entropy_decode(d)
        except JpegError as e:
            return e
    if threads > 1 and len(datas) > 1:
        res = list(_pool(int(threads)).map(host, datas))
    else:
        res = [host(d) for d in datas]
    out = [None] * len(datas)
    for i, r in enumerate(res):
        if isinstance(r, JpegError):
            if isinstance(r, JpegUnsupported) and fallback is not None:
                t = fallback(datas[i])
                if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.ndim != 3 or t.shape[2] != 3:
                    raise TypeError("decode_batch: fallback must return a uint8 [H,W,3] tensor")
                out[i] = t.to(device, non_blocking=True).contiguous()
            else:
                raise type(r)(r.reason, i)
    idx = [i for i, r in enumerate(res) if isinstance(r, JpegCoefficients)]
    if idx:
        for i, t in zip(idx, reconstruct([res[i] for i in idx], device)):
            out[i] = t
    return out
