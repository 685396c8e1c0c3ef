"""numpy restatement of the input-transform contract (include/spe_hip.h, "input transforms on the device"): Pillow's bilinear
Image.resize as a separable fixed-point resample with a uint8 intermediate, crop and flip as views, ToTensor + Normalize as a
3 x 256 table, zero padding to the batch maximum.  Shared by the CPU tests (against the goldens and against Pillow) and by the
GPU tests (against the kernels); never changed by a test."""
import math

import numpy as np
import torch

BITS = 22


def coeffs(inS, outS):
    """-> (ksize, xmin [outS], n [outS], k [outS, ksize] int32) of one axis, fp64 in Pillow's operation order."""
    scale = inS / outS
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    xmin = np.zeros(outS, np.int32)
    cnt = np.zeros(outS, np.int32)
    k = np.zeros((outS, ksize), np.int32)
    ss = 1.0 / fs
    for xx in range(outS):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), inS) - lo
        w = []
        ww = 0.0
        for x in range(n):
            t = abs((x + lo - center + 0.5) * ss)
            v = 1.0 - t if t < 1.0 else 0.0
            w.append(v)
            ww += v
        for x in range(n):
            v = w[x] / ww if ww != 0.0 else w[x]
            k[xx, x] = int(0.5 + v * (1 << BITS))
        xmin[xx], cnt[xx] = lo, n
    return ksize, xmin, cnt, k


def _pass(src, outS):
    """Resample axis 1 of a uint8 [R, inS, C] array -> uint8 [R, outS, C]."""
    _, xmin, cnt, k = coeffs(src.shape[1], outS)
    out = np.empty((src.shape[0], outS, src.shape[2]), np.uint8)
    s = src.astype(np.int64)
    for xx in range(outS):
        lo, n = int(xmin[xx]), int(cnt[xx])
        acc = (1 << (BITS - 1)) + (s[:, lo:lo + n, :] * k[xx, :n].astype(np.int64)[None, :, None]).sum(1)
        out[:, xx, :] = np.clip(acc >> BITS, 0, 255)
    return out


def resize(img, oh, ow):
    """uint8 [H, W, 3] -> uint8 [oh, ow, 3]: horizontal pass into uint8, then the vertical pass over that."""
    tmp = _pass(np.ascontiguousarray(img), ow)
    return _pass(tmp.transpose(1, 0, 2), oh).transpose(1, 0, 2).copy()


def view(img, box, flip):
    """The kernels' index map x -> x0 + (flip ? cw - 1 - x : x), y -> y0 + y over a uint8 [H, W, 3] array."""
    x0, y0, cw, ch = box
    v = img[y0:y0 + ch, x0:x0 + cw]
    return v[:, ::-1] if flip else v


def run_stages(img, stages):
    """stages: [(x0, y0, cw, ch, flip, oh, ow), ...], each applied to the previous one's output."""
    for x0, y0, cw, ch, flip, oh, ow in stages:
        img = resize(view(img, (x0, y0, cw, ch), flip), oh, ow)
    return img


def norm_table(mean=None, std=None):
    """ToTensor + Normalize as the reference computes them, per (channel, byte), in torch CPU fp32."""
    base = torch.arange(256).float().div(255)
    if mean is None:
        return torch.stack([base, base, base])
    return torch.stack([base.sub(mean[c]).div(std[c]) for c in range(3)])


def collate(images_u8, lut):
    """uint8 [h, w, 3] arrays -> (fp32 [B, 3, Hmax, Wmax], bool [B, Hmax, Wmax]) as util.misc.collate_fn pads them."""
    B = len(images_u8)
    H, W = max(i.shape[0] for i in images_u8), max(i.shape[1] for i in images_u8)
    out = torch.zeros((B, 3, H, W), dtype=torch.float32)
    mask = torch.ones((B, H, W), dtype=torch.bool)
    for b, im in enumerate(images_u8):
        t = torch.from_numpy(np.ascontiguousarray(im)).long()
        h, w = im.shape[:2]
        for c in range(3):
            out[b, c, :h, :w] = lut[c][t[:, :, c]]
        mask[b, :h, :w] = False
    return out, mask
