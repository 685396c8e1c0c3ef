"""Baseline JPEG decoding restated in plain Python + numpy (libjpeg-turbo's default path: islow IDCT, fancy upsampling, 16-bit
fixed-point colour conversion), the reference of spe_amd.jpeg (csrc/jpeg_entropy.h, csrc/jpeg_decode.hip).

front(data)       marker parsing + Huffman decoding -> (info, [coefficients per component]): quantised int16 [bh, bw, 64] in natural
                  order over the component's block grid padded to whole MCUs.
back(info, coefs) dequantise, inverse DCT, upsample, colour-convert -> uint8 [H, W, 3].
decode(data)      both.
It reads valid files of the accepted forms only; refusals are the C host pass's business (tests/test_jpeg_cpu.py)."""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def _u16(d, p):
    return (d[p] << 8) | d[p + 1]


def _huff_table(counts, symbols):
    """-> 65536-entry lists (code length, symbol) indexed by the next 16 bits; length 0: no such code."""
    ln = np.zeros(65536, np.uint8)
    sy = np.zeros(65536, np.uint8)
    code, k = 0, 0
    for bits in range(1, 17):
        for _ in range(counts[bits - 1]):
            lo = code << (16 - bits)
            ln[lo:lo + (1 << (16 - bits))] = bits
            sy[lo:lo + (1 << (16 - bits))] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return ln.tolist(), sy.tolist()


def parse(data):
    """Markers up to the scan -> info dict; info["scan"] is the offset of the first entropy-coded byte."""
    d = bytes(data)
    assert d[0] == 0xFF and d[1] == 0xD8
    p = 2
    qt, huff, ri, frame = {}, {}, 0, None
    while True:
        assert d[p] == 0xFF
        while d[p + 1] == 0xFF:
            p += 1
        m = d[p + 1]
        L = _u16(d, p + 2)
        s = p + 4
        if m == 0xDB:
            while s < p + 2 + L:
                pq, tq = d[s] >> 4, d[s] & 15
                assert pq == 0
                t = np.zeros(64, np.int32)
                for k in range(64):
                    t[ZIGZAG[k]] = d[s + 1 + k]
                qt[tq] = t
                s += 65
        elif m == 0xC0:
            assert d[s] == 8
            frame = {"height": _u16(d, s + 1), "width": _u16(d, s + 3),
                     "comps": [(d[s + 6 + 3 * c], d[s + 7 + 3 * c] >> 4, d[s + 7 + 3 * c] & 15, d[s + 8 + 3 * c]) for c in range(d[s + 5])]}
        elif m == 0xC4:
            while s < p + 2 + L:
                tc, th = d[s] >> 4, d[s] & 15
                counts = list(d[s + 1:s + 17])
                n = sum(counts)
                huff[(tc, th)] = _huff_table(counts, d[s + 17:s + 17 + n])
                s += 17 + n
        elif m == 0xDD:
            ri = _u16(d, s)
        elif m == 0xDA:
            ns = d[s]
            assert frame is not None and ns == len(frame["comps"])
            sel = [(d[s + 1 + 2 * c], d[s + 2 + 2 * c] >> 4, d[s + 2 + 2 * c] & 15) for c in range(ns)]
            p += 2 + L
            break
        p += 2 + L
    nc = len(frame["comps"])
    hs = [1] if nc == 1 else [c[1] for c in frame["comps"]]
    vs = [1] if nc == 1 else [c[2] for c in frame["comps"]]
    hmax, vmax = max(hs), max(vs)
    W, H = frame["width"], frame["height"]
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    return {"width": W, "height": H, "ncomp": nc, "h": hs, "v": vs, "restart": ri, "mcux": mcux, "mcuy": mcuy,
            "bw": [mcux * h for h in hs], "bh": [mcuy * v for v in vs], "qt": [qt[c[3]] for c in frame["comps"]],
            "dc": [huff[(0, s_[1])] for s_ in sel], "ac": [huff[(1, s_[2])] for s_ in sel], "scan": p}


def _segments(d, p):
    """The entropy-coded bytes from p, unstuffed, split at the restart markers."""
    segs, cur = [], bytearray()
    n = len(d)
    while p < n:
        b = d[p]
        if b != 0xFF:
            cur.append(b)
            p += 1
            continue
        if p + 1 >= n:
            break
        m = d[p + 1]
        if m == 0:
            cur.append(0xFF)
            p += 2
        elif m == 0xFF:
            p += 1
        elif 0xD0 <= m <= 0xD7:
            segs.append(bytes(cur))
            cur = bytearray()
            p += 2
        else:
            break
    segs.append(bytes(cur))
    return segs


def front(data):
    d = bytes(data)
    info = parse(d)
    nc = info["ncomp"]
    coefs = [np.zeros((info["bh"][c], info["bw"][c], 64), np.int16) for c in range(nc)]
    segs = _segments(d, info["scan"])
    nmcu = info["mcux"] * info["mcuy"]
    ri = info["restart"] or nmcu
    mcu = 0
    for seg in segs:
        if mcu >= nmcu:
            break
        seg = seg + b"\0\0\0\0"
        pos = 0
        pred = [0] * nc

        def peek16():
            i = pos >> 3
            return (((seg[i] << 16) | (seg[i + 1] << 8) | seg[i + 2]) >> (8 - (pos & 7))) & 0xFFFF

        for _ in range(min(ri, nmcu - mcu)):
            my, mx = divmod(mcu, info["mcux"])
            for c in range(nc):
                dl, ds = info["dc"][c]
                al, as_ = info["ac"][c]
                for by in range(info["v"][c]):
                    for bx in range(info["h"][c]):
                        blk = coefs[c][my * info["v"][c] + by, mx * info["h"][c] + bx]
                        w = peek16()
                        pos += dl[w]
                        s = ds[w]
                        if s:
                            v = peek16() >> (16 - s)
                            pos += s
                            if v < (1 << (s - 1)):
                                v -= (1 << s) - 1
                            pred[c] += v
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            w = peek16()
                            pos += al[w]
                            rs = as_[w]
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            v = peek16() >> (16 - s)
                            pos += s
                            if v < (1 << (s - 1)):
                                v -= (1 << s) - 1
                            blk[ZIGZAG[k]] = v
                            k += 1
            mcu += 1
    assert mcu == nmcu
    return info, coefs


def _pass8(i, s):
    """libjpeg's jidctint.c 8-point pass on i[0..7] (equal-shaped int64 arrays), descaled by s."""
    i0, i1, i2, i3, i4, i5, i6, i7 = i
    z1 = (i2 + i6) * 4433
    t2 = z1 - i6 * 15137
    t3 = z1 + i2 * 6270
    t0 = (i0 + i4) << 13
    t1 = (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a, b, c, d = i7, i5, i3, i1
    z1, z2, z3, z4 = a + d, b + c, a + c, b + d
    z5 = (z3 + z4) * 9633
    a, b, c, d = a * 2446, b * 16819, c * 25172, d * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a, b, c, d = a + z1 + z3, b + z2 + z4, c + z2 + z3, d + z1 + z4
    out = (t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d)
    return [(v + (1 << (s - 1))) >> s for v in out]


def idct_planes(coef, qt):
    """int16 [bh, bw, 64] quantised, qt [64] -> uint8 plane [bh * 8, bw * 8]."""
    bh, bw = coef.shape[:2]
    x = (coef.astype(np.int64) * qt.astype(np.int64)).reshape(bh, bw, 8, 8)
    ws = np.stack(_pass8([x[:, :, k, :] for k in range(8)], 11), axis=2)         # down the columns: ws[r][c]
    o = np.stack(_pass8([ws[:, :, :, k] for k in range(8)], 18), axis=3)          # along the rows
    t = (o + 128) & 1023
    smp = np.where(t < 256, t, np.where(t < 640, 255, 0)).astype(np.uint8)
    return smp.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _up_h2v1(c):
    """[dh, dw] int64 -> [dh, 2 dw]."""
    dh, dw = c.shape
    if dw <= 2:
        return np.repeat(c, 2, axis=1)
    l = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    r = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    out = np.empty((dh, 2 * dw), np.int64)
    out[:, 0::2] = (3 * c + l + 1) >> 2
    out[:, 1::2] = (3 * c + r + 2) >> 2
    return out


def _up_h2v2(c):
    """[dh, dw] int64 -> [2 dh, 2 dw]."""
    dh, dw = c.shape
    if dw <= 2:
        return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    up = np.concatenate([c[:1], c[:-1]], axis=0)
    dn = np.concatenate([c[1:], c[-1:]], axis=0)
    out = np.empty((2 * dh, 2 * dw), np.int64)
    for par, nb in ((0, up), (1, dn)):
        s = 3 * c + nb
        l = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        r = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        out[par::2, 0::2] = (3 * s + l + 8) >> 4
        out[par::2, 1::2] = (3 * s + r + 7) >> 4
    return out


def back(info, coefs):
    W, H, nc = info["width"], info["height"], info["ncomp"]
    planes = [idct_planes(coefs[c], info["qt"][c]) for c in range(nc)]
    y = planes[0][:H, :W].astype(np.int64)
    if nc == 1:
        return np.repeat(y.astype(np.uint8)[:, :, None], 3, axis=2)
    hs, vs = info["h"][0], info["v"][0]
    dw, dh = -(-W // hs), -(-H // vs)
    ch = []
    for c in (1, 2):
        p = planes[c][:dh, :dw].astype(np.int64)
        if (hs, vs) == (2, 1):
            p = _up_h2v1(p)
        elif (hs, vs) == (2, 2):
            p = _up_h2v2(p)
        else:
            assert (hs, vs) == (1, 1)
        ch.append(p[:H, :W] - 128)
    cb, cr = ch
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode(data):
    return back(*front(data))
