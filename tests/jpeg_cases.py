"""The JPEG decoding cases (tests/test_jpeg_cpu.py, tests/test_jpeg_gpu.py, tools/gen_jpeg_golden.py).

Sizes are h x w, the smallest at which each edge occurs: 8x8 one block; 16x16 one 4:2:0 MCU; 17x33 one past an MCU both ways; 1x9
one row (both vertical neighbours are the row itself); 9x5 chroma width 3, the first to take the triangle filter; 3x3 chroma width
2, the replication rule; 15x6 odd height (the last chroma row serves one luma row); 37x45 general odd; 31x64 and 40x48 exact
multiples; 2x265 is 34 blocks a row, one workgroup of the IDCT pass covers 32; 2x1030 is 259 lanes a row of the colour pass, one
workgroup has 256.  3W mod 4 is 1 at w = 3, 2 at w = 6 and 1030, 3 at w = 5, 9, 33, 45 and 265, 0 at the rest."""
import hashlib
import io
import os

import numpy as np
import torch

SIZES = [(8, 8), (16, 16), (17, 33), (1, 9), (9, 5), (3, 3), (15, 6), (37, 45), (31, 64), (40, 48), (2, 265), (2, 1030)]
CONTENTS = ["noise", "smooth", "grey", "black", "white"]
# Pillow's save() arguments; "L": encode the luma alone
ENCODINGS = {
    "444": dict(subsampling=0, quality=85),
    "422": dict(subsampling=1, quality=85),
    "420": dict(subsampling=2, quality=85),
    "gray": dict(quality=85, L=True),
    "420_r1": dict(subsampling=2, quality=85, restart_marker_blocks=1),
    "422_r5": dict(subsampling=1, quality=85, restart_marker_blocks=5),        # 5 divides no MCU row of 2, 3, 4 ... MCUs
    "420_opt_q30": dict(subsampling=2, quality=30, optimize=True),
    "444_q100": dict(subsampling=0, quality=100),
    "420_q5": dict(subsampling=2, quality=5),
}
CHROMA_EDGES = [(1, 9), (9, 5), (3, 3), (15, 6)]

# (size, encoding, content): every size, every encoding and every content at least once, every chroma-edge size with 4:2:2 and 4:2:0
SMALL = [((8, 8), "444", "noise"), ((8, 8), "gray", "smooth"), ((8, 8), "420_q5", "white"),
         ((16, 16), "420", "noise"), ((16, 16), "422", "smooth"), ((16, 16), "444_q100", "black"),
         ((17, 33), "420", "noise"), ((17, 33), "422_r5", "smooth"), ((17, 33), "420_r1", "noise"), ((17, 33), "gray", "noise"),
         ((1, 9), "422", "noise"), ((1, 9), "420", "smooth"),
         ((9, 5), "422", "smooth"), ((9, 5), "420", "noise"),
         ((3, 3), "422", "noise"), ((3, 3), "420", "noise"), ((3, 3), "444", "smooth"),
         ((15, 6), "422", "noise"), ((15, 6), "420", "smooth"), ((15, 6), "420_opt_q30", "noise"),
         ((37, 45), "420", "noise"), ((37, 45), "422_r5", "noise"), ((37, 45), "444_q100", "noise"), ((37, 45), "420_q5", "smooth"),
         ((37, 45), "420_opt_q30", "smooth"), ((37, 45), "420_r1", "smooth"),
         ((31, 64), "444", "smooth"), ((31, 64), "420", "grey"),
         ((40, 48), "422", "white"), ((40, 48), "420_opt_q30", "noise"), ((40, 48), "gray", "black"),
         ((2, 265), "444", "noise"), ((2, 265), "420", "smooth"), ((2, 1030), "422", "smooth"), ((2, 1030), "420", "noise")]


def name(size, enc, content):
    return f"{size[0]}x{size[1]}_{enc}_{content}"


SMALL_NAMES = [name(*c) for c in SMALL]
GRID = [(s, e, c) for s in SIZES for e in ENCODINGS for c in CONTENTS]


def fill(content, h, w, seed):
    """uint8 [h, w, 3]."""
    if content == "grey":
        return np.full((h, w, 3), 128, np.uint8)
    if content == "black":
        return np.zeros((h, w, 3), np.uint8)
    if content == "white":
        return np.full((h, w, 3), 255, np.uint8)
    rng = np.random.default_rng(seed)
    if content == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 9.0 + yy / 17.0), 128 + 90 * np.cos(xx / 23.0 - yy / 7.0), (3 * xx + 2 * yy) % 256], axis=2)
    return np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(arr, enc):
    """File bytes of the uint8 [h, w, 3] array under ENCODINGS[enc].  Needs Pillow."""
    from PIL import Image
    kw = dict(ENCODINGS[enc])
    im = Image.fromarray(arr, "RGB")
    if kw.pop("L", False):
        im = im.convert("L")
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def make(size, enc, content):
    """-> file bytes; the content's seed depends on the case alone."""
    seed = int.from_bytes(hashlib.sha256(name(size, enc, content).encode()).digest()[:4], "little")
    return encode(fill(content, size[0], size[1], seed), enc)


def voc_file():
    """One VOC-sized file: 375 x 500, 4:2:0, quality 90."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(fill("smooth", 375, 500, 2012), "RGB").save(buf, "JPEG", subsampling=2, quality=90)
    return buf.getvalue()


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(which):
    """jpeg_small: {name: {"data": uint8 [n] file bytes, "rgb": uint8 [H,W,3] Pillow's decode}}; jpeg_voc: {"data", "sha256": uint8 [32]}."""
    return torch.load(os.path.join(GOLD, which + ".pt"), weights_only=True)
