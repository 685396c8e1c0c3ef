"""Shapes for the input-transform kernels (csrc/img_resample.hip): the smallest ones at which they can go wrong.  The kernels'
own widths: a lane takes 4 consecutive x, a workgroup of the horizontal / uint8 vertical pass 256 x by 4 rows, the final
vertical pass 256 lanes of a flattened (row, 4-x group) index with one extra head lane per row."""
import glob
import os
import random

import numpy as np
import torch

# name, source (h, w), box (x0, y0, cw, ch), flip, output (oh, ow), fill
SINGLE = [
    ("up_3taps", (20, 30), None, False, (45, 70), "rand"),
    ("down_5taps", (50, 45), None, False, (30, 27), "rand"),                 # 1.67x: ceil -> 2, ksize 5
    ("down_7taps", (70, 52), None, False, (27, 20), "rand"),                 # 2.6x: ksize 7
    ("down_4x_9taps", (64, 48), None, False, (16, 12), "rand"),
    ("identity_y", (40, 33), None, False, (40, 60), "rand"),
    ("identity_x", (33, 40), None, False, (60, 40), "rand"),
    ("identity_both", (17, 23), None, False, (17, 23), "rand"),
    ("src_h1", (1, 9), None, False, (5, 3), "rand"),
    ("src_w1", (9, 1), None, False, (3, 5), "rand"),
    ("out_1x1", (9, 12), None, False, (1, 1), "rand"),
    ("out_w1", (9, 12), None, False, (7, 1), "rand"),
    ("crop_flip", (31, 44), (7, 5, 29, 20), True, (33, 41), "rand"),         # non-zero origin under a flip
    ("crop_noflip", (31, 44), (7, 5, 29, 20), False, (13, 17), "rand"),
    ("flip_only", (12, 19), None, True, (12, 19), "rand"),
    ("all0", (13, 17), None, False, (29, 40), "zeros"),
    ("all255_up", (13, 17), None, False, (29, 40), "ones"),
    ("all255_down", (37, 41), None, False, (11, 13), "ones"),               # coefficient sums that are not exactly 2^22
    ("checker_up", (14, 18), None, False, (31, 47), "checker"),
    ("checker_down", (45, 39), None, False, (14, 17), "checker"),
    ("ow_3", (6, 5), None, False, (5, 3), "rand"),
    ("ow_4", (6, 5), None, False, (5, 4), "rand"),
    ("ow_5", (6, 5), None, False, (5, 5), "rand"),
    ("ow_255", (5, 200), None, False, (6, 255), "rand"),
    ("ow_256", (5, 200), None, False, (6, 256), "rand"),
    ("ow_257", (5, 200), None, False, (6, 257), "rand"),
]

# batches for the final epilogue: [(source (h, w), output (oh, ow)), ...]; Wmax = the widest output.  Wmax mod 4 = 0, 1, 2, 3 with a
# second image whose width leaves head and tail of its rows unaligned; heights differ so that whole rows are padding too
BATCHES = [
    ("wmax36", [((20, 30), (17, 36)), ((25, 21), (19, 29))]),
    ("wmax37", [((20, 30), (17, 37)), ((25, 21), (19, 30))]),
    ("wmax38", [((20, 30), (21, 38)), ((25, 21), (18, 31))]),
    ("wmax39", [((20, 30), (17, 39)), ((25, 21), (19, 33)), ((9, 9), (5, 2))]),
    ("wmax3", [((5, 5), (4, 3)), ((5, 5), (6, 1))]),                          # rows shorter than one vector
]

# descriptors the entry points must refuse: name, source (h, w), box, output, status
BAD = [
    ("empty_box", (10, 10), (2, 2, 0, 5), (5, 5), -2),
    ("empty_out", (10, 10), (0, 0, 10, 10), (0, 5), -2),
    ("crop_right", (10, 10), (4, 0, 7, 10), (5, 5), -3),
    ("crop_below", (10, 10), (0, 8, 10, 3), (5, 5), -3),
    ("crop_negative", (10, 10), (-1, 0, 5, 5), (5, 5), -3),
    ("taps", (200, 6), (0, 0, 6, 200), (5, 7), -5),                           # 40x down: ksize 81 > 65
]
TAP_LIMIT_OK = ((64, 8), (2, 8))                                               # 32x down: ksize 65, the limit itself


def fill(kind, h, w, seed):
    if kind == "zeros":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "ones":
        return np.full((h, w, 3), 255, np.uint8)
    if kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- the recorded runs of the reference's pipeline (tools/gen_transforms_golden.py) ----
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = sorted(glob.glob(os.path.join(GOLD, "transforms_*.pt")))
NAMES = [os.path.basename(f)[:-3] for f in FILES]


def load(name):
    return torch.load(os.path.join(GOLD, name + ".pt"), weights_only=True)


def factory(g):
    from spe_amd import transforms as T
    if g["kind"] == "fixed":
        return T.make_transforms("train", max_size=64, fixed=True)
    return T.make_transforms(g["kind"], max_size=g["max_size"])


def run_pipeline(g, device=None):
    """The project's pipeline from the fixture's seeds -> [(PendingTensor, target), ...]."""
    from spe_amd import transforms as T
    random.seed(g["seed"])
    torch.manual_seed(g["seed"])
    tf = factory(g)
    return [tf(T.DeviceImage(im, device=device), {k: v.clone() for k, v in tg.items()}) for im, tg in zip(g["images"], g["targets"])]
