"""Golden vectors of the REFERENCE's input pipeline (datasets/transforms.py classes + util/misc.collate_fn), written by running
the reference's own code in the build container (imported by path from the reference checkout, tools/ref_harness.REF):

    python tools/gen_transforms_golden.py

The reference needs torchvision.transforms, which does not exist here.  The harness-only shim below stands in for the handful of
calls the reference makes, built on Pillow exactly as torchvision builds them for a PIL image: F.crop -> Image.crop, F.hflip ->
transpose(FLIP_LEFT_RIGHT), F.resize(img, (h, w)) -> Image.resize((w, h), BILINEAR), F.to_tensor, F.normalize, and
T.RandomCrop.get_params with its semantics since 0.8 (torch.randint for the row, then the column; no draw when the crop equals
the image).  The shim is this project's text; nothing of the reference is written anywhere.

The pipelines have the structure of the reference's factories at a small scale: make_coco_transforms_specific_size('train' /
'val', max_size=100) - scales 36..60, intermediate sizes 30 / 37 / 45, crops 28..45 - and the fixed factory as Resize((64, 64)).

-> tests/golden/transforms_<kind><i>.pt (data only), one batch of two images per file: the uint8 input images, the input targets,
the seeds of `random` / torch, the call trace (flip, crop regions, resize sizes), the reference's padded batch, mask and output
targets, and both generators' states after the run.  Seeds are searched so that the train files together contain a flip and no
flip, both arms of RandomSelect, a crop that drops a box, a crop equal to the image and the max_size clamp; the generator asserts
that, and that tests/resample_ref.py reproduces every recorded batch bitwise.  Deterministic: the files regenerate bit for bit."""
import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resample_ref as R  # noqa: E402
from tools import ref_harness  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
MAX_SIZE = 100


def install_transforms_shim():
    ref_harness.install_shims()
    tv = sys.modules["torchvision"]
    T = types.ModuleType("torchvision.transforms")
    F = types.ModuleType("torchvision.transforms.functional")
    F.crop = lambda img, top, left, height, width: img.crop((left, top, left + width, top + height))
    F.hflip = lambda img: img.transpose(Image.FLIP_LEFT_RIGHT)
    F.resize = lambda img, size: img.resize((size[1], size[0]), Image.BILINEAR)

    def to_tensor(pic):
        t = torch.from_numpy(np.array(pic, np.uint8, copy=True)).view(pic.size[1], pic.size[0], 3)
        return t.permute((2, 0, 1)).contiguous().to(dtype=torch.float32).div(255)

    def normalize(tensor, mean, std):
        tensor = tensor.clone()
        mean = torch.as_tensor(mean, dtype=tensor.dtype)
        std = torch.as_tensor(std, dtype=tensor.dtype)
        return tensor.sub_(mean.view(-1, 1, 1)).div_(std.view(-1, 1, 1))
    F.to_tensor, F.normalize = to_tensor, normalize

    class RandomCrop:
        @staticmethod
        def get_params(img, output_size):
            w, h = img.size
            th, tw = output_size
            if h + 1 < th or w + 1 < tw:
                raise ValueError("crop larger than the image")
            if w == tw and h == th:
                return 0, 0, h, w
            i = torch.randint(0, h - th + 1, size=(1,)).item()
            j = torch.randint(0, w - tw + 1, size=(1,)).item()
            return i, j, th, tw
    T.RandomCrop = RandomCrop
    T.RandomErasing = object
    T.functional = F
    tv.transforms = T
    sys.modules["torchvision.transforms"] = T
    sys.modules["torchvision.transforms.functional"] = F


def load_reference():
    install_transforms_shim()
    spec = importlib.util.spec_from_file_location("ref_transforms", os.path.join(ref_harness.REF, "datasets", "transforms.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    import util.misc as ref_misc
    return m, ref_misc


def pipeline(T, kind):
    normalize = T.Compose([T.ToTensor(), T.Normalize(MEAN, STD)])
    scales = [s * MAX_SIZE // 1333 for s in (480, 512, 544, 576, 608, 640, 672, 704, 736, 768, 800)]
    if kind == "train":
        return T.Compose([
            T.RandomHorizontalFlip(),
            T.RandomSelect(
                T.RandomResize(scales, max_size=MAX_SIZE),
                T.Compose([T.RandomResize([r * MAX_SIZE // 1333 for r in (400, 500, 600)]),
                           T.RandomSizeCrop(*[c * MAX_SIZE // 1333 for c in (384, 600)]),
                           T.RandomResize(scales, max_size=MAX_SIZE)])),
            normalize])
    if kind == "val":
        return T.Compose([T.RandomResize([800 * MAX_SIZE // 1333], max_size=MAX_SIZE), normalize])
    return T.Compose([T.RandomHorizontalFlip(), T.Resize((64, 64), max_size=64), normalize])


def make_image(rng, h, w):
    """Smooth gradients + noise + saturated patches: every byte value, flat 0 / 255 areas for the clamps."""
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 9) % 256], -1).astype(np.int64)
    img = np.clip(img + rng.integers(-40, 41, img.shape), 0, 255).astype(np.uint8)
    img[: h // 5, : w // 4] = 255
    img[-(h // 5):, -(w // 4):] = 0
    img[h // 2:h // 2 + 4:2, ::2] = 255
    return img


def make_target(rng, h, w, image_id):
    """A few boxes, one of them small in a corner so that a crop can drop it."""
    boxes = [[1.0, 1.0, 5.5, 4.5], [w * 0.25, h * 0.2, w * 0.8, h * 0.9], [w * 0.5, h * 0.1, w - 1.0, h * 0.6]]
    b = torch.tensor(boxes, dtype=torch.float32)
    return {"boxes": b, "labels": torch.tensor([3, 7, 12]), "image_id": torch.tensor([image_id]),
            "area": (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]), "iscrowd": torch.zeros(3, dtype=torch.int64),
            "orig_size": torch.as_tensor([h, w]), "size": torch.as_tensor([h, w])}


def traced(T, trace):
    """Wrap the reference's module-level crop / hflip / resize (its classes call them by global name) to record what was drawn."""
    orig = (T.crop, T.hflip, T.resize)

    def crop(image, target, region):
        out = orig[0](image, target, region)
        trace.append(("crop",) + tuple(int(v) for v in region) + (int(tuple(region[2:]) == image.size[::-1]),
                                                                  int(len(out[1]["labels"]) < len(target["labels"]))))
        return out

    def hflip(image, target):
        trace.append(("hflip",))
        return orig[1](image, target)

    def resize(image, target, size, max_size=None):
        out = orig[2](image, target, size, max_size)
        clamp = 0
        if max_size is not None and not isinstance(size, (list, tuple)):
            w, h = image.size
            clamp = int(float(max(w, h)) / float(min(w, h)) * size > max_size)
        trace.append(("resize", out[0].size[1], out[0].size[0], clamp))
        return out
    T.crop, T.hflip, T.resize = crop, hflip, resize
    return orig


def run_batch(T, misc, kind, images, targets, seed):
    random.seed(seed)
    torch.manual_seed(seed)
    tf = pipeline(T, kind)
    traces, samples = [], []
    for img, tgt in zip(images, targets):
        tr = []
        orig = traced(T, tr)
        try:
            samples.append(tf(Image.fromarray(img), {k: v.clone() for k, v in tgt.items()}))
        finally:
            T.crop, T.hflip, T.resize = orig
        traces.append(tr)
    nt, tout = misc.collate_fn(samples)
    state = (random.getstate(), torch.get_rng_state())
    return nt.tensors, nt.mask, list(tout), traces, state


def branches(traces):
    s = set()
    for tr in traces:
        names = [t[0] for t in tr]
        s.add("flip" if "hflip" in names else "noflip")
        s.add("arm2" if "crop" in names else "arm1")
        for t in tr:
            if t[0] == "crop":
                if t[5]:
                    s.add("crop_equal")
                if t[6]:
                    s.add("crop_drops")
            if t[0] == "resize" and t[3]:
                s.add("clamp")
    return s


def restate(images, traces):
    """The recorded draws replayed through tests/resample_ref.py."""
    outs = []
    for img, tr in zip(images, traces):
        for t in tr:
            if t[0] == "hflip":
                img = img[:, ::-1]
            elif t[0] == "crop":
                img = img[t[1]:t[1] + t[3], t[2]:t[2] + t[4]]
            else:
                img = R.resize(img, t[1], t[2])
        outs.append(img)
    return R.collate(outs, R.norm_table(MEAN, STD))


def main():
    T, misc = load_reference()
    rng = np.random.default_rng(20261)
    # differing aspects in one batch: padding on the right of one image and below the other; 24 x 64 trips the max_size clamp
    shapes = {"a": [(40, 56), (52, 38)], "b": [(24, 64), (44, 48)]}
    images = {k: [make_image(rng, h, w) for h, w in v] for k, v in shapes.items()}
    targets = {k: [make_target(rng, h, w, 10 * (k == "b") + i) for i, (h, w) in enumerate(v)] for k, v in shapes.items()}
    want = {"flip", "noflip", "arm1", "arm2", "crop_equal", "crop_drops", "clamp"}

    # the fewest (pair, seed) train batches that cover every branch: greedy over seeds 0..399
    cand = {}
    for pair in ("a", "b"):
        for seed in range(400):
            cand[(pair, seed)] = branches(run_batch(T, misc, "train", images[pair], targets[pair], seed)[3])
    chosen, covered = [], set()
    while covered != want:
        best = max(sorted(cand), key=lambda k: len(cand[k] - covered))
        assert cand[best] - covered, f"no seed reaches {want - covered}"
        chosen.append(best)
        covered |= cand[best]
    jobs = [("train", p, s) for p, s in chosen] + [("val", "b", 1), ("fixed", "a", 2)]

    seen, count = set(), {}
    for kind, pair, seed in jobs:
        tensors, mask, tout, traces, state = run_batch(T, misc, kind, images[pair], targets[pair], seed)
        rt, rm = restate(images[pair], traces)
        assert torch.equal(rt, tensors) and torch.equal(rm, mask), (kind, pair, seed)
        if kind == "train":
            seen |= branches(traces)
        i = count.get(kind, 0)
        count[kind] = i + 1
        path = os.path.join(GOLD, f"transforms_{kind}{i}.pt")
        torch.save({"kind": kind, "max_size": MAX_SIZE, "seed": seed, "mean": MEAN, "std": STD,
                    "images": [torch.from_numpy(im.copy()) for im in images[pair]], "targets": targets[pair],
                    "trace": traces, "tensors": tensors, "mask": mask, "targets_out": tout,
                    "random_state": state[0], "torch_state": state[1]}, path)
        print(path, os.path.getsize(path), tuple(tensors.shape), traces)
    assert seen == want, want - seen


if __name__ == "__main__":
    main()
