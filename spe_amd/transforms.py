"""Input transforms on the device (reference datasets/transforms.py + util/misc.collate_fn).

The reference module's names and calling convention, `(img, target) -> (img, target)`, with the pixel work deferred: `img` is a
lazy DeviceImage - a uint8 [H,W,3] tensor on the device plus the list of pending stages - and collate_fn executes the pending
stages of the whole batch in batched launches (spe_amd.kernels.resample_batch): Pillow's bilinear resize bit for bit, crop and
flip folded into the source index map, ToTensor + Normalize as a 3 x 256 table and the zero padding in the last pass's epilogue.

Random numbers are drawn exactly where the reference draws them, in the same order, from the same generators (Python's `random`;
`torch.randint` for the crop origin, with torchvision's RandomCrop.get_params semantics since 0.8).  The target side runs eagerly
on the host with the reference's fp32 torch operations.  Segmentation masks, RandomPad and RandomErasing are not built.

decode_jpeg turns file bytes into DeviceImages (spe_amd.jpeg: Huffman decoding on the host, everything after it on the device), so a
loader can hand the files through as they are."""
import random

import torch

from . import kernels as K
from .util.box_ops import box_xyxy_to_cxcywh
from .util.misc import NestedTensor


class DeviceImage:
    """uint8 [H,W,3] on the device + pending stages.  `stages`: finished resize steps (x0, y0, cw, ch, flip, oh, ow), each reading
    the output of the one before (the first one reads `data`); `box` / `flip`: the crop and flip pending on top of the last of them.
    `.size` is the current (w, h), as with PIL.  Operations return a new DeviceImage over the same data."""

    def __init__(self, data, device="cuda", _stages=(), _box=None, _flip=False):
        if not torch.is_tensor(data) or data.dtype != torch.uint8 or data.ndim != 3 or data.shape[2] != 3:
            raise TypeError("DeviceImage: expected a uint8 [H,W,3] tensor")
        if device is not None and not data.is_cuda:       # device=None keeps a host tensor: planning works, the kernels refuse it
            data = data.to(device, non_blocking=True)
        self.data = data.contiguous()
        self.stages = tuple(_stages)
        self.box = tuple(_box) if _box is not None else (0, 0, int(data.shape[1]), int(data.shape[0]))      # x0, y0, cw, ch
        self.flip = bool(_flip)

    @property
    def size(self):
        return (self.box[2], self.box[3])

    @property
    def width(self):
        return self.box[2]

    @property
    def height(self):
        return self.box[3]

    def _new(self, stages, box, flip):
        return DeviceImage(self.data, device=None, _stages=stages, _box=box, _flip=flip)

    def hflip(self):
        return self._new(self.stages, self.box, not self.flip)

    def crop(self, top, left, height, width):
        x0, y0, cw, ch = self.box
        # under a flip the view's column j is source column x0 + cw - 1 - j: the new box starts where the view's last column lies
        nx = x0 + (cw - left - width if self.flip else left)
        return self._new(self.stages, (nx, y0 + top, width, height), self.flip)

    def resize(self, oh, ow):
        st = self.stages + (self.box + (self.flip, int(oh), int(ow)),)
        return self._new(st, (0, 0, int(ow), int(oh)), False)


def decode_jpeg(datas, device="cuda", **kw):
    """[file bytes, ...] -> [DeviceImage, ...], equal to DeviceImage(np.asarray(Image.open(f).convert("RGB"))) bit for bit.  Keyword
    arguments go to spe_amd.jpeg.decode_batch (threads, fallback)."""
    from . import jpeg
    return [DeviceImage(t, device=device) for t in jpeg.decode_batch(datas, device=device, **kw)]


class PendingTensor:
    """What ToTensor returns: the image that collate_fn will write as fp32 [3,h,w], normalised when Normalize has seen it."""

    def __init__(self, image, mean=None, std=None):
        self.image, self.mean, self.std = image, mean, std

    @property
    def shape(self):
        return (3, self.image.height, self.image.width)


def _pixels(img, what):
    if not isinstance(img, DeviceImage):
        raise TypeError(f"{what}: expected a DeviceImage (pixel transforms come before ToTensor), got {type(img).__name__}")
    return img


def _no_masks(target):
    if target is not None and "masks" in target:
        raise NotImplementedError("spe_amd.transforms: segmentation masks in a target are not supported")


def crop(image, target, region):
    _no_masks(target)
    i, j, h, w = region
    cropped_image = _pixels(image, "crop").crop(i, j, h, w)
    target = target.copy()
    target["size"] = torch.tensor([h, w])
    fields = ["labels", "area", "iscrowd"]
    if "boxes" in target:
        boxes = target["boxes"]
        max_size = torch.as_tensor([w, h], dtype=torch.float32)
        cropped_boxes = boxes - torch.as_tensor([j, i, j, i])
        cropped_boxes = torch.min(cropped_boxes.reshape(-1, 2, 2), max_size)
        cropped_boxes = cropped_boxes.clamp(min=0)
        area = (cropped_boxes[:, 1, :] - cropped_boxes[:, 0, :]).prod(dim=1)
        target["boxes"] = cropped_boxes.reshape(-1, 4)
        target["area"] = area
        fields.append("boxes")
        # boxes the crop left without area go, and their labels / area / iscrowd with them
        cb = target["boxes"].reshape(-1, 2, 2)
        keep = torch.all(cb[:, 1, :] > cb[:, 0, :], dim=1)
        for field in fields:
            target[field] = target[field][keep]
    return cropped_image, target


def hflip(image, target):
    _no_masks(target)
    w, h = _pixels(image, "hflip").size
    flipped = image.hflip()
    target = target.copy()
    if "boxes" in target:
        boxes = target["boxes"]
        target["boxes"] = boxes[:, [2, 1, 0, 3]] * torch.as_tensor([-1, 1, -1, 1]) + torch.as_tensor([w, 0, w, 0])
    return flipped, target


def get_size_with_aspect_ratio(image_size, size, max_size=None):
    w, h = image_size
    if max_size is not None:
        min_original_size = float(min((w, h)))
        max_original_size = float(max((w, h)))
        if max_original_size / min_original_size * size > max_size:
            size = int(round(max_size * min_original_size / max_original_size))
    if (w <= h and w == size) or (h <= w and h == size):
        return (h, w)
    if w < h:
        ow = size
        oh = int(size * h / w)
    else:
        oh = size
        ow = int(size * w / h)
    return (oh, ow)


def resize(image, target, size, max_size=None):
    """size: the shorter side (scalar) or a (w, h) pair."""
    _no_masks(target)
    old = _pixels(image, "resize").size
    if isinstance(size, (list, tuple)):
        size = size[::-1]
    else:
        size = get_size_with_aspect_ratio(old, size, max_size)
    rescaled = image.resize(size[0], size[1])
    if target is None:
        return rescaled, None
    ratio_width, ratio_height = tuple(float(s) / float(s_orig) for s, s_orig in zip(rescaled.size, old))
    target = target.copy()
    if "boxes" in target:
        target["boxes"] = target["boxes"] * torch.as_tensor([ratio_width, ratio_height, ratio_width, ratio_height])
    if "area" in target:
        target["area"] = target["area"] * (ratio_width * ratio_height)
    h, w = size
    target["size"] = torch.tensor([h, w])
    return rescaled, target


def _crop_params(img, output_size):
    """torchvision.transforms.RandomCrop.get_params (>= 0.8): torch's generator, no draw when the crop equals the image."""
    w, h = img.size
    th, tw = output_size
    if h + 1 < th or w + 1 < tw:
        raise ValueError(f"Required crop size {(th, tw)} is larger then input image size {(h, w)}")
    if w == tw and h == th:
        return 0, 0, h, w
    i = torch.randint(0, h - th + 1, size=(1,)).item()
    j = torch.randint(0, w - tw + 1, size=(1,)).item()
    return i, j, th, tw


class RandomCrop(object):
    def __init__(self, size):
        self.size = size

    def __call__(self, img, target):
        return crop(img, target, _crop_params(_pixels(img, "RandomCrop"), self.size))


class RandomSizeCrop(object):
    def __init__(self, min_size, max_size):
        self.min_size = min_size
        self.max_size = max_size

    def __call__(self, img, target):
        _pixels(img, "RandomSizeCrop")
        w = random.randint(self.min_size, min(img.width, self.max_size))
        h = random.randint(self.min_size, min(img.height, self.max_size))
        return crop(img, target, _crop_params(img, [h, w]))


class CenterCrop(object):
    def __init__(self, size):
        self.size = size

    def __call__(self, img, target):
        image_width, image_height = _pixels(img, "CenterCrop").size
        crop_height, crop_width = self.size
        crop_top = int(round((image_height - crop_height) / 2.))
        crop_left = int(round((image_width - crop_width) / 2.))
        return crop(img, target, (crop_top, crop_left, crop_height, crop_width))


class RandomHorizontalFlip(object):
    def __init__(self, p=0.5):
        self.p = p

    def __call__(self, img, target):
        if random.random() < self.p:
            return hflip(img, target)
        return img, target


class RandomResize(object):
    def __init__(self, sizes, max_size=None):
        assert isinstance(sizes, (list, tuple))
        self.sizes = sizes
        self.max_size = max_size

    def __call__(self, img, target=None):
        size = random.choice(self.sizes)
        return resize(img, target, size, self.max_size)


class Resize(object):
    def __init__(self, target_size, max_size):
        self.target_size = target_size
        self.max_size = max_size

    def __call__(self, img, target=None):
        return resize(img, target, self.target_size, self.max_size)


class RandomSelect(object):
    """transforms1 with probability p, else transforms2."""

    def __init__(self, transforms1, transforms2, p=0.5):
        self.transforms1 = transforms1
        self.transforms2 = transforms2
        self.p = p

    def __call__(self, img, target):
        if random.random() < self.p:
            return self.transforms1(img, target)
        return self.transforms2(img, target)


class ToTensor(object):
    def __call__(self, img, target):
        return PendingTensor(_pixels(img, "ToTensor")), target


class Normalize(object):
    def __init__(self, mean, std):
        self.mean = mean
        self.std = std

    def __call__(self, image, target=None):
        if not isinstance(image, PendingTensor):
            raise TypeError(f"Normalize: expected the output of ToTensor, got {type(image).__name__}")
        image = PendingTensor(image.image, tuple(self.mean), tuple(self.std))
        if target is None:
            return image, None
        target = target.copy()
        h, w = image.shape[-2:]
        if "boxes" in target:
            boxes = box_xyxy_to_cxcywh(target["boxes"])
            target["boxes"] = boxes / torch.tensor([w, h, w, h], dtype=torch.float32)
        return image, target


class Compose(object):
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, image, target):
        for t in self.transforms:
            image, target = t(image, target)
        return image, target

    def __repr__(self):
        return self.__class__.__name__ + "(" + "".join("\n    {0}".format(t) for t in self.transforms) + "\n)"


def make_transforms(image_set, max_size=1333, fixed=False):
    """The three factories of the reference's datasets/voc.py / coco.py: make_coco_transforms (max_size 1333),
    make_coco_transforms_specific_size (any max_size) and, with fixed=True, make_coco_transforms_specific_size_fixed."""
    normalize = Compose([ToTensor(), Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])])
    if image_set not in ("train", "val"):
        raise ValueError(f"unknown {image_set}")
    if fixed:
        head = [RandomHorizontalFlip()] if image_set == "train" else []
        return Compose(head + [Resize((max_size, max_size), max_size=max_size), normalize])
    scales = [s * max_size // 1333 for s in (480, 512, 544, 576, 608, 640, 672, 704, 736, 768, 800)]
    random_size = [r * max_size // 1333 for r in (400, 500, 600)]
    crop_size = [c * max_size // 1333 for c in (384, 600)]
    if image_set == "train":
        return Compose([
            RandomHorizontalFlip(),
            RandomSelect(
                RandomResize(scales, max_size=max_size),
                Compose([RandomResize(random_size), RandomSizeCrop(*crop_size), RandomResize(scales, max_size=max_size)])),
            normalize])
    return Compose([RandomResize([800 * max_size // 1333], max_size=max_size), normalize])


def norm_table(mean, std, device):
    """ToTensor + Normalize per (channel, byte), computed by torch CPU fp32 exactly as the reference computes every pixel."""
    base = torch.arange(256).float().div(255)
    rows = [base if mean is None else base.sub(mean[c]).div(std[c]) for c in range(3)]
    return torch.stack(rows).to(device, non_blocking=True)


_TABLES = {}


def plan_stages(image):
    """The resize launches an image needs: its finished stages plus the pending crop / flip (a resize to the same size when no
    resize follows it - taps (2^22, 0), the bytes themselves)."""
    x0, y0, cw, ch = image.box
    if not image.stages or image.flip or (x0, y0) != (0, 0) or (ch, cw) != image.stages[-1][5:7]:
        return image.stages + (image.box + (image.flip, ch, cw),)
    return image.stages


def batch_shape(images):
    """(B, 3, Hmax, Wmax) of the batch collate_fn builds from these PendingTensors."""
    return (len(images), 3, max(t.shape[1] for t in images), max(t.shape[2] for t in images))


def collate_fn(batch, out=None):
    """[(PendingTensor, target), ...] -> (NestedTensor, targets): runs every pending stage of the batch.  All stages but an image's
    last one go through uint8 images, one round of launches per depth for all images that have one; the last stages of all images
    are one round that writes the padded fp32 batch and its mask.  out = (tensors, mask): fp32 / bool buffers with at least
    B*3*Hmax*Wmax / B*Hmax*Wmax elements, reused; the result are views of their leading elements."""
    batch = list(zip(*batch))
    imgs = batch[0]
    for t in imgs:
        if not isinstance(t, PendingTensor):
            raise TypeError(f"collate_fn: expected the output of ToTensor, got {type(t).__name__}")
    key = (imgs[0].mean, imgs[0].std)
    if any((t.mean, t.std) != key for t in imgs):
        raise ValueError("collate_fn: one batch, one normalisation")
    dev = imgs[0].image.data.device
    lut = _TABLES.get((key, dev))
    if lut is None:
        lut = _TABLES[(key, dev)] = norm_table(key[0], key[1], dev)
    stages = [list(plan_stages(t.image)) for t in imgs]
    cur = [t.image.data for t in imgs]

    def job(i):                                   # the image's next stage as resample_batch takes it
        x0, y0, cw, ch, flip, oh, ow = stages[i][0]
        return cur[i], (x0, y0, cw, ch), flip, (oh, ow)
    while True:
        idx = [i for i, s in enumerate(stages) if len(s) > 1]
        if not idx:
            break
        res = K.resample_batch([job(i) for i in idx])
        for i, r in zip(idx, res):
            cur[i] = r
            stages[i].pop(0)
    B, _, H, W = batch_shape(imgs)
    if out is None:
        tensors = torch.empty((B, 3, H, W), device=dev, dtype=torch.float32)
        mask = torch.empty((B, H, W), device=dev, dtype=torch.bool)
    else:
        tb, mb = out
        if tb.dtype != torch.float32 or mb.dtype != torch.bool or not tb.is_contiguous() or not mb.is_contiguous() or \
                tb.numel() < B * 3 * H * W or mb.numel() < B * H * W:
            raise ValueError(f"collate_fn: out needs contiguous fp32 / bool buffers of at least {B * 3 * H * W} / {B * H * W} elements")
        tensors = tb.view(-1)[:B * 3 * H * W].view(B, 3, H, W)
        mask = mb.view(-1)[:B * H * W].view(B, H, W)
    K.resample_batch([job(i) for i in range(B)], lut=lut, out=tensors, mask=mask)
    batch[0] = NestedTensor(tensors, mask)
    return tuple(batch)
