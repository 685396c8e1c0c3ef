"""Record the reference's own pseudo_label_to_det_out (engine_loc.py:204-220) -> tests/golden/pseudo_det_out.pt.

    python tools/gen_pseudo_quality_golden.py

engine_loc is imported through tools/ref_harness (its torchvision and timm stand-ins) with an empty `cv2` module stubbed besides: the
module imports it at the top, the function never touches it.  Recorded: the pseudo labels of a few images (normalised cxcywh rows, some
reaching over the left and top border so that the clamp acts, one image without a row), the target sizes as the loader's integer
tensor and as floats, and for both what the reference returns.
Harness only: never imported by the package or on the GPU machine."""
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")


def reference_function():
    from tools import ref_harness
    ref_harness.install_shims()
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    import engine_loc
    return engine_loc.pseudo_label_to_det_out


def main():
    fn = reference_function()
    g = torch.Generator().manual_seed(44)
    pseudo = []
    for n in (3, 0, 17, 1):
        boxes = torch.cat([torch.rand(n, 2, generator=g), torch.rand(n, 2, generator=g) * 0.9], dim=1)
        if n > 2:
            boxes[0] = torch.tensor([0.05, 0.5, 0.4, 0.2])                       # x0 < 0: clamped
            boxes[1] = torch.tensor([0.5, 0.02, 0.2, 0.3])                       # y0 < 0: clamped
        pseudo.append({"boxes": boxes, "labels": torch.randint(1, 21, (n,), generator=g)})
    sizes = torch.tensor([[375, 500], [480, 640], [333, 1], [500, 281]])
    rec = {"pseudo": pseudo, "sizes_int": sizes, "sizes_float": sizes.float() + 0.5}
    for key in ("sizes_int", "sizes_float"):
        out = fn([dict(p) for p in pseudo], rec[key])
        rec["out_" + key] = [{k: v.clone() for k, v in r.items()} for r in out]
        assert all(r["scores"].dtype == torch.int64 for r in out)
    os.makedirs(GOLD, exist_ok=True)
    path = os.path.join(GOLD, "pseudo_det_out.pt")
    torch.save(rec, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
