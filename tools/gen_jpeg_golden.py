"""Write tests/golden/jpeg_small.pt and tests/golden/jpeg_voc.pt: JPEG files encoded by Pillow (tests/jpeg_cases.py) with Pillow's
own decode of each, the yardstick of spe_amd.jpeg.  Needs Pillow, which the machine that runs the GPU tests may not have - hence
recorded files.

    python tools/gen_jpeg_golden.py                  # the two fixtures
    python tools/gen_jpeg_golden.py --dump-dir DIR   # also every file of the full grid as DIR/<case>.jpg (tools/jpeg_host_check.cpp)
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_cases as C  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump-dir")
    args = ap.parse_args()
    import PIL
    small = {}
    for case in C.SMALL:
        data = C.make(*case)
        small[C.name(*case)] = {"data": torch.frombuffer(bytearray(data), dtype=torch.uint8).clone(),
                                "rgb": torch.from_numpy(C.pillow_rgb(data).copy())}
    torch.save(small, os.path.join(C.GOLD, "jpeg_small.pt"))
    voc = C.voc_file()
    rgb = C.pillow_rgb(voc)
    sha = hashlib.sha256(np.ascontiguousarray(rgb).tobytes()).digest()
    torch.save({"data": torch.frombuffer(bytearray(voc), dtype=torch.uint8).clone(),
                "sha256": torch.frombuffer(bytearray(sha), dtype=torch.uint8).clone()}, os.path.join(C.GOLD, "jpeg_voc.pt"))
    for f in ("jpeg_small.pt", "jpeg_voc.pt"):
        print(f, os.path.getsize(os.path.join(C.GOLD, f)), "bytes")
    print("Pillow", PIL.__version__, "-", len(small), "small cases, voc file", len(voc), "bytes, sha256", sha.hex())
    if args.dump_dir:
        os.makedirs(args.dump_dir, exist_ok=True)
        for case in C.GRID:
            with open(os.path.join(args.dump_dir, C.name(*case) + ".jpg"), "wb") as fh:
                fh.write(C.make(*case))
        with open(os.path.join(args.dump_dir, "voc.jpg"), "wb") as fh:
            fh.write(voc)
        print(len(C.GRID) + 1, "files in", args.dump_dir)


if __name__ == "__main__":
    main()
