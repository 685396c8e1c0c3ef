"""The labelling formulation of the CAM -> box step on the CPU: its NumPy restatement (tests/cambox_ref.py) against the border
walks (oracle/cam_oracle.py in NumPy, csrc/cambox.hip natively), and the kernels' own index arithmetic (csrc/cambox_index.h) run
serially by tools/micro/cambox_host.hip under the host address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import cambox_cases as cc  # noqa: E402
import cambox_ref as cr  # noqa: E402
from oracle import cam_oracle as CO  # noqa: E402

SMALL = cc.small_cases()


def test_case_list_covers_the_edges():
    names = [n for n, _ in SMALL]
    assert len(set(names)) == len(names)
    shapes = {im.shape for _, im in SMALL}
    assert (1, 1) in shapes and (70, 300) in shapes
    assert {61, 62, 63, 64, 65, 255, 257} <= {im.shape[1] for _, im in SMALL}
    assert all(im.dtype == np.uint8 and im.shape[0] * im.shape[1] <= 70 * 300 for _, im in SMALL)


@pytest.mark.parametrize("name,img", SMALL, ids=[n for n, _ in SMALL])
def test_restatement_equals_the_border_walk(name, img):
    """areas, boxes and discovery order of every border, as lists of tuples; then the selection at each ratio"""
    walked = CO.find_borders(img)
    bs = cr.borders(img)
    assert bs == walked
    for ratio in cc.RATIOS:
        assert cr.select(bs, ratio) == CO.multi_bboxes_from_image(img, ratio), ratio


def test_known_answers():
    by = dict(SMALL)
    assert cr.borders(by["one_pixel"]) == [(0.0, 0, 0, 0, 0)]
    assert cr.borders(by["all_zero"]) == [] and cr.select([], 0.5) == [[0, 0, 1, 1]]
    assert cr.borders(by["all_ones"]) == [(24.0, 0, 0, 6, 4)]                              # (w-1)(h-1)
    assert cr.borders(by["pixel_hole"]) == [(4.0, 0, 0, 2, 2), (2.0, 0, 0, 2, 2)]            # the hole border is a diamond
    assert len(cr.borders(by["diagonal_blobs"])) == 1                                       # 8-connected: one component
    assert len(cr.borders(by["diagonal_ring"])) == 2                                        # 4-connected inside: a hole
    assert len(cr.borders(by["two_holes_one_cell"])) == 3
    assert len(cr.borders(by["nested"])) == 5
    assert len(cr.borders(by["edge_pocket"])) == 3                                          # three components, no hole
    assert len(cr.borders(by["comb"])) == 1


def test_restatement_equals_the_native_walk_at_full_size():
    """the Python walk is too slow at 1333 x 800: the native host walk (csrc/cambox.hip) is the reference there"""
    from spe_amd import kernels as K
    name, img = cc.full_size_case()
    assert img.shape == (cc.FULL_ROWS, cc.FULL_COLS)
    bs = cr.borders(img)
    assert len(bs) > 3
    t = torch.from_numpy(img)
    for ratio in cc.RATIOS:
        assert cr.select(bs, ratio) == K.cam_contour_boxes(t, ratio, max_boxes=8192).tolist(), ratio


def test_index_arithmetic_under_host_sanitizers(tmp_path):
    """tools/micro/cambox_host.hip: the whole formulation, serially, through the functions of csrc/cambox_index.h that the kernels
    call, built with -fsanitize=address,undefined for the host and run as a child process over every small case and ratio; a
    second pass at max_boxes = 2 exercises the overflow status."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "cambox_host")
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "spe_amd", "csrc"),
           os.path.join(ROOT, "tools", "micro", "cambox_host.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and any(w in r.stderr for w in ("clang_rt", "libclang_rt", "asan", "ubsan")):
        pytest.skip("sanitizer runtime not installed: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    runs = [(n, im, ratio, 4096) for n, im in SMALL for ratio in cc.RATIOS] + [(n, im, 0.0, 2) for n, im in SMALL]
    path = tmp_path / "cases.txt"
    with open(path, "w") as fh:
        for n, im, ratio, mb in runs:
            fh.write(f"{n} {im.shape[0]} {im.shape[1]} {ratio} {mb}\n")
            for row in im:
                fh.write("".join("1" if v else "0" for v in row) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == f"done {len(runs)}"
    walked = {n: CO.find_borders(im) for n, im in SMALL}
    k = 0
    for n, im, ratio, mb in runs:
        tag, name, nb, status, ns = lines[k].split()
        assert tag == "case" and name == n
        nb, status, ns = int(nb), int(status), int(ns)
        bs = [tuple(int(v) for v in ln.split()[1:]) for ln in lines[k + 1:k + 1 + nb]]
        sel = [[int(v) for v in ln.split()[1:]] for ln in lines[k + 1 + nb:k + 1 + nb + ns]]
        k += 1 + nb + ns
        assert [(a2 * 0.5, x0, y0, x1, y1) for a2, x0, y0, x1, y1 in bs] == walked[n], (n, ratio)
        want = CO.multi_bboxes_from_image(im, ratio)
        if len(want) > mb:
            assert status == -5 and ns == 0, (n, mb)
        else:
            assert status == 0 and sel == want, (n, ratio, mb)
    assert k == len(lines) - 1
