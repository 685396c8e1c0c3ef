"""Named thresholded images for the CAM -> box tests (csrc/cambox_labels.hip, tests/cambox_ref.py): the smallest shapes at
which each rule of the labelling formulation can break.  Every image is uint8 [rows, cols], non-zero = foreground."""
import numpy as np


def _a(rows):
    return np.array([[1 if ch == "#" else 0 for ch in r] for r in rows], np.uint8) * 255


def _smooth(seed, rows, cols, sigma, level, pepper=0.0):
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    img = ndimage.gaussian_filter(rng.standard_normal((rows, cols)), sigma) > level
    if pepper:
        img &= rng.random((rows, cols)) >= pepper
    return img.astype(np.uint8) * 255


def _comb(rows, cols):
    """serpentine: full rows every second line, joined alternately at the right and the left end - one component whose
    label chain crosses every 64-pixel segment and every workgroup's rows; the background between is a comb of pockets"""
    a = np.zeros((rows, cols), np.uint8)
    a[::2, :] = 255
    for k, r in enumerate(range(1, rows - 1, 2)):
        a[r, cols - 1 if k % 2 == 0 else 0] = 255
    return a


def _width(cols):
    """blobs, a hole and a diagonal link placed across the 64-pixel segment boundary of the padded image (x = 63 / 64)"""
    a = np.zeros((9, cols), np.uint8)
    a[1, :] = 255                                   # a line over every segment
    a[3:8, max(0, cols - 8):cols] = 255             # block at the right edge ...
    a[5, cols - 3] = 0                              # ... with a one-pixel hole
    a[2, cols - 1] = 255                            # joined to the line
    if cols > 70:
        a[3:8, 58:68] = 255; a[4:7, 61:66] = 0     # a ring around the boundary, its hole spans it
        a[8, 57] = 255                              # diagonal spur
    return a


def small_cases():
    """-> list of (name, image); everything but the full-size map."""
    c = []
    c.append(("one_pixel", _a(["#"])))
    c.append(("all_zero", np.zeros((5, 7), np.uint8)))
    c.append(("all_ones", np.full((5, 7), 255, np.uint8)))
    c.append(("pixel_hole", _a(["###", "#.#", "###"])))
    c.append(("diagonal_blobs", _a(["##...", "##...", "..###", "..###"])))
    c.append(("diagonal_ring", _a([".##..", "#..#.", "#..#.", ".##.."])))                # closed only by diagonal links
    c.append(("two_holes_one_cell", _a(["#####", "#.###", "##.##", "#####"])))             # holes meet across a diagonal
    c.append(("two_holes_big", _a(["######", "#..###", "#..###", "###..#", "###..#", "######"])))
    c.append(("nested", _a(["#########", "#.......#", "#.#####.#", "#.#...#.#", "#.#.#.#.#", "#.#...#.#", "#.#####.#", "#.......#",
                            "#########"])))                                            # island in a hole in a blob in a hole
    c.append(("edge_pocket", _a(["##.##", "#...#", "#####", ".....", "#.#.."])))           # open to the edge: not a hole
    c.append(("lines_spurs", _a(["#......#", "#..#...#", "####.###", "...#.#..", "...###..", ".#......", "..#....#"])))
    c.append(("equal_blobs", _a(["###..###", "###..###", "........", ".###....", ".###...."])))
    c.append(("tie_hole_outer", _a(["#####....", "#...#.###", "#...#.###", "#####.###"])))
    chk = np.zeros((12, 13), np.uint8); chk[::2, ::2] = 255; chk[1::2, 1::2] = 255
    c.append(("checkerboard", chk))
    c.append(("comb", _comb(70, 300)))
    c.append(("serpentine_T", np.ascontiguousarray(_comb(64, 131).T)))
    for w in (61, 62, 63, 64, 65, 255, 257):                                            # image and padded widths 63, 64, 65, 257
        c.append((f"width{w}", _width(w)))
    rng = np.random.default_rng(7)
    for d in (0.2, 0.5, 0.8, 0.95):
        c.append((f"noise{int(d * 100)}", (rng.random((37, 71)) < d).astype(np.uint8) * 255))
    c.append(("blobs_a", _smooth(11, 40, 56, 2.0, 0.0)))
    c.append(("blobs_b", _smooth(12, 64, 130, 3.0, 0.02)))
    c.append(("blobs_pepper", _smooth(13, 48, 90, 2.0, -0.1, pepper=0.07)))
    c.append(("blobs_pepper_tall", _smooth(14, 131, 33, 2.5, -0.05, pepper=0.04)))
    return c


FULL_ROWS, FULL_COLS = 1333, 800


def full_size_case():
    """one full-size smooth map, 1333 rows x 800 columns (an 800 x 1333 image after the reference's (H, W) -> dsize quirk): bumps
    plus a ripple, thresholded at 20 % as the driver does"""
    g = np.random.default_rng(21)
    yy, xx = np.meshgrid(np.arange(FULL_ROWS, dtype=np.float32), np.arange(FULL_COLS, dtype=np.float32), indexing="ij")
    m = np.zeros((FULL_ROWS, FULL_COLS), np.float32)
    for _ in range(5):
        cy, cx = g.random() * FULL_ROWS, g.random() * FULL_COLS
        s = 60.0 + 140.0 * g.random()
        m += (0.4 + g.random()) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    m += 0.04 * np.sin(yy / 9.0) * np.cos(xx / 7.0)
    m -= m.min(); m /= m.max()
    q = (m * 255.0).astype(np.uint8)
    return "full_size", np.where(q > int(0.2 * 255), q, 0).astype(np.uint8)


RATIOS = (0.0, 0.5, 1.0)
