"""NumPy / scipy.ndimage restatement of the labelling formulation behind csrc/cambox_labels.hip (spelled out in
csrc/cambox_index.h): every border of a Suzuki-Abe walk - its shoelace area, inclusive box and discovery position - from two
connected-component labellings of the zero-padded image, one 2x2 window per pixel and the tree the borders form (a border's
polygon encloses every border below it).  It shares no code with the kernels, with
the native border walk (csrc/cambox.hip) or with its NumPy restatement (oracle/cam_oracle.py); tests/test_cambox_ref_cpu.py
holds it against the latter two."""
import numpy as np
from scipy import ndimage

_FG8 = np.ones((3, 3), int)
_BG4 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])


def _first_index(lab, n):
    first = np.full(n + 1, lab.size, np.int64)
    np.minimum.at(first, lab.ravel(), np.arange(lab.size))
    return first


def _add_to_ancestors(is_hole, k, v, ftot, htot, flat_fl, flat_bl, ffirst, bfirst, frame):
    while True:
        if is_hole:
            k = flat_fl[bfirst[k] - 1]
            assert k > 0
            ftot[k] += v
        else:
            k = flat_bl[ffirst[k] - 1]
            assert k > 0
            if k == frame:
                return
            htot[k] += v
        is_hole = not is_hole


def borders(img):
    """-> list of (area, x0, y0, x1, y1), inclusive boxes in unpadded coordinates, in discovery (raster) order: what
    oracle.cam_oracle.find_borders returns."""
    R, C = img.shape
    W = C + 2
    f = np.zeros((R + 2, W), bool)
    f[1:-1, 1:-1] = img != 0
    fl, nf = ndimage.label(f, structure=_FG8)                 # foreground 8-connected
    bl, nb = ndimage.label(~f, structure=_BG4)                # background 4-connected
    frame = bl[0, 0]
    win = lambda a: [a[:-1, :-1], a[:-1, 1:], a[1:, :-1], a[1:, 1:]]
    fw, bw = win(fl), win(bl)
    nfg = sum((x > 0).astype(np.int64) for x in fw)
    cell_lab = np.maximum.reduce(fw)                          # all foreground pixels of a cell share one component
    area2 = np.zeros(nf + 1, np.int64)                        # half units
    np.add.at(area2, cell_lab[nfg == 4], 2)
    np.add.at(area2, cell_lab[nfg == 3], 1)
    hole2 = np.zeros(nb + 1, np.int64)
    for k in range(4):                                        # every distinct hole of a cell once
        new = (bw[k] > 0) & (bw[k] != frame)
        for j in range(k):
            new &= bw[j] != bw[k]
        cnt = sum((bw[j] == bw[k]).astype(np.int64) for j in range(k, 4))
        np.add.at(hole2, bw[k][new], np.where(cnt[new] >= 2, 2, 1))
    ffirst, bfirst = _first_index(fl, nf), _first_index(bl, nb)
    fbox, bbox = ndimage.find_objects(fl), ndimage.find_objects(bl)
    flat_fl, flat_bl = fl.ravel(), bl.ravel()
    # the border tree: a hole hangs under the component west of its first pixel, a component under the hole west of its first
    # pixel (none: the frame).  The polygon of a border encloses everything below it: every node counts for all its ancestors.
    ftot, htot = area2.copy(), hole2.copy()
    for s in range(1, nf + 1):
        _add_to_ancestors(False, s, area2[s], ftot, htot, flat_fl, flat_bl, ffirst, bfirst, frame)
    for h in range(1, nb + 1):
        if h != frame:
            _add_to_ancestors(True, h, hole2[h], ftot, htot, flat_fl, flat_bl, ffirst, bfirst, frame)
    res = []
    for s in range(1, nf + 1):
        ys, xs = fbox[s - 1]
        res.append((int(ffirst[s]), float(ftot[s]) * 0.5, xs.start - 1, ys.start - 1, xs.stop - 2, ys.stop - 2))
    for h in range(1, nb + 1):
        if h != frame:
            ys, xs = bbox[h - 1]
            res.append((int(bfirst[h]) - 1, float(htot[h]) * 0.5, xs.start - 2, ys.start - 2, xs.stop - 1, ys.stop - 1))
    res.sort(key=lambda r: r[0])
    assert len({r[0] for r in res}) == len(res)               # the discovery keys are distinct
    return [r[1:] for r in res]


def select(bs, area_ratio):
    """The selection of cams_deit.py:78-96 on a border list: boxes [x, y, x+w, y+h], largest area first, ties in discovery
    order; [[0, 0, 1, 1]] when there is no border.  area_ratio is taken as the float32 the C ABI receives."""
    if not bs:
        return [[0, 0, 1, 1]]
    order = sorted(range(len(bs)), key=lambda k: bs[k][0], reverse=True)       # stable
    top = bs[order[0]][0]
    ratio = float(np.float32(area_ratio))
    return [[bs[k][1], bs[k][2], bs[k][3] + 1, bs[k][4] + 1] for k in order if bs[k][0] >= top * ratio]
