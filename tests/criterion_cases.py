"""The inputs of tests/test_criterion_ref_cpu.py and tests/test_criterion_kernels_gpu.py: one list of cases per kernel of csrc/loss.hip,
each at the sizes where its launcher or its loops change path, and the seeded generators of their tensors (CPU tensors; the GPU module
moves them).  Both modules import this file, so the conditions the CPU module checks (a unique optimum, ties that coincide in fp32 and
fp64, logits away from the clamp threshold) hold for exactly the inputs the kernels see."""
import torch

# ------------------------------------------------------------------------------------------------------------------------------
# assignment: (L, Q, sizes).  spe_hungarian picks CPL = 2 / 5 / 8 / 16 at Q <= 128 / 320 / 512 / 1024 and stages a problem's costs in
# LDS when n * m <= 36 864 floats
# ------------------------------------------------------------------------------------------------------------------------------
HUNG_LDS_FLOATS = 36 * 1024
HUNG_CASES = [
    (1, 1, [1]),
    (2, 2, [2, 1, 0]),
    (1, 63, [63]),
    (1, 64, [64, 1]),
    (1, 65, [65, 3]),
    (2, 128, [128, 0, 17]),          # CPL 2, its last Q
    (1, 129, [129, 5]),              # CPL 5, its first Q
    (1, 192, [192]),                 # n m = 36 864: the last staged size
    (1, 193, [191, 192]),            # 36 863 staged and 37 056 unstaged in one launch
    (1, 320, [115, 116]),            # 36 800 staged / 37 120 unstaged; CPL 5, its last Q
    (1, 321, [40]),                  # CPL 8, its first Q
    (1, 512, [72, 73]),              # 36 864 staged / 37 376 unstaged; CPL 8, its last Q
    (1, 513, [30]),                  # CPL 16, its first Q
    (1, 1024, [36, 37, 1]),          # staged / unstaged at the largest Q
    (3, 300, [60, 0, 35]),           # the training shape
]
HUNG_FAMILIES = ("cont", "mixed_scale", "int4", "dupcol", "const", "zeros_signed")
HUNG_UNIQUE = ("cont", "mixed_scale")           # families whose optimum must be unique: SciPy's pairs may be demanded
HUNG_INTEGER = ("int4", "const", "zeros_signed")
# mixed_scale draws from a grid of 1/16 (fp32 at 1e6), where two assignments can tie exactly: these cases take a later seed, found by
# tests/test_criterion_ref_cpu.py's condition (lowest-index pairs == SciPy's pairs on every block)
HUNG_RESEED = {(4, "mixed_scale"): 2, (6, "mixed_scale"): 2, (8, "mixed_scale"): 6, (9, "mixed_scale"): 1, (14, "mixed_scale"): 3}


def hung_id(case):
    L, Q, sizes = case
    return f"L{L}-Q{Q}-" + "_".join(str(s) for s in sizes)


def hung_cost(case, fam):
    """-> (cost [L, Q * total] fp32: block b is the row-major [Q, M_b] matrix at Q * toff[b]; base [total] int64 or None: for dupcol,
    which base column each target copies (ids local to its image))."""
    L, Q, sizes = case
    idx = HUNG_CASES.index(case)
    g = torch.Generator().manual_seed(7919 * idx + 31 * HUNG_FAMILIES.index(fam) + 104729 * HUNG_RESEED.get((idx, fam), 0))
    total = sum(sizes)
    cost = torch.empty(L, Q * total)
    base = torch.zeros(total, dtype=torch.int64) if fam == "dupcol" else None
    off = 0
    for n in sizes:
        if n == 0:
            continue
        if fam == "dupcol":
            nb = (n + 2) // 3
            ids = torch.randint(0, nb, (n,), generator=g)
            base[off:off + n] = ids
        for l in range(L):
            if fam == "cont":
                blk = 3 * torch.randn(Q, n, generator=g)
            elif fam == "mixed_scale":
                # neighbouring values one ulp apart.  "Half the columns" flipped, in the kernel's sense of column: hungarian_kernel's columns
                # are the queries (its lanes own them), the rows of this [Q, n] block - so both key ranges meet in one hung_wave_umin
                blk = 1e6 + torch.randn(Q, n, generator=g)
                blk[1::2] *= -1
            elif fam == "int4":
                blk = torch.randint(0, 4, (Q, n), generator=g).float()
            elif fam == "dupcol":
                blk = (3 * torch.randn(Q, nb, generator=g))[:, ids]
            elif fam == "const":
                blk = torch.full((Q, n), 2.5)
            elif fam == "zeros_signed":
                blk = torch.tensor([-0.0, 0.0, 1.0])[torch.randint(0, 3, (Q, n), generator=g)]
            else:
                raise KeyError(fam)
            cost[l, Q * off:Q * (off + n)] = blk.reshape(-1)
        off += n
    return cost, base


# ------------------------------------------------------------------------------------------------------------------------------
# focal loss: (L, R, Kc).  One wave per row, four rows per workgroup, lanes stride the classes by 64; the layer's loss is summed over
# ceil(R / 4) workgroups in groups of 16, then over the groups 16 at a time
# ------------------------------------------------------------------------------------------------------------------------------
FOCAL_R = (1, 3, 4, 5, 64, 65, 1024, 1028)       # 1, 1, 1, 2, 16, 17, 256, 257 row blocks
FOCAL_KC = (1, 20, 63, 64, 65, 91, 130)
FOCAL_SHAPES = sorted({(L, R, 91) for L in (1, 3) for R in FOCAL_R} | {(L, 65, Kc) for L in (1, 3) for Kc in FOCAL_KC})
FOCAL_FAMILIES = ("plain", "saturated", "ties")
FOCAL_PARAMS = ((0.25, 2.0), (0.25, 0.5), (-1.0, 2.0), (0.25, 0.0))         # (alpha, gamma)
FOCAL_GRID = (12.0, 15.0, 20.0, 30.0, 88.0, 100.0)          # |logit| of `saturated`: none within 0.25 of the clamp threshold 11.5129


def focal_inputs(L, R, Kc, fam):
    """-> logits [L,R,Kc], tclass [L,R] int32 in [0, Kc] (the last row of every layer: Kc, no object), roww [L,R] in (0, 1)."""
    g = torch.Generator().manual_seed(10007 * R + 101 * Kc + 7 * L + FOCAL_FAMILIES.index(fam))
    if fam == "plain":
        x = 2 * torch.randn(L, R, Kc, generator=g)
    elif fam == "saturated":
        x = torch.tensor(FOCAL_GRID)[torch.randint(0, len(FOCAL_GRID), (L, R, Kc), generator=g)]
        x = x * torch.where(torch.rand(L, R, Kc, generator=g) < 0.5, -1.0, 1.0)
    elif fam == "ties":            # below 3 everywhere, then 5.0 in two or three columns; every fourth row all equal
        x = (2 * torch.randn(L, R, Kc, generator=g)).clamp(max=3.0)
        for l in range(L):
            for r in range(R):
                kind = (r + l) % 4
                if kind == 0 or Kc < 2:
                    x[l, r] = 1.25
                    continue
                k = min(2 + (r // 4) % 2, Kc)
                perm = torch.randperm(Kc, generator=g)
                if Kc > 65 and kind == 1:                  # all tied maxima in the lanes' second pass
                    cols = 64 + torch.randperm(Kc - 64, generator=g)[:k]
                elif Kc > 64 and kind == 2:                # one lane holds a tied maximum in each of its passes
                    c0 = int(torch.randint(0, Kc - 64, (1,), generator=g))
                    cols = torch.tensor([c0, c0 + 64] + ([int(perm[0])] if k == 3 else []))
                else:
                    cols = perm[:k]
                x[l, r, cols] = 5.0
    else:
        raise KeyError(fam)
    tclass = torch.randint(0, Kc + 1, (L, R), generator=g).int()
    tclass[:, -1] = Kc
    roww = torch.rand(L, R, generator=g) * 0.9 + 0.1
    return x, tclass, roww


# ------------------------------------------------------------------------------------------------------------------------------
# box losses: n pairs pass through LDS in chunks of 1024; thread (l, k) of the one workgroup sums layer l
# ------------------------------------------------------------------------------------------------------------------------------
BOX_CASES = [(n, L) for n in (1, 1023, 1024, 1025, 2049) for L in (1, 6)] + [(600, 512)]
BOX_FAMILIES = ("plain", "dyadic")
BOX_L_REFUSED = 513
BWD_N = (1, 63, 64, 65)                      # n * 4 = 4, 252, 256, 260 elements: below, at and across the 256-thread block


def rand_boxes(n, g):
    """cxcywh, centre in [0.2, 0.8], size in [0.05, 0.4] (the boxes of tests/test_kernels_gpu.py)."""
    c = torch.rand(n, 2, generator=g) * 0.6 + 0.2
    wh = torch.rand(n, 2, generator=g) * 0.35 + 0.05
    return torch.cat([c, wh], 1)


def _xyxy64(x0, y0, x1, y1):
    """xyxy in units of 1/64 -> cxcywh in units of 1/64; the centre must come out whole."""
    assert (x0 + x1) % 2 == 0 and (y0 + y1) % 2 == 0
    return [(x0 + x1) // 2, (y0 + y1) // 2, x1 - x0, y1 - y0]


# (prediction, target) in units of 1/64
DYADIC_SPECIAL = [
    (_xyxy64(16, 16, 40, 40), _xyxy64(16, 16, 40, 40)),            # identical
    (_xyxy64(16, 16, 40, 40), _xyxy64(16, 20, 48, 52)),            # one shared edge
    (_xyxy64(16, 16, 40, 40), _xyxy64(16, 16, 48, 52)),            # two
    (_xyxy64(16, 16, 40, 40), _xyxy64(16, 16, 40, 56)),            # three
    (_xyxy64(10, 10, 54, 54), _xyxy64(20, 22, 40, 44)),            # target nested in the prediction
    (_xyxy64(20, 22, 40, 44), _xyxy64(10, 10, 54, 54)),            # prediction nested in the target
    (_xyxy64(10, 10, 26, 26), _xyxy64(34, 36, 50, 52)),            # disjoint, apart
    (_xyxy64(10, 10, 26, 26), _xyxy64(26, 10, 42, 30)),            # disjoint, touching along an edge
    (_xyxy64(10, 10, 26, 26), _xyxy64(26, 26, 42, 42)),            # disjoint, touching at a corner
    ([32, 30, 16, 20], [32, 36, 24, 12]),                          # equal cx
    ([30, 36, 16, 20], [34, 36, 24, 12]),                          # equal cy
    ([30, 30, 16, 20], [34, 36, 16, 12]),                          # equal w
    ([30, 30, 16, 12], [34, 36, 20, 12]),                          # equal h
]


def box_inputs(n, L, fam):
    """-> pred_boxes [P,4], srow [n] int64 (distinct rows, unordered), tbox [n,4], w [n], lidx [n] int32 (not monotone; for L > 1 layer
    L // 2 receives no pair).  dyadic: every cxcywh component a multiple of 1/64 in [1/8, 7/8], so every xyxy coordinate, and with
    it every comparison, is exact in fp32 and in fp64; DYADIC_SPECIAL comes first."""
    g = torch.Generator().manual_seed(613 * n + L + 17 * BOX_FAMILIES.index(fam))
    P = n + 5
    srow = torch.randperm(P, generator=g)[:n]
    if fam == "plain":
        s, tbox = rand_boxes(n, g), rand_boxes(n, g)
    else:
        s = torch.randint(8, 57, (n, 4), generator=g).float()
        tbox = torch.randint(8, 57, (n, 4), generator=g).float()
        k = min(n, len(DYADIC_SPECIAL))
        s[:k] = torch.tensor([p for p, _ in DYADIC_SPECIAL[:k]], dtype=torch.float32)
        tbox[:k] = torch.tensor([t for _, t in DYADIC_SPECIAL[:k]], dtype=torch.float32)
        s, tbox = s / 64, tbox / 64
    pred = rand_boxes(P, g)
    pred[srow] = s
    w = torch.rand(n, generator=g) * 0.9 + 0.1
    lidx = torch.randint(0, L, (n,), generator=g)
    if L > 1:
        lidx[lidx == L // 2] = 0
    return pred, srow, tbox, w, lidx.int()


def bwd_inputs(n):
    """-> srow [n] int64 (for n >= 3 one row occurs three times), lidx [n] int32, g1, g2 [n,4], c1, c2 [L], number of rows P."""
    g = torch.Generator().manual_seed(4001 + n)
    L, P = 3, n + 2
    srow = torch.randperm(P, generator=g)[:n]
    if n >= 3:
        srow[n // 2] = srow[0]
        srow[n - 1] = srow[0]
    lidx = torch.randint(0, L, (n,), generator=g).int()
    g1, g2 = torch.randn(n, 4, generator=g), torch.randn(n, 4, generator=g)
    return srow, lidx, g1, g2, torch.tensor([1.0, 2.0, 3.0]), torch.tensor([0.5, 0.25, 2.0]), P


# ------------------------------------------------------------------------------------------------------------------------------
# matcher cost: (L, B, Q, Kc, sizes).  One thread per (query, target) pair of the same image, 256 per block; the image of an
# element is searched through toff
# ------------------------------------------------------------------------------------------------------------------------------
COST_CASES = [
    (1, 1, 1, 1, [1]),
    (2, 5, 17, 21, [0, 3, 0, 0, 15]),        # 306 elements: across a block edge; leading, middle and trailing empty images
    (3, 2, 300, 91, [7, 0]),
    (1, 3, 64, 80, [4, 4, 4]),               # 768 elements: exactly three blocks
]
COST_FAMILIES = {"plain": (0.0, 6.0), "saturated": (40.0, 100.0), "band": (6.0, 40.0)}      # range of |logit|
COST_WEIGHTS = (2.0, 5.0, 2.0)               # w_class, w_bbox, w_giou


def cost_inputs(case, fam):
    """-> logits [L,B,Q,Kc], boxes [L,B,Q,4], tgt_ids [total] int32, tgt_boxes [total,4]."""
    L, B, Q, Kc, sizes = case
    g = torch.Generator().manual_seed(389 * COST_CASES.index(case) + list(COST_FAMILIES).index(fam))
    lo, hi = COST_FAMILIES[fam]
    mag = lo + (hi - lo) * torch.rand(L, B, Q, Kc, generator=g)
    logits = mag * torch.where(torch.rand(L, B, Q, Kc, generator=g) < 0.5, -1.0, 1.0)
    boxes = rand_boxes(L * B * Q, g).view(L, B, Q, 4)
    total = sum(sizes)
    return logits, boxes, torch.randint(0, Kc, (total,), generator=g).int(), rand_boxes(total, g)


def cost_degenerate_inputs():
    """One prediction box of negative width and one target box of negative height among ordinary ones: (case, tensors)."""
    case = (1, 1, 4, 3, [2])
    g = torch.Generator().manual_seed(91)
    logits = 2 * torch.randn(1, 1, 4, 3, generator=g)
    boxes = rand_boxes(4, g).view(1, 1, 4, 4)
    boxes[0, 0, 2] = torch.tensor([0.5, 0.5, -0.2, 0.3])
    tgt_boxes = rand_boxes(2, g)
    tgt_boxes[1] = torch.tensor([0.4, 0.6, 0.3, -0.1])
    return case, (logits, boxes, torch.tensor([0, 2], dtype=torch.int32), tgt_boxes)


# ------------------------------------------------------------------------------------------------------------------------------
# sorted NMS: one workgroup of 256 threads per image, at most 4096 detections
# ------------------------------------------------------------------------------------------------------------------------------
NMS_N = (1, 255, 256, 257, 700, 4096)
NMS_IMAGES = 3
NMS_REFUSED = 4097
NMS_THR = 0.5


def nms_inputs(n):
    """-> boxes [3,n,4] xyxy, labels [3,n] int64, scores [3,n], every image ordered by (label ascending, score descending), and the
    per-image counts (n, 0, n // 2).  Clusters of near-duplicates, an exact duplicate, two pairs straddling IoU 0.5 (0.5015 and 0.4993)
    in a class of their own; from n = 700 half of the detections share class 0, so one class is longer than 256."""
    g = torch.Generator().manual_seed(50 + n)
    bs, ls, ss = [], [], []
    for _ in range(NMS_IMAGES):
        c = torch.rand(n, 2, generator=g) * 500 + 100
        wh = torch.rand(n, 2, generator=g) * 150 + 20
        labels = torch.randint(0, 5, (n,), generator=g)
        if n >= 700:
            labels[torch.rand(n, generator=g) < 0.5] = 0
        h = n // 2
        if n >= 8:
            c[h:2 * h] = c[:h] + torch.randn(h, 2, generator=g) * 5
            wh[h:2 * h] = wh[:h] * (1 + 0.05 * torch.randn(h, 2, generator=g))
            labels[h:2 * h] = labels[:h]
        boxes = torch.cat([c - wh / 2, c + wh / 2], 1)
        if n >= 8:
            boxes[n - 1] = boxes[0]; labels[n - 1] = labels[0]
            boxes[1] = torch.tensor([0., 0., 100., 100.]); boxes[2] = torch.tensor([33.2, 0., 133.2, 100.])
            boxes[3] = torch.tensor([300., 0., 400., 100.]); boxes[4] = torch.tensor([333.4, 0., 433.4, 100.])
            labels[1:5] = 9
        scores = torch.rand(n, generator=g)
        order = torch.argsort(scores, descending=True, stable=True)
        order = order[torch.argsort(labels[order], stable=True)]
        bs.append(boxes[order]); ls.append(labels[order]); ss.append(scores[order])
    return torch.stack(bs), torch.stack(ls), torch.stack(ss), (n, 0, n // 2)


# ------------------------------------------------------------------------------------------------------------------------------
# jitter pick: one wave per box, candidates 64 at a time, the fill loop strides the `ratio` rows by 64
# ------------------------------------------------------------------------------------------------------------------------------
JITTER_CASES = [(M, ncand, ratio) for M in (1, 9) for ncand in (0, 1, 63, 64, 65, 1000) for ratio in (1, 2, 5, 70)]


def jitter_inputs(M, ncand, ratio):
    """-> box [M,4] cxcywh, scale [M,ncand,4] uniform in [1 - j, 1 + j], j = 0.1.  With M = 9: box 0 has size 1e-6 (every candidate
    fails the IoU test), box 1 is jittered by j = 0.001 only (every candidate passes)."""
    g = torch.Generator().manual_seed(97 * ncand + 5 * ratio + M)
    box = torch.rand(M, 4, generator=g) * 0.5 + 0.2
    j = torch.full((M, 1, 1), 0.1)
    if M > 1:
        box[0, 2:] = 1e-6
        j[1] = 0.001
    scale = 1 + j * (2 * torch.rand(M, ncand, 4, generator=g) - 1)
    return box, scale


def hung_blocks(case):
    """(layer, image, first target, n) of every non-empty problem of a case."""
    L, Q, sizes = case
    out, off = [], 0
    for b, n in enumerate(sizes):
        if n:
            out += [(l, b, off, n) for l in range(L)]
        off += n
    return sorted(out)


def staged(Q, n):
    return n * Q <= HUNG_LDS_FLOATS

