"""Plain restatements of the seven set-criterion kernels of csrc/loss.hip (matcher cost, assignment, focal loss, box losses and their
scatter, sorted NMS, jitter pick) for tests/test_criterion_ref_cpu.py and tests/test_criterion_kernels_gpu.py.  CPU only, fp64 torch /
numpy unless a function says otherwise; nothing of spe_amd is imported, so a defect of the package cannot hide in its own yardstick.

Layouts are those of include/spe_hip.h: cost[l] is the concatenation over images b of row-major [Q, M_b] blocks (block b starts at
Q * toff[b]); the assignment comes back as (srow, gidx, lidx) triples ordered (layer, image, query)."""
import math

import numpy as np
import torch

U32 = 2.0 ** -24                      # unit round-off of fp32
CLAMP_LOGIT = math.log((1 - 1e-5) / 1e-5)      # 11.5129: |logit| at which the focal p_t clamp (1e-5, 1 - 1e-5) takes over


def rel(a, b):
    """The norm ratio of tests/test_kernels_gpu.py."""
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def ulp32(x):
    """Spacing of fp32 at |x| (fp64 tensor in, fp64 tensor out; the smallest normal's spacing below it)."""
    ax = x.double().abs().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(ax)) - 23)


def toff_of(sizes):
    t = [0]
    for s in sizes:
        t.append(t[-1] + int(s))
    return t


# ------------------------------------------------------------------------------------------------------------------------------
# matcher cost
# ------------------------------------------------------------------------------------------------------------------------------
def to_xyxy(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


def giou_pairwise(a, b):
    """a [Q,4], b [M,4] xyxy -> [Q,M]."""
    area1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt, rb = torch.max(a[:, None, :2], b[None, :, :2]), torch.min(a[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = area1[:, None] + area2[None, :] - inter
    iou = inter / union
    lt, rb = torch.min(a[:, None, :2], b[None, :, :2]), torch.max(a[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    ea = wh[..., 0] * wh[..., 1]
    return iou - (ea - union) / ea


def matcher_cost_ref(logits, boxes, tgt_ids, tgt_boxes, sizes, w_class, w_bbox, w_giou, dtype=torch.float64):
    """C = w_bbox L1(cxcywh) + w_class (pos_focal - neg_focal)[label] - w_giou GIoU with alpha 0.25, gamma 2, eps 1e-8, every operation
    carried out in `dtype` (float64: the reference value; float32: the same composition in the arithmetic the formula was written for).
    logits [L,B,Q,Kc], boxes [L,B,Q,4] -> (cost [L, Q * total], x [L, Q * total]: the logit each cost element read, fp64)."""
    L, B, Q, Kc = logits.shape
    toff = toff_of(sizes)
    lg, bx, tb = logits.to(dtype), boxes.to(dtype), tgt_boxes.to(dtype)
    cost = torch.zeros(L, Q * toff[-1], dtype=dtype)
    xs = torch.zeros(L, Q * toff[-1], dtype=torch.float64)
    for l in range(L):
        for b in range(B):
            if sizes[b] == 0:
                continue
            ids = tgt_ids[toff[b]:toff[b + 1]].long()
            t = tb[toff[b]:toff[b + 1]]
            p = lg[l, b].sigmoid()
            neg = 0.75 * p ** 2 * (-(1 - p + 1e-8).log())
            pos = 0.25 * (1 - p) ** 2 * (-(p + 1e-8).log())
            c_class = pos[:, ids] - neg[:, ids]
            c_bbox = (bx[l, b][:, None, :] - t[None, :, :]).abs().sum(-1)
            c_giou = -giou_pairwise(to_xyxy(bx[l, b]), to_xyxy(t))
            blk = w_bbox * c_bbox + w_class * c_class + w_giou * c_giou
            cost[l, Q * toff[b]:Q * toff[b + 1]] = blk.reshape(-1)
            xs[l, Q * toff[b]:Q * toff[b + 1]] = logits[l, b].double()[:, ids].reshape(-1)
    return cost, xs


def class_cost_tol(x):
    """What four fp32 roundings of p = sigmoid(x) (expf, the add, the divide, the subtract 1 - p) can move the class term by:
    |d class / dp| 4 u, on top of the project's 2e-5 for well-conditioned logits.  1 - p cancels as p -> 1, so the term is
    ill-conditioned in the formula's own fp32 arithmetic between x ~ 8 and x ~ 25."""
    p = torch.as_tensor(x, dtype=torch.float64).sigmoid()
    return 2e-5 + 4 * U32 * (0.75 * p ** 2 / (1 - p + 1e-8) + 0.25 * (1 - p) ** 2 / (p + 1e-8))


def matcher_cost_tol(x, w_class, w_bbox, w_giou):
    """Per-element bound of the whole cost: four L1 terms at 1e-6, GIoU at 2e-6, the class term by its conditioning."""
    return w_bbox * 1e-6 * 4 + w_giou * 2e-6 + w_class * class_cost_tol(x)


# ------------------------------------------------------------------------------------------------------------------------------
# focal loss
# ------------------------------------------------------------------------------------------------------------------------------
def argmax_lowest(logits):
    """Top-1 class per row, the lowest index among equal maxima.  logits [..., Kc] -> int64 [...]."""
    x = logits.double()
    is_max = x == x.max(-1, keepdim=True).values
    idx = torch.arange(x.shape[-1]).expand_as(x)
    return torch.where(is_max, idx, torch.full_like(idx, x.shape[-1])).min(-1).values


def focal_ref(logits, tclass, roww, alpha, gamma, dtype=torch.float64):
    """Weighted sigmoid focal loss: loss[l] = sum_rows sum_c w alpha_t BCE(x, t) (1 - clamp(p_t, 1e-5, 1 - 1e-5))^gamma; tclass in
    [0, Kc], Kc = no object (all-zero one-hot); alpha < 0: no alpha_t.  logits [L,R,Kc] -> (loss [L], d sum(loss) / d logits by
    autograd, clamp included, argmax [L,R] lowest index on ties), loss and gradient in `dtype`."""
    L, R, Kc = logits.shape
    x = logits.to(dtype).clone().requires_grad_()
    t = torch.nn.functional.one_hot(tclass.long(), Kc + 1)[..., :Kc].to(dtype)
    p = x.sigmoid()
    ce = x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    pt = (p * t + (1 - p) * (1 - t)).clamp(1e-5, 1 - 1e-5)
    at = alpha * t + (1 - alpha) * (1 - t) if alpha >= 0 else torch.ones_like(t)
    w = 1.0 if roww is None else roww.to(dtype)[..., None]
    loss = (w * at * ce * (1 - pt) ** gamma).sum((1, 2))
    (grad,) = torch.autograd.grad(loss.sum(), x)
    return loss.detach(), grad, argmax_lowest(logits)


def focal_grad_tol(ref_grad):
    """Per-element bound of the gradient on logits far from the clamp threshold: 1e-4 max|ref| + 4 ulp32(|ref|)."""
    return 1e-4 * ref_grad.abs().max() + 4 * ulp32(ref_grad)


# ------------------------------------------------------------------------------------------------------------------------------
# box losses
# ------------------------------------------------------------------------------------------------------------------------------
def giou_diag(a, b):
    """a, b [n,4] xyxy -> [n] through torch.maximum / minimum / clamp (their autograd splits ties 1/2 - 1/2)."""
    area1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = (torch.minimum(a[:, 2], b[:, 2]) - torch.maximum(a[:, 0], b[:, 0])).clamp(min=0)
    ih = (torch.minimum(a[:, 3], b[:, 3]) - torch.maximum(a[:, 1], b[:, 1])).clamp(min=0)
    inter = iw * ih
    union = area1 + area2 - inter
    ew = (torch.maximum(a[:, 2], b[:, 2]) - torch.minimum(a[:, 0], b[:, 0])).clamp(min=0)
    eh = (torch.maximum(a[:, 3], b[:, 3]) - torch.minimum(a[:, 1], b[:, 1])).clamp(min=0)
    ea = ew * eh
    return inter / union - (ea - union) / ea


def box_loss_ref(pred_boxes, srow, tbox, w, lidx, L, dtype=torch.float64):
    """Pair i = (prediction row srow[i], target tbox[i], weight w[i] or 1, layer lidx[i]) -> (sums [L,2] = per layer
    (sum w L1, sum w (1 - GIoU)), g_l1 [n,4], g_giou [n,4]: the gradients of the two totals w.r.t. the gathered cxcywh boxes)."""
    s = pred_boxes.to(dtype)[srow.long()].clone().requires_grad_()
    t = tbox.to(dtype)
    wt = torch.ones(s.shape[0], dtype=dtype) if w is None else w.to(dtype)
    l1 = (s - t).abs().sum(1) * wt
    gi = (1 - giou_diag(to_xyxy(s), to_xyxy(t))) * wt
    (g1,) = torch.autograd.grad(l1.sum(), s, retain_graph=True)
    (g2,) = torch.autograd.grad(gi.sum(), s)
    sums = torch.zeros(L, 2, dtype=dtype)
    sums.index_add_(0, lidx.long(), torch.stack([l1, gi], 1).detach())
    return sums, g1, g2


def box_loss_bwd_ref(srow, lidx, g1, g2, c1, c2, shape):
    """dpred[srow[i]] += c1[lidx[i]] g1[i] + c2[lidx[i]] g2[i] (a row may occur more than once)."""
    li = lidx.long()
    d = torch.zeros(shape, dtype=torch.float64)
    d.index_add_(0, srow.long(), c1.double()[li][:, None] * g1.double() + c2.double()[li][:, None] * g2.double())
    return d


# ------------------------------------------------------------------------------------------------------------------------------
# assignment
# ------------------------------------------------------------------------------------------------------------------------------
def lsap_lowest_index(blk):
    """hungarian_kernel's algorithm restated: blk [Q, M] (queries x targets, M <= Q) -> (queries ascending, their targets).
    Shortest augmenting paths with dual potentials in fp64; the targets are inserted in order; the reduced cost of query j from the
    tree's current target i0 is (a - u[i0]) - v[j]; minv is replaced on strict < only; among equal minima the free query with the
    lowest index is taken (numpy's argmin returns the first).  -0.0 == +0.0 here; the kernel's integer keys order them."""
    a = np.ascontiguousarray(np.asarray(blk, dtype=np.float64).T)        # a[i, j]: target i, query j
    n, m = a.shape
    assert n <= m
    v, ucol = np.zeros(m), np.zeros(m)              # ucol[j]: potential of the target matched to query j
    p, way = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)     # 1-based; 0: free / the virtual query
    for i in range(1, n + 1):
        minv = np.full(m, np.inf)
        used = np.zeros(m, dtype=bool)
        u0, j0, i0, ui0 = 0.0, 0, i, 0.0
        while True:
            if j0:
                used[j0 - 1] = True
            free = ~used
            cur = (a[i0 - 1] - ui0) - v
            upd = free & (cur < minv)
            minv[upd] = cur[upd]
            way[upd] = j0
            masked = np.where(free, minv, np.inf)
            j1 = int(np.argmin(masked))
            delta = masked[j1]
            assert np.isfinite(delta)
            u0 += delta
            ucol[used] += delta
            v[used] -= delta
            minv[free] -= delta
            j0 = j1 + 1
            i0, ui0 = int(p[j1]), ucol[j1]
            if i0 == 0:
                break
        while j0:
            j1 = int(way[j0 - 1])
            p[j0 - 1], ucol[j0 - 1] = (i, u0) if j1 == 0 else (p[j1 - 1], ucol[j1 - 1])
            j0 = j1
    q = np.nonzero(p)[0]
    return q, p[q] - 1


def assignment_triples(cost, L, Q, sizes, solve):
    """Every (layer, image) block of `cost` [L, Q * total] through solve(blk [Q, M]) -> (srow, gidx, lidx) int64 tensors in
    (layer, image, query) order; empty images contribute nothing."""
    toff, B = toff_of(sizes), len(sizes)
    c = cost.cpu()
    es, eg, el = [], [], []
    for l in range(L):
        for b in range(B):
            if sizes[b] == 0:
                continue
            blk = c[l, Q * toff[b]:Q * toff[b + 1]].view(Q, sizes[b]).numpy()
            i, j = solve(blk)
            es.append(torch.as_tensor(np.asarray(i), dtype=torch.int64) + (l * B + b) * Q)
            eg.append(torch.as_tensor(np.asarray(j), dtype=torch.int64) + toff[b])
            el.append(torch.full((len(i),), l, dtype=torch.int64))
    z = torch.zeros(0, dtype=torch.int64)
    return (torch.cat(es) if es else z), (torch.cat(eg) if eg else z), (torch.cat(el) if el else z)


def check_assignment(srow, gidx, lidx, case):
    """Distinct queries per problem, every target exactly once per layer, (layer, image, query) order, lidx = layer."""
    L, Q, sizes = case
    B, total, toff = len(sizes), sum(sizes), toff_of(sizes)
    assert srow.numel() == gidx.numel() == lidx.numel() == L * total
    pos = 0
    for l in range(L):
        for b in range(B):
            n = sizes[b]
            s, g_, li = srow[pos:pos + n], gidx[pos:pos + n], lidx[pos:pos + n]
            pos += n
            if n == 0:
                continue
            q = s - (l * B + b) * Q
            assert bool(((q >= 0) & (q < Q)).all()) and bool((q[1:] > q[:-1]).all()), (l, b, "queries not ascending / distinct")
            assert torch.equal(torch.sort(g_).values, torch.arange(toff[b], toff[b + 1])), (l, b, "targets not a permutation")
            assert bool((li == l).all())


def assignment_totals(cost, srow, gidx, case):
    """fp64 total of every layer's assignment."""
    L, Q, sizes = case
    B, total, toff = len(sizes), sum(sizes), torch.tensor(toff_of(sizes))
    l = srow // (B * Q)
    b = (srow // Q) % B
    q = srow % Q
    n = (toff[1:] - toff[:-1])[b]
    e = Q * toff[b] + q * n + (gidx - toff[b])
    vals = cost.double()[l, e]
    return torch.zeros(L, dtype=torch.float64).index_add_(0, l, vals)


# ------------------------------------------------------------------------------------------------------------------------------
# NMS, jitter
# ------------------------------------------------------------------------------------------------------------------------------
def greedy_nms_ref(boxes, labels, thr, count=None):
    """One image's detections ordered by (label ascending, score descending): visit in order, a surviving box suppresses every later
    box of its label whose IoU exceeds thr.  fp32, torchvision's arithmetic: areas (x1 - x0) (y1 - y0), extents clamped at 0,
    inter / (a_i + a_j - inter) > thr.  boxes [n,4] xyxy, labels [n]; only the first `count` are looked at -> keep bool [n]."""
    bx = boxes.float().numpy()
    lb = labels.numpy()
    n = bx.shape[0] if count is None else int(count)
    assert (np.diff(lb[:n]) >= 0).all(), "labels must ascend"
    end = np.searchsorted(lb[:n], lb[:n], side="right")              # one past the last detection of the label
    area = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
    dead = np.zeros(bx.shape[0], dtype=bool)
    t = np.float32(thr)
    for i in range(n):
        if dead[i] or i + 1 >= end[i]:
            continue
        s = slice(i + 1, end[i])
        w = np.maximum(np.minimum(bx[i, 2], bx[s, 2]) - np.maximum(bx[i, 0], bx[s, 0]), np.float32(0))
        h = np.maximum(np.minimum(bx[i, 3], bx[s, 3]) - np.maximum(bx[i, 1], bx[s, 1]), np.float32(0))
        inter = w * h
        with np.errstate(invalid="ignore", divide="ignore"):
            dead[s] |= inter / (area[i] + area[s] - inter) > t
    keep = ~dead
    keep[n:] = False
    return torch.from_numpy(keep)


def jitter_pick_ref(box, scale, ratio):
    """box [M,4] cxcywh, scale [M,ncand,4] -> [M, ratio, 4]: candidate c of box m is scale[m,c] * box[m]; the first ratio - 1
    candidates whose IoU with the box exceeds 0.7, in candidate order, then the box itself in every remaining row (so the original is
    last).  The fp32 elementwise composition of torch: one rounding per operation."""
    box, scale = box.float(), scale.float()
    M, ncand = scale.shape[0], scale.shape[1]
    out = box[:, None, :].repeat(1, ratio, 1)
    if ncand == 0 or ratio == 1:
        return out
    cand = scale * box[:, None, :]
    a, b = to_xyxy(cand), to_xyxy(box)[:, None, :]
    wh = (torch.min(a[..., 2:], b[..., 2:]) - torch.max(a[..., :2], b[..., :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    area = lambda z: (z[..., 2] - z[..., 0]) * (z[..., 3] - z[..., 1])
    keep = inter / (area(a) + area(b) - inter) > 0.7
    for m in range(M):
        idx = keep[m].nonzero().reshape(-1)[:ratio - 1]
        out[m, :idx.numel()] = cand[m, idx]
    return out
