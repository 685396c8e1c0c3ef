"""The error bounds of tests/rownorm_ref.py must be satisfiable: an fp32 numpy emulation of a CORRECT row kernel - lane-strided
partial sums, a butterfly over the lanes, two-pass variance, the backward formula of ln_bwd_kernel with per-wave column accumulators
combined in a second level - stays under 0.5 x every bound, with the reduction order randomised (column permutation, 32 or 64 lanes,
row permutation and wave count of the column sums), for the six conditioning families at C in {4, 64, 128, 192, 256, 384, 512, 1024}.
A one-pass variance, the mistake the bounds exist to catch, is far outside them on the offset rows (second test).

Worst emulation / bound ratios seen (R = 64, eps 1e-6 and 1e-5, all families and widths): y 0.301 and mean 0.301 (the constant
row at C = 4), rstd 0.091, dx 0.030, dgamma 0.158, dbeta 0.043.  Every test prints its own (prefix ROWNORM, `pytest -s`)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rownorm_ref as rr  # noqa: E402

WIDTHS = (4, 64, 128, 192, 256, 384, 512, 1024)
R = 64

f32 = np.float32


def _lane_sum(v, lanes, perm):
    """Sum over the last axis the way a wave does: column i goes to lane perm(i) % lanes, a lane adds its columns in order, then a
    butterfly (xor 16, 8, ...) over the lanes.  Everything in fp32."""
    v = v[:, perm]
    Rr, C = v.shape
    pad = (-C) % lanes
    if pad:
        v = np.concatenate([v, np.zeros((Rr, pad), f32)], 1)
    part = np.zeros((Rr, lanes), f32)
    for i in range(v.shape[1] // lanes):
        part = (part + v[:, i * lanes:(i + 1) * lanes]).astype(f32)
    o = lanes // 2
    while o >= 1:
        part = (part + part[:, np.arange(lanes) ^ o]).astype(f32)
        o //= 2
    return part[:, 0]


def _col_sum(v, rng):
    """Column sums in fp32: rows dealt to nw accumulators in a random order, the accumulators added in order."""
    nw = int(rng.choice([1, 4, 16]))
    order = rng.permutation(v.shape[0])
    acc = np.zeros((nw, v.shape[1]), f32)
    for i, r in enumerate(order):
        acc[i % nw] = (acc[i % nw] + v[r]).astype(f32)
    t = np.zeros(v.shape[1], f32)
    for w in range(nw):
        t = (t + acc[w]).astype(f32)
    return t


def emulate(x, gamma, beta, dy, eps, rng, one_pass=False):
    x, gamma, beta, dy = (np.asarray(t, f32) for t in (x, gamma, beta, dy))
    C = x.shape[1]
    lanes = int(rng.choice([32, 64]))
    perm = rng.permutation(C)
    mu = (_lane_sum(x, lanes, perm) / f32(C)).astype(f32)
    if one_pass:
        var = (_lane_sum((x * x).astype(f32), lanes, perm) / f32(C) - mu * mu).astype(f32)
    else:
        d = (x - mu[:, None]).astype(f32)
        var = (_lane_sum((d * d).astype(f32), lanes, perm) / f32(C)).astype(f32)
    with np.errstate(invalid="ignore"):             # one_pass: the variance can come out negative
        rs = (f32(1) / np.sqrt((var + f32(eps)).astype(f32))).astype(f32)
    xh = ((x - mu[:, None]).astype(f32) * rs[:, None]).astype(f32)
    y = ((xh * gamma).astype(f32) + beta).astype(f32)
    dg = (dy * gamma).astype(f32)
    s1 = (_lane_sum(dg, lanes, perm) / f32(C)).astype(f32)
    s2 = (_lane_sum((dg * xh).astype(f32), lanes, perm) / f32(C)).astype(f32)
    dx = (rs[:, None] * ((dg - s1[:, None]).astype(f32) - (xh * s2[:, None]).astype(f32)).astype(f32)).astype(f32)
    return {"y": y, "mean": mu, "rstd": rs, "dx": dx, "dgamma": _col_sum((dy * xh).astype(f32), rng), "dbeta": _col_sum(dy, rng)}


def ratios(em, x, gamma, beta, dy, eps):
    y, mean, rstd = rr.ln_fwd(x, gamma, beta, eps)
    dx, dgam, dbet, _ = rr.ln_bwd(dy, x, gamma, eps)
    fb, bb = rr.ln_fwd_bounds(x, gamma, beta, eps), rr.ln_bwd_bounds(dy, x, gamma, eps)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    return {"y": rr.worst_ratio(t(em["y"]) - y, fb["y"]),
            "mean": rr.worst_ratio(t(em["mean"]) - mean, fb["mean"]),
            "rstd": rr.worst_ratio((t(em["rstd"]) - rstd) / rstd, fb["rstd_rel"]),
            "dx": rr.worst_ratio(t(em["dx"]) - dx, bb["dx"]),
            "dgamma": rr.worst_ratio(t(em["dgamma"]) - dgam, bb["dgamma"]),
            "dbeta": rr.worst_ratio(t(em["dbeta"]) - dbet, bb["dbeta"])}


def _inputs(fam, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = rr.family(fam, R, C, g)
    return x, torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(R, C, generator=g)


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("fam", rr.FAMILIES)
def test_correct_fp32_kernel_is_inside_the_bounds(fam, C):
    worst = {}
    for trial, eps in enumerate((1e-6, 1e-5, 1e-6)):
        x, gamma, beta, dy = _inputs(fam, C, 1000 * trial + C)
        rng = np.random.default_rng(C * 7 + trial)
        em = emulate(x.numpy(), gamma.numpy(), beta.numpy(), dy.numpy(), eps, rng)
        for k, v in ratios(em, x, gamma, beta, dy, eps).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("ROWNORM cpu-emulation", fam, C, " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v < 0.5, (fam, C, k, v)


@pytest.mark.parametrize("fam", ["offset1e3", "offset1e4"])
def test_one_pass_variance_is_outside_the_bounds(fam):
    x, gamma, beta, dy = _inputs(fam, 256, 5)
    em = emulate(x.numpy(), gamma.numpy(), beta.numpy(), dy.numpy(), 1e-6, np.random.default_rng(1), one_pass=True)
    r = ratios(em, x, gamma, beta, dy, 1e-6)
    assert not r["rstd"] <= 1.0 and not r["y"] <= 1.0, r          # (NaN - a negative variance - counts as outside)


def test_restatements_against_autograd():
    """The closed-form backward restatements against torch.autograd in fp64 (layer_norm with skip, second gradient and keep-scale;
    masked softmax with keep-scale)."""
    g = torch.Generator().manual_seed(9)
    Rr, C, p = 13, 20, 0.25
    x, z = (torch.randn(Rr, C, generator=g, dtype=torch.float64).requires_grad_() for _ in range(2))
    gamma, beta = (torch.randn(C, generator=g, dtype=torch.float64).requires_grad_() for _ in range(2))
    keep = (torch.rand(Rr, C, generator=g) >= p).double() / (1 - p)
    dy, dy2, add = (torch.randn(Rr, C, generator=g, dtype=torch.float64) for _ in range(3))
    s = x + z * keep
    y = torch.nn.functional.layer_norm(s, (C,), gamma, beta, 1e-5)
    ax, az, ag, ab = torch.autograd.grad([y, s], [x, z, gamma, beta], [dy + dy2, add])
    yr, _, _ = rr.ln_fwd(s.detach(), gamma, beta, 1e-5)
    dx, dgam, dbet, dz = rr.ln_bwd(dy, s.detach(), gamma.detach(), 1e-5, add=add, dy2=dy2, keep=keep)
    for a, b in ((yr, y), (dx, ax), (dz, az), (dgam, ag), (dbet, ab)):
        assert rr.rel(a, b.detach()) < 1e-13
    B, H, Nq, Nk = 3, 2, 5, 70
    S = torch.randn(B, H, Nq, Nk, generator=g, dtype=torch.float64).requires_grad_()
    mask = torch.zeros(B, Nk, dtype=torch.bool)
    mask[1, 40:] = True
    mask[2, 5::64] = True
    keep = (torch.rand(B, H, Nq, Nk, generator=g) >= p).double() / (1 - p)
    go = torch.randn(B, H, Nq, Nk, generator=g, dtype=torch.float64)
    P = S.masked_fill(mask[:, None, None, :], float("-inf")).softmax(-1)
    (aS,) = torch.autograd.grad(P * keep, S, go)
    Pr = rr.softmax_fwd(S.detach(), mask)
    assert rr.rel(Pr, P.detach()) < 1e-14 and bool((Pr[1, ..., 40:] == 0).all())
    assert rr.rel(rr.softmax_bwd(go, Pr, keep), aS) < 1e-13
