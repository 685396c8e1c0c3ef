"""fp64 restatements of the row kernels of csrc/rowops.hip - LayerNorm forward / backward (optional skip gradient, second output
gradient, dropout keep-scale of the `norm(x + dropout(z))` site), the LayerScale ride-along of spe_layernorm_bwd_ls, the masked
softmax forward / backward - and per-element error bounds for a correct fp32 LayerNorm on badly conditioned rows.  Plain torch on
whatever device the arguments live on; no project code is imported here.

The bounds.  u = 2^-24 (fp32 unit round-off), kappa = log2(C) + 8, A = max |x_row|, delta = kappa u A rstd_ref.  A two-pass fp32
kernel computes the mean with an error of at most ~log2(C) u A (any summation tree of depth >= log2 C over terms bounded by A; the
constant 8 covers lane-strided partial sums in front of the tree, the division and the subtraction x - mean), so every x - mean
is off by at most kappa u A and xhat = (x - mean) rstd by delta (1 + |xhat|) once the relative error of rstd - the same delta,
amplified by the largest |xhat| of the row, plus the rsqrt and the eps addition - is counted:

  |d mean|        <= kappa u A
  |d rstd| / rstd <= delta max(1, max |xhat|) + 4 u
  |d y|           <= |gamma| delta (1 + |xhat|) + 8 u (|gamma xhat| + |beta|)
  |d dx|          <= rstd max_row |dy gamma| (4 delta (1 + |xhat|)^2 + 16 u (1 + xhat^2))        (+ 2 u |dx| when a skip gradient is added)
  |d dgamma_c|    <= sum_r |dy| delta_r (1 + |xhat|) + 4 (log2 R + 8) u sum_r |dy xhat|
  |d dbeta_c|     <= 4 (log2 R + 8) u sum_r |dy|

and for the LayerScale ride-along, by the same pattern (B_dx = the dx bound above):

  |d ls_dg_c|     <= sum_r B_dx |ls_y| + 4 (log2 R + 8) u sum_r |dx ls_y|
  |d ls_db_c|     <= |ls_gamma| sum_r B_dx + 4 (log2 R + 8) u |ls_gamma| sum_r |dx|
  |d dy16|        <= 2^-8 |ls_gamma dx| + |ls_gamma| B_dx       (bf16 keeps 8 significant bits: round-to-nearest is off by up to
                                                                 2^-8 / (1 + 2^-8) relative at the bottom of a binade, so a correct
                                                                 kernel comes close to this bound: the first term has no slack)

A one-pass variance E[x^2] - mean^2 loses ~u A^2 rstd^2 = delta A rstd / kappa relative in rstd: on a row with a large common offset
(A rstd >> kappa) it is far outside these bounds.  tests/test_rownorm_ref_cpu.py checks that a correct fp32 kernel is inside them."""
import math

import torch

U = 2.0 ** -24


def kappa(C):
    return math.log2(C) + 8.0


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def row_rel(a, b):
    """max over rows ||a_r - b_r|| / rms over rows ||b_r||: one wrong row among thousands shows here and not in `rel`."""
    a, b = a.double().reshape(b.shape[0], -1), b.double().reshape(b.shape[0], -1)
    den = b.norm(dim=1).pow(2).mean().sqrt() + 1e-30
    return ((a - b).norm(dim=1).max() / den).item()


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------
def ln_fwd(x, gamma, beta, eps):
    """-> (y [R,C], mean [R], rstd [R]) in fp64."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    mean = x.mean(1)
    xc = x - mean[:, None]
    rstd = (xc.pow(2).mean(1) + eps).rsqrt()
    return xc * rstd[:, None] * gamma + beta, mean, rstd


def ln_bwd(dy, x, gamma, eps, add=None, dy2=None, keep=None):
    """-> (dx, dgamma, dbeta, dz): dy2 is a second gradient of the output, add the gradient of a skip path around the norm (summed
    into dx), keep [R,C] the dropout keep-scale of the branch z of norm(x + dropout(z)) (dz = dx keep; None without it)."""
    x, gamma = x.double(), gamma.double()
    dy = dy.double() if dy2 is None else dy.double() + dy2.double()
    _, mean, rstd = ln_fwd(x, gamma, torch.zeros_like(gamma), eps)
    xh = (x - mean[:, None]) * rstd[:, None]
    dg = dy * gamma
    dx = rstd[:, None] * (dg - dg.mean(1, keepdim=True) - xh * (dg * xh).mean(1, keepdim=True))
    if add is not None:
        dx = dx + add.double()
    dz = None if keep is None else dx * keep.double()
    return dx, (dy * xh).sum(0), dy.sum(0), dz


def ls_ride(dx, ls_y, ls_gamma):
    """LayerScale backward of the node out = res + ls_gamma ls_y whose output gradient is dx -> (dy16 (in fp64), ls_db, ls_dg)."""
    dx, ls_y, ls_gamma = dx.double(), ls_y.double(), ls_gamma.double()
    dy = ls_gamma * dx
    return dy, dy.sum(0), (dx * ls_y).sum(0)


def ln_fwd_bounds(x, gamma, beta, eps):
    """-> dict of per-element (y), per-row (mean, rstd_rel, delta) bounds and the fp64 xhat."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    C = x.shape[1]
    _, mean, rstd = ln_fwd(x, gamma, beta, eps)
    xh = (x - mean[:, None]) * rstd[:, None]
    A = x.abs().amax(1)
    delta = kappa(C) * U * A * rstd
    y = gamma.abs() * delta[:, None] * (1 + xh.abs()) + 8 * U * ((gamma * xh).abs() + beta.abs())
    rstd_rel = delta * xh.abs().amax(1).clamp(min=1.0) + 4 * U
    return {"y": y, "mean": kappa(C) * U * A, "rstd_rel": rstd_rel, "delta": delta, "xh": xh, "rstd": rstd}


def ln_bwd_bounds(dy, x, gamma, eps, add=None, dy2=None):
    """-> dict of bounds on dx [R,C], dgamma [C], dbeta [C]."""
    x, gamma = x.double(), gamma.double()
    dy = dy.double() if dy2 is None else dy.double() + dy2.double()
    R = x.shape[0]
    f = ln_fwd_bounds(x, gamma, torch.zeros_like(gamma), eps)
    xh, delta, rstd = f["xh"], f["delta"][:, None], f["rstd"][:, None]
    dgmax = (dy * gamma).abs().amax(1, keepdim=True)
    dx = rstd * dgmax * (4 * delta * (1 + xh.abs()).pow(2) + 16 * U * (1 + xh.pow(2)))
    if add is not None:
        dx = dx + 2 * U * ln_bwd(dy, x, gamma, eps, add=add)[0].abs()
    kr = 4 * (math.log2(R) + 8.0) * U
    dgamma = (dy.abs() * delta * (1 + xh.abs())).sum(0) + kr * (dy * xh).abs().sum(0)
    dbeta = kr * dy.abs().sum(0)
    return {"dx": dx, "dgamma": dgamma, "dbeta": dbeta}


def ls_ride_bounds(dx_ref, dx_bound, ls_y, ls_gamma):
    """-> dict of bounds on dy16 [R,C], ls_db [C], ls_dg [C] given the fp64 dx and the bound on the kernel's fp32 dx."""
    dx_ref, ls_y, ls_gamma = dx_ref.double(), ls_y.double(), ls_gamma.double()
    kr = 4 * (math.log2(dx_ref.shape[0]) + 8.0) * U
    return {"dy16": 2.0 ** -8 * (ls_gamma * dx_ref).abs() + ls_gamma.abs() * dx_bound,
            "ls_dg": (dx_bound * ls_y.abs()).sum(0) + kr * (dx_ref * ls_y).abs().sum(0),
            "ls_db": ls_gamma.abs() * (dx_bound.sum(0) + kr * dx_ref.abs().sum(0))}


def worst_ratio(err, bound):
    """max |err| / bound (0 where both are 0; inf where only the bound is)."""
    err, bound = err.double().abs(), bound.double()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return r.max().item()


FAMILIES = ("offset1e3", "offset1e4", "const", "tiny_var", "outlier", "plain")


def family(name, R, C, g):
    """The conditioning rows (fp32, CPU): a large common offset, zero variance, variance far below eps, one large outlier, and the
    plain input of the existing tests."""
    z = torch.randn(R, C, generator=g)
    if name == "offset1e3":
        return z + 1e3
    if name == "offset1e4":
        return 1e-2 * z + 1e4
    if name == "const":
        return torch.full((R, C), 3.7)
    if name == "tiny_var":
        return 1e-4 * z + 0.5
    if name == "outlier":
        col = torch.randint(0, C, (R,), generator=g)
        z[torch.arange(R), col] = 1e4
        return z
    if name == "plain":
        return z * 3 + 1
    raise KeyError(name)


# ---- masked softmax --------------------------------------------------------------------------------------------------------------
def softmax_fwd(S, mask=None):
    """S [B,H,Nq,Nk], mask [B,Nk] bool (True = padded key) -> P in fp64 (masked columns exactly 0)."""
    S = S.double()
    if mask is not None:
        S = S.masked_fill(mask[:, None, None, :], float("-inf"))
    return S.softmax(-1)


def softmax_bwd(dPd, P, keep=None):
    """dS = P (dP - sum_k dP P), dP = dPd keep."""
    dP = dPd.double() if keep is None else dPd.double() * keep.double()
    P = P.double()
    return P * (dP - (dP * P).sum(-1, keepdim=True))
