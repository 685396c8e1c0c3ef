"""fp64 restatements of the lower half of csrc/rowops.hip - the column sum, the LayerScale residual forward / backward and its 16-bit
backward, the ReLU / GELU backward, dropout - with the error bounds a correct fp32 kernel stays inside, and exact fp32 / bf16 torch
arithmetic where the kernel's result is determined bit for bit.  Plain torch on whatever device the arguments live on; no project code
is imported here.

The bounds.  u = 2^-24 (fp32 unit round-off).  A sum of fp32 terms taken in ANY fixed order is off by at most n_add u sum|terms| (first
order), n_add = the longest chain of inexact additions a term passes through.  An addition with a zero operand is exact, so a sum of T
terms has at most T - 1 inexact additions whatever the tree: n_add = min(chain of the branch, T - 1).  The chains, per branch (t = rows
one thread adds, m = members of the sum across workgroups, tree(m) = 0 for m = 1, m for m <= 16, 16 + ceil(m / 16) above: one group of
up to 16 rows, then the group sums - csrc/det_reduce.h; the flush of a DEFERRED sum adds ceil(m / 16) members per lane and then 16 lanes):

  colsum_wide        R                                              (one thread walks the R rows; `out` is the first operand)
  colsum_tall4       ceil(R / (16 m)) + 16 + tree(m) + 1            (rows of a thread, 16 row lanes, the tree, `out +=`)
  colsum             ceil(R / (4 m)) + 3 + tree(m) + 1              (rows of a thread, 4 row lanes, the tree, `out +=`)
  lsres_bwd_rows     ceil(R / (16 m)) + 16 + tree(m) + 1            (rows of a wave, 16 waves, the tree, `dgamma +=`)
  lsres_bwd          ceil(R / (4 m)) + 3 + tree(m) + 1
  lsres_bwd16        4 ceil(tiles / m) + 16 + tree(m) + 1           (4 rows of each 64-row tile per wave, 16 waves, the tree, `+=`)
  deferred           ... with ceil(m / 16) + 16 in the place of tree(m)

A product that enters a sum (dout s y) is rounded before it is added unless the compiler fuses the multiplication into the addition: one
more u per possible rounding of the term, which `extra` counts (the worst case: nothing fused).  The project's own figures (rel < 2e-6 for the column sum, rel < 1e-5 for the gradients of
gamma and the GELU backward: the formula of test_kernels_gpu.rel) are kept beside the bounds."""
import math

import torch

U = 2.0 ** -24
REL_COLSUM, REL_GRAD = 2e-6, 1e-5


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def worst_ratio(err, bound):
    """max |err| / bound (0 where the error is 0; inf where only the bound is)."""
    err, bound = err.double().abs(), bound.double()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return r.max().item() if r.numel() else 0.0


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- chains ----------------------------------------------------------------------------------------------------------------------
def tree(m):
    return 0 if m <= 1 else (m if m <= 16 else 16 + -(-m // 16))


def flush_chain(m):
    return -(-m // 16) + 16


def chain(kernel, R, members, tiles=None, deferred=False):
    """Longest addition chain of a branch (the table above); kernel: a name of kernels.ROWOPS_KERNELS."""
    m = max(members, 1)
    across = flush_chain(m) if (deferred and m > 1) else tree(m)
    if kernel == "colsum_wide":
        return R
    if kernel in ("colsum_tall4", "lsres_bwd_rows"):
        return -(-R // (16 * m)) + 16 + across + 1
    if kernel in ("colsum", "lsres_bwd"):
        return -(-R // (4 * m)) + 3 + across + 1
    if kernel.startswith("lsres_bwd16"):
        return 4 * -(-tiles // m) + 16 + across + 1
    raise KeyError(kernel)


def n_add(kernel, R, members, prefilled, tiles=None, deferred=False):
    """min(chain, T - 1) for T = R terms (+ 1: the value the destination held)."""
    return max(min(chain(kernel, R, members, tiles, deferred), R + int(bool(prefilled)) - 1), 0)


# ---- column sum ------------------------------------------------------------------------------------------------------------------
def colsum(x, out0=None):
    """-> (fp64 column sums (+ out0), sum of |terms| per column)."""
    x = x.double()
    s, a = x.sum(0), x.abs().sum(0)
    if out0 is not None:
        s, a = s + out0.double(), a + out0.double().abs()
    return s, a


def sum_bound(n, mag, extra=0):
    """(n + extra) u sum|terms|: n additions, `extra` roundings of every term in front of them."""
    return (n + extra) * U * mag


# ---- LayerScale residual ---------------------------------------------------------------------------------------------------------
def row_scale(sample_scale, rows_per_sample, R):
    """[R, 1] per-row DropPath scale (ones without one), in the dtype of sample_scale (fp32 if None)."""
    if sample_scale is None:
        return None
    return sample_scale[torch.arange(R, device=sample_scale.device) // rows_per_sample][:, None]


def lsres_fwd(x, y, gamma, sample_scale=None, rows_per_sample=1):
    """-> (fp64 x + s gamma y, bound 3 u (|x| + |s gamma y|): two multiplications and one addition)."""
    s = row_scale(sample_scale, rows_per_sample, x.shape[0])
    t = gamma.double() * y.double() if s is None else s.double() * gamma.double() * y.double()
    return x.double() + t, 3 * U * (x.double().abs() + t.abs())


def lsres_bwd(dout, y, gamma, sample_scale=None, rows_per_sample=1):
    """-> (dy in exact fp32: (dout s) gamma in that order, fp64 dgamma = sum dout s y, sum |dout s y|)."""
    s = row_scale(sample_scale, rows_per_sample, dout.shape[0])
    d = dout if s is None else dout * s                 # fp32, one rounding
    dy = d * gamma                                       # fp32, one rounding
    t = dout.double() * y.double() if s is None else dout.double() * s.double() * y.double()
    return dy, t.sum(0), t.abs().sum(0)


def lsres_bwd16(dout, y, gamma, keep=None, sample_scale=None, rows_per_sample=1, ldt=None):
    """The 16-bit backward.  keep [R, C]: the dropout keep-scales (0 or 1 / (1 - p) in fp32) or None; y fp32 or IEEE fp16.
    -> dict: dy16 [R, C] bf16 (round to nearest even of ((dout s) keep) gamma, the kernel's order), dy16T [C, ldt] bf16 with exact
    zeros from column R on, db / dgamma in fp64 (sums of the unrounded fp32 dy and of d y) and the sums of |terms| of both."""
    R, C = dout.shape
    s = row_scale(sample_scale, rows_per_sample, R)
    d = dout if s is None else dout * s
    if keep is not None:
        d = d * keep
    dy = d * gamma
    dy16 = dy.to(torch.bfloat16)
    ldt = (R + 63) // 64 * 64 if ldt is None else ldt
    dy16T = torch.zeros((C, ldt), dtype=torch.bfloat16, device=dout.device)
    dy16T[:, :R] = dy16.t()
    t = d.double() * y.double()
    return {"dy16": dy16, "dy16T": dy16T, "db": dy.double().sum(0), "db_mag": dy.double().abs().sum(0),
            "dgamma": t.sum(0), "dgamma_mag": t.abs().sum(0)}


def keep_value(p):
    """fp32(1 / (1 - p)) as the kernels form it: fp32 subtraction, fp32 division."""
    one = torch.tensor(1.0, dtype=torch.float32)
    return (one / (one - torch.tensor(p, dtype=torch.float32))).item()


def check_keep(keep, p):
    """The recovered keep-scales: exactly 0 or fp32(1 / (1 - p)), keep rate within 0.03 of 1 - p.  -> the measured keep rate."""
    kv = keep_value(p)
    assert bool(((keep == 0) | (keep == kv)).all()), "a keep-scale that is neither 0 nor 1 / (1 - p)"
    rate = (keep != 0).double().mean().item()
    assert abs(rate - (1 - p)) <= 0.03, rate
    return rate


# ---- activation backward ---------------------------------------------------------------------------------------------------------
def relu_bwd(dy, aux):
    """Exact: dy where aux > 0, +0 elsewhere."""
    return torch.where(aux > 0, dy, torch.zeros_like(dy))


def gelu_bwd(dy, h):
    """fp64 dy (Phi(h) + h phi(h))."""
    dy, h = dy.double(), h.double()
    cdf = 0.5 * (1 + torch.erf(h / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * h * h) / math.sqrt(2 * math.pi)
    return dy * (cdf + h * pdf)


def gelu_err_units(got, dy, h):
    """Worst per-element error against fp64 in units of |dy| (elements with dy == 0 must be exact zeros)."""
    ref = gelu_bwd(dy, h)
    err = (got.double() - ref).abs()
    nz = dy != 0
    assert bool((err[~nz] == 0).all())
    return (err[nz] / dy.double().abs()[nz]).max().item() if bool(nz.any()) else 0.0


def gelu_allowance(torch_units):
    """4 x the worst figure of torch's own fp32 autograd of F.gelu on the same inputs, plus 2^-23."""
    return 4 * torch_units + 2.0 ** -23


def torch_gelu_bwd(dy, h):
    """torch's fp32 autograd of F.gelu (the yardstick), on the device of the arguments."""
    hh = h.detach().clone().requires_grad_()
    (g,) = torch.autograd.grad(torch.nn.functional.gelu(hh), hh, dy)
    return g


# ---- dropout ---------------------------------------------------------------------------------------------------------------------
def check_dropout(x, y, p):
    """Every output is exactly x 0 or x fp32(1 / (1 - p)) (fp32 product).  -> the mask (True = kept; undecided where x == 0)."""
    kv = torch.tensor(keep_value(p), dtype=torch.float32, device=x.device)
    kept, dropped = bits(y) == bits(x * kv), bits(y) == bits(x * 0.0)
    assert bool((kept | dropped).all()), "an output that is neither x * 0 nor x / (1 - p)"
    return kept.view(x.shape)
