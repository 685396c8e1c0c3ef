"""fp64 references of the four small-row Linear operations (csrc/linear_small.hip) on the operands as the kernels see them, the error
bounds of the bounded cases, and a torch emulation of the kernels' roundings.  Plain torch, any device; nothing here calls the library.

What the kernels see: the forward stages x rounded to bf16 (round to nearest even), with W16lo also bf16(x - bf16(x)), and multiplies
x_hi W_hi (+ x_hi W_lo + x_lo W_hi: the lo x lo term is dropped) into fp32 accumulators, 32 contraction elements per MFMA.  The backward
forms dy' = dy times the derivative of the fused activation in fp32, sums db from dy' itself and multiplies bf16(dy') with W^T / x16."""
import math

import torch

BF = torch.bfloat16


def rne_bf16(x32):
    """fp32 -> the nearest bf16 value, ties to even, as fp32; by integer arithmetic on the bits (finite inputs)."""
    b = x32.contiguous().view(torch.int32)
    r = (b + 0x7FFF + ((b >> 16) & 1)) & ~0xFFFF
    return r.view(torch.float32)


def hilo(x):
    """fp64 holding fp32 values -> (bf16(x), bf16(x - bf16(x))) as fp64."""
    hi = rne_bf16(x.float())
    lo = rne_bf16(x.float() - hi)
    return hi.double(), lo.double()


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dgelu64(h):
    return 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0))) + h * torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)


def act64(pre, act):
    return pre if act == 0 else pre.clamp_min(0.0) if act == 1 else gelu64(pre)


def dact64(dy, aux, act):
    """dy' = dy * act'(aux); act 1: aux is the forward OUTPUT, the derivative is 1 where aux > 0 (so +0 and -0 give 0)."""
    if act == 0 or aux is None:
        return dy
    if act == 1:
        return torch.where(aux > 0, dy, torch.zeros_like(dy))
    return dy * dgelu64(aux)


def fwd_ref(x, Wh, Wl, bias, add=None):
    """-> (pre-activation, |x| |W|) in fp64; x [R, K] (fp32 values), Wh / Wl [N, K] (bf16 values; Wl None: single term)."""
    xh, xl = hilo(x)
    if Wl is None:
        acc, mag = xh @ Wh.t(), x.abs() @ Wh.abs().t()
    else:
        acc, mag = xh @ Wh.t() + xh @ Wl.t() + xl @ Wh.t(), x.abs() @ (Wh + Wl).abs().t()
    if add is not None:
        acc = acc + add
    if bias is not None:
        acc = acc + bias
    return acc, mag


def bwd_ref(dy, aux, act, x16, WT):
    """-> dict(dx [R, K], dW [N, K], db [N], and the magnitudes mdx, mdw, mdb of the bounds); dy / aux [R, N], x16 [R, K], WT [K, N], fp64."""
    dyp = dact64(dy, aux, act)
    d16 = rne_bf16(dyp.float()).double()
    out = dict(dyp=dyp, db=dyp.sum(0), mdb=dyp.abs().sum(0))
    if WT is not None:
        out["dx"], out["mdx"] = d16 @ WT.t(), dyp.abs() @ WT.abs().t()
    if x16 is not None:
        out["dW"], out["mdw"] = d16.t() @ x16, dyp.abs().t() @ x16.abs()
    return out


def group_fwd_ref(x, Whs, Wls, biases, adds):
    return [fwd_ref(x, Whs[i], None if Wls is None else Wls[i], biases[i], adds[i])[0] for i in range(len(Whs))]


def group_bwd_ref(dys, x16, WTs):
    """-> (dx [R, K] or None without WTs, [dW_i or None], [db_i or None]); dys[i] None: output i has no gradient."""
    dx = None
    if WTs is not None:
        dx = torch.zeros((x16.shape[0], WTs[0].shape[0]), dtype=torch.float64, device=x16.device)
        for dy, WT in zip(dys, WTs):
            if dy is not None:
                dx = dx + rne_bf16(dy.float()).double() @ WT.t()
    dWs = [None if dy is None else rne_bf16(dy.float()).double().t() @ x16 for dy in dys]
    dbs = [None if dy is None else dy.sum(0) for dy in dys]
    return dx, dWs, dbs


# ---- bounds of the random-normal cases (element-wise, against the fp64 product of the UNROUNDED fp32 operand) -------------------------------
def bound_plain(mag, depth):
    """One operand rounded to bf16 while staged (relative 2^-9, the other is bf16 already): 2^-8 |A| |B| with room to spare, plus one fp32
    rounding per 32-deep MFMA step and three for the epilogue."""
    return (2.0 ** -8 + (depth / 32 + 3) * 2.0 ** -24) * mag


def bound_split(mag, depth):
    """Three-term product: the residual of x beyond hi + lo (2^-18), of W beyond hi + lo (2^-18) and the dropped lo x lo term (2^-18)."""
    return (3 * 2.0 ** -18 + (depth / 32 + 3) * 2.0 ** -24) * mag


def bound_db(mdb, R):
    return R * 2.0 ** -24 * mdb


# ---- emulation of the kernels' roundings --------------------------------------------------------------------------------------------------
def emulate_nt(A32, Bh, Bl=None):
    """C = A B^T as ls_nt_tile computes it: A fp32 [R, K] staged as RNE bf16 (hi, and with Bl the low part too), B bf16 values [N, K] (fp64 or
    fp32 tensors); per 32-deep step the MFMAs (lo-of-B x hi, hi x lo-of-A, hi x hi) each add their exact sum into the fp32 accumulator."""
    Ah = rne_bf16(A32.float())
    Al = rne_bf16(A32.float() - Ah)
    Ah, Al, Bh = Ah.double(), Al.double(), Bh.double()
    acc = torch.zeros((A32.shape[0], Bh.shape[0]), dtype=torch.float32, device=A32.device)
    for k in range(0, A32.shape[1], 32):
        s = slice(k, k + 32)
        if Bl is not None:
            acc = (acc.double() + Ah[:, s] @ Bl.double()[:, s].t()).float()
            acc = (acc.double() + Al[:, s] @ Bh[:, s].t()).float()
        acc = (acc.double() + Ah[:, s] @ Bh[:, s].t()).float()
    return acc


def emulate_tn(dyp32, x16):
    """dW = bf16(dy')^T x16 as the dW program computes it: one exact 32-row sum per MFMA, added into the fp32 accumulator."""
    d = rne_bf16(dyp32.float()).double()
    x = x16.double()
    acc = torch.zeros((d.shape[1], x.shape[1]), dtype=torch.float32, device=d.device)
    for r in range(0, d.shape[0], 32):
        acc = (acc.double() + d[r:r + 32].t() @ x[r:r + 32]).float()
    return acc


def emulate_db(dyp32):
    """db as the dW program sums it: row r goes to partial r % 32 (fp32, rows in order), the 32 partials are added in order."""
    R, N = dyp32.shape
    pad = torch.zeros((-R % 32, N), dtype=torch.float32, device=dyp32.device)
    p = torch.cat([dyp32.float(), pad]).view(-1, 32, N)
    part = torch.zeros((32, N), dtype=torch.float32, device=dyp32.device)
    for i in range(p.shape[0]):
        part = part + p[i]
    s = torch.zeros((N,), dtype=torch.float32, device=dyp32.device)
    for i in range(32):
        s = s + part[i]
    return s


# ---- operands ----------------------------------------------------------------------------------------------------------------------------
def ints(g, shape, lim):
    """Random integers in [-lim, lim] as fp64."""
    return torch.randint(-lim, lim + 1, shape, generator=g).double()


def ties_bf16(g, shape):
    """Odd integers of 9 significant bits, either sign: each exactly halfway between two bf16 neighbours; -> (values, their RNE roundings
    worked out by hand: 2m + 1 goes to 2m when m is even, to 2m + 2 when m is odd)."""
    m = torch.randint(128, 256, shape, generator=g)
    sign = (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()
    rounded = torch.where(m % 2 == 0, 2 * m, 2 * m + 2).double()
    return sign * (2 * m + 1).double(), sign * rounded


def random_operands(c, dev):
    """Random-normal operands of a bounded case: forward -> (x fp32 [R, K], Wh, Wl or None: fp64 holding bf16 values [N, K]);
    backward -> (dy fp32 [R, N], x16 [R, K], WT [K, N]: fp64 holding bf16 values)."""
    g = torch.Generator().manual_seed(17 * c["R"] + c["N"] + c["K"])
    if c["entry"] == "fwd":
        x = torch.randn((c["R"], c["K"]), generator=g)
        W = torch.randn((c["N"], c["K"]), generator=g) / math.sqrt(c["K"])
        Wh, Wl = hilo(W.double())
        return x.to(dev), Wh.to(dev), (Wl.to(dev) if c["split"] else None)
    dy = torch.randn((c["R"], c["N"]), generator=g)
    x16 = rne_bf16(torch.randn((c["R"], c["K"]), generator=g)).double()
    WT = rne_bf16(torch.randn((c["K"], c["N"]), generator=g) / math.sqrt(c["N"])).double()
    return dy.to(dev), x16.to(dev), WT.to(dev)
