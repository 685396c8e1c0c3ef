"""numpy restatement of spe_grad_report's record (include/spe_hip.h): the documented fp32 order, the same quantities in fp64, the bound
between the two, and a brute-force computation of the exact words.  Nothing here calls the library.

The order of a sum over a parameter of L elements (x_j the squares, +0.0 past the end), chunk by chunk of 16384 elements (T = 256 lanes):
  1. y_v = (x_4v + x_4v+1) + (x_4v+2 + x_4v+3)                    two additions
  2. a_t = ((0 + y_t) + y_(t+T)) + ...                             one addition per pass of 1024 elements, 16 passes at most
  3. six xor-butterfly steps inside each wave of 64 lanes          six additions
  4. P_c = (((0 + w_0) + w_1) + w_2) + w_3 over the 4 wave sums    four additions (the first one exact)
  5. ((0 + P_0) + P_1) + ... over the chunks                       one addition per chunk (the first one exact)"""
import numpy as np

from grad_report_cases import CHUNK, PASS_SPAN, THREADS

U = 2.0 ** -24                       # unit roundoff of fp32, round to nearest
F32 = np.float32


def sum32(x):
    """The documented order over fp32 values x (1-D), every addition rounded to fp32; all chunks at once along the first axis."""
    x = np.asarray(x, dtype=F32)
    chunks = max(1, -(-x.size // CHUNK))
    a = np.zeros(chunks * CHUNK, dtype=F32)
    a[:x.size] = x
    a = a.reshape(chunks, CHUNK // PASS_SPAN, THREADS, 4)
    with np.errstate(over="ignore", invalid="ignore"):
        y = (a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])
        acc = np.zeros((chunks, THREADS), dtype=F32)
        for k in range(CHUNK // PASS_SPAN):              # passes past the chunk's end add +0.0: the bits stay
            acc = acc + y[:, k]
        w = acc.reshape(chunks, THREADS // 64, 64)
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            w = w + w[:, :, lanes ^ o]
        part = np.zeros(chunks, dtype=F32)
        for i in range(THREADS // 64):
            part = part + w[:, i, 0]
        r = F32(0.0)
        for c in range(chunks):
            r = r + part[c]
    assert r.dtype == F32
    return r


def chain(L):
    """Additions the square of one element passes through on its way into the sum: the longest chain - two inside its vector, one per
    pass of its chunk, six butterfly steps, four wave sums, one per chunk."""
    return 2 + min(CHUNK // PASS_SPAN, max(1, -(-L // PASS_SPAN))) + 6 + THREADS // 64 + max(1, -(-L // CHUNK))


def record32(g, p, scale):
    """-> dict of the record's words 0..6 in the documented fp32 arithmetic (p None: words 2, 3 are 0)."""
    g = np.asarray(g, dtype=F32).reshape(-1)
    fin = np.isfinite(g)
    g0 = np.where(fin, g, F32(0.0)).astype(F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        s = F32(scale) * g0
        q = s * s
        rec = {"grad_sq": sum32(q), "grad_absmax": np.max(np.abs(s), initial=F32(0.0)), "weight_sq": F32(0.0), "weight_absmax": F32(0.0)}
        if p is not None:
            p = np.asarray(p, dtype=F32).reshape(-1)
            rec["weight_sq"] = sum32(p * p)
            rec["weight_absmax"] = np.fmax.reduce(np.abs(p), initial=F32(0.0))
    bad = np.flatnonzero(~fin)
    rec["nan"], rec["inf"] = int(np.isnan(g).sum()), int(np.isinf(g).sum())
    rec["first_bad"] = int(bad[0]) if bad.size else -1
    return rec


def words(rec, attempt=0):
    """The eight 4-byte words of a record as uint32."""
    f = np.array([rec["grad_sq"], rec["grad_absmax"], rec["weight_sq"], rec["weight_absmax"]], dtype=F32).view(np.uint32)
    i = np.array([rec["nan"], rec["inf"], rec["first_bad"], attempt], dtype=np.int32).view(np.uint32)
    return np.concatenate([f, i])


def record64(g, p, scale):
    """The two sums in fp64 from the fp32 inputs (non-finite gradient elements contribute nothing)."""
    g = np.asarray(g, dtype=F32).reshape(-1).astype(np.float64)
    g = np.where(np.isfinite(g), g, 0.0)
    out = {"grad_sq": float(np.sum((float(F32(scale)) * g) ** 2)), "weight_sq": 0.0}
    if p is not None:
        out["weight_sq"] = float(np.sum(np.asarray(p, dtype=F32).reshape(-1).astype(np.float64) ** 2))
    return out


def bound(L, exact, roundings_before):
    """|fp32 sum - fp64 sum| for non-negative terms that do not overflow: every term carries `roundings_before` relative roundings
    into its square (grad: s = scale * g, then s * s squares the first one - three factors (1 + d); weight: p * p, one) and then at most
    chain(L) additions, each one more factor (1 + d), |d| <= U: (1 + U)^(chain + before) - 1 of the exact sum.  A product that lands
    in the subnormal range is off by at most half a subnormal step instead (2^-150 for s, which moves s * s by less than that again,
    and 2^-150 for the square): 2^-149 per element; additions of subnormals are exact.  The fp64 sum itself: L roundings of 2^-53."""
    return ((1.0 + U) ** (chain(L) + roundings_before) - 1.0 + L * 2.0 ** -53) * exact + L * 2.0 ** -149


def brute(g, p, scale):
    """Counts, first index and both maxima by the plainest means: a Python loop over the elements as Python floats.  The product of two
    fp32 values is exact in fp64, and rounding is monotonic, so the largest exact |scale * g| rounded once to fp32 is the largest of
    the rounded products."""
    nan = inf = 0
    first = -1
    gmax, sc = 0.0, float(F32(scale))
    for j, x in enumerate(np.asarray(g, dtype=F32).reshape(-1).tolist()):
        if x != x:
            nan += 1
        elif x in (float("inf"), float("-inf")):
            inf += 1
        else:
            gmax = max(gmax, abs(sc * x))
            continue
        if first < 0:
            first = j
    pmax = 0.0
    if p is not None:
        for x in np.asarray(p, dtype=F32).reshape(-1).tolist():
            if x == x:
                pmax = max(pmax, abs(x))
    with np.errstate(over="ignore", under="ignore"):
        return {"nan": nan, "inf": inf, "first_bad": first, "grad_absmax": F32(gmax), "weight_absmax": F32(pmax)}
