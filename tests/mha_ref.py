"""fp64 restatement of the flash multi-head attention (csrc/mha_flash.hip) on the operands the kernels see, element-wise error bounds
derived from the kernels' rounding points, and a torch emulation of the kernels' arithmetic (tests/test_mha_ref_cpu.py shows that a
correct implementation fits the bounds before any GPU run).  No project code is imported here.

Operands.  The kernels read q^ = fp16(q * scale * log2 e), k^ = fp16(k), v^ = fp16(v) in the forward and the bf16 roundings of the
same values, and bf16(dO), in the backward.  `operands()` draws q^, k^, v^ and dO on a grid both 16-bit formats hold (8 significant
bits, magnitude in [2^-14, 2^15] or 0), so reference and kernel share every operand and only the kernel's internal roundings remain.

Operator (log2 domain; kd = keep / (1 - p_drop), 1 without dropout; masked and out-of-range keys excluded):
  s = q^ k^T     LSE = log2 sum_k 2^s     P = 2^(s - LSE)     O = sum_k P kd v^
  dP = dO v^T    D = rowsum(dO . O) rounded to fp32, as handed to the kernel    dS = P (kd dP - D)
  dq = scale dS k^      dk = ln 2 dS^T q^      dv = (P kd)^T dO

Bounds.  u16 = 2^-11 (fp16), ub = 2^-9 (bf16), u32 = 2^-24 (fp32) are unit roundoffs.  |x| is the element-wise absolute value,
ntk the key tiles, nch the key chunks.
  scores      e_s(q,k)  = (dk + 8) u32 sum_d |q^||k^|                        fp32 sum of exact products
              a score error moves P by the factor 2^(ds - sum_j P_j ds_j):   relP(q,k) = ln2 (e_s + E_s),  E_s(q) = sum_j P_j e_s(q,j)
  exp2, alpha eps_x(q)  = (ntk + nch + 4) 2^-22 + ln2 2^-22 (max_k s - min_k s)
              one hardware exp2 (1 ulp) per element and one per rescale and merge step, and the fp32 rounding of their arguments,
              whose magnitudes along the chain of rescales add up to at most the row's score range
  row sum l   eps_l     = (6 ntk + nch + 4) u32                              l = l alpha + (p0 + p1 + p2 + p3), lane and chunk sums
  P.V sum     g_o       = (Lk + 2 ntk + nch + 4) u32                         fp32 accumulation, rescales, merge
  flush       F_O(q,d)  = sum_k [2^(s - max s) < 2^-14] P kd |v^|            p relative to any running maximum <= the final one is
              at least that, so only these can fall below fp16's normal range, where they lose at most their whole value
  O           A = sum_k P kd |v^|;   |O - ref| <= A (u16 + g_o + 2 eps_x + eps_l + 4 u32) + sum_k P relP kd |v^| + F_O
              u16 is the rounding of p (times kd) to fp16 in front of P.V; 4 u32 the reciprocal and the final product
  LSE         |LSE - ref| <= E_s + (eps_l + eps_x) / ln2 + 2^-22 max(1, |log2 L|) + 2 u32 (|M| + |LSE|),   L = sum_k 2^(s - M), M = max s
              (score error of the terms, relative error of L through one log2, the hardware log2, the fp32 sum M + log2 L)
  backward    eps_p(q,k) = ln2 (e_s + u32 (|LSE| + |s - LSE|)) + 2^-22       P recomputed as exp2(s - fp32(LSE))
              e_dp(q,k)  = (dv + 8) u32 sum_d |dO||v^|
              e_dS       = P (eps_p |kd dP - D| + kd e_dp + 3 u32 (|kd dP| + |D|)) + ub |dS|        (ub: dS through bf16)
              g          = (max(Lq, Lk) + ntk + nch + 8) u32
              |dq - ref| <= scale (sum_k e_dS |k^| + g sum_k |dS||k^|)
              |dk - ref| <= ln2   (sum_q e_dS |q^| + g sum_q |dS||q^|)
              |dv - ref| <= sum_q P kd (ub + eps_p + g) |dO|                                        (ub: P kd through bf16)
Every bound is multiplied by (1 + 2^-8) for the products of two error terms and carries 2^-100 for flushed subnormals.  The
leading terms are u16 sum_k P |v^| for O and ub times the absolute contraction for dq, dk, dv.  The GPU test asserts
err <= 2 bound.

ub.  bf16 keeps 8 significant bits, so ONE rounding can be off by up to 2^-8 relative (1 + 2^-8 lies midway between two bf16
values); 2^-9 is what the backward bounds (bdq, bdk, bdv) use, and a contraction of a single term - Lk = 1, one key left by the mask,
Lq = 1 for dk and dv - can therefore reach 2 x bound with correct arithmetic, all of the factor the GPU test allows.  The CPU
emulation is held to 1 x bound for O and LSE and, for the gradients, to 1 x the same bounds with ub = 2^-8 (bdqw, bdkw, bdvw), which
are nowhere above 2 x the asserted ones: a correct implementation fits what the GPU test asserts."""
import math

import torch

U16, UB, U32 = 2.0 ** -11, 2.0 ** -9, 2.0 ** -24
UB_WORST = 2.0 ** -8            # the largest relative error of one bf16 rounding (8 significant bits); see the docstring
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
TINY = 2.0 ** -100
SLACK = 1.0 + 2.0 ** -8


def grid(x):
    """Round to 8 significant bits inside fp16's normal range: exact in fp16 and in bf16."""
    y = x.to(torch.bfloat16).to(torch.float64).clamp(-32768.0, 32768.0)
    return torch.where(y.abs() < 2.0 ** -14, torch.zeros_like(y), y)


def coarse(x):
    """Multiples of 1/8 up to 4: every sum of up to 96 products is exact in fp32 in any order."""
    return (x * 8).round().clamp(-32, 32) / 8


def operands(case, device="cpu"):
    """-> dict: q [B,Lq,H,dk], k [B,Lk,H,dk], v [B,Lk,H,dv], do [B,Lq,H,dv] (fp64, on the 16-bit grid; q already carries
    scale * log2 e), mask (bool [B,Lk], True = padded, or None), scale (what spe_mha_bwd multiplies dq by)."""
    import mha_cases as C
    B, H, Lq, Lk, dk, dv, mfam, sfam, p, nch = case
    g = torch.Generator().manual_seed(7 + 13 * Lq + 17 * Lk + 19 * dk + 23 * dv + 29 * B + C.SCORES.index(sfam))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    q = rn(B, Lq, H, dk) * (LOG2E * dk ** -0.5)
    k, v, do = rn(B, Lk, H, dk), rn(B, Lk, H, dv), rn(B, Lq, H, dv)
    ntk = (Lk + 15) // 16
    tile = torch.arange(Lk) // 16
    if sfam in ("ascending", "descending"):
        q *= 0.5                   # the seeded part moves a tile's maximum by well under the step of 4
        q[..., 0] = 1.0
        k[..., 0] = (4.0 * (tile if sfam == "ascending" else ntk - 1 - tile)).to(torch.float64)[None, :, None]
    elif sfam == "wide":
        q[..., 0] = 1.0
        k[..., 0] = torch.randint(-30, 31, (B, Lk, H), generator=g).to(torch.float64)
    elif sfam == "ties":
        q[..., 0] = 1.0
        k[..., 0] = 0.0
        ties = C.tie_keys(Lk)
        k[:, ties] = k[:, ties[0]].clone().unsqueeze(1)
        k[:, ties, :, 0] = 16.0
    if mfam == "one_key":
        q, k = coarse(q), coarse(k)
    rows = C.mask_rows(case)
    mask = None if rows is None else torch.tensor(rows, dtype=torch.bool)
    out = dict(q=grid(q), k=grid(k), v=grid(v), do=grid(do), mask=mask, scale=dk ** -0.5)
    return {n: (t.to(device) if torch.is_tensor(t) else t) for n, t in out.items()}


def host_keep(case, seed=5):
    """A seeded keep matrix [B,H,Lq,Lk] for the CPU checks (the GPU test decodes the kernel's own)."""
    B, H, Lq, Lk, p = case[0], case[1], case[2], case[3], case[8]
    if p == 0:
        return None
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, H, Lq, Lk, generator=g) >= p


def _t(x):
    return x.permute(0, 2, 1, 3)            # [B,L,H,d] <-> [B,H,L,d]


def reference(op, p_drop=0.0, keep=None, nch=1):
    """fp64 outputs and bounds.  -> dict: O [B,Lq,H,dv], LSE [B,H,Lq], D [B,H,Lq] (fp32-rounded), dq, dk, dv [B,L,H,d], their
    bounds bO, bLSE, bdq, bdk, bdv (and bdqw, bdkw, bdvw: ub = 2^-8), and dead (bool [B]: batches with every key padded, whose rows are excluded: P = 0 there)."""
    q, k, v, do = (_t(op[n]) for n in ("q", "k", "v", "do"))               # [B,H,L,d]
    B, H, Lq, dk = q.shape
    Lk, dv = k.shape[2], v.shape[3]
    ntk = (Lk + 15) // 16
    valid = torch.ones(B, 1, 1, Lk, dtype=torch.bool, device=q.device) if op["mask"] is None else ~op["mask"][:, None, None, :]
    dead = ~valid.reshape(B, Lk).any(-1)
    s = q @ k.transpose(-1, -2)
    sm = s.masked_fill(~valid, float("-inf"))
    M = sm.amax(-1, keepdim=True)
    M = torch.where(dead[:, None, None, None], torch.zeros_like(M), M)
    prel = torch.exp2(sm - M)
    L = prel.sum(-1, keepdim=True)
    L = torch.where(dead[:, None, None, None], torch.ones_like(L), L)
    LSE = M + torch.log2(L)
    P = prel / L
    kd = torch.ones_like(P) if keep is None else keep.to(P.dtype) / (1.0 - p_drop)
    Pd = P * kd
    O = Pd @ v
    D = (do * O).sum(-1, keepdim=True).float().double()
    dP = do @ v.transpose(-1, -2)
    T = kd * dP - D
    dS = P * T
    dq = op["scale"] * (dS @ k)
    dk_ = LN2 * (dS.transpose(-1, -2) @ q)
    dv_ = Pd.transpose(-1, -2) @ do
    # ---- bounds (module docstring) ----
    aq, ak, av, ado = q.abs(), k.abs(), v.abs(), do.abs()
    e_s = (dk + 8) * U32 * (aq @ ak.transpose(-1, -2))
    E_s = (P * e_s).sum(-1, keepdim=True)
    relP = LN2 * (e_s + E_s)
    smin = s.masked_fill(~valid, float("inf")).amin(-1, keepdim=True)
    rng = torch.where(dead[:, None, None, None], torch.zeros_like(M), M - smin)
    eps_x = (ntk + nch + 4) * 2.0 ** -22 + LN2 * 2.0 ** -22 * rng
    eps_l = (6 * ntk + nch + 4) * U32
    g_o = (Lk + 2 * ntk + nch + 4) * U32
    bO = ((Pd @ av) * (U16 + g_o + 2 * eps_x + eps_l + 4 * U32) + (Pd * relP) @ av + (Pd * (prel < 2.0 ** -14)) @ av) * SLACK + TINY
    bLSE = (E_s + (eps_l + eps_x) / LN2 + 2.0 ** -22 * torch.log2(L).abs().clamp(min=1.0) + 2 * U32 * (M.abs() + LSE.abs())) * SLACK + TINY
    eps_p = LN2 * (e_s + U32 * (LSE.abs() + (s - LSE).abs())) + 2.0 ** -22
    e_dp = (dv + 8) * U32 * (ado @ av.transpose(-1, -2))
    g = (max(Lq, Lk) + ntk + nch + 8) * U32
    e_dS0 = P * (eps_p * T.abs() + kd * e_dp + 3 * U32 * ((kd * dP).abs() + D.abs()))
    out = {}
    for tag, ub in (("", UB), ("w", UB_WORST)):
        e_dS = e_dS0 + ub * dS.abs()
        out["bdq" + tag] = _t(op["scale"] * (e_dS @ ak + g * (dS.abs() @ ak)) * SLACK + TINY)
        out["bdk" + tag] = _t(LN2 * (e_dS.transpose(-1, -2) @ aq + g * (dS.abs().transpose(-1, -2) @ aq)) * SLACK + TINY)
        out["bdv" + tag] = _t(((Pd * (ub + eps_p + g)).transpose(-1, -2) @ ado) * SLACK + TINY)
    LSE = torch.where(dead[:, None, None, None], torch.full_like(LSE, float("-inf")), LSE)
    return dict(O=_t(O), LSE=LSE[..., 0], D=D[..., 0], dq=_t(dq), dk=_t(dk_), dv=_t(dv_), bO=_t(bO), bLSE=bLSE[..., 0],
                dead=dead, P=P, valid=valid, **out)


def ratio(got, ref, bound, live=None):
    """Worst |got - ref| / bound over the rows of live batches; inf if anything there is not finite."""
    err = (got.double() - ref).abs() / bound
    if live is not None:
        err = err[live]
    if err.numel() == 0:
        return 0.0
    return float("inf") if not bool(torch.isfinite(err).all()) else float(err.max())


def emulate(op, ch_len, p_drop=0.0, keep=None, lse=None, D=None, bwd_ch_len=None):
    """The kernels' arithmetic in torch: fp32 score sums, a per-tile online softmax inside chunks of ch_len key tiles and the merge
    of the chunk partials, p through fp16 in front of P.V; backward with P recomputed from the fp32 LSE, dS and P kd through bf16,
    fp32 sums, dq as per-chunk slabs added in chunk order.  -> O, LSE, dq, dk, dv (fp32; layouts of reference())."""
    q, k, v, do = (_t(op[n]).float() for n in ("q", "k", "v", "do"))
    B, H, Lq, dk = q.shape
    Lk, dv = k.shape[2], v.shape[3]
    ntk = (Lk + 15) // 16
    ninf = float("-inf")
    valid = torch.ones(B, 1, 1, Lk, dtype=torch.bool) if op["mask"] is None else ~op["mask"][:, None, None, :]
    kd = torch.ones(B, H, Lq, Lk) if keep is None else keep.float() * torch.tensor(1.0 / (1.0 - p_drop), dtype=torch.float32)
    s = (q @ k.transpose(-1, -2)).masked_fill(~valid, ninf)
    parts = []
    for t0 in range(0, ntk, ch_len):
        m = torch.full((B, H, Lq, 1), ninf); l = torch.zeros(B, H, Lq, 1); o = torch.zeros(B, H, Lq, dv)
        for t in range(t0, min(t0 + ch_len, ntk)):
            sl = slice(16 * t, min(16 * t + 16, Lk))
            sv = s[..., sl]
            mn = torch.maximum(m, sv.amax(-1, keepdim=True))
            alpha = torch.where(m > ninf, torch.exp2(m - mn), torch.zeros_like(m))
            p = torch.where(sv > ninf, torch.exp2(sv - mn), torch.zeros_like(sv))
            l = l * alpha + p.sum(-1, keepdim=True)
            o = o * alpha + (p * kd[..., sl]).half().float() @ v[:, :, sl]
            m = mn
        parts.append((m, l, o))
    Mx = parts[0][0]
    for m, _, _ in parts[1:]:
        Mx = torch.maximum(Mx, m)
    Lsum = torch.zeros(B, H, Lq, 1); acc = torch.zeros(B, H, Lq, dv)
    for m, l, o in parts:
        w = torch.where(m > ninf, torch.exp2(m - Mx), torch.zeros_like(m))
        Lsum = Lsum + l * w
        acc = acc + o * w
    O = acc * (1.0 / Lsum)
    LSE = Mx + torch.log2(Lsum)
    if lse is None:
        return _t(O), LSE[..., 0]
    lse32, D32 = lse.float()[..., None], D.float()[..., None]
    p = torch.where(s > ninf, torch.exp2(s - lse32), torch.zeros_like(s))
    dp = do @ v.transpose(-1, -2)
    ds = (p * (dp * kd - D32)).bfloat16().float()
    pb = (p * kd).bfloat16().float()
    dq = torch.zeros(B, H, Lq, dk)
    step = 16 * (bwd_ch_len or ch_len)
    for k0 in range(0, Lk, step):
        dq = dq + (ds[..., k0:k0 + step] @ k[:, :, k0:k0 + step]) * torch.tensor(op["scale"], dtype=torch.float32)
    dk_ = (ds.transpose(-1, -2) @ q) * torch.tensor(LN2, dtype=torch.float32)
    dv_ = pb.transpose(-1, -2) @ do
    return _t(O), LSE[..., 0], _t(dq), _t(dk_), _t(dv_)
