"""The decoder's memory-side key / value path (csrc/decoder_kv.hip, ops._MemorySideKV / ops._CrossAttentionKV) tested on its own.

Tier 1 - bit exact: spe_kv_frags against an index restatement of the four fragment layouts (tests/kv_layout.py) and against
         spe_attn_pack_multi (the header promises the same layouts); its argument checks; spe_kv_grad_scatter (stores exactly its
         three column blocks, nothing else).
Tier 2 - the fp16 projection GEMM element by element (one fp16 ulp); ops.memory_side_kv + ops.cross_attention_kv against an fp64 restatement (softmax(scale q [k_c | k_p]^T + mask) v, autograd).
         Two metrics per tensor - the global Frobenius ratio `rel` and a per-row one (one wrong 16-token tile shows as a row error near 1)
         - and thresholds that come from a ROUNDED-OPERAND MODEL evaluated here in fp64 with no project kernel involved: the same
         formulas with a cast to fp16 / bf16 wherever the path rounds (list below).  With e_model = the model's distance from exact
         fp64, the kernels must satisfy err <= 2 e_model + 1e-5 in both metrics (model and kernel are two draws of a rounding error of
         the same size; the kernel adds fp32 accumulation order and online-softmax rescaling), and the project's global bounds:
         TOL["bf16"] on O, 2 TOL["bf16"] on gradients.
Tier 3 - TransformerDecoder (3 layers, 2 stages, a 2-D padding mask) against the fp64 oracle, with the MEMKV = False path as a second
         witness: this is what pins the layer-0 identity q_c (k_c + k_p) + q_s k_p = q_c k_c + (q_s + q_c) k_p.

Rounding points of the path (csrc/mha_flash.hip, ops.py):
  fp16: memory, pos, the stacked weights (K.cvt_f16 / K.weightcat_f16), the GEMM outputs ym / yp (act bit 9), q * scale * log2(e)
        (Qf), the forward's probabilities relative to the row maximum (the P.V operand);
  bf16: K16, Vf (spe_kv_frags), Q16 = bf16(q * scale * log2(e)), dO (dOf, dO16), dS and P of the backward, the scattered dk / dv
        (spe_kv_grad_scatter), memory / pos / weights as operands of the backward GEMMs.
Measured figures: profiles/decoder_kv_direct.txt (every line this module prints with the prefix KVDIRECT)."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import kv_layout as kl  # noqa: E402
from test_kernels_gpu import TOL, rel  # noqa: E402  (the project's existing bounds and global metric)

pytestmark = pytest.mark.gpu

FILL = 0x5A5A               # the 16-bit pattern every output buffer holds before a launch (fp16 203.25, bf16 1.5e16: never produced here)
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453


def _filled(shape, dtype, dev):
    return torch.full(shape, FILL, dtype=torch.int16, device=dev).view(dtype)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _untouched(t):
    return bool((_bits(t) == FILL).all())


# ------------------------------------------------------------------------------------------------------------------------------
# Tier 1
# ------------------------------------------------------------------------------------------------------------------------------
def _frag_outputs(L, B, S, H, dh, dev, train):
    nt, dk = (S + 15) // 16, 2 * dh
    Kf = _filled((L, B, H, nt, (dk + 31) // 32, 64, 8), torch.float16, dev)
    V16 = _filled((L, B, H, nt, (dh + 15) // 16, 64, 4), torch.float16, dev)
    K16 = _filled((L, B, H, nt, (dk + 15) // 16, 64, 4), torch.bfloat16, dev) if train else None
    Vf = _filled((L, B, H, nt, (dh + 31) // 32, 64, 8), torch.bfloat16, dev) if train else None
    return Kf, V16, K16, Vf


def _kv_frags_raw(ym, ldm, yp, ldp, outs, L, B, S, H, dh):
    from spe_amd import kernels as K
    ptr = lambda t: None if t is None else t.data_ptr()
    K.lib.call("spe_kv_frags", ym.data_ptr(), ldm, yp.data_ptr(), ldp, *[ptr(o) for o in outs], L, B, S, H, dh, K._st())


def _gemm_outputs(L, B, S, H, dh, dev, wide, seed):
    """Seeded fp16 `ym` [B*S, 2 L d] / `yp` [B*S, L d]; wide: column views (16-byte aligned start, ld > columns, ld % 8 == 0) of buffers
    whose other columns hold a value that appears nowhere else."""
    d = H * dh
    g = torch.Generator().manual_seed(seed)

    def one(cols):
        x = (2 * torch.randn(B * S, cols, generator=g)).half()
        flat = x.view(-1)
        flat[0::97] = 6.0e-8            # fp16 subnormals, negative zero and large magnitudes also go through the bf16 conversion
        flat[1::89] = -0.0
        flat[2::83] = 60000.0
        flat[3::79] = -3.1e-5
        if not wide:
            return x.to(dev)
        buf = torch.full((B * S, cols + 24), 777.0, dtype=torch.float16)
        buf[:, 8:8 + cols] = x
        return buf.to(dev)[:, 8:8 + cols]
    return one(2 * L * d), one(L * d)


WIDE = {(3, 1, 523, 4, 24), (2, 2, 1100, 8, 32), (1, 1, 5, 3, 40)}


@pytest.mark.parametrize("train", [True, False], ids=["train", "fwdonly"])
@pytest.mark.parametrize("L,B,S,H,dh", kl.FRAG_CASES)
def test_kv_frags_layouts_bit_exact(dev, L, B, S, H, dh, train):
    """Every 16-bit pattern of Kf / V16 / K16 / Vf: the values at their slots, zeros in the rows >= S and the dims beyond the head dim
    of the half-filled last steps, over buffers that held FILL before the launch - against (a) tests/kv_layout.py and (b)
    spe_attn_pack_multi of the fp32 upcast of the per-layer keys / values.  cfg2's 25 248 records make every wave of the capped grid
    (4096 workgroups of 4 waves) reuse its LDS tile for a second record."""
    from spe_amd import kernels as K
    wide = (L, B, S, H, dh) in WIDE
    ym, yp = _gemm_outputs(L, B, S, H, dh, dev, wide, seed=S * 7 + dh)
    assert (ym.stride(0) > ym.shape[1]) == wide and ym.stride(0) % 8 == 0 and yp.stride(0) % 8 == 0
    outs = _frag_outputs(L, B, S, H, dh, dev, train)
    _kv_frags_raw(ym, ym.stride(0), yp, yp.stride(0), outs, L, B, S, H, dh)
    eKf, eV16, eK16, eVf, k, v = kl.expected_frags(ym, yp, L, B, S, H, dh)
    names = ("Kf", "V16", "K16", "Vf")
    for name, got, exp in zip(names, outs, (eKf, eV16, eK16, eVf)):
        if got is None:
            continue
        assert got.shape == exp.shape, name
        assert torch.equal(_bits(got), exp), f"{name}: {int((_bits(got) != exp).sum())} of {exp.numel()} patterns differ from the layout restatement"
    for l in range(L):
        kl32, vl32 = k[l].float().contiguous(), v[l].float().contiguous()
        jobs = [(kl32, 1.0, 322 + K.F16), (vl32, 1.0, 16 + K.F16)] + ([(kl32, 1.0, 16), (vl32, 1.0, 322)] if train else [])
        for name, got, pk in zip(names, outs, K.attn_pack_multi(jobs)):
            assert torch.equal(_bits(got[l]), _bits(pk)), f"{name}[{l}] differs from spe_attn_pack_multi"


def test_kv_frags_argument_checks(dev):
    """dh = 12, ldm % 8 != 0, K16 without Vf: status -2 before any launch, outputs untouched."""
    from spe_amd import kernels as K
    L, B, S, H = 1, 1, 16, 1
    ym, yp = _gemm_outputs(L, B, S, H, 16, dev, False, seed=1)
    outs = _frag_outputs(L, B, S, H, 16, dev, True)
    Kf, V16, K16, Vf = outs
    for args in [(ym, ym.stride(0), yp, yp.stride(0), outs, L, B, S, H, 12),
                 (ym, ym.stride(0) + 4, yp, yp.stride(0), outs, L, B, S, H, 16),
                 (ym, ym.stride(0), yp, yp.stride(0), (Kf, V16, K16, None), L, B, S, H, 16)]:
        with pytest.raises(K.lib.SpeLibraryError, match="status -2"):
            _kv_frags_raw(*args)
    torch.cuda.synchronize()
    assert all(_untouched(o) for o in outs)
    _kv_frags_raw(ym, ym.stride(0), yp, yp.stride(0), outs, L, B, S, H, 16)         # the same buffers are accepted with valid arguments
    torch.cuda.synchronize()
    assert not any(_untouched(o) for o in outs)


# (B, S, H, dh, L, layer, wide).  The last: B*S*H*3*dh/4 = 2 304 000 > 8192 * 256 threads -> the grid-stride loop runs a second pass
@pytest.mark.parametrize("B,S,H,dh,L,layer,wide", [(2, 37, 3, 8, 3, 1, False), (1, 523, 4, 24, 4, 2, True), (1, 12000, 8, 32, 3, 1, False)])
def test_kv_grad_scatter_stores_its_blocks_only(dev, B, S, H, dh, L, layer, wide):
    from spe_amd import kernels as K
    d, R = H * dh, B * S
    assert 0 < layer < L - 1                       # a middle layer: blocks on both sides must keep the sentinel
    g = torch.Generator().manual_seed(S + dh)
    dk = torch.randn(B, S, H, 2 * dh, generator=g).to(dev)
    dv = torch.randn(B, S, H, dh, generator=g).to(dev)
    pad = 24 if wide else 0
    bm, bp = _filled((R, 2 * L * d + pad), torch.bfloat16, dev), _filled((R, L * d + pad), torch.bfloat16, dev)
    off = 8 if wide else 0
    dYm, dYp = bm[:, off:off + 2 * L * d], bp[:, off:off + L * d]
    K.kv_grad_scatter(dk, dv, dYm, dYp, layer, B, S, H, dh)
    em, ep = _filled(bm.shape, torch.bfloat16, dev), _filled(bp.shape, torch.bfloat16, dev)
    em[:, off + 2 * layer * d:off + (2 * layer + 1) * d] = dk[..., :dh].reshape(R, d).to(torch.bfloat16)
    em[:, off + (2 * layer + 1) * d:off + (2 * layer + 2) * d] = dv.reshape(R, d).to(torch.bfloat16)
    ep[:, off + layer * d:off + (layer + 1) * d] = dk[..., dh:].reshape(R, d).to(torch.bfloat16)
    assert torch.equal(_bits(bm), _bits(em)), f"dYm: {int((_bits(bm) != _bits(em)).sum())} patterns differ"
    assert torch.equal(_bits(bp), _bits(ep)), f"dYp: {int((_bits(bp) != _bits(ep)).sum())} patterns differ"


# ------------------------------------------------------------------------------------------------------------------------------
# Tier 2
# ------------------------------------------------------------------------------------------------------------------------------
def _r16(x):
    return x.to(torch.float16).to(torch.float64)


def _rb(x):
    return x.to(torch.bfloat16).to(torch.float64)


def grid_mask():
    """The model's 2-D padding mask, flattened: a 50 x 84 grid whose second image is padded in rows >= 48 and columns >= 80 - a
    periodic pattern over the key index, not one contiguous tail."""
    m = torch.zeros(2, 50, 84, dtype=torch.bool)
    m[1, 48:, :] = True
    m[1, :, 80:] = True
    return m.flatten(1)


def _mask_of(kind, B, S):
    if kind is None:
        return None
    if kind == "grid":
        assert (B, S) == (2, 4200)
        return grid_mask()
    m = torch.zeros(B, S, dtype=torch.bool)
    m[B - 1, (6 * S) // 7:] = True              # one contiguous tail in the last image, not tile aligned
    return m


# name -> ((B, S, d, H, L, Lq), mask kind)
NODE_CASES = {"tail_1100": ((2, 1100, 256, 8, 2, 200), "tail"), "cfg2_grid": ((2, 4200, 256, 8, 6, 200), "grid"),
              "dh48_700": ((3, 700, 384, 8, 1, 37), "tail"), "dh8_520": ((4, 520, 64, 8, 3, 100), None)}


def make_inputs(name, dev):
    (B, S, d, H, L, Lq), mk = NODE_CASES[name]
    dh = d // H
    g = torch.Generator().manual_seed(1000 + S + d)
    rn = lambda *s: torch.randn(*s, generator=g)
    inp = dict(memory=rn(B, S, d), pos=rn(B, S, d),
               Wm=[rn(d, d) / math.sqrt(d) for _ in range(2 * L)], Wp=[rn(d, d) / math.sqrt(d) for _ in range(L)],
               bm=[0.1 * rn(d) for _ in range(2 * L)], bp=[0.1 * rn(d) for _ in range(L)],
               q=[2.0 * rn(B, Lq, H, 2 * dh) for _ in range(L)], go=[rn(B, Lq, d) for _ in range(L)])
    inp = {k: (v.to(dev) if torch.is_tensor(v) else [t.to(dev) for t in v]) for k, v in inp.items()}
    mask = _mask_of(mk, B, S)
    if mask is not None:
        assert not mask.all(1).any()           # no fully masked row
        mask = mask.to(dev)
    inp.update(mask=mask, dims=(B, S, d, H, L, Lq), scale=float(2 * dh) ** -0.5)
    return inp


def _result(L, O, dq, dmem, dpos, dWm, dWp, dbm, dbp, dYn):
    """One flat dict of tensors; the names carry the layer."""
    r = {"dmemory": dmem, "dpos": dpos}
    for l in O:
        r[f"O{l}"], r[f"dq{l}"] = O[l], dq[l]
    for l in range(L):
        r[f"dW_kc{l}"], r[f"dW_v{l}"], r[f"dW_kp{l}"] = dWm[2 * l], dWm[2 * l + 1], dWp[l]
        r[f"db_kc{l}"], r[f"db_v{l}"], r[f"db_kp{l}"] = dbm[2 * l], dbm[2 * l + 1], dbp[l]
    r["_dYnorm"] = dYn            # {name of a k bias: ||dY block||_F}, from the exact run only
    return r


def exact_fp64(inp, layers):
    """softmax(scale q [k_c | k_p]^T + mask) v per layer, loss = sum_l <O_l, go_l>, autograd - all in fp64."""
    B, S, d, H, L, Lq = inp["dims"]
    dh = d // H
    lf = lambda t: t.double().requires_grad_()
    mem, pos = lf(inp["memory"]), lf(inp["pos"])
    Wm, Wp, bm, bp = ([lf(t) for t in inp[k]] for k in ("Wm", "Wp", "bm", "bp"))
    q = {l: lf(inp["q"][l]) for l in layers}
    O, kcs, kps, loss = {}, {}, {}, 0.0
    for l in layers:
        kcs[l], kps[l] = F.linear(mem, Wm[2 * l], bm[2 * l]), F.linear(pos, Wp[l], bp[l])
        v = F.linear(mem, Wm[2 * l + 1], bm[2 * l + 1]).view(B, S, H, dh)
        k = torch.cat([kcs[l].view(B, S, H, dh), kps[l].view(B, S, H, dh)], dim=3)
        s = torch.einsum("bqhd,bkhd->bhqk", q[l] * inp["scale"], k)
        if inp["mask"] is not None:
            s = s.masked_fill(inp["mask"][:, None, None], float("-inf"))
        O[l] = torch.einsum("bhqk,bkhd->bqhd", s.softmax(-1), v).reshape(B, Lq, d)
        loss = loss + (O[l] * inp["go"][l].double()).sum()
    leaves = [mem, pos] + Wm + Wp + bm + bp + [q[l] for l in layers] + [kcs[l] for l in layers] + [kps[l] for l in layers]
    gr = torch.autograd.grad(loss, leaves, allow_unused=True)
    gr = [torch.zeros_like(t) if g is None else g for g, t in zip(gr, leaves)]
    n = len(layers)
    dq = dict(zip(layers, gr[2 + 6 * L:2 + 6 * L + n]))
    dYn = {}
    for i, l in enumerate(layers):
        dYn[f"db_kc{l}"] = gr[2 + 6 * L + n + i].norm().item()
        dYn[f"db_kp{l}"] = gr[2 + 6 * L + 2 * n + i].norm().item()
    return _result(L, {l: O[l].detach() for l in layers}, dq, gr[0], gr[1], gr[2:2 + 2 * L], gr[2 + 2 * L:2 + 3 * L], gr[2 + 3 * L:2 + 5 * L],
                   gr[2 + 5 * L:2 + 6 * L], dYn)


@torch.no_grad()
def rounded_model_fp64(inp, layers):
    """The same operator and its hand-written backward in fp64, with a cast to fp16 / bf16 at every rounding point of the path (module
    docstring).  No project kernel: torch casts and fp64 products only."""
    B, S, d, H, L, Lq = inp["dims"]
    dh, R, sc = d // H, B * S, inp["scale"]
    mem, pos = inp["memory"].double(), inp["pos"].double()
    Wm, Wp, bm, bp = ([t.double() for t in inp[k]] for k in ("Wm", "Wp", "bm", "bp"))
    memh, posh = _r16(mem).view(R, d), _r16(pos).view(R, d)
    dYm = torch.zeros(2 * L, R, d, dtype=torch.float64, device=mem.device)
    dYp = torch.zeros(L, R, d, dtype=torch.float64, device=mem.device)
    O, dq = {}, {}
    for l in layers:
        kc = _r16(memh @ _r16(Wm[2 * l]).t() + bm[2 * l])                      # fp16 operands, fp16 output
        v = _r16(memh @ _r16(Wm[2 * l + 1]).t() + bm[2 * l + 1]).view(B, S, H, dh)
        kp = _r16(posh @ _r16(Wp[l]).t() + bp[l])
        k = torch.cat([kc.view(B, S, H, dh), kp.view(B, S, H, dh)], dim=3)
        qs = inp["q"][l].double() * (sc * LOG2E)
        qf, qb = _r16(qs), _rb(qs)                                             # Qf (fp16), Q16 (bf16)
        s2 = torch.einsum("bqhd,bkhd->bhqk", qf, k)                            # log2 domain
        if inp["mask"] is not None:
            s2 = s2.masked_fill(inp["mask"][:, None, None], float("-inf"))
        p = torch.exp2(s2 - s2.amax(-1, keepdim=True))
        lsum = p.sum(-1, keepdim=True)
        o = torch.einsum("bhqk,bkhd->bqhd", _r16(p), v) / lsum.permute(0, 2, 1, 3)
        O[l] = o.reshape(B, Lq, d)
        # backward
        dO = inp["go"][l].double().view(B, Lq, H, dh)
        D = (dO * o).sum(-1).permute(0, 2, 1)[..., None]                       # [B,H,Lq,1] = rowsum(dO . O), unrounded operands
        P = p / lsum
        dOb = _rb(dO)
        dp = torch.einsum("bqhd,bkhd->bhqk", dOb, _rb(v))                      # dOf . Vf
        dsb = _rb(P * (dp - D))
        dq[l] = sc * torch.einsum("bhqk,bkhd->bqhd", dsb, _rb(k))              # dS K16
        dk = LN2 * torch.einsum("bhqk,bqhd->bkhd", dsb, qb)                    # dS^T Q16
        dv = torch.einsum("bhqk,bqhd->bkhd", _rb(P), dOb)                      # P^T dO16
        dYm[2 * l] = _rb(dk[..., :dh]).reshape(R, d)                           # the scatter rounds to bf16
        dYm[2 * l + 1] = _rb(dv).reshape(R, d)
        dYp[l] = _rb(dk[..., dh:]).reshape(R, d)
    memb, posb = _rb(mem).view(R, d), _rb(pos).view(R, d)
    dWm = [dYm[i].t() @ memb for i in range(2 * L)]
    dWp = [dYp[i].t() @ posb for i in range(L)]
    dmem = sum(dYm[i] @ _rb(Wm[i]) for i in range(2 * L)).view(B, S, d)
    dpos = sum(dYp[i] @ _rb(Wp[i]) for i in range(L)).view(B, S, d)
    return _result(L, O, dq, dmem, dpos, dWm, dWp, [dYm[i].sum(0) for i in range(2 * L)], [dYp[i].sum(0) for i in range(L)], None)


# (M, N, K): K = 64 is ONE stage of the fp16 kernel's ring (d_model 64, the dh = 8 case below); rows and columns off the 128 / 160 tiles
@pytest.mark.parametrize("M,N,K_", [(2080, 384, 64), (2049, 64, 128), (2100, 768, 384), (8400, 3072, 256)])
def test_memory_side_projection_gemm_fp16(dev, M, N, K_):
    """The stacked projection GEMM of _MemorySideKV (spe_gemm_bf16nt, act bits 8 + 9: fp16 operands, fp16 output) element by element
    against fp64 on the same fp16 operands.  Bound per element: the fp16 rounding of the output is half an ulp (2^-11 relative) and
    the fp32 accumulation (<= 384 products of O(1) terms: ~1e-6) can move a sum across a rounding boundary - one ulp, 2^-10 |ref|, plus
    2e-5 absolute for that accumulation error where |ref| is small."""
    from spe_amd import kernels as K
    g = torch.Generator().manual_seed(M + N + K_)
    x = torch.randn(M, K_, generator=g).to(dev)
    W = (torch.randn(N, K_, generator=g) / math.sqrt(K_)).to(dev)
    b = (0.1 * torch.randn(N, generator=g)).to(dev)
    xh, Wh = K.cvt_f16(x), K.cvt_f16(W)
    assert torch.equal(xh, x.half()) and torch.equal(Wh, W.half())
    y = _filled((M, N), torch.float16, dev)
    K.gemm16(xh, Wh, y, M, N, K_, K_, K_, N, bias=b, act=0x300)
    ref = xh.double() @ Wh.double().t() + b.double()
    err = (y.double() - ref).abs()
    bound = 2.0 ** -10 * ref.abs() + 2e-5
    worst = (err / bound).max().item()
    print(f"KVDIRECT gemm_fp16 {M}x{N}x{K_}: worst |err| / (2^-10 |ref| + 2e-5) = {worst:.3f}, global {rel(y, ref):.3e}")
    assert worst <= 1.0, f"{int((err > bound).sum())} of {M * N} elements beyond one fp16 ulp"


def _leaves(inp, memory_side=True, queries=True):
    from_ = lambda t, rg: t.clone().requires_grad_(rg)
    mem, pos = from_(inp["memory"], memory_side), from_(inp["pos"], memory_side)
    Wm, Wp, bm, bp = ([from_(t, memory_side) for t in inp[k]] for k in ("Wm", "Wp", "bm", "bp"))
    q = [from_(t, queries) for t in inp["q"]]
    return mem, pos, Wm, Wp, bm, bp, q


def run_nodes(inp, layers, prec, p_drop=0.0, memory_side=True):
    """ops.memory_side_kv + ops.cross_attention_kv on fresh fp32 leaves; -> the same flat dict as the fp64 functions."""
    from spe_amd import kernels as K
    from spe_amd import ops
    K.set_precision(prec)
    B, S, d, H, L, Lq = inp["dims"]
    mem, pos, Wm, Wp, bm, bp, q = _leaves(inp, memory_side)
    assert ops.memory_side_kv_ok(mem, Wm, Wp, H), "the case would not reach the fragment path"
    holder, toks = ops.memory_side_kv(mem, pos, H, Wm, Wp, bm, bp)
    assert holder.K16 is not None and holder.Vf is not None
    O = {l: ops.cross_attention_kv(q[l], toks[l], holder, l, inp["mask"], inp["scale"], p_drop) for l in layers}
    assert all(o.grad_fn.__class__.__name__.startswith("_CrossAttentionKV") for o in O.values())
    loss = sum((O[l] * inp["go"][l]).sum() for l in layers)
    if not memory_side:
        dq = torch.autograd.grad(loss, [q[l] for l in layers])
        return {**{f"O{l}": O[l].detach() for l in layers}, **{f"dq{l}": g for l, g in zip(layers, dq)}}
    leaves = [mem, pos] + Wm + Wp + bm + bp + [q[l] for l in layers]
    gr = torch.autograd.grad(loss, leaves)
    assert holder.dYm is None and holder.dYp is None and not holder.written        # the step's buffers are released
    return _result(L, {l: O[l].detach() for l in layers}, dict(zip(layers, gr[2 + 6 * L:])), gr[0], gr[1], gr[2:2 + 2 * L],
                   gr[2 + 2 * L:2 + 3 * L], gr[2 + 3 * L:2 + 5 * L], gr[2 + 5 * L:2 + 6 * L], None)


def _rows(name, t):
    """[rows, row length]: rows are tokens (dmemory, dpos), queries (O, dq: all heads of a query), weight rows; a bias is one row."""
    if name.startswith("dq"):
        return t.reshape(t.shape[0] * t.shape[1], -1)
    return t.reshape(-1, t.shape[-1])


def row_err(name, a, r):
    """max over rows ||a_row - r_row|| / rms over rows ||r_row||: one wrong tile is a row error near 1 however large the tensor is, and rows
    of tiny norm do not blow it up."""
    a2, r2 = _rows(name, a.double()), _rows(name, r.double())
    return ((a2 - r2).norm(dim=1).max() / (r2.norm(dim=1).pow(2).mean().sqrt() + 1e-300)).item()


def errors(name, a, ref, dYnorm):
    """-> (global, per row).  The k-projection bias gradients are exactly zero in exact arithmetic (the rows of dS sum to zero): they are
    measured absolutely, in units of ||dY||_F of their column block."""
    if name in dYnorm:
        e = (a.double() - ref.double()).norm().item() / dYnorm[name]
        return e, e
    return rel(a, ref), row_err(name, a, ref)


_REFS = {}


def references(name, layers, dev):
    """(inputs, exact fp64, rounded model, {tensor: (e_model global, e_model row)}) - computed once per (case, layer set), never modified."""
    key = (name, tuple(layers))
    if key not in _REFS:
        inp = make_inputs(name, dev)
        ex, mo = exact_fp64(inp, layers), rounded_model_fp64(inp, layers)
        used = _used(inp["dims"][4], layers)
        em = {n: errors(n, mo[n], ex[n], ex["_dYnorm"]) for n in used}
        _REFS[key] = (inp, ex, mo, em)
    return _REFS[key]


def _used(L, layers):
    names = ["dmemory", "dpos"]
    for l in layers:
        names += [f"O{l}", f"dq{l}", f"dW_kc{l}", f"dW_v{l}", f"dW_kp{l}", f"db_kc{l}", f"db_v{l}", f"db_kp{l}"]
    return names


def check_bounds(tag, got, ex, em, names):
    """Prints every figure, then asserts err <= 2 e_model + 1e-5 in both metrics and the project's global bounds."""
    bad = []
    for n in names:
        eg, er = errors(n, got[n], ex[n], ex["_dYnorm"])
        mg, mr = em[n]
        print(f"KVDIRECT {tag} {n}: e_model global {mg:.3e} row {mr:.3e} | measured global {eg:.3e} row {er:.3e}")
        if not eg <= 2 * mg + 1e-5:
            bad.append(f"{n}: global {eg:.3e} > 2 * {mg:.3e} + 1e-5")
        if not er <= 2 * mr + 1e-5:
            bad.append(f"{n}: per-row {er:.3e} > 2 * {mr:.3e} + 1e-5")
        if n not in ex["_dYnorm"]:
            tol = TOL["bf16"] if n.startswith("O") else 2 * TOL["bf16"]
            if not eg < tol:
                bad.append(f"{n}: global {eg:.3e} >= {tol:.1e}")
    assert not bad, f"{tag}: " + "; ".join(bad)


def _assert_bitwise(a, b, names):
    for n in names:
        assert torch.equal(a[n], b[n]), f"{n} differs between two identical runs"


@pytest.mark.parametrize("prec", ["bf16s", "bf16"])
@pytest.mark.parametrize("name", list(NODE_CASES))
def test_nodes_against_fp64(dev, name, prec):
    """O_l, dq_l, dmemory, dpos, every dW and db of the two autograd nodes, all layers in the loss; at the masked cases the gradient rows
    of padded tokens are exactly zero; a second run of the same graph gives the same bits."""
    L = NODE_CASES[name][0][4]
    layers = list(range(L))
    inp, ex, mo, em = references(name, layers, dev)
    got = run_nodes(inp, layers, prec)
    names = _used(L, layers)
    again = run_nodes(inp, layers, prec)
    check_bounds(f"{name} {prec}", got, ex, em, names)
    _assert_bitwise(got, again, names)
    if inp["mask"] is not None:
        for n in ("dmemory", "dpos"):
            for r in (ex, mo, got):
                assert not r[n][inp["mask"]].any(), f"{n}: a padded token has a non-zero gradient row"
            assert got[n][~inp["mask"]].abs().sum(-1).min() > 0


@pytest.mark.parametrize("name", ["cfg2_grid", "dh8_520"])
def test_nodes_unused_layers(dev, name):
    """Only layers {0, L-1} in the loss: the memory-side backward zeroes the blocks no cross-attention node wrote (the buffers come
    from torch.empty) - dW / db of the unused layers are exactly 0 and dmemory / dpos still meet their bounds."""
    L = NODE_CASES[name][0][4]
    layers = [0, L - 1]
    inp, ex, mo, em = references(name, layers, dev)
    got = run_nodes(inp, layers, "bf16s")
    check_bounds(f"{name} bf16s layers0,{L - 1}", got, ex, em, _used(L, layers))
    for l in range(1, L - 1):
        for n in (f"dW_kc{l}", f"dW_v{l}", f"dW_kp{l}", f"db_kc{l}", f"db_v{l}", f"db_kp{l}"):
            for r in (ex, mo, got):
                assert not r[n].any(), f"{n}: layer {l} is not in the loss"
    if inp["mask"] is not None:
        assert not got["dmemory"][inp["mask"]].any() and not got["dpos"][inp["mask"]].any()
    _assert_bitwise(got, run_nodes(inp, layers, "bf16s"), _used(L, layers))


def test_nodes_frozen_memory_side(dev):
    """memory, pos and the projections take no gradient, the queries do: the holder still carries K16 / Vf (want_bwd) and dq meets
    the same bound as in the full run."""
    name = "tail_1100"
    layers = list(range(NODE_CASES[name][0][4]))
    inp, ex, mo, em = references(name, layers, dev)
    got = run_nodes(inp, layers, "bf16s", memory_side=False)
    check_bounds(f"{name} bf16s frozen-memory-side", got, ex, em, [n for l in layers for n in (f"O{l}", f"dq{l}")])


def test_nodes_no_grad_forward(dev):
    """Under no_grad the holder has no backward fragments and O has the bits of the grad-mode forward."""
    from spe_amd import ops
    name = "tail_1100"
    inp, ex, mo, em = references(name, list(range(NODE_CASES[name][0][4])), dev)
    H = inp["dims"][3]
    mem, pos, Wm, Wp, bm, bp, q = _leaves(inp)
    holder, toks = ops.memory_side_kv(mem, pos, H, Wm, Wp, bm, bp)
    O1 = ops.cross_attention_kv(q[1], toks[1], holder, 1, inp["mask"], inp["scale"], 0.0)
    with torch.no_grad():
        holder0, toks0 = ops.memory_side_kv(mem, pos, H, Wm, Wp, bm, bp)
        assert holder0.K16 is None and holder0.Vf is None and holder0.Kf is not None
        O0 = ops.cross_attention_kv(q[1], toks0[1], holder0, 1, inp["mask"], inp["scale"], 0.0)
    assert not O0.requires_grad and torch.equal(O0, O1.detach())
    assert rel(O0, ex["O1"]) < TOL["bf16"]


def test_second_node_on_one_layer_is_refused(dev):
    """spe_kv_grad_scatter stores: two cross-attention nodes on one (holder, layer) would lose the first one's key / value gradients, so
    the backward raises."""
    from spe_amd import ops
    name = "tail_1100"
    inp, *_ = references(name, list(range(NODE_CASES[name][0][4])), dev)
    H = inp["dims"][3]
    mem, pos, Wm, Wp, bm, bp, q = _leaves(inp)
    holder, toks = ops.memory_side_kv(mem, pos, H, Wm, Wp, bm, bp)
    O1 = ops.cross_attention_kv(q[0], toks[0], holder, 0, inp["mask"], inp["scale"], 0.0)
    O2 = ops.cross_attention_kv(q[1], toks[0], holder, 0, inp["mask"], inp["scale"], 0.0)
    with pytest.raises(RuntimeError, match="already written in this backward pass"):
        (O1.sum() + O2.sum()).backward()


def test_nodes_dropout_matches_materialising_path(dev):
    """p_drop = 0.1: the fragment path and ops.attention's materialising path draw the same Philox stream (same seed, same first
    offset, same element index), so they agree like test_attention_flash's pair does.  ops.attention gets fp32 keys / values built in
    torch from the same fp16-rounded operands."""
    from spe_amd import kernels as K
    from spe_amd import ops
    name = "tail_1100"
    inp, ex, *_ = references(name, list(range(NODE_CASES[name][0][4])), dev)
    B, S, d, H, L, Lq = inp["dims"]
    dh, l = d // H, 1
    K.manual_seed(77)
    got = run_nodes(inp, [l], "bf16s", p_drop=0.1)
    mem, pos, Wm, Wp, bm, bp, q = _leaves(inp)
    h16 = lambda t: t.half().float()
    proj = lambda x, W, b: h16(F.linear(h16(x), h16(W), b))
    k = torch.cat([proj(mem, Wm[2 * l], bm[2 * l]).view(B, S, H, dh), proj(pos, Wp[l], bp[l]).view(B, S, H, dh)], dim=3)
    v = proj(mem, Wm[2 * l + 1], bm[2 * l + 1]).view(B, S, H, dh)
    old = ops.FLASH_MHA
    try:
        ops.FLASH_MHA = False
        K.manual_seed(77)
        o, _ = ops.attention(q[l], k, v, inp["mask"], scale=inp["scale"], p_drop=0.1, need_map=False)
        assert o.grad_fn.__class__.__name__.startswith("_Attention") and not o.grad_fn.__class__.__name__.startswith("_AttentionFlash")
        leaves = [q[l], mem, pos, Wm[2 * l], Wm[2 * l + 1], Wp[l], bm[2 * l + 1]]
        gr = torch.autograd.grad((o * inp["go"][l]).sum(), leaves)
    finally:
        ops.FLASH_MHA = old
    assert rel(got[f"O{l}"], ex[f"O{l}"]) > 0.05           # dropout took effect: far from the p_drop = 0 result
    pairs = dict(zip([f"dq{l}", "dmemory", "dpos", f"dW_kc{l}", f"dW_v{l}", f"dW_kp{l}", f"db_v{l}"], gr))
    pairs[f"O{l}"] = o
    for n, ref in pairs.items():
        e = rel(got[n], ref)
        print(f"KVDIRECT {name} bf16s dropout0.1 {n}: vs materialising path global {e:.3e}")
        assert e < 2 * TOL["bf16"], n


# ------------------------------------------------------------------------------------------------------------------------------
# Tier 3
# ------------------------------------------------------------------------------------------------------------------------------
def _decoder_case():
    from spe_amd.models.layers import LayerNorm
    from spe_amd.models.transformer import TransformerDecoder, TransformerDecoderLayer
    d, H, NL, Q, R, B, S = 256, 8, 3, 100, 2, 2, 4200
    torch.manual_seed(11)
    dec = TransformerDecoder(TransformerDecoderLayer(d, H, dim_feedforward=256, dropout=0.0), NL, LayerNorm(d), return_intermediate=True, d_model=d)
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for p in dec.parameters():
            if p.dim() > 1:                 # Xavier-uniform, as Transformer._reset_parameters
                p.copy_((2 * torch.rand(p.shape, generator=g) - 1) * math.sqrt(6.0 / (p.shape[0] + p.shape[1])))
            else:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    data = dict(memory=torch.randn(B, S, d, generator=g), pos=torch.randn(B, S, d, generator=g), query_pos=torch.randn(B, R * Q, d, generator=g),
                g_hs=torch.randn(NL, B, R * Q, d, generator=g), g_ref=torch.randn(B, R * Q, 2, generator=g), mask=grid_mask())
    return dec, data, (d, H, NL, Q, R, B, S)


def _ca_params(dec):
    return [(n, p) for n, p in dec.named_parameters() if ".ca_" in n]


def _decoder_oracle_fp64(dec, data, dims):
    """oracle.spe_oracle.decoder in fp64 on the CPU, once per proposal stage (the stages share weights and memory and only the query
    self-attention must not mix them: the product stacks them along the query axis).  The oracle's sine embedding keeps its fp32
    frequency table - the constants the product uses too - and promotes to fp64 with its input; nothing there pins the arithmetic.
    The biases of ca_kcontent_proj / ca_kpos_proj enter as [S, B, d] copies of themselves (the same sums): their gradient is dY, which
    gives the exact bias gradient (its sum over the tokens: zero in exact arithmetic) AND the scale ||dY||_F it is measured in."""
    from oracle import spe_oracle as O
    d, H, NL, Q, R, B, S = dims
    sd = {"transformer.decoder." + n: p.detach().double().requires_grad_(".ca_" in n) for n, p in dec.named_parameters()}
    for n in list(sd):
        if _k_bias(n):
            sd[n] = sd[n].detach().expand(S, B, d).clone().requires_grad_()
    mem, pos = data["memory"].double().requires_grad_(), data["pos"].double().requires_grad_()
    cfg = O.make_cfg(nheads=H, dec_layers=NL)
    hs, refs = [], []
    for r in range(R):
        qp = data["query_pos"][:, r * Q:(r + 1) * Q].double().transpose(0, 1)
        h, ref = O.decoder(mem.transpose(0, 1), data["mask"], pos.transpose(0, 1), qp, sd, cfg)
        hs.append(h)
        refs.append(ref)
    hs, refs = torch.cat(hs, dim=2), torch.cat(refs, dim=1)
    loss = (hs * data["g_hs"].double()).sum() + (refs * data["g_ref"].double()).sum()
    names = [n for n, _ in _ca_params(dec)]
    gr = torch.autograd.grad(loss, [mem, pos] + [sd["transformer.decoder." + n] for n in names])
    out = {"hs": hs.detach(), "ref": refs.detach(), "dmemory": gr[0], "dpos": gr[1]}
    dYnorm = {}
    for n, g in zip(names, gr[2:]):
        if _k_bias(n):
            dYnorm["d " + n], g = g.norm().item(), g.sum((0, 1))
        out["d " + n] = g
    return out, dYnorm


def _k_bias(n):
    return n.endswith("ca_kcontent_proj.bias") or n.endswith("ca_kpos_proj.bias")


def _decoder_run(dec, data, dims, dev, memkv):
    from spe_amd import kernels as K
    from spe_amd import ops
    d, H, NL, Q, R, B, S = dims
    for p in dec.parameters():
        p.grad = None
    mem, pos = data["memory"].to(dev).requires_grad_(), data["pos"].to(dev).requires_grad_()
    qp = data["query_pos"].to(dev)
    old = ops.MEMKV
    try:
        ops.MEMKV = memkv
        K.lib.count_launches(True)
        hs, ref = dec(torch.zeros_like(qp), mem, data["mask"].to(dev), pos, qp, n_stages=R)
        loss = (hs * data["g_hs"].to(dev)).sum() + (ref * data["g_ref"].to(dev)).sum()
        names = [n for n, _ in _ca_params(dec)]
        gr = torch.autograd.grad(loss, [mem, pos] + [p for _, p in _ca_params(dec)])
    finally:
        counts = K.lib.count_launches(False)
        ops.MEMKV = old
    out = {"hs": hs.detach(), "ref": ref.detach(), "dmemory": gr[0], "dpos": gr[1]}
    out.update({"d " + n: g for n, g in zip(names, gr[2:])})
    return out, counts


def test_decoder_against_fp64_oracle(dev):
    """TransformerDecoder (d 256, 8 heads, 3 layers, 2 stages of 100 queries, memory 2 x (50 x 84) with the 2-D padding mask) against the
    fp64 oracle: hs, reference points, gradients of memory, pos and all ca_* parameters.  The bound rule of Tier 2 with the error of the
    MEMKV = False path (split-bf16 fp32 keys, per-layer pack: another memory-side code path) in the place of e_model; both paths
    within 2 TOL["bf16"] of fp64 and of each other.  The first layer's k_content + k_pos is carried by the query side in the fragment
    path only, so a slip there separates the two runs."""
    dec, data, dims = _decoder_case()
    ex, dYnorm = _decoder_oracle_fp64(dec, data, dims)
    ex = {n: t.to(dev) for n, t in ex.items()}
    dec.to(dev)
    a, ca = _decoder_run(dec, data, dims, dev, memkv=True)
    b, cb = _decoder_run(dec, data, dims, dev, memkv=False)
    assert ca.get("spe_kv_frags", 0) == 1 and ca.get("spe_kv_grad_scatter", 0) == dims[2], ca
    assert "spe_kv_frags" not in cb and "spe_kv_grad_scatter" not in cb
    bad = []
    for n in ex:
        ea, eb = errors(n, a[n], ex[n], dYnorm), errors(n, b[n], ex[n], dYnorm)
        ab = errors(n, a[n], b[n], dYnorm)[0]
        print(f"KVDIRECT decoder bf16s {n}: MEMKV=False global {eb[0]:.3e} row {eb[1]:.3e} | MEMKV global {ea[0]:.3e} row {ea[1]:.3e} | "
              f"between the paths {ab:.3e}")
        for what, e, w in (("global", ea[0], eb[0]), ("per-row", ea[1], eb[1])):
            if not e <= 2 * w + 1e-5:
                bad.append(f"{n}: {what} {e:.3e} > 2 * {w:.3e} + 1e-5")
        if n in dYnorm:
            continue            # exactly zero in exact arithmetic: measured in units of ||dY||_F, which the relative bound below does not apply to
        for what, e in (("MEMKV vs fp64", ea[0]), ("MEMKV=False vs fp64", eb[0]), ("between the paths", ab)):
            if not e < 2 * TOL["bf16"]:
                bad.append(f"{n}: {what} {e:.3e} >= {2 * TOL['bf16']:.1e}")
    assert not bad, "; ".join(bad)
