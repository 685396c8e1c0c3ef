"""The flash multi-head attention kernels (csrc/mha_flash.hip: spe_mha_plan / spe_mha_fwd / spe_mha_bwd) and the fragment pack that
feeds them, at every tile, chunk, mask and head-dim edge of tests/mha_cases.py, element-wise against the fp64 restatement and the
bounds of tests/mha_ref.py (operands on a grid fp16 and bf16 both hold, so only the kernels' internal roundings remain; the
assertion is err <= 2 x bound).  The kernels are called on fragments built by tests/kv_layout.py, through kernels.mha_fwd / mha_bwd
and - for the store-confinement checks - through the same C entry points with NaN-filled buffers the test owns.

Every test prints one line `MHAEDGE <case> <output>=<worst err / bound> ...` (recorded in profiles/mha_edges.txt)."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_layout as KV  # noqa: E402
import mha_cases as C  # noqa: E402
import mha_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [C.case_id(c) for c in C.GPU_CASES]
SPARE = 192                      # canary elements behind every buffer
SEED, OFFSET = 0x5DEECE66D, 48   # the Philox stream of the dropout cases
_prepared = {}


def _bits(a):
    return a.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _frags(op):
    """The eight fragment stacks from the operands (already on the 16-bit grid: the conversions are exact)."""
    h16 = lambda x: x.half().contiguous().view(torch.int16)
    b16 = lambda x: x.bfloat16().contiguous().view(torch.int16)
    q, k, v, do = op["q"], op["k"], op["v"], op["do"]
    return dict(Qf=KV.pack32(h16(q)).contiguous(), Kf=KV.pack32(h16(k)).contiguous(), V16=KV.pack16(h16(v)).contiguous(),
                Q16=KV.pack16(b16(q)).contiguous(), K16=KV.pack16(b16(k)).contiguous(), Vf=KV.pack32(b16(v)).contiguous(),
                dOf=KV.pack32(b16(do)).contiguous(), dO16=KV.pack16(b16(do)).contiguous())


def _keep_matrix(case, dev):
    """What the materialising path draws from (SEED, OFFSET): spe_softmax_fwd's dropout over a [B*H*Lq, ld4] array."""
    from spe_amd import kernels as K
    B, H, Lq, Lk, p = case[0], case[1], case[2], case[3], case[8]
    if p == 0:
        return None
    ld = K.pad4(Lk)
    S = torch.zeros((B, H, Lq, ld), device=dev, dtype=torch.float32)
    _, Pd = K.softmax_fwd(S, None, B, H, Lq, Lk, ld, p, SEED, OFFSET)
    return Pd[..., :Lk] > 0


def _prep(case, dev):
    """Operands, fragments, mask and the fp64 reference of a case - computed once, shared by the tests, never modified."""
    key = C.case_id(case)
    if key not in _prepared:
        op = R.operands(case, dev)
        keep = _keep_matrix(case, dev)
        ref = R.reference(op, case[8], keep, case[9])
        mask_u8 = None if op["mask"] is None else op["mask"].to(torch.uint8).contiguous()
        _prepared[key] = (op, _frags(op), mask_u8, keep, ref)
    return _prepared[key]


def _nan(n, dev):
    return torch.full((n,), float("nan"), device=dev, dtype=torch.float32)


def _untouched(buf, n):
    return bool(torch.isnan(buf[n:]).all())


def _fwd_owned(fr, mask_u8, case, dev, nch=None, p=None):
    """spe_mha_fwd into NaN-filled buffers with SPARE elements behind each.  -> O [B,Lq,H,dv], LSE [B,H,Lq], keep words, report."""
    from spe_amd import kernels as K
    B, H, Lq, Lk, dk, dv = case[:6]
    p = case[8] if p is None else p
    nch = case[9] if nch is None else nch
    ntq, ntk, dvt = (Lq + 15) // 16, (Lk + 15) // 16, (dv + 15) // 16
    items = B * H * ntq * nch
    n_op, n_ml, n_o, n_l, n_k = items * dvt * 256, items * 32, B * Lq * H * dv, B * H * Lq, B * H * ntq * ntk * 4
    opart, ml, O, lse = _nan(n_op + SPARE, dev), _nan(n_ml + SPARE, dev), _nan(n_o + SPARE, dev), _nan(n_l + SPARE, dev)
    keep = torch.full((n_k + SPARE,), 0x5A5A5A5A5A5A5A5A, device=dev, dtype=torch.int64) if p > 0 else None
    K._call("spe_mha_fwd", K._p(fr["Qf"]), K._p(fr["Kf"]), K._p(fr["V16"]), K._p(mask_u8), K._p(opart), K._p(ml), K._p(O), K._p(lse),
            K._p(keep), B, H, Lq, Lk, dk, dv, nch, float(p), SEED, OFFSET, K._st())
    torch.cuda.synchronize()
    confined = all(_untouched(b, n) for b, n in ((opart, n_op), (ml, n_ml), (O, n_o), (lse, n_l)))
    if keep is not None:
        confined = confined and bool((keep[n_k:] == 0x5A5A5A5A5A5A5A5A).all())
        keep = keep[:n_k]
    return O[:n_o].view(B, Lq, H, dv), lse[:n_l].view(B, H, Lq), keep, confined


def _bwd_owned(fr, mask_u8, lse, D, keep, case, dev, scale, nch=None, live=None):
    """spe_mha_bwd into NaN-filled dq, dk, dv and slab buffers; the slabs are added by kernels.colsum as kernels.mha_bwd does.
    live: the batches whose slab elements have to be finite (all of them by default)."""
    from spe_amd import kernels as K
    B, H, Lq, Lk, dk, dv = case[:6]
    p = case[8]
    nch = case[9] if nch is None else nch
    n_q, n_k, n_v = B * Lq * H * dk, B * Lk * H * dk, B * Lk * H * dv
    dq, dk_, dv_ = _nan(n_q + SPARE, dev), _nan(n_k + SPARE, dev), _nan(n_v + SPARE, dev)
    ws = _nan(nch * n_q + SPARE, dev) if nch > 1 else None
    K._call("spe_mha_bwd", K._p(fr["Qf"]), K._p(fr["Kf"]), K._p(fr["Vf"]), K._p(fr["dOf"]), K._p(fr["K16"]), K._p(fr["Q16"]),
            K._p(fr["dO16"]), K._p(mask_u8), K._p(lse), K._p(D), K._p(keep), K._p(dq), K._p(ws), K._p(dk_), K._p(dv_), B, H, Lq, Lk,
            dk, dv, nch, float(scale), float(p), K._st())
    torch.cuda.synchronize()
    confined = _untouched(dk_, n_k) and _untouched(dv_, n_v)
    if ws is not None:
        # with slabs the kernel leaves dq alone altogether; every slab element of a real query row is written
        slabs = ws[:nch * n_q].view(nch, B, Lq * H * dk)
        confined = (confined and bool(torch.isnan(dq).all()) and _untouched(ws, nch * n_q)
                    and bool(torch.isfinite(slabs if live is None else slabs[:, live]).all()))
        out = torch.empty(n_q, device=dev, dtype=torch.float32)
        K.colsum(ws[:nch * n_q].view(nch, n_q), out=out, accumulate=False)
        dq = out
    else:
        confined = confined and _untouched(dq, n_q)
    return dq[:n_q].view(B, Lq, H, dk), dk_[:n_k].view(B, Lk, H, dk), dv_[:n_v].view(B, Lk, H, dv), confined


def _lse_d(ref):
    """LSE and D as handed to the backward: the reference's, rounded to fp32."""
    return ref["LSE"].float().contiguous(), ref["D"].float().contiguous()


def _decode_keep(words, B, H, Lq, Lk):
    """keep words [B*H*ntq*ntk*4] -> bool [B,H,Lq,Lk]: word r, bit lane <-> query lane & 15, key 4 (lane >> 4) + r."""
    ntq, ntk = (Lq + 15) // 16, (Lk + 15) // 16
    w = words.view(B, H, ntq, ntk, 4, 1)
    bit = (w >> torch.arange(64, device=words.device)) & 1                       # [B,H,ntq,ntk,r,lane]
    bit = bit.view(B, H, ntq, ntk, 4, 4, 16).permute(0, 1, 2, 6, 3, 5, 4)        # [B,H,ntq,ql,ntk,g,r]
    return bit.reshape(B, H, ntq * 16, ntk * 16)[:, :, :Lq, :Lk] != 0


def _report(case, tag, ratios):
    print("MHAEDGE", C.case_id(case), tag, " ".join("%s=%.3f" % kv for kv in ratios.items()))


# ---- pack ---------------------------------------------------------------------------------------------------------------------
PACKS = [("rec", 2, 37, 3, 48), ("rec", 1, 16, 1, 8), ("rec", 2, 100, 4, 64), ("unit-dk96", 2, 37, 3, 96), ("unit-dh10", 2, 37, 3, 10),
         ("unit-offset", 2, 37, 3, 48), ("fused-rec", 2, 37, 3, 48), ("fused-unit", 2, 37, 3, 10), ("unit-dh6", 1, 5, 2, 6)]


@pytest.mark.parametrize("how,B,N,H,dh", PACKS, ids=["%s-%dx%dx%dx%d" % p for p in PACKS])
def test_pack_bit_exact(dev, how, B, N, H, dh):
    """spe_attn_pack_multi kinds 2 and 1, fp16 and bf16, against kv_layout.pack32 / pack16 of the rounded tensor, bit for bit - zeros
    in the padding rows and dims included - on the wave-per-record path and on the per-unit path (dk = 96, dh % 4 != 0, a base
    pointer 4 bytes past a 16-byte boundary, slices of a fused [B, L, 3, H, d] tensor)."""
    from spe_amd import kernels as K
    g = torch.Generator().manual_seed(N + dh)
    if how.startswith("fused"):
        x = torch.randn(B, N, 3, H, dh, generator=g).to(dev)[:, :, 1]
        assert not x.is_contiguous()
    elif how == "unit-offset":
        x = torch.randn(B * N * H * dh + 4, generator=g).to(dev)[1:1 + B * N * H * dh].view(B, N, H, dh)
        assert x.data_ptr() % 16 == 4
    else:
        x = torch.randn(B, N, H, dh, generator=g).to(dev)
    rec = how.endswith("rec") and x.data_ptr() % 16 == 0 and all(s % 4 == 0 for s in x.stride()[:3])
    assert rec == (C.pack_path(dh, dh) == "pack_rec" and how != "unit-offset")
    scale = 0.375
    outs = K.attn_pack_multi([(x, scale, 322 + K.F16), (x, scale, 322), (x, scale, 16 + K.F16), (x, scale, 16)])
    y = x * torch.tensor(scale, device=dev)
    h16, b16 = y.half().contiguous().view(torch.int16), y.bfloat16().contiguous().view(torch.int16)
    want = [KV.pack32(h16), KV.pack32(b16), KV.pack16(h16), KV.pack16(b16)]
    for o, w, n in zip(outs, want, ("kind2-fp16", "kind2-bf16", "kind1-fp16", "kind1-bf16")):
        assert o.shape == w.shape, (n, o.shape, w.shape)
        assert torch.equal(o.view(torch.int16), w), n
    print("MHAEDGE pack-%s-%dx%dx%dx%d" % (how, B, N, H, dh), "path=%s" % ("record" if rec else "per-unit"), "bits=equal")


# ---- forward --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.GPU_CASES, ids=IDS)
def test_forward(dev, case):
    """O and LSE element-wise under the bounds, stores confined to the outputs, the same bits from a second call; with one key left
    per batch O is that key's v and LSE its score, bit for bit; with dropout the keep words decode to the materialising path's draw."""
    from spe_amd import kernels as K
    B, H, Lq, Lk, dk, dv, mfam, sfam, p, nch = case
    op, fr, mask_u8, keep, ref = _prep(case, dev)
    assert K.mha_plan(B, H, Lq, Lk) == nch
    live = ~ref["dead"]
    O, lse, words, confined = _fwd_owned(fr, mask_u8, case, dev)
    r = dict(O=R.ratio(O, ref["O"], ref["bO"], live), LSE=R.ratio(lse, ref["LSE"], ref["bLSE"], live))
    _report(case, "fwd", r)
    assert confined, "a store left O / LSE / the partials / the keep words"
    assert bool(torch.isfinite(O[live]).all()) and bool(torch.isfinite(lse[live]).all())
    assert r["O"] <= 2.0 and r["LSE"] <= 2.0, r
    O2, lse2, words2 = K.mha_fwd(fr["Qf"], fr["Kf"], fr["V16"], mask_u8, B, H, Lq, Lk, dk, dv, nch, p, SEED, OFFSET)
    assert _same_bits(O2.view(B, Lq, H, dv)[live], O[live]) and _same_bits(lse2[live], lse[live])
    if mfam == "one_key":
        for b in range(B):
            kb = C.one_key(case, b)
            assert _same_bits(O[b], op["v"][b, kb].float().expand(Lq, H, dv)), b
            s = torch.einsum("qhd,hd->hq", op["q"][b], op["k"][b, kb])
            assert _same_bits(lse[b], s.float()), b
    if p > 0:
        assert torch.equal(words, words2)
        got = _decode_keep(words, B, H, Lq, Lk)
        assert torch.equal(got, keep), "keep words differ from the materialising path's draw of the same (seed, offset)"
        n = got.numel()
        share = float(got.double().mean())
        assert abs(share - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n), (share, n)


RAGGED = [c for c in C.GPU_CASES if (c[2] % 16 or c[3] % 16) and c[6] != "all_padded_batch"][::4]


@pytest.mark.parametrize("case", RAGGED, ids=[C.case_id(c) for c in RAGGED])
def test_poisoned_padding(dev, case):
    """Finite garbage (+-3) in the fragment rows of keys >= Lk and queries >= Lq: every result keeps its bits (no NaN or inf here:
    0 x NaN inside an MFMA is NaN by contract, and the pack guarantees zeros)."""
    B, H, Lq, Lk, dk, dv, mfam, sfam, p, nch = case
    op, fr, mask_u8, keep, ref = _prep(case, dev)
    poisoned = {}
    for name, f in fr.items():
        L, D = (Lq, dk) if name in ("Qf", "Q16") else (Lq, dv) if name in ("dOf", "dO16") else (Lk, dk) if name in ("Kf", "K16") else (Lk, dv)
        wide = name.endswith("f")
        tok, _ = (KV._index32 if wide else KV._index16)(L, D, dev)
        fp16 = name in ("Qf", "Kf", "V16")
        three = torch.tensor([3.0, -3.0], device=dev).to(torch.float16 if fp16 else torch.bfloat16).view(torch.int16)
        g = f.clone()
        pad = (tok >= L).expand(g.shape)
        sign = (torch.arange(g.numel(), device=dev).view(g.shape) % 2)
        g[pad] = three[sign[pad]]
        poisoned[name] = g
        assert (L % 16 == 0) == bool((g == f).all())
    lse32, D32 = _lse_d(ref)
    res = []
    for frags in (fr, poisoned):
        O, lse, words, ok1 = _fwd_owned(frags, mask_u8, case, dev)
        dq, dk_, dv_, ok2 = _bwd_owned(frags, mask_u8, lse32, D32, words, case, dev, op["scale"])
        assert ok1 and ok2
        res.append((O, lse, dq, dk_, dv_))
    same = {n: _same_bits(a, b) for n, a, b in zip(("O", "LSE", "dq", "dk", "dv"), *res)}
    _report(case, "poison", {n: 0.0 if s else float("inf") for n, s in same.items()})
    assert all(same.values()), same


# ---- backward -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.GPU_CASES, ids=IDS)
def test_backward(dev, case):
    """dq, dk, dv element-wise under the bounds with LSE and D from the reference, exact zeros in the dk / dv rows of padded keys,
    stores confined (dq slabs included), the same bits from a second call (slab sum included)."""
    from spe_amd import kernels as K
    B, H, Lq, Lk, dk, dv, mfam, sfam, p, nch = case
    op, fr, mask_u8, keep, ref = _prep(case, dev)
    live = ~ref["dead"]
    lse32, D32 = _lse_d(ref)
    words = K.mha_fwd(fr["Qf"], fr["Kf"], fr["V16"], mask_u8, B, H, Lq, Lk, dk, dv, nch, p, SEED, OFFSET)[2] if p > 0 else None
    dq, dk_, dv_, confined = _bwd_owned(fr, mask_u8, lse32, D32, words, case, dev, op["scale"])
    r = {n: R.ratio(x, ref[n], ref["b" + n], live) for n, x in (("dq", dq), ("dk", dk_), ("dv", dv_))}
    # printed only: the same errors over the bounds with one bf16 rounding at its worst case 2^-8 (mha_ref: ub)
    rw = {n + "w": R.ratio(x, ref[n], ref["b" + n + "w"], live) for n, x in (("dq", dq), ("dk", dk_), ("dv", dv_))}
    _report(case, "bwd", dict(r, **rw))
    assert confined, "a store left dq / dk / dv / the dq slabs"
    assert all(bool(torch.isfinite(x[live]).all()) for x in (dq, dk_, dv_))
    assert all(x <= 2.0 for x in r.values()), r
    if op["mask"] is not None:
        padded = op["mask"] & live[:, None]
        assert bool((dk_[padded] == 0).all()) and bool((dv_[padded] == 0).all())
    dq2, dk2, dv2 = K.mha_bwd(fr["Qf"], fr["Kf"], fr["Vf"], fr["dOf"], fr["K16"], fr["Q16"], fr["dO16"], mask_u8, lse32, D32, words,
                              B, H, Lq, Lk, dk, dv, nch, op["scale"], p)
    assert _same_bits(dq2[live], dq[live]) and _same_bits(dk2[live], dk_[live]) and _same_bits(dv2[live], dv_[live])


ONE_CHUNK = [(3, 5, 33, 272, 48, 48, "chunk_mid", "normal", 0, 4), (2, 4, 17, 272, 10, 6, "scatter", "normal", 0, 4),
             (2, 4, 17, 336, 96, 48, "chunk_mid", "normal", 0, 5)]
assert all(c in C.GPU_CASES for c in ONE_CHUNK)


@pytest.mark.parametrize("case", ONE_CHUNK, ids=[C.case_id(c) for c in ONE_CHUNK])
def test_backward_slabs_against_one_chunk(dev, case):
    """The same operands with nch forced to 1 in the backward (mha_fill accepts a smaller count there): the single-chunk kernel and
    the slab sum both meet the bound, and dk / dv - which do not depend on the chunking - keep their bits."""
    B, H, Lq, Lk, dk, dv, mfam, sfam, p, nch = case
    op, fr, mask_u8, keep, ref = _prep(case, dev)
    live = ~ref["dead"]
    lse32, D32 = _lse_d(ref)
    many = _bwd_owned(fr, mask_u8, lse32, D32, None, case, dev, op["scale"])
    one = _bwd_owned(fr, mask_u8, lse32, D32, None, case, dev, op["scale"], nch=1)
    assert many[3] and one[3]
    r = dict(dq_slabs=R.ratio(many[0], ref["dq"], ref["bdq"], live), dq_one=R.ratio(one[0], ref["dq"], ref["bdq"], live))
    _report(case, "bwd-nch1", r)
    assert all(x <= 2.0 for x in r.values()), r
    assert _same_bits(many[1], one[1]) and _same_bits(many[2], one[2])


# ---- a batch with every key padded ------------------------------------------------------------------------------------------------
ALL_PADDED = [c for c in C.GPU_CASES if c[6] == "all_padded_batch"]


@pytest.mark.parametrize("case", ALL_PADDED, ids=[C.case_id(c) for c in ALL_PADDED])
def test_all_padded_batch(dev, case):
    """The other batches are bit-identical to a run of those batches alone; the padded batch's outputs are what the materialising
    path gives for it (softmax over an empty set: NaN, as torch), NaN positions included."""
    from spe_amd import kernels as K
    from spe_amd import ops
    B, H, Lq, Lk, dk, dv, mfam, sfam, p, nch = case
    op, fr, mask_u8, keep, ref = _prep(case, dev)
    live = ~ref["dead"]
    nl = int(live.sum())
    assert nl == B - 1 and K.mha_plan(nl, H, Lq, Lk) == nch
    lse32, D32 = _lse_d(ref)
    D32 = D32.clone()
    D32[~live] = float("nan")                     # what rowsum(dO . O) is for that batch in a training step
    O, lse, _, ok1 = _fwd_owned(fr, mask_u8, case, dev)
    assert bool((lse[~live] == float("-inf")).all()) and bool(torch.isnan(O[~live]).all())
    dq, dk_, dv_, ok2 = _bwd_owned(fr, mask_u8, lse32, D32, None, case, dev, op["scale"], live=live)
    sub = {n: (t[live].contiguous() if torch.is_tensor(t) else t) for n, t in op.items()}
    fs = _frags(sub)
    cs = (nl,) + case[1:]
    Os, lses, _, ok3 = _fwd_owned(fs, mask_u8[live].contiguous(), cs, dev)
    dqs, dks, dvs, ok4 = _bwd_owned(fs, mask_u8[live].contiguous(), lse32[live].contiguous(), D32[live].contiguous(), None, cs, dev, op["scale"])
    assert ok1 and ok2 and ok3 and ok4
    same = {n: _same_bits(a[live], b) for n, a, b in (("O", O, Os), ("LSE", lse, lses), ("dq", dq, dqs), ("dk", dk_, dks), ("dv", dv_, dvs))}
    # through ops.attention: flash against the materialising path
    res = {}
    old = ops.FLASH_MHA, ops.FLASH_MIN_KEYS
    try:
        ops.FLASH_MIN_KEYS = 1
        for flash in (True, False):
            ops.FLASH_MHA = flash
            q, k, v = (op[n].float().requires_grad_() for n in ("q", "k", "v"))
            o, _ = ops.attention(q, k, v, op["mask"], scale=R.LN2, p_drop=0.0)
            assert o.grad_fn.__class__.__name__.startswith("_AttentionFlash" if flash else "_AttentionBackward")
            res[flash] = (o.detach().view(B, Lq, H, dv),) + torch.autograd.grad(o, (q, k, v), op["do"].float().reshape(o.shape))
    finally:
        ops.FLASH_MHA, ops.FLASH_MIN_KEYS = old
    d = C.ALL_PADDED_BATCH
    nanmap = {n: torch.equal(torch.isnan(a[d]), torch.isnan(b[d])) for n, a, b in zip(("O", "dq", "dk", "dv"), res[True], res[False])}
    close = {n: torch.allclose(a[d], b[d], rtol=0, atol=1e-2, equal_nan=True) for n, a, b in zip(("O", "dq", "dk", "dv"), res[True], res[False])}
    _report(case, "all-padded", {n: 0.0 if s else float("inf") for n, s in same.items()})
    print("MHAEDGE", C.case_id(case), "all-padded-vs-materialising nan-positions", nanmap, "values", close,
          "flash nan share", {n: float(torch.isnan(a[d]).float().mean()) for n, a in zip(("O", "dq", "dk", "dv"), res[True])},
          "materialising nan share", {n: float(torch.isnan(a[d]).float().mean()) for n, a in zip(("O", "dq", "dk", "dv"), res[False])})
    assert all(same.values()), same
    assert all(nanmap.values()) and all(close.values()), (nanmap, close)
    for a, b in zip(res[True], res[False]):              # and the live batches agree between the two paths as ever
        assert float((a[live] - b[live]).norm() / b[live].norm()) < 2e-2


# ---- through ops.attention --------------------------------------------------------------------------------------------------------
def _qkv(dev, Lk, dk=16, dv=16, Lq=8, B=1, H=2, seed=0):
    g = torch.Generator().manual_seed(seed + Lk)
    mk = lambda *s: torch.randn(*s, generator=g).to(dev).requires_grad_()
    return mk(B, Lq, H, dk), mk(B, Lk, H, dk), mk(B, Lk, H, dv)


def _path(o):
    n = o.grad_fn.__class__.__name__
    return "flash" if n.startswith("_AttentionFlash") else "materialising" if n.startswith("_Attention") else n


def test_dispatch(dev):
    """Which path ops.attention takes, by grad_fn class."""
    from spe_amd import kernels as K
    from spe_amd import ops
    assert ops.FLASH_MHA and ops.FLASH_MIN_KEYS == 512
    got = {}
    got["Lk=511"] = _path(ops.attention(*_qkv(dev, 511), scale=0.25)[0])
    got["Lk=512"] = _path(ops.attention(*_qkv(dev, 512), scale=0.25)[0])
    got["need_map"] = _path(ops.attention(*_qkv(dev, 512), scale=0.25, need_map=True)[0])
    K.set_precision("bf16x3")
    try:
        got["bf16x3"] = _path(ops.attention(*_qkv(dev, 512), scale=0.25)[0])
    finally:
        K.set_precision("bf16s")
    got["dk=97"] = _path(ops.attention(*_qkv(dev, 512, dk=97), scale=0.25)[0])
    got["dv=65"] = _path(ops.attention(*_qkv(dev, 512, dv=65), scale=0.25)[0])
    got["dk=96,dv=64"] = _path(ops.attention(*_qkv(dev, 512, dk=96, dv=64), scale=0.25)[0])
    got["dk=10,dv=6"] = _path(ops.attention(*_qkv(dev, 512, dk=10, dv=6), scale=0.25)[0])
    print("MHAEDGE dispatch", got)
    assert got == {"Lk=511": "materialising", "Lk=512": "flash", "need_map": "materialising", "bf16x3": "materialising",
                   "dk=97": "materialising", "dv=65": "materialising", "dk=96,dv=64": "flash", "dk=10,dv=6": "flash"}
    # a last stride other than 1 is sent to the materialising path, which states that it does not take it
    q, k, v = _qkv(dev, 512)
    qt = q.detach().transpose(2, 3).contiguous().transpose(2, 3)
    assert qt.shape == q.shape and qt.stride(3) != 1
    with pytest.raises(AssertionError, match="last dim must be contiguous"):
        ops.attention(qt, k, v, scale=0.25)


def test_fused_slices_and_no_grad(dev):
    """q, k, v as strided slices of one fused [B, L, 3, H, d] tensor give the bits of contiguous copies; the forward under no_grad
    (no backward fragments packed) gives the bits of the training forward."""
    from spe_amd import ops
    B, L, H, d = 2, 515, 3, 40
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(B, L, 3, H, d, generator=g).to(dev)
    mask = torch.zeros(B, L, dtype=torch.bool, device=dev)
    mask[1, 100:300] = True
    go = torch.randn(B, L, H * d, generator=g).to(dev)
    res = []
    for contiguous in (False, True):
        parts = [qkv[:, :, i] for i in range(3)]
        assert not parts[0].is_contiguous()
        if contiguous:
            parts = [t.contiguous() for t in parts]
        q, k, v = (t.detach().requires_grad_() for t in parts)
        o, _ = ops.attention(q, k, v, mask, scale=d ** -0.5)
        assert _path(o) == "flash"
        res.append((o.detach(),) + torch.autograd.grad(o, (q, k, v), go))
    same = {n: _same_bits(a, b) for n, a, b in zip(("O", "dq", "dk", "dv"), *res)}
    with torch.no_grad():
        o_ng, _ = ops.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], mask, scale=d ** -0.5)
    same["O_no_grad"] = _same_bits(o_ng, res[0][0])
    print("MHAEDGE fused-slices", same)
    assert all(same.values()), same


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(dev):
    """spe_mha_fwd: -2 for a head dim over the limit or dropout without keep words, -5 for a chunk count that mha_fill would change
    (the check the entry point makes: it compares with its own chunking, not with spe_mha_plan), 0 and untouched buffers for an
    empty problem."""
    from spe_amd import kernels as K
    from spe_amd import lib
    B, H, Lq, Lk, dk, dv = 1, 2, 17, 144, 32, 16
    case = (B, H, Lq, Lk, dk, dv, "none", "normal", 0, 2)
    op, fr, mask_u8, keep, ref = _prep(case, dev)
    bufs = [_nan(1 << 16, dev) for _ in range(4)]

    def call(B=B, H=H, Lq=Lq, Lk=Lk, dk=dk, dv=dv, nch=2, p=0.0):
        K._call("spe_mha_fwd", K._p(fr["Qf"]), K._p(fr["Kf"]), K._p(fr["V16"]), None, *[K._p(b) for b in bufs], None, B, H, Lq, Lk, dk, dv,
                nch, float(p), 0, 0, K._st())

    # nine key tiles: the plan says 2 chunks (5 + 4); 7 chunks would be 5 of 2 tiles, 10 are more than there are tiles
    for kw, status in ((dict(dk=97), -2), (dict(dv=65), -2), (dict(p=0.1), -2), (dict(nch=0), -5), (dict(nch=7), -5), (dict(nch=10), -5)):
        with pytest.raises(lib.SpeLibraryError, match="status %d$" % status):
            call(**kw)
    for kw in (dict(B=0), dict(H=0), dict(Lq=0), dict(Lk=0)):
        call(**kw)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(b).all()) for b in bufs)
    call()                                              # and the accepted call does write
    torch.cuda.synchronize()
    assert bool(torch.isfinite(bufs[2][:B * Lq * H * dv]).all())
    # a chunk count that is consistent with the tiles (3 x 3) but not the plan's is taken as it is - the caller sizes the
    # partials with the count it passes - and gives the same operator
    O3, lse3, _, ok = _fwd_owned(fr, None, case, dev, nch=3)
    r = dict(O=R.ratio(O3, ref["O"], ref["bO"]), LSE=R.ratio(lse3, ref["LSE"], ref["bLSE"]))
    assert ok and r["O"] <= 2.0 and r["LSE"] <= 2.0, r
    print("MHAEDGE refusals dk=97:-2 dv=65:-2 p>0-without-words:-2 nch-not-a-chunking:-5 empty:0-untouched nch=3-of-9-tiles", r)


def test_bwd_refuses_chunks_without_slabs(dev):
    """spe_mha_bwd: -2 and nothing launched for more than one key chunk without dq slabs (chunks never add into one dq); one chunk
    without slabs is accepted and overwrites dq directly."""
    from spe_amd import kernels as K
    from spe_amd import lib
    B, H, Lq, Lk, dk, dv = 1, 2, 17, 144, 32, 16
    case = (B, H, Lq, Lk, dk, dv, "none", "normal", 0, 2)
    op, fr, mask_u8, keep, ref = _prep(case, dev)
    lse, D = _lse_d(ref)
    n_q, n_k, n_v = B * Lq * H * dk, B * Lk * H * dk, B * Lk * H * dv
    dq, dk_, dv_ = _nan(n_q + SPARE, dev), _nan(n_k + SPARE, dev), _nan(n_v + SPARE, dev)

    def call(nch):
        K._call("spe_mha_bwd", K._p(fr["Qf"]), K._p(fr["Kf"]), K._p(fr["Vf"]), K._p(fr["dOf"]), K._p(fr["K16"]), K._p(fr["Q16"]),
                K._p(fr["dO16"]), None, K._p(lse), K._p(D), None, K._p(dq), None, K._p(dk_), K._p(dv_), B, H, Lq, Lk, dk, dv, nch,
                float(op["scale"]), 0.0, K._st())
        torch.cuda.synchronize()

    with pytest.raises(lib.SpeLibraryError, match="status -2$"):
        call(2)
    assert all(bool(torch.isnan(b).all()) for b in (dq, dk_, dv_))
    call(1)
    assert all(bool(torch.isfinite(b[:n]).all()) and _untouched(b, n) for b, n in ((dq, n_q), (dk_, n_k), (dv_, n_v)))
    r = R.ratio(dq[:n_q].view(B, Lq, H, dk), ref["dq"], ref["bdq"])
    print("MHAEDGE bwd-refusal nch=2-without-slabs:-2-untouched nch=1-without-slabs:dq-direct dq=%.3f" % r)
    assert r <= 2.0, r
