"""Plain-torch restatement of the two MFMA operand fragment layouts of the flash MHA kernels (include/spe_hip.h: spe_kv_frags,
spe_attn_pack_multi kinds 2 and 1), as index arithmetic on a token-major tensor x [..., S, H, D]:

  pack32: out[..., h, tile, st, lane, j] = x[..., tile*16 + (lane & 15), h, st*32 + (lane >> 4)*8 + j]      (32-wide steps)
  pack16: out[..., h, tile, dt, lane, j] = x[..., tile*16 + 4*(lane >> 4) + j, h, dt*16 + (lane & 15)]      (16-wide tiles)

and of the record of the backbone score kernels (spe_attn_pack, spe_attn_pack_multi kind 32): pack32t, 32-wide steps plus one 16-wide
tail step (see _index32t),

with zeros where the token is >= S or the dim is >= D.  Elements are moved, never converted: any dtype (the tests pass raw 16-bit
patterns as int16).  No project code is imported here."""
import torch


def _index32(S, D, device):
    nt, steps = (S + 15) // 16, (D + 31) // 32
    tile = torch.arange(nt, device=device).view(nt, 1, 1, 1)
    st = torch.arange(steps, device=device).view(1, steps, 1, 1)
    lane = torch.arange(64, device=device).view(1, 1, 64, 1)
    j = torch.arange(8, device=device).view(1, 1, 1, 8)
    tok = (tile * 16 + (lane & 15)).expand(nt, steps, 64, 8)
    dim = (st * 32 + (lane >> 4) * 8 + j).expand(nt, steps, 64, 8)
    return tok, dim


def _index16(S, D, device):
    nt, DT = (S + 15) // 16, (D + 15) // 16
    tile = torch.arange(nt, device=device).view(nt, 1, 1, 1)
    dt = torch.arange(DT, device=device).view(1, DT, 1, 1)
    lane = torch.arange(64, device=device).view(1, 1, 64, 1)
    j = torch.arange(4, device=device).view(1, 1, 1, 4)
    tok = (tile * 16 + 4 * (lane >> 4) + j).expand(nt, DT, 64, 4)
    dim = (dt * 16 + (lane & 15)).expand(nt, DT, 64, 4)
    return tok, dim


def _pack(x, index):
    S, D = x.shape[-3], x.shape[-1]
    tok, dim = index(S, D, x.device)
    valid = (tok < S) & (dim < D)
    xh = x.movedim(-2, -3)                                              # [..., H, S, D]
    out = xh[..., tok.clamp(max=S - 1), dim.clamp(max=D - 1)]          # [..., H, nt, steps, 64, width]
    return torch.where(valid, out, torch.zeros((), dtype=x.dtype, device=x.device))


def _unpack(frag, S, D, index):
    """-> (x [..., S, H, D], pad): pad = the fragment elements that belong to no (token, dim) of x."""
    tok, dim = index(S, D, frag.device)
    assert frag.shape[-4:] == tok.shape, (frag.shape, tok.shape)
    valid = (tok < S) & (dim < D)
    xh = torch.zeros(frag.shape[:-4] + (S, D), dtype=frag.dtype, device=frag.device)
    xh[..., tok[valid], dim[valid]] = frag[..., valid]
    return xh.movedim(-3, -2), frag[..., ~valid]


def pack32(x):
    return _pack(x, _index32)


def pack16(x):
    return _pack(x, _index16)


def unpack32(frag, S, D):
    return _unpack(frag, S, D, _index32)


def unpack16(frag, S, D):
    return _unpack(frag, S, D, _index16)


def frag_geom32t(D):
    """(full, tail) of the kind-32 record: `full` 32-wide steps, then one 16-wide tail step when D % 32 is in 1 .. 16 (csrc/attn_pack.h:
    frag_geom - a remainder of 17 .. 31 dims takes a whole 32-wide step instead)."""
    rem = D % 32
    return D // 32 + (1 if rem > 16 else 0), 1 if 0 < rem <= 16 else 0


def record_elems32t(D):
    full, tail = frag_geom32t(D)
    return full * 512 + tail * 256


def _index32t(S, D, device):
    """Kind 32 (spe_attn_pack, spe_attn_pack_multi kind 32), restated from attn_pack_unit_t of csrc/attn_pack.h: the 8-byte unit u of a
    record holds, for u < full * 128, step st = u >> 7, lane = (u & 127) >> 1 and dims st*32 + (lane >> 4)*8 + (u & 1)*4 + j - the first
    `full` steps of pack32 - and beyond that lane = u - full*128 with dims full*32 + (lane >> 4)*4 + j; token tile*16 + (lane & 15) in both:
      out[.., tile, st*512 + lane*8 + j]   = x[.., tile*16 + (lane & 15), h, st*32 + (lane >> 4)*8 + j]      (j < 8, st < full)
      out[.., tile, full*512 + lane*4 + j] = x[.., tile*16 + (lane & 15), h, full*32 + (lane >> 4)*4 + j]    (j < 4, the tail step)"""
    nt = (S + 15) // 16
    full, tail = frag_geom32t(D)
    e = torch.arange(full * 512 + tail * 256, device=device)
    in_full = e < full * 512
    st, lane_f, j_f = e // 512, (e % 512) // 8, e % 8
    t = (e - full * 512).clamp(min=0)
    lane_t, j_t = t // 4, t % 4
    lane = torch.where(in_full, lane_f, lane_t)
    dim = torch.where(in_full, st * 32 + (lane_f >> 4) * 8 + j_f, full * 32 + (lane_t >> 4) * 4 + j_t)
    tile = torch.arange(nt, device=device).view(nt, 1)
    tok = tile * 16 + (lane & 15).view(1, -1)
    return tok, dim.view(1, -1).expand(nt, -1)


def pack32t(x):
    """x [..., S, H, D] -> kind-32 records [..., H, nt, record_elems32t(D)], zeros where the token is >= S or the dim is >= D."""
    S, D = x.shape[-3], x.shape[-1]
    tok, dim = _index32t(S, D, x.device)
    valid = (tok < S) & (dim < D)
    xh = x.movedim(-2, -3)
    out = xh[..., tok.clamp(max=S - 1), dim.clamp(max=D - 1)]
    return torch.where(valid, out, torch.zeros((), dtype=x.dtype, device=x.device))


def unpack32t(frag, S, D):
    """-> (x [..., S, H, D], pad): pad = the record elements that belong to no (token, dim) of x."""
    tok, dim = _index32t(S, D, frag.device)
    assert frag.shape[-2:] == tok.shape, (frag.shape, tok.shape)
    valid = (tok < S) & (dim < D)
    xh = torch.zeros(frag.shape[:-2] + (S, D), dtype=frag.dtype, device=frag.device)
    xh[..., tok[valid], dim[valid]] = frag[..., valid]
    return xh.movedim(-3, -2), frag[..., ~valid]


# the Tier-1 shapes (L, B, S, H, dh) of tests/test_decoder_kv_gpu.py; the last one is cfg2 (25 248 records: every wave of
# kv_frag_kernel's capped grid takes a second record)
FRAG_CASES = [(1, 1, 16, 1, 8), (1, 1, 5, 3, 40), (3, 1, 523, 4, 24), (2, 3, 777, 8, 48), (1, 2, 2049, 2, 64), (2, 2, 1100, 8, 32),
              (6, 2, 4200, 8, 32)]


def expected_frags(ym, yp, L, B, S, H, dh):
    """The four fragment stacks of spe_kv_frags as raw int16 patterns, from the fp16 GEMM outputs ym [B*S, >= 2 L d] (column block
    2l = k_content of layer l, 2l + 1 = v) and yp [B*S, >= L d] (block l = k_pos): Kf / V16 carry the fp16 patterns, K16 / Vf the
    bf16 roundings of the same values with keys and values exchanged between the two layouts."""
    d = H * dh
    m = ym[:, :2 * L * d].reshape(B, S, L, 2, H, dh)
    p = yp[:, :L * d].reshape(B, S, L, H, dh)
    k = torch.cat([m[:, :, :, 0], p], dim=-1).permute(2, 0, 1, 3, 4)              # [L, B, S, H, 2 dh] = [k_content | k_pos]
    v = m[:, :, :, 1].permute(2, 0, 1, 3, 4)                                       # [L, B, S, H, dh]
    bits = lambda t: t.contiguous().view(torch.int16)
    kb, vb = k.float().to(torch.bfloat16), v.float().to(torch.bfloat16)
    return pack32(bits(k)), pack16(bits(v)), pack16(bits(kb)), pack32(bits(vb)), k, v
