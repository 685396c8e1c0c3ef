"""Plain-torch restatement of the two MFMA operand fragment layouts of the flash MHA kernels (include/spe_hip.h: spe_kv_frags,
spe_attn_pack_multi kinds 2 and 1), as index arithmetic on a token-major tensor x [..., S, H, D]:

  pack32: out[..., h, tile, st, lane, j] = x[..., tile*16 + (lane & 15), h, st*32 + (lane >> 4)*8 + j]      (32-wide steps)
  pack16: out[..., h, tile, dt, lane, j] = x[..., tile*16 + 4*(lane >> 4) + j, h, dt*16 + (lane & 15)]      (16-wide tiles)

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
