"""tests/kv_layout.py on the CPU: the layout restatement the GPU test of spe_kv_frags compares against is a bijection between the
(token, dim) elements and their fragment slots, and every other slot is zero - at the shapes the GPU test uses."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import kv_layout as kl  # noqa: E402


@pytest.mark.parametrize("L,B,S,H,dh", kl.FRAG_CASES)
def test_pack_unpack_identity_and_zero_padding(L, B, S, H, dh):
    if L * B * S * H * dh > 1 << 22:           # the cfg2 stack is L copies of one layout: one layer checks the same index arithmetic
        L = 1
    g = torch.Generator().manual_seed(S * 131 + dh)
    for D in (dh, 2 * dh):
        # non-zero everywhere, so that a zero in a fragment can only be padding
        x = torch.randint(1, 32767, (L, B, S, H, D), generator=g, dtype=torch.int16)
        for pack, unpack, width, span in ((kl.pack32, kl.unpack32, 8, 32), (kl.pack16, kl.unpack16, 4, 16)):
            f = pack(x)
            assert f.shape == (L, B, H, (S + 15) // 16, (D + span - 1) // span, 64, width)
            back, pad = unpack(f, S, D)
            assert torch.equal(back, x)
            assert pad.numel() == f.numel() - x.numel() and not pad.any()
            assert int((f != 0).sum()) == x.numel()


def test_layout_formulas_by_hand():
    """A few elements spelled out from the header's formulas, independent of the index helpers."""
    S, H, D = 21, 2, 40
    x = torch.arange(1, S * H * D + 1, dtype=torch.int32).view(S, H, D)
    f32, f16 = kl.pack32(x), kl.pack16(x)
    for h, tile, st, lane, j in [(0, 0, 0, 0, 0), (1, 1, 1, 4, 7), (1, 0, 1, 63, 0), (0, 1, 0, 37, 3), (1, 1, 0, 5, 2)]:
        tok, dim = tile * 16 + (lane & 15), st * 32 + (lane >> 4) * 8 + j
        assert int(f32[h, tile, st, lane, j]) == (int(x[tok, h, dim]) if tok < S and dim < D else 0)
    for h, tile, dt, lane, j in [(0, 0, 0, 0, 0), (1, 1, 2, 4, 1), (1, 0, 2, 63, 0), (0, 1, 0, 21, 3), (1, 1, 1, 16, 0)]:
        tok, dim = tile * 16 + 4 * (lane >> 4) + j, dt * 16 + (lane & 15)
        assert int(f16[h, tile, dt, lane, j]) == (int(x[tok, h, dim]) if tok < S and dim < D else 0)


DH32T = (8, 16, 17, 24, 32, 33, 40, 48, 49, 64)
N32T = (1, 15, 16, 17, 100)


@pytest.mark.parametrize("dh", DH32T)
def test_pack32t_identity_and_zero_padding(dh):
    """The kind-32 record (32-wide steps + one 16-wide tail step): a bijection between the (token, dim) elements and their slots, zeros in
    every other slot, at every head dim class of frag_geom and token counts around the 16-row tile."""
    B, H = 2, 3
    full, tail = kl.frag_geom32t(dh)
    assert (full, tail) == {8: (0, 1), 16: (0, 1), 17: (1, 0), 24: (1, 0), 32: (1, 0), 33: (1, 1), 40: (1, 1), 48: (1, 1), 49: (2, 0), 64: (2, 0)}[dh]
    for N in N32T:
        g = torch.Generator().manual_seed(N * 131 + dh)
        x = torch.randint(1, 32767, (B, N, H, dh), generator=g, dtype=torch.int16)
        f = kl.pack32t(x)
        assert f.shape == (B, H, (N + 15) // 16, full * 512 + tail * 256)
        back, pad = kl.unpack32t(f, N, dh)
        assert torch.equal(back, x)
        assert pad.numel() == f.numel() - x.numel() and not pad.any()
        assert int((f != 0).sum()) == x.numel()
        # the full steps are those of pack32
        p32 = kl.pack32(x)
        assert torch.equal(f[..., :full * 512], p32[:, :, :, :full].reshape(B, H, (N + 15) // 16, full * 512))


@pytest.mark.parametrize("dh", DH32T)
def test_pack32t_record_size_is_the_librarys(dh):
    from spe_amd import kernels as K
    assert kl.record_elems32t(dh) == K.frag_record_elems(dh)


def test_pack32t_formula_by_hand():
    """Single elements spelled out from attn_pack_unit_t (8-byte unit u of a record -> lane, first dim), independent of _index32t."""
    S, H, D = 21, 2, 40                                  # one full step + the tail step
    x = torch.arange(1, S * H * D + 1, dtype=torch.int32).view(S, H, D)
    f = kl.pack32t(x)
    full = 1
    for h, tile, u, j in [(0, 0, 0, 0), (1, 1, 127, 3), (0, 1, 77, 2), (1, 0, 128, 0), (0, 0, 128 + 17, 1), (1, 1, 128 + 40, 3), (0, 1, 191, 0)]:
        if u < full * 128:
            st, w = u >> 7, u & 127
            ln = w >> 1
            d0 = st * 32 + (ln >> 4) * 8 + (w & 1) * 4
        else:
            ln = u - full * 128
            d0 = full * 32 + (ln >> 4) * 4
        tok, dim = tile * 16 + (ln & 15), d0 + j
        assert int(f[h, tile, u * 4 + j]) == (int(x[tok, h, dim]) if tok < S and dim < D else 0), (h, tile, u, j)


def test_expected_frags_sources():
    """expected_frags reads k_content from block 2l of ym, v from block 2l + 1, k_pos from block l of yp, and honours wider rows."""
    L, B, S, H, dh = 2, 1, 3, 2, 8
    d = H * dh
    ym = torch.zeros(B * S, 2 * L * d + 8, dtype=torch.float16)
    yp = torch.zeros(B * S, L * d + 16, dtype=torch.float16)
    for blk in range(2 * L):
        ym[:, blk * d:(blk + 1) * d] = 1 + blk
    for blk in range(L):
        yp[:, blk * d:(blk + 1) * d] = 10 + blk
    ym[:, 2 * L * d:] = 99
    yp[:, L * d:] = 99
    *_, k, v = kl.expected_frags(ym, yp, L, B, S, H, dh)
    for l in range(L):
        assert (k[l, ..., :dh] == 1 + 2 * l).all() and (k[l, ..., dh:] == 10 + l).all() and (v[l] == 2 + 2 * l).all()
