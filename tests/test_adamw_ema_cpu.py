"""The weight-EMA contract of FlatAdamW without a GPU: the fp32 restatement (adamw_ema_ref.py) against the all-fp64 recurrence, the
warm-up table, and the declarations of the new entries."""
import struct
from fractions import Fraction

import numpy as np
import pytest

import adamw_ema_ref as R
from adamw_ema_cases import TRIPLES, WEIGHT_BITS

T = 50


@pytest.mark.parametrize("decay,warmup", [(0.9998, True), (0.9998, False), (0.9, True), (0.5, False), (0.0, True)])
@pytest.mark.parametrize("scale", [1.0, 1e-3, 1e4])
def test_fp32_restatement_stays_within_the_rounding_bound_of_the_fp64_recurrence(decay, warmup, scale):
    """|e32 - e64| <= 6 T 2^-24 M after T steps, M the largest |p| or |e| of the run: three roundings per step, each at most 2^-24 of a
    magnitude at most 2M (p - e, w * (p - e), e + w * (p - e)); an earlier error is carried on with the factor 1 - w, 0 <= 1 - w < 1, so
    the errors add up at worst and never grow."""
    rng = np.random.default_rng(7)
    n = 4096
    e32 = (rng.standard_normal(n) * scale).astype(np.float32)
    e64 = e32.astype(np.float64)
    M = float(np.abs(e32).max())
    for t in range(1, T + 1):
        p = (rng.standard_normal(n) * scale).astype(np.float32)
        w = R.ema_weight(decay, warmup, t)
        assert 0.0 < float(w) <= 1.0
        e32 = R.ema_step32(e32, p, w)
        e64 = R.ema_step64(e64, p, w)
        M = max(M, float(np.abs(p).max()), float(np.abs(e32).max()), float(np.abs(e64).max()))
    err = float(np.abs(e32.astype(np.float64) - e64).max())
    bound = 6 * T * 2.0 ** -24 * M
    print(f"decay {decay} warmup {warmup} scale {scale}: max |e32 - e64| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def _f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]          # struct rounds a Python float (fp64) to fp32 to nearest even


@pytest.mark.parametrize("decay,warmup,t", TRIPLES)
def test_warmup_table(decay, warmup, t):
    """The restatement's w against plain Python floats (IEEE fp64) rounded by struct, against the bit patterns written down in the
    cases file, and - where the warm-up decides - against the exact rational 1 - (1 + t) / (10 + t) to within fp32 rounding."""
    w = R.ema_weight(decay, warmup, t)
    assert w.dtype == np.float32
    d = min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay
    assert int(w.view(np.uint32)) == _f32_bits(1.0 - d)
    if (decay, warmup, t) in WEIGHT_BITS:
        assert int(w.view(np.uint32)) == WEIGHT_BITS[(decay, warmup, t)]
    exact_warm = Fraction(1 + t, 10 + t)
    if warmup and exact_warm < Fraction(decay):
        exact = 1 - exact_warm
        assert abs(Fraction(float(w)) - exact) <= exact * Fraction(1, 2 ** 24) + Fraction(1, 2 ** 52)
    else:
        assert int(w.view(np.uint32)) == _f32_bits(1.0 - decay)


def test_warmup_crossover_and_saturation():
    """The weight falls with t while the warm-up is active, and is the plain 1 - decay from the crossover on."""
    ws = [float(R.ema_weight(0.9998, True, t)) for t in (1, 5, 100, 44989)]
    assert all(a > b for a, b in zip(ws, ws[1:]))
    flat = R.ema_weight(0.9998, False, 1)
    assert ws[-1] > float(flat)
    for t in (44990, 44991, 10 ** 6):
        assert R.ema_weight(0.9998, True, t) == flat
    assert float(R.ema_weight(0.9, True, 79)) > float(R.ema_weight(0.9, True, 80)) == float(R.ema_weight(0.9, False, 80))


def test_decay_zero_tracks_the_parameter():
    rng = np.random.default_rng(3)
    e, p = rng.standard_normal(100).astype(np.float32), rng.standard_normal(100).astype(np.float32)
    out = R.ema_step32(e, p, R.ema_weight(0.0, True, 1))
    assert np.allclose(out, p, rtol=0, atol=2.0 ** -22 * float(np.abs(np.concatenate([e, p])).max()))


def test_header_declares_the_new_entries():
    import ctypes
    from spe_amd import lib
    sig = lib.PROTOS["spe_adamw_flat_ema"]
    names = [n for _, n in sig]
    assert names[:5] == ["p", "g", "m", "v", "e"] and names[-5:] == ["guard", "decay", "warmup", "t", "stream"]
    assert dict((n, t) for t, n in sig)["decay"] is ctypes.c_double and dict((n, t) for t, n in sig)["t"] is ctypes.c_long
    assert [n for _, n in lib.PROTOS["spe_swap_flat"]] == ["a", "b", "n", "stream"]
    # the existing entries keep their signatures: the EMA entry is spe_adamw_flat's argument list with e, guard, decay, warmup and t added
    flat = [n for _, n in lib.PROTOS["spe_adamw_flat"]]
    assert [n for n in names if n not in ("e", "guard", "decay", "warmup", "t")] == flat
    assert len(lib.PROTOS["spe_adamw_flat_guarded"]) == 15
