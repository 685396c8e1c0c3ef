"""The weight-EMA contract of FlatAdamW(..., ema_decay=d) (spe_adamw_flat_ema, include/spe_hip.h) restated in numpy.

    d = min(decay, (1 + t) / (10 + t)) if warmup else decay        fp64, t the 1-based count of applied steps
    w = float32(1 - d)                                             rounded once
    e' = e + w * (p' - e)                                          three float32 operations, each rounded, no fused multiply-add

ema_step64 is the same recurrence with every operation in fp64 (on the contract's w, which IS a float32 number): the yardstick the
fp32 restatement is bounded against in test_adamw_ema_cpu.py."""
import numpy as np


def ema_weight(decay, warmup, t):
    """w as a numpy float32."""
    d = np.float64(decay)
    if warmup:
        t = np.float64(t)
        d = min(d, (np.float64(1.0) + t) / (np.float64(10.0) + t))
    return np.float32(np.float64(1.0) - d)


def ema_step32(e, p, w):
    """One update of float32 arrays; numpy rounds every elementwise float32 operation on its own."""
    e, p, w = np.asarray(e, np.float32), np.asarray(p, np.float32), np.float32(w)
    d = p - e
    s = w * d
    out = e + s
    assert out.dtype == np.float32
    return out


def ema_step64(e, p, w):
    e, p = np.asarray(e, np.float64), np.asarray(p, np.float64)
    return e + np.float64(w) * (p - e)


def ema_run32(e0, ps, decay, warmup, t0=1):
    """The EMA after the parameter sequence ps (one entry per applied step, the first being step t0), starting from e0."""
    e = np.asarray(e0, np.float32).copy()
    for k, p in enumerate(ps):
        e = ema_step32(e, p, ema_weight(decay, warmup, t0 + k))
    return e
