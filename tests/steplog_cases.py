"""Shapes and sequences of the step-ledger tests (tests/test_steplog_cpu.py, tests/test_steplog_gpu.py), and the helpers that turn a
[M, 5] table (rows: K unscaled, K scaled, loss, E extras) into the reference's named meters."""
import os

import numpy as np
import torch

import steplog_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FMTS = {"lr": "{value:.6f}", "class_error": "{value:.2f}"}
WINDOWS = {"lr": 1, "class_error": 1}

# the kernels' edges: one key, a wave and one more / less, the limit; no, one and the most host scalars; step counts around the
# reference's window (20), around the ring's depth (64) and two wraps (130)
KS = (1, 2, 63, 64, 65, 255, 256)
ES = (0, 1, 8)
STEPS = (1, 2, 20, 21, 63, 64, 65, 130)
WINS = (1, 2, 19, 20, 21, 64)


def load_golden(name):
    return torch.load(os.path.join(HERE, "golden", name + ".pt"), weights_only=False)


def golden_step(g_keys, st):
    """-> (loss_dict of 0-dim fp32 tensors, weight_dict, lr) of one recorded step."""
    return {k: st["values"][j].clone() for j, k in enumerate(g_keys)}, dict(st["weight_dict"]), st["lr"]


def sequence(K, E, steps, seed=0):
    """A run: mask [K], per step (values fp32 [K], weights fp32 [K], extras [E]).  Contents chosen for the edges: ties (values drawn
    from a small set under key 0, an all-equal window under key 1 when K > 1), +0.0 / -0.0, denormals, a key that changes sign, zero
    weights, a weight that is no short binary fraction, a weight change half way, keys outside the mask."""
    rng = np.random.default_rng([K, E, steps, seed])
    mask = rng.random(K) < 0.8
    mask[0] = True
    if K > 2:
        mask[2] = False
    w0 = rng.choice(np.float32([0.0, 1.0, 2.0, 5.0, 0.3]), K).astype(np.float32)
    w1 = np.where(rng.random(K) < 0.5, w0, np.float32(0.7)).astype(np.float32)
    scale = (10.0 ** rng.uniform(-6, 3, K)).astype(np.float32)
    run = []
    for s in range(steps):
        v = (scale * rng.uniform(0.5, 1.5, K)).astype(np.float32)
        v[0] = np.float32([0.25, 0.5, 0.75][int(rng.integers(0, 3))])
        if K > 1:
            v[1] = np.float32(3.5)                                  # an all-equal window
        if K > 3:
            v[3] = np.float32([0.0, -0.0][s % 2])                   # signed zeros
        if K > 4:
            v[4] = np.float32(1e-42) * np.float32(1 + s % 3)        # denormals
        if K > 5:
            v[5] = -v[5] if s % 3 == 0 else v[5]
        w = (w0 if s < steps // 2 else w1) * mask
        run.append((v, w.astype(np.float32), [1e-4 / (1 + s // 7) * (j + 1) for j in range(E)]))
    return mask, run


def windows_for(K, E, seed=0):
    """One window per table row, cycling through WINS (so even and odd counts and the limits all occur for every kind of row)."""
    return [WINS[(i + seed) % len(WINS)] for i in range(2 * K + 1 + E)]


def named(table, keys, mask, enames, alias=("class_error",), sort_keys=False):
    """{meter name: {five}} from a [M, 5] table; an alias meter shows its key's newest value (window 1)."""
    K = len(keys)
    out = {}
    idx = sorted(range(K), key=lambda i: keys[i]) if sort_keys else list(range(K))
    rows = [("loss", 2 * K)] + [(keys[i], K + i) for i in idx if mask[i]] + [(keys[i] + "_unscaled", i) for i in idx] + \
           [(e, 2 * K + 1 + j) for j, e in enumerate(enames)]
    for name, r in rows:
        out[name] = dict(zip(R.FIELDS, (float(x) for x in table[r])))
    for a in alias:
        if a in keys and not mask[keys.index(a)]:
            t = table[keys.index(a)]
            out[a] = {"median": float(np.float32(t[4])), "avg": float(np.float32(t[4])), "global_avg": float(t[2]), "max": float(t[4]),
                      "value": float(t[4])}
    return out


def render(meters, order, fmts=FMTS, delimiter="  "):
    return delimiter.join("{}: {}".format(n, fmts.get(n, R.DEFAULT_FMT).format(**meters[n])) for n in order)


def same_float(a, b):
    return R.same_bits(np.float64([a]), np.float64([b]))
