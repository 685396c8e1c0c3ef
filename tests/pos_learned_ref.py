"""Restatement of the learned position embedding (reference models/position_encoding.py:60-85) and of its adjoint in plain indexing, in
the dtype of its inputs (fp64 in the kernel tests).  Pinned by tests/test_pos_learned_cpu.py against the reference's own `pos` tensor and against
torch autograd; the GPU kernel tests lean on it."""
import torch


def forward(col, row, B, h, w):
    """col, row [50, npf] -> [B, h, w, 2 * npf]: channels c < npf = col[x, c], channels npf + c = row[y, c]."""
    npf = col.shape[1]
    out = col.new_empty((B, h, w, 2 * npf))
    out[..., :npf] = col[:w].view(1, 1, w, npf)
    out[..., npf:] = row[:h].view(1, h, 1, npf)
    return out


def adjoint(g, h, w, rows=50):
    """g [B, h, w, 2 * npf] (or [B, h * w, 2 * npf]) -> (d_col, d_row), both [rows, npf]; table rows the grid does not reach are zero."""
    B, npf = g.shape[0], g.shape[-1] // 2
    g = g.reshape(B, h, w, 2 * npf)
    d_col, d_row = g.new_zeros((rows, npf)), g.new_zeros((rows, npf))
    d_col[:w] = g[..., :npf].sum((0, 1))
    d_row[:h] = g[..., npf:].sum((0, 2))
    return d_col, d_row
