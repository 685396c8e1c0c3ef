"""tests/rowsum_ref.py on the CPU: its restatements against torch autograd of the plain formulas in fp64, and every bound against fp32
torch evaluations of the same quantity summed in several orders (forward, reverse, pairwise, the chunked order of a kernel) - a correct
fp32 evaluation alone must stay inside every bound before a kernel is asked to."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowsum_ref as rs  # noqa: E402


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def sum_forward(x):
    acc = torch.zeros(x.shape[1], dtype=torch.float32)
    for r in range(x.shape[0]):
        acc = acc + x[r]
    return acc


def sum_reverse(x):
    return sum_forward(x.flip(0))


def sum_pairwise(x):
    while x.shape[0] > 1:
        if x.shape[0] & 1:
            x = torch.cat([x, torch.zeros(1, x.shape[1])])
        x = x[0::2] + x[1::2]
    return x[0]


def sum_chunked(x, lanes, members):
    """The order of a kernel: thread (member, lane) adds rows lane + lanes (member + members k), the lanes in order, the members in order."""
    R = x.shape[0]
    tot = torch.zeros(x.shape[1])
    for m in range(members):
        part = torch.zeros(x.shape[1])
        for ln in range(lanes):
            idx = list(range(m * lanes + ln, R, members * lanes))
            part = part + (sum_forward(x[idx]) if idx else torch.zeros(x.shape[1]))
        tot = tot + part
    return tot


def test_chains():
    assert [rs.tree(m) for m in (1, 2, 16, 17, 256, 257)] == [0, 2, 16, 18, 32, 33]
    assert rs.chain("colsum_wide", 64, 0) == 64 and rs.chain("colsum_tall4", 16448, 257) == 4 + 16 + 33 + 1
    assert rs.chain("colsum", 16640, 64) == 65 + 3 + 20 + 1 and rs.chain("lsres_bwd_rows", 2049, 128) == 2 + 16 + 24 + 1
    assert rs.chain("lsres_bwd16<2>", 16385, 256, tiles=257) == 8 + 16 + 32 + 1
    assert rs.chain("lsres_bwd16<2>", 129, 3, tiles=3, deferred=True) == 4 + 16 + 17 + 1
    assert rs.n_add("colsum", 1, 1, False) == 0 and rs.n_add("colsum", 1, 1, True) == 1 and rs.n_add("colsum_tall4", 3, 1, False) == 2
    for R in (1, 5, 100, 5000):
        for k, m in (("colsum_wide", 0), ("colsum_tall4", 3), ("colsum", 17), ("lsres_bwd", 300)):
            assert rs.n_add(k, R, m, True) <= R


@pytest.mark.parametrize("R,C", [(1, 7), (3, 5), (300, 9), (4097, 3)])
def test_colsum_bound_holds_for_fp32_sums(R, C):
    g = _gen(R + C)
    x = torch.randn(R, C, generator=g) * 3 + 1
    out0 = torch.randn(C, generator=g)
    ref, mag = rs.colsum(x)
    assert torch.equal(ref, x.double().sum(0))
    # each order against the chain of that order (forward / reverse: R; pairwise: ceil(log2 R); chunked: the kernel's table)
    orders = {"forward": (sum_forward(x), R), "reverse": (sum_reverse(x), R), "pairwise": (sum_pairwise(x), max(R - 1, 0).bit_length()),
              "chunk4x2": (sum_chunked(x, 4, 2), rs.chain("colsum", R, 2) - 1)}
    for name, (got, ch) in orders.items():
        n = max(min(ch, R - 1), 0)
        assert rs.worst_ratio(got.double() - ref, rs.sum_bound(n, mag)) <= 1.0, name
        assert R < 100 or rs.rel(got, ref) < rs.REL_COLSUM, name
    ref2, mag2 = rs.colsum(x, out0)
    got2 = out0 + sum_chunked(x, 4, 2)
    assert rs.worst_ratio(got2.double() - ref2, rs.sum_bound(rs.n_add("colsum", R, 2, True), mag2)) <= 1.0


def test_lsres_fwd_and_bwd_against_autograd():
    g = _gen(5)
    R, C, rps = 130, 12, 50
    x, y, dout = (torch.randn(R, C, generator=g) for _ in range(3))
    gamma = torch.randn(C, generator=g)
    ss = torch.tensor([0.0, 1.25, 0.8])
    for s in (None, ss):
        xd, yd, gd = (t.double().requires_grad_() for t in (x, y, gamma))
        sc = 1.0 if s is None else s.double()[torch.arange(R) // rps][:, None]
        out = xd + sc * gd * yd
        gy, gg = torch.autograd.grad(out, (yd, gd), dout.double())
        ref, bound = rs.lsres_fwd(x, y, gamma, s, rps)
        assert torch.allclose(ref, out.detach(), rtol=0, atol=1e-14)
        f32 = x + (y * gamma if s is None else s[torch.arange(R) // rps][:, None] * gamma * y)          # fp32, three roundings
        assert rs.worst_ratio(f32.double() - ref, bound) <= 1.0
        dy, dg, mag = rs.lsres_bwd(dout, y, gamma, s, rps)
        assert dy.dtype == torch.float32 and rs.rel(dy, gy) < 1e-6 and torch.allclose(dg, gg, rtol=1e-12, atol=1e-12)
        if s is not None:
            assert bool((dy[:rps] == 0).all())
        # fp32 evaluations of dgamma: the product rounded twice (dout s, then y), summed in three orders
        d = dout if s is None else dout * s[torch.arange(R) // rps][:, None]
        t = d * y
        for fn, ch in ((sum_forward, R), (sum_reverse, R), (sum_pairwise, 8), (lambda v: sum_chunked(v, 4, 3), rs.chain("lsres_bwd", R, 3) - 1)):
            assert rs.worst_ratio(fn(t).double() - dg, rs.sum_bound(min(ch, R - 1), mag, extra=2)) <= 1.0
        r16 = rs.lsres_bwd16(dout, y, gamma, None, s, rps, ldt=256)
        assert torch.equal(r16["dy16"], dy.to(torch.bfloat16)) and r16["dy16T"].shape == (C, 256)
        assert torch.equal(r16["dy16T"][:, :R], r16["dy16"].t()) and bool((r16["dy16T"][:, R:].view(torch.int16) == 0).all())
        assert torch.allclose(r16["dgamma"], gg, rtol=1e-6, atol=1e-6) and torch.allclose(r16["db"], gy.sum(0), rtol=1e-6, atol=1e-6)


def test_lsres_bwd16_order_and_keep():
    g = _gen(6)
    R, C, p = 70, 8, 0.1
    dout, y = torch.randn(R, C, generator=g), torch.randn(R, C, generator=g)
    gamma = torch.randn(C, generator=g)
    kv = rs.keep_value(p)
    assert kv == float(torch.tensor(1.0) / torch.tensor(0.9)) and rs.keep_value(0.5) == 2.0 and rs.keep_value(0.0) == 1.0
    keep = torch.where(torch.rand(R, C, generator=g) >= p, torch.tensor(kv), torch.tensor(0.0))
    assert abs(rs.check_keep(keep, p) - 0.9) <= 0.03
    with pytest.raises(AssertionError):
        rs.check_keep(keep * 1.0000001 + 1e-9, p)
    ss = torch.tensor([0.0, 1.0 / 0.9])
    r = rs.lsres_bwd16(dout, y.half(), gamma, keep, ss, 50)
    want = (((dout * ss[torch.arange(R) // 50][:, None]) * keep) * gamma)
    assert torch.equal(r["dy16"], want.to(torch.bfloat16))
    assert torch.allclose(r["db"], want.double().sum(0), rtol=0, atol=0)
    d = (dout * ss[torch.arange(R) // 50][:, None]) * keep
    assert torch.equal(r["dgamma"], (d.double() * y.half().double()).sum(0))
    # the other order of the two scales (an extra rounding) gives other bits somewhere: the restated order is a real condition
    big, sc = torch.randn(4000, 8, generator=g), torch.tensor(1.0 / 0.7)
    assert not torch.equal((big * sc) * torch.tensor(kv), (big * torch.tensor(kv)) * sc)
    # fp32 sums of db / dgamma in the kernel's chunked order stay inside the bounds
    for key, terms, extra in (("db", want, 0), ("dgamma", d * y.half().float(), 1)):
        got = sum_chunked(terms, 16, 2)
        n = rs.n_add("lsres_bwd16<2>", R, 2, False, tiles=2)
        assert rs.worst_ratio(got.double() - r[key], rs.sum_bound(n, r[key + "_mag"], extra=extra)) <= 1.0, key


def test_act_bwd_restatements():
    g = _gen(7)
    h = torch.cat([torch.linspace(-12, 12, 4801), torch.tensor([40.0, -40.0]), torch.randn(3000, generator=g) * 3])
    dy = torch.randn(h.shape, generator=g)
    hd = h.double().requires_grad_()
    (ref,) = torch.autograd.grad(torch.nn.functional.gelu(hd), hd, dy.double())
    got = rs.gelu_bwd(dy, h)
    assert float((got - ref).abs().max()) < 1e-14
    assert got[4801].item() == dy[4801].double().item() and got[4802].item() == 0.0
    # torch's fp32 autograd (the yardstick) is itself inside its own allowance, and a derivative that is off by 1e-5 |dy| is not
    t32 = rs.torch_gelu_bwd(dy, h)
    units = rs.gelu_err_units(t32, dy, h)
    assert units < 1e-6 and rs.gelu_allowance(units) < 5e-6
    assert rs.gelu_err_units((ref + 1e-5 * dy.double()).float(), dy, h) > rs.gelu_allowance(units)
    den = torch.tensor(2.0 ** -149)
    aux = torch.tensor([0.0, -0.0, den, -den, float("inf"), float("-inf"), 1.0, -1.0])
    d = torch.arange(1.0, 9.0) * -1.5
    out = rs.relu_bwd(d, aux)
    assert out.tolist() == [0.0, 0.0, -4.5, 0.0, -7.5, 0.0, -10.5, 0.0]
    assert bool((rs.bits(out)[[0, 1, 3, 5, 7]] == 0).all())                      # +0, not -0
    xd = torch.tensor([1.0, -1.0], dtype=torch.float64, requires_grad=True)
    (gr,) = torch.autograd.grad(torch.relu(xd), xd, torch.tensor([2.0, 3.0], dtype=torch.float64))
    assert gr.tolist() == rs.relu_bwd(torch.tensor([2.0, 3.0]), torch.tensor([1.0, -1.0])).tolist()


def test_dropout_restatement():
    g = _gen(8)
    x = torch.randn(1000, generator=g)
    kv = torch.tensor(rs.keep_value(0.1))
    mask = torch.rand(1000, generator=g) >= 0.1
    y = torch.where(mask, x * kv, x * 0.0)
    assert torch.equal(rs.check_dropout(x, y, 0.1), mask)
    with pytest.raises(AssertionError):
        rs.check_dropout(x, torch.where(mask, x / 0.9 * 1.000001, x * 0.0), 0.1)
    assert bool(rs.check_dropout(x, x.clone(), 0.0).all())
