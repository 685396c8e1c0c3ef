"""tests/cvt16_ref.py and tests/cvt16_cases.py on the CPU, no device: the integer restatements of the two roundings agree with torch's
conversions over the whole value list, the transpose helper round-trips, and the geometry list reaches every path of cvt_bf16_tile
(csrc/gemm_bf16.hip) that the issue behind these tests names - so that a later edit cannot thin the list silently."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvt16_cases as CS  # noqa: E402
import cvt16_ref as CR  # noqa: E402


def _values(bits):
    return CR.bits_to_f32(torch.tensor(bits, dtype=torch.int64))


def _same_but_nan(got, want, fmt):
    ng, nw = CR.is_nan16(got, fmt), CR.is_nan16(want, fmt)
    return torch.equal(ng, nw) and torch.equal(got.masked_fill(ng, 0), want.masked_fill(nw, 0))


def test_value_list_holds_what_it_promises():
    x = _values(CS.VALUE_BITS)
    assert len(CS.RANDOM_BITS) == 4096 and {(b >> 23) & 0xFF for b in CS.RANDOM_BITS} == set(range(256))
    assert len(CS.MAIN_BITS) + len(CS.SUBNORMAL_BITS) == len(CS.VALUE_BITS) and len(CS.SUBNORMAL_BITS) >= 8
    assert torch.isinf(x).sum() >= 2 and torch.isnan(x).sum() >= 2
    for v in (0.0, 65504.0, 65520.0, 1e9, 6.1e-5, 6.0e-8, 2.9e-8, 1e-10, 3.4028234663852886e38):
        assert (x == torch.tensor(v, dtype=torch.float32)).any(), v
    assert ((x == 0) & torch.signbit(x)).any()
    xf = _values(CS.FINITE_BITS)
    assert torch.isfinite(xf).all() and xf.abs().max() < 2.0 ** 40 and not ((xf != 0) & (xf.abs() < 2.0 ** -126)).any()
    # ties and their neighbours: 1 + 2^-8 is halfway between the bf16 values 1 and 1 + 2^-7, lower neighbour even; 0x3F81 is odd
    b = CR.bf16_rne_bits(_values([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0x7F7F8000, 0x7F7F7FFF]))
    assert [int(v) & 0xFFFF for v in b] == [0x3F80, 0x3F82, 0x3F80, 0x3F81, 0x3F81, 0x3F82, 0x7F80, 0x7F7F]


def test_bf16_rne_bits_is_torchs_rounding():
    x = _values(CS.VALUE_BITS)
    got, want = CR.bf16_rne_bits(x), x.to(torch.bfloat16).view(torch.int16)
    assert _same_but_nan(got, want, "bf16")
    assert int(CR.is_nan16(got, "bf16").sum()) == int(torch.isnan(x).sum())


def test_lo_bits_is_the_definition():
    """lo = bf16(x - bf16(x)) with torch's own conversions; hi + lo reproduces x to 16 significant bits; the pinned outcomes."""
    x = _values(CS.VALUE_BITS)
    hi = x.to(torch.bfloat16)
    want = (x - hi.float()).to(torch.bfloat16).view(torch.int16)
    got = CR.lo_bits(x)
    assert _same_but_nan(got, want, "bf16")
    fin = torch.isfinite(hi.float())
    rec = hi.float().double() + CR.bf16_bits_to_f32(got).double()
    assert ((rec - x.double()).abs()[fin] <= x.double().abs()[fin] * 2.0 ** -16 + 2.0 ** -133).all()
    pin = CR.lo_bits(_values([0x7F800000, 0xFF800000, 0x7F7F8000, 0xFF7FFFFF]))
    assert CR.is_nan16(pin[:2], "bf16").all()                                     # inf - inf
    assert [int(v) & 0xFFFF for v in pin[2:]] == [0xFF80, 0x7F80]                 # finite - (+-inf) = -+inf


def test_f16_sat_bits_is_torchs_half_of_the_clamp():
    x = _values(CS.VALUE_BITS)
    want = torch.where(torch.isnan(x), x, x.clamp(-65504.0, 65504.0)).half().view(torch.int16)
    got = CR.f16_sat_bits(x)
    assert _same_but_nan(got, want, "f16")
    assert int(CR.is_nan16(got, "f16").sum()) == int(torch.isnan(x).sum())
    assert not ((got.to(torch.int64) & 0x7FFF) == 0x7C00).any()                   # saturating: never an infinity
    pin = CR.f16_sat_bits(torch.tensor([1e9, -1e9, 65520.0, float("inf"), 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 1e-10, -1e-10]))
    assert [int(v) & 0xFFFF for v in pin] == [0x7BFF, 0xFBFF, 0x7BFF, 0x7BFF, 0x0001, 0x0000, 0x0002, 0x0000, 0x8000]
    sub = (got.to(torch.int64) & 0x7C00) == 0
    assert int((sub & ((got.to(torch.int64) & 0x3FF) != 0)).sum()) >= 8            # fp16 subnormal results occur in the list


def test_transposeT_round_trips():
    g = torch.Generator().manual_seed(3)
    for R, C, ldt in ((1, 1, 1), (5, 3, 5), (5, 3, 9), (65, 67, 65 + 68), (64, 4, 64)):
        b = torch.randint(1, 32767, (R, C), generator=g, dtype=torch.int16)
        t = CR.transposeT(b, ldt)
        assert t.shape == (C, ldt)
        back, pad = CR.untransposeT(t, R)
        assert torch.equal(back, b) and pad.shape == (C, ldt - R) and not pad.any()
        assert all(int(t[c, r]) == int(b[r, c]) for r, c in ((0, 0), (R - 1, C - 1), (R // 2, C // 3)))


def test_act_bwd64_and_colsum64():
    x = torch.tensor([[1.5, -2.0, 3.0, 4.0], [0.5, 0.25, -1.0, 2.0]])
    aux = torch.tensor([[1.0, 0.0, -0.0, -3.0], [2.0, -1.0, 1e-30, 0.5]])
    assert torch.equal(CR.act_bwd64(x, aux, 1), torch.tensor([[1.5, 0, 0, 0], [0.5, 0, -1.0, 2.0]], dtype=torch.float64))
    assert torch.equal(CR.colsum64(x), torch.tensor([2.0, -1.75, 2.0, 6.0], dtype=torch.float64))
    h = torch.linspace(-6, 6, 97, dtype=torch.float64).requires_grad_()
    (gd,) = torch.autograd.grad(torch.nn.functional.gelu(h).sum(), h)
    assert (CR.gelu_grad64(h.detach()) - gd).abs().max() < 1e-14
    assert float(CR.gelu_grad64(torch.tensor([0.0]))) == 0.5
    f32 = CR.gelu_bwd_f32_formula(torch.ones(97), h.detach().float())
    assert (f32.double() - CR.act_bwd64(torch.ones(97), h.detach().float(), 2)).abs().max() < 1e-6


# ---- the geometry list ---------------------------------------------------------------------------------------------------------------
def case_paths(c):
    """The branches of cvt_bf16_tile a case runs, from the conditions in csrc/gemm_bf16.hip."""
    R, C, ldx, ldo, ldt, outs = c["R"], c["C"], c["ldx"], c["ldo"], c["ldt"], c["outputs"]
    p = set()
    vec_x = ldx % 4 == 0 and c["xoff"] == 0
    p.add("x:vector" if vec_x and C >= 4 else "x:scalar")
    if C % 4:
        p.add("C%4")
    if ldx % 4:
        p.add("ldx%4")
    if c["xoff"]:
        p.add("x:unaligned")
    if "out" in outs or "lo" in outs:
        p.add("out:vector" if ldo % 4 == 0 and C >= 4 else "out:scalar")
        if ldo % 4:
            p.add("ldo%4")
        if ldo > C:
            p.add("out:block")
            p.add("out:block@%d" % c["off"])
    if "T" in outs:
        p.add("T:vector" if ldt % 4 == 0 else "T:scalar")
        if ldt % 4:
            p.add("ldt%4")
        if ldt >= R + 64:
            p.add("T:padding-tile")
        if ldt > R:
            p.add("T:padded")
        if "colsum" in outs and ldt >= R + 64:
            p.add("colsum+padding-tile")
    if R > 64:
        p.add("row-tiles>1")
    if C > 64:
        p.add("col-tiles>1")
    return p


def test_geometry_list_reaches_every_path():
    names = [c["name"] for c in CS.GEOMETRY]
    assert len(set(names)) == len(names) and 55 <= len(names) <= 80
    reached = set()
    for c in CS.GEOMETRY:
        assert c["entry"] in ("cvt", "h") and c["outputs"], c["name"]
        assert c["R"] * c["C"] <= CS.MAX_ELEMS and c["ldx"] >= c["C"] and c["off"] + c["C"] <= c["ldo"] and c["ldt"] >= c["R"], c["name"]
        assert c["xoff"] in (0, 1) and set(c["outputs"]) <= set(CS.CVT_OUTPUTS if c["entry"] == "cvt" else CS.H_OUTPUTS), c["name"]
        # the contract: vector stores need 8-byte aligned output blocks, i.e. a column offset that is a multiple of 4 when ldo is
        assert c["ldo"] % 4 or c["off"] % 4 == 0, c["name"]
        reached |= {"%s:%s" % (c["entry"], q) for q in case_paths(c)}
    want = {"C%4", "ldx%4", "x:unaligned", "ldo%4", "ldt%4", "T:padding-tile", "out:block", "out:block@0", "out:block@4", "out:block@64",
            "x:vector", "x:scalar", "out:vector", "out:scalar", "T:vector", "T:scalar", "T:padded", "row-tiles>1", "col-tiles>1"}
    for entry in ("cvt", "h"):
        missing = {q for q in want if "%s:%s" % (entry, q) not in reached} - ({"out:block@0"} if entry == "h" else set())
        assert not missing, (entry, missing)
    assert "cvt:colsum+padding-tile" in reached
    assert {c["R"] for c in CS.GEOMETRY} >= set(CS.R_VALUES) and {c["C"] for c in CS.GEOMETRY} >= set(CS.C_VALUES)
    # ldx: C, C rounded up to 4, an odd value > C; ldt: R, R up to 64, R + 1, R + 3, R + 68
    assert any(c["ldx"] == c["C"] for c in CS.GEOMETRY) and any(c["ldx"] > c["C"] and c["ldx"] == CS.rup(c["C"], 4) for c in CS.GEOMETRY)
    assert any(c["ldx"] > c["C"] and c["ldx"] % 2 for c in CS.GEOMETRY)
    for d in (0, 1, 3, 68):
        assert any("T" in c["outputs"] and c["ldt"] == c["R"] + d for c in CS.GEOMETRY), d
    assert any("T" in c["outputs"] and c["ldt"] == CS.rup(c["R"], 64) > c["R"] for c in CS.GEOMETRY)


def test_every_output_subset_occurs():
    for entry, names in (("cvt", CS.CVT_OUTPUTS), ("h", CS.H_OUTPUTS)):
        have = {frozenset(c["outputs"]) for c in CS.GEOMETRY if c["entry"] == entry}
        for n in range(1, 2 ** len(names)):
            s = frozenset(names[i] for i in range(len(names)) if n >> i & 1)
            assert s in have, (entry, sorted(s))


def test_side_lists_cover_the_issue():
    assert {(R, C) for R, C, _ in CS.COLSUM} >= {(R, C) for R in (1, 63, 64, 65, 129, 200) for C in (5, 64, 132)}
    assert any(ldt is not None and ldt > R + 64 for R, C, ldt in CS.COLSUM)
    assert all(R * C <= CS.MAX_ELEMS for R, C, _ in CS.COLSUM)
    assert {a for a, *_ in CS.ACT} == {1, 2} and all(ldx > C for _, _, C, ldx in CS.ACT)
    assert {R for R, *_ in CS.F16} == {1, 7, 300} and {C for _, C, *_ in CS.F16} == {4, 8, 132}
    assert all(C % 4 == 0 and ldx % 4 == 0 and ldo % 4 == 0 for _, C, ldx, ldo in CS.F16)
    assert any(ldx > C for _, C, ldx, _ in CS.F16) and any(ldo > C for _, C, _, ldo in CS.F16)
