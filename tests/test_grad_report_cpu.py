"""The gradient report's contract without a GPU: the fp32 restatement of the documented order (grad_report_ref.py) against fp64 and
against a brute-force computation, the declaration of the entry, and the one-line formatter of the training loop."""
import ctypes
import math
import re

import numpy as np
import pytest

import grad_report_ref as R
from grad_report_cases import (CHUNK, FOLD_TILE, LENGTHS, LONG_LENGTH, OVERFLOWS, PASS_SPAN, THREADS, TRIP_PASSES, VALUE_SETS, grad_values,
                               weight_values)

SCALES = [1.0, 0.5, 1.0 / 3.0]


@pytest.mark.parametrize("name", VALUE_SETS)
def test_restatement_stays_within_its_bound_of_fp64(name):
    """Every length and three gradient scales; the bound is R.bound's: the longest addition chain plus the roundings before it."""
    worst = 0.0
    for L in LENGTHS:
        g, p = grad_values(name, L), weight_values(L)
        for scale in SCALES:
            r32, r64 = R.record32(g, p, scale), R.record64(g, p, scale)
            if name in OVERFLOWS and L >= OVERFLOWS[name] and not math.isfinite(float(r32["grad_sq"])):
                assert r64["grad_sq"] > 3.0e38                       # the overflow is real, not the restatement's
            else:
                err, b = abs(float(r32["grad_sq"]) - r64["grad_sq"]), R.bound(L, r64["grad_sq"], 3)
                assert math.isfinite(float(r32["grad_sq"])) and err <= b, (L, scale, err, b)
                worst = max(worst, err / b if b else 0.0)
            err, b = abs(float(r32["weight_sq"]) - r64["weight_sq"]), R.bound(L, r64["weight_sq"], 1)
            assert err <= b, (L, err, b)
            worst = max(worst, err / b)
    print(f"{name}: largest error / bound = {worst:.3f}")


@pytest.mark.parametrize("name", VALUE_SETS)
def test_exact_words_of_the_restatement_equal_brute_force(name):
    for L in LENGTHS:
        g, p = grad_values(name, L), weight_values(L)
        for scale in SCALES[:2]:
            r, b = R.record32(g, p, scale), R.brute(g, p, scale)
            for k in ("nan", "inf", "first_bad"):
                assert r[k] == b[k], (L, k)
            for k in ("grad_absmax", "weight_absmax"):
                assert np.float32(r[k]).view(np.uint32) == np.float32(b[k]).view(np.uint32), (L, k, r[k], b[k])


def test_overflow_cases_overflow_where_the_guard_does():
    """A finite 3e19 makes its own parameter's sum infinite at any length; values near 1.3e19 have finite squares whose sum leaves fp32
    from three elements on.  Neither counts as NaN or inf."""
    for L in LENGTHS:
        r = R.record32(grad_values("big_finite", L), None, 1.0)
        assert np.isposinf(r["grad_sq"]) and r["nan"] == r["inf"] == 0 and r["first_bad"] == -1 and float(r["grad_absmax"]) == float(np.float32(3e19))
        r = R.record32(grad_values("sum_overflow", L), None, 1.0)
        assert np.isposinf(r["grad_sq"]) == (L >= 3) and r["nan"] == r["inf"] == 0 and np.isfinite(r["grad_absmax"])
        assert float(r["grad_absmax"]) ** 2 < 3.4e38


def test_nonfinite_elements_count_as_plus_zero():
    for name in ("nan_first", "inf_last", "neginf_middle", "nan_then_inf", "inf_then_nan"):
        for L in LENGTHS:
            g = grad_values(name, L)
            clean = np.where(np.isfinite(g), g, np.float32(0.0)).astype(np.float32)
            a, b = R.record32(g, None, 0.5), R.record32(clean, None, 0.5)
            assert np.array_equal(R.words(a)[:2], R.words(b)[:2]) and a["nan"] + a["inf"] > 0 and b["nan"] + b["inf"] == 0
    assert R.record32(grad_values("nan_then_inf", 1025), None, 1.0)["first_bad"] == 1025 // 3
    g = grad_values("inf_then_nan", 1025)
    assert np.isinf(g[R.record32(g, None, 1.0)["first_bad"]]) and R.record32(g, None, 1.0)["nan"] == 3


def test_sum32_follows_the_documented_order_on_a_hand_made_case():
    """Powers of two chosen so that the order shows: 1 in lane 0 of pass 0, then 2^-24 in pass 1 and pass 2 of the same lane are each
    lost against the 1 (added one at a time), while in one vector they first add up to 2^-23 and survive."""
    x = np.zeros(2 * PASS_SPAN + 1, dtype=np.float32)
    x[0], x[PASS_SPAN], x[2 * PASS_SPAN] = 1.0, 2.0 ** -24, 2.0 ** -24
    assert float(R.sum32(x)) == 1.0
    y = np.zeros(8, dtype=np.float32)
    y[0], y[2], y[3] = 1.0, 2.0 ** -24, 2.0 ** -24
    assert float(R.sum32(y)) == 1.0 + 2.0 ** -23
    z = np.zeros(2 * CHUNK + 1, dtype=np.float32)                    # the same across chunks: one at a time, in chunk order
    z[0], z[CHUNK], z[2 * CHUNK] = 1.0, 2.0 ** -24, 2.0 ** -24
    assert float(R.sum32(z)) == 1.0
    z[2 * CHUNK], z[CHUNK + 7] = 0.0, 2.0 ** -24
    assert float(R.sum32(z)) == 1.0 + 2.0 ** -23
    assert R.chain(1) == R.chain(PASS_SPAN) == 14 and R.chain(PASS_SPAN + 1) == 15 and R.chain(CHUNK) == 29 and R.chain(CHUNK + 1) == 30
    assert PASS_SPAN == 4 * THREADS and CHUNK % PASS_SPAN == 0 and LONG_LENGTH > FOLD_TILE * CHUNK
    assert any((TRIP_PASSES - 1) * PASS_SPAN + 4 <= L <= CHUNK for L in LENGTHS) and any(PASS_SPAN < L <= 3 * PASS_SPAN for L in LENGTHS)
    assert any(CHUNK < L <= 2 * CHUNK for L in LENGTHS) and any(2 * CHUNK < L for L in LENGTHS)


def test_header_declares_the_entry_and_the_constant():
    from spe_amd import kernels as K, lib
    sig = lib.PROTOS["spe_grad_report"]
    assert [n for _, n in sig] == ["g", "p", "n", "par_beg", "par_len", "npar", "grad_scale", "guard", "when", "out", "stream"]
    types = dict((n, t) for t, n in sig)
    assert types["n"] is ctypes.c_long and types["npar"] is ctypes.c_int and types["grad_scale"] is ctypes.c_float and types["when"] is ctypes.c_int
    m = re.search(r"#define\s+SPE_GRAD_REPORT_WORDS\s+(\d+)", open(lib.HEADER).read())
    assert m and int(m.group(1)) == K.GRAD_REPORT_WORDS == 8
    assert len(lib.PROTOS["spe_adamw_gate"]) == 8 and len(lib.PROTOS["spe_adamw_flat_guarded"]) == 15           # the neighbours keep their signatures


# ---- format_skip_report ----------------------------------------------------------------------------------------------------------------
def _row(name, nan=0, inf=0, first_bad=None, grad_sq=1.0, grad_absmax=0.5):
    return {"name": name, "shape": (4, 5), "numel": 20, "nan": nan, "inf": inf, "first_bad": first_bad, "grad_sq": grad_sq,
            "grad_norm": math.sqrt(grad_sq), "grad_absmax": grad_absmax, "weight_norm": 1.0, "weight_absmax": 0.25}


def _report(rows, attempt=7, top=5):
    culprits = [r for r in rows if r["nan"] + r["inf"] > 0 or not math.isfinite(r["grad_sq"])]
    return {"attempt": attempt, "params": rows, "culprits": culprits, "largest": sorted(rows, key=lambda r: -r["grad_absmax"])[:top],
            "total_overflow": not culprits}


def test_format_names_the_culprits():
    from spe_amd.engine import format_skip_report
    rows = [_row("a.weight"), _row("b.weight", nan=2, inf=1, first_bad=(3, 1)), _row("c.bias", inf=1, first_bad=(0, 0))]
    line = format_skip_report(_report(rows))
    assert "\n" not in line and line.startswith("Skipped step 7: ")
    assert "b.weight[3, 1] nan=2 inf=1" in line and "c.bias[0, 0] nan=0 inf=1" in line
    assert "a.weight" not in line and "more)" not in line and "overflow" not in line


def test_format_words_the_overflow_of_one_parameter():
    from spe_amd.engine import format_skip_report
    rows = [_row("a.weight"), _row("d.weight", grad_sq=math.inf, grad_absmax=3e19)]
    line = format_skip_report(_report(rows, attempt=2))
    assert line == "Skipped step 2: d.weight |g|max=3e+19 (square overflows fp32)"


def test_format_words_the_total_overflow():
    from spe_amd.engine import format_skip_report
    rows = [_row(f"p{i}", grad_sq=1.6e38, grad_absmax=1.3e19 + i * 1e17) for i in range(4)]
    rep = _report(rows, top=3)
    assert rep["total_overflow"] and not rep["culprits"]
    line = format_skip_report(rep)
    assert "\n" not in line and "only the total squared norm overflows fp32" in line
    assert line.index("p3 |g|max=") < line.index("p2 |g|max=") < line.index("p1 |g|max=") and "p0" not in line
    assert "nan=" not in line and "square overflows" not in line


def test_format_limits_the_list_and_counts_the_rest():
    from spe_amd.engine import format_skip_report
    rows = [_row(f"w{i}", nan=1, first_bad=(0, i)) for i in range(8)]
    line = format_skip_report(_report(rows))
    assert line.count("nan=1") == 5 and line.endswith(" (+3 more)") and "w4[0, 4]" in line and "w5" not in line
    line = format_skip_report(_report(rows), limit=2)
    assert line.count("nan=1") == 2 and line.endswith(" (+6 more)")
    assert "more)" not in format_skip_report(_report(rows), limit=8)
    rep = _report([_row(f"p{i}", grad_sq=1.6e38, grad_absmax=1e19 + i) for i in range(6)], top=6)
    assert format_skip_report(rep, limit=4).endswith(" (+2 more)")
