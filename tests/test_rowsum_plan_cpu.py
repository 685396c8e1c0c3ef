"""The launch choices of the column-sum, LayerScale, activation-backward and dropout launchers of csrc/rowops.hip (spe_rowops_plan through
kernels.rowops_plan; no GPU) against the launchers' grid arithmetic as it was written before it moved into one host function per
launcher (tests/rowsum_cases.expected), and the coverage of the GPU test's cases (tests/rowsum_cases.py): every case takes the branch and
the member count it claims, every branch and every member regime of the fixed-order sum (1, 2-16, 17-256, > 256) keeps a case."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowsum_cases as C  # noqa: E402

ALL_CASES = [c for cs in C.GPU_CASES.values() for c in cs]


def plan_of(c):
    from spe_amd import kernels as K
    ld = None
    if c["launcher"] == "colsum":
        ld = c["C"] + c.get("pad", 0)
    elif c["launcher"] == "lsres_bwd16":
        ld = c["ldt"] if "ldt" in c else C.ldt_of(c)
    return K.rowops_plan(c["launcher"], c["R"], c["C"], ld=ld, aligned=C.aligned_of(c))


def as_tuple(plan):
    return (plan["kernel"], plan["grid_x"], plan["grid_y"], plan["members"], plan["status"])


def test_case_ids_are_unique():
    assert len({c["id"] for c in ALL_CASES}) == len(ALL_CASES)
    assert len({r["id"] for r in C.BWD16_REFUSALS}) == len(C.BWD16_REFUSALS)


@pytest.mark.parametrize("c", ALL_CASES, ids=lambda c: c["id"])
def test_gpu_case_hits_the_branch_it_claims(c):
    plan = plan_of(c)
    assert plan["status"] == 0
    assert (plan["kernel"], plan["members"]) == (c["kernel"], c["members"]), plan
    assert as_tuple(plan) == C.expected(c)


def test_gpu_cases_reach_every_branch_and_member_regime():
    """A condition on tests/rowsum_cases.py: take a case away so that a kernel or a member regime is no longer reached, and this fails."""
    kernels = {c["kernel"] for c in ALL_CASES}
    assert kernels == set(C.KERNELS), set(C.KERNELS) ^ kernels
    reached = {(c["kernel"], C.regime(c["members"])) for c in ALL_CASES}
    missing = [kr for kr in C.REQUIRED_REGIMES if kr not in reached]
    assert not missing, missing
    assert {r for _, r in reached if r} == set(C.REGIMES)


def test_named_edges():
    """The edges the case lists are built around, written out by hand."""
    from spe_amd import kernels as K
    p = K.rowops_plan
    assert as_tuple(p("colsum", 64, 4096)) == ("colsum_wide", 4, 1, 0, 0) and as_tuple(p("colsum", 1, 4100)) == ("colsum_wide", 5, 1, 0, 0)
    assert p("colsum", 65, 4096)["kernel"] == "colsum_tall4" and p("colsum", 64, 4092)["kernel"] == "colsum_tall4"
    assert p("colsum", 64, 4096, aligned=False)["kernel"] == "colsum" and p("colsum", 64, 4096, ld=4098)["kernel"] == "colsum"
    for R, m in ((64, 1), (65, 2), (1024, 16), (1025, 17), (16384, 256), (16448, 257), (10 ** 6, 2048)):
        assert as_tuple(p("colsum", R, 64)) == ("colsum_tall4", 1, m, m, 0), R
    assert as_tuple(p("colsum", 4096, 2048)) == ("colsum_tall4", 32, 64, 64, 0) and as_tuple(p("colsum", 4160, 2048)) == ("colsum_tall4", 32, 64, 64, 0)
    for R, m in ((1, 1), (256, 1), (257, 2), (4096, 16), (4097, 17), (16384, 64), (16640, 64)):
        assert as_tuple(p("colsum", R, 91)) == ("colsum", 2, m, m, 0), R
    assert as_tuple(p("lsres_fwd", 256, 4)) == ("lsres_fwd", 1, 1, 0, 0) and as_tuple(p("lsres_fwd", 257, 4)) == ("lsres_fwd", 2, 1, 0, 0)
    assert as_tuple(p("lsres_fwd", 4096, 1024)) == ("lsres_fwd", 4096, 1, 0, 0) and as_tuple(p("lsres_fwd", 4100, 1024)) == ("lsres_fwd", 4096, 1, 0, 0)
    for R, m in ((16, 1), (17, 2), (256, 16), (257, 17), (2048, 128), (2049, 128)):
        assert as_tuple(p("lsres_bwd", R, 1024)) == ("lsres_bwd_rows", m, 1, m, 0), R
    assert p("lsres_bwd", 100, 1028)["kernel"] == "lsres_bwd" and p("lsres_bwd", 100, 1024, aligned=False)["kernel"] == "lsres_bwd"
    for R, m in ((64, 1), (65, 2), (16384, 256), (16385, 256)):
        assert as_tuple(p("lsres_bwd", R, 91)) == ("lsres_bwd", 2, m, m, 0), R
    assert p("lsres_bwd16", 65, 512)["kernel"] == "lsres_bwd16<2>" and p("lsres_bwd16", 65, 516)["kernel"] == "lsres_bwd16<4>"
    for R, m in ((64, 1), (65, 2), (16384, 256), (16385, 256)):
        assert p("lsres_bwd16", R, 64)["members"] == m, R
    assert p("lsres_bwd16", 1, 64, ld=192)["members"] == 3
    assert as_tuple(p("act_bwd", 1024)) == ("act_bwd", 1, 1, 0, 0) and as_tuple(p("act_bwd", 1028)) == ("act_bwd", 2, 1, 0, 0)
    assert p("act_bwd", 4096 * 1024)["grid_x"] == 4096 and p("act_bwd", 4096 * 1024 + 4)["grid_x"] == 4096
    assert as_tuple(p("dropout", 256)) == ("dropout", 1, 1, 0, 0) and as_tuple(p("dropout", 257)) == ("dropout", 2, 1, 0, 0)
    assert p("dropout", 8192 * 256 + 1)["grid_x"] == 8192


def test_sweep_against_the_restated_expressions():
    for R in (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 16385, 40000):
        for Cc in (1, 4, 60, 64, 68, 91, 512, 516, 1024, 1028, 2048, 4092, 4096, 4100):
            for kw in ({}, {"off": 1}, {"pad": 2}, {"pad": 8}):
                for L in ("colsum", "lsres_fwd", "lsres_bwd", "lsres_bwd16"):
                    c = dict(launcher=L, R=R, C=Cc, **kw)
                    assert as_tuple(plan_of(c)) == C.expected(c), c
    for n in (0, 1, 3, 4, 1020, 1024, 1028, 4096 * 1024, 4096 * 1024 + 4, 8192 * 256, 8192 * 256 + 1):
        for L in ("act_bwd", "dropout"):
            c = dict(launcher=L, R=n, C=0)
            assert as_tuple(plan_of(c)) == C.expected(c), c


def test_status_codes():
    from spe_amd import kernels as K, lib
    for c in C.REFUSED:
        assert as_tuple(plan_of(c)) == (None, 0, 0, 0, -2), c
    for r in C.BWD16_REFUSALS:
        if "p" in r:                                    # the rate / rows_per_sample refusals belong to the entry point, not the shape
            continue
        c = dict(launcher="lsres_bwd16", **r)
        assert as_tuple(plan_of(c)) == (None, 0, 0, 0, -2), r
    for L in K.ROWOPS_LAUNCHERS:                         # nothing to do comes before every refusal
        assert as_tuple(K.rowops_plan(L, 0, 6, ld=7, aligned=False)) == (None, 0, 0, 0, 0), L
    assert as_tuple(K.rowops_plan("colsum", 5, 0)) == (None, 0, 0, 0, 0)
    v = (ctypes.c_long * 4)(9, 9, 9, 9)
    assert lib.load().spe_rowops_plan(6, 10, 8, 8, 1, v) == -2 and list(v) == [0, 0, 0, 0]
    assert lib.load().spe_abi_version() == 7 and len(lib.PROTOS["spe_rowops_plan"]) == 6
    assert len(lib.PROTOS["spe_colsum"]) == 7 and len(lib.PROTOS["spe_layerscale_residual_bwd16d"]) == 17      # the launchers keep their signatures
