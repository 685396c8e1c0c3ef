"""The kernel selection of the weight-gradient TN GEMM (tn_gemm_select in csrc/gemm_bf16tn.hip through kernels.gemm16_tn_plan; no GPU):
the choices it must make, its status codes, the Python split heuristic that has to agree with it, and the coverage of the GPU test's shapes."""
import ctypes
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tn_gemm_cases as C  # noqa: E402


def _plan(M, N, R, splitk, **kw):
    from spe_amd import kernels as K
    return K.gemm16_tn_plan(M, N, R, splitk, **kw)


def _status(M, N, R, lda, ldb, splitk):
    from spe_amd import lib
    v = (ctypes.c_int * 4)()
    return lib.load().spe_gemm_bf16tn_plan(M, N, R, lda, ldb, splitk, v)


def _tiles_per_split(R, plan):
    """Row tiles of each split, as the kernel divides them: split z takes tiles [z * rt_per_split, (z + 1) * rt_per_split) of ceil(R / 64)."""
    rtiles, rt = -(-R // 64), plan["rt_per_split"]
    return [max(0, min(rtiles, (z + 1) * rt) - z * rt) for z in range(plan["splits"])]


def _t128(M, N, splits):
    return -(-M // 128) * -(-N // 128) * splits


def test_instance_list():
    assert len(set(C.INSTANCES)) == 3


@pytest.mark.parametrize("problem,expected", C.PINNED, ids=lambda v: "x".join(map(str, v)) if len(v) == 4 else None)
def test_pinned_choices(problem, expected):
    """Written out by hand from the dispatch code before it became one function (tests/tn_gemm_cases.py)."""
    assert C.tn(*expected) in C.INSTANCES
    plan = _plan(*problem)
    assert plan is not None and (plan["BM"], plan["BN"]) == expected
    assert plan["splits"] == max(1, -problem[3])


def test_plan_never_leaves_the_instance_list():
    """Whatever the problem, the selection names one of the compiled instances or refuses; the splits it plans cover every row tile."""
    seen = set()
    dims = (8, 56, 64, 72, 384, 1160, 2048, 2056)
    for M, N, R, sk in itertools.product(dims, dims, (1, 63, 64, 65, 1100, 8300), (1, -2, -9, -16)):
        plan = _plan(M, N, R, sk)
        if plan is None:                        # more splits than row tiles, nothing else in this sweep
            assert _status(M, N, R, M, N, sk) == -5 and -sk > -(-R // 64), (M, N, R, sk)
            continue
        assert C.kernel_name(plan) in C.INSTANCES, (M, N, R, sk, plan)
        assert plan["splits"] == max(1, -sk)
        assert plan["rt_per_split"] * plan["splits"] >= -(-R // 64), (M, N, R, sk, plan)
        assert sum(_tiles_per_split(R, plan)) == -(-R // 64)
        seen.add(C.kernel_name(plan))
    assert seen == set(C.INSTANCES)             # and every instance is somebody's answer


def test_gpu_cases_reach_every_launch_site_and_pipeline_state():
    """A condition on tests/tn_gemm_cases.py: the shapes of the GPU test reach each of the four launch sites (the 64 x 64 kernel counted
    once by the small-tile rule and once by M <= 64), and within each site some split sees 0, 1, 2, 3 and at least 4 row tiles: the
    nt > 0 guard, no prefetch, one prefetch, the third register stage, both LDS buffer parities."""
    from spe_amd import kernels as K
    assert set(C.GPU_SITES) == set(C.SITE_INSTANCE) == {"small", "128x128", "128x64", "m64"}
    for site, cases in C.GPU_SITES.items():
        states = set()
        for M, N, R, sk in cases:
            plan = _plan(M, N, R, sk, lda=M + 16, ldb=N + 24)          # the strides the GPU test runs them with
            assert plan is not None, (site, M, N, R, sk)
            assert (plan["BM"], plan["BN"]) == C.SITE_INSTANCE[site], (site, M, N, R, sk, plan)
            small = _t128(M, N, plan["splits"]) < K.TN_SMALL_MAX
            assert small == (site == "small"), (site, M, N, R, sk)
            if site == "m64":
                assert M <= 64
            states |= {min(t, 4) for t in _tiles_per_split(R, plan)}
        assert states == {0, 1, 2, 3, 4}, (site, states)
    for case in C.SCALAR_STORE_CASES:
        assert case in C.GPU_CASES
    assert [next(s for s, cs in C.GPU_SITES.items() if c in cs) for c in C.SCALAR_STORE_CASES] == list(C.GPU_SITES)
    assert {R for _, _, R, _ in C.GPU_CASES} >= {1, 63, 65}                 # a ragged last 64-row tile, and one row alone


def test_python_threshold_is_the_library_threshold():
    """kernels.TN_SMALL_MAX and the library's SPE_TN_SMALL_TILES are one number kept in two places: one 128-tile column of TN_SMALL_MAX - 1
    tiles takes the small tiles, of TN_SMALL_MAX tiles the wide ones."""
    from spe_amd import kernels as K
    T = K.TN_SMALL_MAX
    assert C.kernel_name(_plan(128 * (T - 1), 128, 400, 1)) == C.tn(64, 64)
    assert C.kernel_name(_plan(128 * T, 128, 400, 1)) == C.tn(128, 128)
    assert C.kernel_name(_plan(128, 128 * (T - 1), 400, 1)) == C.tn(64, 64)
    assert C.kernel_name(_plan(128, 128 * T, 400, 1)) == C.tn(128, 128)


def test_auto_splitk_agrees_with_the_selection():
    """kernels._dw16_tn asks for min(auto_splitk, R // 64) splits.  The library never refuses that (-5), and wherever auto_splitk sized the
    split for 64 x 64 tiles - 128-tiles x splits below TN_SMALL_MAX before the re-sizing - the library does pick them."""
    from spe_amd import kernels as K
    dims = (64, 256, 384, 1152, 1536, 2048, 4608)
    branch = 0
    for M, N, R in itertools.product(dims, dims, (400, 1100, 8300)):
        sk = min(K.auto_splitk(M, N, R, 1), max(1, R // 64))
        splitk = -sk if sk > 1 else 1
        assert _status(M, N, R, M, N, splitk) == 0, (M, N, R, sk)
        plan = _plan(M, N, R, splitk)
        assert plan["splits"] == sk
        # auto_splitk's own first sizing, repeated here: tiles of 128, at most 512 workgroups, at least 512 rows per split, at most 16
        tiles = _t128(M, N, 1)
        if tiles >= 256 or R < 1024:
            assert sk == 1
            continue
        sk128 = max(1, min(512 // tiles, R // 512, 16))
        if tiles * sk128 < K.TN_SMALL_MAX:
            branch += 1
            assert (plan["BM"], plan["BN"]) == (64, 64), (M, N, R, sk, plan)
    assert branch > 0


def test_status_codes():
    """What spe_gemm_bf16tn returns for a problem it refuses (all but the pointer-alignment part of -2), from the plan entry."""
    ok = (72, 136, 400, 72, 136, 1)
    assert _status(*ok) == 0
    for M, N in ((70, 136), (72, 132), (4, 8), (8, 12)):                    # M or N no multiple of 8
        assert _status(M, N, 400, 72, 136, 1) == -2, (M, N)
    for lda, ldb in ((76, 136), (72, 140), (73, 136), (72, 137)):           # lda or ldb no multiple of 8
        assert _status(72, 136, 400, lda, ldb, 1) == -2, (lda, ldb)
    assert _status(72, 136, 400, 80, 160, 1) == 0                           # wider operands are fine
    for sk in (2, 3, 16):                                                   # slabs are asked for with a negative count
        assert _status(72, 136, 400, 72, 136, sk) == -2, sk
    for R in (0, -1):
        assert _status(72, 136, R, 72, 136, 1) == -4, R
        assert _status(70, 136, R, 72, 136, 1) == -4, R                     # ... reported before the alignment
    assert _status(72, 136, 400, 72, 136, -7) == 0                          # ceil(400 / 64) = 7 row tiles
    assert _status(72, 136, 400, 72, 136, -8) == -5
    assert _status(72, 136, 1, 72, 136, -2) == -5
    assert _status(72, 136, 400, 72, 136, 0) == 0 and _plan(72, 136, 400, 0)["splits"] == 1
    assert _status(72, 136, 400, 72, 136, -1) == 0 and _plan(72, 136, 400, -1)["splits"] == 1
    for M, N in ((0, 136), (72, 0), (-8, 136)):                             # nothing to do: the launcher returns 0 without a launch
        assert _status(M, N, 400, 72, 136, 1) == 0
        assert _plan(M, N, 400, 1, lda=72, ldb=136) == dict(BM=0, BN=0, splits=0, rt_per_split=0)
    assert _plan(70, 136, 400, 1) is None
