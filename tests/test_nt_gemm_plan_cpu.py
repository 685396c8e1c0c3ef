"""The kernel selection of the 16-bit NT GEMM family (csrc/gemm_nt_select.h through kernels.gemm16_plan; no GPU): the choices it must
make, the Python predicate that has to agree with it, and the coverage of the GPU test's shapes."""
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nt_gemm_cases as C  # noqa: E402


def _name(problem):
    from spe_amd import kernels as K
    p = dict(problem)
    return C.kernel_name(K.gemm16_plan(p.pop("M"), p.pop("N"), p.pop("K"), **p))


def test_instance_list_is_14_plus_10():
    assert len(set(C.INSTANCES)) == 24
    assert sum(n.startswith("gemm_nt2_kernel") for n in C.INSTANCES) == 14
    assert sum(n.startswith("gemm_bf16nt_kernel") for n in C.INSTANCES) == 10


@pytest.mark.parametrize("problem,expected", C.PINNED, ids=lambda v: None if not isinstance(v, dict) else
                         "-".join(f"{k}{v[k]}" for k in v))
def test_pinned_choices(problem, expected):
    """Written out by hand from the dispatch code before it became one function (tests/nt_gemm_cases.py)."""
    assert expected is None or expected in C.INSTANCES
    assert _name(problem) == expected


def test_plan_never_leaves_the_instance_list():
    """Whatever the problem, the selection names one of the compiled instances or reports that no kernel covers it."""
    seen = set()
    dims = dict(M=(1, 64, 65, 130, 2047, 2048, 7169, 8300), N=(8, 56, 64, 72, 384, 1023, 1024, 2047, 2048, 4608), K=(8, 64, 128, 200, 448, 512, 1024))
    flags = [dict(split=s, ex=e, op_f16=f, lo_f16=l) for s, e, f, l in itertools.product((False, True), repeat=4)]
    for M, N, K_ in itertools.product(*dims.values()):
        for fl in flags:
            for extra in (dict(), dict(splitk=-2), dict(out16T=True, ld16t=((M + 63) // 64) * 64)):
                if ("splitk" in extra and (fl["ex"] or K_ < 128)) or ("out16T" in extra and not fl["ex"]):
                    continue
                n = _name(dict(M=M, N=N, K=K_, **fl, **extra))
                assert n is None or n in C.INSTANCES, (M, N, K_, fl, extra, n)
                seen.add(n)
    assert seen - {None} == set(C.INSTANCES)          # and every instance is somebody's answer


def test_mlp_f16_ok_implies_the_fp16_ex_kernels():
    """kernels.mlp_f16_ok stays a Python predicate (it runs per forward); wherever it says yes, both products of the MLP must have an
    fp16-operand extended-epilogue kernel in the table (fc1: R x Hd x K with the fp16 second copy, fc2: R x N x Hd)."""
    from spe_amd import kernels as K
    old = K.MLP_F16, K.get_precision()
    K.MLP_F16 = True
    K.set_precision("bf16s")
    yes = 0
    try:
        for R, Kd, Hd, N in itertools.product((2047, 2048, 8300), (64, 96, 128, 384, 1536), (64, 96, 128, 384, 1536), (56, 64, 384)):
            if not K.mlp_f16_ok(R, Kd, Hd, N):
                continue
            yes += 1
            for plan in (K.gemm16_plan(R, Hd, Kd, ex=True, op_f16=True, lo_f16=True), K.gemm16_plan(R, N, Hd, ex=True, op_f16=True)):
                assert plan is not None and plan["family"] == "nt2" and plan["F16"] and plan["EX"], (R, Kd, Hd, N, plan)
    finally:
        K.MLP_F16 = old[0]
        K.set_precision(old[1])
    assert yes > 0


def test_gpu_cases_reach_every_instance():
    """A condition on tests/nt_gemm_cases.py: the shapes of the GPU test hit each of the 14 + 10 compiled kernels at least once."""
    hit = {_name(p) for p in C.GPU_CASES}
    assert None not in hit
    assert set(C.INSTANCES) - hit == set(), sorted(set(C.INSTANCES) - hit)
