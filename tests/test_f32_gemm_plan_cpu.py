"""The kernel selection of the fp32-operand strided GEMM (gemm_f32_select in csrc/gemm.hip through kernels.gemm_plan; no GPU): the choices
it must make, its status codes, and the coverage of the GPU test's cases (tests/f32_gemm_cases.py) - every one of the 12 instances in
every state of the kernel that the case table lists."""
import ctypes
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f32_gemm_cases as C  # noqa: E402


def _fill(kw):
    """Contiguous leading dimensions where the entry names none."""
    kw = dict(kw)
    ta, tb = kw.get("transA", False), kw.get("transB", False)
    kw.setdefault("lda", kw["M"] if ta else kw["K"])
    kw.setdefault("ldb", kw["K"] if tb else kw["N"])
    kw.setdefault("ldc", kw["N"])
    return kw


def _plan(**kw):
    from spe_amd import kernels as K
    return K.gemm_plan(**_fill(kw))


def _status(**kw):
    from spe_amd import lib
    kw = _fill(kw)
    sA, sB, sC = kw.get("sA", (0, 0)), kw.get("sB", (0, 0)), kw.get("sC", (0, 0))
    v = (ctypes.c_long * 11)()
    return lib.load().spe_gemm_f32_plan(kw["M"], kw["N"], kw["K"], kw["lda"], kw["ldb"], kw["ldc"], int(kw.get("transA", 0)),
                                        int(kw.get("transB", 0)), kw.get("batch0", 1), kw.get("batch1", 1), sA[0], sA[1], sB[0], sB[1],
                                        sC[0], sC[1], kw.get("splitk", 1), kw.get("precision", 0), int(kw.get("a_bf16", 0)),
                                        int(kw.get("epilogue", 0)), kw.get("a_mod16", 0), kw.get("b_mod16", 0), v)


def test_instance_list():
    assert len(set(C.INSTANCES)) == 12
    assert C.instance(128, 0, 1, 1) == "spe_gemm_kernel<128, false, true, true>" and C.instance(128, 0, 1, 1) in C.INSTANCES
    assert C.instance(64, 1, 1, 0) not in C.INSTANCES


@pytest.mark.parametrize("idx", range(len(C.PINNED)), ids=lambda i: f"{i}-" + "-".join(f"{k}{v}" for k, v in C.PINNED[i][0].items())[:60])
def test_pinned_choices(idx):
    """Written out by hand from the rules of csrc/gemm.hip and csrc/gemm_tiles.h (tests/f32_gemm_cases.py)."""
    kw, expected = C.PINNED[idx]
    plan = _plan(**kw)
    if isinstance(expected, int):
        assert plan is None and _status(**kw) == expected
        return
    assert _status(**kw) == 0 and plan is not None
    assert {k: plan[k] for k in expected} == expected, plan
    if plan["T"]:
        assert C.kernel_name(plan) in C.INSTANCES


def test_plan_never_leaves_the_instance_list():
    """Whatever the problem, the selection names one of the compiled instances or refuses with a known status; the splits it plans cover
    every k-tile; grid.x holds every tile."""
    seen = set()
    dims = (1, 64, 65, 129, 1025, 2049)
    for M, N, K_, (b0, b1), sk, (lay, (ta, tb)), prec in itertools.product(
            dims, dims, (1, 32, 40, 160, 2048), ((1, 1), (8, 8), (16, 16)), (1, 4, 7, 64, -4, -64), C.LAYOUTS.items(), (0, 1)):
        kw = dict(M=M, N=N, K=K_, batch0=b0, batch1=b1, splitk=sk, transA=ta, transB=tb, precision=prec,
                  sA=(b1 * M * K_, M * K_), sB=(b1 * N * K_, N * K_), sC=(b1 * M * N, M * N))
        plan = _plan(**kw)
        ktiles = -(-K_ // C.BK)
        if plan is None:                        # more slabs than k-tiles, nothing else in this sweep
            assert _status(**kw) == -5 and -sk > ktiles, kw
            continue
        assert C.kernel_name(plan) in C.INSTANCES, (kw, plan)
        assert (plan["TA"], plan["TB"], plan["SPLIT"]) == (ta, tb, prec)
        assert plan["splitk"] == min(abs(sk), ktiles) and plan["kt_per_split"] * plan["splitk"] >= ktiles, (kw, plan)
        assert (plan["slab"] != 0) == (sk < 0)
        T = plan["T"]
        t128 = -(-M // 128) * -(-N // 128) * b0 * b1 * plan["splitk"]
        assert T == (128 if t128 >= 256 and M > 64 and N > 64 else 64), (kw, plan)
        tm, tn = -(-M // T), -(-N // T)
        assert plan["xcd_bind"] in (0, 1, 2) and (plan["xcd_bind"] == 0) == (tm < 16 and tn < 16), (kw, plan)
        assert plan["grid_x"] == {0: tm * tn, 1: 8 * -(-tm // 8) * tn, 2: 8 * -(-tn // 8) * tm}[plan["xcd_bind"]], (kw, plan)
        seen.add(C.kernel_name(plan))
    assert seen == set(C.INSTANCES)             # and every instance is somebody's answer


def test_gpu_cases_reach_every_instance_in_every_state():
    """A condition on tests/f32_gemm_cases.py: for each of the 12 instances the GPU cases reach every state of REQUIRED (and M = 1 on the
    64-tile ones), each state computed by f32_gemm_cases.states from the launcher's own plan and the shape."""
    reached = {name: set() for name in C.INSTANCES}
    ids = set()
    for c in C.GPU_CASES:
        assert c["id"] not in ids
        ids.add(c["id"])
        plan = _plan(**C.plan_args(c))
        assert plan is not None, c["id"]
        assert plan["T"] == c["T"] and (plan["TA"], plan["TB"]) == C.LAYOUTS[c["layout"]] and plan["SPLIT"] == c["prec"], (c["id"], plan)
        a_vec_wanted, b_vec_wanted = c["a"] == "vec", c["b"] == "vec"
        assert (plan["vecA"], plan["vecB"]) == (a_vec_wanted, b_vec_wanted), (c["id"], plan)
        if c["splitk"] < 0:
            L = C.layout(c)["c"]                # the extent formula of kernels.gemm_splitk_into
            extent = (((c["b0"] - 1) * L["s0"] + (c["b1"] - 1) * L["s1"] + (c["M"] - 1) * L["ld"] + c["N"]) + 3) & ~3
            assert plan["slab"] == (c["M"] * L["ld"] if c["b0"] * c["b1"] == 1 else extent)
        reached[C.kernel_name(plan)] |= C.states(c, plan)
    for name in C.INSTANCES:
        need = C.REQUIRED | (C.REQUIRED_64_ONLY if "<64," in name else set())
        assert not need - reached[name], (name, sorted(need - reached[name]))
    # the operand kinds the exactness argument of the GPU test rests on, per instance
    for name in C.INSTANCES:
        split = name.endswith("true>")
        kinds = {c["ops"] for c in C.GPU_CASES if C.kernel_name(_plan(**C.plan_args(c))) == name}
        assert kinds >= ({"int", "both10", "random"} if split else {"int", "ties"}), (name, kinds)
        if "<64," in name:
            assert "random" in kinds


def test_hi_plus_lo_holds_every_16_bit_integer():
    """What the exactness of the SPLIT cases rests on: hi = bf16(x), lo = bf16(x - hi) reproduce every integer of up to 16 bits, |lo| <= 128;
    and the ties of the plain cases are ties: both bf16 neighbours are equally far, the rounding goes to the even one."""
    import torch
    x = torch.arange(-65535, 65536, dtype=torch.float32)
    hi = x.to(torch.bfloat16).float()
    lo = (x - hi).to(torch.bfloat16).float()
    assert torch.equal(hi + lo, x) and float(lo.abs().max()) == 128.0
    for p in (13, 14, 15):
        j = torch.arange(128, 256, dtype=torch.float32)
        t = (2 * j + 1) * 2.0 ** (p - 8)
        r = t.to(torch.bfloat16).float()
        assert bool(((r - t).abs() == 2.0 ** (p - 8)).all())                # half a bf16 step of binade p either way
        assert bool(((r / 2.0 ** (p - 7)) % 2 == 0).all())                  # ... resolved to the even significand


def test_random_bounds_hold_for_correct_arithmetic():
    """The element-wise bounds of the random-normal GPU cases, 2^-8 |A| |B| plain and (3 * 2^-18 + (K / 32 + 3) * 2^-24) |A| |B| SPLIT, against a
    torch emulation of the staging roundings on the very operands the GPU cases use: correct arithmetic stays inside (the figures go into
    profiles/f32_gemm_edges.txt)."""
    import torch
    import test_f32_gemm_gpu as G
    worst = {0: 0.0, 1: 0.0}
    for idx, c in enumerate(C.GPU_CASES):
        if c["ops"] != "random":
            continue
        A, B, _ = G._operands(c, 7919 * idx + 13)
        prod, _ = G._product(c, A, B)
        unit = (2.0 ** -8 if c["prec"] == 0 else 3 * 2.0 ** -18 + (c["K"] / 32 + 3) * 2.0 ** -24) * (A.abs() @ B.abs())
        worst[c["prec"]] = max(worst[c["prec"]], float(((prod - A @ B).abs() / unit).max()))
    print(f"F32GEMM random bounds, emulation: plain {worst[0]:.3f}, SPLIT {worst[1]:.3f}")
    assert 0 < worst[0] < 1 and 0 < worst[1] < 1, worst


def test_scalar_reasons_all_occur():
    """The three reasons for the scalar loaders - leading dimension, base address, batch stride - occur for A and for B at both tile sizes,
    and the exact-integer cases respect the contraction lengths their operand widths allow."""
    for T in (64, 128):
        for x in ("a", "b"):
            assert {t[x] for t in C.TEMPLATES[T]} >= {"vec", "ld", "off", "bs"}, (T, x)
        assert {t["c"] for t in C.TEMPLATES[T]} == {"vec", "ld", "off", "c2off", "sc0"}
        assert {t["epi"] for t in C.TEMPLATES[T]} == {"none", "bias", "relu", "gelu"}
    for c in C.GPU_CASES:
        if c["ops"] == "both10":
            assert c["K"] <= 15
        if c["ops"] == "ties":
            assert c["K"] < 64 and c["prec"] == 0
