"""The launch choices of the small-row Linear kernels (ls_plan in csrc/linear_small.hip through kernels.linear_small_plan; no GPU): the
hand-written choices it must make, its status codes, the coverage of the GPU test's cases (tests/linear_small_cases.py) and the torch
emulation of the kernels' roundings against the bounds the GPU test applies to the kernels."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_small_cases as C  # noqa: E402
import linear_small_ref as REF  # noqa: E402


def _plan(entry, **kw):
    from spe_amd import kernels as K
    return K.linear_small_plan(entry, **kw)


def plan_of_problem(entry, prob):
    if entry == "fwd":
        R, N, K_, sp = prob
        return _plan(entry, R=R, N=N, K=K_, split=sp)
    if entry == "bwd":
        R, N, K_, w = prob
        return _plan(entry, R=R, N=N, K=K_, dx="x" in w, dW="w" in w, db="b" in w)
    if entry == "group_fwd":
        R, nb, N, K_, sp = prob
        return _plan(entry, R=R, N=N, K=K_, nblk=nb, split=sp)
    R, nb, N, K_, dx, anyw = prob
    return _plan(entry, R=R, N=N, K=K_, nblk=nb, dx=dx, any_dw=anyw)


def plan_of_case(c):
    e = c["entry"]
    if e == "fwd":
        return _plan(e, R=c["R"], N=c["N"], K=c["K"], split=c["split"], ldx=c["K"] + (12 if "s" in c["flags"] else 0))
    if e == "bwd":
        return _plan(e, R=c["R"], N=c["N"], K=c["K"], dx="x" in c["wants"], dW="w" in c["wants"], db="b" in c["wants"])
    if e == "group_fwd":
        return _plan(e, R=c["R"], N=c["N"], K=c["K"], nblk=c["nblk"], split=c["split"], ldx=c["K"] + (12 if "s" in c["flags"] else 0))
    return _plan(e, R=c["R"], N=c["N"], K=c["K"], nblk=c["nblk"], dx=c["dx"], any_dw=C.any_dw(c))


ALL_CASES = [c for cs in C.GPU_CASES.values() for c in cs]


def test_instance_list():
    assert len(set(C.INSTANCES)) == 6 and len(set(C.STATES)) == len(C.STATES)
    assert len({c["id"] for c in ALL_CASES}) == len(ALL_CASES)


@pytest.mark.parametrize("entry,prob,inst,tdx,tdw", C.PINNED, ids=[f"{p[0]}-{'x'.join(map(str, p[1]))}" for p in C.PINNED])
def test_pinned_choices(entry, prob, inst, tdx, tdw):
    """Written out by hand from the four launchers as they stood before the choice became one function."""
    plan = plan_of_problem(entry, prob)
    assert plan["status"] == 0
    assert (plan["tiles_dx"], plan["tiles_dw"]) == (tdx, tdw)
    if inst is None:
        assert plan["grid_x"] == 0 and plan["KC"] == 0 and plan["lds_bytes"] == 0
        return
    assert inst in C.INSTANCES and C.kernel_name(entry, plan) == inst
    R = prob[0]
    if entry in ("fwd", "group_fwd"):
        cols = prob[1] if entry == "fwd" else prob[1] * prob[2]
        assert plan["grid_x"] == -(-R // 32) * -(-cols // 32) and plan["RC"] == 0
        assert plan["lds_bytes"] == (4 if plan["SPLIT"] else 2) * 32 * (plan["KC"] + 8) * 2
    else:
        assert plan["grid_x"] == tdx + tdw and plan["SPLIT"] == 0
        assert plan["lds_bytes"] == max(2 * 32 * (plan["KC"] + 8) * 2, 2 * plan["RC"] * 40 * 2 + 4096)


@pytest.mark.parametrize("c", ALL_CASES, ids=lambda c: c["id"])
def test_gpu_case_runs_where_the_arithmetic_says(c):
    """The plan's instance and tile counts for every GPU case equal what tests/linear_small_cases.py works out from the shape."""
    plan = plan_of_case(c)
    assert plan["status"] == 0
    tdx, tdw, grid = C.tiles_of(c)
    assert (plan["tiles_dx"], plan["tiles_dw"], plan["grid_x"]) == (tdx, tdw, grid)
    inst = C.instance_of(c)
    assert (C.kernel_name(c["entry"], plan) if grid else None) == inst
    assert all(s in C.STATES for s in C.states_of(c))


def test_gpu_cases_reach_every_instance_and_state():
    """A condition on tests/linear_small_cases.py: take a case away so that an instance or a named state is no longer reached, and this fails."""
    reached, insts = set(), {e: set() for e in C.GPU_CASES}
    for e, cs in C.GPU_CASES.items():
        for c in cs:
            reached |= set(C.states_of(c))
            insts[e].add(C.instance_of(c))
    missing = [s for s in C.STATES if s not in reached]
    assert not missing, missing
    assert insts["fwd"] == set(C.INSTANCES[:4]) and insts["group_fwd"] == set(C.INSTANCES[:4])
    assert insts["bwd"] == set(C.INSTANCES[4:]) | {None} and insts["group_bwd"] == set(C.INSTANCES[4:]) | {None}


def test_status_codes():
    """What the entries return for a shape they refuse (all but the pointer part of -2), and status 0 with an all-zero plan for nothing to do."""
    zero = dict(KC=0, RC=0, SPLIT=0, tiles_dx=0, tiles_dw=0, grid_x=0, lds_bytes=0)
    ok = dict(R=33, N=40, K=24)
    assert _plan("fwd", **ok)["status"] == 0 and _plan("bwd", dx=True, **ok)["status"] == 0
    for K_ in (0, -8, 4, 12, 25):                                     # K <= 0 or no multiple of 8
        assert _plan("fwd", R=33, N=40, K=K_, ldx=32)["status"] == -2, K_
        assert _plan("group_fwd", R=33, N=32, K=K_, nblk=2, ldx=32)["status"] == -2, K_
    for K_ in (4, 12, 25):
        assert _plan("bwd", R=33, N=40, K=K_, dx=True)["status"] == -2, K_
        assert _plan("group_bwd", R=33, N=128, K=K_, nblk=2, dx=True)["status"] == -2, K_
    for K_ in (0, -8):                                                # the backward entries call K <= 0 "nothing to do"
        assert _plan("bwd", R=33, N=40, K=K_, dx=True) == dict(zero, status=0)
        assert _plan("group_bwd", R=33, N=128, K=K_, nblk=2, dx=True) == dict(zero, status=0)
    for N in (4, 12, 41):                                             # the forward takes any N, the backward multiples of 8
        assert _plan("fwd", R=33, N=N, K=24)["status"] == 0, N
        assert _plan("bwd", R=33, N=N, K=24, dx=True)["status"] == -2, N
    for N in (8, 16, 48, 100):
        assert _plan("group_fwd", R=33, N=N, K=24, nblk=2)["status"] == -2, N
    for N in (32, 64, 96, 192, 200):
        assert _plan("group_bwd", R=33, N=N, K=24, nblk=2, dx=True)["status"] == -2, N
    assert _plan("group_fwd", R=33, N=96, K=24, nblk=2)["status"] == 0 and _plan("group_bwd", R=33, N=256, K=24, nblk=2, dx=True)["status"] == 0
    for ldx in (25, 26, 30):                                          # ldx no multiple of 4 (forward entries only have one)
        assert _plan("fwd", ldx=ldx, **ok)["status"] == -2, ldx
        assert _plan("group_fwd", R=33, N=32, K=24, nblk=2, ldx=ldx)["status"] == -2, ldx
    assert _plan("fwd", ldx=28, **ok)["status"] == 0
    for e in ("group_fwd", "group_bwd"):
        assert _plan(e, R=33, N=128, K=24, nblk=16, dx=True)["status"] == 0
        assert _plan(e, R=33, N=128, K=24, nblk=17, dx=True)["status"] == -2
    for e in C.GPU_CASES:                                             # nothing to do comes before every refusal
        for kw in (dict(R=0), dict(R=-1), dict(N=0), dict(N=-8)) + ((dict(nblk=0), dict(nblk=-1)) if e.startswith("group") else ()):
            args = dict(dict(R=33, N=128, K=12, nblk=17, ldx=13, dx=True), **kw)
            assert _plan(e, **args) == dict(zero, status=0), (e, kw)
    assert _plan("bwd", **ok) == dict(zero, status=0)                 # no output wanted
    assert _plan("group_bwd", R=33, N=128, K=24, nblk=2) == dict(zero, status=0)
    from spe_amd import lib
    import ctypes
    v = (ctypes.c_long * 7)()
    assert lib.load().spe_linear_small_plan(4, 33, 40, 24, 0, 24, 0, 0, 0, 0, 0, v) == -2 and list(v) == [0] * 7


def test_threshold_is_320():
    for e, kw in (("fwd", {}), ("group_fwd", dict(nblk=1))):
        assert _plan(e, R=5, N=10240, K=8, **kw)["KC"] == 384 and _plan(e, R=5, N=10272, K=8, **kw)["KC"] == 128
    assert _plan("bwd", R=1, N=10240, K=8, db=True)["RC"] == 512 and _plan("bwd", R=1, N=10272, K=8, db=True)["RC"] == 256
    assert _plan("group_bwd", R=33, N=384, K=32, nblk=16, dx=True, any_dw=True)["RC"] == 512       # 2 + 192
    assert _plan("group_bwd", R=33, N=384, K=64, nblk=16, dx=True, any_dw=True)["RC"] == 256       # 4 + 384
    assert _plan("group_bwd", R=33, N=128, K=8, nblk=1, dx=True, any_dw=True)["RC"] == 256         # N % 384 != 0


def test_rne_by_bits_is_torch_rne():
    g = torch.Generator().manual_seed(3)
    x = torch.randn((4096,), generator=g) * 2.0 ** torch.randint(-20, 20, (4096,), generator=g).float()
    assert torch.equal(REF.rne_bf16(x), x.to(torch.bfloat16).float())
    t, r = REF.ties_bf16(g, (512,))
    assert torch.equal(REF.rne_bf16(t.float()).double(), r) and torch.equal(t.float().to(torch.bfloat16).double(), r)
    assert bool(((t - r).abs() == 1).all()) and {int(v) for v in (t - r).unique()} == {-1, 1}      # half of them round up, half down


RANDOM = [c for c in ALL_CASES if "r" in c.get("flags", "")]


@pytest.mark.parametrize("c", RANDOM, ids=lambda c: c["id"])
def test_emulation_stays_inside_the_bounds(c):
    """The random-normal cases of the GPU test: the kernels' roundings, emulated with torch, stay inside the element-wise bounds derived
    in tests/linear_small_ref.py - before the kernels are asked to."""
    ops = REF.random_operands(c, "cpu")
    if c["entry"] == "fwd":
        x, Wh, Wl = ops
        ref, mag = (x.double() @ (Wh + (Wl if Wl is not None else 0)).t()), x.double().abs() @ (Wh + (Wl if Wl is not None else 0)).abs().t()
        emu = REF.emulate_nt(x, Wh, Wl).double()
        bound = REF.bound_split(mag, c["K"]) if c["split"] else REF.bound_plain(mag, c["K"])
        ratio = float(((emu - ref).abs() / bound).max())
        assert ratio <= 1.0, ratio
        return
    dy, x16, WT = ops
    r = REF.bwd_ref(dy.double(), None, 0, x16, WT)
    if "x" in c["wants"]:
        ref, emu = dy.double() @ WT.t(), REF.emulate_nt(dy, WT).double()
        assert float(((emu - ref).abs() / REF.bound_plain(r["mdx"], c["N"])).max()) <= 1.0
    if "w" in c["wants"]:
        ref, emu = dy.double().t() @ x16, REF.emulate_tn(dy, x16).double()
        assert float(((emu - ref).abs() / REF.bound_plain(r["mdw"], c["R"])).max()) <= 1.0
    if "b" in c["wants"]:
        emu = REF.emulate_db(dy).double()
        assert float(((emu - r["db"]).abs() / REF.bound_db(r["mdb"], c["R"])).max()) <= 1.0

