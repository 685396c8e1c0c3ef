"""The step ledger without a GPU: the numpy restatement (tests/steplog_ref.py) and spe_amd.steplog.StepLedger on CPU tensors against
the recorded behaviour of the reference's MetricLogger (tests/golden/steplog_small.pt, steplog_edges.pt; tools/gen_steplog_golden.py).

Equalities at world 1: str(ledger), median, global_avg, max and value of every meter and the bits of the weighted total are the
reference's.  `avg` is the reference's float32 mean in whatever order torch adds; it is held to the any-order summation bound
(n - 1) 2^-24 sum|x| / n + 2^-24 |avg| (steplog_ref.avg_bound).  World 2 over gloo: see test_gloo_world2."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import steplog_cases as cases
import steplog_ref as R
from steplog_cases import FMTS, WINDOWS, golden_step, load_golden, named, render, same_float

EXACT = ("median", "global_avg", "max", "value")


def _ledger():
    from spe_amd.steplog import StepLedger
    return StepLedger(windows=WINDOWS, window=20, fmts=FMTS, delimiter="  ")


def _check_meters(got, want, avg_tol):
    assert list(got) == list(want), (list(got), list(want))
    for name in want:
        for f in EXACT:
            assert same_float(got[name][f], want[name][f]), (name, f, got[name][f], want[name][f])
        assert abs(got[name]["avg"] - want[name]["avg"]) <= avg_tol(name), (name, got[name]["avg"], want[name]["avg"])


def _ref_run(g):
    keys = g["keys"]
    mask = [k in g["steps"][0]["weight_dict"] for k in keys]
    K = len(keys)
    win = [20] * (2 * K + 1) + [1]
    ref = R.RefLedger(mask, win)
    return keys, mask, ref


def _avg_tol(ref, keys, mask):
    """per-meter bound for avg: the any-order summation bound of the contract, steplog_ref.avg_bound, once."""
    K = len(keys)
    rows = {"loss": 2 * K, "lr": 2 * K + 1}
    for i, k in enumerate(keys):
        rows[k + "_unscaled"] = i
        if mask[i]:
            rows[k] = K + i

    def tol(name):
        if name == "class_error":
            return 0.0
        return R.avg_bound(ref.series[rows[name]], ref.windows[rows[name]])
    return tol


def test_restatement_reproduces_small_golden():
    g = load_golden("steplog_small")
    keys, mask, ref = _ref_run(g)
    for i, st in enumerate(g["steps"]):
        w = np.float32([st["weight_dict"].get(k, 0.0) for k in keys])
        t = ref.record(st["values"].numpy(), w, [st["lr"]])
        assert int(np.float32(t).view(np.int32)) == int(g["losses_bits"][i]), i
        if i in g["snapshots"]:
            shot = g["snapshots"][i]
            got = named(ref.table(), keys, mask, ["lr"])
            got = {n: got[n] for n in shot["meters"]}
            _check_meters(got, shot["meters"], _avg_tol(ref, keys, mask))
            assert render(got, list(shot["meters"])) == shot["str"]
    assert ref.bad is None


def test_ledger_cpu_reproduces_small_golden():
    g = load_golden("steplog_small")
    keys, mask, ref = _ref_run(g)
    led = _ledger()
    for i, st in enumerate(g["steps"]):
        ld, wd, lr = golden_step(keys, st)
        total = led.record(ld, wd, lr=lr)
        ref.record(st["values"].numpy(), np.float32([wd.get(k, 0.0) for k in keys]), [lr])
        assert total.ndim == 0 and int(total.detach().view(torch.int32)) == int(g["losses_bits"][i]), i
        if i in g["snapshots"]:
            shot = g["snapshots"][i]
            assert str(led) == shot["str"], i
            _check_meters(led.summary(), shot["meters"], _avg_tol(ref, keys, mask))
    ga = led.global_avg()
    assert list(ga) == list(g["global_avg"])
    for k, v in g["global_avg"].items():
        assert same_float(ga[k], v), k
    led.check()


@pytest.mark.parametrize("name", ["inf_masked", "nan_unmasked", "zero_times_nan", "inf_minus_inf", "overflow", "finite"])
def test_edges_golden(name):
    g = load_golden("steplog_edges")
    keys, case = g["keys"], g["cases"][name]
    mask = [k in case["steps"][0]["weight_dict"] for k in keys]
    ref, led = R.RefLedger(mask, [20] * (2 * len(keys) + 1) + [1]), _ledger()
    for i, st in enumerate(case["steps"]):
        ld, wd, lr = golden_step(keys, st)
        t = ref.record(st["values"].numpy(), np.float32([wd.get(k, 0.0) for k in keys]), [lr])
        total = led.record(ld, wd, lr=lr)
        if i < len(case["losses_bits"]):
            want = int(case["losses_bits"][i])
            for got in (int(np.float32(t).view(np.int32)), int(total.detach().view(torch.int32))):
                assert got == want or (np.isnan(np.int32(got).view(np.float32)) and np.isnan(np.int32(want).view(np.float32))), i
    assert (-1 if ref.bad is None else ref.bad) == case["trip"]
    if case["trip"] < 0:
        led.check()
        assert str(led) == case["str"]
        if name == "nan_unmasked":
            assert "nan" in str(led)
    else:
        for _ in range(2):                                # sticky: the finite steps after it did not clear it
            with pytest.raises(FloatingPointError) as e:
                led.check()
            assert e.value.args[1] == case["trip"]
            assert e.value.args[2] is not None and list(e.value.args[2]) == keys
        with pytest.raises(FloatingPointError):
            str(led)


def test_gradient_is_the_weight():
    keys = ["a", "class_error", "b", "c"]
    wd = {"a": 2.0, "b": 0.3, "c": 0.0}
    leaves = {k: torch.tensor(float(i + 1), requires_grad=True) for i, k in enumerate(keys)}
    led = _ledger()
    total = led.record({k: v * 1.0 for k, v in leaves.items()}, wd, lr=1e-4)
    assert total.requires_grad
    total.backward()
    for k in keys:
        if k in wd:
            assert torch.equal(leaves[k].grad, torch.tensor(np.float32(wd[k])))
        else:
            assert leaves[k].grad is None


def test_refusals():
    from spe_amd.steplog import StepLedger
    one = lambda: torch.tensor(1.0)
    led = _ledger()
    led.record({"a": one(), "b": one()}, {"a": 1.0}, lr=0.1)
    with pytest.raises(ValueError):
        led.record({"b": one(), "a": one()}, {"a": 1.0}, lr=0.1)                 # another key sequence
    with pytest.raises(ValueError):
        led.record({"a": one()}, {"a": 1.0}, lr=0.1)
    with pytest.raises(ValueError):
        led.record({"a": one(), "b": one()}, {"a": 1.0, "b": 1.0}, lr=0.1)       # another set of weighted keys
    with pytest.raises(ValueError):
        _ledger().record({"k%d" % i: one() for i in range(257)}, {"k0": 1.0})
    _ledger().record({"k%d" % i: one() for i in range(256)}, {"k0": 1.0})
    with pytest.raises(ValueError):
        StepLedger(windows={"lr": 65})
    with pytest.raises(ValueError):
        StepLedger(window=0)
    StepLedger(windows={"lr": 64})
    with pytest.raises(ValueError):
        _ledger().record({"a": one()}, {"a": 1.0}, **{"e%d" % i: 0.0 for i in range(9)})
    _ledger().record({"a": one()}, {"a": 1.0}, **{"e%d" % i: 0.0 for i in range(8)})


def test_entry_points_refuse_null_pointers_on_the_host():
    """The validation runs on the host before any launch, so it is checked here without a device: every required pointer, one at a
    time, as NULL -> -2 (the state: -4).  The other arguments are valid, the non-NULL pointers are host buffers nobody follows."""
    import ctypes
    from spe_amd import lib, steplog as S
    L = lib.load()
    K, E = 4, 1
    nbytes = S.state_layout(K, E)["bytes"]
    buf = (ctypes.c_double * (nbytes // 8 + 64))()
    p = ctypes.addressof(buf)
    win = (ctypes.c_int * (2 * K + 1 + E))(*([20] * (2 * K + 1 + E)))
    w = ctypes.addressof(win)
    rec = [p, p, p, p, K, E, p, nbytes, p, None]
    for i in (0, 1, 2, 3, 8):
        a = list(rec)
        a[i] = None
        assert L.spe_ledger_record(*a) == -2, i
    a = list(rec)
    a[6] = None
    assert L.spe_ledger_record(*a) == -4
    bwd = [p, p, p, K, p, None]
    for i in (0, 1, 2, 4):
        a = list(bwd)
        a[i] = None
        assert L.spe_ledger_total_bwd(*a) == -2, i
    summ = [p, nbytes, K, E, w, w, None, None, p, None]
    for i in (4, 5, 8):
        a = list(summ)
        a[i] = None
        assert L.spe_ledger_summary(*a) == -2, i
    a = list(summ)
    a[0] = None
    assert L.spe_ledger_summary(*a) == -4
    assert L.spe_ledger_state_bytes(K, E, None) == -2
    assert not any(buf)                                   # nothing was written


def test_engine_weight_helpers_against_literal_dicts():
    """get_refine_weight_dict and the epoch curriculum (reference engine.py:107-109, 134-142, 260-268) against dicts written out by
    hand: the GPU loop test takes these helpers from spe_amd.engine on both sides, so their content is pinned here."""
    from spe_amd import engine
    base = {"loss_ce": 2, "loss_bbox": 5, "img_label_logits": 1, "drloc_x": 0.5, "loss_ce_0": 2}
    wd = dict(base)
    assert engine.get_refine_weight_dict(wd, 2, header="ref") is wd
    full = {"loss_ce": 2, "loss_bbox": 5, "img_label_logits": 1, "drloc_x": 0.5, "loss_ce_0": 2,
            "ref_1_loss_ce": 2, "ref_1_loss_bbox": 5, "ref_1_img_label_logits": 1, "ref_1_drloc_x": 0.5, "ref_1_loss_ce_0": 2,
            "ref_2_loss_ce": 2, "ref_2_loss_bbox": 5, "ref_2_img_label_logits": 1, "ref_2_drloc_x": 0.5, "ref_2_loss_ce_0": 2}
    assert wd == full and list(wd) == list(full)
    assert engine.get_refine_weight_dict({"a": 3}, 0) == {"a": 3}
    assert engine.get_refine_weight_dict({"a": 3}, 1) == {"a": 3, "rf_1_a": 3}              # the reference's default header
    zeros = {k: 0.0 for k in full}
    want = {6: dict(zeros, img_label_logits=1, drloc_x=0.5),                                # the refine copies of both are zeroed by < 15
            0: dict(zeros, img_label_logits=1, drloc_x=0.5),
            7: dict(full, **{k: 0.0 for k in full if k.startswith("ref_")}),
            14: dict(full, **{k: 0.0 for k in full if k.startswith("ref_")}),
            15: dict(full), 40: dict(full)}
    for epoch, expect in want.items():
        got = dict(full)
        assert engine.apply_curriculum(got, epoch) is got
        assert got == expect and list(got) == list(full), epoch
        assert engine.apply_curriculum(dict(got), epoch) == expect                          # applied every step: idempotent


def test_engine_refinement_targets():
    """get_refinements_pseudo_label (engine.py:271-308): stage k's detections become stage k + 1's targets, up to num_refines; the
    other target fields are kept and the loader's dicts are not written to."""
    import argparse
    from spe_amd import engine
    calls = []

    def post(outputs, sizes, targets):
        calls.append((outputs, sizes.tolist()))
        return [{"labels": torch.tensor([outputs, i]), "boxes": torch.full((2, 4), float(outputs)), "scores": torch.tensor([0.5, 0.25])}
                for i in range(len(targets))]
    targets = [{"boxes": torch.zeros(1, 4), "labels": torch.tensor([9]), "orig_size": torch.tensor([64, 96]), "img_label": torch.tensor([1, 0])},
               {"boxes": torch.ones(3, 4), "labels": torch.tensor([1, 2, 3]), "orig_size": torch.tensor([48, 80]), "img_label": torch.tensor([0, 1])}]
    for num_refines, stages in ((1, [1]), (2, [1, 2])):
        calls.clear()
        out = engine.get_refinements_pseudo_label({0: 10, 1: 11, 2: 12}, None, targets, argparse.Namespace(num_refines=num_refines), {"bbox": post})
        assert list(out) == stages and [c[0] for c in calls] == [10 + s - 1 for s in stages]
        assert all(c[1] == [[64, 96], [48, 80]] for c in calls)
        for s in stages:
            for i, p in enumerate(out[s]):
                assert set(p) == {"boxes", "labels", "orig_size", "img_label", "scores"}
                assert p["labels"].tolist() == [10 + s - 1, i] and torch.equal(p["boxes"], torch.full((2, 4), float(10 + s - 1)))
                assert p["scores"].tolist() == [0.5, 0.25] and p["img_label"] is targets[i]["img_label"]
    assert targets[0]["labels"].tolist() == [9] and "scores" not in targets[0]


def test_k256_tells_the_summation_orders_apart():
    """The order test shows something only if another order gives other bits: at K = 256 the pairwise sum differs from the sequential
    one in at least one step of the sequence the GPU test uses."""
    mask, run = cases.sequence(256, 1, 20)
    diff = sum(int(np.float32(R.seq_total(v, w, mask)).view(np.int32) != np.float32(R.tree_total(v, w, mask)).view(np.int32))
               for v, w, _ in run)
    assert diff >= 1


@pytest.mark.parametrize("K,E,steps", [(1, 0, 1), (2, 1, 21), (65, 8, 65), (256, 1, 130)])
def test_host_path_equals_restatement(K, E, steps):
    """summary_host / record_host (the ring, the state block) against the list-based restatement, bit for bit - avg included, both
    add in order."""
    from spe_amd import steplog as S
    mask, run = cases.sequence(K, E, steps)
    win = cases.windows_for(K, E)
    ref = R.RefLedger(mask, win)
    state = torch.zeros((S.state_layout(K, E)["bytes"],), dtype=torch.uint8)
    m8 = torch.from_numpy(mask.astype(np.uint8))
    for v, w, ex in run:
        t = S.record_host(torch.from_numpy(v), torch.from_numpy(w), m8, ex, state)
        assert int(t.view(torch.int32)) == int(np.float32(ref.record(v, w, ex)).view(np.int32))
    tab = S.summary_host(state, K, E, win).numpy()
    M = 2 * K + 1 + E
    want = ref.table()
    rows = [i for i in range(M) if not (K <= i < 2 * K and not mask[i - K])]
    assert R.same_bits(tab[:M * 5].reshape(M, 5)[rows], want[rows])
    assert tab[M * 5] == steps and tab[M * 5 + 1] == 0


# ---- two processes over gloo --------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


W2_KEYS = ["zeta", "class_error", "alpha", "mid", "beta"]          # insertion order is not sorted order
W2_WD = {"zeta": 2.0, "alpha": 0.3, "mid": 5.0, "beta": 1.0}


def _w2_values(rank, steps=30):
    rng = np.random.default_rng(900 + rank)
    return [(10.0 ** rng.uniform(-3, 3, len(W2_KEYS)) * rng.uniform(0.5, 1.5, len(W2_KEYS))).astype(np.float32) for _ in range(steps)]


def _worker(rank, world, port, out, nan_on_rank1):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        led = _ledger()
        vals = _w2_values(rank)
        if nan_on_rank1 and rank == 1:
            vals[7][0] = np.float32("nan")
        for v in vals:
            led.record({k: torch.tensor(v[j]) for j, k in enumerate(W2_KEYS)}, W2_WD, lr=1e-4)
        try:
            out[rank] = ("ok", led.summary(), str(led))
        except FloatingPointError as e:
            out[rank] = ("bad", e.args[1], None)
    finally:
        dist.destroy_process_group()


def test_gloo_world2():
    """Against the reference's rule applied to the per-step rank means: reduce_dict (sum, / world in fp32, keys sorted), the scaled
    products of the means, `loss` summed in SORTED key order, SmoothedValue over them.  median / value / max: exact.
    global_avg: the reference adds the fp32-rounded mean per step, the ledger adds every rank's own values and divides the all-reduced
    total.  Every meter is held to the contract's 2^-23 relative (losses are non-negative); lr is a host scalar and exact."""
    world = 2
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), out, False), nprocs=world, join=True)
    res = dict(out)
    assert res[0][0] == res[1][0] == "ok"
    assert res[0][2] == res[1][2]                                    # both ranks print the same line
    K = len(W2_KEYS)
    mask = [k in W2_WD for k in W2_KEYS]
    order = sorted(range(K), key=lambda i: W2_KEYS[i])
    ref = R.RefLedger(mask, [20] * (2 * K + 1) + [1], order=order)
    w = np.float32([W2_WD.get(k, 0.0) for k in W2_KEYS])
    for a, b in zip(_w2_values(0), _w2_values(1)):
        ref.record((a + b) / np.float32(2), w, [1e-4])
    want = named(ref.table(), W2_KEYS, mask, ["lr"], sort_keys=True)
    got = res[0][1]
    names = ["lr", "class_error", "loss"] + [W2_KEYS[i] for i in order if mask[i]] + [W2_KEYS[i] + "_unscaled" for i in order]
    assert list(got) == names                                        # sorted key order, as reduce_dict rebuilds the dict
    for n in names:
        for f in ("median", "value", "max"):
            assert same_float(got[n][f], want[n][f]), (n, f, got[n][f], want[n][f])
        if n == "lr":
            assert same_float(got[n]["global_avg"], want[n]["global_avg"])
        else:
            rel = abs(got[n]["global_avg"] - want[n]["global_avg"]) / abs(want[n]["global_avg"])
            print("global_avg %s: %.3f x 2^-23" % (n, rel * 2.0 ** 23))
            assert rel <= 2.0 ** -23, (n, rel)
    # the order matters: with the keys in insertion order `loss` has other bits in at least one step
    ins = R.RefLedger(mask, [20] * (2 * K + 1) + [1])
    for a, b in zip(_w2_values(0), _w2_values(1)):
        ins.record((a + b) / np.float32(2), w, [1e-4])
    assert ins.series[2 * K] != ref.series[2 * K]


def test_gloo_world2_both_ranks_raise():
    world = 2
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), out, True), nprocs=world, join=True)
    assert dict(out) == {0: ("bad", 7, None), 1: ("bad", 7, None)}
