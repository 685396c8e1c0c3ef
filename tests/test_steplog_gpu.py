"""The step-ledger kernels (csrc/step_ledger.hip) on the device against the numpy restatement (tests/steplog_ref.py) and the recorded
behaviour of the reference's MetricLogger (tests/golden/steplog_*.pt), and the public loop (spe_amd.engine) against the same loop
written out with per-key host reads.

spe_ledger_record / _total_bwd / _summary are called through the C ABI on buffers this file owns: longer than needed by a guard band
and pre-filled with NaN / 0xFF, so a store past the end shows; the bands are checked after every call.  Everything is compared
bitwise (NaN matching NaN); only `avg` uses the any-order summation bound (n - 1) 2^-24 sum|x| / n + 2^-24 |avg| the contract states."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import steplog_cases as cases
import steplog_ref as R
from steplog_cases import FMTS, WINDOWS, golden_step, load_golden, named, render, same_float

pytestmark = pytest.mark.gpu
GUARD = 64
OUT_FILL = -7.25
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Abi(object):
    """One ledger driven through the C ABI on guarded buffers."""

    def __init__(self, dev, K, E, mask, windows, state_bytes=None):
        from spe_amd import kernels as Kn, lib, steplog as S
        self.K, self.E, self.M, self.dev = K, E, 2 * K + 1 + E, dev
        self.lib, self.st = lib.load(), Kn._st
        self.nbytes = S.state_layout(max(min(K, 256), 1), max(min(E, 8), 0))["bytes"] if state_bytes is None else state_bytes
        self.state = torch.zeros((self.nbytes + GUARD,), dtype=torch.uint8, device=dev)
        self.state[self.nbytes:] = 0xFF
        n = max(K, 1)
        self.vals = torch.zeros((n,), dtype=torch.float32, device=dev)
        self.w = torch.zeros((n,), dtype=torch.float32, device=dev)
        self.mask = torch.from_numpy(np.resize(np.asarray(mask, np.uint8), n)).to(dev)
        self.total = torch.full((1 + GUARD,), float("nan"), dtype=torch.float32, device=dev)
        self.dvals = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev)
        self.out = torch.full((max(self.M, 1) * 5 + 2 + GUARD,), OUT_FILL, dtype=torch.float64, device=dev)
        self.win_host = torch.tensor(list(windows), dtype=torch.int32)
        self.win_dev = self.win_host.to(dev)

    def guards(self):
        torch.cuda.synchronize()
        assert bool((self.state[self.nbytes:] == 0xFF).all()), "state written past its end"
        assert bool(torch.isnan(self.total[1:]).all()), "total written past its end"
        assert bool(torch.isnan(self.dvals[max(self.K, 1):]).all()), "dvals written past its end"
        assert bool((self.out[max(self.M, 1) * 5 + 2:] == OUT_FILL).all()), "summary written past its end"

    def record(self, v, w, extras, expect=0):
        self.vals[:len(v)].copy_(torch.from_numpy(np.asarray(v, np.float32)))
        self.w[:len(w)].copy_(torch.from_numpy(np.asarray(w, np.float32)))
        ex = (ctypes.c_double * 8)(*[float(e) for e in extras][:8])
        rc = self.lib.spe_ledger_record(self.vals.data_ptr(), self.w.data_ptr(), self.mask.data_ptr(), ctypes.addressof(ex), self.K, self.E,
                                        self.state.data_ptr(), self.nbytes, self.total.data_ptr(), self.st())
        assert rc == expect, rc
        self.guards()
        return self.total[:1].cpu().numpy().view(np.int32)[0]

    def bwd(self, g, expect=0):
        gt = torch.tensor([g], dtype=torch.float32, device=self.dev)
        rc = self.lib.spe_ledger_total_bwd(gt.data_ptr(), self.w.data_ptr(), self.mask.data_ptr(), self.K, self.dvals.data_ptr(), self.st())
        assert rc == expect, rc
        self.guards()
        return self.dvals[:max(self.K, 1)].cpu().numpy()

    def summary(self, ring=None, order=None, expect=0):
        rc = self.lib.spe_ledger_summary(self.state.data_ptr(), self.nbytes, self.K, self.E, self.win_host.data_ptr(), self.win_dev.data_ptr(),
                                         None if ring is None else ring.data_ptr(), None if order is None else order.data_ptr(),
                                         self.out.data_ptr(), self.st())
        assert rc == expect, rc
        self.guards()
        o = self.out.cpu().numpy()
        return o[:self.M * 5].reshape(self.M, 5), o[self.M * 5], o[self.M * 5 + 1]

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.state[:self.nbytes] == 0).all()) and bool(torch.isnan(self.total).all()) and bool((self.out == OUT_FILL).all())


def check_table(tab, ref, K, mask):
    want = ref.table()
    rows = [i for i in range(len(want)) if not (K <= i < 2 * K and not mask[i - K])]
    for c, f in enumerate(R.FIELDS):
        if f == "avg":
            for i in rows:
                if tab[i, c] == want[i, c] or (np.isnan(tab[i, c]) and np.isnan(want[i, c])):       # (an infinite or NaN mean has no bound)
                    continue
                assert abs(tab[i, c] - want[i, c]) <= R.avg_bound(ref.series[i], ref.windows[i]), (i, tab[i, c], want[i, c])
        else:
            assert R.same_bits(tab[rows, c], want[rows, c]), (f, [(i, tab[i, c], want[i, c]) for i in rows
                                                                  if not R.same_bits(tab[i:i + 1, c], want[i:i + 1, c])][:5])


# every K, E and step count of steplog_cases.KS / ES / STEPS occurs; the windows cycle through WINS over the rows of every table
ABI_CASES = [(1, 0, 1), (2, 1, 2), (63, 8, 20), (64, 0, 21), (65, 1, 63), (255, 8, 64), (256, 1, 65), (256, 8, 130), (2, 0, 130), (64, 1, 64)]


def test_cases_cover_the_edges():
    assert {c[0] for c in ABI_CASES} == set(cases.KS) and {c[1] for c in ABI_CASES} == set(cases.ES)
    assert {c[2] for c in ABI_CASES} == set(cases.STEPS)


@pytest.mark.parametrize("K,E,steps", ABI_CASES)
def test_record_and_summary_c_abi(dev, K, E, steps):
    from spe_amd import kernels as Kn, steplog as S
    assert Kn.ledger_state_bytes(K, E) == S.state_layout(K, E)["bytes"]
    mask, run = cases.sequence(K, E, steps)
    win = cases.windows_for(K, E, seed=steps)
    a, ref = Abi(dev, K, E, mask, win), R.RefLedger(mask, win)
    for s, (v, w, ex) in enumerate(run):
        bits = a.record(v, w, ex)
        assert int(bits) == int(np.float32(ref.record(v, w, ex)).view(np.int32)), s
        if s + 1 in cases.STEPS or s + 1 == steps:
            tab, nsteps, bad = a.summary()
            assert nsteps == s + 1 and bad == 0
            check_table(tab, ref, K, mask)
    g = np.float32(0.37)
    dv = a.bwd(g)
    w = run[-1][1]
    assert R.same_bits(dv.astype(np.float64), np.where(mask, w * g, np.float32(0)).astype(np.float64))


def test_override_ring_and_order(dev):
    """The rank-averaged ring replaces the values (weights stay the state's) and `loss` is re-summed in the given key order."""
    K, E, steps = 65, 1, 70
    mask, run = cases.sequence(K, E, steps)
    win = cases.windows_for(K, E)
    order = np.random.default_rng(5).permutation(K).astype(np.int32)
    a, ref = Abi(dev, K, E, mask, win), R.RefLedger(mask, win, order=list(order))
    ring = torch.zeros((64, K), dtype=torch.float32, device=dev)
    for s, (v, w, ex) in enumerate(run):
        a.record(v, w, ex)
        other = (v * np.float32(1.5)).astype(np.float32)
        ring[s % 64] = torch.from_numpy(other).to(dev)
        ref.record(other, w, ex)
    tab, _, _ = a.summary(ring=ring, order=torch.from_numpy(order).to(dev))
    rows = [i for i in range(2 * K + 1 + E) if not (K <= i < 2 * K and not mask[i - K])]
    want = ref.table()
    for c in (0, 3, 4):                                   # median, max, value: the window's own; totals stay the local ones
        assert R.same_bits(tab[rows, c], want[rows, c]), c
    seq = R.RefLedger(mask, win)
    for v, w, ex in run:
        seq.record((v * np.float32(1.5)).astype(np.float32), w, ex)
    assert seq.series[2 * K] != ref.series[2 * K], "the permuted order must change some bits, or the order table is not tested"


def test_non_finite_and_stickiness(dev):
    K, E = 5, 1
    mask = np.array([True, False, True, True, False])
    win = [3] * (2 * K + 1 + E)
    a, ref = Abi(dev, K, E, mask, win), R.RefLedger(mask, win)
    w = np.float32([1, 0, 0, 2, 0])
    inf, nan = np.float32("inf"), np.float32("nan")
    rows = [[1, 2, 3, 4, 5], [1, nan, 3, 4, inf], [1, 2, 3, 4, 5], [1, 2, nan, 4, 5], [inf, 2, 3, 4, 5], [1, 2, 3, 4, 5], [1, 2, 3, 4, 5],
            [1, 2, 3, 4, 5]]
    bads = []
    for s, r in enumerate(rows):
        bits = a.record(np.float32(r), w, [0.5])
        t = ref.record(np.float32(r), w, [0.5])
        assert int(bits) == int(np.float32(t).view(np.int32)) or (np.isnan(t) and np.isnan(np.int32(bits).view(np.float32)))
        tab, nsteps, bad = a.summary()
        bads.append(int(bad))
        check_table(tab, ref, K, mask)
    # NaN / inf under unmasked keys (step 1) set nothing; 0 * NaN under a masked key (step 3) does; inf at step 4 does not replace it
    assert bads == [0, 0, 0, 4, 4, 4, 4, 4] and ref.bad == 3
    assert np.isnan(tab[:, 0]).sum() == 0                 # the last three steps are finite again: no NaN left in any window


@pytest.mark.parametrize("K,E,window,state_short,status", [(0, 0, 20, 0, -2), (257, 0, 20, 0, -2), (4, 9, 20, 0, -2), (4, -1, 20, 0, -2),
                                                           (4, 1, 0, 0, -2), (4, 1, 65, 0, -2), (4, 1, 20, 8, -4)])
def test_refusals_write_nothing(dev, K, E, window, state_short, status):
    from spe_amd import steplog as S
    Kc, Ec = max(min(K, 256), 1), max(min(E, 8), 0)
    nbytes = S.state_layout(Kc, Ec)["bytes"] - state_short
    a = Abi(dev, K, E, [1] * max(K, 1), [window] * max(2 * K + 1 + E, 1), state_bytes=nbytes)
    if window == 20:
        a.record(np.ones(max(K, 1), np.float32), np.ones(max(K, 1), np.float32), [0.0] * 8, expect=status)
    rc = a.lib.spe_ledger_summary(a.state.data_ptr(), a.nbytes, K, E, a.win_host.data_ptr(), a.win_dev.data_ptr(), None, None,
                                  a.out.data_ptr(), a.st())
    assert rc == status
    a.guards()
    assert a.untouched()
    if K in (0, 257):
        a.bwd(1.0, expect=-2)
        assert bool(torch.isnan(a.dvals).all())
    n = ctypes.c_size_t(7)
    assert a.lib.spe_ledger_state_bytes(K, E, ctypes.addressof(n)) == (0 if status == -4 or window != 20 else -2)


# ---- the class on the device ---------------------------------------------------------------------------------------------------
def _ledger():
    from spe_amd.steplog import StepLedger
    return StepLedger(windows=WINDOWS, window=20, fmts=FMTS, delimiter="  ")


def _run_golden(dev, g):
    led, bits, strs = _ledger(), [], {}
    for i, st in enumerate(g["steps"]):
        ld, wd, lr = golden_step(g["keys"], st)
        total = led.record({k: v.to(dev) for k, v in ld.items()}, wd, lr=lr)
        bits.append(total.detach().view(torch.int32))
        if i in g["snapshots"]:
            strs[i] = (str(led), led.summary())
    return led, torch.stack(bits).cpu(), strs


def test_ledger_reproduces_golden_and_is_deterministic(dev):
    g = load_golden("steplog_small")
    led, bits, strs = _run_golden(dev, g)
    assert torch.equal(bits, g["losses_bits"])
    for i, shot in g["snapshots"].items():
        assert strs[i][0] == shot["str"], i
        assert list(strs[i][1]) == list(shot["meters"])
        for n, five in shot["meters"].items():
            for f in ("median", "global_avg", "max", "value"):
                assert same_float(strs[i][1][n][f], five[f]), (i, n, f)
    ga = led.global_avg()
    assert list(ga) == list(g["global_avg"]) and all(same_float(ga[k], v) for k, v in g["global_avg"].items())
    led2, bits2, strs2 = _run_golden(dev, g)
    assert torch.equal(bits, bits2) and torch.equal(led.state, led2.state)
    assert {i: s[0] for i, s in strs.items()} == {i: s[0] for i, s in strs2.items()}


@pytest.mark.parametrize("name", ["inf_masked", "nan_unmasked", "zero_times_nan", "inf_minus_inf", "overflow", "finite"])
def test_ledger_edges_golden(dev, name):
    g = load_golden("steplog_edges")
    case = g["cases"][name]
    led = _ledger()
    for st in case["steps"]:
        ld, wd, lr = golden_step(g["keys"], st)
        led.record({k: v.to(dev) for k, v in ld.items()}, wd, lr=lr)
    if case["trip"] < 0:
        led.check()
        assert str(led) == case["str"]
    else:
        for _ in range(2):
            with pytest.raises(FloatingPointError) as e:
                led.check()
            assert e.value.args[1] == case["trip"]
        with pytest.raises(FloatingPointError):
            led.summary()


def test_record_does_not_synchronise(dev):
    """record() and the backward of its total read no device data on the host: under torch's sync debug mode any .item() / .cpu()
    would raise."""
    g = load_golden("steplog_small")
    led = _ledger()
    leaves = [st["values"].to(dev).requires_grad_() for st in g["steps"][:3]]
    feed = lambda i: led.record({k: leaves[i][j] for j, k in enumerate(g["keys"])}, dict(g["steps"][i]["weight_dict"]), lr=g["steps"][i]["lr"])
    feed(0).backward()                                   # first call: allocations, library load, the weight upload
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in (1, 2):
            feed(i).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    wd = g["steps"][2]["weight_dict"]
    want = torch.tensor([np.float32(wd.get(k, 0.0)) for k in g["keys"]])
    assert torch.equal(leaves[2].grad.cpu(), want)
    assert "loss:" in str(led)


# ---- the loop --------------------------------------------------------------------------------------------------------------------
def _to_dev(targets, dev):
    return [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in t.items()} for t in targets]


def _setup(blob, dev, flat):
    from spe_amd import kernels as Kn
    from spe_amd.dp import GradAllReducer
    from spe_amd.models import build_model
    from spe_amd.optim import FlatAdamW
    torch.manual_seed(11)
    Kn.manual_seed(11)
    args = argparse.Namespace(**blob["args"])
    args.device, args.num_classes, args.cam_thr, args.multi_box_ratio = "cuda", 20, 0.2, 0.5
    model, crit, crit_r, pp, rpp = build_model(args)
    model.load_state_dict(blob["state_dict"], strict=True)
    model, crit, crit_r = model.to(dev), crit.to(dev), crit_r.to(dev)
    named_p = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    groups = [{"params": [p for n, p in named_p if "backbone" not in n], "lr": 2e-3},
              {"params": [p for n, p in named_p if "backbone" in n], "lr": 5e-4}]
    red = None
    if flat:
        red = GradAllReducer([p for _, p in named_p], bucket_bytes=1 << 16, flatten_params=True)
        opt = FlatAdamW(groups, red, weight_decay=1e-2, max_grad_norm=0.1)
    else:
        opt = torch.optim.AdamW(groups, weight_decay=1e-2)
    return args, model, crit, crit_r, rpp, opt, red, named_p


def _loader(blob):
    from spe_amd.util.misc import NestedTensor
    g = torch.Generator().manual_seed(3)
    return [(NestedTensor(blob["tensors"] + 0.1 * i * torch.randn(blob["tensors"].shape, generator=g), blob["mask"]),
             [dict(t) for t in blob["targets"]]) for i in range(4)]


def _weighted_total(loss_dict, wd, dev):
    terms = [loss_dict[k] for k in loss_dict if k in wd]                 # bench.py's weighted_total: one stack, one product, one sum
    w = torch.tensor([float(wd[k]) for k in loss_dict if k in wd], dtype=torch.float32).to(dev)
    return (torch.stack(terms) * w).sum()


def _meters_of(line):
    m = re.search(r"eta: \S+  (.*)  time: ", line)
    return m.group(1) if m else None


@pytest.mark.parametrize("epoch,flat", [(6, False), (7, False), (15, True)])
def test_loop_equals_the_loop_with_host_reads(dev, capsys, epoch, flat):
    from spe_amd import camboxes, engine
    blob = torch.load(os.path.join(GOLD, "e2e_single.pt"), weights_only=False)
    max_norm = 0.1

    # (a) the public loop
    args, model, crit, crit_r, rpp, opt, red, named_p = _setup(blob, dev, flat)
    capsys.readouterr()
    stats = engine.train_one_epoch_refine(model, crit, _loader(blob), opt, dev, epoch, max_norm, args, rpp, crit_r)
    lines = capsys.readouterr().out.splitlines()
    if red is not None:
        red.remove()
    params_a = {n: p.detach().clone() for n, p in named_p}

    # (b) the same components, the total as bench.py forms it, every value read back with .item() into restated meters
    args, model, crit, crit_r, rpp, opt, red, named_p = _setup(blob, dev, flat)
    model.train(); crit.train(); crit_r.train()
    wd = engine.get_refine_weight_dict(dict(crit.weight_dict), args.num_refines, header="ref")
    ref, printed = None, []
    for i, (samples, targets) in enumerate(_loader(blob)):
        samples, targets = samples.to(dev), _to_dev(targets, dev)
        outputs = model(samples)
        for t, p in zip(targets, camboxes.get_pseudo_label_multi_boxes(outputs[0], samples, targets, args)):
            t.update(p)
        pseudo = engine.get_refinements_pseudo_label(outputs, samples, targets, args, rpp)
        loss_dict = crit(outputs[0], targets)
        for k, v in crit_r(outputs[1], pseudo[1]).items():
            loss_dict[f"ref_1_{k}"] = v
        engine.apply_curriculum(wd, epoch)
        total = _weighted_total(loss_dict, wd, dev)
        if flat:
            opt.zero_grad()
        else:
            opt.zero_grad(set_to_none=True)
        total.backward()
        if flat:
            red.finish()
        else:
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
        opt.step()
        keys = list(loss_dict)
        mask = [k in wd for k in keys]
        if ref is None:
            ref = R.RefLedger(mask, [20] * (2 * len(keys) + 1) + [1])
        ref.record(np.float32([loss_dict[k].item() for k in keys]), np.float32([wd.get(k, 0.0) for k in keys]), [opt.param_groups[0]["lr"]])
        if i in (0, 3):
            printed.append(named(ref.table(), keys, mask, ["lr"]))
    if red is not None:
        red.remove()
    params_b = {n: p.detach().clone() for n, p in named_p}

    assert len(keys) >= 20 and sum(mask) >= 10             # both criteria's keys, stage 1 under the ref_1_ prefix
    for n in params_a:
        assert torch.equal(params_a[n], params_b[n]), n
    order = ["lr", "class_error", "loss"] + [k for k, m in zip(keys, mask) if m] + [k + "_unscaled" for k in keys]
    want = named(ref.table(), keys, mask, ["lr"])
    assert list(stats) == order
    for n in order:
        assert same_float(stats[n], want[n]["global_avg"]), (n, stats[n], want[n]["global_avg"])
    got_lines = [m for m in (_meters_of(l) for l in lines) if m is not None]
    assert got_lines == [render(p, order) for p in printed]
    assert lines[-1] == "Averaged stats: " + render(want, order)
    nonzero = {k for k in keys if k in wd and wd[k] != 0.0}
    assert all(("img_label" in k) for k in nonzero) if epoch < 7 else (any("ref" in k for k in nonzero) == (epoch >= 15))
