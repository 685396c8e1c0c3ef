"""spe_proposal_recall (csrc/proposal_recall.hip) on the device.

The entry point through the C ABI on buffers the test owns, with guard words on both sides of the counters, over every case of
tests/proposal_recall_cases.py: all counters equal the numpy restatement (tests/proposal_recall_ref.py) exactly, and a second run gives
the same bits.  The wrapper's refusals leave canary-filled counters alone.  ProposalRecallMeter.update under torch's sync debug mode:
one launch, no synchronising call, the CPU meter's counters.  Recall at k = 1 against spe_refine_pick + spe_pseudo_quality.  The stub
training loop and evaluate_det_voc on the device against a meter fed by hand."""
import numpy as np
import pytest
import torch

import proposal_recall_cases as Q
import proposal_recall_loops as PL
import proposal_recall_ref as R

pytestmark = pytest.mark.gpu


def _launch(dev, case):
    """One call on fresh buffers -> the counters as numpy int64 [rows, C + 1]; the guard words are checked here."""
    from spe_amd import kernels as K, lib
    words = case.rows * (case.C + 1)
    buf = torch.full((words + 2 * Q.GUARD_WORDS,), Q.GUARD, dtype=torch.int64, device=dev)
    counters = buf[Q.GUARD_WORDS:Q.GUARD_WORDS + words]
    if case.preload is None:
        counters.zero_()
    else:
        counters.copy_(torch.from_numpy(case.preload.reshape(-1)))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    prob, boxes, gboxes, glabels = up(case.prob), up(case.boxes), up(case.gboxes), up(case.glabels)
    hg, thr, ks = np.asarray(case.goff, np.int32), np.asarray(case.thr, np.float32), np.asarray(case.ks, np.int32)
    goff = up(hg)
    lib.call("spe_proposal_recall", K._p(prob), K._p(boxes), K._p(gboxes), K._p(glabels), K._p(goff), hg.ctypes.data, case.B, case.Q, case.Kc,
             int(hg[-1]), case.C, thr.ctypes.data, case.T, ks.ctypes.data, case.K, K._p(counters), K._st())
    host = buf.cpu()
    assert bool((host[:Q.GUARD_WORDS] == Q.GUARD).all()) and bool((host[Q.GUARD_WORDS + words:] == Q.GUARD).all()), case.name
    return host[Q.GUARD_WORDS:Q.GUARD_WORDS + words].numpy().reshape(case.rows, case.C + 1).copy()


@pytest.mark.parametrize("case", Q.cases(), ids=lambda c: c.name)
def test_counters_equal_the_restatement_and_two_runs_agree(dev, case):
    got = _launch(dev, case)
    want = case.expected()
    names = R.names(case.T, case.K)
    assert np.array_equal(got, want), {n: (got[k].tolist(), want[k].tolist()) for k, n in enumerate(names) if not np.array_equal(got[k], want[k])}
    assert np.array_equal(_launch(dev, case), got)                            # integer atomics only: the same bits


def test_wrapper_refuses_what_the_library_refuses(dev):
    from spe_amd import kernels as K, lib
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
    canary = 0x0123456789ABCDEF
    counters = torch.full((2 + 2 + 2 * 3, 4), canary, dtype=torch.int64, device=dev)
    goff = torch.tensor([0, 1], dtype=torch.int32, device=dev)

    def call(Q_=5, host=(0, 1), thr=(0.5, 0.75), ks=(1, 10, 100), C=3, prob=None, counters_=counters):
        return K.proposal_recall(z((1, Q_, 3), torch.float32) if prob is None else prob, z((1, Q_, 4), torch.float32), z((1, 4), torch.float32),
                                 z(1, torch.int64), goff, host, C, thr, ks, counters_)
    with pytest.raises(lib.SpeLibraryError, match="status -2"):
        call(Q_=1025)
    for kw in ({"host": (1, 1)}, {"thr": (0.75, 0.5)}, {"thr": (0.5, float("inf"))}, {"ks": (1, 1, 2)}, {"ks": (0, 1, 2)}):
        with pytest.raises(lib.SpeLibraryError, match="status -3"):
            call(**kw)
    with pytest.raises(lib.SpeLibraryError, match="status -3"):              # nine thresholds: the counters sized to fit, so the library answers
        call(thr=tuple(0.1 * i for i in range(1, 10)), counters_=torch.full((2 + 9 + 9 * 3, 4), canary, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="inconsistent shapes"):
        call(C=4)
    with pytest.raises(ValueError, match="inconsistent shapes"):
        call(ks=(1, 10))
    with pytest.raises(lib.SpeLibraryError):
        call(prob=torch.zeros(1, 5, 3))
    with pytest.raises(TypeError):
        call(prob=z((1, 5, 3), torch.float64))
    assert bool((counters == canary).all())                                  # nothing was written on any refusal
    call()
    got = counters.cpu() - canary
    assert got[0].tolist() == [1, 0, 0, 0] and not bool(got[1:].any())        # and the accepted call counts its one row (IoU 0 / 0: nothing else)


@pytest.mark.parametrize("name", ["q63", "q300", "nans", "saturated", "labels_c3"])
def test_update_is_one_launch_without_a_synchronising_call_and_equals_the_cpu_meter(dev, name):
    """Under torch's sync debug mode every synchronising call raises: update() makes none, and the library is entered exactly once."""
    from spe_amd import lib
    from spe_amd.evalmetrics import ProposalRecallMeter
    case = Q.by_name(name)
    outputs, gts = case.outputs(torch, dev), case.gts(torch, dev)
    make = lambda: ProposalRecallMeter(case.C, ["a", "b"], iou_threshs=case.thr, ks=case.ks)
    m = make()
    m.update("a", outputs, gts)                                               # first call: allocations, library load
    m.reset()
    m._state(dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for stage in ("a", "b", "b"):
            lib.count_launches(True)
            m.update(stage, outputs, gts)
            counts = lib.count_launches(False)
            assert counts == {"spe_proposal_recall": 1}, (stage, counts)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        lib.count_launches(False)
    cpu = make()
    for stage in ("a", "b", "b"):
        cpu.update(stage, case.outputs(torch, "cpu"), case.gts(torch, "cpu"))
    got = m.counters()
    assert m._counters.is_cuda and got.device.type == "cpu" and torch.equal(got, cpu.counters()) and torch.equal(2 * got[0], got[1])
    assert int(got[0, 2].sum()) > 0
    a, b = m.summarize(), cpu.summarize()
    for stage in ("a", "b"):
        for k in ("recall", "ceiling", "selection_gap", "mean_best_iou", "mean_recall"):
            assert np.array_equal(a[stage][k].numpy().view(np.int64), b[stage][k].numpy().view(np.int64)), (stage, k)
    assert str(m) == str(cpu)


def test_recall_at_1_is_the_covered_count_of_the_refine_picks_on_the_device(dev):
    """spe_refine_pick + spe_pseudo_quality against spe_proposal_recall at k = 1, and both against the CPU meters."""
    from test_proposal_recall_cpu import k1_identity
    pseudo, prop = k1_identity(dev)
    assert pseudo._counters.is_cuda and prop._counters.is_cuda
    cpu_pseudo, cpu_prop = k1_identity("cpu")
    assert torch.equal(prop.counters(), cpu_prop.counters()) and torch.equal(pseudo.counters(), cpu_pseudo.counters())


def test_training_loop_on_the_device_counts_what_the_host_composition_counts(dev, capsys):
    """The stub loop with the meter on the device: the statistics of the loop without one, bit for bit, and the counters of a meter fed
    by hand with what the model returned - through the host composition, over the probabilities the device computed."""
    plain = PL.run_epochs(dev)
    stats, params, meter, recorded, batches = PL.run_epochs(dev, PL.meter_factory)
    assert torch.equal(params, plain[1]) and list(stats) == list(plain[0]) + PL.stat_keys()
    for k in plain[0]:
        assert np.float64(stats[k]).view(np.int64) == np.float64(plain[0][k]).view(np.int64), k
    hand = PL.fed_by_hand(PL.meter_factory(), PL.last_epoch_updates(recorded, batches))
    want = hand.counters()
    assert meter._counters.is_cuda and recorded[0][0]["pred_logits"].is_cuda and torch.equal(meter.counters(), want)
    assert int(want[:, 2].sum()) > 0 and int(want[:, 4].sum()) > 0
    summary = hand.summarize()
    for stage in PL.STAGES:
        assert np.float64(stats[f"prop_{stage}_ceiling"]).view(np.int64) == np.float64(summary[stage]["mean_ceiling"][0].item()).view(np.int64)
    assert capsys.readouterr().out.count("Proposals [s0]") == 2


def test_training_loop_on_the_device_counts_what_the_cpu_loop_counts(dev, monkeypatch):
    """The loop on the device and the loop on CPU tensors - its prepare step, for which CPU tensors have no kernel, borrowed from the
    device - at a learning rate of 0, so that both sides see the same outputs at every step: the same counters."""
    from spe_amd import camboxes
    still = PL.run_epochs(dev, PL.meter_factory, lr=0.0)
    prepare = camboxes.K.cam_prepare
    monkeypatch.setattr(camboxes.K, "cam_prepare", lambda maps, rows, cols, thr: prepare(maps.to(dev), rows, cols, thr).cpu())
    camboxes.set_contours("host")                                             # CPU tensors take the host borders
    try:
        cpu = PL.run_epochs(torch.device("cpu"), PL.meter_factory, lr=0.0)
    finally:
        camboxes.set_contours("device")
        monkeypatch.undo()
    assert cpu[2]._counters.device.type == "cpu" and still[2]._counters.is_cuda and torch.equal(still[2].counters(), cpu[2].counters())


@pytest.mark.parametrize("flip", [False, True])
def test_evaluate_det_voc_on_the_device_counts_what_the_host_composition_counts(dev, flip):
    from test_proposal_recall_cpu import voc_loop
    out, lines, meter, hand = voc_loop(flip, dev)
    want = hand.counters()
    assert meter._counters.is_cuda and torch.equal(meter.counters(), want) and int(want[0, 2].sum()) > 0
    assert torch.equal(out["proposals"]["counters"], hand.summarize()["det"]["counters"]) and lines[-1] == str(hand)
    cpu_out, _, cpu_meter, _ = voc_loop(flip, torch.device("cpu"))
    assert torch.equal(cpu_meter.counters(), want)                            # and the loop on CPU tensors counts the same
