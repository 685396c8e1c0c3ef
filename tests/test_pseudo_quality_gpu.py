"""spe_pseudo_quality (csrc/pseudo_quality.hip) on the device.

The entry point through the C ABI on buffers the test owns, with guard words on both sides of the counters, over every case of
tests/pseudo_quality_cases.py: all counters equal the numpy restatement (tests/pseudo_quality_ref.py) exactly, and a second run gives
the same bits.  PseudoLabelMeter.update under torch's sync debug mode: one launch, no synchronising call; the device meter against the
CPU meter; the stub training loop on the device against the loop on CPU tensors."""
import numpy as np
import pytest
import torch

import pseudo_quality_cases as Q
import pseudo_quality_loops as L

pytestmark = pytest.mark.gpu


def _launch(dev, case, with_scores=True):
    """One call on fresh buffers -> the counters as numpy int64 [10, C + 1]; the guard words are checked here."""
    from spe_amd import kernels as K, lib
    C, words = case.C, 10 * (case.C + 1)
    buf = torch.full((words + 2 * Q.GUARD_WORDS,), Q.GUARD, dtype=torch.int64, device=dev)
    counters = buf[Q.GUARD_WORDS:Q.GUARD_WORDS + words]
    if case.preload is None:
        counters.zero_()
    else:
        counters.copy_(torch.from_numpy(case.preload.reshape(-1)))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    boxes, labels, gboxes, glabels = up(case.boxes), up(case.labels), up(case.gboxes), up(case.glabels)
    scores = up(case.scores) if (case.scores is not None and with_scores) else None
    ho, hg = np.asarray(case.off, np.int32), np.asarray(case.goff, np.int32)
    off, goff = up(ho), up(hg)
    lib.call("spe_pseudo_quality", K._p(boxes), K._p(labels), K._p(scores), K._p(off), K._p(gboxes), K._p(glabels), K._p(goff), ho.ctypes.data,
             hg.ctypes.data, len(ho) - 1, int(ho[-1]), int(hg[-1]), C, float(case.thr), K._p(counters), K._st())
    host = buf.cpu()
    assert bool((host[:Q.GUARD_WORDS] == Q.GUARD).all()) and bool((host[Q.GUARD_WORDS + words:] == Q.GUARD).all()), case.name
    return host[Q.GUARD_WORDS:Q.GUARD_WORDS + words].numpy().reshape(10, C + 1).copy()


@pytest.mark.parametrize("case", Q.cases(), ids=lambda c: c.name)
def test_counters_equal_the_restatement_and_two_runs_agree(dev, case):
    got = _launch(dev, case)
    want = case.expected()
    assert np.array_equal(got, want), {n: (got[k].tolist(), want[k].tolist()) for k, n in enumerate(Q.R.NAMES) if not np.array_equal(got[k], want[k])}
    assert np.array_equal(_launch(dev, case), got)                            # integer atomics only: the same bits


def test_wrapper_refuses_what_the_library_refuses(dev):
    from spe_amd import kernels as K, lib
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
    n = Q.LIMIT + 1
    off, goff = torch.tensor([0, n], dtype=torch.int32, device=dev), torch.tensor([0, 1], dtype=torch.int32, device=dev)
    counters = z((10, 4), torch.int64)
    with pytest.raises(lib.SpeLibraryError, match="status -2"):
        K.pseudo_quality(z((n, 4), torch.float32), z(n, torch.int64), None, off, z((1, 4), torch.float32), z(1, torch.int64), goff,
                         ([0, n], [0, 1]), 3, 0.5, counters)
    with pytest.raises(lib.SpeLibraryError, match="status -3"):
        K.pseudo_quality(z((1, 4), torch.float32), z(1, torch.int64), None, goff, z((1, 4), torch.float32), z(1, torch.int64), goff,
                         ([0, 1], [1, 1]), 3, 0.5, counters)
    with pytest.raises(ValueError):
        K.pseudo_quality(z((1, 4), torch.float32), z(1, torch.int64), None, goff, z((1, 4), torch.float32), z(1, torch.int64), goff,
                         ([0, 1], [0, 1]), 4, 0.5, counters)
    with pytest.raises(lib.SpeLibraryError):
        K.pseudo_quality(z((1, 4), torch.float32).cpu(), z(1, torch.int64), None, goff, z((1, 4), torch.float32), z(1, torch.int64), goff,
                         ([0, 1], [0, 1]), 3, 0.5, counters)
    assert not bool(counters.any())


@pytest.mark.parametrize("name", ["counts_a_scored", "edges_nan", "counts_c_scored", "full"])
def test_update_is_one_launch_without_a_synchronising_call_and_equals_the_cpu_meter(dev, name):
    """Under torch's sync debug mode every synchronising call raises: update() makes none, in any of the three input forms, and the
    library is entered exactly once per update."""
    from spe_amd import lib
    from spe_amd.camboxes import PseudoTargets
    from spe_amd.evalmetrics import PseudoLabelMeter
    case = Q.by_name(name)
    pseudo, gts = case.per_image(torch, dev)
    flat = {"boxes": torch.cat([p["boxes"] for p in pseudo]), "labels": torch.cat([p["labels"] for p in pseudo]), "offsets": list(case.off)}
    if case.scores is not None:
        flat["scores"] = torch.cat([p["scores"] for p in pseudo])
    forms = {"list": pseudo, "flat": flat, "targets": PseudoTargets(flat["boxes"], flat["labels"], list(case.off), None)}
    stages = list(forms)
    m = PseudoLabelMeter(case.C, stages, iou_thresh=case.thr)
    m.update("list", pseudo, gts)                                             # first call: allocations, library load
    m.reset()
    m._state(dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for stage, form in forms.items():
            lib.count_launches(True)
            m.update(stage, form, gts)
            counts = lib.count_launches(False)
            assert counts == {"spe_pseudo_quality": 1}, (stage, counts)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        lib.count_launches(False)
    cpu = PseudoLabelMeter(case.C, stages, iou_thresh=case.thr)
    cpseudo, cgts = case.per_image(torch, "cpu")
    cflat = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in flat.items()}
    for stage, form in (("list", cpseudo), ("flat", cflat), ("targets", PseudoTargets(cflat["boxes"], cflat["labels"], list(case.off), None))):
        cpu.update(stage, form, cgts)
    got = m.counters()
    assert got.device.type == "cpu" and torch.equal(got, cpu.counters())
    if case.preload is None:
        assert torch.equal(got[0], torch.from_numpy(case.expected().copy())) and torch.equal(got[0], got[1])
    a, b = m.summarize(), cpu.summarize()
    for stage in stages:
        for k in ("corloc", "any_hit", "precision", "recall", "mean_iou"):
            assert np.array_equal(a[stage][k].numpy().view(np.int64), b[stage][k].numpy().view(np.int64)), (stage, k)
    assert str(m) == str(cpu)


def test_loop_on_the_device_counts_what_the_cpu_loop_counts(dev, monkeypatch, capsys):
    """The stub loop with a meter on the device: the statistics of the loop without one, bit for bit, and the counters of the
    restatement over the rows the criteria were given.  Then the loop on CPU tensors - its prepare step, for which CPU tensors have no
    kernel, borrowed from the device - at a learning rate of 0, so that both sides see the same rows at every step: the same counters."""
    from spe_amd import camboxes
    from spe_amd.evalmetrics import PseudoLabelMeter
    factory = lambda: PseudoLabelMeter(L.NUM_CLASSES, L.STAGES)
    plain = L.run_epochs(dev)
    stats, params, meter, crit, crit_r, batches = L.run_epochs(dev, factory)
    assert torch.equal(params, plain[1]) and list(stats)[:len(plain[0])] == list(plain[0]) and len(stats) == len(plain[0]) + 4 * len(L.STAGES)
    for k in plain[0]:
        assert np.float64(stats[k]).view(np.int64) == np.float64(plain[0][k]).view(np.int64), k
    want = torch.from_numpy(L.expected_counters(crit, crit_r, batches))
    assert meter._counters.is_cuda and torch.equal(meter.counters(), want)
    assert int(want[:, 0].sum()) > 0 and int(want[:, 4].sum()) > 0
    still = L.run_epochs(dev, factory, lr=0.0)
    prepare = camboxes.K.cam_prepare
    monkeypatch.setattr(camboxes.K, "cam_prepare", lambda maps, rows, cols, thr: prepare(maps.to(dev), rows, cols, thr).cpu())
    camboxes.set_contours("host")                                             # CPU tensors take the host borders: the same boxes in the same order
    try:
        cpu = L.run_epochs(torch.device("cpu"), factory, lr=0.0)
    finally:
        camboxes.set_contours("device")
        monkeypatch.undo()
    assert cpu[2]._counters.device.type == "cpu" and torch.equal(still[2].counters(), cpu[2].counters())
    assert torch.equal(still[2].counters(), torch.from_numpy(L.expected_counters(still[3], still[4], still[5])))
    assert capsys.readouterr().out.count("Pseudo labels [cam]") == 6
