"""Host side of the pseudo-label quality meter: PseudoLabelMeter on CPU tensors against the numpy restatement
(tests/pseudo_quality_ref.py) over every case of tests/pseudo_quality_cases.py, its three input forms, the merge over two gloo ranks,
the argument checks of spe_pseudo_quality (host returns: nothing is launched), infer.pseudo_label_to_det_out against the recording of
the reference's function, and the training loop on the stub model with and without a meter."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pseudo_quality_cases as Q
import pseudo_quality_loops as L
import pseudo_quality_ref as R
import train_targets_cases as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pseudo_det_out.pt")


def _flat(case, with_scores=True):
    d = {"boxes": torch.from_numpy(case.boxes), "labels": torch.from_numpy(case.labels), "offsets": list(case.off)}
    if case.scores is not None and with_scores:
        d["scores"] = torch.from_numpy(case.scores)
    return d


def _meter(case, stages=("s",)):
    from spe_amd.evalmetrics import PseudoLabelMeter
    m = PseudoLabelMeter(case.C, list(stages), iou_thresh=case.thr)
    if case.preload is not None:
        m._state(torch.device("cpu"))[0].copy_(torch.from_numpy(case.preload))
    return m


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
def test_the_cases_reach_every_edge_they_are_listed_for():
    seen = Q.plan()
    assert seen["pseudo_counts"] >= set(Q.PSEUDO_COUNTS) and seen["gt_counts"] >= set(Q.GT_COUNTS), seen
    assert seen["B"] == set(Q.BATCHES) and seen["C"] == set(Q.CLASSES)
    assert seen["empty_at"] == {"first", "middle", "last"}
    assert seen["labels"] == seen["glabels"] == {"zero", "top", "below", "at_C"}
    assert seen["nan_coord"] == seen["inf_coord"] == {"pseudo", "gt"}
    for k in ("iou_one", "iou_touching", "iou_nan_zero_area", "iou_threshold_no_hit", "orphans", "pairs_empty",
              "gt_same_class", "equal_scores", "nan_score", "preload"):
        assert seen[k], k
    assert seen["rows_same_class"] == {False: True, True: True} and seen["lead_misses_later_hits"] == {False: True, True: True}
    assert len({c.name for c in Q.cases()}) == len(Q.cases())
    assert max(max(np.diff(c.off).max(), np.diff(c.goff).max()) for c in Q.cases()) == Q.LIMIT


def test_the_hand_made_rows_count_as_their_comments_say():
    """What the edge rows are for, read off the restatement's counters: class by class."""
    e = Q.by_name("edges").expected()
    col = lambda c: dict(zip(R.NAMES, e[:, c].tolist()))
    assert col(3) == {**col(3), "pairs": 1, "pairs_lead_hit": 1, "rows": 5, "rows_hit": 1, "rows_orphan": 1, "gts": 1, "gts_covered": 1, "iou_q": 1 << 20}
    assert col(4) == {**col(4), "rows_hit": 0, "iou_q": 0, "gts_covered": 0} and col(5) == {**col(5), "rows": 1, "rows_hit": 0, "rows_orphan": 0, "iou_q": 0}
    assert col(7)["rows_hit"] == 0 and col(7)["iou_q"] == 1 << 19 and col(7)["gts_covered"] == 0          # exactly the threshold: not a hit
    assert col(8)["rows_hit"] == 1 and col(8)["iou_q"] == (1 << 19) + (1 << 11) and col(8)["gts_covered"] == 1
    assert col(9) == {**col(9), "pairs": 0, "rows": 1, "rows_orphan": 1} and col(10) == {**col(10), "pairs": 1, "pairs_empty": 1, "rows": 0, "gts": 1}
    assert col(11) == {**col(11), "pairs": 1, "pairs_lead_hit": 1, "gts": 2, "gts_covered": 1}
    assert col(12) == {**col(12), "pairs": 1, "pairs_lead_hit": 0, "pairs_any_hit": 1, "rows": 2, "rows_hit": 1}
    assert col(6) == {**col(6), "pairs": 2, "rows": 1, "rows_hit": 1, "gts": 3, "gts_covered": 1}          # NaN and -inf ground-truth rows beside a good one
    assert e[4, 21] == 2 and e[7, 21] == 2 and e[:, 21].sum() == 4                                        # the dropped labels, and nothing else in column C
    lead = {k: Q.by_name("edges_" + k).expected()[1, 12] for k in ("equal", "nan", "best_last", "two_nans")}
    assert lead == {"equal": 0, "nan": 1, "best_last": 1, "two_nans": 0}


# ---- the meter against the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", Q.cases(), ids=lambda c: c.name)
def test_meter_on_cpu_tensors_equals_the_restatement(case):
    m = _meter(case)
    m.update("s", _flat(case), case.per_image(torch, "cpu")[1])
    want = case.expected()
    assert torch.equal(m.counters()[0], torch.from_numpy(want.copy()))
    out = m.summarize()["s"]
    assert torch.equal(out["counters"], torch.from_numpy(want[:, :case.C].copy()))
    assert out["dropped_rows"] == want[4, case.C] and out["dropped_gts"] == want[7, case.C]
    for name, (per, mean) in R.summary(want, case.C).items():
        got = out[name].numpy()
        assert got.dtype == np.float64 and np.array_equal(got.view(np.int64), per.view(np.int64)), name
        assert np.float64(out["mean_" + name]).view(np.int64) == np.float64(mean).view(np.int64), name
    line = str(m)
    assert line.count("\n") == 0 and "[s]" in line and all(w in line for w in ("CorLoc", "precision", "recall", "mean IoU"))


def test_summary_of_nothing_is_nan_and_reset_forgets():
    from spe_amd.evalmetrics import PseudoLabelMeter
    m = PseudoLabelMeter(3, ["a", "b"])
    out = m.summarize()
    assert list(out) == ["a", "b"] and all(np.isnan(out["a"]["mean_" + k]) for k in ("corloc", "any_hit", "precision", "recall", "mean_iou"))
    assert torch.isnan(out["b"]["corloc"]).all() and out["b"]["corloc"].shape == (3,)
    case = Q.by_name("one_class")
    m = _meter(case, stages=("x", "s"))
    m.update("s", _flat(case), case.per_image(torch, "cpu")[1])
    m.update("s", _flat(case), case.per_image(torch, "cpu")[1])
    assert torch.equal(m.counters()[1], torch.from_numpy(2 * case.expected())) and not m.counters()[0].any()
    m.update("s", [], [])                                                        # an empty batch: not an error, nothing counted
    assert torch.equal(m.counters()[1], torch.from_numpy(2 * case.expected()))
    m.reset()
    assert not m.counters().any()
    with pytest.raises(ValueError, match="unknown stage"):
        m.update("nope", [], [])
    with pytest.raises(ValueError):
        PseudoLabelMeter(0, ["a"])
    with pytest.raises(ValueError):
        PseudoLabelMeter(3, ["a", "a"])
    with pytest.raises(ValueError, match="images"):
        m.update("s", _flat(case), case.per_image(torch, "cpu")[1][:1])


@pytest.mark.parametrize("name", ["counts_a", "counts_a_scored", "edges_nan", "counts_c_scored"])
def test_the_three_input_forms_agree(name):
    from spe_amd.camboxes import PseudoTargets
    case = Q.by_name(name)
    per_image, gts = case.per_image(torch, "cpu")
    want = torch.from_numpy(case.expected().copy())
    flat, listed = _meter(case), _meter(case)
    flat.update("s", _flat(case), gts)
    listed.update("s", per_image, gts)
    assert torch.equal(flat.counters()[0], want) and torch.equal(listed.counters()[0], want)
    # a PseudoTargets carries no scores: it equals the two other forms without theirs
    pt = _meter(case)
    pt.update("s", PseudoTargets(torch.from_numpy(case.boxes), torch.from_numpy(case.labels), list(case.off), None), gts)
    bare_flat, bare_list = _meter(case), _meter(case)
    bare_flat.update("s", _flat(case, with_scores=False), gts)
    bare_list.update("s", [{k: v for k, v in p.items() if k != "scores"} for p in per_image], gts)
    bare = torch.from_numpy(R.quality(case.boxes, case.labels, None, case.off, case.gboxes, case.glabels, case.goff, case.C, case.thr, case.preload))
    assert torch.equal(pt.counters()[0], bare) and torch.equal(bare_flat.counters()[0], bare) and torch.equal(bare_list.counters()[0], bare)
    if case.scores is not None:
        assert not torch.equal(bare, want)                                        # the scores move the lead rows of these cases


def test_more_rows_than_the_limit_are_refused_on_cpu_tensors_too():
    from spe_amd.evalmetrics import PseudoLabelMeter
    m = PseudoLabelMeter(3, ["s"])
    n = Q.LIMIT + 1
    many = {"boxes": torch.rand(n, 4), "labels": torch.zeros(n, dtype=torch.int64)}
    few = {"boxes": torch.rand(1, 4), "labels": torch.zeros(1, dtype=torch.int64)}
    with pytest.raises(ValueError, match="at most"):
        m.update("s", [many], [few])
    with pytest.raises(ValueError, match="at most"):
        m.update("s", [few], [many])


# ---- two ranks over gloo ---------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


_MERGE_CASES = ("counts_a_scored", "edges")                                     # both C = 21: one meter, two stages


def _worker(rank, world, port, out):
    from spe_amd.evalmetrics import PseudoLabelMeter
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = PseudoLabelMeter(21, ["x", "y", "unused"], iou_thresh=Q.THRESH)
    for stage, name in zip(("x", "y"), _MERGE_CASES):
        case = Q.by_name(name)
        pseudo, gts = case.per_image(torch, "cpu")
        mine = [b for b in range(len(gts)) if (b * 3 + 1) % world == rank]       # an uneven split; rank 1 has nothing of "edges"
        m.update(stage, [pseudo[b] for b in mine], [gts[b] for b in mine])
    m.merge()
    out[rank] = m.counters().numpy()
    dist.barrier()
    dist.destroy_process_group()


def test_merge_over_gloo_world2_gives_the_single_process_counters():
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    res = dict(out)
    for rank in range(world):
        for s, name in enumerate(_MERGE_CASES):
            assert np.array_equal(res[rank][s], Q.by_name(name).expected()), (rank, name)
        assert not res[rank][2].any()


# ---- the entry point refuses on the host ----------------------------------------------------------------------------------------------
def test_entry_point_refuses_on_the_host():
    """The launcher looks at the shapes and at both host offset vectors before anything is launched: -2 for a limit, -3 for arguments."""
    import ctypes
    from spe_amd import lib
    Lb = lib.load()
    one = ctypes.c_void_p(256)                                               # a non-NULL address that is never touched

    def pq(off, goff, C=21, B=None, T=None, G=None, counters=one, boxes=one, gboxes=one, dev_off=one, host=(True, True)):
        ho, hg = np.asarray(off, np.int32), np.asarray(goff, np.int32)
        B = len(off) - 1 if B is None else B
        return Lb.spe_pseudo_quality(boxes, one, None, dev_off, gboxes, one, one, ho.ctypes.data if host[0] else None,
                                     hg.ctypes.data if host[1] else None, B, off[-1] if T is None else T, goff[-1] if G is None else G, C,
                                     0.5, counters, None)
    assert pq([0, 1025], [0, 1]) == -2 and pq([0, 1], [0, 1025]) == -2 and pq([0, 3, 3 + 1025], [0, 0, 1]) == -2
    assert pq([0, 0], [0, 0]) == 0 and pq([0], [0]) == 0                     # T = G = 0 and an empty batch: valid, nothing launched
    assert pq([0, 1], [0, 1], C=0) == -3 and pq([0, 1], [0, 1], C=-4) == -3
    assert pq([1, 1], [0, 1]) == -3 and pq([0, 2, 1], [0, 1, 1]) == -3 and pq([0, 1], [0, 2, 1, 1], B=1) == -3      # start, descent, end
    assert pq([0, 1], [0, 1], T=2) == -3 and pq([0, 1], [0, 1], G=0) == -3 and pq([0, 1], [0, 1], B=-1) == -3
    assert pq([0, 1], [0, 1], counters=None) == -3 and pq([0, 1], [0, 1], boxes=None) == -3 and pq([0, 1], [0, 1], gboxes=None) == -3
    assert pq([0, 1], [0, 1], dev_off=None) == -3
    assert pq([0, 1], [0, 1], host=(False, True)) == -3 and pq([0, 1], [0, 1], host=(True, False)) == -3
    assert Lb.spe_abi_version() == 7 and len(lib.PROTOS["spe_pseudo_quality"]) == 16
    assert len(lib.PROTOS["spe_refine_pick"]) == 14 and len(lib.PROTOS["spe_cam_targets"]) == 12              # the neighbours keep their signatures


# ---- pseudo_label_to_det_out -----------------------------------------------------------------------------------------------------------
def test_pseudo_label_to_det_out_equals_the_reference_recording():
    from spe_amd import infer
    from spe_amd.evalmetrics import VOCDetectionMeter
    rec = torch.load(GOLDEN)
    for key in ("sizes_int", "sizes_float"):
        got = infer.pseudo_label_to_det_out([dict(p) for p in rec["pseudo"]], rec[key])
        assert len(got) == len(rec["out_" + key]) == 4
        for a, b in zip(got, rec["out_" + key]):
            assert sorted(a) == sorted(b) == ["boxes", "labels", "scores"]
            for k in a:
                assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (key, k)
            assert a["scores"].dtype == torch.int64 and bool((a["scores"] == 1).all()) and bool((a["boxes"] >= 0).all())
    # and the list is what a detection meter takes
    got = infer.pseudo_label_to_det_out(rec["pseudo"], rec["sizes_float"])
    meter = VOCDetectionMeter(num_classes=20)
    meter.update(got, [{"boxes": r["boxes"].double(), "labels": r["labels"], "difficult": torch.zeros_like(r["labels"], dtype=torch.uint8),
                        "image_id": torch.tensor(i)} for i, r in enumerate(got)])
    out = meter.summarize()
    assert int(np.asarray(out["npos"]).sum()) == sum(r["labels"].numel() for r in got)            # every row was taken, under its label


# ---- the training loop -------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def host_contours(monkeypatch):
    """The "host" contours with a stand-in for the device's prepare step, as tests/test_train_targets_cpu.py has it: CPU tensors have no
    resize kernel, and what the maps become is not the subject here."""
    from spe_amd import camboxes

    def prepare(maps, rows, cols, cam_thr):
        big = torch.nn.functional.interpolate(maps[:, None], size=(rows, cols), mode="bilinear", align_corners=False)[:, 0]
        lo, hi = big.amin((1, 2), keepdim=True), big.amax((1, 2), keepdim=True)
        q = ((big - lo) / (hi - lo) * 255).to(torch.uint8)
        return torch.where(q > int(cam_thr * 255), q, torch.zeros_like(q))
    monkeypatch.setattr(camboxes.K, "cam_prepare", prepare)
    camboxes.set_contours("host")
    yield camboxes
    camboxes.set_contours("device")


class _Trap:
    """Tensor.item / Tensor.tolist raise while the batch loop runs - from the model's first call until the loader is exhausted.  Let
    through by name is what reads by design on CPU tensors: the ledger's log line, the "host" contours' box lists and presence lists,
    torch.max's host pick, and the meter's host composition of the kernel.  What the loop itself gained for the meter is not among them."""

    def __init__(self, monkeypatch):
        from spe_amd import camboxes, evalmetrics, infer
        from spe_amd.steplog import SmoothedValue, StepLedger
        self.on, self.steps = False, 0

        def guard(fn):
            def guarded(t, *a, **k):
                if self.on:
                    raise AssertionError("host read of a tensor inside the batch loop")
                return fn(t, *a, **k)
            return guarded

        def free(fn):
            def freed(*a, **k):
                was, self.on = self.on, False
                try:
                    return fn(*a, **k)
                finally:
                    self.on = was
            return freed
        monkeypatch.setattr(torch.Tensor, "item", guard(torch.Tensor.item))
        monkeypatch.setattr(torch.Tensor, "tolist", guard(torch.Tensor.tolist))
        monkeypatch.setattr(StepLedger, "summary", free(StepLedger.summary))
        monkeypatch.setattr(SmoothedValue, "__str__", free(SmoothedValue.__str__))
        for mod, name in ((camboxes, "pseudo_targets"), (camboxes, "present_lists"), (infer, "_refine_pick_host"),
                          (evalmetrics, "_pseudo_quality_host")):
            monkeypatch.setattr(mod, name, free(getattr(mod, name)))

    def arm(self, engine, monkeypatch):
        """The trap is on between the first forward and the end of the loader."""
        trap, real = self, engine.StepLedger.log_every

        def log_every(ledger, loader, *a, **k):
            for item in real(ledger, loader, *a, **k):
                trap.on = True
                trap.steps += 1
                yield item
            trap.on = False
        monkeypatch.setattr(engine.StepLedger, "log_every", log_every)


def _same_bits(a, b):
    return np.float64(a).view(np.int64) == np.float64(b).view(np.int64)


def test_loop_with_a_meter_keeps_its_statistics_and_counts_what_the_criteria_saw(host_contours, monkeypatch, capsys):
    from spe_amd import engine
    from spe_amd.evalmetrics import PseudoLabelMeter
    cpu = torch.device("cpu")
    plain_stats, plain_params, none, _, _, _ = L.run_epochs(cpu)
    parent_stats, parent_params = T.run_parent_epochs(cpu)
    capsys.readouterr()
    trap = _Trap(monkeypatch)
    trap.arm(engine, monkeypatch)
    stats, params, meter, crit, crit_r, batches = L.run_epochs(cpu, lambda: PseudoLabelMeter(L.NUM_CLASSES, L.STAGES))
    printed = capsys.readouterr().out
    assert not trap.on and trap.steps == 2 * 3                                # armed at every step of both epochs, off after the loader
    trap.on = True                                                            # the trap itself works
    with pytest.raises(AssertionError, match="host read"):
        torch.zeros(1).item()
    trap.on = False
    monkeypatch.undo()
    # without a meter: the parent commit's loop, whatever else the targets carry
    assert none is None and list(plain_stats) == list(parent_stats) and torch.equal(plain_params, parent_params)
    assert all(_same_bits(plain_stats[k], parent_stats[k]) for k in plain_stats)
    # with a meter: the same losses and parameters, and the new keys behind the old ones
    new = [f"pseudo_{s}_{k}" for s in L.STAGES for k in ("corloc", "precision", "recall", "mean_iou")]
    assert list(stats) == list(plain_stats) + new and torch.equal(params, plain_params)
    assert all(_same_bits(stats[k], plain_stats[k]) for k in plain_stats)
    want = L.expected_counters(crit, crit_r, batches)
    assert torch.equal(meter.counters(), torch.from_numpy(want))
    assert want[:, 0].sum() > 0 and want[:, 4, :L.NUM_CLASSES].sum() > 0 and want[0, 7, L.NUM_CLASSES] > 0      # pairs, rows, a dropped ground-truth label
    for s, stage in enumerate(L.STAGES):
        ref = R.summary(want[s], L.NUM_CLASSES)
        for k in ("corloc", "precision", "recall", "mean_iou"):
            assert _same_bits(stats[f"pseudo_{stage}_{k}"], ref[k][1]) or (np.isnan(stats[f"pseudo_{stage}_{k}"]) and np.isnan(ref[k][1])), (stage, k)
        assert f"Pseudo labels [{stage}]: CorLoc" in printed
    assert printed.count("Pseudo labels [") == 2 * len(L.STAGES)              # one block per epoch


def test_loop_with_a_meter_names_the_missing_key(host_contours, capsys):
    from spe_amd import engine
    from spe_amd.evalmetrics import PseudoLabelMeter
    from spe_amd.models.conditional_detr import PostProcessRefine
    batches = T.stub_batches(1)                                               # the stub's own targets: no ground-truth rows
    model = T.StubModel(batches)
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    with pytest.raises(ValueError, match="'boxes'"):
        engine.train_one_epoch_refine(model, T.StubCriterion(), T.stub_loader(batches), opt, torch.device("cpu"), T.STUB_EPOCH, 0.1, T.stub_args(),
                                      {"bbox": PostProcessRefine()}, T.StubCriterion(), pseudo_meter=PseudoLabelMeter(L.NUM_CLASSES, L.STAGES))
    import inspect
    for fn in (engine.train_one_epoch_refine, engine.train_one_epoch_refine_coco):
        names = list(inspect.signature(fn).parameters)
        assert names[-1] == "pseudo_meter" and inspect.signature(fn).parameters["pseudo_meter"].default is None
