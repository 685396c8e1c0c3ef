"""ProposalRecallMeter and spe_proposal_recall without a GPU (csrc/proposal_recall.hip): the cases reach what they
are listed for, the hand-made rows count what their comments say, the meter's host composition equals the numpy restatement
(tests/proposal_recall_ref.py) on every case, recall at k = 1 is PseudoLabelMeter's covered count over PostProcessRefine's picks, the
header and every host refusal of the entry point, the ValueErrors, the world-2 merge over gloo, the summary's NaN rules, and the
training and evaluation loops with and without the meter."""
import contextlib
import io
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import detect_loops as D
import proposal_recall_cases as Q
import proposal_recall_loops as PL
import proposal_recall_ref as R
import pseudo_quality_loops as L
import train_targets_cases as T
import voc_eval_cases


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def test_the_cases_reach_every_edge_they_are_listed_for():
    plan = Q.plan()
    assert {1, 63, 64, 65, 300, 1024} <= plan["Q"] and {0, 1, 5, 257} <= plan["rows"] and 1 in plan["B"]
    assert {(1, 1), (2, 3), (8, 8)} <= plan["TK"]
    assert plan["empty_between"] and plan["ks_1_Q_Q5"] and plan["C_below_Kc"] and plan["preload"]
    by = Q.by_name
    p = by("ties").prob
    assert any(len(np.unique(p[b, :, c])) < p.shape[1] // 4 for b in range(p.shape[0]) for c in range(p.shape[2]))       # runs of equal values
    z = by("zeros").prob
    assert bool((np.signbit(z) & (z == 0)).any()) and bool((~np.signbit(z) & (z == 0)).any())                            # both zeros
    assert int(np.isnan(by("nans").prob[0, :, 0]).sum()) > 1 and bool((by("saturated").prob == 1).all())
    w = by("wild")
    assert np.isnan(w.boxes).any() and np.isinf(w.boxes).any() and np.isnan(w.gboxes).any()
    assert bool((w.boxes[:, :, 2:] == 0).all(-1).any()) and bool((w.gboxes[:, 2:] == 0).all(-1).any())
    assert bool((w.boxes[0, 0] == w.gboxes[0]).all())                                                                    # identical to its ground truth
    assert {-1, 5, 8} <= set(by("labels").glabels.tolist()) and by("labels").Kc == 5 and by("labels").C == 8
    for c in Q.cases():
        want = c.expected()
        base = np.zeros_like(want) if c.preload is None else c.preload
        G = c.goff[-1]
        assert int((want - base)[0].sum()) == G, c.name                                                                  # every row is counted once
        if c.empty:
            assert G == 0 and np.array_equal(want, base)
            continue
        d = (want - base)[:, :c.C]
        assert d[0].sum() > 0 and d[1].sum() > 0 and d[2].sum() > 0 and d[2 + c.T:].sum() > 0, c.name                    # rows, IoUs, ceiling, hits
    big = Q.by_name("q300").expected()
    assert (big[2, :21] > big[4, :21]).any() and big[4, :21].sum() > 0                                                   # ceil[0] > hit[0][0] > 0 somewhere


def test_the_hand_made_rows_count_as_their_comments_say():
    case = Q.by_name("hand")
    want = Q.hand_expected()
    assert np.array_equal(case.expected(), want), (case.expected().tolist(), want.tolist())
    iou = R.P.iou_matrix(case.gboxes[:2], np.stack([case.boxes[0, 0], case.boxes[1, 2]]))
    assert iou[0, 0] == np.float32(0.5) and iou[1, 1] == np.float32(0.75)                                                # exactly the thresholds
    assert want[2, 1] == 1 and want[3, 1] == 0                                                                           # 0.75 covers at 0.5 only; 0.5 nowhere
    assert want[2, 2] > want[4, 2] > 0                                                                                   # the selection gap of class 2
    assert R.names(2, 4)[4] == "hit[0][0]" and len(R.names(2, 4)) == want.shape[0]


def test_the_order_is_total_and_starts_with_the_pick():
    p = np.float32([0.5, np.nan, 0.75, -0.0, 0.75, np.nan, 0.0, np.inf])
    assert R.positions(p) == [5, 0, 3, 6, 4, 1, 7, 2]                                                                    # NaNs, inf, 0.75 twice, 0.5, -0.0 before +0.0 by index
    for col in (np.float32([0.25, 0.75, 0.75]), np.float32([0.25, np.nan, 0.9, np.nan]), np.float32([1.0, 1.0])):
        first = R.positions(col).index(0)
        assert first == int(torch.from_numpy(col).max(dim=0).indices)                                                    # torch.max's pick


@pytest.mark.parametrize("case", Q.cases(), ids=lambda c: c.name)
def test_host_composition_equals_the_restatement(case):
    from spe_amd import evalmetrics, kernels as K
    counters = torch.zeros((case.rows, case.C + 1), dtype=torch.int64) if case.preload is None else torch.from_numpy(case.preload.copy())
    thr, ks = evalmetrics._proposal_tables("test", case.thr, case.ks)
    evalmetrics._proposal_recall_host(torch.from_numpy(case.prob), torch.from_numpy(case.boxes), torch.from_numpy(case.gboxes),
                                      torch.from_numpy(case.glabels), case.goff, case.C, thr, ks, counters)
    got, want = counters.numpy(), case.expected()
    rows = K.proposal_recall_counters(case.T, case.K)
    assert list(rows) == R.names(case.T, case.K)
    assert np.array_equal(got, want), {n: (got[k].tolist(), want[k].tolist()) for k, n in enumerate(rows) if not np.array_equal(got[k], want[k])}


@pytest.mark.parametrize("name", ["q63", "ties", "nans", "saturated", "labels_c3"])
def test_meter_on_cpu_tensors_orders_by_its_own_sigmoid(name):
    from spe_amd.evalmetrics import ProposalRecallMeter
    case = Q.by_name(name)
    outputs, gts = case.outputs(torch, "cpu"), case.gts(torch, "cpu")
    m = ProposalRecallMeter(case.C, ["a", "b"], iou_threshs=case.thr, ks=case.ks)
    m.update("b", outputs, gts)
    m.update("b", outputs, gts)
    want = R.recall(outputs["pred_logits"].sigmoid().numpy(), case.boxes, case.gboxes, case.glabels, case.goff, case.C, case.thr, case.ks)
    got = m.counters()
    assert got.shape == (2, case.rows, case.C + 1) and not bool(got[0].any()) and np.array_equal(got[1].numpy(), 2 * want)


# ---- k = 1 is the refine pick ----------------------------------------------------------------------------------------------------------
def k1_inputs(device):
    g = np.random.default_rng(77)
    Kc = 6
    prob, boxes, gboxes, glabels, goff = Q.random_batch(g, 2, 65, Kc, Kc, (5, 40))
    case = Q.Case("k1", Kc, (prob, boxes, gboxes, glabels, goff), (0.5,), (1,))
    outputs, gts = case.outputs(torch, device), case.gts(torch, device)
    classes = [sorted({int(l) for l in t["labels"].tolist() if 0 <= l < Kc}) for t in case.gts(torch, "cpu")]
    return case, outputs, gts, classes


def k1_identity(device):
    """With class lists equal to each image's ground-truth label set, hit[0.5][k = 1] is PseudoLabelMeter's gts_covered over the rows of
    infer.refine_targets, and gts equals gts - dropped labels included.  -> the two meters."""
    from spe_amd import infer
    from spe_amd.evalmetrics import ProposalRecallMeter, PseudoLabelMeter
    case, outputs, gts, classes = k1_inputs(device)
    pseudo, prop = PseudoLabelMeter(case.C, ["s"], iou_thresh=0.5), ProposalRecallMeter(case.C, ["s"], iou_threshs=(0.5,), ks=(1,))
    pseudo.update("s", infer.refine_targets(outputs, classes), gts)
    prop.update("s", outputs, gts)
    a, b = pseudo.counters()[0], prop.counters()[0]
    assert torch.equal(a[7], b[0]) and torch.equal(a[8], b[3]) and int(b[3].sum()) > 0 and int(b[0, case.C]) > 0
    assert int(b[2].sum()) > int(b[3].sum())                                    # the ceiling lies above: the identity is not trivial
    return pseudo, prop


def test_recall_at_1_is_the_covered_count_of_the_refine_picks():
    k1_identity("cpu")


# ---- the entry point refuses on the host ----------------------------------------------------------------------------------------------
def test_header_prototype_and_every_host_refusal():
    import ctypes
    from spe_amd import kernels as K, lib
    sig = lib.PROTOS["spe_proposal_recall"]
    assert [n for _, n in sig] == ["prob", "boxes", "gboxes", "glabels", "goff", "goff_host", "B", "Q", "Kc", "G", "C", "thr", "T", "ks", "K",
                                   "counters", "stream"] and len(sig) == 17
    Lb = lib.load()
    assert Lb.spe_abi_version() == 7 and len(lib.PROTOS["spe_pseudo_quality"]) == 16 and len(lib.PROTOS["spe_refine_pick"]) == 14
    assert K.PROPOSAL_RECALL_MAX_Q == 1024 and K.PROPOSAL_RECALL_IOU_SCALE == 1 << 20
    one = ctypes.c_void_p(256)                                               # a non-NULL address that is never touched

    def pr(goff=(0, 1), Q_=5, Kc=3, C=3, thr=(0.5, 0.75), ks=(1, 10), B=None, G=None, T=None, K_=None, host=True, tables=(True, True),
           counters=one, prob=one, boxes=one, gboxes=one, glabels=one, dev_off=one):
        hg, th, kk = np.asarray(goff, np.int32), np.asarray(thr, np.float32), np.asarray(ks, np.int32)
        return Lb.spe_proposal_recall(prob, boxes, gboxes, glabels, dev_off, hg.ctypes.data if host else None,
                                      len(goff) - 1 if B is None else B, Q_, Kc, goff[-1] if G is None else G, C,
                                      th.ctypes.data if tables[0] else None, len(thr) if T is None else T,
                                      kk.ctypes.data if tables[1] else None, len(ks) if K_ is None else K_, counters, None)
    assert pr(Q_=1025) == -2 and pr(Q_=4096) == -2                           # the LDS staging
    assert pr(goff=(0, 0)) == 0 and pr(goff=(0,)) == 0 and pr(goff=(0, 0, 0)) == 0                    # G = 0, B = 0: valid, nothing launched
    assert pr(goff=(0, 0), prob=None, boxes=None, gboxes=None, glabels=None, dev_off=None) == 0       # and nothing is needed for it
    assert pr(Q_=0) == -3 and pr(Kc=0) == -3 and pr(C=0) == -3 and pr(C=-2) == -3 and pr(B=-1) == -3
    assert pr(T=0) == -3 and pr(T=9) == -3 and pr(K_=0) == -3 and pr(K_=9) == -3
    assert pr(thr=(0.5, 0.5)) == -3 and pr(thr=(0.75, 0.5)) == -3 and pr(thr=(0.5, np.inf)) == -3 and pr(thr=(np.nan,)) == -3
    assert pr(thr=(-np.inf, 0.5)) == -3
    assert pr(ks=(0, 1)) == -3 and pr(ks=(1, 1)) == -3 and pr(ks=(10, 1)) == -3 and pr(ks=(-1,)) == -3
    assert pr(goff=(1, 1)) == -3 and pr(goff=(0, 2, 1)) == -3 and pr(goff=(0, 1), G=2) == -3 and pr(goff=(0, 1), G=-1) == -3
    assert pr(host=False) == -3 and pr(tables=(False, True)) == -3 and pr(tables=(True, False)) == -3 and pr(counters=None) == -3
    for name in ("prob", "boxes", "gboxes", "glabels", "dev_off"):
        assert pr(**{name: None}) == -3, name
    assert pr(Q_=1025, C=0) == -3                                            # an argument error is named before a limit
    assert pr(thr=tuple(0.1 * i for i in range(1, 9)), ks=tuple(range(1, 9)), goff=(0, 0)) == 0       # eight of both are taken


# ---- ValueErrors -----------------------------------------------------------------------------------------------------------------------
def test_value_errors_name_the_argument():
    from spe_amd.evalmetrics import ProposalRecallMeter as M
    for kw, word in (({"iou_threshs": ()}, "iou_threshs"), ({"iou_threshs": (0.5, 0.5)}, "iou_threshs"), ({"iou_threshs": (0.5, float("nan"))}, "iou_threshs"),
                     ({"iou_threshs": tuple(0.1 * i for i in range(9))}, "iou_threshs"), ({"ks": ()}, "ks"), ({"ks": (0, 1)}, "ks"),
                     ({"ks": (1, 1)}, "ks"), ({"ks": (1.5, 2)}, "ks"), ({"ks": tuple(range(1, 10))}, "ks")):
        with pytest.raises(ValueError, match=word):
            M(3, ["s"], **kw)
    with pytest.raises(ValueError, match="num_classes"):
        M(0, ["s"])
    with pytest.raises(ValueError, match="stages"):
        M(3, ["s", "s"])
    with pytest.raises(ValueError, match="stages"):
        M(3, [])
    m = M(3, ["s"])
    out = {"pred_logits": torch.zeros(2, 4, 3), "pred_boxes": torch.rand(2, 4, 4)}
    gt = {"boxes": torch.rand(1, 4), "labels": torch.zeros(1, dtype=torch.int64)}
    with pytest.raises(ValueError, match="unknown stage 't'"):
        m.update("t", out, [gt, gt])
    with pytest.raises(ValueError, match="outputs of 2 images, gts of 1"):
        m.update("s", out, [gt])
    with pytest.raises(ValueError, match="'pred_boxes'"):
        m.update("s", {"pred_logits": out["pred_logits"]}, [gt, gt])
    with pytest.raises(ValueError, match="pred_boxes \\[B, Q, 4\\]"):
        m.update("s", {"pred_logits": out["pred_logits"], "pred_boxes": torch.rand(2, 5, 4)}, [gt, gt])
    with pytest.raises(ValueError, match="'labels'"):
        m.update("s", out, [gt, {"boxes": gt["boxes"]}])
    with pytest.raises(ValueError, match="1 to 1024 queries"):
        m.update("s", {"pred_logits": torch.zeros(1, 1025, 3), "pred_boxes": torch.zeros(1, 1025, 4)}, [gt])
    assert not bool(m.counters().any())
    m.update("s", {"pred_logits": torch.zeros(0, 4, 3), "pred_boxes": torch.zeros(0, 4, 4)}, [])          # an empty batch: nothing
    assert m._counters is None
    if torch.cuda.is_available():                                                                       # a device mismatch needs a device
        m.update("s", out, [gt, gt])
        with pytest.raises(ValueError, match="earlier updates on cpu"):
            m.update("s", {k: v.cuda() for k, v in out.items()}, [{k: v.cuda() for k, v in gt.items()}] * 2)
        with pytest.raises(ValueError, match="different devices"):
            M(3, ["s"]).update("s", {k: v.cuda() for k, v in out.items()}, [gt, gt])


# ---- two ranks over gloo ---------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


_MERGE_CASES = ("ties", "wild")                                                 # both C = 6 with thresholds THR2: one meter, two stages


def _merge_meter():
    from spe_amd.evalmetrics import ProposalRecallMeter
    return ProposalRecallMeter(6, ["x", "y", "unused"], iou_threshs=Q.THR2, ks=(1, 2, 3))


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = _merge_meter()
    for stage, name in zip(("x", "y"), _MERGE_CASES):
        case = Q.by_name(name)
        outputs, gts = case.outputs(torch, "cpu"), case.gts(torch, "cpu")
        mine = [b for b in range(case.B) if (b % world == rank if stage == "x" else rank == 0)]          # rank 1 has nothing of "y"
        m.update(stage, {k: v[mine] for k, v in outputs.items()}, [gts[b] for b in mine])
    m.merge()
    out[rank] = m.counters().numpy()
    dist.barrier()
    dist.destroy_process_group()


def test_merge_over_gloo_world2_gives_the_single_process_counters():
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    res = dict(out)
    single = _merge_meter()
    for stage, name in zip(("x", "y"), _MERGE_CASES):
        case = Q.by_name(name)
        single.update(stage, case.outputs(torch, "cpu"), case.gts(torch, "cpu"))
    want = single.counters().numpy()
    assert want[0].any() and want[1].any() and not want[2].any()
    for rank in range(world):
        assert np.array_equal(res[rank], want), rank


# ---- the summary -----------------------------------------------------------------------------------------------------------------------
def test_summary_follows_the_nan_rules_and_reset_forgets(capsys):
    from spe_amd.evalmetrics import ProposalRecallMeter
    case = Q.by_name("hand")
    m = ProposalRecallMeter(case.C, ["s", "idle"], iou_threshs=case.thr, ks=case.ks)
    empty = m.summarize()["s"]
    assert np.isnan(empty["mean_mean_best_iou"]) and bool(torch.isnan(empty["recall"]).all()) and bool(torch.isnan(empty["mean_ceiling"]).all())
    assert empty["dropped_gts"] == 0 and not bool(m.counters().any())
    from spe_amd import evalmetrics
    evalmetrics._proposal_recall_host(torch.from_numpy(case.prob), torch.from_numpy(case.boxes), torch.from_numpy(case.gboxes),
                                      torch.from_numpy(case.glabels), case.goff, case.C, m._thr, m._ks, m._state(torch.device("cpu"))[0])
    out = m.summarize()
    got, want = out["s"], R.summary(Q.hand_expected(), case.C, case.T, case.K)
    assert got["recall"].shape == (2, 4, 4) and got["ceiling"].shape == (2, 4) and got["selection_gap"].shape == (2, 4)
    assert got["recall"].dtype == got["ceiling"].dtype == got["mean_best_iou"].dtype == torch.float64
    for k in ("recall", "ceiling", "selection_gap", "mean_best_iou", "mean_recall", "mean_ceiling", "mean_selection_gap"):
        assert _same_bits(got[k].numpy(), want[k]), k
    assert _same_bits(got["mean_mean_best_iou"], want["mean_mean_best_iou"])
    assert bool(torch.isnan(got["recall"][:, :, 3]).all()) and not bool(torch.isnan(got["recall"][:, :, :3]).any())      # class 3 has no rows: NaN, left out
    assert got["ceiling"][0].tolist()[:3] == [0.0, 0.5, 1.0] and got["selection_gap"][0, 2].item() == 0.5
    assert got["mean_ceiling"][0].item() == 0.5 and got["mean_best_iou"][1].item() == 0.625 and got["mean_best_iou"][0].item() == 0.0
    assert got["dropped_gts"] == 2 and got["gts"].tolist() == [1, 2, 2, 0] and torch.equal(got["counters"], torch.from_numpy(Q.hand_expected()[:, :4]))
    assert bool(torch.isnan(out["idle"]["mean_recall"]).all())
    text = str(m).splitlines()
    assert text[0] == "Proposals [s] IoU > 0.5: recall@1 {:.4f}  recall@2 {:.4f}  recall@6 {:.4f}  recall@11 {:.4f}  ceiling 0.5000".format(
        *want["mean_recall"][0].tolist())
    assert text[1].startswith("Proposals [idle] IoU > 0.5: recall@1 nan")
    m.reset()
    assert not bool(m.counters().any())


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


def _lines(text):
    return [l for l in text.splitlines() if "Epoch: [" not in l]              # the ledger's timed lines aside


def test_loop_with_and_without_the_meter(host_contours, capsys):
    from spe_amd.evalmetrics import PseudoLabelMeter
    cpu = torch.device("cpu")
    parent_stats, parent_params = T.run_parent_epochs(cpu)
    capsys.readouterr()
    plain_stats, plain_params, none, _, _ = PL.run_epochs(cpu)
    plain_out = capsys.readouterr().out
    # without a meter: the parent commit's loop, whatever else the targets carry, and the lines of the loop with a pseudo meter alone
    assert none is None and list(plain_stats) == list(parent_stats) and torch.equal(plain_params, parent_params)
    assert all(_same_bits(plain_stats[k], parent_stats[k]) for k in plain_stats)
    assert "Proposals [" not in plain_out and "Pseudo labels [" not in plain_out
    L.run_epochs(cpu)
    assert _lines(capsys.readouterr().out) == _lines(plain_out)
    # with the meter: the same losses and parameters, the new keys behind the old ones, equal to a meter fed by hand
    stats, params, meter, recorded, batches = PL.run_epochs(cpu, PL.meter_factory)
    out = capsys.readouterr().out
    assert list(stats) == list(plain_stats) + PL.stat_keys() and torch.equal(params, plain_params)
    assert all(_same_bits(stats[k], plain_stats[k]) for k in plain_stats)
    hand = PL.fed_by_hand(PL.meter_factory(), PL.last_epoch_updates(recorded, batches))
    want = hand.counters()
    assert len(recorded) == 6 and torch.equal(meter.counters(), want)
    assert int(want[:, 0, :PL.NUM_CLASSES].sum()) > 0 and int(want[:, 0, PL.NUM_CLASSES].sum()) > 0 and int(want[:, 2].sum()) > 0
    summary = hand.summarize()
    for stage in PL.STAGES:
        for k, v in zip(PL.KS, summary[stage]["mean_recall"][0].tolist()):
            assert _same_bits(stats[f"prop_{stage}_recall_at_{k}"], v)
        assert _same_bits(stats[f"prop_{stage}_ceiling"], summary[stage]["mean_ceiling"][0].item())
        assert _same_bits(stats[f"prop_{stage}_mean_best_iou"], summary[stage]["mean_mean_best_iou"])
    body = _lines(out)
    assert body.count(str(hand).splitlines()[0]) >= 1 and sum(l.startswith("Proposals [") for l in body) == 2 * len(PL.STAGES)
    assert [l for l in body if not l.startswith("Proposals [")] == _lines(plain_out)
    # both meters together share the rows kept aside; the pseudo meter's numbers do not move
    both = PL.run_epochs(cpu, PL.meter_factory, lambda: PseudoLabelMeter(L.NUM_CLASSES, L.STAGES))
    alone = L.run_epochs(cpu, lambda: PseudoLabelMeter(L.NUM_CLASSES, L.STAGES))
    assert torch.equal(both[2].counters(), want)
    assert all(_same_bits(both[0][k], alone[0][k]) for k in alone[0]) and list(both[0])[:len(alone[0])] == list(alone[0])


def test_loop_names_the_missing_key_and_keeps_its_signature(host_contours, capsys):
    import inspect
    from spe_amd import engine
    from spe_amd.models.conditional_detr import PostProcessRefine
    batches = T.stub_batches(1)                                               # the stub's own targets: no ground-truth rows
    model = T.StubModel(batches)
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    with pytest.raises(ValueError, match="'boxes'"):
        engine.train_one_epoch_refine(model, T.StubCriterion(), T.stub_loader(batches), opt, torch.device("cpu"), T.STUB_EPOCH, 0.1, T.stub_args(),
                                      {"bbox": PostProcessRefine()}, T.StubCriterion(), proposal_meter=PL.meter_factory())
    for fn in (engine.train_one_epoch_refine, engine.train_one_epoch_refine_coco):
        assert inspect.signature(fn).parameters["proposal_meter"].default is None
    assert inspect.signature(engine.evaluate_det_voc).parameters["proposal_meter"].default is None


# ---- evaluate_det_voc --------------------------------------------------------------------------------------------------------------------
def voc_loop(flip, device, with_meter=True):
    """evaluate_det_voc over the canned VOC run -> (its return, the printed lines, the caller's meter, a meter fed by hand)."""
    from spe_amd import engine
    from spe_amd.evalmetrics import ProposalRecallMeter
    g = voc_eval_cases.load_golden("voc_eval_small")
    images, C, batch = g["images"], g["num_classes"], 8
    model, loader, base_ds, canned = D.voc_run(images, C, batch, flip=flip)
    make = lambda: ProposalRecallMeter(C + 1, ["det"], ks=(1, 10, 100))
    meter = make() if with_meter else None
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = engine.evaluate_det_voc(model, D.StubCriterion(), {}, loader, base_ds, device, None, None, with_flip=flip, num_classes=C,
                                      **({"proposal_meter": meter} if with_meter else {}))
    hand = PL.fed_by_hand(make(), PL.voc_updates(images, canned, batch, flip, device))
    return out, [l for l in buf.getvalue().splitlines() if "=> Test:" not in l], meter, hand


@pytest.mark.parametrize("flip", [False, True])
def test_evaluate_det_voc_with_and_without_the_meter(flip):
    from spe_amd import engine
    from spe_amd.evalmetrics import ProposalRecallMeter
    cpu = torch.device("cpu")
    plain, plain_lines, _, _ = voc_loop(flip, cpu, with_meter=False)
    out, lines, meter, hand = voc_loop(flip, cpu)
    assert "proposals" not in plain and list(out) == list(plain) + ["proposals"]
    for k in plain:
        assert voc_eval_cases.same(out[k], plain[k]), k
    assert lines[:len(plain_lines)] == plain_lines and lines[len(plain_lines):] == str(hand).splitlines() and len(lines) == len(plain_lines) + 1
    want = hand.counters()
    assert torch.equal(meter.counters(), want) and int(want[0, 2].sum()) > 0 and int(want[0, 4].sum()) > 0
    assert torch.equal(out["proposals"]["counters"], hand.summarize()["det"]["counters"])
    assert _same_bits(out["proposals"]["recall"].numpy(), hand.summarize()["det"]["recall"].numpy())
    g = voc_eval_cases.load_golden("voc_eval_small")
    model, loader, base_ds, _ = D.voc_run(g["images"], g["num_classes"], 8)
    with pytest.raises(ValueError, match="'det'"):
        engine.evaluate_det_voc(model, D.StubCriterion(), {}, loader, base_ds, cpu, None, None, num_classes=g["num_classes"],
                                proposal_meter=ProposalRecallMeter(21, ["s0"]))
