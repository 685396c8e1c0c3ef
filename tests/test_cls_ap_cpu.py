"""spe_amd.evalmetrics.ClassificationAPMeter on CPU tensors (the numpy composition of the device rules): the recorded results of the
reference's own AveragePrecisionMeter (tests/golden/cls_ap_*.pt, tools/gen_cls_ap_golden.py; tie-free by the generator's assertion),
the plain-Python restatement (tests/cls_ap_ref.py) on tied, NaN and +-0 scores, the shape rules, the empty meter, the class without
a positive, the world-2 merge over gloo, and spe_amd.engine.evaluate_det_voc with and without a meter.

Every equality is exact: 'ap' and 'map' as fp64 bit patterns (NaN matching NaN), value() by torch.equal, the counts as integers."""
import contextlib
import io
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import cls_ap_cases as cases
import cls_ap_ref as R
import detect_loops as loops
import voc_eval_cases
from cls_ap_cases import check_summary, load_golden, run_meter, same_bits
from spe_amd import engine
from spe_amd.evalmetrics import ClassificationAPMeter


# ---- the reference's recorded numbers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "difficult"])
@pytest.mark.parametrize("name", cases.GOLDENS)
def test_golden(name, mode):
    g = load_golden(name)
    m = run_meter(g["scores"], g["targets"], g["batches"], difficult=mode == "difficult")
    value = m.value()
    assert value.dtype == torch.float32 and torch.equal(value, g["value_" + mode])
    out = m.summarize()
    assert same_bits(out["ap"], g["ap64_" + mode])
    check_summary(out, R.evaluate(g["scores"].numpy(), g["targets"].numpy(), mode == "difficult"))
    assert same_bits([out["map"]], [np.mean(g["ap64_" + mode].numpy())])            # every class has a positive here
    one_add = run_meter(g["scores"], g["targets"], [g["scores"].shape[0]], difficult=mode == "difficult").summarize()
    assert same_bits(one_add["ap"], out["ap"])


def test_golden_pins_where_a_nan_score_ranks():
    """One NaN score, on a positive: the reference's torch.sort(descending=True) walks it first.  Ranked last the class would score
    lower, and the recorded number tells the two apart."""
    g = load_golden("cls_ap_special")
    i, c = g["nan_at"]
    s, t = g["scores"][:, c].numpy(), g["targets"][:, c].numpy()
    assert np.isnan(s[i]) and np.isnan(s).sum() == 1 and t[i] == 1
    assert R.walk_order(s)[0] == i
    last = np.where(np.isnan(s), -np.inf, s)
    for mode in (False, True):
        want = float(g["ap64_difficult" if mode else "ap64_plain"][c])
        assert R.average_precision(s, t, mode)[0] == want and R.average_precision(last, t, mode)[0] < want


# ---- the restatement, where the order is this package's own rule ---------------------------------------------------------------------------
def test_cases_cover_the_kinds():
    assert all(cases.kinds_of(N, 20) == set(cases.KINDS) for N in cases.NS)
    assert set().union(*(cases.kinds_of(N, 1) | cases.kinds_of(N, 2) for N in cases.NS)) >= {("equal", "random"), ("special", "random"), ("ramp", "alternating"), ("distinct", "all")}
    s, t, codes = cases.case(513, 20)
    assert np.isnan(s).any() and np.isinf(s).any() and (np.signbit(s) & (s == 0)).any() and ((s == 0) & ~np.signbit(s)).any()
    assert np.isnan(t).any() and set(np.unique(codes).tolist()) >= {-128, -3, -1, 0, 1, 2, 127}
    ref = cases.reference(513, 20, True)
    assert (ref["npos"] == 0).any() and (ref["npos"] == 1).any() and (ref["npos"] == 513).any() and (ref["ncounted"] < 513).any()


@pytest.mark.parametrize("difficult", [False, True])
@pytest.mark.parametrize("N,C", [(N, 20) for N in cases.NS] + [(257, 1), (64, 2), (1025, 91)])
def test_restatement(N, C, difficult):
    scores, targets, _ = cases.case(N, C)
    sizes = [N] if N < 4 else [N // 3, 1, N - N // 3 - 1]
    check_summary(run_meter(scores, targets, sizes, difficult).summarize(), cases.reference(N, C, difficult))


def test_hand_worked_order():
    """Four samples, one class.  Equal scores rank by index; +0.0 and -0.0 are equal; NaN ranks first."""
    def ap(scores, targets, difficult=False):
        m = ClassificationAPMeter(difficult)
        m.add(torch.tensor(scores, dtype=torch.float32), torch.tensor(targets))
        return m.summarize()
    out = ap([0.5, 0.5, 0.5, 0.5], [0, 1, 0, 1])                                   # walk 0 1 2 3: 1/2 + 2/4
    assert out["ap"].tolist() == [(1 / 2 + 2 / 4) / 2] and out["npos"].tolist() == [2] and out["ncounted"].tolist() == [4]
    assert ap([0.5, 0.5, 0.5, 0.5], [1, 0, 1, 0])["ap"].tolist() == [(1 / 1 + 2 / 3) / 2]
    assert ap([-0.0, 0.0, -0.0, 1.0], [0, 1, 1, 0])["ap"].tolist() == [(1 / 3 + 2 / 4) / 2]      # walk 3 0 1 2
    assert ap([0.0, -0.0, 0.0, 1.0], [1, 0, 1, 0])["ap"].tolist() == [(1 / 2 + 2 / 4) / 2]
    assert ap([1.0, float("inf"), float("nan"), 2.0], [0, 0, 1, 1])["ap"].tolist() == [(1 / 1 + 2 / 3) / 2]     # walk 2 1 3 0
    assert ap([float("nan"), 3.0, float("nan"), 2.0], [0, 1, 1, 0])["ap"].tolist() == [(1 / 2 + 2 / 3) / 2]     # walk 0 2 1 3
    out = ap([4.0, 3.0, 2.0, 1.0], [0, 1, 0, 1], difficult=True)                   # zeros are not counted
    assert out["ap"].tolist() == [1.0] and out["ncounted"].tolist() == [2]
    out = ap([4.0, 3.0, 2.0, 1.0], [-1, 1, 7, 1], difficult=True)                  # -1 and 7 are negatives, and counted
    assert out["ap"].tolist() == [(1 / 2 + 2 / 4) / 2] and out["ncounted"].tolist() == [4]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16, torch.int64, torch.int8, torch.uint8, torch.bool])
def test_target_dtypes(dtype):
    scores, targets, _ = cases.case(255, 20)
    multi_hot = (targets == 1).astype(np.float32)
    want = R.evaluate(scores, multi_hot, True)
    check_summary(run_meter(scores, multi_hot, [100, 155], True, target_dtype=dtype).summarize(), want)


def test_inputs_and_shape_rules():
    scores, targets, _ = cases.case(65, 2)
    m = ClassificationAPMeter()
    m.add(scores[:10, 0].copy(), targets[:10, 0].copy())                           # numpy, 1-D: one column
    m.add(torch.from_numpy(scores[10:, :1].copy()), torch.from_numpy(targets[10:, 0].copy()))      # [B, 1] with a 1-D target
    check_summary(m.summarize(), R.evaluate(scores[:, :1], targets[:, :1], False))
    with pytest.raises(ValueError, match="previously added"):
        m.add(torch.zeros(3, 2), torch.zeros(3, 2))
    with pytest.raises(ValueError, match="wrong output size"):
        m.add(torch.zeros(3, 1, 1), torch.zeros(3))
    with pytest.raises(ValueError, match="wrong target size"):
        m.add(torch.zeros(3), torch.zeros(3, 1, 1))
    with pytest.raises(ValueError):
        m.add(torch.zeros(3), torch.zeros(4))
    check_summary(m.summarize(), R.evaluate(scores[:, :1], targets[:, :1], False))   # a refused add leaves the meter as it was
    m.reset()
    m.add(torch.zeros(3, 2), torch.ones(3, 2))                                     # another C after reset()
    assert m.value().tolist() == [1.0, 1.0]


def test_empty_meter():
    m = ClassificationAPMeter()
    assert m.value() == 0
    with pytest.raises(RuntimeError, match="nothing accumulated"):
        m.summarize()
    m.add(torch.zeros(0, 3), torch.zeros(0, 3))                                    # classes known, no sample
    assert m.value() == 0
    out = m.summarize()
    assert np.isnan(out["ap"].numpy()).all() and np.isnan(out["map"]) and out["npos"].tolist() == [0] * 3 and out["ncounted"].tolist() == [0] * 3


def test_class_without_a_counted_positive():
    s = torch.tensor([[3.0, 1.0, 2.0], [2.0, 2.0, 1.0], [1.0, 3.0, 3.0]])
    t = torch.tensor([[1, 0, 0], [0, -1, 0], [1, 2, 0]])
    for difficult in (False, True):
        m = ClassificationAPMeter(difficult)
        m.add(s, t)
        out = m.summarize()
        assert out["npos"].tolist() == [2, 0, 0] and out["ncounted"].tolist() == ([2, 2, 0] if difficult else [3, 3, 3])
        assert np.isnan(out["ap"][1:].numpy()).all() and out["map"] == float(out["ap"][0])
        value = m.value()
        assert value.dtype == torch.float32 and np.isnan(value[1:].numpy()).all()
    m = ClassificationAPMeter()
    m.add(s[:, 1:], t[:, 1:])
    assert np.isnan(m.summarize()["map"])


def test_growth_keeps_the_samples():
    scores, targets, _ = cases.case(1025, 2)
    rep = lambda a: np.concatenate([a, a, a])                                       # 3075 samples: capacities 1024 -> 2052 -> 6150
    m = run_meter(rep(scores), rep(targets), [500, 526, 1, 2048], True)
    assert m._scores.shape == (2, 6150)
    check_summary(m.summarize(), R.evaluate(rep(scores), rep(targets), True))


# ---- merge -------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out, idle_rank):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    scores, targets, _ = cases.case(257, 20)
    cut = 0 if idle_rank == 0 else 257 if idle_rank == 1 else 101                  # rank 0 holds [0, cut), rank 1 the rest: rank-major
    lo, hi = (0, cut) if rank == 0 else (cut, 257)
    single = run_meter(scores, targets, [257], True).summarize()
    m = run_meter(scores[lo:hi], targets[lo:hi], [b for b in ((hi - lo) // 2, hi - lo - (hi - lo) // 2) if b], True)
    m.merge()
    got = m.summarize()
    ok = same_bits(got["ap"], single["ap"]) and same_bits([got["map"]], [single["map"]])
    ok = ok and torch.equal(got["npos"], single["npos"]) and torch.equal(got["ncounted"], single["ncounted"])
    try:
        m.merge()
        ok = False
    except RuntimeError:
        pass
    try:
        m.add(torch.zeros(1, 20), torch.zeros(1, 20))
        ok = False
    except RuntimeError:
        pass
    out[rank] = (ok, hi - lo)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("idle_rank", [None, 1])
def test_gloo_world2_merge(idle_rank):
    """Tied scores everywhere (case(257, 20)): the merged meter equals the single-process one on the concatenation only if the
    samples arrive in rank order.  idle_rank 1 makes no add() at all and learns the class count from rank 0."""
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(2, _free_port(), out, idle_rank), nprocs=2, join=True)
    assert dict(out) == ({0: (True, 101), 1: (True, 156)} if idle_rank is None else {0: (True, 257), 1: (True, 0)})


def test_merge_without_process_group_is_a_noop():
    scores, targets, _ = cases.case(64, 2)
    m = run_meter(scores, targets, [64])
    a = m.summarize()
    m.merge()
    m.merge()
    m.add(torch.from_numpy(scores[:1].copy()), torch.from_numpy(targets[:1].copy()))
    assert same_bits(run_meter(scores, targets, [64]).summarize()["ap"], a["ap"])


# ---- evaluate_det_voc --------------------------------------------------------------------------------------------------------------------
class _WithClassLogits:
    """detect_loops.StubModel plus the image-level logits of the batch under 'x_logits' and 'x_cls_logits'.  Under with_flip the model
    sees [images ; mirrored images]: the two halves get logits whose element-wise maximum - what decouple_output keeps - is the batch's."""

    def __init__(self, model, logits, flip):
        self.model, self.logits, self.flip = model, logits, flip

    def eval(self):
        self.model.eval()

    def __call__(self, samples):
        x = self.logits[self.model.calls]
        out = self.model(samples)

        def halves(v):
            first = (torch.arange(v.numel()).reshape(v.shape) % 2 == 0)
            return torch.cat([torch.where(first, v, v - 1.5), torch.where(first, v - 0.25, v)]) if self.flip else v.clone()
        out[0]["x_logits"], out[0]["x_cls_logits"] = halves(x), halves(-x)
        return out


def _voc_loop(flip, K=5):
    g = voc_eval_cases.load_golden("voc_eval_small")
    images, C, batch = g["images"], g["num_classes"], 8
    model, loader, base_ds, _ = loops.voc_run(images, C, batch, flip=flip)
    gen = torch.Generator().manual_seed(12)
    logits = [torch.randn(len(t), K, generator=gen).round(decimals=1) for _, t in loader]          # one decimal: ties between images
    labels = [(torch.rand(len(t), K, generator=gen) < 0.4).float() for _, t in loader]
    loader = [(s, [{**t, "label": lab[i]} for i, t in enumerate(ts)]) for (s, ts), lab in zip(loader, labels)]
    return _WithClassLogits(model, logits, flip), loader, base_ds, C, torch.cat(logits), torch.cat(labels)


def _run_loop(model, loader, base_ds, C, flip, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = engine.evaluate_det_voc(model, loops.StubCriterion(), {}, loader, base_ds, torch.device("cpu"), None, None, with_flip=flip,
                                      num_classes=C, **kw)
    lines = buf.getvalue().splitlines()
    return out, [l for l in lines if "=> Test:" not in l], sum("=> Test:" in l for l in lines)


@pytest.mark.parametrize("flip", [False, True])
def test_evaluate_det_voc_without_a_meter_is_unchanged(flip):
    """Against tests/golden/cls_ap_voc_loop.pt: the lines and the return of the loop as it was before it took `cls_meter`."""
    rec = load_golden("cls_ap_voc_loop")[flip]
    model, loader, base_ds, C, _, _ = _voc_loop(flip)
    out, lines, timed = _run_loop(model, loader, base_ds, C, flip)
    assert lines == rec["lines"] and timed == rec["timed_lines"]
    assert list(out) == list(rec["out"])
    for k, v in rec["out"].items():
        assert type(out[k]) is type(v) and voc_eval_cases.same(out[k], v), k


@pytest.mark.parametrize("key", ["x_logits", "x_cls_logits"])
@pytest.mark.parametrize("flip", [False, True])
def test_evaluate_det_voc_with_a_meter(flip, key):
    rec = load_golden("cls_ap_voc_loop")[flip]
    model, loader, base_ds, C, logits, labels = _voc_loop(flip)
    meter = ClassificationAPMeter()
    out, lines, timed = _run_loop(model, loader, base_ds, C, flip, cls_meter=meter, **({} if key == "x_logits" else {"cls_key": key}))
    want = R.evaluate((logits if key == "x_logits" else -logits).numpy(), labels.numpy(), False)
    assert same_bits(out["cls_ap"], want["ap"]) and same_bits([out["cls_map"]], [want["map"]]) and not np.isnan(want["map"])
    n = len(rec["lines"])
    assert lines[:n] == rec["lines"] and timed == rec["timed_lines"]               # the detection lines first, untouched
    assert lines[n:] == ["AP (cls) for class{} = {:.4f}".format(c + 1, v) for c, v in enumerate(want["ap"].tolist())] + \
        ["Mean AP (cls) = {:.4f}".format(want["map"])]
    assert list(out) == list(rec["out"]) + ["cls_ap", "cls_map"]
    for k, v in rec["out"].items():
        assert voc_eval_cases.same(out[k], v), k
    assert meter.summarize()["npos"].tolist() == want["npos"].tolist()             # the caller's meter holds the run
