"""The classification-AP kernels (csrc/cls_ap.hip) on the device against the plain-Python restatement (tests/cls_ap_ref.py) and the
recorded results of the reference's AveragePrecisionMeter (tests/golden/cls_ap_*.pt).

spe_cls_ap is called through the C ABI on buffers this file owns.  The class rows are longer than n (ld > n) and the slack holds NaN
scores with target 1 - samples that would rank first, as positives, if the kernel read them; the workspace and every output sit
between guard bands pre-filled with a sentinel, and the inputs are compared with what was uploaded.  Every equality is exact: 'ap' as
fp64 bit patterns (NaN matching NaN), the counts as integers."""
import numpy as np
import pytest
import torch

import cls_ap_cases as cases
from cls_ap_cases import check_summary, load_golden, run_meter, same_bits

pytestmark = pytest.mark.gpu

GUARD, SLACK, AP_FILL, COUNT_FILL = 64, 37, -7.25, -77


def call_cls_ap(dev, scores, codes, difficult, n=None, ld=None, expect=0):
    """spe_cls_ap through the C ABI on scores fp32 [N, C] / int8 codes [N, C] -> (ap, npos, ncounted) as numpy, guard bands checked."""
    from spe_amd import kernels as K, lib
    N, C = scores.shape
    n = N if n is None else n
    ld = N + SLACK if ld is None else ld
    s = torch.full((C, ld), float("nan"), dtype=torch.float32)                     # class-major rows of exactly ld columns
    t = torch.ones((C, ld), dtype=torch.int8)
    m = min(N, ld)
    s[:, :m], t[:, :m] = torch.from_numpy(scores.T[:, :m].copy()), torch.from_numpy(codes.T[:, :m].copy())
    sd, td = s.to(dev), t.to(dev)
    words = K.cls_ap_workspace_bytes(n, C) // 8 if expect == 0 else N * C
    assert words == n * C or expect != 0
    ws = torch.full((GUARD + words + GUARD,), AP_FILL, dtype=torch.float64, device=dev)
    ap = torch.full((GUARD + C + GUARD,), AP_FILL, dtype=torch.float64, device=dev)
    cnt = torch.full((2, GUARD + C + GUARD), COUNT_FILL, dtype=torch.int32, device=dev)
    f = getattr(lib.load(), "spe_cls_ap")
    rc = f(sd.data_ptr(), td.data_ptr(), n, C, ld, int(difficult), ws[GUARD:].data_ptr(), ap[GUARD:].data_ptr(), cnt[0, GUARD:].data_ptr(),
           cnt[1, GUARD:].data_ptr(), K._st())
    torch.cuda.synchronize()
    assert rc == expect, rc
    ws, ap, cnt = ws.cpu().numpy(), ap.cpu().numpy(), cnt.cpu().numpy()
    assert (ws[:GUARD] == AP_FILL).all() and (ws[GUARD + words:] == AP_FILL).all(), "written outside the workspace"
    assert (ap[:GUARD] == AP_FILL).all() and (ap[GUARD + C:] == AP_FILL).all(), "written outside ap"
    assert (cnt[:, :GUARD] == COUNT_FILL).all() and (cnt[:, GUARD + C:] == COUNT_FILL).all(), "written outside the counts"
    assert torch.equal(sd.cpu().view(torch.int32), s.view(torch.int32)) and torch.equal(td.cpu(), t), "an input was written"
    if expect != 0:
        assert (ws == AP_FILL).all() and (ap == AP_FILL).all() and (cnt == COUNT_FILL).all(), "a refused call wrote"
    return ap[GUARD:GUARD + C], cnt[0, GUARD:GUARD + C], cnt[1, GUARD:GUARD + C]


@pytest.mark.parametrize("difficult", [False, True])
@pytest.mark.parametrize("C", cases.CS)
@pytest.mark.parametrize("N", cases.NS)
def test_c_abi(dev, N, C, difficult):
    scores, _, codes = cases.case(N, C)
    ref = cases.reference(N, C, difficult)
    ap, npos, ncounted = call_cls_ap(dev, scores, codes, difficult)
    assert same_bits(ap, ref["ap"]), (ap, ref["ap"])
    assert np.array_equal(npos, ref["npos"]) and np.array_equal(ncounted, ref["ncounted"])


def test_cases_cover_the_edges():
    """What the shapes above are for: every kind of column at every N once C >= 20; 1025 positives pass the 1024-slot chunk of the
    sequential sum; tie runs lie across the tile edges; a class of alternating 0 / 1 in walk order has only skipped neighbours."""
    assert all(cases.kinds_of(N, C) == set(cases.KINDS) for N in cases.NS for C in (20, 91))
    assert (cases.reference(1025, 20, False)["npos"] == 1025).any()
    s = cases.score_column("tie_blocks", 1025, None)
    assert all(s[e - 1] == s[e] for e in (256, 512, 1024)) and len(set(s.tolist())) == 7
    ref = cases.reference(256, 20, True)
    c = [k for k in range(20) if cases.KINDS[(k + 256) % 20] == ("ramp", "alternating")][0]
    assert ref["ap"][c] == 1.0 and ref["ncounted"][c] == 128 and cases.reference(256, 20, False)["ap"][c] < 0.76


def test_rows_are_independent_of_ld(dev):
    """The same samples with no slack (ld = n), and as the first n columns of longer rows whose tail holds OTHER real samples."""
    scores, _, codes = cases.case(513, 20)
    for n, ld in ((513, 513), (257, 513), (256, 300), (1, 513)):
        ref = cases.R.evaluate(scores[:n], cases.case(513, 20)[1][:n], True)
        ap, npos, ncounted = call_cls_ap(dev, scores, codes, True, n=n, ld=ld)
        assert same_bits(ap, ref["ap"]) and np.array_equal(npos, ref["npos"]) and np.array_equal(ncounted, ref["ncounted"]), (n, ld)


def test_no_samples(dev):
    scores, _, codes = cases.case(2, 20)
    for ld in (0, 2):
        ap, npos, ncounted = call_cls_ap(dev, scores, codes, False, n=0, ld=ld)
        assert np.isnan(ap).all() and (npos == 0).all() and (ncounted == 0).all()


def test_refusals_need_no_allocation():
    """-2 before any launch: the pointers are never touched, so none is given (and no device either)."""
    import ctypes
    from spe_amd import kernels as K, lib
    f = getattr(lib.load(), "spe_cls_ap")
    big = K.CLS_AP_MAX_N
    assert big == 1 << 24
    for n, C, ld in ((big + 1, 1, big + 1), (-1, 1, 4), (4, 0, 4), (4, -3, 4), (4, 65536, 4), (4, 2, 3), (big, 1, big - 1)):
        assert f(None, None, n, C, ld, 0, None, None, None, None, None) == -2, (n, C, ld)
    b = ctypes.c_size_t(123)
    w = getattr(lib.load(), "spe_cls_ap_workspace")
    for n, C in ((big + 1, 1), (-1, 1), (4, 0), (4, 65536)):
        assert w(n, C, ctypes.byref(b)) == -2 and b.value == 123
    assert w(4, 2, None) == -2
    assert K.cls_ap_workspace_bytes(big, 91) == big * 91 * 8 and K.cls_ap_workspace_bytes(0, 1) == 0 and K.cls_ap_workspace_bytes(513, 20) == 513 * 20 * 8


def test_refusals_write_nothing(dev):
    scores, _, codes = cases.case(65, 2)
    call_cls_ap(dev, scores, codes, False, n=65, ld=64, expect=-2)
    call_cls_ap(dev, scores, codes, False, n=-1, ld=65, expect=-2)


@pytest.mark.parametrize("mode", ["plain", "difficult"])
@pytest.mark.parametrize("name", cases.GOLDENS)
def test_golden_on_device(dev, name, mode):
    g = load_golden(name)
    m = run_meter(g["scores"], g["targets"], g["batches"], difficult=mode == "difficult", device=dev)
    value = m.value()
    assert value.dtype == torch.float32 and value.device.type == "cpu" and torch.equal(value, g["value_" + mode])
    assert same_bits(m.summarize()["ap"], g["ap64_" + mode])


@pytest.mark.parametrize("difficult", [False, True])
def test_meter_against_its_cpu_path_across_two_growths(dev, difficult):
    """3075 samples in uneven adds: the class rows move to a larger allocation twice (1024 -> 2052 -> 6150 columns)."""
    scores, targets, _ = cases.case(1025, 20)
    rep = lambda a: np.concatenate([a, a[::-1], a])
    sizes = [500, 526, 1, 2048]
    m = run_meter(rep(scores), rep(targets), sizes, difficult, device=dev)
    assert m._scores.shape == (20, 6150) and m._scores.is_cuda and m._targets.dtype == torch.int8
    host = run_meter(rep(scores), rep(targets), sizes, difficult).summarize()
    out = m.summarize()
    assert same_bits(out["ap"], host["ap"]) and same_bits([out["map"]], [host["map"]])
    assert torch.equal(out["npos"], host["npos"]) and torch.equal(out["ncounted"], host["ncounted"])
    value = m.value()                                                              # two classes without a positive: NaN
    assert value.dtype == torch.float32 and same_bits(value.double(), out["ap"].float().double()) and np.isnan(value.numpy()).sum() == 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.int64, torch.uint8, torch.bool])
def test_target_dtypes_on_device(dev, dtype):
    scores, targets, _ = cases.case(255, 20)
    multi_hot = (targets == 1).astype(np.float32)
    want = cases.R.evaluate(scores, multi_hot, True)
    check_summary(run_meter(scores, multi_hot, [100, 155], True, device=dev, target_dtype=dtype).summarize(), want)


def test_add_does_not_synchronise(dev):
    """add() reads no device data on the host, a growth included: under torch's sync debug mode any .item() / .cpu() would raise."""
    from spe_amd.evalmetrics import ClassificationAPMeter
    scores, targets, _ = cases.case(1025, 20)
    s, t = torch.from_numpy(scores.copy()).to(dev), torch.from_numpy(targets.copy()).to(dev)
    m = ClassificationAPMeter(True)
    m.add(s[:300], t[:300])                            # first call: allocations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.add(s[300:301], t[300:301])
        m.add(s[301:], t[301:])                        # 1025 > 1024: grows
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert m._scores.shape[1] == 2050
    check_summary(m.summarize(), cases.reference(1025, 20, True))


def test_two_runs_bitwise_equal(dev):
    scores, targets, _ = cases.case(1025, 91)
    runs = [run_meter(scores, targets, [1000, 25], True, device=dev).summarize() for _ in range(2)]
    assert np.array_equal(cases.bits(runs[0]["ap"]), cases.bits(runs[1]["ap"]))      # the raw bits, NaN payloads included
    assert torch.equal(runs[0]["npos"], runs[1]["npos"]) and torch.equal(runs[0]["ncounted"], runs[1]["ncounted"])
    check_summary(runs[0], cases.reference(1025, 91, True))


def test_evaluate_det_voc_on_the_device_with_a_meter(dev):
    """The loop on the device feeds the caller's meter device logits; its numbers equal the CPU run's."""
    import contextlib
    import io

    import detect_loops as loops
    import voc_eval_cases
    from spe_amd import engine
    from spe_amd.evalmetrics import ClassificationAPMeter
    g = voc_eval_cases.load_golden("voc_eval_small")
    images, C, K_ = g["images"], g["num_classes"], 5
    outs = []
    for device in (torch.device("cpu"), dev):
        model, loader, base_ds, canned = loops.voc_run(images, C, 8)
        for b, (out, (_, ts)) in enumerate(zip(canned, loader)):
            out["x_logits"] = torch.randn(len(ts), K_, generator=torch.Generator().manual_seed(b)).round(decimals=1)
            for i, t in enumerate(ts):
                t["label"] = (out["x_logits"][i].flip(0) > 0.3).float()
        meter = ClassificationAPMeter()
        with contextlib.redirect_stdout(io.StringIO()):
            outs.append(engine.evaluate_det_voc(model, loops.StubCriterion(), {}, loader, base_ds, device, None, None, num_classes=C,
                                                cls_meter=meter))
        assert meter._device.type == device.type
    assert same_bits(outs[0]["cls_ap"], outs[1]["cls_ap"]) and same_bits([outs[0]["cls_map"]], [outs[1]["cls_map"]])
    assert not np.isnan(outs[0]["cls_map"])
