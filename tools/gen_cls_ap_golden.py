"""Record the reference's own AveragePrecisionMeter (cams_deit.py:493-574) -> tests/golden/cls_ap_*.pt.

    python tools/gen_cls_ap_golden.py

The class is imported through tools/ref_harness with an empty `cv2` module stubbed (cams_deit.py imports it at the top; the meter
never touches it).  Per golden: scores [N, C] fp32 and targets [N, C], added to the reference's meter in several unequal batches;
recorded for both settings of difficult_examples are value() (fp32 [C]) and the fp64 number of average_precision per class.

Every column is TIE-FREE - a permutation of values that are distinct as fp32 compares them - and this script asserts it: then the
reference's torch.sort(descending=True) has one answer and the recording pins the package's meter bit for bit.  The only special
values are one column with a single NaN (it pins where a NaN ranks) and one with +inf and -inf, both in cls_ap_special.

    python tools/gen_cls_ap_golden.py --voc-loop

records tests/golden/cls_ap_voc_loop.pt instead: what engine.evaluate_det_voc prints and returns without a classification meter
(record_voc_loop; it was run on the commit before the loop took `cls_meter`, and needs no reference).
Harness only: never imported by the package or on the GPU machine."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")


def reference_meter():
    from tools import ref_harness
    ref_harness.install_shims()
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    import cams_deit
    return cams_deit.AveragePrecisionMeter


def assert_tie_free(scores, nan_cols=(), inf_cols=()):
    for c in range(scores.shape[1]):
        col = scores[:, c]
        nan = np.isnan(col)
        assert int(nan.sum()) == (1 if c in nan_cols else 0), c
        assert bool(np.isinf(col).any()) == (c in inf_cols), c
        v = np.sort(col[~nan])
        assert (v[1:] > v[:-1]).all(), f"column {c} holds two scores that compare equal"       # +0.0 next to -0.0 fails here too


def distinct_columns(rng, N, C):
    """Every column a permutation of N distinct fp32 values; another value set per column."""
    cols = []
    for c in range(C):
        base = (np.arange(N, dtype=np.float64) - N / 2) * (0.011 + 0.003 * c) + rng.uniform(-0.004, 0.004, N)
        cols.append(rng.permutation(base).astype(np.float32))
    return np.stack(cols, 1)


def record(Meter, scores, targets, batches):
    out = {"scores": torch.from_numpy(scores), "targets": torch.from_numpy(targets), "batches": list(batches)}
    assert sum(batches) == scores.shape[0]
    for name, difficult in (("plain", False), ("difficult", True)):
        m, at = Meter(difficult_examples=difficult), 0
        for b in batches:
            m.add(out["scores"][at:at + b], out["targets"][at:at + b])
            at += b
        out["value_" + name] = m.value().clone()
        out["ap64_" + name] = torch.tensor([float(Meter.average_precision(m.scores[:, k], m.targets[:, k], difficult))
                                            for k in range(scores.shape[1])], dtype=torch.float64)
        assert out["value_" + name].dtype == torch.float32 and torch.equal(out["ap64_" + name].float(), out["value_" + name])
    return out


def record_voc_loop():
    """spe_amd.engine.evaluate_det_voc WITHOUT a classification meter, on the stub run of tests/detect_loops.py over voc_eval_small in
    batches of 8, both with_flip settings: the printed lines (those of the step ledger carry clock times: only counted) and the returned
    dict.  Recorded from the package as it stood before the loop learnt `cls_meter`; the loop without one must keep giving exactly this."""
    import contextlib
    import io
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import detect_loops as loops
    import voc_eval_cases
    from spe_amd import engine
    g = voc_eval_cases.load_golden("voc_eval_small")
    rec = {}
    for flip in (False, True):
        model, loader, base_ds, _ = loops.voc_run(g["images"], g["num_classes"], 8, flip=flip)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            out = engine.evaluate_det_voc(model, loops.StubCriterion(), {}, loader, base_ds, torch.device("cpu"), None, None, with_flip=flip,
                                          num_classes=g["num_classes"])
        lines = buf.getvalue().splitlines()
        rec[flip] = {"lines": [l for l in lines if "=> Test:" not in l], "timed_lines": sum("=> Test:" in l for l in lines), "out": out}
    path = os.path.join(GOLD, "cls_ap_voc_loop.pt")
    torch.save(rec, path)
    print(path, os.path.getsize(path), "bytes;", len(rec[False]["lines"]), "lines, keys", sorted(rec[False]["out"]))


def main():
    if "--voc-loop" in sys.argv:
        return record_voc_loop()
    Meter = reference_meter()
    os.makedirs(GOLD, exist_ok=True)

    # the loader's float multi-hot labels, ~25 % positives
    rng = np.random.default_rng(20)
    N, C = 300, 20
    scores = distinct_columns(rng, N, C)
    targets = (rng.random((N, C)) < 0.25).astype(np.float32)
    targets[rng.integers(0, N, C), np.arange(C)] = 1                            # no class without a positive: the reference would raise
    assert_tie_free(scores)
    small = record(Meter, scores, targets, (7, 64, 1, 100, 128))

    # integer targets of -1 / 0 / 1 (anything but 1 is a negative; 0 is skipped with difficult_examples), a NaN and a +-inf column
    rng = np.random.default_rng(21)
    N, C = 257, 20
    scores = distinct_columns(rng, N, C)
    targets = rng.choice(np.array([-1, 0, 1], np.int8), (N, C), p=[0.35, 0.35, 0.3])       # int8: a small file; the reference copies into int64
    targets[rng.integers(0, N, C), np.arange(C)] = 1
    i_nan, i_hi, i_lo = 100, 17, 200
    scores[i_nan, 18] = np.nan
    targets[i_nan, 18] = 1                                                      # a positive: its place in the walk moves the AP
    scores[i_hi, 19], scores[i_lo, 19] = np.inf, -np.inf
    targets[i_hi, 19] = targets[i_lo, 19] = 1
    assert_tie_free(scores, nan_cols=(18,), inf_cols=(19,))
    special = record(Meter, scores, targets, (100, 1, 156))
    special["nan_at"] = (i_nan, 18)

    for name, g in (("cls_ap_small", small), ("cls_ap_special", special)):
        path = os.path.join(GOLD, name + ".pt")
        torch.save(g, path)
        print(path, os.path.getsize(path), "bytes; mAP plain / difficult:",
              float(g["ap64_plain"].mean()), float(g["ap64_difficult"].mean()))


if __name__ == "__main__":
    main()
