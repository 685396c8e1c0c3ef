"""Golden vectors of the REFERENCE's loss bookkeeping (engine.py:144-169 driving util/misc.py's MetricLogger / SmoothedValue), written
by running the reference's own classes in the build container (util.misc imported through tools/ref_harness.install_shims()):

    python tools/gen_steplog_golden.py

A no-op without the reference checkout.  A seeded sequence of 45 steps x 12 loss keys is pushed through the statements of
engine.py:144-169 (the weighted sum, reduce_dict, the scaled / unscaled dicts, the isfinite test, the three metric_logger.update
calls): two keys outside the weight dict, zero weights, a weight change at step 25 (the epoch curriculum), exact ties inside a window,
the window-1 meters lr and class_error, magnitudes from 1e-8 to 1e4 and a weight that is no fp32 number.

-> tests/golden/steplog_small.pt (data only): the inputs of every step, the bits of `losses` at every step, and at steps
   {0, 1, 19, 20, 21, 44} str(metric_logger) and the five properties of every meter.
-> tests/golden/steplog_edges.pt: short sequences with non-finite values and the step at which the reference's isfinite test trips
   (-1: never), with str(metric_logger) after the last step of a sequence that never trips.
Deterministic: the files regenerate bit for bit."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.ref_harness import REF, install_shims  # noqa: E402

KEYS = ["loss_ce", "class_error", "loss_bbox", "loss_giou", "cardinality_error", "loss_img_label", "loss_ce_0", "loss_bbox_0",
        "loss_giou_0", "ref_1_loss_ce", "ref_1_loss_bbox", "ref_1_loss_giou"]
UNWEIGHTED = ("class_error", "cardinality_error")
SNAP = (0, 1, 19, 20, 21, 44)
FIELDS = ("median", "avg", "global_avg", "max", "value")


def small_case():
    rng = np.random.default_rng(4711)
    base = {k: w for k, w in zip([k for k in KEYS if k not in UNWEIGHTED], [2.0, 5.0, 2.0, 1.0, 2.0, 5.0, 0.3, 0.0, 0.0, 0.0])}
    late = dict(base, ref_1_loss_ce=2.0, ref_1_loss_bbox=5.0, ref_1_loss_giou=0.3, loss_img_label=0.0)
    scale = 10.0 ** rng.uniform(-8, 4, len(KEYS))                       # one magnitude per key, 1e-8 .. 1e4
    scale[0], scale[-1] = 1e-8, 1e4
    steps = []
    for s in range(45):
        v = (scale * rng.uniform(0.5, 1.5, len(KEYS))).astype(np.float32)
        v[3] = np.float32([0.25, 0.75, 0.5][int(rng.integers(0, 3))])    # exact ties inside every window
        v[1] = np.float32(100.0 - 2.0 * s)                               # class_error
        v[7] = np.float32(-v[7]) if s % 5 == 0 else v[7]                 # a key that changes sign
        steps.append({"values": torch.from_numpy(v), "weight_dict": dict(base if s < 25 else late), "lr": 1e-4 if s < 30 else 1e-5})
    return steps


def edge_cases():
    f = lambda *rows: [torch.tensor(r, dtype=torch.float32) for r in rows]
    keys, wd = ["a", "class_error", "b"], {"a": 1.0, "b": 0.0}
    inf, nan = float("inf"), float("nan")
    return {"keys": keys, "weight_dict": wd, "cases": {
        "inf_masked": f([1, 2, 3], [2, 2, 3], [inf, 2, 3], [1, 2, 3]),
        "nan_unmasked": f([1, 2, 3], [2, nan, 3], [3, 2, 3], [1, inf, 3]),
        "zero_times_nan": f([1, 2, 3], [1, 2, nan], [1, 2, 3]),
        "inf_minus_inf": f([inf, 2, inf], [1, 2, 3]),
        "overflow": f([3e38, 2, 3], [1, 2, 3]),
        "finite": f([1, 2, 3], [-0.0, 2, 3], [1e-42, 2, 3]),
    }, "weight_dicts": {"inf_minus_inf": {"a": 1.0, "b": -1.0}, "overflow": {"a": 2.0, "b": 0.0}}}


def drive(misc, keys, steps, snap=()):
    """engine.py:101-103, 144-169, statement for statement.  -> (bits of `losses` per step, snapshots, tripping step, logger)."""
    ml = misc.MetricLogger(delimiter="  ")
    ml.add_meter("lr", misc.SmoothedValue(window_size=1, fmt="{value:.6f}"))
    ml.add_meter("class_error", misc.SmoothedValue(window_size=1, fmt="{value:.2f}"))
    bits, shots, trip = [], {}, -1
    for i, st in enumerate(steps):
        loss_dict = {k: st["values"][j].clone() for j, k in enumerate(keys)}
        weight_dict = st["weight_dict"]
        losses = sum(loss_dict[k] * weight_dict[k] for k in loss_dict.keys() if k in weight_dict)
        bits.append(int(losses.view(torch.int32)))
        loss_dict_reduced = misc.reduce_dict(loss_dict)
        loss_dict_reduced_unscaled = {f"{k}_unscaled": v for k, v in loss_dict_reduced.items()}
        loss_dict_reduced_scaled = {k: v * weight_dict[k] for k, v in loss_dict_reduced.items() if k in weight_dict}
        losses_reduced_scaled = sum(loss_dict_reduced_scaled.values())
        loss_value = losses_reduced_scaled.item()
        if not math.isfinite(loss_value):
            trip = i
            break                                                         # the reference exits here
        ml.update(loss=loss_value, **loss_dict_reduced_scaled, **loss_dict_reduced_unscaled)
        ml.update(class_error=loss_dict_reduced["class_error"])
        ml.update(lr=st["lr"])
        if i in snap:
            shots[i] = {"str": str(ml), "meters": {n: {f: float(getattr(m, f)) for f in FIELDS} for n, m in ml.meters.items()}}
    return bits, shots, trip, ml


def main():
    if not os.path.isdir(REF):
        print("no reference checkout at", REF, "- nothing to do")
        return
    install_shims()
    import util.misc as misc
    steps = small_case()
    bits, shots, trip, ml = drive(misc, KEYS, steps, SNAP)
    assert trip == -1 and sorted(shots) == list(SNAP)
    rec = {"keys": KEYS, "steps": steps, "losses_bits": torch.tensor(bits, dtype=torch.int32), "snapshots": shots,
           "global_avg": {k: float(m.global_avg) for k, m in ml.meters.items()}}
    path = os.path.join(ROOT, "tests", "golden", "steplog_small.pt")
    torch.save(rec, path)
    print("wrote", path, os.path.getsize(path), "bytes;", len(steps), "steps x", len(KEYS), "keys;", shots[44]["str"][:120], "...")

    e = edge_cases()
    out = {"keys": e["keys"], "cases": {}}
    for name, rows in e["cases"].items():
        wd = e["weight_dicts"].get(name, e["weight_dict"])
        sts = [{"values": r, "weight_dict": wd, "lr": 1e-4} for r in rows]
        bits, _, trip, ml = drive(misc, e["keys"], sts)
        out["cases"][name] = {"steps": sts, "losses_bits": torch.tensor(bits, dtype=torch.int32), "trip": trip,
                              "str": str(ml) if trip == -1 else None}
        print(name, "trips at", trip)
    path = os.path.join(ROOT, "tests", "golden", "steplog_edges.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
