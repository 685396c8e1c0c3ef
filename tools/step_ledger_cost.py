#!/usr/bin/env python
"""What the loss bookkeeping of a training step costs at cfg2 on one GPU: bench.py's step in three forms, timed
in ONE process on the same model, optimizer and batch:

  1 stacked   no bookkeeping beyond the stacked total (bench.py's step as it is)
  2 reference engine.py:144-169 restated: per-key products and sum(), reduce_dict's dicts, .item() BEFORE the backward for the isfinite
              guard, MetricLogger.update's .item() per value (~95) after the optimizer step
  3 ledger    spe_amd.steplog.StepLedger.record, str(ledger) every 100 steps

    python tools/step_ledger_cost.py [--steps 50] [--warmup 3] [--rounds 2] [--out profiles/step_ledger.txt]

Each round times the forms as blocks of --steps steps in the order 1 2 3 and then 3 2 1 (drift and warm-up effects hit every form from
both sides).  Per block: wall ms / step (device idle before and after) and host ms / step (until the last step is enqueued).  The
report gives every block, the mean and the spread (min .. max) per form."""
import argparse
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)         # 4 blocks of 50: the ledger's every-100th-step summary falls into two of them
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_ledger.txt"))
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps must be >= 20")

    from spe_amd import build as _build
    if _build.needs_build():
        _build.build()
    from spe_amd import kernels as K, lib
    from spe_amd.dp import GradAllReducer
    from spe_amd.engine import get_refine_weight_dict
    from spe_amd.models import build_model
    from spe_amd.optim import FlatAdamW
    from spe_amd.steplog import SmoothedValue, StepLedger
    from spe_amd.util.misc import NestedTensor
    lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    K.set_precision("bf16s")
    K.manual_seed(1234)
    args = bench.model_args()
    torch.manual_seed(0)
    model, crit, crit_r, pp, rpp = build_model(args)
    model.to(dev).train(); crit.to(dev).train(); crit_r.to(dev).train()
    wd = crit.weight_dict
    wd_ref = get_refine_weight_dict(dict(wd), 1, header="ref")
    params = [p for p in model.parameters() if p.requires_grad]
    reducer = GradAllReducer(params, flatten_params=True)
    groups = [{"params": [p for n, p in model.named_parameters() if "backbone" not in n and p.requires_grad], "lr": 1e-4},
              {"params": [p for n, p in model.named_parameters() if "backbone" in n and p.requires_grad], "lr": 1e-5}]
    opt = FlatAdamW(groups, reducer, lr=1e-4, weight_decay=1e-4, max_grad_norm=0.1)
    torch.manual_seed(1234)
    img, mask, targets = bench.synth_batch(1234, dev)
    samples = NestedTensor(img, mask)

    def losses():
        out = model(samples)
        l0 = crit(out[0], targets)
        with torch.no_grad():
            ps = bench.pseudo_labels(rpp, out[0], targets)
        return l0, crit_r(out[1], ps)

    def merged(l0, l1):
        d = dict(l0)
        for k, v in l1.items():
            d[f"ref_1_{k}"] = v
        return d

    def step_stacked(i, st):
        reducer.reset()
        l0, l1 = losses()
        total = bench.weighted_total(l0, l1, wd)
        total.backward()
        reducer.finish()
        opt.step()

    def step_reference(i, st):
        reducer.reset()
        loss_dict = merged(*losses())
        total = sum(loss_dict[k] * wd_ref[k] for k in loss_dict.keys() if k in wd_ref)
        unscaled = {f"{k}_unscaled": v for k, v in loss_dict.items()}
        scaled = {k: v * wd_ref[k] for k, v in loss_dict.items() if k in wd_ref}
        value = sum(scaled.values()).item()                                  # drains the queue between forward and backward
        if not math.isfinite(value):
            raise SystemExit("Loss is {}, stopping training".format(value))
        total.backward()
        reducer.finish()
        opt.step()
        meters = st.setdefault("meters", {})
        for k, v in [("loss", value)] + list(scaled.items()) + list(unscaled.items()) + \
                [("class_error", loss_dict["class_error"]), ("lr", opt.param_groups[0]["lr"])]:
            meters.setdefault(k, SmoothedValue()).update(v.item() if torch.is_tensor(v) else v)
        st["reads"] = 1 + sum(torch.is_tensor(v) for v in list(scaled.values()) + list(unscaled.values())) + 1

    def step_ledger(i, st):
        reducer.reset()
        loss_dict = merged(*losses())
        led = st.setdefault("ledger", StepLedger(windows={"lr": 1, "class_error": 1}, fmts={"lr": "{value:.6f}", "class_error": "{value:.2f}"},
                                                 delimiter="  "))
        total = led.record(loss_dict, wd_ref, lr=opt.param_groups[0]["lr"])
        total.backward()
        reducer.finish()
        opt.step()
        if st["n"] % 100 == 0:
            st["line"] = str(led)
        st["n"] += 1

    forms = [("1 stacked", step_stacked), ("2 reference", step_reference), ("3 ledger", step_ledger)]
    state = [{"n": 0} for _ in forms]
    for f, (_, fn) in enumerate(forms):
        for i in range(a.warmup):
            fn(i, state[f])
    torch.cuda.synchronize()
    blocks = [[] for _ in forms]
    for r in range(a.rounds):
        for order in ((0, 1, 2), (2, 1, 0)):
            for f in order:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(a.steps):
                    forms[f][1](i, state[f])
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                blocks[f].append(((t2 - t0) / a.steps * 1e3, (t1 - t0) / a.steps * 1e3))

    lines = ["step ledger: cost of the loss bookkeeping at cfg2 (TSCAM_cait_S24, 2 x 3x800x1333, bf16s, 1 GPU: %s)" % torch.cuda.get_device_name(dev),
             "tools/step_ledger_cost.py --steps %d --warmup %d --rounds %d: %d blocks per form, orders 1 2 3 / 3 2 1 per round" %
             (a.steps, a.warmup, a.rounds, 2 * a.rounds),
             "loss keys per step: %d (%d weighted); host reads per step of form 2: %d" %
             (state[2]["ledger"].K, sum(state[2]["ledger"].masked), state[1]["reads"]), "",
             "%-12s %10s %19s %10s %19s   blocks (wall ms/step)" % ("form", "wall ms", "spread", "host ms", "spread")]
    mean = {}
    for f, (name, _) in enumerate(forms):
        wall, host = [b[0] for b in blocks[f]], [b[1] for b in blocks[f]]
        mean[f] = sum(wall) / len(wall)
        lines.append("%-12s %10.2f %8.2f .. %-8.2f %10.2f %8.2f .. %-8.2f   %s" %
                     (name, mean[f], min(wall), max(wall), sum(host) / len(host), min(host), max(host), " ".join("%.2f" % w for w in wall)))
    lines += ["", "form 2 - form 1: %+.2f ms/step; form 3 - form 1: %+.2f ms/step" % (mean[1] - mean[0], mean[2] - mean[0]),
              "wall: device idle -> all steps done; host: until the last step's work is enqueued (form 2's host time contains its waits)",
              "log line of form 3: " + state[2].get("line", "")[:160]]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
