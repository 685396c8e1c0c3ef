"""Step ledger: the loss bookkeeping of a training step without host round trips (reference engine.py:134-169 with
util/misc.py:34-93, 139-253 behind it; csrc/step_ledger.hip).

    ledger = StepLedger(windows={"lr": 1, "class_error": 1}, fmts={"lr": "{value:.6f}", "class_error": "{value:.2f}"}, delimiter="  ")
    for samples, targets in ledger.log_every(loader, 100, header):
        ...
        total = ledger.record(loss_dict, weight_dict, lr=opt.param_groups[0]["lr"])    # one launch, nothing read back
        total.backward()

The reference multiplies and adds the ~52 loss scalars one launch at a time, reads the weighted sum back BEFORE the backward for its
isfinite guard and reads ~95 scalars back after the optimizer step for its meters.  Here `record` is one stack and one launch that
returns the total to back-propagate and files every value in device-resident meters; `str(ledger)`, `summary()`, `global_avg()` and
`check()` are the only host reads (one launch and one copy).  The non-finite stop therefore comes at the next log line or at the end
of the epoch, not before the optimizer step of the bad iteration.

Meters carry the reference's names in the reference's order: the meters announced through `windows` / `fmts` (add_meter), `loss`,
the keys of the weight dict, every key + "_unscaled", then the host scalars.  An announced meter that repeats a loss key outside the
weight dict (`class_error`, engine.py:103, 168) shows that key's newest value; it takes window 1.

CPU tensors take a numpy path with the same arithmetic on the same state layout, so the class also runs without a GPU and over gloo."""
import datetime
import time
from collections import deque

import numpy as np
import torch
import torch.distributed as dist

from . import kernels as K
from .util.misc import host_to_device

D, MAX_K, MAX_E = K.LEDGER_D, K.LEDGER_MAX_K, K.LEDGER_MAX_E
FIELDS = ("median", "avg", "global_avg", "max", "value")
DEFAULT_FMT = "{median:.4f} ({global_avg:.4f})"


def state_layout(Kk, E):
    """Byte offsets of the state block (include/spe_hip.h): totals, extras ring, value ring, weight ring, mask, size."""
    M = 2 * Kk + 1 + E
    tot = 32
    re_ = tot + 8 * M
    rv = re_ + 8 * D * E
    rw = rv + 4 * D * Kk
    mk = rw + 4 * D * Kk
    return {"totals": tot, "ring_e": re_, "ring_v": rv, "ring_w": rw, "mask": mk, "bytes": mk + ((Kk + 7) & ~7)}


def _views(state, Kk, E):
    """Typed torch views of a state block (either device)."""
    L = state_layout(Kk, E)
    M = 2 * Kk + 1 + E
    return {"head": state[:32].view(torch.int64), "totals": state[L["totals"]:L["ring_e"]].view(torch.float64),
            "ring_e": state[L["ring_e"]:L["ring_v"]].view(torch.float64).view(D, E),
            "ring_v": state[L["ring_v"]:L["ring_w"]].view(torch.float32).view(D, Kk),
            "ring_w": state[L["ring_w"]:L["mask"]].view(torch.float32).view(D, Kk),
            "mask": state[L["mask"]:L["mask"] + Kk], "M": M}


# ---- the host path: spe_ledger_record / spe_ledger_summary restated in numpy, operation for operation ----------------------------
def record_host(vals, weights, mask, extras, state):
    Kk, E = vals.numel(), len(extras)
    s = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in _views(state, Kk, E).items()}
    v, w, m = vals.detach().numpy().astype(np.float32), weights.numpy(), mask.numpy() != 0
    step = int(s["head"][0])
    row = step % D
    with np.errstate(all="ignore"):
        sc = v * w                                                   # fp32 products, each rounded
        t = np.float32(0.0)
        for k in range(Kk):
            if m[k]:
                t = np.float32(t + sc[k])
        s["ring_v"][row], s["ring_w"][row], s["mask"][:] = v, w, m
        ex = np.asarray(extras, np.float64).reshape(E)
        s["ring_e"][row] = ex
        tot = s["totals"]
        tot[:Kk] += v.astype(np.float64)
        tot[Kk:2 * Kk][m] += sc.astype(np.float64)[m]
        tot[2 * Kk] += np.float64(t)
        tot[2 * Kk + 1:] += ex
    if not np.isfinite(t) and s["head"][1] == 0:
        s["head"][1] = step + 1
    s["head"][0] = step + 1
    return torch.tensor(t, dtype=torch.float32)


def summary_host(state, Kk, E, windows, ring=None, order=None):
    s = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in _views(state, Kk, E).items()}
    M, steps = s["M"], int(s["head"][0])
    out = np.full((M * 5 + 2,), np.nan)
    out[M * 5], out[M * 5 + 1] = steps, s["head"][1]
    rv = s["ring_v"] if ring is None else ring.numpy().reshape(D, Kk)
    rw, msk = s["ring_w"], s["mask"] != 0
    order = list(range(Kk)) if order is None else [int(k) for k in order]
    with np.errstate(all="ignore"):
        for m in range(M):
            n = min(steps, int(windows[m]))
            if n <= 0:
                continue
            rows = [(steps - n + i) % D for i in range(n)]
            if m < Kk:
                xd = rv[rows, m].astype(np.float64)
            elif m < 2 * Kk:
                xd = (rv[rows, m - Kk] * rw[rows, m - Kk]).astype(np.float64)
            elif m == 2 * Kk:
                sc = rv[rows] * rw[rows]
                t = np.zeros((n,), np.float32)
                for k in order:
                    if msk[k]:
                        t = t + sc[:, k]
                xd = t.astype(np.float64)
            else:
                xd = s["ring_e"][rows, m - 2 * Kk - 1].copy()
            xf = xd.astype(np.float32)
            nan = bool(np.isnan(xd).any())
            mx = xd[0]
            for x in xd[1:]:
                if x > mx:
                    mx = x
            o = out[m * 5:m * 5 + 5]
            o[0] = np.nan if nan else np.float64(xf[np.argsort(xf, kind="stable")[(n - 1) // 2]])
            o[1] = np.float64(np.float32(np.cumsum(xd)[-1] / np.float64(n)))
            o[2] = s["totals"][m] / np.float64(steps)
            o[3] = np.nan if nan else mx
            o[4] = xd[-1]
    return torch.from_numpy(out)


class SmoothedValue(object):
    """The reference's host meter (util/misc.py:34-93), restated: for what is measured on the host anyway (iteration / data time)."""

    def __init__(self, window_size=20, fmt=None):
        self.deque = deque(maxlen=window_size)
        self.total, self.count, self.fmt = 0.0, 0, DEFAULT_FMT if fmt is None else fmt

    def update(self, value, n=1):
        self.deque.append(value)
        self.count += n
        self.total += value * n

    median = property(lambda self: torch.tensor(list(self.deque)).median().item())
    avg = property(lambda self: torch.tensor(list(self.deque), dtype=torch.float32).mean().item())
    global_avg = property(lambda self: self.total / self.count)
    max = property(lambda self: max(self.deque))
    value = property(lambda self: self.deque[-1])

    def __str__(self):
        return self.fmt.format(median=self.median, avg=self.avg, global_avg=self.global_avg, max=self.max, value=self.value)


class StepLedger(object):
    def __init__(self, windows=None, window=20, fmts=None, delimiter="\t", group=None):
        self.windows, self.fmts = dict(windows or {}), dict(fmts or {})
        self.window, self.delimiter, self.group = int(window), delimiter, group
        for name, w in list(self.windows.items()) + [("window", self.window)]:
            if not 1 <= int(w) <= D:
                raise ValueError(f"StepLedger: the window of {name!r} is {w}; a window is 1 .. {D} steps (the ring's depth)")
        self.announced = list(dict.fromkeys(list(self.windows) + list(self.fmts)))       # add_meter order
        self.keys = None

    # ---- recording ------------------------------------------------------------------------------------------------------------
    def _start(self, loss_dict, weight_dict, extras):
        keys, enames = list(loss_dict), list(extras)
        if not 1 <= len(keys) <= MAX_K:
            raise ValueError(f"StepLedger: {len(keys)} loss values per step; the ledger takes 1 .. {MAX_K}")
        if len(enames) > MAX_E:
            raise ValueError(f"StepLedger: {len(enames)} host scalars per step; the ledger takes at most {MAX_E}")
        first = loss_dict[keys[0]]
        self.device = first.device
        self.keys, self.enames, self.K, self.E = keys, enames, len(keys), len(enames)
        self.masked = [k in weight_dict for k in keys]
        self.alias = {}                          # announced meter -> index of the loss key it repeats (engine.py:168)
        for name in self.announced:
            if name in keys and not self.masked[keys.index(name)]:
                if int(self.windows.get(name, self.window)) != 1:
                    raise ValueError(f"StepLedger: the meter {name!r} repeats a loss key; such a meter takes window 1")
                self.alias[name] = keys.index(name)
        Kk, E = self.K, self.E
        self.M = 2 * Kk + 1 + E
        win = [self.window] * self.M
        for i, k in enumerate(keys):
            win[i] = int(self.windows.get(k + "_unscaled", self.window))
            win[Kk + i] = int(self.windows.get(k, self.window)) if self.masked[i] else self.window
        win[2 * Kk] = int(self.windows.get("loss", self.window))
        for j, e in enumerate(enames):
            win[2 * Kk + 1 + j] = int(self.windows.get(e, self.window))
        self._win_host = torch.tensor(win, dtype=torch.int32)
        nbytes = K.ledger_state_bytes(Kk, E) if self.device.type == "cuda" else state_layout(Kk, E)["bytes"]
        assert nbytes == state_layout(Kk, E)["bytes"]
        self.state = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        self._win_dev = host_to_device(win, torch.int32, self.device)
        self._mask = host_to_device([int(m) for m in self.masked], torch.uint8, self.device)
        self._order = host_to_device(sorted(range(Kk), key=lambda i: keys[i]), torch.int32, self.device)     # reduce_dict's sorted keys
        self._wkey, self._weights = None, None

    def record(self, loss_dict, weight_dict, **extras):
        """File one step; -> the 0-dim weighted total sum_k weight_dict[k] * loss_dict[k] (keys of loss_dict in their order), with grad.
        extras: host scalars of the step (lr=...).  Nothing is read back."""
        if self.keys is None:
            self._start(loss_dict, weight_dict, extras)
        if list(loss_dict) != self.keys or list(extras) != self.enames:
            raise ValueError("StepLedger.record: the loss keys (or the host scalars) differ from those of the first step, or come in another order")
        if [k in weight_dict for k in self.keys] != self.masked:
            raise ValueError("StepLedger.record: the set of weighted keys changed; only their weights may")
        wkey = tuple(float(weight_dict[k]) if m else 0.0 for k, m in zip(self.keys, self.masked))
        if wkey != self._wkey:                   # by value: the epoch curriculum (engine.py:134-142) changes weights a few times per run
            self._weights, self._wkey = host_to_device(list(wkey), torch.float32, self.device), wkey
        from . import ops
        vals = torch.cat([(loss_dict[k] if m else loss_dict[k].detach()).reshape(1) for k, m in zip(self.keys, self.masked)])
        if vals.dtype != torch.float32:
            raise TypeError(f"StepLedger.record: loss values must be float32, got {vals.dtype}")
        return ops.ledger_total(vals, self._weights, self._mask, [float(extras[e]) for e in self.enames], self.state)

    # ---- reading --------------------------------------------------------------------------------------------------------------
    def _world(self):
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    def _names(self, world):
        """[(name, row of the summary table or ('alias', key index))] in the reference's meter order."""
        Kk = self.K
        idx = sorted(range(Kk), key=lambda i: self.keys[i]) if world > 1 else range(Kk)
        rows = [("loss", 2 * Kk)] + [(self.keys[i], Kk + i) for i in idx if self.masked[i]] + \
               [(self.keys[i] + "_unscaled", i) for i in idx] + [(e, 2 * Kk + 1 + j) for j, e in enumerate(self.enames)]
        have = dict(rows)
        for name, i in self.alias.items():
            have[name] = ("alias", i)
        first = [n for n in self.announced if n in have]
        return [(n, have[n]) for n in first] + [(n, r) for n, r in rows if n not in first]

    def _raise_bad(self, bad_plus1):
        step = int(bad_plus1) - 1
        v = _views(self.state, self.K, self.E)
        steps = int(v["head"][0])
        vals = dict(zip(self.keys, v["ring_v"][step % D].tolist())) if steps - step <= D else None
        raise FloatingPointError(f"Loss is not finite at step {step}, stopping training", step, vals)

    def summary(self):
        """{meter: {median, avg, global_avg, max, value}} in the reference's meter order: one summary launch and one device -> host
        copy (with more than one rank: plus the all-reduce of the ring, of the totals and of the first bad step).  Raises
        FloatingPointError like check()."""
        if self.keys is None:
            return {}
        Kk, E, M, world = self.K, self.E, self.M, self._world()
        cuda = self.device.type == "cuda"
        ring = order = None
        if world > 1:
            ring = _views(self.state, Kk, E)["ring_v"].clone()           # reduce_dict: all-reduce (sum), then / world in fp32
            dist.all_reduce(ring, group=self.group)
            ring /= world
            order = self._order
        if cuda:
            tab = K.ledger_summary(self.state, Kk, E, self._win_host, self._win_dev, ring, order)
        else:
            tab = summary_host(self.state, Kk, E, self._win_host.tolist(), ring, None if order is None else order.tolist())
        if world > 1:
            tot = torch.cat([_views(self.state, Kk, E)["totals"], tab[M * 5:M * 5 + 1]])
            dist.all_reduce(tot, group=self.group)                         # SmoothedValue.synchronize_between_processes
            bad = tab[M * 5 + 1:].clone()
            bad[bad == 0] = float("inf")
            dist.all_reduce(bad, op=dist.ReduceOp.MIN, group=self.group)
            tab = torch.cat([tab[:M * 5], tot, bad])
        host = tab.cpu().numpy()                                           # the one copy
        t5 = host[:M * 5].reshape(M, 5)
        if world > 1:
            t5[:, 2] = host[M * 5:M * 6] / host[M * 6]
            bad = host[M * 6 + 1]
            bad = 0 if np.isinf(bad) else bad
        else:
            bad = host[M * 5 + 1]
        if bad:
            self._raise_bad(bad)
        out = {}
        for name, r in self._names(world):
            if isinstance(r, tuple):
                val, ga = float(t5[r[1], 4]), float(t5[r[1], 2])
                out[name] = {"median": float(np.float32(val)), "avg": float(np.float32(val)), "global_avg": ga, "max": val, "value": val}
            else:
                out[name] = dict(zip(FIELDS, (float(x) for x in t5[r])))
        return out

    def check(self):
        """Raise FloatingPointError(message, first bad step, that step's loss values) if the weighted total of any recorded step - on
        any rank - was not finite.  Sticky: later finite steps do not clear it.  One small host read."""
        if self.keys is None:
            return
        bad = _views(self.state, self.K, self.E)["head"][1:2].to(torch.float64)
        if self._world() > 1:
            bad = bad.clone()
            bad[bad == 0] = float("inf")
            dist.all_reduce(bad, op=dist.ReduceOp.MIN, group=self.group)
        b = float(bad.cpu()[0])
        if b and not np.isinf(b):
            self._raise_bad(b)

    def global_avg(self):
        """{meter: global average}: what train_one_epoch_refine returns (engine.py:174), synchronised between the ranks."""
        return {k: v["global_avg"] for k, v in self.summary().items()}

    def __str__(self):
        return self.delimiter.join("{}: {}".format(name, self.fmts.get(name, DEFAULT_FMT).format(**five)) for name, five in self.summary().items())

    def log_every(self, iterable, print_freq, header=None):
        """MetricLogger.log_every (util/misc.py:201-253): the same lines; the meters are read only on the steps that print."""
        i = 0
        header = header or ""
        start_time = end = time.time()
        iter_time, data_time = SmoothedValue(fmt="{avg:.4f}"), SmoothedValue(fmt="{avg:.4f}")
        space_fmt = ":" + str(len(str(len(iterable)))) + "d"
        parts = [header, "[{0" + space_fmt + "}/{1}]", "eta: {eta}", "{meters}", "time: {time}", "data: {data}"]
        cuda = torch.cuda.is_available()
        if cuda:
            parts.append("max mem: {memory:.0f}")
        log_msg = self.delimiter.join(parts)
        MB = 1024.0 * 1024.0
        for obj in iterable:
            data_time.update(time.time() - end)
            yield obj
            iter_time.update(time.time() - end)
            if i % print_freq == 0 or i == len(iterable) - 1:
                eta = str(datetime.timedelta(seconds=int(iter_time.global_avg * (len(iterable) - i))))
                kw = {"memory": torch.cuda.max_memory_allocated() / MB} if cuda else {}
                print(log_msg.format(i, len(iterable), eta=eta, meters=str(self), time=str(iter_time), data=str(data_time), **kw))
            i += 1
            end = time.time()
        total_time = time.time() - start_time
        print("{} Total time: {} ({:.4f} s / it)".format(header, str(datetime.timedelta(seconds=int(total_time))), total_time / len(iterable)))
