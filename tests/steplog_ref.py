"""numpy restatement of the step ledger (spe_amd/steplog.py, csrc/step_ledger.hip) and of the reference's meters behind it
(engine.py:144-169, util/misc.py:34-93): a plain list of steps, no ring, no state block.

  total      sequential fp32: ((0 + v0 w0) + v1 w1) + ... over the keys of the weight dict, in the order given
  tree_total the same products added pairwise - NOT what the ledger computes; used to prove that a case tells the orders apart
  totals     fp64 running sums of the fp32 values, in step order
  median     float32 sorted[(n - 1) // 2] (torch.median's lower median), ties by position
  avg        float32(fp64 in-order sum / n)
  max        the first of the largest values (Python's max), NaN when the window holds one; value: the newest"""
import numpy as np

FIELDS = ("median", "avg", "global_avg", "max", "value")
DEFAULT_FMT = "{median:.4f} ({global_avg:.4f})"


def seq_total(v, w, mask, order=None):
    v, w = np.asarray(v, np.float32), np.asarray(w, np.float32)
    with np.errstate(all="ignore"):
        s = v * w
        t = np.float32(0.0)
        for k in (range(len(v)) if order is None else order):
            if mask[k]:
                t = np.float32(t + s[k])
    return t


def tree_total(v, w, mask):
    with np.errstate(all="ignore"):
        s = [x for x, m in zip(np.asarray(v, np.float32) * np.asarray(w, np.float32), mask) if m]
        while len(s) > 1:
            s = [np.float32(s[i] + s[i + 1]) if i + 1 < len(s) else s[i] for i in range(0, len(s), 2)]
    return s[0] if s else np.float32(0.0)


def five(series, window, total=None, count=None):
    """The five statistics of a meter whose values (Python floats / doubles, in step order) are `series`."""
    xd = np.asarray(series[-window:], np.float64)
    n = xd.size
    xf = xd.astype(np.float32)
    nan = bool(np.isnan(xd).any())
    mx = xd[0]
    for x in xd[1:]:
        if x > mx:
            mx = x
    s = np.float64(0.0)
    for x in xd:
        s = s + x
    if total is None:
        total = np.float64(0.0)
        with np.errstate(all="ignore"):
            for x in series:
                total = total + np.float64(x)
        count = len(series)
    with np.errstate(all="ignore"):
        return {"median": float("nan") if nan else float(xf[np.argsort(xf, kind="stable")[(n - 1) // 2]]),
                "avg": float(np.float32(s / np.float64(n))), "global_avg": float(total / np.float64(count)),
                "max": float("nan") if nan else float(mx), "value": float(xd[-1])}


class RefLedger(object):
    """steps: list of (values fp32 [K], weights fp32 [K], extras [E]); mask bool [K]; windows: per row of the ledger's table
    (K unscaled, K scaled, loss, E extras)."""

    def __init__(self, mask, windows, order=None):
        self.mask, self.windows, self.order = list(mask), list(windows), order
        self.series = None
        self.totals, self.bad, self.steps = [], None, 0

    def record(self, v, w, extras=()):
        v, w = np.asarray(v, np.float32), np.asarray(w, np.float32)
        K = len(v)
        with np.errstate(all="ignore"):
            s = v * w
        t = seq_total(v, w, self.mask)
        logged = t if self.order is None else seq_total(v, w, self.mask, self.order)
        row = [float(x) for x in v] + [float(x) for x in s] + [float(logged)] + [float(e) for e in extras]
        if self.series is None:
            self.series = [[] for _ in row]
        for i, x in enumerate(row):
            if K <= i < 2 * K and not self.mask[i - K]:
                continue
            self.series[i].append(x)
        if not np.isfinite(t) and self.bad is None:
            self.bad = self.steps
        self.steps += 1
        return t

    def table(self):
        """[M, 5] float64; rows of unmasked scaled slots are NaN except global_avg = 0 / steps."""
        out = np.full((len(self.series), 5), np.nan)
        for i, ser in enumerate(self.series):
            if ser:
                f = five(ser, self.windows[i])
                out[i] = [f[k] for k in FIELDS]
        return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def avg_bound(series, window):
    """Any-order fp32 summation bound the reference's float32 mean is held to: (n - 1) 2^-24 sum|x| / n + 2^-24 |avg|."""
    x = np.abs(np.asarray(series[-window:], np.float64))
    n = x.size
    return (n - 1) * 2.0 ** -24 * x.sum() / n + 2.0 ** -24 * abs(np.asarray(series[-window:], np.float64).sum() / n)
