"""Optimiser step of the SPE training loop (reference engine.py:161-165 + main.py:177-191):

    torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)      # 0.1 in the reference scripts
    optimizer.step()                                                  # torch.optim.AdamW, 3 LR groups

as two HIP launches per gradient bucket (csrc/optim.hip) on the flat buffers of spe_amd.dp.GradAllReducer
(flatten_params=True): parameters, gradients and both Adam moments share one layout, the global gradient norm is
reduced from per-block partial sums inside the update kernel (no host round trip), and the per-group learning
rate / weight decay come from a small segment table.  FlatAdamW is a torch.optim.Optimizer: `param_groups`,
LR schedulers (StepLR in the reference) and state_dict()/load_state_dict() keep working; the per-parameter state
entries are views into the flat moment buffers.

FlatAdamW(..., skip_nonfinite=True) is the guarded step: one more one-workgroup launch decides on the device, from the norm partials
that are there anyway, whether the reduced gradient is finite, and the update launches leave parameters, moments and gradients
untouched when it is not (see the class docstring).

FlatAdamW(..., ema_decay=d) keeps an exponential moving average of the weights as one more flat fp32 buffer per bucket, updated by the
update launch itself; `with optimizer.ema_weights():` swaps it into the parameters for an evaluation (see the class docstring).

FlatAdamW(..., skip_nonfinite=True, skip_report="first" | "last") makes the guard's decision explainable: one gated spe_grad_report per bucket
(csrc/grad_report.hip) writes, on a skipped step only, a record per parameter - NaN / inf counts, the first bad index, squared norm and
largest magnitude of the gradient, the weight norm - and skip_report() reads it on the host afterwards.  grad_stats() is the same table
on demand (per-layer gradient / weight norms for logging).
"""
import contextlib
import math

import torch

from . import kernels as K
from .util.misc import host_to_device

_NORM_BLOCKS = 256


class FlatAdamW(torch.optim.Optimizer):
    """skip_nonfinite=False: two launches per bucket (one without clipping), bias corrections from the host's step count.

    skip_nonfinite=True: every step() runs the squared-norm pass of every bucket (also with max_grad_norm unset: no clip then), ONE gate
    launch (spe_adamw_gate) and one guarded update per bucket (spe_adamw_flat_guarded).  The gate sums the partials and applies the
    step only if that sum is finite: a NaN or an infinity anywhere in the gradient buckets skips it, and so does a squared norm that
    overflows fp32 (one element beyond ~1.8e19).  A skipped step writes nothing - parameters, both moments and the gradient buckets
    keep their bits - and does not advance the bias corrections: they follow the count of APPLIED steps, kept on the device, so the
    run continues as if the bad iteration had not happened.  step() reads nothing back; applied_steps(), skipped_steps() and
    first_skipped() are the host reads (each one small device-to-host copy: they synchronise).  `_step` counts attempts; the
    per-parameter `step` entries are one 0-dim device tensor inside the guard block that holds the applied count.
    * Gradient accumulation needs nothing special: a non-finite micro-step makes the accumulated sum non-finite, and the whole
      cycle is skipped.
    * Several ranks: the decision is a function of the all-reduced buckets only, which are identical on every rank, so every rank
      takes the same decision without a further collective.
    * Only the gradient decides.  A non-finite LOSS whose gradients are all finite is still applied; the step ledger
      (spe_amd.steplog) stops such a run at its next check, as before.

    ema_decay=d (0 <= d < 1; None: off, nothing allocated, the entries without the EMA are called): one more flat buffer per bucket,
    a bit copy of the parameters at construction, updated by every APPLIED step() inside the update launch (spe_adamw_flat_ema: the
    same number of launches, nothing read back) and by nothing else:
        e' = e + w * (p' - e)  in fp32,  w = float(1 - min(d, (1 + t) / (10 + t)))  (ema_warmup=False: w = float(1 - d))
    with p' the parameter the step has just computed and t the 1-based count of applied steps - a skipped step leaves the EMA and the
    warm-up where they were, and with gradient accumulation the EMA moves once per completed cycle.  Parameters are identical on
    every rank, so the EMA is too: no collective.
    * ema_of(p): a view into the EMA buffer shaped like p.  ema_state_dict(model) / load_ema_state_dict(model, sd): the EMA in the
      layout of model.state_dict() (a checkpoint's "model_ema").  state_dict() / load_state_dict() neither export nor touch it.
    * `with optimizer.ema_weights(): evaluate(...)` exchanges parameters and EMA on entry and again on exit (one spe_swap_flat per
      bucket, cached 16-bit operand copies invalidated both times).  Inside the block step(), ema_reset(), ema_state_dict(),
      load_ema_state_dict() and a second ema_weights() raise RuntimeError.
    * ema_reset(): see there - needed when model weights are loaded after the optimizer was built.

    skip_report="first" | "last" (None: off, nothing allocated, step() issues the launches it issues without it; needs skip_nonfinite):
    after the gate and before the update launches, step() issues one spe_grad_report per bucket, gated on the guard block - on an applied
    step every workgroup returns after reading the guard words; on a skipped step ("first": on the first skipped step of the run only,
    "last": on every skipped one, the latest overwrites) it writes one record per parameter from the buckets the skipped update then
    leaves untouched.  step() still reads nothing back; skip_report() is the host read, grad_stats() the same table on demand.
    What the report cannot resolve:
    * Gradient accumulation: it sees the accumulated sum of the cycle, not the micro-batch that poisoned it.
    * Several ranks: the buckets are identical on every rank after the all-reduce, so every rank holds the same report without a
      collective - and none can say which rank produced the value.
    * The records square grad_scale * g, the guard's norm squares g before it scales: with grad_scale < 1 an element in
      (1.8e19, 1.8e19 / grad_scale) skips the step without an infinite grad_sq of its own; such a step reads as a total overflow
      (below) with that parameter on top of "largest"."""

    def __init__(self, params, reducer, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None,
                 write_clipped_grads=True, skip_nonfinite=False, ema_decay=None, ema_warmup=True, skip_report=None):
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:          # NaN fails the comparison too
            raise ValueError(f"FlatAdamW: ema_decay must be None or in [0, 1), got {ema_decay}")
        if skip_report not in (None, "first", "last"):
            raise ValueError(f"FlatAdamW: skip_report must be None, 'first' or 'last', got {skip_report!r}")
        if skip_report is not None and not skip_nonfinite:
            raise ValueError("FlatAdamW: skip_report needs skip_nonfinite=True (it reports what the guard skipped)")
        if not getattr(reducer, "flatten_params", False):
            raise ValueError("FlatAdamW needs GradAllReducer(..., flatten_params=True)")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.reducer = reducer
        # Gradient averaging (1/world) rides on the update launch.  This changes what the reducer's buckets (and p.grad) hold
        # after finish(): the SUM over ranks (and over the micro-steps of an accumulation cycle, 1/(world * accum_steps) then), not DDP's
        # mean - any other consumer must multiply by reducer.grad_scale() (or read
        # reducer.averaged_grad(p)).  A reducer can therefore serve ONE FlatAdamW and nothing that expects means.
        if getattr(reducer, "_folded_into", None) not in (None, id(self)):
            raise ValueError("FlatAdamW: this GradAllReducer already folds its averaging into another optimizer")
        reducer.average_in_optimizer = True
        reducer._folded_into = id(self)
        self.max_grad_norm = max_grad_norm
        self.write_clipped_grads = write_clipped_grads
        gid = {}
        for gi, grp in enumerate(self.param_groups):
            if tuple(grp["betas"]) != tuple(self.param_groups[0]["betas"]) or grp["eps"] != self.param_groups[0]["eps"]:
                raise ValueError("FlatAdamW: betas / eps must be the same for all parameter groups")
            for p in grp["params"]:
                gid[p] = gi
        self._step = 0
        self.skip_nonfinite = bool(skip_nonfinite)
        dev = reducer.buckets[0]["flat"].device
        # ONE 0-dim step tensor shared by every parameter's state entry (torch.optim.AdamW semantics: optimizer.state[p]["step"] is always
        # current) and bumped by a single host op per step() - not 717 tensor increments.  Guarded: the applied count lives on the
        # device, so the shared tensor is the guard block's float copy of it, written by the gate launch.
        self._guard = None
        if self.skip_nonfinite:
            self._guard = torch.zeros((K.ADAMW_GUARD_WORDS,), device=dev, dtype=torch.int32)
            self._step_t = self._guard.view(torch.float32)[K.GUARD_STEP_F]
        else:
            self._step_t = torch.zeros((), dtype=torch.float32)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self._ema_swapped = False
        self._ema_views = {}
        self.skip_report_mode = skip_report          # (the method skip_report() is the host read)
        self._buckets = []
        for b in reducer.buckets:
            n = b["flat"].numel()
            m, v = torch.zeros_like(b["flat"]), torch.zeros_like(b["flat"])
            ema = torch.zeros_like(b["flat_p"]) if self.ema_decay is not None else None
            # runs of consecutive parameters of one group -> (segment end, group); padding follows its parameter
            ends, groups = [], []
            offs = b["offsets"]
            for i, (p, off) in enumerate(offs):
                if p not in gid:
                    raise ValueError("FlatAdamW: a parameter of the reducer is in no parameter group")
                end = offs[i + 1][1] if i + 1 < len(offs) else n
                if groups and groups[-1] == gid[p]:
                    ends[-1] = end
                else:
                    ends.append(end); groups.append(gid[p])
                st = self.state[p]
                st["step"] = self._step_t
                st["exp_avg"] = m[off:off + p.numel()].view_as(p)
                st["exp_avg_sq"] = v[off:off + p.numel()].view_as(p)
                if ema is not None:
                    self._ema_views[p] = ema[off:off + p.numel()].view_as(p)
            if len(ends) > 64:
                raise ValueError("FlatAdamW: more than 64 parameter-group runs in one bucket")
            self._buckets.append({"b": b, "m": m, "v": v, "ema": ema, "groups": groups,
                                  "seg_end": host_to_device(ends, torch.int64, m.device), "tab": None, "tab_key": None,
                                  "par_tab": None, "report": None, "stats": None})
            if skip_report is not None:
                e = self._buckets[-1]
                e["par_tab"] = self._par_tables(e)
                e["report"] = torch.zeros((len(offs), K.GRAD_REPORT_WORDS), device=dev, dtype=torch.int32)
        self._partials = torch.zeros((_NORM_BLOCKS * len(self._buckets),), device=dev, dtype=torch.float32)
        if self.ema_decay is not None:
            self.ema_reset()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if getattr(self.reducer, "micro", 0) != 0:
            raise RuntimeError(f"FlatAdamW.step() inside an accumulation cycle: micro-step {self.reducer.micro} of accum_steps = "
                               f"{self.reducer.accum_steps} comes next - run the remaining backward passes (or reducer.restart_cycle())")
        self._ema_check("step()", need_ema=False)
        self._step += 1
        guarded = self.skip_nonfinite
        if not guarded:
            self._step_t += 1
        b1, b2 = self.param_groups[0]["betas"]
        eps = self.param_groups[0]["eps"]
        bc1, bc2 = 1.0 - b1 ** self._step, 1.0 - b2 ** self._step
        clip = float(self.max_grad_norm) if self.max_grad_norm else 0.0
        if clip > 0 or guarded:
            for i, e in enumerate(self._buckets):
                K.sqnorm_partials(e["b"]["flat"], self._partials[i * _NORM_BLOCKS:(i + 1) * _NORM_BLOCKS])
        if guarded:
            K.adamw_gate(self._guard, self._partials, clip, self.reducer.grad_scale(), b1, b2)
            if self.skip_report_mode is not None:          # gated on the block the gate has just written: returns at once on an applied step
                when = 2 if self.skip_report_mode == "first" else 1
                for e in self._buckets:
                    K.grad_report(e["b"]["flat"], e["b"]["flat_p"], e["par_tab"][0], e["par_tab"][1], self.reducer.grad_scale(),
                                  e["report"], guard_i32=self._guard, when=when)
        for e in self._buckets:
            key = tuple((self.param_groups[g]["lr"], self.param_groups[g]["weight_decay"]) for g in e["groups"])
            if key != e["tab_key"]:            # LR scheduler moved: refresh the (tiny) per-segment table
                dev = e["m"].device
                e["tab"] = (host_to_device([k[0] for k in key], torch.float32, dev),
                            host_to_device([k[1] for k in key], torch.float32, dev))
                e["tab_key"] = key
            if e["ema"] is not None:           # the same launch with the EMA stream; unguarded: _step is the applied count
                K.adamw_flat_ema(e["b"]["flat_p"], e["b"]["flat"], e["m"], e["v"], e["ema"], e["seg_end"], e["tab"][0], e["tab"][1],
                                 b1, b2, eps, self.write_clipped_grads, self.ema_decay, self.ema_warmup,
                                 guard_i32=self._guard if guarded else None, bias_c1=bc1, bias_c2=bc2, partials=self._partials,
                                 max_norm=clip, grad_scale=self.reducer.grad_scale(), t=self._step)
            elif guarded:
                K.adamw_flat_guarded(e["b"]["flat_p"], e["b"]["flat"], e["m"], e["v"], e["seg_end"], e["tab"][0], e["tab"][1],
                                     b1, b2, eps, self._guard, self.write_clipped_grads)
            else:
                K.adamw_flat(e["b"]["flat_p"], e["b"]["flat"], e["m"], e["v"], e["seg_end"], e["tab"][0], e["tab"][1],
                             b1, b2, eps, bc1, bc2, self._partials, clip, self.write_clipped_grads,
                             grad_scale=self.reducer.grad_scale())
        K.weights_changed()            # the update bypassed autograd's version counters: drop cached bf16 weight copies
        return loss

    # ---- weight EMA ------------------------------------------------------------------------------------------------------------
    def _ema_check(self, what, need_ema=True):
        if need_ema and self.ema_decay is None:
            raise RuntimeError(f"FlatAdamW.{what} needs ema_decay (the optimizer was built without a weight EMA)")
        if self._ema_swapped:
            raise RuntimeError(f"FlatAdamW.{what} inside `with optimizer.ema_weights()`: the parameters hold the EMA there")

    def ema_of(self, p):
        """The EMA of parameter p: a view into the flat EMA buffer, shaped like p (it shows the buffer as it is now; inside
        ema_weights() that is the training weights)."""
        if self.ema_decay is None:
            raise RuntimeError("FlatAdamW.ema_of() needs ema_decay (the optimizer was built without a weight EMA)")
        return self._ema_views[p]

    @torch.no_grad()
    def ema_reset(self):
        """EMA := the current parameters, bit for bit.  The constructor does this; call it again after loading model weights into an
        optimizer that already exists - the reference's resume order builds the optimizer first and calls model.load_state_dict()
        afterwards, and the EMA would otherwise still average the initial weights (a checkpoint with a "model_ema" entry is
        restored with load_ema_state_dict() instead).  The warm-up is not reset: it follows the count of applied steps."""
        self._ema_check("ema_reset()")
        for e in self._buckets:
            K.accum_flat(e["ema"], e["b"]["flat_p"])

    @torch.no_grad()
    def ema_state_dict(self, model):
        """A dict with the keys and shapes of model.state_dict(): clones of the EMA for the parameters this optimizer owns, clones of
        the current values for everything else.  model.load_state_dict() of a plain model consumes it."""
        self._ema_check("ema_state_dict()")
        return {k: (self._ema_views[v] if v in self._ema_views else v).detach().clone()
                for k, v in model.state_dict(keep_vars=True).items()}

    @torch.no_grad()
    def load_ema_state_dict(self, model, sd):
        """The inverse of ema_state_dict(): the entries of the parameters this optimizer owns are copied INTO the flat EMA buffer (the
        views stay views); the other entries belong to the model and are ignored here."""
        self._ema_check("load_ema_state_dict()")
        for k, v in model.state_dict(keep_vars=True).items():
            if v in self._ema_views:
                if tuple(sd[k].shape) != tuple(v.shape):
                    raise ValueError(f"load_ema_state_dict: {k} has shape {tuple(sd[k].shape)}, the parameter {tuple(v.shape)}")
                self._ema_views[v].copy_(sd[k])

    def _ema_swap(self):
        for e in self._buckets:
            K.swap_flat(e["b"]["flat_p"], e["ema"])
        K.weights_changed()            # the parameters changed behind autograd's version counters: drop cached 16-bit copies

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the model's parameters ARE the EMA, bit for bit (and the EMA buffer holds the training weights); on exit -
        also through an exception - both buffers have their earlier bits again.  For evaluation:
            with optimizer.ema_weights(): evaluate_det_voc(model, ...)"""
        self._ema_check("ema_weights()")
        self._ema_swap()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._ema_swap()
            self._ema_swapped = False

    # ---- gradient report ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def _par_tables(e):
        """(par_beg, par_len) of spe_grad_report for one bucket: the reducer's (parameter, offset) table on the device."""
        offs, dev = e["b"]["offsets"], e["m"].device
        return (host_to_device([off for _, off in offs], torch.int64, dev), host_to_device([p.numel() for p, _ in offs], torch.int64, dev))

    def _report_rows(self, recs, model):
        """Rows of the report from one host copy of the records per bucket, in reducer order."""
        names = {} if model is None else {p: n for n, p in model.named_parameters()}
        rows = []
        for bi, (e, rec) in enumerate(zip(self._buckets, recs)):
            f, r = rec.view(torch.float32).tolist(), rec.tolist()
            for i, (p, _) in enumerate(e["b"]["offsets"]):
                first = r[i][K.REPORT_FIRST_BAD]
                shape = tuple(p.shape)
                idx = None
                if first >= 0:
                    idx, rest = [], first
                    for d in reversed(shape):
                        idx.append(rest % d); rest //= d
                    idx = tuple(reversed(idx))
                gsq, wsq = f[i][K.REPORT_GRAD_SQ], f[i][K.REPORT_WEIGHT_SQ]
                rows.append({"name": names.get(p, f"bucket{bi}.param{i}"), "shape": shape, "numel": p.numel(),
                             "nan": r[i][K.REPORT_NAN], "inf": r[i][K.REPORT_INF], "first_bad": idx,
                             "grad_sq": gsq, "grad_norm": math.sqrt(gsq) if gsq == gsq else gsq, "grad_absmax": f[i][K.REPORT_GRAD_ABSMAX],
                             "weight_norm": math.sqrt(wsq) if wsq == wsq else wsq, "weight_absmax": f[i][K.REPORT_WEIGHT_ABSMAX]})
        return rows

    def skip_report(self, model=None, top=5):
        """What the guard skipped: None while no report has been written (no skipped step yet), otherwise a dict
            "attempt"         1-based index, among the step() calls, of the skipped step the records describe ("first": == first_skipped())
            "params"          one row per parameter, in reducer order: name, shape, numel, nan, inf, first_bad (index tuple or None),
                              grad_sq, grad_norm, grad_absmax (of grad_scale * g over its finite elements), weight_norm, weight_absmax
            "culprits"        the rows with nan + inf > 0 or a non-finite grad_sq (a finite element whose square overflows fp32)
            "largest"         the `top` rows by grad_absmax
            "total_overflow"  True when no row is a culprit: only the sum over all parameters left fp32, and "largest" is the answer
        Names come from model.named_parameters() when model is given, "bucket{b}.param{i}" otherwise.  One small device-to-host copy
        per bucket: synchronises.  With accumulation the rows describe the accumulated sum; every rank holds the same report."""
        if self.skip_report_mode is None:
            raise RuntimeError("FlatAdamW.skip_report() needs skip_report='first' or 'last' (the optimizer was built without the report)")
        recs = [e["report"].cpu() for e in self._buckets]
        attempt = int(recs[0][0, K.REPORT_ATTEMPT])
        if attempt == 0:
            return None
        rows = self._report_rows(recs, model)
        culprits = [r for r in rows if r["nan"] + r["inf"] > 0 or not math.isfinite(r["grad_sq"])]
        largest = sorted(rows, key=lambda r: -r["grad_absmax"])[:top]
        return {"attempt": attempt, "params": rows, "culprits": culprits, "largest": largest, "total_overflow": not culprits}

    @torch.no_grad()
    def grad_stats(self, model=None, raw=False):
        """The rows of skip_report()["params"] for what the buckets hold NOW - per-parameter gradient norms and maxima (of
        reducer.grad_scale() * g), NaN / inf counts, weight norms - from one unconditional spe_grad_report per bucket.  Needs neither
        skip_nonfinite nor skip_report; its buffers are allocated on the first call.  raw=True: the device tensors (int32
        [parameters, GRAD_REPORT_WORDS] per bucket, overwritten by the next call) and no host read; otherwise one small copy per
        bucket (synchronises).  Call it after the backward (reducer.finish()) and before zero_grad().  After a step() with
        write_clipped_grads=True the buckets hold the CLIPPED gradient with grad_scale folded in (the table multiplies by grad_scale
        all the same: the same figures only while it is 1); before the step, the raw sums.  Inside an
        open accumulation cycle the buckets hold one micro-batch: RuntimeError, as step()."""
        if getattr(self.reducer, "micro", 0) != 0:
            raise RuntimeError(f"FlatAdamW.grad_stats() inside an accumulation cycle: micro-step {self.reducer.micro} of accum_steps = "
                               f"{self.reducer.accum_steps} comes next - the buckets hold one micro-batch, not the step's gradient")
        for e in self._buckets:
            if e["par_tab"] is None:
                e["par_tab"] = self._par_tables(e)
            if e["stats"] is None:
                e["stats"] = torch.zeros((len(e["b"]["offsets"]), K.GRAD_REPORT_WORDS), device=e["m"].device, dtype=torch.int32)
            K.grad_report(e["b"]["flat"], e["b"]["flat_p"], e["par_tab"][0], e["par_tab"][1], self.reducer.grad_scale(), e["stats"])
        if raw:
            return [e["stats"] for e in self._buckets]
        return self._report_rows([e["stats"].cpu() for e in self._buckets], model)

    def _guard_counts(self):
        if self._guard is None:
            raise RuntimeError("FlatAdamW: applied_steps() / skipped_steps() / first_skipped() need skip_nonfinite=True")
        return self._guard[:3].tolist()

    def applied_steps(self):
        """Steps the guard applied so far.  A device-to-host copy: synchronises."""
        return self._guard_counts()[K.GUARD_APPLIED]

    def skipped_steps(self):
        """Steps the guard skipped so far (since construction or the last load_state_dict()).  Synchronises."""
        return self._guard_counts()[K.GUARD_SKIPPED]

    def first_skipped(self):
        """1-based index, among the step() calls, of the first skipped step; 0 if none was skipped.  Synchronises."""
        return self._guard_counts()[K.GUARD_FIRST]

    def state_dict(self):
        """torch's format.  Inside this optimizer every parameter's `step` entry is the one shared, always current tensor; the EXPORTED
        dict gives each parameter its own copy: pickle / torch.save keep aliasing, and torch.optim.AdamW (the reference's optimizer,
        main.py:189-191 and its resume path :224-232) bumps every entry of the list it is handed - one shared tensor would advance by
        the parameter count per step after such a resume.  The inner dicts are copies: torch hands out the live per-parameter dicts
        of optimizer.state, and a clone written into those would cut optimizer.state[p]["step"] off the shared tensor.
        Guarded: `step` is the APPLIED count, read from the device (synchronises)."""
        sd = super().state_dict()
        step = float(self.applied_steps()) if self.skip_nonfinite else float(self._step)
        sd["state"] = {k: ({**st, "step": torch.tensor(step, dtype=torch.float32)} if "step" in st else dict(st))
                       for k, st in sd["state"].items()}
        return sd

    def zero_grad(self, set_to_none=True):
        """The reference loop calls optimizer.zero_grad() before backward (engine.py:161): the gradients live in the
        reducer's buckets, so this re-arms them (zeroes the buckets, detaches .grad, resets the bucket counters).  Inside an
        accumulation cycle it is called before every backward all the same: the running sums live beside the buckets."""
        self.reducer.reset()

    def load_state_dict(self, state_dict):
        """Standard torch format; the moments are copied INTO the flat buffers (the views must stay views).  Guarded: the loaded count
        becomes the applied count of the guard block (skipped and first-skipped start again at 0), so a guarded run resumed from its
        own checkpoint continues bit for bit."""
        views = {p: (self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"]) for g in self.param_groups for p in g["params"]}
        super().load_state_dict(state_dict)
        steps = []
        for g in self.param_groups:
            for p in g["params"]:
                st = self.state[p]
                m, v = views[p]
                if "exp_avg" in st and st["exp_avg"].data_ptr() != m.data_ptr():
                    m.copy_(st["exp_avg"]); v.copy_(st["exp_avg_sq"])
                st["exp_avg"], st["exp_avg_sq"] = m, v
                if "step" in st:
                    steps.append(int(st["step"]))
        if steps:
            self._step = max(steps)
        if self.skip_nonfinite:
            self._guard.copy_(host_to_device([self._step] + [0] * (K.ADAMW_GUARD_WORDS - 1), torch.int32, self._guard.device))
        self._step_t.fill_(float(self._step))
        for g in self.param_groups:                 # re-share the step tensor (load_state_dict gave every parameter its own copy)
            for p in g["params"]:
                self.state[p]["step"] = self._step_t
