"""FlatAdamW(..., ema_decay=d): the weight EMA kept inside the update launch (spe_adamw_flat_ema), its exchange with the parameters
(spe_swap_flat, optimizer.ema_weights()) and the checkpoint interface, against the numpy restatement of adamw_ema_ref.py - bit for bit.

C-ABI tests run on buffers with 64 poisoned elements on EACH side of the n the entry may touch; the optimizer-level tests use the
six-tensor, two-bucket, two-group setup of test_adamw_guard_gpu.py."""
import numpy as np
import pytest
import torch

import adamw_ema_ref as R
from adamw_ema_cases import BETAS, EPS, SHAPES, SIZES, TRIPLES

pytestmark = pytest.mark.gpu

BAND = 64
SENTINEL = 12345.0
MAX_NORM, GSCALE = 0.1, 0.5


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _np_same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- the entries through the C ABI ---------------------------------------------------------------------------------------------------
class _Banded:
    """n floats between two poisoned bands of 64 (256 B: the data stays 16-B aligned)."""

    def __init__(self, dev, data):
        self.n = data.numel()
        self.buf = torch.full((self.n + 2 * BAND,), SENTINEL, device=dev)
        self.buf.view(torch.int32)[BAND:BAND + self.n] = data.contiguous().view(torch.int32).to(dev)      # as integers: every bit pattern survives

    @property
    def data(self):
        return self.buf[BAND:BAND + self.n]

    def ptr(self):
        return self.buf.data_ptr() + 4 * BAND

    def bands_intact(self):
        return bool((self.buf[:BAND] == SENTINEL).all()) and bool((self.buf[BAND + self.n:] == SENTINEL).all())

    def clone(self):
        c = _Banded.__new__(_Banded)
        c.n, c.buf = self.n, self.buf.clone()
        return c


class _Abi:
    """Inputs of one update of n elements in three segments; `fresh()` hands out banded copies of them."""

    def __init__(self, dev, n, seed):
        from spe_amd import kernels as K, lib
        self.lib, self.st, self.n, self.K, self.dev = lib, K._st, n, K, dev
        gen = torch.Generator().manual_seed(seed)
        self.src = {}
        for name in "pgmve":
            x = torch.randn(n, generator=gen)
            self.src[name] = _Banded(dev, x.abs() if name == "v" else x)
        self.partials = torch.zeros((256,), device=dev)
        lib.call("spe_sqnorm_partials", self.src["g"].ptr(), n, self.partials.data_ptr(), 256, self.st())
        self.seg_end = torch.tensor([n // 3, 2 * n // 3, n], dtype=torch.int64, device=dev)        # (empty segments for n < 3)
        self.lr = torch.tensor([1e-2, 3e-3, 1e-3], device=dev)
        self.wd = torch.tensor([1e-2, 0.0, 1e-4], device=dev)
        self.bc = (1 - BETAS[0] ** 3, 1 - BETAS[1] ** 3)

    def fresh(self):
        return {k: b.clone() for k, b in self.src.items()}

    def guard_for(self, t, apply=True):
        """A guard block as spe_adamw_gate leaves it at the t-th applied step (the gate itself runs: applied = t - 1 before it)."""
        guard = torch.full((self.K.ADAMW_GUARD_WORDS + BAND,), 0x5A5A5A5A, dtype=torch.int32, device=self.dev)
        guard[:9] = 0
        guard[self.K.GUARD_APPLIED] = t - 1
        self.lib.call("spe_adamw_gate", guard.data_ptr(), self.partials.data_ptr(), 256, MAX_NORM, GSCALE, BETAS[0], BETAS[1], self.st())
        if not apply:
            guard[self.K.GUARD_APPLY] = 0
        return guard

    def tail(self):
        return (self.seg_end.data_ptr(), self.lr.data_ptr(), self.wd.data_ptr(), 3, BETAS[0], BETAS[1], EPS)

    def plain(self, b, guard):
        p = [b[k].ptr() for k in "pgmv"]
        if guard is None:
            self.lib.call("spe_adamw_flat", *p, self.n, *self.tail(), *self.bc, self.partials.data_ptr(), 256, MAX_NORM, 1, GSCALE, self.st())
        else:
            self.lib.call("spe_adamw_flat_guarded", *p, self.n, *self.tail(), guard.data_ptr(), 1, self.st())

    def ema(self, b, guard, decay, warmup, t, e_ptr="own", n=None):
        p = [b[k].ptr() for k in "pgmv"]
        e = b["e"].ptr() if e_ptr == "own" else e_ptr
        self.lib.call("spe_adamw_flat_ema", *p, e, self.n if n is None else n, *self.tail(), *self.bc, self.partials.data_ptr(), 256, MAX_NORM,
                      1, GSCALE, None if guard is None else guard.data_ptr(), decay, int(warmup), t, self.st())


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_c_abi_ema_entry_matches_the_restatement_and_leaves_the_update_alone(dev, n, guarded):
    """For every (decay, warmup, t): p, m, v and g get the bits of the entry without the EMA on copies of the same inputs; e is the
    restatement applied to (e, that p'); exactly n elements of e are written (both bands intact)."""
    a = _Abi(dev, n, n)
    e0 = a.src["e"].data.cpu().numpy()
    ref_by_t = {}
    for decay, warmup, t in TRIPLES:
        key = t if guarded else 0                 # unguarded: the update itself does not depend on t (fixed bias corrections)
        if key not in ref_by_t:
            ref = a.fresh()
            a.plain(ref, a.guard_for(t) if guarded else None)
            ref_by_t[key] = ref
        ref = ref_by_t[key]
        b = a.fresh()
        guard = a.guard_for(t) if guarded else None
        a.ema(b, guard, decay, warmup, 0 if guarded else t)           # guarded: the t argument is ignored, the block's count holds
        torch.cuda.synchronize()
        for k in "pgmv":
            assert _same_bits(b[k].buf, ref[k].buf), (k, decay, warmup, t)
        assert all(x.bands_intact() for x in b.values())
        want = R.ema_step32(e0, ref["p"].data.cpu().numpy(), R.ema_weight(decay, warmup, t))
        assert _np_same_bits(b["e"].data.cpu().numpy(), want), (decay, warmup, t)
        assert not _same_bits(b["e"].data, a.src["e"].data)
        if guarded:
            assert bool((guard[9:] == 0x5A5A5A5A).all()) and int(guard[a.K.GUARD_APPLIED]) == t


@pytest.mark.parametrize("n", SIZES)
def test_c_abi_guarded_skip_keeps_every_bit_of_e(dev, n):
    a = _Abi(dev, n, n + 1)
    b = a.fresh()
    guard = a.guard_for(5, apply=False)
    a.ema(b, guard, 0.9, True, 5)
    torch.cuda.synchronize()
    assert all(_same_bits(b[k].buf, a.src[k].buf) for k in "pgmve")


def test_c_abi_refusals(dev):
    from spe_amd import lib
    a = _Abi(dev, 1024, 3)
    b = a.fresh()
    guard = a.guard_for(1)
    for g in (None, guard):
        for e_ptr in (None, b["e"].ptr() + 4):
            with pytest.raises(lib.SpeLibraryError, match="-2"):
                a.ema(b, g, 0.9, True, 1, e_ptr=e_ptr)
        for decay in (1.0, -0.1, float("nan")):
            with pytest.raises(lib.SpeLibraryError, match="-2"):
                a.ema(b, g, decay, True, 1)
    with pytest.raises(lib.SpeLibraryError, match="-2"):              # a misaligned guard block is no "unguarded"
        lib.call("spe_adamw_flat_ema", *[b[k].ptr() for k in "pgmv"], b["e"].ptr(), 1024, *a.tail(), *a.bc, a.partials.data_ptr(), 256,
                 MAX_NORM, 1, GSCALE, guard.data_ptr() + 4, 0.9, 1, 1, a.st())
    a.ema(b, None, 0.9, True, 1, n=0)                                 # n <= 0: status 0, nothing launched
    a.ema(b, guard, 0.9, True, 1, n=-5)
    st = a.st()
    for x, y in ((b["p"].ptr(), b["p"].ptr()), (b["p"].ptr() + 4, b["e"].ptr()), (b["p"].ptr(), b["e"].ptr() + 4), (None, b["e"].ptr()),
                 (b["p"].ptr(), None)):
        with pytest.raises(lib.SpeLibraryError, match="-2"):
            lib.call("spe_swap_flat", x, y, 1024, st)
    lib.call("spe_swap_flat", b["p"].ptr(), b["p"].ptr(), 0, st)      # n <= 0: nothing to exchange, status 0
    torch.cuda.synchronize()
    assert all(_same_bits(b[k].buf, a.src[k].buf) for k in "pgmve")


@pytest.mark.parametrize("n", SIZES)
def test_swap_flat_exchanges_bits(dev, n):
    """Random bit patterns - NaN payloads, infinities, denormals and -0.0 among them - change places; twice gives the identity."""
    from spe_amd import kernels as K, lib
    gen = torch.Generator().manual_seed(n)
    raw = [torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=gen, dtype=torch.int64).to(torch.int32) for _ in range(2)]
    special = torch.tensor([0x7FC00001, -0x7FFFFF, -2 ** 31, 0x7F800000, 0x7FA5A5A5, 1], dtype=torch.int64).to(torch.int32)   # quiet NaN + payload, -NaN, -0.0, inf, signalling NaN, denormal
    for i, r in enumerate(raw):
        k = min(n, special.numel())
        r[:k] = special[:k]
        r[n - 1] = special[(2 + i) % special.numel()]                 # the last element (inside the scalar tail where n % 4 != 0)
    x, y = (_Banded(dev, r.view(torch.float32)) for r in raw)
    assert torch.equal(_bits(x.data).cpu(), raw[0]) and torch.equal(_bits(y.data).cpu(), raw[1])      # the upload kept the bits
    lib.call("spe_swap_flat", x.ptr(), y.ptr(), n, K._st())
    torch.cuda.synchronize()
    assert torch.equal(_bits(x.data).cpu(), raw[1]) and torch.equal(_bits(y.data).cpu(), raw[0])
    assert x.bands_intact() and y.bands_intact()
    K.swap_flat(x.data, y.data)
    torch.cuda.synchronize()
    assert torch.equal(_bits(x.data).cpu(), raw[0]) and torch.equal(_bits(y.data).cpu(), raw[1])
    assert x.bands_intact() and y.bands_intact()


# ---- the optimizer -------------------------------------------------------------------------------------------------------------------
def _params(dev):
    return [torch.nn.Parameter(torch.randn(*s, generator=torch.Generator().manual_seed(i)).to(dev)) for i, s in enumerate(SHAPES)]


def _groups(ps):
    return [{"params": ps[:3], "lr": 1e-2, "weight_decay": 1e-2}, {"params": ps[3:], "lr": 3e-3, "weight_decay": 0.0}]


class _Opt:
    """Six parameters in flat buckets with a FlatAdamW on them."""

    def __init__(self, dev, guarded=True, accum_steps=1, **kw):
        from spe_amd.dp import GradAllReducer
        from spe_amd.optim import FlatAdamW
        self.ps = _params(dev)
        self.red = GradAllReducer(self.ps, bucket_bytes=4096, flatten_params=True, accum_steps=accum_steps)
        if guarded:
            kw["skip_nonfinite"] = True
        self.opt = FlatAdamW(_groups(self.ps), self.red, betas=BETAS, eps=EPS, max_grad_norm=0.1, **kw)
        assert len(self.red.buckets) >= 2

    def feed(self, grads):
        self.red.reset()
        for y, gr in zip(self.ps, grads):
            y.grad = self.red._views[y]
            y.grad.copy_(gr)
        self.red.finish()

    def flats(self):
        """Clones of the flat parameter and EMA buffers of every bucket."""
        return [t.clone() for e in self.opt._buckets for t in (e["b"]["flat_p"], e["ema"])]

    def emas(self):
        return [self.opt.ema_of(p).clone() for p in self.ps]

    def close(self):
        self.red.remove()


def _grads(dev, seed, scale=0.01):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(dev) * scale for s in SHAPES]


@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("guarded", [True, False])
def test_twenty_steps_follow_the_restatement(dev, guarded, warmup):
    """ema_of(p) is the restatement applied to the parameter sequence the optimizer itself produced; padding between the parameters
    stays zero."""
    o = _Opt(dev, guarded, ema_decay=0.9, ema_warmup=warmup)
    assert all(_same_bits(o.opt.ema_of(p), p) for p in o.ps)          # construction: a bit copy
    e0 = [p.detach().cpu().numpy().copy() for p in o.ps]
    seq = []
    for it in range(20):
        o.feed(_grads(dev, 100 + it, 10.0 if it % 7 == 1 else 0.01))
        o.opt.step()
        seq.append([p.detach().cpu().numpy().copy() for p in o.ps])
    for i, p in enumerate(o.ps):
        want = R.ema_run32(e0[i], [s[i] for s in seq], 0.9, warmup)
        got = o.opt.ema_of(p)
        assert got.shape == p.shape and got.data_ptr() != p.data_ptr()
        assert _np_same_bits(got.cpu().numpy(), want), i
        assert not _same_bits(got, p)
    for e in o.opt._buckets:                                          # zeros stay zeros
        pad = torch.ones_like(e["ema"], dtype=torch.bool)
        for p, off in e["b"]["offsets"]:
            pad[off:off + p.numel()] = False
        assert bool((e["ema"][pad] == 0).all()) and bool((e["b"]["flat_p"][pad] == 0).all())
    o.close()


def test_poisoned_step_leaves_the_ema_of_the_clean_run(dev):
    g1, g2 = _grads(dev, 11), _grads(dev, 12, 10.0)
    bad = [g.clone() for g in g2]
    bad[4].view(-1)[7] = float("inf")
    a, b = _Opt(dev, ema_decay=0.9), _Opt(dev, ema_decay=0.9)
    a.feed(g1); a.opt.step()
    before = a.flats()
    a.feed(bad); a.opt.step()
    assert all(_same_bits(x, y) for x, y in zip(a.flats(), before))   # the skipped step wrote neither parameters nor EMA
    a.feed(g2); a.opt.step()
    for grads in (g1, g2):
        b.feed(grads); b.opt.step()
    assert (a.opt.applied_steps(), a.opt.skipped_steps()) == (2, 1)
    assert all(_same_bits(x, y) for x, y in zip(a.flats(), b.flats()))
    assert any(not _same_bits(x, y) for x, y in zip(a.flats(), before))
    a.close(); b.close()


@pytest.mark.parametrize("guarded", [True, False])
def test_accumulation_moves_the_ema_once_per_cycle(dev, guarded):
    """accum_steps = 2, the training loop's order (finish, then step() where the cycle is complete): the EMA changes at every second
    finish() only, and then to the restatement of the parameters that step produced."""
    o = _Opt(dev, guarded, accum_steps=2, ema_decay=0.5, ema_warmup=False)
    last = o.emas()
    for it in range(6):
        o.feed(_grads(dev, 200 + it))
        if o.red.micro == 0:
            o.opt.step()
        now = o.emas()
        changed = [not _same_bits(x, y) for x, y in zip(now, last)]
        assert all(changed) if it % 2 == 1 else not any(changed), (it, changed)
        if it % 2 == 1:
            for e_old, e_new, p in zip(last, now, o.ps):
                want = R.ema_step32(e_old.cpu().numpy(), p.detach().cpu().numpy(), R.ema_weight(0.5, False, it // 2 + 1))
                assert _np_same_bits(e_new.cpu().numpy(), want)
        last = now
    o.close()


def test_without_ema_decay_nothing_is_allocated(dev):
    from spe_amd import lib
    o, plain = _Opt(dev, False, ema_decay=None), _Opt(dev, False)
    assert all(e["ema"] is None for e in o.opt._buckets)
    with pytest.raises(RuntimeError):
        o.opt.ema_of(o.ps[0])
    for f in (o.opt.ema_reset, lambda: o.opt.ema_state_dict(torch.nn.ParameterList(o.ps)), lambda: o.opt.ema_weights().__enter__()):
        with pytest.raises(RuntimeError):
            f()
    lib.count_launches(True)
    for x in (o, plain):
        x.feed(_grads(dev, 5)); x.opt.step()
    counts = lib.count_launches(False)
    assert "spe_adamw_flat_ema" not in counts and counts["spe_adamw_flat"] == 2 * len(o.opt._buckets)
    sa, sb = o.opt.state_dict(), plain.opt.state_dict()
    assert sa.keys() == sb.keys() and sa["state"].keys() == sb["state"].keys()
    assert all(sa["state"][k].keys() == sb["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"} for k in sa["state"])
    assert [g.keys() for g in sa["param_groups"]] == [g.keys() for g in sb["param_groups"]]
    assert all(_same_bits(x, y) for x, y in zip(o.ps, plain.ps))
    from spe_amd.optim import FlatAdamW
    for bad in (1.0, -0.1, float("nan"), 2):
        with pytest.raises(ValueError):
            FlatAdamW(_groups(o.ps), o.red, ema_decay=bad)            # (refused before the reducer is touched)
    o.close(); plain.close()


@pytest.mark.parametrize("guarded", [True, False])
def test_ema_step_issues_the_launches_of_the_plain_step_and_reads_nothing_back(dev, guarded):
    from spe_amd import lib
    o, plain = _Opt(dev, guarded, ema_decay=0.9998), _Opt(dev, guarded)
    for x in (o, plain):
        x.feed(_grads(dev, 40)); x.opt.step()                         # first call: the segment tables
    counts = []
    for x in (o, plain):
        x.feed(_grads(dev, 41))
        torch.cuda.synchronize()
        lib.count_launches(True)
        torch.cuda.set_sync_debug_mode("error")
        try:
            x.opt.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        counts.append(lib.count_launches(False))
    nb = len(o.opt._buckets)
    upd = "spe_adamw_flat_guarded" if guarded else "spe_adamw_flat"
    assert counts[0].get("spe_adamw_flat_ema") == nb and upd not in counts[0] and counts[1].get(upd) == nb
    assert sum(counts[0].values()) == sum(counts[1].values())
    sd = o.opt.state_dict()                                           # the EMA is no optimizer state
    assert all(st.keys() == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values())
    o.close(); plain.close()


def test_ema_weights_swaps_in_and_out(dev):
    from spe_amd import ops
    o = _Opt(dev, ema_decay=0.9)
    for it in range(3):
        o.feed(_grads(dev, 300 + it, 1.0)); o.opt.step()
    W, b = o.ps[0], o.ps[1]                                            # a Linear node 32 -> 64
    x = torch.randn(256, 32, generator=torch.Generator().manual_seed(9)).to(dev)
    with torch.no_grad():
        y_train = ops.linear(x, W, b).clone()                         # (caches the 16-bit copy of W)
        We, be = o.opt.ema_of(W).clone(), o.opt.ema_of(b).clone()
        y_hand = ops.linear(x, We, be).clone()                        # the EMA values copied in by hand
    assert not torch.equal(y_train, y_hand)
    before = o.flats()
    with o.opt.ema_weights() as inside:
        assert inside is o.opt
        now = o.flats()
        assert all(_same_bits(now[2 * i], before[2 * i + 1]) and _same_bits(now[2 * i + 1], before[2 * i]) for i in range(len(before) // 2))
        assert _same_bits(W, We) and _same_bits(b, be)
        with torch.no_grad():
            assert torch.equal(ops.linear(x, W, b), y_hand)           # no stale 16-bit copy
        o.feed(_grads(dev, 310))
        for f in (o.opt.step, o.opt.ema_reset, lambda: o.opt.ema_state_dict(torch.nn.ParameterList(o.ps)),
                  lambda: o.opt.load_ema_state_dict(torch.nn.ParameterList(o.ps), {}), lambda: o.opt.ema_weights().__enter__()):
            with pytest.raises(RuntimeError):
                f()
        assert all(_same_bits(x_, y_) for x_, y_ in zip(o.flats(), now))
    assert all(_same_bits(x_, y_) for x_, y_ in zip(o.flats(), before))
    with torch.no_grad():
        assert torch.equal(ops.linear(x, W, b), y_train)
    with pytest.raises(KeyError):                                     # an exception inside still restores
        with o.opt.ema_weights():
            raise KeyError("evaluation failed")
    assert all(_same_bits(x_, y_) for x_, y_ in zip(o.flats(), before))
    with torch.no_grad():
        assert torch.equal(ops.linear(x, W, b), y_train)
    o.opt.step()                                                      # and the optimizer steps again
    assert o.opt.applied_steps() == 4
    o.close()


class _Model(torch.nn.Module):
    """The six parameters plus a buffer and a parameter the optimizer does not own."""

    def __init__(self, ps, dev):
        super().__init__()
        self.w = torch.nn.ParameterList(ps)
        self.frozen = torch.nn.Parameter(torch.full((5,), 2.5, device=dev), requires_grad=False)
        self.register_buffer("count", torch.arange(3, device=dev))


@pytest.mark.parametrize("guarded", [True, False])
def test_checkpoint_resumes_bitwise(dev, guarded):
    """ema_state_dict(model) -> fresh parameters, reducer and optimizer -> the loads -> five more steps: parameters and EMA are those of
    the uninterrupted run.  A plain model loads the exported dict."""
    a = _Opt(dev, guarded, ema_decay=0.9)
    ma = _Model(a.ps, dev)
    for it in range(4):
        a.feed(_grads(dev, 400 + it)); a.opt.step()
    ckpt = {"model": {k: v.detach().clone() for k, v in ma.state_dict().items()}, "optimizer": a.opt.state_dict(),
            "model_ema": a.opt.ema_state_dict(ma)}
    assert ckpt["model_ema"].keys() == ma.state_dict().keys()
    assert all(ckpt["model_ema"][k].shape == v.shape and ckpt["model_ema"][k].data_ptr() != v.data_ptr() for k, v in ma.state_dict().items())
    assert all(_same_bits(ckpt["model_ema"][f"w.{i}"], a.opt.ema_of(p)) for i, p in enumerate(a.ps))
    assert torch.equal(ckpt["model_ema"]["frozen"], ma.frozen) and torch.equal(ckpt["model_ema"]["count"], ma.count)
    assert not any(k.startswith("ema") for k in ckpt["optimizer"]) and len(ckpt["optimizer"]["state"]) == len(SHAPES)
    plain = _Model([torch.nn.Parameter(torch.zeros(s, device=dev)) for s in SHAPES], dev)
    plain.load_state_dict(ckpt["model_ema"])
    assert all(_same_bits(x, a.opt.ema_of(p)) for x, p in zip(plain.w, a.ps))

    b = _Opt(dev, guarded, ema_decay=0.9)
    mb = _Model(b.ps, dev)
    views = [b.opt.ema_of(p) for p in b.ps]
    mb.load_state_dict(ckpt["model"])
    b.opt.load_state_dict(ckpt["optimizer"])
    b.opt.load_ema_state_dict(mb, ckpt["model_ema"])
    assert all(b.opt.ema_of(p).data_ptr() == v.data_ptr() for p, v in zip(b.ps, views))            # the views stay views
    for it in range(5):
        for o in (a, b):
            o.feed(_grads(dev, 500 + it, 10.0 if it == 2 else 0.01)); o.opt.step()
    assert all(_same_bits(x, y) for x, y in zip(a.flats(), b.flats()))
    assert all(bool(torch.isfinite(x).all()) for x in a.flats())
    a.close(); b.close()


def test_ema_reset_after_loading_model_weights(dev):
    o = _Opt(dev, ema_decay=0.9)
    m = _Model(o.ps, dev)
    o.feed(_grads(dev, 600)); o.opt.step()
    loaded = {k: torch.randn(v.shape, generator=torch.Generator().manual_seed(7 + i)).to(dev) if v.dtype == torch.float32 else v.clone()
              for i, (k, v) in enumerate(m.state_dict().items())}
    m.load_state_dict(loaded)
    assert not any(_same_bits(o.opt.ema_of(p), p) for p in o.ps)      # the EMA still averages the earlier weights
    o.opt.ema_reset()
    assert all(_same_bits(o.opt.ema_of(p), loaded[f"w.{i}"]) and _same_bits(p, loaded[f"w.{i}"]) for i, p in enumerate(o.ps))
    o.close()
