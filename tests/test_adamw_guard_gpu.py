"""FlatAdamW(..., skip_nonfinite=True): the update is decided on the device from the gradient norm (spe_adamw_gate) and a step whose
reduced gradient is not finite writes nothing (spe_adamw_flat_guarded).  Shapes, groups and scales are those of
test_grad_accum_gpu.py::test_flat_adamw_accumulated_matches_torch: six tensors, bucket_bytes=4096, hence two buckets and two groups.

The buckets are padded to multiples of 64 floats, so at the optimizer level no launch has an n % 4 tail; the "tail" position of the
poisoning test is the last element of a tensor whose size is no multiple of 4, and the kernels' own n % 4 tails are poisoned in the
C-ABI test at the end, on sizes that have one."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

GRID_CAP = 2048                     # workgroups of spe_adamw_flat(_guarded) at most; each sweeps 1024 elements per pass
GUARD = 64
SENTINEL = 12345.0
SIZES = [1, 3, 4, 5, 255, 256, 1023, 1024, 1025, GRID_CAP * 1024 + 7]
SHAPES = [(64, 32), (64,), (7, 5, 3), (1,), (300, 17), (33,)]
BETAS, EPS = (0.9, 0.999), 1e-8
BAD = {"inf": float("inf"), "-inf": float("-inf"), "nan": float("nan"), "3e19": 3e19}       # 3e19^2 > FLT_MAX: the squared norm overflows


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _params(dev):
    return [torch.nn.Parameter(torch.randn(*s, generator=torch.Generator().manual_seed(i)).to(dev)) for i, s in enumerate(SHAPES)]


def _groups(ps):
    return [{"params": ps[:3], "lr": 1e-2, "weight_decay": 1e-2}, {"params": ps[3:], "lr": 3e-3, "weight_decay": 0.0}]


class _Opt:
    """Six parameters in flat buckets with a FlatAdamW on them."""

    def __init__(self, dev, guarded=True, max_grad_norm=0.1, accum_steps=1):
        from spe_amd.dp import GradAllReducer
        from spe_amd.optim import FlatAdamW
        self.dev = dev
        self.ps = _params(dev)
        self.red = GradAllReducer(self.ps, bucket_bytes=4096, flatten_params=True, accum_steps=accum_steps)
        kw = {"skip_nonfinite": True} if guarded else {}
        self.opt = FlatAdamW(_groups(self.ps), self.red, betas=BETAS, eps=EPS, max_grad_norm=max_grad_norm, **kw)
        assert len(self.red.buckets) >= 2

    def feed(self, grads):
        """One reset / "backward" / finish round with the given gradients."""
        self.red.reset()
        for y, gr in zip(self.ps, grads):
            y.grad = self.red._views[y]
            y.grad.copy_(gr)
        self.red.finish()

    def snapshot(self):
        """Clones of every flat buffer the update could write: parameters, both moments, gradient buckets."""
        return [t.clone() for e in self.opt._buckets for t in (e["b"]["flat_p"], e["m"], e["v"], e["b"]["flat"])]

    def state(self):
        """Parameters and moments only."""
        return [t.clone() for e in self.opt._buckets for t in (e["b"]["flat_p"], e["m"], e["v"])]

    def close(self):
        self.red.remove()


def _grads(dev, seed, scale=0.01):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(dev) * scale for s in SHAPES]


def _poisoned(grads, value, tensor=4, index=7):
    out = [g.clone() for g in grads]
    out[tensor].view(-1)[index] = value
    return out


@pytest.mark.parametrize("max_grad_norm", [0.1, None])
def test_clean_guarded_run_matches_torch(dev, max_grad_norm):
    """Three steps, the middle one clipped when a clip is set, against clip_grad_norm_ + torch.optim.AdamW and against the unguarded
    FlatAdamW (bounds of test_flat_adamw_accumulated_matches_torch; guarded against unguarded is not bitwise: the bias corrections are
    rounded on different sides)."""
    pa = _params(dev)
    ref = torch.optim.AdamW(_groups(pa), betas=BETAS, eps=EPS)
    g, u = _Opt(dev, True, max_grad_norm), _Opt(dev, False, max_grad_norm)
    for it in range(3):
        grads = _grads(dev, 100 + it, 10.0 if it == 1 else 0.01)
        for x, gr in zip(pa, grads):
            x.grad = gr.clone()
        if max_grad_norm:
            torch.nn.utils.clip_grad_norm_(pa, max_grad_norm)
        ref.step()
        for o in (g, u):
            o.feed(grads)
            o.opt.step()
        for x, y, z in zip(pa, g.ps, u.ps):
            assert rel(y, x) < 2e-6, (it, rel(y, x))
            assert rel(y.grad, x.grad) < 2e-6
            assert rel(y, z) < 2e-6 and rel(y.grad, z.grad) < 2e-6
    for x, y, z in zip(pa, g.ps, u.ps):
        for other in (ref.state[x], u.opt.state[z]):
            assert rel(g.opt.state[y]["exp_avg"], other["exp_avg"]) < 2e-6
            assert rel(g.opt.state[y]["exp_avg_sq"], other["exp_avg_sq"]) < 5e-5
    assert (g.opt.applied_steps(), g.opt.skipped_steps(), g.opt.first_skipped()) == (3, 0, 0)
    assert g.opt._step == 3 and float(g.opt.state[g.ps[0]]["step"]) == 3.0
    with pytest.raises(RuntimeError):
        u.opt.applied_steps()
    g.close(); u.close()


@pytest.mark.parametrize("where", ["first", "last", "tail"])
@pytest.mark.parametrize("bucket", [0, -1])
@pytest.mark.parametrize("bad", list(BAD))
def test_poisoned_step_leaves_everything_bitwise(dev, bad, bucket, where):
    o = _Opt(dev)
    o.feed(_grads(dev, 1))
    o.opt.step()                                          # moments and counters are not at their initial values
    o.feed(_grads(dev, 2, 10.0))
    flat = o.red.buckets[bucket]["flat"]
    if where == "tail":                                   # last element of a tensor of 33 (bucket 0) / 105 (last bucket) elements
        p, off = next((p, off) for p, off in o.red.buckets[bucket]["offsets"] if p.numel() % 4 != 0 and p.numel() > 1)
        idx = off + p.numel() - 1
    else:
        idx = 0 if where == "first" else flat.numel() - 1
    flat[idx] = BAD[bad]
    before = o.snapshot()
    o.opt.step()
    after = o.snapshot()
    assert all(_same_bits(a, b) for a, b in zip(after, before))
    assert (o.opt.applied_steps(), o.opt.skipped_steps(), o.opt.first_skipped()) == (1, 1, 2)
    assert o.opt._step == 2                               # attempts
    o.close()


def test_run_with_a_poisoned_step_equals_the_run_without(dev):
    """g1, BAD, g2, g3 against g1, g2, g3: equal bits at the end - the skipped attempt does not shift the bias corrections."""
    g1, g2, g3 = _grads(dev, 11), _grads(dev, 12, 10.0), _grads(dev, 13)
    a, b = _Opt(dev), _Opt(dev)
    for grads in (g1, _poisoned(g2, float("inf")), g2, g3):
        a.feed(grads)
        a.opt.step()
    for grads in (g1, g2, g3):
        b.feed(grads)
        b.opt.step()
    assert all(torch.equal(x, y) for x, y in zip(a.state(), b.state()))
    assert all(bool(torch.isfinite(x).all()) for x in a.state())
    assert a.opt.applied_steps() == 3 and b.opt.applied_steps() == 3
    assert (a.opt.skipped_steps(), a.opt.first_skipped()) == (1, 2) and (b.opt.skipped_steps(), b.opt.first_skipped()) == (0, 0)
    a.close(); b.close()


def test_accumulation_cycle_with_a_poisoned_micro_step_is_skipped(dev):
    KS = 3
    c1 = [_grads(dev, 20 + m) for m in range(KS)]
    c1[1] = _poisoned(c1[1], float("inf"), tensor=0, index=5)
    c2 = [_grads(dev, 30 + m, 10.0) for m in range(KS)]
    a, fresh = _Opt(dev, accum_steps=KS), _Opt(dev, accum_steps=KS)
    start = a.state()
    for grads in c1:
        a.feed(grads)
    before = a.snapshot()
    a.opt.step()
    assert all(_same_bits(x, y) for x, y in zip(a.snapshot(), before))
    assert all(torch.equal(x, y) for x, y in zip(a.state(), start))
    assert (a.opt.applied_steps(), a.opt.skipped_steps()) == (0, 1)
    for o in (a, fresh):
        for grads in c2:
            o.feed(grads)
        o.opt.step()
    assert all(torch.equal(x, y) for x, y in zip(a.state(), fresh.state()))
    assert any(not torch.equal(x, y) for x, y in zip(a.state(), start))
    assert (a.opt.applied_steps(), a.opt.skipped_steps(), a.opt.first_skipped()) == (1, 1, 1)
    a.close(); fresh.close()


def test_guarded_step_reads_nothing_back(dev):
    """An applied and a skipped step() under torch's sync debug mode: any .item() / .cpu() would raise."""
    o = _Opt(dev)
    o.feed(_grads(dev, 40))
    o.opt.step()                                          # first call: library load, the segment tables
    torch.cuda.synchronize()
    for grads in (_grads(dev, 41), _poisoned(_grads(dev, 42), float("nan"))):
        o.feed(grads)
        torch.cuda.set_sync_debug_mode("error")
        try:
            o.opt.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert (o.opt.applied_steps(), o.opt.skipped_steps(), o.opt.first_skipped()) == (2, 1, 3)
    o.close()


def test_checkpoint_after_a_skip_resumes_bitwise(dev):
    g1, g2, g3 = _grads(dev, 51), _grads(dev, 52, 10.0), _grads(dev, 53)
    a = _Opt(dev)
    for grads in (g1, _poisoned(g1, float("-inf")), g2):
        a.feed(grads)
        a.opt.step()
    sd = a.opt.state_dict()
    assert len(sd["state"]) == len(SHAPES) and all(float(st["step"]) == 2.0 for st in sd["state"].values())
    steps = [st["step"] for st in sd["state"].values()]
    assert len({t.data_ptr() for t in steps}) == len(steps)             # every parameter its own tensor
    b = _Opt(dev)
    with torch.no_grad():
        for x, y in zip(a.ps, b.ps):
            y.copy_(x)
    b.opt.load_state_dict(sd)
    assert (b.opt.applied_steps(), b.opt.skipped_steps(), b.opt.first_skipped()) == (2, 0, 0)
    # into the reference's optimizer: it loads and steps
    pt = [torch.nn.Parameter(x.detach().clone()) for x in a.ps]
    ref = torch.optim.AdamW(_groups(pt), betas=BETAS, eps=EPS)
    ref.load_state_dict(copy.deepcopy(sd))                # (torch adopts tensors of the right dtype and device: sd's moments are a's views)
    for x, gr in zip(pt, g3):
        x.grad = gr.clone()
    torch.nn.utils.clip_grad_norm_(pt, 0.1)
    ref.step()
    assert all(float(ref.state[x]["step"]) == 3.0 and bool(torch.isfinite(x).all()) for x in pt)
    for o in (a, b):
        o.feed(g3)
        o.opt.step()
    assert all(torch.equal(x, y) for x, y in zip(a.state(), b.state()))
    assert a.opt.applied_steps() == 3 and b.opt.applied_steps() == 3
    for x, y in zip(pt, a.ps):
        assert rel(x, y) < 2e-6                          # torch resumed from the same checkpoint lands on the same parameters
    a.close(); b.close()


@pytest.mark.parametrize("guarded", [True, False])
def test_live_step_entry_stays_current_after_state_dict(dev, guarded):
    """state_dict() exports copies of the per-parameter dicts: optimizer.state[p]["step"] keeps tracking afterwards."""
    o = _Opt(dev, guarded)
    o.feed(_grads(dev, 61))
    o.opt.step()
    sd = o.opt.state_dict()
    o.feed(_grads(dev, 62))
    o.opt.step()
    assert all(float(o.opt.state[p]["step"]) == 2.0 for p in o.ps)
    assert all(float(st["step"]) == 1.0 for st in sd["state"].values())             # the export is a snapshot
    live = [o.opt.state[p] for g in o.opt.param_groups for p in g["params"]]
    assert all(sd["state"][i] is not st for i, st in enumerate(live))
    o.close()


# ---- the two entries through the C ABI, on buffers with sentinel bands ----------------------------------------------------------
class _Abi:
    def __init__(self, dev, n, seed):
        from spe_amd import kernels as K, lib
        self.lib, self.st, self.n, self.K = lib, K._st, n, K
        gen = torch.Generator().manual_seed(seed)
        self.bufs = {}
        for name in "pgmv":
            src = torch.randn(n, generator=gen).abs() if name == "v" else torch.randn(n, generator=gen)
            buf = torch.full((n + GUARD,), SENTINEL, device=dev)
            buf[:n] = src.to(dev)
            self.bufs[name] = buf
        self.partials = torch.full((256 + GUARD,), SENTINEL, device=dev)
        self.guard = torch.full((K.ADAMW_GUARD_WORDS + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        self.guard[:9] = 0
        self.seg_end = torch.tensor([n], dtype=torch.int64, device=dev)
        self.lr = torch.tensor([1e-2], device=dev)
        self.wd = torch.tensor([1e-2], device=dev)

    def ptr(self, name):
        return self.bufs[name].data_ptr()

    def norm_and_gate(self, max_norm, gscale):
        self.lib.call("spe_sqnorm_partials", self.ptr("g"), self.n, self.partials.data_ptr(), 256, self.st())
        self.lib.call("spe_adamw_gate", self.guard.data_ptr(), self.partials.data_ptr(), 256, max_norm, gscale, BETAS[0], BETAS[1], self.st())

    def update(self, write_grad=1):
        self.lib.call("spe_adamw_flat_guarded", self.ptr("p"), self.ptr("g"), self.ptr("m"), self.ptr("v"), self.n, self.seg_end.data_ptr(),
                      self.lr.data_ptr(), self.wd.data_ptr(), 1, BETAS[0], BETAS[1], EPS, self.guard.data_ptr(), write_grad, self.st())

    def bands_intact(self):
        torch.cuda.synchronize()
        return (all(bool((b[self.n:] == SENTINEL).all()) for b in self.bufs.values()) and bool((self.partials[256:] == SENTINEL).all())
                and bool((self.guard[9:] == 0x5A5A5A5A).all()))       # the reserved words 9 .. 15 and the band behind the block

    def words(self):
        g = self.guard[:9].cpu()
        return g[:4].tolist(), g[4:].view(torch.float32).tolist()


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("n", SIZES)
def test_c_abi_skip_writes_nothing_and_apply_writes_n(dev, n, where):
    """A NaN at the first / the last element (inside the scalar tail where n % 4 != 0): nothing is written.  The same buffers with the
    element repaired: exactly n elements of p, m, v and g are written, and m, v and the clipped g have the BITS of spe_adamw_flat on copies
    (same clip factor, arithmetic that does not see the bias corrections); p agrees to the bound of the torch comparison."""
    a = _Abi(dev, n, n)
    max_norm, gscale = 0.1, 0.5
    idx = 0 if where == "first" else n - 1
    good = a.bufs["g"][idx].clone()
    a.bufs["g"][idx] = float("nan")
    before = {k: b.clone() for k, b in a.bufs.items()}
    a.norm_and_gate(max_norm, gscale)
    a.update()
    assert a.bands_intact()
    assert all(_same_bits(a.bufs[k], before[k]) for k in "pgmv")
    ints, floats = a.words()
    assert ints == [0, 1, 1, 0] and floats[0] == 0.0 and floats[3] != floats[3] and floats[4] == 0.0

    a.bufs["g"][idx] = good
    ref = {k: b.clone() for k, b in a.bufs.items()}
    a.norm_and_gate(max_norm, gscale)
    a.update()
    assert a.bands_intact()
    ints, floats = a.words()
    assert ints == [1, 1, 1, 1] and floats[4] == 1.0
    want_norm = gscale * float(ref["g"][:n].double().pow(2).sum().sqrt())
    assert abs(floats[3] - want_norm) <= 1e-5 * want_norm
    assert abs(floats[0] - gscale * min(1.0, max_norm / (want_norm + 1e-6))) <= 1e-5 * floats[0]
    assert abs(floats[1] - (1 - BETAS[0])) <= 1e-7 and abs(floats[2] - (1 - BETAS[1]) ** 0.5) <= 1e-8
    a.lib.call("spe_adamw_flat", ref["p"].data_ptr(), ref["g"].data_ptr(), ref["m"].data_ptr(), ref["v"].data_ptr(), n, a.seg_end.data_ptr(),
               a.lr.data_ptr(), a.wd.data_ptr(), 1, BETAS[0], BETAS[1], EPS, 1 - BETAS[0], 1 - BETAS[1], a.partials.data_ptr(), 256, max_norm,
               1, gscale, a.st())
    torch.cuda.synchronize()
    for k in "gmv":
        assert torch.equal(a.bufs[k], ref[k]), k
    assert rel(a.bufs["p"][:n], ref["p"][:n]) < 2e-6
    # (exactly n written: the n elements equal those of the unguarded entry, the bands behind them are intact)
    assert not torch.equal(a.bufs["p"][:n], before["p"][:n])


def test_c_abi_refusals(dev):
    from spe_amd import lib
    a = _Abi(dev, 1024, 3)
    st = a.st()
    before = {k: b.clone() for k, b in a.bufs.items()}
    gp, pp = a.guard.data_ptr(), a.partials.data_ptr()
    for args in ((gp + 4, pp, 256), (None, pp, 256), (gp, None, 256), (gp, pp, 0)):
        with pytest.raises(lib.SpeLibraryError, match="-2"):
            lib.call("spe_adamw_gate", args[0], args[1], args[2], 0.1, 1.0, BETAS[0], BETAS[1], st)
    ptrs = [a.ptr(k) for k in "pgmv"]
    tail = (a.seg_end.data_ptr(), a.lr.data_ptr(), a.wd.data_ptr())

    def upd(ptrs, n, nseg, guard):
        lib.call("spe_adamw_flat_guarded", *ptrs, n, *tail, nseg, BETAS[0], BETAS[1], EPS, guard, 1, st)
    a.guard[3] = 1                                        # apply: a refused call must not have launched
    armed = a.guard.clone()
    for i in range(4):
        bad = list(ptrs)
        bad[i] += 4
        with pytest.raises(lib.SpeLibraryError, match="-2"):
            upd(bad, 1024, 1, gp)
    for nseg in (0, 65):
        with pytest.raises(lib.SpeLibraryError, match="-2"):
            upd(ptrs, 1024, nseg, gp)
    for g in (gp + 4, None):
        with pytest.raises(lib.SpeLibraryError, match="-2"):
            upd(ptrs, 1024, 1, g)
    upd(ptrs, 0, 1, gp)                                   # n <= 0: status 0, nothing launched
    upd(ptrs, -5, 1, gp)
    torch.cuda.synchronize()
    assert all(_same_bits(a.bufs[k], before[k]) for k in "pgmv")
    assert torch.equal(a.guard, armed)
