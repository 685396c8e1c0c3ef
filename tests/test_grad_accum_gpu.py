"""Gradient accumulation on the GPU: the spe_accum_flat kernel, FlatAdamW over a cycle of micro-steps against torch, and the
product model - the merged bucket of a cycle is bit for bit the ordered sum of the micro-steps' own buckets, an accumulated step
equals a plain step on the averaged bucket, and the whole thing is reproducible run to run."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
pytestmark = pytest.mark.gpu

GRID_CAP = 2048                     # workgroups of spe_accum_flat (and spe_adamw_flat) at most; each sweeps 1024 elements per pass
GUARD = 64
SENTINEL = 12345.0
SIZES = [1, 3, 4, 5, 255, 256, 1023, 1024, 1025, GRID_CAP * 1024 + 7]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _bits(t):
    return t.view(torch.int32)


def _guarded(src, dev):
    """A device buffer of src.numel() + GUARD floats: src, then the sentinel.  -> (buffer, view of the first n)"""
    n = src.numel()
    buf = torch.full((n + GUARD,), SENTINEL, device=dev)
    buf[:n] = src.to(dev)
    return buf, buf[:n]


def _data(n, seed):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    # special values wherever they fit: -0.0 (alone and against -0.0 / +0.0), inf, NaN
    a[0] = -0.0; b[0] = -0.0
    if n > 2:
        a[1] = float("inf")
        a[2] = -0.0; b[2] = 0.0
    if n > 4:
        a[n - 1] = float("nan")           # in the scalar tail when n % 4 != 0
        b[n // 2] = float("-inf")
    return a, b


@pytest.mark.parametrize("form", ["fresh", "dst_is_a", "dst_is_b"])
@pytest.mark.parametrize("n", SIZES)
def test_accum_flat_sum(dev, n, form):
    from spe_amd import kernels as K
    a_h, b_h = _data(n, n)
    abuf, a = _guarded(a_h, dev)
    bbuf, b = _guarded(b_h, dev)
    want = a + b                                             # an fp32 add is exactly rounded: one right answer
    a0, b0 = a.clone(), b.clone()
    if form == "fresh":
        dbuf, dst = _guarded(torch.full((n,), 777.0), dev)
    else:
        dbuf, dst = (abuf, a) if form == "dst_is_a" else (bbuf, b)
    assert K.accum_flat(dst, a, b) is dst
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(dst), nan)
    assert torch.equal(dst[~nan], want[~nan])
    assert torch.equal(_bits(dst)[~nan], _bits(want)[~nan])          # the sign of zero too
    for buf in (abuf, bbuf, dbuf):
        assert bool((buf[n:] == SENTINEL).all()), "wrote past the end"
    if dst is not a:
        assert torch.equal(_bits(a), _bits(a0))
    if dst is not b:
        assert torch.equal(_bits(b), _bits(b0))


@pytest.mark.parametrize("form", ["fresh", "dst_is_a"])
@pytest.mark.parametrize("n", SIZES)
def test_accum_flat_copy_is_bitwise(dev, n, form):
    from spe_amd import kernels as K
    a_h, _ = _data(n, 1000 + n)
    abuf, a = _guarded(a_h, dev)
    a0 = a.clone()
    dbuf, dst = _guarded(torch.full((n,), 777.0), dev) if form == "fresh" else (abuf, a)
    K.accum_flat(dst, a)
    assert torch.equal(_bits(dst), _bits(a0))                # -0.0 stays -0.0, the NaN keeps its bits
    assert torch.equal(_bits(a), _bits(a0))
    assert bool((abuf[n:] == SENTINEL).all()) and bool((dbuf[n:] == SENTINEL).all())


def test_accum_flat_rejects_misaligned_and_empty(dev):
    from spe_amd import kernels as K
    from spe_amd import lib
    n = 1024
    a, b = torch.randn(n + 4, device=dev), torch.randn(n + 4, device=dev)
    dst = torch.full((n + 4,), SENTINEL, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    ptrs = [dst.data_ptr(), a.data_ptr(), b.data_ptr()]
    for i in range(3):
        args = list(ptrs)
        args[i] += 4
        with pytest.raises(lib.SpeLibraryError, match="-2"):
            lib.call("spe_accum_flat", *args, n, st)
    with pytest.raises(lib.SpeLibraryError, match="-2"):
        lib.call("spe_accum_flat", ptrs[0] + 4, ptrs[1], None, n, st)
    lib.call("spe_accum_flat", ptrs[0], ptrs[1], ptrs[2], 0, st)         # n <= 0: status 0, nothing launched
    lib.call("spe_accum_flat", ptrs[0], ptrs[1], None, -5, st)
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all())
    with pytest.raises(ValueError):
        K.accum_flat(dst, a[:n], b)
    with pytest.raises(lib.SpeLibraryError):
        K.accum_flat(dst.cpu(), a.cpu(), b.cpu())


def test_flat_adamw_accumulated_matches_torch(dev):
    """FlatAdamW over cycles of K = 3 micro-steps == clip_grad_norm_(0.1) + torch.optim.AdamW on the MEAN of the three gradients
    (shapes, groups, scales and bounds of test_flat_adamw_matches_torch): the 1/K rides on the update launch's grad_scale."""
    from spe_amd.dp import GradAllReducer
    from spe_amd.optim import FlatAdamW
    KS = 3
    g = torch.Generator().manual_seed(21)
    shapes = [(64, 32), (64,), (7, 5, 3), (1,), (300, 17), (33,)]
    mk = lambda: [torch.nn.Parameter(torch.randn(*s, generator=torch.Generator().manual_seed(i)).to(dev)) for i, s in enumerate(shapes)]
    pa, pb = mk(), mk()
    groups = lambda ps: [{"params": ps[:3], "lr": 1e-2, "weight_decay": 1e-2}, {"params": ps[3:], "lr": 3e-3, "weight_decay": 0.0}]
    ref = torch.optim.AdamW(groups(pa), betas=(0.9, 0.999), eps=1e-8)
    red = GradAllReducer(pb, bucket_bytes=4096, flatten_params=True, accum_steps=KS)
    opt = FlatAdamW(groups(pb), red, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.1)
    assert red.grad_scale() == 1.0 / KS
    for it in range(3):
        micro = []
        for m in range(KS):
            red.reset()
            grs = []
            for y in pb:
                gr = torch.randn(y.shape, generator=g).to(dev) * (10.0 if it == 1 else 0.01)      # clipped and unclipped steps
                y.grad = red._views[y]; y.grad.copy_(gr)
                grs.append(gr)
            micro.append(grs)
            red.finish()
            if m == 0:
                with pytest.raises(RuntimeError, match="accum_steps = 3"):
                    opt.step()
                assert opt._step == it                       # the refused call changed nothing
        for i, x in enumerate(pa):
            x.grad = (micro[0][i] + micro[1][i] + micro[2][i]) / KS
        torch.nn.utils.clip_grad_norm_(pa, 0.1)
        ref.step(); opt.step()
        for x, y in zip(pa, pb):
            assert rel(y, x) < 2e-6, (it, rel(y, x))
            assert rel(y.grad, x.grad) < 2e-6
    for x, y in zip(pa, pb):
        assert rel(opt.state[y]["exp_avg"], ref.state[x]["exp_avg"]) < 2e-6
        # v accumulates (clip * g)^2: twice the relative rounding difference of the two global-norm reductions
        assert rel(opt.state[y]["exp_avg_sq"], ref.state[x]["exp_avg_sq"]) < 5e-5
    red.remove()


# ---- product model ------------------------------------------------------------------------------------------------------------
DEPTH, HW = 2, (256, 320)


class _Run:
    """The training step of tools/determinism_step.py at a small size, one micro-batch per round (seeds 4321, 4322, ...)."""

    def __init__(self, dev, accum_steps, nbatches):
        import bench
        from spe_amd import kernels as K
        from spe_amd.dp import GradAllReducer
        from spe_amd.optim import FlatAdamW
        from spe_amd.models import build_model
        from spe_amd.models.cait import TSCAM_cait, _make, register_model
        from spe_amd.util.misc import NestedTensor
        name = f"TSCAM_cait_S24_depth{DEPTH}"

        def fac(pretrained=False, **kw):
            return _make(TSCAM_cait, 384, DEPTH, 8, 1e-5, False, **kw)
        fac.__name__ = name
        try:
            register_model(fac)
        except Exception:
            pass
        K.set_precision("bf16s")
        K.manual_seed(77)
        args = bench.model_args(backbone=name, enc_layers=1, layer_to_det=DEPTH - 1, dropout=0.1)
        torch.manual_seed(0)
        self.model, self.crit, self.crit_r, _, self.rpp = build_model(args)
        with torch.no_grad():
            for n, p in self.model.named_parameters():
                if n.endswith("gamma_1") or n.endswith("gamma_2"):
                    p.fill_(0.2)
        self.model.to(dev).train(); self.crit.to(dev).train(); self.crit_r.to(dev).train()
        named = [(n, p) for n, p in self.model.named_parameters() if p.requires_grad]
        self.params = [p for _, p in named]
        self.red = GradAllReducer(self.params, flatten_params=True, accum_steps=accum_steps)
        groups = [{"params": [p for n, p in named if "backbone" not in n], "lr": 1e-4},
                  {"params": [p for n, p in named if "backbone" in n], "lr": 1e-5}]
        self.opt = FlatAdamW(groups, self.red, lr=1e-4, weight_decay=1e-4, max_grad_norm=0.1)
        self.batches = []
        for k in range(nbatches):
            img, mask, targets = bench.synth_batch(4321 + k, dev, batch=1, H=HW[0], W=HW[1])
            self.batches.append((NestedTensor(img, mask), targets))

    def round(self, k):
        """reset / forward / backward / finish on micro-batch k -> clones of the buckets afterwards"""
        import bench
        samples, targets = self.batches[k]
        self.red.reset()
        out = self.model(samples)
        l0 = self.crit(out[0], targets)
        with torch.no_grad():
            ps = bench.pseudo_labels(self.rpp, out[0], targets)
        l1 = self.crit_r(out[1], ps)
        bench.weighted_total(l0, l1, self.crit.weight_dict).backward()
        self.red.finish()
        return [b["flat"].clone() for b in self.red.buckets]

    def close(self):
        self.red.remove()


def _bad_params(run, got, want):
    """Names of the parameters whose bucket slice differs (for the message: small ones point at the deferred sums)."""
    names = {p: n for n, p in run.model.named_parameters()}
    bad = []
    for b, x, y in zip(run.red.buckets, got, want):
        for p, off in b["offsets"]:
            if not torch.equal(x[off:off + p.numel()], y[off:off + p.numel()]):
                bad.append((names[p], p.numel()))
    return bad


def test_model_bucket_of_a_cycle_is_the_ordered_sum(dev):
    """accum_steps = 3 on micro-batches [A, B, C] leaves (gA + gB) + gC in every bucket, where gA, gB, gC are the buckets of the same
    three rounds with accum_steps = 1 (no optimizer step in either run: same parameters, same call sequence, same Philox offsets)."""
    a = _Run(dev, 1, 3)
    gA, gB, gC = a.round(0), a.round(1), a.round(2)
    assert a.red.grad_scale() == 1.0 and all(b["acc"] is None for b in a.red.buckets)
    a.close()
    assert any(float(x.abs().max()) > 0 for x in gA) and not all(torch.equal(x, y) for x, y in zip(gA, gB))
    r = _Run(dev, 3, 3)
    assert r.red.grad_scale() == 1.0 / 3
    f0 = r.round(0)
    assert r.red.micro == 1 and all(b["work"] == "local" for b in r.red.buckets)
    assert not _bad_params(r, f0, gA)                        # a non-final micro-step leaves its own gradient in the bucket
    r.round(1)
    assert r.red.micro == 2
    got = r.round(2)
    assert r.red.micro == 0
    want = [(x + y) + z for x, y, z in zip(gA, gB, gC)]
    bad = _bad_params(r, got, want)
    r.close()
    assert not bad, (bad[:10], len(bad))
    assert all(torch.equal(x, y) for x, y in zip(got, want))             # the padding between the views too


def test_model_accumulated_step_equals_step_on_the_mean(dev):
    """K = 2 on [A, B] then opt.step() == accum_steps = 1, buckets overwritten with (gA + gB) * 0.5, then opt.step(): bitwise equal
    parameters (the factor 0.5 is exact through the norm, the clip factor and the update of adamw_flat_kernel)."""
    a = _Run(dev, 1, 2)
    gA, gB = a.round(0), a.round(1)
    for b, x, y in zip(a.red.buckets, gA, gB):
        b["flat"].copy_((x + y) * 0.5)
    a.opt.step()
    want = [p.detach().clone() for p in a.params]
    names = [n for n, p in a.model.named_parameters() if p.requires_grad]
    a.close()
    r = _Run(dev, 2, 2)
    before = [p.detach().clone() for p in r.params]
    r.round(0)
    got_flat = r.round(1)
    assert all(torch.equal(f, x + y) for f, x, y in zip(got_flat, gA, gB))
    r.opt.step()
    got = [p.detach().clone() for p in r.params]
    r.close()
    assert any(not torch.equal(x, y) for x, y in zip(before, got))       # the step moved something
    bad = [n for n, x, y in zip(names, got, want) if not torch.equal(x, y)]
    assert not bad, (bad[:10], len(bad))


def test_accumulated_training_is_bitwise_reproducible(dev):
    """Two optimizer steps of two micro-batches each, run twice with foreign kernels in between in the second run."""
    import determinism_step as D
    xs = torch.randn(2048, 1024, device=dev)
    runs = []
    for r in range(2):
        noise = None if r == 0 else (lambda r=r: [(xs @ xs.t()[:, :512 * r]).sum() for _ in range(2 * r)])
        runs.append(D.run_steps(dev, depth=DEPTH, H=HW[0], W=HW[1], batch=1, enc_layers=1, steps=2, precision="bf16s", noise=noise,
                                accum_steps=2))
    names, g0, p0, loss0 = runs[0]
    _, g1, p1, loss1 = runs[1]
    assert loss1 == loss0
    bad_g = [n for n, a, b in zip(names, g0, g1) if a is not None and not torch.equal(a, b)]
    bad_p = [n for n, a, b in zip(names, p0, p1) if not torch.equal(a, b)]
    assert not bad_g, ("gradients differ run to run", bad_g[:10], len(bad_g))
    assert not bad_p, ("parameters differ run to run", bad_p[:10], len(bad_p))
