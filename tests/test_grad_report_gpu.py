"""spe_grad_report and FlatAdamW(skip_report=...) / grad_stats() on the GPU: the records against the numpy restatement of the documented
order (grad_report_ref.py) bit for bit, the exact words against brute force, the gating on the guard block, the refusals, and the
optimizer-level behaviour on the six-tensor, two-bucket setup of test_adamw_guard_gpu.py.

The C-entry tests pack one parameter per length of grad_report_cases.LENGTHS into a single bucket; the space between the parameters
and 64 elements in front of and behind the bucket hold NaN, so a read outside a parameter shows in its record."""
import functools
import math

import numpy as np
import pytest
import torch

import grad_report_ref as R
from grad_report_cases import BETAS, CHUNK, EPS, LENGTHS, LONG_LENGTH, SHAPES, VALUE_SETS, grad_values, weight_values

pytestmark = pytest.mark.gpu

BAND = 64
PATTERN = 0x5A5A5A5A
SCALES = [1.0, 0.5]
NONFINITE_SETS = ["nan_first", "inf_last", "neginf_middle", "nan_then_inf", "inf_then_nan"]


@functools.lru_cache(maxsize=None)
def _tensors(name, L):
    return grad_values(name, L), weight_values(L)


@functools.lru_cache(maxsize=None)
def _ref_words(name, L, scale, with_p=True):
    """The restatement's eight words (attempt 0): computed once per case, shared by every test, never modified."""
    g, p = _tensors(name, L)
    w = R.words(R.record32(g, p if with_p else None, scale))
    w.setflags(write=False)
    return w


class _Bucket:
    """Parameters (g, p pairs) at given offsets of two flat buffers of n elements between two bands; everything else is `fill`."""

    def __init__(self, dev, pairs, offsets, n, fill=float("nan")):
        g = np.full(n + 2 * BAND, fill, dtype=np.float32)
        p = np.full(n + 2 * BAND, fill, dtype=np.float32)
        for (gv, pv), off in zip(pairs, offsets):
            assert 0 <= off and off + gv.size <= n
            g[BAND + off:BAND + off + gv.size] = gv
            p[BAND + off:BAND + off + pv.size] = pv
        self.n, self.npar = n, len(pairs)
        self.g, self.p = torch.from_numpy(g).to(dev), torch.from_numpy(p).to(dev)
        self.beg = torch.tensor(list(offsets), dtype=torch.int64, device=dev)
        self.len = torch.tensor([gv.size for gv, _ in pairs], dtype=torch.int64, device=dev)

    def args(self, with_p=True):
        return (self.g.data_ptr() + 4 * BAND, self.p.data_ptr() + 4 * BAND if with_p else None, self.n, self.beg.data_ptr(), self.len.data_ptr(),
                self.npar)


def _fresh_out(dev, npar):
    return torch.full((npar, 8), PATTERN, dtype=torch.int32, device=dev)


def _run(dev, b, scale=1.0, with_p=True, guard=None, when=0, out=None):
    """-> the records as uint32 [npar, 8] on the host."""
    from spe_amd import kernels as K, lib
    out = _fresh_out(dev, b.npar) if out is None else out
    lib.call("spe_grad_report", *b.args(with_p), scale, None if guard is None else guard.data_ptr(), when, out.data_ptr(), K._st())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def _aligned_offsets(lengths, gap=0):
    offs, off = [], 0
    for L in lengths:
        offs.append(off)
        off = ((off + L + 63) & ~63) + gap
    return offs, off


def _packed(dev, name, fill=float("nan")):
    offs, n = _aligned_offsets(LENGTHS)
    return _Bucket(dev, [_tensors(name, L) for L in LENGTHS], offs, n, fill)


# ---- the C entry, when = 0 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", VALUE_SETS)
def test_c_abi_records_match_the_restatement_and_brute_force(dev, name, scale):
    """Every length: words 0 and 2 have the restatement's bits, words 1 and 3 .. 6 the brute-force values, word 7 is 0 without a guard
    block; NaN in the padding changes nothing (so it is never read); a second run returns the same bits."""
    b = _packed(dev, name)
    got = _run(dev, b, scale)
    for i, L in enumerate(LENGTHS):
        want = _ref_words(name, L, scale)
        assert np.array_equal(got[i, :7], want[:7]), (L, got[i], want)
        assert got[i, 7] == 0
        g, p = _tensors(name, L)
        br = R.brute(g, p, scale)
        ints = got[i].view(np.int32)
        assert (ints[4], ints[5], ints[6]) == (br["nan"], br["inf"], br["first_bad"]), L
        assert got[i, 1] == np.float32(br["grad_absmax"]).view(np.uint32) and got[i, 3] == np.float32(br["weight_absmax"]).view(np.uint32), L
    assert np.array_equal(_run(dev, b, scale), got)
    assert np.array_equal(_run(dev, _packed(dev, name, fill=0.0), scale), got)


@pytest.mark.parametrize("name", VALUE_SETS)
def test_c_abi_without_weights_words_two_and_three_are_zero(dev, name):
    b = _packed(dev, name)
    got, full = _run(dev, b, 0.5, with_p=False), _run(dev, b, 0.5)
    assert not got[:, 2:4].any() and full[:, 2:4].any()
    assert np.array_equal(got[:, [0, 1, 4, 5, 6, 7]], full[:, [0, 1, 4, 5, 6, 7]])
    for i, L in enumerate(LENGTHS):
        assert np.array_equal(got[i], _ref_words(name, L, 0.5, with_p=False))


@pytest.mark.parametrize("name", VALUE_SETS)
def test_c_abi_record_is_a_function_of_the_parameter_alone(dev, name):
    """The same tensors in reverse order, at other offsets (16-B aligned or not), in a larger bucket, beside further parameters, and
    one alone at offset 0: the same bits every time."""
    base = _run(dev, _packed(dev, name), 0.5)
    order = list(reversed(range(len(LENGTHS))))
    pairs, offs, off = [], [], 128
    for k, i in enumerate(order):
        pairs.append(_tensors(name, LENGTHS[i]))
        offs.append(off + (k % 4))                                   # 0, 1, 2, 3 elements past a 256-B boundary
        off = ((off + LENGTHS[i] + 67) & ~63) + 64 * (k % 3)
        if k % 5 == 0:                                               # a neighbour full of NaN and infinities in between
            junk = np.full(97, np.nan, dtype=np.float32)
            junk[::2] = np.inf
            pairs.append((junk, junk))
            offs.append(off)
            off += 128
    other = _run(dev, _Bucket(dev, pairs, offs, off + 4096), 0.5)
    assert len(pairs) > len(LENGTHS)
    rows = [r for r, pr in zip(other, pairs) if pr[0].size != 97]
    for k, i in enumerate(order):
        assert np.array_equal(rows[k], base[i]), LENGTHS[i]
    for i in (0, 5, len(LENGTHS) - 1):
        alone = _run(dev, _Bucket(dev, [_tensors(name, LENGTHS[i])], [0], LENGTHS[i]), 0.5)
        assert np.array_equal(alone[0], base[i]), LENGTHS[i]


@pytest.mark.parametrize("name", NONFINITE_SETS)
def test_c_abi_nonfinite_elements_count_as_plus_zero(dev, name):
    offs, n = _aligned_offsets(LENGTHS)
    cleaned = [(np.where(np.isfinite(g), g, np.float32(0.0)).astype(np.float32), p) for g, p in (_tensors(name, L) for L in LENGTHS)]
    dirty, clean = _run(dev, _packed(dev, name), 0.5), _run(dev, _Bucket(dev, cleaned, offs, n), 0.5)
    assert np.array_equal(dirty[:, :4], clean[:, :4])
    assert (dirty[:, 4] + dirty[:, 5] > 0).all() and not clean[:, 4:6].any() and (clean[:, 6].view(np.int32) == -1).all()


def test_c_abi_parameter_whose_fold_wraps(dev):
    """More chunks than the folding workgroup stages per round, beside a small neighbour: still the restatement's bits."""
    rng = np.random.default_rng(5)
    g, p = rng.standard_normal(LONG_LENGTH).astype(np.float32), rng.standard_normal(LONG_LENGTH).astype(np.float32)
    g[200 * CHUNK + 17], g[LONG_LENGTH - 2] = np.nan, np.inf
    off = ((64 + LONG_LENGTH + 63) & ~63) + 64
    got = _run(dev, _Bucket(dev, [(g, p), _tensors("normal", 65)], [64, off], off + 128), 0.5)
    want = R.record32(g, p, 0.5)
    assert np.array_equal(got[0, :7], R.words(want)[:7]) and np.array_equal(got[1], _ref_words("normal", 65, 0.5))
    fin = np.isfinite(g)
    assert (want["nan"], want["inf"], want["first_bad"]) == (1, 1, 200 * CHUNK + 17)
    assert want["grad_absmax"] == np.abs(np.float32(0.5) * g[fin]).max() and want["weight_absmax"] == np.abs(p).max()
    assert abs(float(want["grad_sq"]) - 0.25 * float(np.sum(g[fin].astype(np.float64) ** 2))) <= R.bound(LONG_LENGTH, 0.25 * float(np.sum(g[fin].astype(np.float64) ** 2)), 3)


# ---- gating ----------------------------------------------------------------------------------------------------------------------------
def _guard(dev, applied, skipped, apply):
    from spe_amd import kernels as K
    g = torch.full((K.ADAMW_GUARD_WORDS,), 0x33333333, dtype=torch.int32, device=dev)
    g[K.GUARD_APPLIED], g[K.GUARD_SKIPPED], g[K.GUARD_FIRST], g[K.GUARD_APPLY] = applied, skipped, (applied + 1 if skipped else 0), apply
    return g


def test_gating_on_the_guard_block(dev):
    b = _packed(dev, "inf_last")
    plain = _run(dev, b, 1.0)
    untouched = _fresh_out(dev, b.npar).cpu().numpy().view(np.uint32)
    for applied, skipped, apply, writes in ((3, 1, 1, {0}), (4, 0, 1, {0}), (3, 1, 0, {0, 1, 2}), (3, 2, 0, {0, 1}), (0, 1, 0, {0, 1, 2})):
        guard = _guard(dev, applied, skipped, apply)
        before = guard.clone()
        for when in (0, 1, 2):
            got = _run(dev, b, 1.0, guard=guard, when=when)
            if when in writes:
                assert np.array_equal(got[:, :7], plain[:, :7]) and (got[:, 7] == applied + skipped).all(), (applied, skipped, apply, when)
            else:
                assert np.array_equal(got, untouched), (applied, skipped, apply, when)
        assert torch.equal(guard, before)                            # the guard block is read only


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals(dev):
    from spe_amd import kernels as K, lib
    b = _Bucket(dev, [_tensors("normal", 257), _tensors("normal", 1025)], [0, 320], 1408)
    out = _fresh_out(dev, b.npar)
    guard = _guard(dev, 1, 1, 0)
    g, p, n, beg, ln, npar = b.args()
    o, gd, st = out.data_ptr(), guard.data_ptr(), K._st()
    refused = [
        (None, p, n, beg, ln, npar, 1.0, None, 0, o), (g + 4, p, n, beg, ln, npar, 1.0, None, 0, o),          # g NULL / misaligned
        (g, p, n, beg, ln, npar, 1.0, None, 0, None), (g, p, n, beg, ln, npar, 1.0, None, 0, o + 4),          # out NULL / misaligned
        (g, p + 4, n, beg, ln, npar, 1.0, None, 0, o),                                                        # p misaligned
        (g, p, n, beg, ln, 0, 1.0, None, 0, o), (g, p, n, beg, ln, -1, 1.0, None, 0, o),                      # npar < 1
        (g, p, n, beg, ln, npar, 1.0, gd, -1, o), (g, p, n, beg, ln, npar, 1.0, gd, 3, o),                    # when outside 0..2
        (g, p, n, beg, ln, npar, 1.0, None, 1, o), (g, p, n, beg, ln, npar, 1.0, None, 2, o),                 # gated without a guard block
        (g, p, n, beg, ln, npar, 1.0, gd + 4, 1, o), (g, p, n, beg, ln, npar, 1.0, gd + 4, 2, o),             # ... with a misaligned one
        (g, p, n, None, ln, npar, 1.0, None, 0, o), (g, p, n, beg, None, npar, 1.0, None, 0, o),              # a table missing
    ]
    for a in refused:
        with pytest.raises(lib.SpeLibraryError, match="-2"):
            lib.call("spe_grad_report", *a, st)
    lib.call("spe_grad_report", g, p, 0, beg, ln, npar, 1.0, None, 0, o, st)                                  # n <= 0: status 0, nothing launched
    lib.call("spe_grad_report", g, p, -5, beg, ln, npar, 1.0, gd, 1, o, st)
    torch.cuda.synchronize()
    assert bool((out == PATTERN).all())
    with pytest.raises(TypeError):
        K.grad_report(b.g.double(), None, b.beg, b.len, 1.0, out)
    with pytest.raises(ValueError):
        K.grad_report(b.g, None, b.beg, b.len, 1.0, out[:1])
    with pytest.raises(ValueError):
        K.grad_report(b.g, None, b.beg.int(), b.len, 1.0, out)
    assert K.GRAD_REPORT_WORDS == 8


# ---- the optimizer ---------------------------------------------------------------------------------------------------------------------
def _params(dev):
    return [torch.nn.Parameter(torch.randn(*s, generator=torch.Generator().manual_seed(i)).to(dev)) for i, s in enumerate(SHAPES)]


def _groups(ps):
    return [{"params": ps[:3], "lr": 1e-2, "weight_decay": 1e-2}, {"params": ps[3:], "lr": 3e-3, "weight_decay": 0.0}]


class _Opt:
    """Six parameters in flat buckets with a guarded FlatAdamW on them."""

    def __init__(self, dev, accum_steps=1, **kw):
        from spe_amd.dp import GradAllReducer
        from spe_amd.optim import FlatAdamW
        self.ps = _params(dev)
        self.model = torch.nn.ParameterList(self.ps)                  # names "0" .. "5"
        self.red = GradAllReducer(self.ps, bucket_bytes=4096, flatten_params=True, accum_steps=accum_steps)
        self.opt = FlatAdamW(_groups(self.ps), self.red, betas=BETAS, eps=EPS, max_grad_norm=0.1, skip_nonfinite=True, **kw)
        assert len(self.red.buckets) >= 2

    def feed(self, grads):
        self.red.reset()
        for y, gr in zip(self.ps, grads):
            y.grad = self.red._views[y]
            y.grad.copy_(gr)
        self.red.finish()

    def state(self):
        """Clones of parameters, both moments and (where kept) the EMA of every bucket."""
        return [t.clone() for e in self.opt._buckets for t in (e["b"]["flat_p"], e["m"], e["v"], e["ema"]) if t is not None]

    def close(self):
        self.red.remove()


def _grads(dev, seed, scale=0.01):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(dev) * scale for s in SHAPES]


def _poisoned(grads, which, flat_index, value):
    bad = [g.clone() for g in grads]
    bad[which].view(-1)[flat_index] = value
    return bad


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_report_names_the_parameter_behind_the_skipped_step(dev):
    """clean, inf at parameter 4, clean, NaN at parameter 2: "first" keeps the first skipped step, "last" shows the latest."""
    first, last = _Opt(dev, skip_report="first"), _Opt(dev, skip_report="last")
    g1, g2 = _grads(dev, 11), _grads(dev, 12, 10.0)
    bad = _poisoned(g2, 4, 7, float("inf"))
    for o in (first, last):
        assert o.opt.skip_report() is None
        o.feed(g1); o.opt.step()
        assert o.opt.skip_report(o.model) is None
        o.feed(bad)
        raw = [t.clone() for t in o.opt.grad_stats(raw=True)]        # the same buckets, unconditionally
        o.opt.step()
        rep = o.opt.skip_report(o.model)
        assert rep["attempt"] == o.opt.first_skipped() == 2 and o.opt.skipped_steps() == 1
        assert [r["name"] for r in rep["culprits"]] == ["4"] and not rep["total_overflow"]
        c = rep["culprits"][0]
        assert (c["inf"], c["nan"], c["first_bad"], c["shape"], c["numel"]) == (1, 0, tuple(int(i) for i in np.unravel_index(7, SHAPES[4])), SHAPES[4], 300 * 17)
        number = {id(p): str(i) for i, p in enumerate(o.ps)}
        assert [r["name"] for r in rep["params"]] == [number[id(p)] for b in o.red.buckets for p, _ in b["offsets"]]
        for e, r in zip(o.opt._buckets, raw):
            assert torch.equal(e["report"][:, :7], r[:, :7]) and bool((e["report"][:, 7] == 2).all()) and not bool(r[:, 7].any())
        rows = o.opt.grad_stats(o.model)                             # and as rows
        assert [(r["name"], r["grad_sq"], r["nan"], r["inf"], r["first_bad"]) for r in rows] == \
               [(r["name"], r["grad_sq"], r["nan"], r["inf"], r["first_bad"]) for r in rep["params"]]
        for r, p in zip(rows, (p for b in o.red.buckets for p, _ in b["offsets"])):
            assert abs(r["weight_norm"] - float(p.detach().double().norm())) <= 1e-5 * r["weight_norm"] + 1e-30
            assert r["weight_absmax"] == float(p.detach().abs().max()) and r["grad_norm"] == math.sqrt(r["grad_sq"])
        assert len(rep["largest"]) == 5 and len(o.opt.skip_report(top=2)["largest"]) == 2
        assert o.opt.skip_report()["culprits"][0]["name"].startswith("bucket")          # without a model: positional names
        o.feed(g2); o.opt.step()                                     # an applied step writes nothing
        assert o.opt.skip_report(o.model)["attempt"] == 2
        o.feed(_poisoned(g1, 2, 50, float("nan"))); o.opt.step()
        assert (o.opt.applied_steps(), o.opt.skipped_steps(), o.opt.first_skipped()) == (2, 2, 2)
    rep = first.opt.skip_report(first.model)
    assert rep["attempt"] == 2 and [r["name"] for r in rep["culprits"]] == ["4"]
    rep = last.opt.skip_report(last.model)
    assert rep["attempt"] == 4 and [r["name"] for r in rep["culprits"]] == ["2"]
    c = rep["culprits"][0]
    assert (c["nan"], c["inf"], c["first_bad"]) == (1, 0, tuple(int(i) for i in np.unravel_index(50, SHAPES[2])))
    first.close(); last.close()


def test_a_finite_element_whose_square_overflows_is_the_only_culprit(dev):
    o = _Opt(dev, skip_report="first")
    o.feed(_poisoned(_grads(dev, 21), 0, 5, 3e19)); o.opt.step()
    assert (o.opt.applied_steps(), o.opt.skipped_steps()) == (0, 1)
    rep = o.opt.skip_report(o.model)
    assert all(r["nan"] == 0 and r["inf"] == 0 and r["first_bad"] is None for r in rep["params"])
    assert [r["name"] for r in rep["culprits"]] == ["0"] and not rep["total_overflow"]
    c = rep["culprits"][0]
    assert c["grad_sq"] == float("inf") and c["grad_norm"] == float("inf") and c["grad_absmax"] == float(np.float32(3e19))
    assert rep["largest"][0]["name"] == "0"
    o.close()


def test_total_only_overflow_has_no_culprit(dev):
    """Two elements per parameter whose squares sum to a finite value in three parameters; only the sum over the parameters overflows."""
    grads = _grads(dev, 31)
    for which, value in ((4, 1.25e19), (0, 1.2e19), (2, 1.1e19)):
        grads[which].view(-1)[3] = value
        grads[which].view(-1)[-2] = -value
    o = _Opt(dev, skip_report="last")
    o.feed(grads); o.opt.step()
    assert o.opt.skipped_steps() == 1
    rep = o.opt.skip_report(o.model, top=4)
    assert rep["culprits"] == [] and rep["total_overflow"] is True
    assert all(np.isfinite(r["grad_sq"]) for r in rep["params"])
    assert [r["name"] for r in rep["largest"][:3]] == ["4", "0", "2"] and len(rep["largest"]) == 4
    amax = [r["grad_absmax"] for r in rep["largest"]]
    assert amax == sorted(amax, reverse=True) and amax[3] == max(r["grad_absmax"] for r in rep["params"] if r["name"] not in "402")
    o.close()


def test_accumulation_reports_the_accumulated_sum(dev):
    o = _Opt(dev, accum_steps=2, skip_report="first")
    o.feed(_poisoned(_grads(dev, 41), 4, 7, float("inf")))
    assert o.red.micro == 1
    with pytest.raises(RuntimeError):
        o.opt.grad_stats()
    with pytest.raises(RuntimeError):
        o.opt.grad_stats(raw=True)
    o.feed(_grads(dev, 42))
    assert o.red.micro == 0
    o.opt.step()
    assert (o.opt.applied_steps(), o.opt.skipped_steps()) == (0, 1)
    rep = o.opt.skip_report(o.model)
    assert rep["attempt"] == 1 and [r["name"] for r in rep["culprits"]] == ["4"]
    assert rep["culprits"][0]["inf"] == 1 and rep["culprits"][0]["first_bad"] == (0, 7)
    assert len(o.opt.grad_stats()) == len(SHAPES)                   # the cycle is complete: allowed again
    o.close()


def _step_counts(dev, o, seed):
    from spe_amd import lib
    o.feed(_grads(dev, seed))
    torch.cuda.synchronize()
    lib.count_launches(True)
    torch.cuda.set_sync_debug_mode("error")
    try:
        o.opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return lib.count_launches(False)


def test_without_skip_report_nothing_is_allocated_and_nothing_is_launched(dev):
    o, plain = _Opt(dev, skip_report=None), _Opt(dev)
    assert o.opt.skip_report_mode is None
    assert all(e["report"] is None and e["par_tab"] is None and e["stats"] is None for e in o.opt._buckets)
    with pytest.raises(RuntimeError):
        o.opt.skip_report()
    for x in (o, plain):
        x.feed(_grads(dev, 50)); x.opt.step()                        # first call: the segment tables
    a, b = _step_counts(dev, o, 51), _step_counts(dev, plain, 51)
    assert a == b and "spe_grad_report" not in a and a["spe_adamw_flat_guarded"] == len(o.opt._buckets)
    sa, sb = o.opt.state_dict(), plain.opt.state_dict()
    assert sa.keys() == sb.keys() and sa["state"].keys() == sb["state"].keys()
    o.close(); plain.close()


@pytest.mark.parametrize("mode", ["first", "last"])
def test_report_adds_one_gated_launch_per_bucket_and_reads_nothing_back(dev, mode):
    o, plain = _Opt(dev, skip_report=mode), _Opt(dev)
    for x in (o, plain):
        x.feed(_grads(dev, 60)); x.opt.step()
    a, b = _step_counts(dev, o, 61), _step_counts(dev, plain, 61)    # step() ran under set_sync_debug_mode("error")
    nb = len(o.opt._buckets)
    assert a.pop("spe_grad_report") == nb and a == b
    sa, sb = o.opt.state_dict(), plain.opt.state_dict()              # the report is no optimizer state
    assert sa.keys() == sb.keys() and sa["state"].keys() == sb["state"].keys()
    assert all(sa["state"][k].keys() == sb["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"} for k in sa["state"])
    assert [g.keys() for g in sa["param_groups"]] == [g.keys() for g in sb["param_groups"]]
    o.close(); plain.close()


@pytest.mark.parametrize("mode", ["first", "last"])
def test_run_with_the_report_has_the_bits_of_the_run_without(dev, mode):
    a, b = _Opt(dev, skip_report=mode, ema_decay=0.9), _Opt(dev, ema_decay=0.9)
    seq = [_grads(dev, 70), _poisoned(_grads(dev, 71), 4, 7, float("inf")), _grads(dev, 72, 10.0), _poisoned(_grads(dev, 73), 1, 0, float("nan")),
           _grads(dev, 74)]
    for grads in seq:
        for o in (a, b):
            o.feed(grads); o.opt.step()
    a.opt.grad_stats()                                               # reads only
    assert (a.opt.applied_steps(), a.opt.skipped_steps()) == (b.opt.applied_steps(), b.opt.skipped_steps()) == (3, 2)
    sa, sb = a.state(), b.state()
    assert len(sa) == len(sb) == 4 * len(a.opt._buckets) and all(_same_bits(x, y) for x, y in zip(sa, sb))
    assert torch.equal(a.opt._guard, b.opt._guard)
    a.close(); b.close()


def test_grad_stats_needs_neither_guard_nor_report(dev):
    """An unguarded optimizer: the rows follow the restatement, before the step on the raw sums and after it on the clipped gradient
    the update wrote back."""
    from spe_amd.dp import GradAllReducer
    from spe_amd.optim import FlatAdamW
    ps = _params(dev)
    red = GradAllReducer(ps, bucket_bytes=4096, flatten_params=True)
    opt = FlatAdamW(_groups(ps), red, betas=BETAS, eps=EPS, max_grad_norm=0.1)
    assert all(e["stats"] is None and e["par_tab"] is None for e in opt._buckets)
    grads = _grads(dev, 80, 10.0)
    red.reset()
    for y, gr in zip(ps, grads):
        y.grad = red._views[y]
        y.grad.copy_(gr)
    red.finish()
    order = [p for b in red.buckets for p, _ in b["offsets"]]
    rows = opt.grad_stats()
    for r, p in zip(rows, order):
        want = R.record32(red._views[p].cpu().numpy(), p.detach().cpu().numpy(), 1.0)
        assert np.float32(r["grad_sq"]) == want["grad_sq"] and np.float32(r["grad_absmax"]) == want["grad_absmax"]
        assert np.float32(r["weight_norm"] ** 2) == pytest.approx(float(want["weight_sq"]), rel=1e-6) and r["first_bad"] is None
    before = sum(r["grad_sq"] for r in rows) ** 0.5
    opt.step()
    after = sum(r["grad_sq"] for r in opt.grad_stats()) ** 0.5
    assert before > 1.0 and abs(after - 0.1) < 1e-4                  # write_clipped_grads: the buckets hold the clipped gradient now
    red.remove()


def test_constructor_refusals(dev):
    from spe_amd.dp import GradAllReducer
    from spe_amd.optim import FlatAdamW
    ps = _params(dev)
    red = GradAllReducer(ps, bucket_bytes=4096, flatten_params=True)
    with pytest.raises(ValueError, match="skip_nonfinite"):
        FlatAdamW(_groups(ps), red, skip_report="first")
    with pytest.raises(ValueError, match="skip_report"):
        FlatAdamW(_groups(ps), red, skip_nonfinite=True, skip_report="all")
    with pytest.raises(ValueError, match="skip_report"):
        FlatAdamW(_groups(ps), red, skip_nonfinite=True, skip_report=True)
    assert getattr(red, "_folded_into", None) is None                # refused before the reducer was touched
    FlatAdamW(_groups(ps), red, skip_nonfinite=True, skip_report="last")
    red.remove()
