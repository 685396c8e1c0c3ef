"""The learned position embedding on the GPU: the gather and its fixed-order adjoint (csrc/pos_learned.hip) against the plain-indexing
restatement tests/pos_learned_ref.py in fp64, the whole detector against the reference's own results (tests/golden/pos_learned_*.pt,
tools/gen_pos_learned_golden.py) in the benchmark and parity modes, bitwise-reproducible training steps with and without the flat all-reduce
buckets, and the frozen / no_grad forward."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pos_learned_cases as pc  # noqa: E402
import pos_learned_ref as pr  # noqa: E402
import test_config_golden as tcg  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(HERE, "golden")
ROWS = 50

# (B, h, w, npf): smallest case; the tiny case's grid; table limit; w at the limit; h at the limit; the launch scripts' 32 x 32 grid; scalar tail
SHAPES = [(1, 1, 1, 16), (2, 4, 6, 16), (2, 50, 50, 192), (3, 7, 50, 96), (2, 50, 3, 24), (1, 32, 32, 96), (2, 5, 9, 17)]
# rows wider than one pass of the adjoint's 256 lanes (a second trip through its column loop): one-float lanes, float4 lanes
SHAPES += [(2, 3, 5, 258), (1, 2, 3, 1028)]


def nrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _tables(B, h, w, npf):
    g = torch.Generator().manual_seed(B + 10 * h + 1000 * w + 100000 * npf)
    return torch.randn(ROWS, npf, generator=g), torch.randn(ROWS, npf, generator=g), torch.randn(B, h * w, 2 * npf, generator=g)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("B,h,w,npf", SHAPES)
def test_forward_is_the_index_gather(dev, B, h, w, npf):
    from spe_amd import kernels as K
    col, row, _ = _tables(B, h, w, npf)
    out = K.pos_learned_fwd(col.to(dev), row.to(dev), B, h, w)
    torch.cuda.synchronize()
    assert out.shape == (B, h, w, 2 * npf) and out.is_contiguous()
    want = torch.cat([col[torch.arange(w)].view(1, w, npf).expand(h, w, npf), row[torch.arange(h)].view(h, 1, npf).expand(h, w, npf)], -1)
    assert torch.equal(out[0].cpu(), want)                    # a copy: bit for bit
    assert torch.equal(want, pr.forward(col, row, 1, h, w)[0])
    for b in range(1, B):
        assert torch.equal(out[b], out[0])


@pytest.mark.parametrize("B,h,w,npf", SHAPES)
def test_backward_matches_fp64_and_is_reproducible(dev, B, h, w, npf):
    """Norm-relative error < 1e-5 against the fp64 restatement (the project's bound for exact-fp32 kernels: sums of <= 50 B fp32 terms), two
    calls bitwise equal, every one of the 50 rows stored into NaN-filled destinations, a skipped table untouched."""
    from spe_amd import kernels as K
    _, _, g = _tables(B, h, w, npf)
    ref_c, ref_r = pr.adjoint(g.double(), h, w)
    gd = g.to(dev)
    nan = lambda: torch.full((ROWS, npf), float("nan"), device=dev)
    dc, dr = K.pos_learned_bwd(gd, B, h, w, npf, dcol_out=nan(), drow_out=nan())
    dc2, dr2 = K.pos_learned_bwd(gd.view(B, h, w, 2 * npf), B, h, w, npf)
    torch.cuda.synchronize()
    ec, er = nrel(dc, ref_c), nrel(dr, ref_r)
    print(f"[pos_learned bwd {B},{h},{w},{npf}] d_col {ec:.2e} d_row {er:.2e}")
    assert not bool(torch.isnan(dc).any()) and not bool(torch.isnan(dr).any())
    assert float(dc[w:].abs().sum()) == 0.0 and float(dr[h:].abs().sum()) == 0.0
    assert float(dc[:w].abs().min()) > 0.0 and float(dr[:h].abs().min()) > 0.0
    assert ec < 1e-5 and er < 1e-5, (ec, er)
    assert torch.equal(dc, dc2) and torch.equal(dr, dr2)
    # a NULL destination: the other table as before, nothing written for the skipped one
    keep_r, keep_c = nan(), nan()
    dc3, none_r = K.pos_learned_bwd(gd, B, h, w, npf, need_row=False, dcol_out=nan(), drow_out=keep_r)
    none_c, dr3 = K.pos_learned_bwd(gd, B, h, w, npf, need_col=False, dcol_out=keep_c, drow_out=nan())
    torch.cuda.synchronize()
    assert none_r is None and none_c is None
    assert torch.equal(dc3, dc) and torch.equal(dr3, dr)
    assert bool(torch.isnan(keep_r).all()) and bool(torch.isnan(keep_c).all())


def test_backward_on_a_4_byte_aligned_gradient(dev):
    """npf % 4 == 0 but the gradient starts off a 16-byte boundary: the one-float lanes run and give the same sums (another fixed order)."""
    from spe_amd import kernels as K
    B, h, w, npf = 2, 4, 6, 16
    col, row, g = _tables(B, h, w, npf)
    buf = torch.zeros(g.numel() + 4, device=dev)
    gd = buf[1:1 + g.numel()].view(g.shape)
    gd.copy_(g)
    assert gd.data_ptr() % 16 == 4 and gd.is_contiguous()
    dc, dr = K.pos_learned_bwd(gd, B, h, w, npf)
    ref_c, ref_r = pr.adjoint(g.double(), h, w)
    torch.cuda.synchronize()
    assert nrel(dc, ref_c) < 1e-5 and nrel(dr, ref_r) < 1e-5
    cbuf = torch.zeros(ROWS * npf + 4, device=dev)
    cd = cbuf[1:1 + ROWS * npf].view(ROWS, npf)
    cd.copy_(col)
    out = K.pos_learned_fwd(cd, row.to(dev), B, h, w)
    assert torch.equal(out.cpu(), pr.forward(col, row, B, h, w))


@pytest.mark.parametrize("B,h,w", [(1, 51, 4), (1, 4, 51), (2, 0, 4), (2, 4, 0), (0, 4, 4)])
def test_grid_outside_the_tables_is_refused_without_a_launch(dev, B, h, w):
    from spe_amd import kernels as K
    from spe_amd import lib
    npf = 16
    col, row = torch.randn(ROWS, npf, device=dev), torch.randn(ROWS, npf, device=dev)
    with pytest.raises(lib.SpeLibraryError, match="spe_pos_learned_fwd failed with status -2"):
        K.pos_learned_fwd(col, row, B, h, w)
    g = torch.randn(B, h * w, 2 * npf, device=dev)
    dst_c, dst_r = torch.full((ROWS, npf), 7.0, device=dev), torch.full((ROWS, npf), 7.0, device=dev)
    with pytest.raises(lib.SpeLibraryError, match="spe_pos_learned_bwd failed with status -2"):
        K.pos_learned_bwd(g, B, h, w, npf, dcol_out=dst_c, drow_out=dst_r)
    torch.cuda.synchronize()
    assert bool((dst_c == 7.0).all()) and bool((dst_r == 7.0).all())        # nothing ran


# ------------------------------------------------------------------------------------------------ the detector against the reference
def _blob(case):
    return torch.load(os.path.join(GOLD, f"pos_learned_{case}.pt"), weights_only=False)


def _setup(dev, case, prec="bf16s"):
    from spe_amd import kernels as K
    from spe_amd.util.misc import NestedTensor
    blob = _blob(case)
    args, (model, crit, crit_r, pp, rpp), tensors, mask, targets = pc.build_case(case)
    K.set_precision(prec)
    model.to(dev).train(); crit.to(dev).eval(); crit_r.to(dev).eval()           # all drop rates 0; eval criteria = no jitter
    tg = [{k: v.to(dev) for k, v in t.items()} for t in targets]
    pseudo = [{k: v.to(dev) for k, v in p.items()} for p in blob["pseudo"]]
    return blob, model, crit, crit_r, NestedTensor(tensors.to(dev), mask.to(dev)), tg, pseudo


def _total(crit, l0, l1):
    wd = crit.weight_dict
    return sum(l0[k] * wd[k] for k in l0 if k in wd) + sum(l1[k] * wd[k] for k in l1 if k in wd)


def _assert_assignment(crit, stage_out, targets, recorded, tag):
    """The device assignment the criterion consumes (matcher.match_flat: (prediction row, global target index, layer) triples in (layer, image,
    query) order) equals the reference's recorded per-call, per-image index pairs."""
    outs = [stage_out] + list(stage_out["aux_outputs"])
    logits = torch.stack([o["pred_logits"] for o in outs]).float().detach()
    boxes = torch.stack([o["pred_boxes"] for o in outs]).float().detach()
    L, B, Q, _ = logits.shape
    assert len(recorded) == L
    flat = crit.matcher.match_flat(logits, boxes, targets)
    assert flat is not None
    toff = [0]
    for t in targets:
        toff.append(toff[-1] + len(t["labels"]))
    srow, gidx, lidx = [], [], []
    for l in range(L):
        for b in range(B):
            i, j = recorded[l][b]
            o = torch.argsort(i)
            srow.append((l * B + b) * Q + i[o]); gidx.append(toff[b] + j[o]); lidx.append(torch.full_like(i, l))
    msg = f"the Hungarian assignment of criterion {tag} differs from the reference's recorded one: the case sits on a tie - pick another seed"
    assert torch.equal(flat[0].cpu(), torch.cat(srow)) and torch.equal(flat[1].cpu(), torch.cat(gidx)), msg
    assert torch.equal(flat[2].cpu().long(), torch.cat(lidx)), msg


def _memory_side_shapes_ok(model, samples):
    """ops.memory_side_kv_ok for the case's memory shape and the decoder's stacked projections, in the benchmark precision mode."""
    from spe_amd import kernels as K
    from spe_amd import ops
    dec = model.transformer.decoder
    mem_w = [m.weight for layer in dec.layers for m in (layer.ca_kcontent_proj, layer.ca_v_proj)]
    pos_w = [layer.ca_kpos_proj.weight for layer in dec.layers]
    B, _, Hi, Wi = samples.tensors.shape
    d = pos_w[0].shape[0]
    memory = torch.empty(B, (Hi // 16) * (Wi // 16), d, device=samples.tensors.device)
    prev = K.get_precision()
    K.set_precision("bf16s")
    try:
        return ops.memory_side_kv_ok(memory, mem_w, pos_w, dec.layers[0].nhead)
    finally:
        K.set_precision(prev)


@pytest.mark.parametrize("case,prec", [(c, p) for c in ("tiny", "n1024") for p in ("bf16s", "bf16x3")])
def test_learned_matches_reference(dev, case, prec):
    blob, model, crit, crit_r, samples, tg, pseudo = _setup(dev, case, prec)
    if case == "n1024":
        assert _memory_side_shapes_ok(model, samples), "n1024 must take the fp16 fragment path of the decoder's memory side"
    out = model(samples)
    _assert_assignment(crit, out[0], tg, blob["indices0"], "0")
    _assert_assignment(crit_r, out[1], pseudo, blob["indices1"], "1 (refine)")
    l0 = crit(out[0], tg)
    l1 = crit_r(out[1], pseudo)
    total = _total(crit, l0, l1)
    total.backward()
    torch.cuda.synchronize()
    oe = tcg.compare_outputs(out, blob)
    le = tcg.compare_losses(l0, l1, blob, skip_logging=False)
    ne = {}
    ge = tcg.compare_grads([(k, p.grad) for k, p in model.named_parameters()], blob, ne)
    te = abs(float(total.detach()) - float(blob["total"])) / abs(float(blob["total"]))
    gs = sorted(ge.values())
    wo, wl, wn = (max(d.items(), key=lambda kv: kv[1]) for d in (oe, le, ne))
    print(f"[pos_learned {case} {prec}] worst output {wo}, worst loss {wl}, total {te:.2e}, grads {len(ge)}: median {gs[len(gs) // 2]:.2e} "
          f"p90 {gs[(9 * len(gs)) // 10]:.2e} worst norm {wn}; tables: " + ", ".join(f"{k} sampled {ge.get(k, -1):.2e} norm {ne.get(k, -1):.2e}" for k in pc.TABLES))
    to, tl, tt, tgm, tg90, tgn = tcg.TOL[prec]
    for k in pc.TABLES:
        assert k in ge and k in ne, k
        assert ne[k] < tgn, (k, ne[k])
    assert wo[1] < to, wo
    assert wl[1] < tl and te < tt, (wl, te)
    assert gs[len(gs) // 2] < tgm and gs[(9 * len(gs)) // 10] < tg90 and wn[1] < tgn, (gs[len(gs) // 2], gs[(9 * len(gs)) // 10], wn)


def _step(model, crit, crit_r, samples, tg, pseudo):
    out = model(samples)
    total = _total(crit, crit(out[0], tg), crit_r(out[1], pseudo))
    total.backward()
    return out


def test_learned_training_step_is_bitwise_reproducible(dev):
    """Two identical n1024 training steps (flash encoder + fp16 fragment path, both feeding dpos) give bitwise-equal gradients."""
    blob, model, crit, crit_r, samples, tg, pseudo = _setup(dev, "n1024")
    grads = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        _step(model, crit, crit_r, samples, tg, pseudo)
        torch.cuda.synchronize()
        grads.append({n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 50 and all(k in grads[0] for k in pc.TABLES)
    bad = [n for n in grads[0] if not torch.equal(grads[0][n], grads[1][n])]
    assert not bad, bad[:10]


def _flat_run(dev, steps=2):
    """n1024 under GradAllReducer(flatten_params=True) + FlatAdamW (built as tests/test_grad_accum_gpu.py builds them): -> (the tables' bucket
    gradients after the first backward, the tables before the first and after the last optimizer step)."""
    from spe_amd.dp import GradAllReducer
    from spe_amd.optim import FlatAdamW
    blob, model, crit, crit_r, samples, tg, pseudo = _setup(dev, "n1024")
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    red = GradAllReducer([p for _, p in named], flatten_params=True)
    groups = [{"params": [p for n, p in named if "backbone" not in n], "lr": 1e-4},
              {"params": [p for n, p in named if "backbone" in n], "lr": 1e-5}]
    opt = FlatAdamW(groups, red, lr=1e-4, weight_decay=1e-4, max_grad_norm=0.1)
    tables = {n: p for n, p in named if n in pc.TABLES}
    assert len(tables) == 2
    before = {n: p.detach().clone() for n, p in tables.items()}
    first = None
    try:
        for s in range(steps):
            red.reset()
            _step(model, crit, crit_r, samples, tg, pseudo)
            red.finish()
            if s == 0:
                for n, p in tables.items():
                    assert p.grad is not None and p.grad.data_ptr() == red._views[p].data_ptr(), f"{n}: the gradient was not written in its bucket view"
                first = {n: red._views[p].detach().clone() for n, p in tables.items()}
            opt.step()
        torch.cuda.synchronize()
        after = {n: p.detach().clone() for n, p in tables.items()}
    finally:
        red.remove()
    return first, before, after


def test_learned_tables_in_flat_buckets(dev):
    blob, model, crit, crit_r, samples, tg, pseudo = _setup(dev, "n1024")
    _step(model, crit, crit_r, samples, tg, pseudo)
    torch.cuda.synchronize()
    plain = {n: p.grad.detach().clone() for n, p in model.named_parameters() if n in pc.TABLES}
    del model
    first, before, after = _flat_run(dev)
    first2, before2, after2 = _flat_run(dev)
    for n in pc.TABLES:
        assert torch.equal(first[n], plain[n]), f"{n}: the bucket gradient differs from plain autograd's"
        assert float(plain[n][:32].abs().min()) > 0.0 and float(plain[n][32:].abs().max()) == 0.0       # a 32 x 32 grid
        assert torch.equal(before[n], before2[n])
        assert not torch.equal(after[n][:32], before[n][:32]), f"{n} did not move in two optimizer steps"
        assert torch.equal(first2[n], first[n]) and torch.equal(after2[n], after[n]), f"{n}: not reproducible run to run"


def test_frozen_tables_and_no_grad_launch_no_backward(dev):
    from spe_amd import lib
    from spe_amd import ops
    blob, model, crit, crit_r, samples, tg, pseudo = _setup(dev, "n1024")
    pe = model.backbone[1]
    keys = ("pred_logits", "pred_boxes", "x_logits")

    def counted(fn):
        lib.count_launches(True)
        try:
            res = fn()
            torch.cuda.synchronize()
        finally:
            counts = lib.count_launches(False)
        return res, (counts.get("spe_pos_learned_fwd", 0), counts.get("spe_pos_learned_bwd", 0))

    model.zero_grad(set_to_none=True)
    out_t, n_t = counted(lambda: _step(model, crit, crit_r, samples, tg, pseudo))
    assert n_t == (1, 1)
    assert all(p.grad is not None for p in pe.parameters())
    want = {(s, k): out_t[s][k].detach().clone() for s in (0, 1) for k in keys}

    def no_grad_forward():
        with torch.no_grad():
            return model(samples)
    out_n, n_n = counted(no_grad_forward)
    assert n_n == (1, 0)
    with torch.no_grad():
        f = ops.pos_learned(pe.col_embed.weight, pe.row_embed.weight, 2, 32, 32)
    assert f.grad_fn is None and not f.requires_grad                            # nothing saved

    for p in pe.parameters():
        p.requires_grad_(False)
    f = ops.pos_learned(pe.col_embed.weight, pe.row_embed.weight, 2, 32, 32)
    assert f.grad_fn is None and not f.requires_grad
    model.zero_grad(set_to_none=True)
    out_f, n_f = counted(lambda: _step(model, crit, crit_r, samples, tg, pseudo))
    assert n_f == (1, 0)
    assert all(p.grad is None for p in pe.parameters())
    assert model.transformer.decoder.layers[0].ca_kpos_proj.weight.grad is not None
    for s in (0, 1):
        for k in keys:
            assert torch.equal(out_n[s][k], want[(s, k)]) and torch.equal(out_f[s][k], want[(s, k)]), (s, k)

    # one table frozen: only the other one is written
    pe.col_embed.weight.requires_grad_(True)
    model.zero_grad(set_to_none=True)
    _, n_h = counted(lambda: _step(model, crit, crit_r, samples, tg, pseudo))
    assert n_h == (1, 1) and pe.col_embed.weight.grad is not None and pe.row_embed.weight.grad is None
