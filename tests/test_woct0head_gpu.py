"""The woct0head TSCAM backbones on the GPU: the conv class head (csrc/conv_head.hip) against fp64 F.conv2d and its autograd, the head-mean
accumulation of the attention probabilities (csrc/attn_pmean.hip) against an fp64 restatement, the whole detector against the reference's own
results (tests/golden/woct0_*.pt, tools/gen_woct0_golden.py) in the benchmark and parity modes, and a bitwise-reproducible training step."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cfg_cases as cc  # noqa: E402
import test_config_golden as tcg  # noqa: E402
import woct0_cases as wc  # noqa: E402

GOLD = os.path.join(HERE, "golden")


def nrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------------------------------------ conv head
CONV_SHAPES = [(2, 192, 20, 32, 32), (2, 384, 90, 50, 83), (1, 32, 20, 4, 6), (1, 192, 20, 1, 1), (3, 64, 17, 7, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,Kc,h,w", CONV_SHAPES)
def test_conv_head_matches_fp64_conv2d(dev, B, C, Kc, h, w):
    """Exact fp32 arithmetic: map, pooled logits, dx, dW, db within 1e-5 of fp64, for a general dmap and for the pooled gradient alone;
    the weight gradients of two identical calls are bitwise equal."""
    from spe_amd import kernels as K
    g = torch.Generator().manual_seed(B * 1000 + C + Kc + h * w)
    x = torch.randn(B, h * w, C, generator=g)
    W = torch.randn(Kc, C, 3, 3, generator=g) / (9 * C) ** 0.5
    b = torch.randn(Kc, generator=g)
    dmap = torch.randn(B, Kc, h, w, generator=g)
    dlog = torch.randn(B, Kc, generator=g)
    xd, Wd, bd = (t.double().requires_grad_(True) for t in (x, W, b))
    ref_map = F.conv2d(xd.transpose(1, 2).reshape(B, C, h, w), Wd, bd, padding=1)
    ref_log = ref_map.mean((2, 3))
    m, lg = K.conv_head_fwd(x.to(dev), W.to(dev), b.to(dev), h, w)
    torch.cuda.synchronize()
    assert nrel(m, ref_map) < 1e-5 and nrel(lg, ref_log) < 1e-5, (nrel(m, ref_map), nrel(lg, ref_log))
    for gm, gl in ((dmap, None), (None, dlog), (dmap, dlog)):
        gx, gW, gb = torch.autograd.grad((ref_map * (gm.double() if gm is not None else 0)).sum()
                                         + (ref_log * (gl.double() if gl is not None else 0)).sum(), (xd, Wd, bd), retain_graph=True)
        args = (x.to(dev), W.to(dev), gm.to(dev) if gm is not None else None, gl.to(dev) if gl is not None else None, h, w)
        dx, dW, db = K.conv_head_bwd(*args)
        dx2, dW2, db2 = K.conv_head_bwd(*args)
        torch.cuda.synchronize()
        errs = (nrel(dx, gx), nrel(dW, gW), nrel(db, gb))
        print(f"[conv head {B},{C},{Kc},{h}x{w} dmap={gm is not None} dlog={gl is not None}] dx {errs[0]:.1e} dW {errs[1]:.1e} db {errs[2]:.1e}")
        assert max(errs) < 1e-5, errs
        assert torch.equal(dW, dW2) and torch.equal(db, db2) and torch.equal(dx, dx2)


# ------------------------------------------------------------------------------------------------ attention-probability accumulation
PMEAN_SHAPES = [(2, 8, 4150, 48), (1, 4, 1024, 48), (1, 4, 24, 8), (1, 4, 17, 48), (1, 8, 1000, 32)]
PMEAN_TOL = 3e-3          # max |M - M_fp64| / max |M| (the level of the fp64 attention tests: fp16 q / k fragments)


def _pmean_ref(qkv, Wl, bl, H, scale):
    """fp64 restatement: sum over the heads of softmax(proj_l(scale q k^T)) [B,N,N]."""
    B, N, C3 = qkv.shape
    dh = C3 // (3 * H)
    v5 = qkv.double().view(B, N, 3, H, dh)
    out = []
    for bi in range(B):
        q, k = v5[bi, :, 0].transpose(0, 1), v5[bi, :, 1].transpose(0, 1)          # [H, N, dh]
        S = scale * q @ k.transpose(1, 2)
        S = torch.einsum("gh,hqk->gqk", Wl.double(), S) + bl.double().view(H, 1, 1)
        out.append(S.softmax(-1).sum(0))
    return torch.stack(out)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,N,dh", PMEAN_SHAPES)
def test_attention_probability_accumulation(dev, B, H, N, dh):
    """Two accumulations with alpha = 0.5 / H (the head mean, halved) give the head mean of the probabilities: rows sum to 1, elements within
    PMEAN_TOL of the fp64 restatement; the materialised path's kernel agrees with the fused one."""
    from spe_amd import kernels as K
    from spe_amd import ops
    g = torch.Generator().manual_seed(N + 7 * H + dh)
    C = H * dh
    qkv = (torch.randn(B, N, 3 * C, generator=g) * 1.5).to(dev)
    Wl = (torch.eye(H) + 0.3 * torch.randn(H, H, generator=g)).to(dev)
    bl = (0.1 * torch.randn(H, generator=g)).to(dev)
    Ww = (torch.eye(H) + 0.3 * torch.randn(H, H, generator=g)).to(dev)
    bw = (2e-4 * torch.randn(H, generator=g)).to(dev)
    scale = dh ** -0.5
    ref = _pmean_ref(qkv, Wl, bl, H, scale) / H
    maps = {}
    with torch.no_grad():
        for fused in (True, False):
            if fused and not K.fused_supported(H, dh):
                continue
            M = torch.zeros(B, N, N, device=dev)
            for _ in range(2):
                ops.talking_heads_attention(qkv, Wl, bl, Ww, bw, H, scale, 0.0, fused=fused, acc=(M, 0.5 / H))
            torch.cuda.synchronize()
            maps[fused] = M
            Mr = ref.to(dev)
            err = float((M.double() - Mr).abs().max() / Mr.abs().max())
            rows = float((M.double().sum(-1) - 1.0).abs().max())
            print(f"[pmean {B},{H},{N},{dh} fused={fused}] max err / max|M| {err:.2e}, row-sum err {rows:.2e}")
            assert rows < 1e-3 and err < PMEAN_TOL, (err, rows)
    assert True in maps, "the fused accumulation must run at these head geometries"
    d = float((maps[True] - maps[False]).abs().max() / maps[False].abs().max())
    assert d < PMEAN_TOL, d


def test_accumulator_default_launches_nothing_new():
    """With acc = None (every existing model) the attention functions take the same arguments as before: nothing of the new kernels runs."""
    import inspect
    from spe_amd import ops
    for fn in (ops.talking_heads_attention, ops.qkv_talking_attention):
        assert inspect.signature(fn).parameters["acc"].default is None


# ------------------------------------------------------------------------------------------------ the detector against the reference
def _run(dev, case, prec):
    from spe_amd import kernels as K
    from spe_amd.util.misc import NestedTensor
    args, (model, crit, crit_r, pp, rpp), tensors, mask, targets = wc.build_case(case)
    K.set_precision(prec)
    model.to(dev).train(); crit.to(dev).eval(); crit_r.to(dev).eval()
    tg = [{k: v.to(dev) for k, v in t.items()} for t in targets]
    out = model(NestedTensor(tensors.to(dev), mask.to(dev)))
    l0 = crit(out[0], tg)
    return model, crit, crit_r, out, l0


@pytest.mark.gpu
@pytest.mark.parametrize("case,prec", [(c, p) for c in sorted(wc.CASES) for p in ("bf16s", "bf16x3")])
def test_woct0head_matches_reference(dev, case, prec):
    blob = torch.load(os.path.join(GOLD, f"woct0_{case}.pt"), weights_only=False)
    model, crit, crit_r, out, l0 = _run(dev, case, prec)
    pseudo = [{k: v.to(dev) for k, v in p.items()} for p in blob["pseudo"]]
    l1 = crit_r(out[1], pseudo)
    wd = blob["weight_dict"]
    total = sum(l0[k] * wd[k] for k in l0 if k in wd) + sum(l1[k] * wd[k] for k in l1 if k in wd)
    total.backward()
    torch.cuda.synchronize()
    oe = tcg.compare_outputs(out, blob)
    if wc.CASES[case]["variant"] == "v1":
        for st, key in ((0, "out0"), (1, "out1")):
            oe[f"{st}.cams_cls_patch"] = tcg.err_of(out[st]["cams_cls_patch"], blob[key]["cams_cls_patch"])
    else:
        assert "cams_cls_patch" not in out[0] and "cams_cls_patch" not in blob["out0"]
    le = tcg.compare_losses(l0, l1, blob, skip_logging=False)
    ne = {}
    ge = tcg.compare_grads([(k, p.grad) for k, p in model.named_parameters()], blob, ne)
    te = abs(float(total.detach()) - float(blob["total"])) / abs(float(blob["total"]))
    gs = sorted(ge.values())
    wo, wl, wn = (max(d.items(), key=lambda kv: kv[1]) for d in (oe, le, ne))
    print(f"[woct0 {case} {prec}] worst output {wo}, worst loss {wl}, total {te:.2e}, grads {len(ge)}: median {gs[len(gs) // 2]:.2e} "
          f"p90 {gs[(9 * len(gs)) // 10]:.2e} worst norm {wn}")
    to, tl, tt, tgm, tg90, tgn = tcg.TOL[prec]
    assert "backbone.0.body.conv_head.weight" in ge and "backbone.0.body.conv_head.bias" in ge
    assert wo[1] < to, wo
    assert wl[1] < tl and te < tt, (wl, te)
    assert gs[len(gs) // 2] < tgm and gs[(9 * len(gs)) // 10] < tg90 and wn[1] < tgn, (gs[len(gs) // 2], gs[(9 * len(gs)) // 10], wn)


@pytest.mark.gpu
def test_woct0head_training_step_is_bitwise_reproducible(dev):
    """Two identical v1 training steps at N = 1024 (fused attention + accumulation, conv head) give bitwise-equal gradients."""
    from spe_amd import kernels as K
    from spe_amd.util.misc import NestedTensor
    args, (model, crit, crit_r, pp, rpp), tensors, mask, targets = wc.build_case("n1024_v1")
    K.set_precision("bf16s")
    model.to(dev).train(); crit.to(dev).eval(); crit_r.to(dev).eval()
    tg = [{k: v.to(dev) for k, v in t.items()} for t in targets]
    blob = torch.load(os.path.join(GOLD, "woct0_n1024_v1.pt"), weights_only=False)
    pseudo = [{k: v.to(dev) for k, v in p.items()} for p in blob["pseudo"]]
    samples = NestedTensor(tensors.to(dev), mask.to(dev))
    grads, cams = [], []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        out = model(samples)
        l0 = crit(out[0], tg)
        l1 = crit_r(out[1], pseudo)
        wd = crit.weight_dict
        total = sum(l0[k] * wd[k] for k in l0 if k in wd) + sum(l1[k] * wd[k] for k in l1 if k in wd)
        total.backward()
        torch.cuda.synchronize()
        grads.append({n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
        cams.append(out[0]["cams_cls_patch"].detach().clone())
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 50 and "backbone.0.body.conv_head.weight" in grads[0]
    bad = [n for n in grads[0] if not torch.equal(grads[0][n], grads[1][n])]
    assert not bad, bad[:10]
    assert torch.equal(cams[0], cams[1])
