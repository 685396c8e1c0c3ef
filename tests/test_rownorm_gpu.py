"""The LayerNorm and masked-softmax row kernels of csrc/rowops.hip against the fp64 restatements of tests/rownorm_ref.py, at every
dispatch edge of their launchers:

  forward   ln_fwd_hw_kernel<NV> (C = 128 NV <= 512; grid-stride loop from R > 4096, an odd last row leaves one half-wave without
            a row) and ln_fwd_kernel (every other C % 4 == 0 up to 1024), both eps values of the model;
  stores    caller-allocated outputs with canary rows behind row R - 1 (spe_layernorm_fwd, _fwd_h, _res_fwd);
  16 bit    y16, the split low part y16lo and the saturating fp16 copy, bit for bit against torch casts of the kernel's own fp32 y;
  backward  ln_bwd_kernel<MAXV = 2> (C <= 512), <MAXV = 4>, and the LS instantiation, from R = 1 over the 16-rows-per-workgroup edge to
            the grid-stride loop (R > 4096), with and without the skip gradient, onto pre-filled dgamma / dbeta (/ ls_dg / ls_db);
  refusals  C % 4, C > 1024, LS with C > 512, LS with a misaligned pointer;
  residual  norm(x + dropout(z)) with p > 0: the mask recovered from the kernel's `sum`, compared with spe_dropout's, fed to fp64;
  rows      badly conditioned rows (rownorm_ref.FAMILIES) judged element by element by the bounds of rownorm_ref.py;
  softmax   Nk from 1 (lanes without a key) over the multiples of 64 to 2100, lanes whose keys are all masked, a masked first block,
            one mask per batch entry, large scores, dropout drawn alike by forward and backward.

Well-conditioned input is held to the project's criterion rel < 1e-5 (the formula of test_kernels_gpu.rel) and, for C >= 64, to
the same figure per row (rownorm_ref.row_rel: with x = 3 randn + 1 and C >= 64, max|x| rstd stays below ~6, so even the worst-case
bound of rownorm_ref, delta = (log2 C + 8) 2^-24 max|x| rstd ~ 5e-6 per element, is below it: a correct kernel cannot miss it and
one wrong row among 8193 does; at C = 4 a row of four close values is not well conditioned and only the bound judges it).  The forward's
y, mean and rstd are always held to their per-element / per-row bounds as well.
Measured figures: profiles/rownorm_direct.txt (every line this module prints with the prefix ROWNORM)."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rownorm_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

FILL16, FILL32 = 0x5A5A, 0x5A5A5A5A      # what every canary holds (fp32 1.5e16, bf16 1.5e16, fp16 203.25: never produced here)
EPS = (1e-6, 1e-5)                        # models/cait.py and models/transformer.py
HW_C, HW_R = (128, 256, 384, 512), (1, 2, 7, 8, 9, 4095, 4097, 8193)
WAVE_C, WAVE_R = (4, 64, 192, 252, 640, 1020, 1024), (1, 3, 5, 1001)


def _filled(shape, dtype, dev):
    if dtype == torch.float32:
        return torch.full(shape, FILL32, dtype=torch.int32, device=dev).view(torch.float32)
    return torch.full(shape, FILL16, dtype=torch.int16, device=dev).view(dtype)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _untouched(t):
    return bool((_bits(t) == (FILL32 if t.dtype == torch.float32 else FILL16)).all())


def _plain(R, C, dev, seed, n_rc=1, n_c=2):
    """x = 3 randn + 1 (the input of test_layernorm) and further randn tensors: n_rc - 1 of [R,C], n_c of [C]."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(R, C, generator=g) * 3 + 1).to(dev)
    return [x] + [torch.randn(R, C, generator=g).to(dev) for _ in range(n_rc - 1)] + [torch.randn(C, generator=g).to(dev) for _ in range(n_c)]


def _finite(*ts):
    return all(bool(torch.isfinite(t.float()).all()) for t in ts if t is not None)


# ------------------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------------------
def _check_fwd(x, gamma, beta, eps, y, mean, rstd, tag):
    yr, mr, rsr = rr.ln_fwd(x, gamma, beta, eps)
    fb = rr.ln_fwd_bounds(x, gamma, beta, eps)
    figs = {"rel": rr.rel(y, yr), "row": rr.row_rel(y, yr), "y/bound": rr.worst_ratio(y.double() - yr, fb["y"]),
            "mean/bound": rr.worst_ratio(mean.double() - mr, fb["mean"]), "rstd/bound": rr.worst_ratio((rstd.double() - rsr) / rsr, fb["rstd_rel"])}
    print("ROWNORM fwd", tag, f"eps {eps:g}", " ".join(f"{k} {v:.3e}" for k, v in figs.items()))
    assert _finite(y, mean, rstd), tag
    assert figs["rel"] < 1e-5 and (figs["row"] < 1e-5 or x.shape[1] < 64), (tag, figs)
    assert figs["y/bound"] <= 1.0 and figs["mean/bound"] <= 1.0 and figs["rstd/bound"] <= 1.0, (tag, figs)


@pytest.mark.parametrize("R", HW_R)
@pytest.mark.parametrize("C", HW_C)
def test_forward_half_wave(dev, C, R):
    from spe_amd import kernels as K
    x, gamma, beta = _plain(R, C, dev, 1031 * R + C)
    for eps in EPS:
        _check_fwd(x, gamma, beta, eps, *K.layernorm_fwd(x, gamma, beta, eps), f"hw C{C} R{R}")


@pytest.mark.parametrize("R", WAVE_R)
@pytest.mark.parametrize("C", WAVE_C)
def test_forward_wave_per_row(dev, C, R):
    from spe_amd import kernels as K
    x, gamma, beta = _plain(R, C, dev, 1031 * R + C)
    for eps in EPS:
        _check_fwd(x, gamma, beta, eps, *K.layernorm_fwd(x, gamma, beta, eps), f"wave C{C} R{R}")


@pytest.mark.parametrize("R", [1, 9, 4097])
@pytest.mark.parametrize("C", [128, 256, 384, 512, 192, 1024])
def test_forward_stores_its_rows_only(dev, C, R):
    """Outputs allocated here with canary rows behind row R - 1: the canaries keep their bit pattern and the R rows are, bit for bit,
    what the wrapper's own launch gives (so every one of them was written)."""
    from spe_amd import kernels as K
    x, z, gamma, beta = _plain(R, C, dev, 77 * R + C, n_rc=2)
    pad, eps = 5, 1e-6
    p = lambda t: None if t is None else t.data_ptr()
    K.set_precision("bf16s")
    want = {"spe_layernorm_fwd": K.layernorm_fwd(x, gamma, beta, eps, want16=True),
            "spe_layernorm_fwd_h": K.layernorm_fwd(x, gamma, beta, eps, want16=True, f16=True)}
    assert want["spe_layernorm_fwd"][4].dtype == torch.bfloat16 and want["spe_layernorm_fwd_h"][4].dtype == torch.float16
    for name, ref in want.items():
        for with16 in (True, False):
            y, mean, rstd = _filled((R + pad, C), torch.float32, dev), _filled((R + pad,), torch.float32, dev), _filled((R + pad,), torch.float32, dev)
            y16 = _filled((R + pad, C), torch.bfloat16, dev)
            y16lo = _filled((R + pad, C), ref[4].dtype, dev)
            K.lib.call(name, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), R, C, eps,
                       p(y16 if with16 else None), p(y16lo if with16 else None), K._st())
            outs = (y, mean, rstd, y16, y16lo)
            for i, (o, r) in enumerate(zip(outs, ref)):
                assert _untouched(o[R:]), (name, with16, i, "stored behind row R - 1")
                if i < 3 or with16:
                    assert torch.equal(_bits(o[:R]), _bits(r)), (name, with16, i)
                else:
                    assert _untouched(o), (name, i, "16-bit copy written although no buffer was passed for it")
    for pd in (0.0, 0.1):
        ref = K.layernorm_res_fwd(x, z, gamma, beta, eps, pd, 11, 3)             # (y, sum, mean, rstd)
        y, sm = _filled((R + pad, C), torch.float32, dev), _filled((R + pad, C), torch.float32, dev)
        mean, rstd = _filled((R + pad,), torch.float32, dev), _filled((R + pad,), torch.float32, dev)
        K.lib.call("spe_layernorm_res_fwd", x.data_ptr(), z.data_ptr(), gamma.data_ptr(), beta.data_ptr(), sm.data_ptr(), y.data_ptr(),
                   mean.data_ptr(), rstd.data_ptr(), R, C, eps, pd, 11, 3, K._st())
        for i, (o, r) in enumerate(zip((y, sm, mean, rstd), ref)):
            assert _untouched(o[R:]), ("spe_layernorm_res_fwd", pd, i, "stored behind row R - 1")
            assert torch.equal(_bits(o[:R]), _bits(r)), ("spe_layernorm_res_fwd", pd, i)


@pytest.mark.parametrize("R", [9, 4097])
@pytest.mark.parametrize("C", [192, 256, 384, 1024])
def test_forward_16bit_copies_bit_exact(dev, C, R):
    """y16 = bf16(y); bf16s: y16lo = bf16(y - y16), or with f16 the fp16 copy of y saturated at +-65504; bf16: no second copy.  The
    casts are torch's on the CPU, of the kernel's own fp32 y; the second round scales gamma so that |y| passes 65504."""
    from spe_amd import kernels as K
    x, gamma, beta = _plain(R, C, dev, 13 * R + C)
    for scale in (1.0, 3.0e4):
        gs = gamma * scale
        K.set_precision("bf16s")
        y, _, _, y16, y16lo = K.layernorm_fwd(x, gs, beta, 1e-6, want16=True)
        yc = y.cpu()
        hi = yc.to(torch.bfloat16)
        assert torch.equal(_bits(y16.cpu()), _bits(hi)), (scale, "y16")
        assert y16lo.dtype == torch.bfloat16 and torch.equal(_bits(y16lo.cpu()), _bits((yc - hi.float()).to(torch.bfloat16))), (scale, "y16lo")
        y2, _, _, y16b, yh = K.layernorm_fwd(x, gs, beta, 1e-6, want16=True, f16=True)
        assert torch.equal(_bits(y2), _bits(y)) and torch.equal(_bits(y16b), _bits(y16))
        assert yh.dtype == torch.float16 and torch.equal(_bits(yh.cpu()), _bits(yc.clamp(-65504, 65504).to(torch.float16))), (scale, "fp16 copy")
        if scale > 1:
            assert float(yc.abs().max()) > 65504 and float(yh.float().abs().max()) == 65504.0
        K.set_precision("bf16")
        y3, _, _, y16c, none = K.layernorm_fwd(x, gs, beta, 1e-6, want16=True, f16=True)
        assert none is None and torch.equal(_bits(y3), _bits(y)) and torch.equal(_bits(y16c), _bits(y16))


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("R,C", [(1, 4), (5, 192), (3, 1020), (1001, 1024)])
def test_res_forward_is_plain_forward_of_its_sum(dev, R, C, p):
    """norm(x + dropout(z)) runs the row body of the plain forward: y, mean and rstd are, bit for bit, what spe_layernorm_fwd makes
    of the kernel's own `sum`, and without dropout `sum` is torch's fp32 x + z.  Wave-per-row widths only (C = 1024 is a multiple of
    128 but above 512): a width the plain forward hands to the half-wave kernel is reduced by another tree there."""
    from spe_amd import kernels as K
    x, z, gamma, beta = _plain(R, C, dev, 41 * R + C, n_rc=2)
    eps = 1e-5
    y, sm, mean, rstd = K.layernorm_res_fwd(x, z, gamma, beta, eps, p, 29, 5)
    if p == 0:
        assert torch.equal(_bits(sm), _bits(x + z))
    for name, got, want in zip(("y", "mean", "rstd"), (y, mean, rstd), K.layernorm_fwd(sm, gamma, beta, eps)):
        assert torch.equal(_bits(got), _bits(want)), (name, R, C, p)


# ------------------------------------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------------------------------------
BWD_C, BWD_R = (64, 128, 256, 384, 512, 516, 1024), (1, 15, 16, 17, 4096, 4097, 8200)
BWD_CASES = sorted({(C, R) for C in BWD_C for R in (17, 4097)} | {(C, R) for C in (256, 1024) for R in BWD_R})


def _check_cols(name, got, pre, ref, bound, figs):
    """An accumulate-into column sum: got = pre-fill + sum, to rel < 1e-5 and, per element, to the bound of the sum plus the
    round-off of the final addition."""
    want = pre.double() + ref
    figs[name] = rr.rel(got, want)
    figs[name + "/bound"] = rr.worst_ratio(got.double() - want, bound + 2 * rr.U * want.abs())


@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("C,R", BWD_CASES)
def test_backward_plain(dev, C, R, add):
    from spe_amd import kernels as K
    x, dy, addt, gamma, beta, pre_g, pre_b = _plain(R, C, dev, 517 * R + C, n_rc=3, n_c=4)
    addt = addt if add else None
    eps = EPS[int(add)]
    _, mean, rstd = K.layernorm_fwd(x, gamma, beta, eps)
    dg_out, db_out = pre_g.clone(), pre_b.clone()
    dx, dg, db = K.layernorm_bwd(dy, x, gamma, mean, rstd, dg_out=dg_out, db_out=db_out, add=addt)
    assert dg.data_ptr() == dg_out.data_ptr() and db.data_ptr() == db_out.data_ptr()
    dxr, dgr, dbr, _ = rr.ln_bwd(dy, x, gamma, eps, add=addt)
    bb = rr.ln_bwd_bounds(dy, x, gamma, eps, add=addt)
    figs = {"dx": rr.rel(dx, dxr), "dx row": rr.row_rel(dx, dxr), "dx/bound": rr.worst_ratio(dx.double() - dxr, bb["dx"])}
    _check_cols("dgamma", dg, pre_g, dgr, bb["dgamma"], figs)
    _check_cols("dbeta", db, pre_b, dbr, bb["dbeta"], figs)
    print("ROWNORM bwd", f"C{C} R{R} add{int(add)}", " ".join(f"{k} {v:.3e}" for k, v in figs.items()))
    assert _finite(dx, dg, db)
    for k, v in figs.items():
        assert v <= 1.0 if k.endswith("/bound") else v < 1e-5, (k, figs)


def _ls_inputs(R, C, dev, seed):
    g = torch.Generator().manual_seed(seed)
    ls_y = torch.randn(R, C, generator=g).to(dev)
    ls_gamma = (torch.rand(C, generator=g) + 0.5).to(dev) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0).to(dev)
    return ls_y, ls_gamma, torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev)


def _check_ls(K, x, dy, gamma, beta, eps, addt, ls_y, ls_gamma, pre, tag, well):
    """spe_layernorm_bwd_ls against fp64.  well: also the norm criteria rel < 1e-5; always the per-element bounds."""
    pre_g, pre_b, pre_ldb, pre_ldg = pre
    _, mean, rstd = K.layernorm_fwd(x, gamma, beta, eps)
    outs = [t.clone() for t in pre]
    dx, dg, db, (dy16, ldb, ldg) = K.layernorm_bwd(dy, x, gamma, mean, rstd, dg_out=outs[0], db_out=outs[1], add=addt,
                                                   ls=(ls_y, ls_gamma, outs[2], outs[3]))
    assert [t.data_ptr() for t in (dg, db, ldb, ldg)] == [t.data_ptr() for t in outs] and dy16.dtype == torch.bfloat16
    dxr, dgr, dbr, _ = rr.ln_bwd(dy, x, gamma, eps, add=addt)
    dy16r, ldbr, ldgr = rr.ls_ride(dxr, ls_y, ls_gamma)
    bb = rr.ln_bwd_bounds(dy, x, gamma, eps, add=addt)
    lb = rr.ls_ride_bounds(dxr, bb["dx"], ls_y, ls_gamma)
    figs = {"dx": rr.rel(dx, dxr), "dx row": rr.row_rel(dx, dxr), "dx/bound": rr.worst_ratio(dx.double() - dxr, bb["dx"]),
            "dy16/bound": rr.worst_ratio(dy16.double() - dy16r, lb["dy16"])}
    _check_cols("dgamma", dg, pre_g, dgr, bb["dgamma"], figs)
    _check_cols("dbeta", db, pre_b, dbr, bb["dbeta"], figs)
    _check_cols("ls_dg", ldg, pre_ldg, ldgr, lb["ls_dg"], figs)
    _check_cols("ls_db", ldb, pre_ldb, ldbr, lb["ls_db"], figs)
    print("ROWNORM bwd_ls", tag, " ".join(f"{k} {v:.3e}" for k, v in figs.items()))
    assert _finite(dx, dg, db, dy16, ldb, ldg), tag
    for k, v in figs.items():
        if k.endswith("/bound"):
            assert v <= 1.0, (tag, k, figs)
        elif well:
            assert v < 1e-5, (tag, k, figs)
    return figs


@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("R", [17, 2200, 4097])
@pytest.mark.parametrize("C", [128, 256, 384, 512])
def test_backward_ls(dev, C, R, add):
    from spe_amd import kernels as K
    x, dy, addt, gamma, beta, pre_g, pre_b = _plain(R, C, dev, 311 * R + C, n_rc=3, n_c=4)
    ls_y, ls_gamma, pre_ldb, pre_ldg = _ls_inputs(R, C, dev, R + C)
    _check_ls(K, x, dy, gamma, beta, EPS[int(add)], addt if add else None, ls_y, ls_gamma, (pre_g, pre_b, pre_ldb, pre_ldg),
              f"C{C} R{R} add{int(add)}", well=True)


def test_refusals(dev):
    from spe_amd import kernels as K
    from spe_amd.lib import SpeLibraryError
    R = 8
    for C in (6, 1028):
        x, dy, z, gamma, beta = _plain(R, C, dev, C, n_rc=3)
        mean, rstd = torch.zeros(R, device=dev), torch.ones(R, device=dev)
        with pytest.raises(SpeLibraryError):
            K.layernorm_fwd(x, gamma, beta, 1e-6)
        with pytest.raises(SpeLibraryError):
            K.layernorm_fwd(x, gamma, beta, 1e-6, want16=True)
        with pytest.raises(SpeLibraryError):
            K.layernorm_res_fwd(x, z, gamma, beta, 1e-5, 0.1, 1, 1)
        with pytest.raises(SpeLibraryError):
            K.layernorm_bwd(dy, x, gamma, mean, rstd)
        with pytest.raises(SpeLibraryError):
            K.layernorm_res_bwd(dy, x, gamma, mean, rstd, 0.1, 1, 1)
    for C, misalign in ((516, False), (256, True)):
        x, dy, gamma, beta = _plain(R, C, dev, C, n_rc=2)
        ls_y, ls_gamma, _, _ = _ls_inputs(R, C, dev, C)
        _, mean, rstd = K.layernorm_fwd(x, gamma, beta, 1e-6)
        if misalign:                    # ls_y one float behind a 16-byte boundary
            buf = torch.zeros(R * C + 4, device=dev)
            assert buf.data_ptr() % 16 == 0
            ls_y = buf[1:1 + R * C].view(R, C).copy_(ls_y)
            assert ls_y.data_ptr() % 16 == 4 and ls_y.is_contiguous()
        with pytest.raises(SpeLibraryError):
            K.layernorm_bwd(dy, x, gamma, mean, rstd, ls=(ls_y, ls_gamma, None, None))
        if misalign:                    # the same call is taken once the pointer is aligned
            K.layernorm_bwd(dy, x, gamma, mean, rstd, ls=(ls_y.clone(), ls_gamma, None, None))


# ------------------------------------------------------------------------------------------------------------------------------
# norm(x + dropout(z)), p > 0
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dyb", [False, True])
@pytest.mark.parametrize("R", [77, 4097])
@pytest.mark.parametrize("C", [64, 256, 1024])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_residual_dropout_norm(dev, p, C, R, dyb):
    """|z| in [1, 2) and |x| < 1/8: the kept elements of sum = x + z k have |sum| <= 1.07 |z k|, so (sum - x) / z in fp64 is k up to
    the two fp32 roundings of the kernel (z k, then the sum: <= 2.1 u relative) - inside 2 ulp of k = 1 / (1 - p), whose ulp is
    >= 1.8 u relative; a dropped element has sum == x exactly."""
    from spe_amd import kernels as K
    g = torch.Generator().manual_seed(97 * R + C)
    x = ((torch.rand(R, C, generator=g) - 0.5) * 0.25).to(dev)
    z = ((1 + torch.rand(R, C, generator=g)) * torch.where(torch.rand(R, C, generator=g) < 0.5, -1.0, 1.0)).to(dev)
    gamma, beta = torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev)
    dy, dy2 = torch.randn(R, C, generator=g).to(dev), (torch.randn(R, C, generator=g).to(dev) if dyb else None)
    seed, offset, eps = 0x1234567 + C, R, 1e-5
    y, sm, mean, rstd = K.layernorm_res_fwd(x, z, gamma, beta, eps, p, seed, offset)
    krec = (sm.double() - x.double()) / z.double()
    kept = krec != 0
    k32 = (1.0 / (1.0 - torch.tensor(p, dtype=torch.float32))).item()              # fp32 arithmetic, as in the kernel
    ulp = 2.0 ** (math.floor(math.log2(k32)) - 23)
    assert float((krec[kept] - k32).abs().max()) <= 2 * ulp
    share = kept.double().mean().item()
    assert abs(share - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / (R * C)), share
    drawn = K.dropout(torch.ones(R, C, device=dev), p, seed, offset)
    assert torch.equal(drawn != 0, kept), "spe_layernorm_res_fwd and spe_dropout drew different masks"
    assert float((drawn[kept].double() - k32).abs().max()) <= 2 * ulp
    keep = kept.double() / (1.0 - p)
    s = x.double() + z.double() * keep
    yr, mr, rsr = rr.ln_fwd(s, gamma, beta, eps)
    fb = rr.ln_fwd_bounds(s, gamma, beta, eps)
    ds, dz, dg, db = K.layernorm_res_bwd(dy, sm, gamma, mean, rstd, p, seed, offset, dy_b=dy2)
    dsr, dgr, dbr, dzr = rr.ln_bwd(dy, s, gamma, eps, dy2=dy2, keep=keep)
    figs = {"sum": rr.rel(sm, s), "y": rr.rel(y, yr), "y row": rr.row_rel(y, yr), "ds": rr.rel(ds, dsr), "ds row": rr.row_rel(ds, dsr),
            "dz": rr.rel(dz, dzr), "dz row": rr.row_rel(dz, dzr), "dgamma": rr.rel(dg, dgr), "dbeta": rr.rel(db, dbr)}
    print("ROWNORM res", f"p{p} C{C} R{R} dyb{int(dyb)}", " ".join(f"{k} {v:.3e}" for k, v in figs.items()))
    assert _finite(y, sm, mean, rstd, ds, dz, dg, db)
    assert rr.worst_ratio(mean.double() - mr, fb["mean"]) <= 1.0 and rr.worst_ratio((rstd.double() - rsr) / rsr, fb["rstd_rel"]) <= 1.0
    assert bool((dz[~kept] == 0).all()) and dz.data_ptr() != ds.data_ptr()
    for k, v in figs.items():
        assert v < 1e-5, (k, figs)


# ------------------------------------------------------------------------------------------------------------------------------
# badly conditioned rows
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [256, 384, 1024])
@pytest.mark.parametrize("fam", rr.FAMILIES)
def test_conditioning(dev, fam, C):
    """Forward, backward and (C <= 512) LS backward on rows with a large common offset, zero variance, variance far below eps, one
    outlier: every element inside the bounds of rownorm_ref.py (no norm ratio: it hides single rows), nothing NaN or Inf."""
    from spe_amd import kernels as K
    R = 64
    g = torch.Generator().manual_seed(C + len(fam))
    x = rr.family(fam, R, C, g).to(dev)
    gamma, beta, pre_g, pre_b = (torch.randn(C, generator=g).to(dev) for _ in range(4))
    dy = torch.randn(R, C, generator=g).to(dev)
    ls_y, ls_gamma, pre_ldb, pre_ldg = _ls_inputs(R, C, dev, C)
    for eps in EPS:
        y, mean, rstd = K.layernorm_fwd(x, gamma, beta, eps)
        yr, mr, rsr = rr.ln_fwd(x, gamma, beta, eps)
        fb = rr.ln_fwd_bounds(x, gamma, beta, eps)
        dg_out, db_out = pre_g.clone(), pre_b.clone()
        dx, dg, db = K.layernorm_bwd(dy, x, gamma, mean, rstd, dg_out=dg_out, db_out=db_out)
        dxr, dgr, dbr, _ = rr.ln_bwd(dy, x, gamma, eps)
        bb = rr.ln_bwd_bounds(dy, x, gamma, eps)
        figs = {"y": rr.worst_ratio(y.double() - yr, fb["y"]), "mean": rr.worst_ratio(mean.double() - mr, fb["mean"]),
                "rstd": rr.worst_ratio((rstd.double() - rsr) / rsr, fb["rstd_rel"]), "dx": rr.worst_ratio(dx.double() - dxr, bb["dx"])}
        _check_cols("dgamma", dg, pre_g, dgr, bb["dgamma"], figs)
        _check_cols("dbeta", db, pre_b, dbr, bb["dbeta"], figs)
        figs = {k: v for k, v in figs.items() if k not in ("dgamma", "dbeta")}            # (the norm ratios: not used here)
        print("ROWNORM cond", fam, f"C{C} eps {eps:g}", " ".join(f"{k.replace('/bound', '')} {v:.3f}" for k, v in figs.items()))
        assert _finite(y, mean, rstd, dx, dg, db), (fam, C, eps)
        for k, v in figs.items():
            assert v <= 1.0, (fam, C, eps, k, figs)
        if C <= 512:
            _check_ls(K, x, dy, gamma, beta, eps, None, ls_y, ls_gamma, (pre_g, pre_b, pre_ldb, pre_ldg), f"cond {fam} C{C} eps {eps:g}",
                      well=False)


# ------------------------------------------------------------------------------------------------------------------------------
# masked softmax
# ------------------------------------------------------------------------------------------------------------------------------
SM_NK = (1, 20, 63, 64, 65, 128, 300, 2100)
SM_B, SM_H, SM_NQ = 3, 2, 5
PAD = 7.25                                  # what the padding columns Nk..ld hold


def _sm_mask(kind, Nk):
    """-> [B, Nk] bool or None; never a whole row.  None where Nk does not allow the kind."""
    m = torch.zeros(SM_B, Nk, dtype=torch.bool)
    if kind == "none":
        return m, False
    if kind == "tail" and Nk >= 2:
        m[:, Nk - max(1, Nk // 3):] = True
    elif kind == "lane5" and Nk >= 7:           # lane 5 of the wave sees keys 5, 69, ...: all of them masked
        m[:, 5::64] = True
    elif kind == "head64" and Nk > 64:          # every lane's first key is masked: its running maximum starts at -inf
        m[:, :64] = True
    elif kind == "perbatch" and Nk >= 2:        # rows of batch entry b must read mask row b
        m[1, Nk // 2:] = True
        m[2, 1::3] = True
    else:
        return None, False
    assert not m.all(1).any()
    return m, True


SM_CASES = [(Nk, kind, 4.0) for Nk in SM_NK for kind in ("none", "tail", "lane5", "head64", "perbatch") if _sm_mask(kind, Nk)[0] is not None]
SM_CASES.append((300, "lane5", 80.0))


def _sm_buffers(Nk, scale, dev, seed):
    from spe_amd import kernels as K
    g = torch.Generator().manual_seed(seed)
    ld = K.pad4(Nk)
    S = torch.full((SM_B, SM_H, SM_NQ, ld), PAD)
    S[..., :Nk] = torch.randn(SM_B, SM_H, SM_NQ, Nk, generator=g) * scale
    go = torch.full((SM_B, SM_H, SM_NQ, ld), PAD)
    go[..., :Nk] = torch.randn(SM_B, SM_H, SM_NQ, Nk, generator=g)
    return S.to(dev), go.to(dev), ld


@pytest.mark.parametrize("Nk,kind,scale", SM_CASES)
def test_softmax_masks_and_sizes(dev, Nk, kind, scale):
    from spe_amd import kernels as K
    S, go, ld = _sm_buffers(Nk, scale, dev, 7 * Nk + len(kind))
    mask, masked = _sm_mask(kind, Nk)
    mask = mask.to(dev)
    mk = mask[:, None, None, :].expand(SM_B, SM_H, SM_NQ, Nk)
    Pr = rr.softmax_fwd(S[..., :Nk], mask if masked else None)
    P, Pd = K.softmax_fwd(S.clone(), mask.to(torch.uint8) if masked else None, SM_B, SM_H, SM_NQ, Nk, ld, 0.0, 0, 0)
    dS = K.softmax_bwd(go.clone(), P, SM_B, SM_H, SM_NQ, Nk, ld, 0.0, 0, 0)
    dSr = rr.softmax_bwd(go[..., :Nk], Pr)
    figs = {"P": rr.rel(P[..., :Nk], Pr), "dS": rr.rel(dS[..., :Nk], dSr), "rowsum": float((P[..., :Nk].double().sum(-1) - 1).abs().max())}
    print("ROWNORM softmax", f"Nk{Nk} {kind} scale{scale:g}", " ".join(f"{k} {v:.3e}" for k, v in figs.items()))
    assert Pd is None and _finite(P[..., :Nk], dS[..., :Nk])
    assert bool((P[..., :Nk][mk] == 0).all()) and bool((dS[..., :Nk][mk] == 0).all()), "a masked key got probability or gradient"
    assert torch.equal(_bits(P[..., Nk:]), _bits(S[..., Nk:])) and torch.equal(_bits(dS[..., Nk:]), _bits(go[..., Nk:])), "padding columns written"
    assert figs["P"] < 1e-5 and figs["dS"] < 1e-5 and figs["rowsum"] < 1e-5, figs


@pytest.mark.parametrize("Nk", [20, 300])
def test_softmax_dropout_same_mask_both_ways(dev, Nk):
    from spe_amd import kernels as K
    p, seed, offset = 0.25, 4321, 9
    S, go, ld = _sm_buffers(Nk, 4.0, dev, Nk)
    mask, _ = _sm_mask("tail", Nk)
    mask = mask.to(dev)
    live = ~mask[:, None, None, :].expand(SM_B, SM_H, SM_NQ, Nk)
    P0, _ = K.softmax_fwd(S.clone(), mask.to(torch.uint8), SM_B, SM_H, SM_NQ, Nk, ld, 0.0, 0, 0)
    P, Pd = K.softmax_fwd(S.clone(), mask.to(torch.uint8), SM_B, SM_H, SM_NQ, Nk, ld, p, seed, offset)
    assert torch.equal(_bits(P), _bits(P0)) and bool((P[..., :Nk][live] > 0).all())
    assert bool((Pd[..., :Nk][~live] == 0).all())
    ratio = Pd[..., :Nk].double()[live] / P[..., :Nk].double()[live]
    kept = ratio != 0
    assert float((ratio[kept] * (1 - p) - 1).abs().max()) < 4 * rr.U            # Pd = fl(P fl(1 / (1 - p)))
    assert abs(kept.double().mean().item() - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / kept.numel())
    keep = torch.zeros(SM_B, SM_H, SM_NQ, Nk, dtype=torch.float64, device=dev)
    keep[live] = kept.double() / (1 - p)
    Pr = rr.softmax_fwd(S[..., :Nk], mask)
    dS = K.softmax_bwd(go.clone(), P, SM_B, SM_H, SM_NQ, Nk, ld, p, seed, offset)
    figs = {"Pd": rr.rel(Pd[..., :Nk], Pr * keep), "dS": rr.rel(dS[..., :Nk], rr.softmax_bwd(go[..., :Nk], Pr, keep))}
    print("ROWNORM softmax-dropout", f"Nk{Nk}", " ".join(f"{k} {v:.3e}" for k, v in figs.items()))
    assert figs["Pd"] < 1e-5 and figs["dS"] < 1e-5, figs          # dS: only with the forward's mask
    assert torch.equal(_bits(dS[..., Nk:]), _bits(go[..., Nk:]))
