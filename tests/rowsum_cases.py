"""The cases of tests/test_rowsum_gpu.py, each with the branch (kernel) and the members of the cross-workgroup sum it is meant to
hit, and the launchers' grid arithmetic restated from csrc/rowops.hip as it stood before it moved into one host function per launcher
(`expected`).  tests/test_rowsum_plan_cpu.py holds the library's spe_rowops_plan to both, without a GPU: a case that no longer takes its
branch, or a branch / member regime that loses its last case, fails there.  No project code is imported here.

A case is a dict: id, launcher, R, C and, where they apply,
  colsum       pad (ld = C + pad, the columns behind C hold canaries), off (the view starts `off` floats into its buffer)
  lsres_fwd    rps (rows per sample of the DropPath scale; one scale is exactly 0), 0: no scale
  lsres_bwd    rps, off (dy starts `off` floats into its buffer), prefill (dgamma holds a running sum)
  lsres_bwd16  ldt_extra (ldt = R rounded up to 64, + this), f16 (y as IEEE fp16), outs ("both", "row", "T"), p (dropout rate), rps,
               prefill, entry ("bwd16" or "bwd16d")
  act_bwd / dropout: R is the element count n
and kernel / members: what the case claims."""

REGIMES = ("1", "2-16", "17-256", ">256")
KERNELS = ("colsum_wide", "colsum_tall4", "colsum", "lsres_fwd", "lsres_bwd_rows", "lsres_bwd", "lsres_bwd16<2>", "lsres_bwd16<4>",
           "act_bwd", "dropout")


def regime(members):
    return None if members == 0 else "1" if members == 1 else "2-16" if members <= 16 else "17-256" if members <= 256 else ">256"


def ceil_div(a, b):
    return -(-a // b)


def ldt_of(c):
    return ceil_div(c["R"], 64) * 64 + c.get("ldt_extra", 0)


def aligned_of(c):
    return c.get("off", 0) % 4 == 0


def expected(c):
    """(kernel, grid_x, grid_y, members, status) from the launchers' expressions, as they were written in the launchers."""
    L, R, C = c["launcher"], c["R"], c["C"]
    if L == "colsum":
        ld = C + c.get("pad", 0)
        if C <= 0 or R <= 0:
            return (None, 0, 0, 0, 0)
        al4 = C % 4 == 0 and ld % 4 == 0 and aligned_of(c)
        if al4 and R <= 64 and C >= 4096:
            return ("colsum_wide", (C // 4 + 255) // 256, 1, 0, 0)
        if al4:
            gx = (C // 4 + 15) // 16
            ry = max(min((R + 63) // 64, (2048 + gx - 1) // gx), 1)
            return ("colsum_tall4", gx, ry, ry, 0)
        ry = max(min((R + 255) // 256, 64), 1)
        return ("colsum", (C + 63) // 64, ry, ry, 0)
    if L == "lsres_fwd":
        if R <= 0:
            return (None, 0, 0, 0, 0)
        if C & 3:
            return (None, 0, 0, 0, -2)
        return ("lsres_fwd", min((R * C // 4 + 255) // 256, 4096), 1, 0, 0)
    if L == "lsres_bwd":
        if R <= 0:
            return (None, 0, 0, 0, 0)
        if C % 4 == 0 and C <= 1024 and aligned_of(c):
            nb = min((R + 15) // 16, 128)
            return ("lsres_bwd_rows", nb, 1, nb, 0)
        ry = max(min((R + 63) // 64, 256), 1)
        return ("lsres_bwd", (C + 63) // 64, ry, ry, 0)
    if L == "lsres_bwd16":
        ldt = c["ldt"] if "ldt" in c else ldt_of(c)
        if R <= 0:
            return (None, 0, 0, 0, 0)
        if C & 3 or C > 1024 or ldt & 63 or ldt < R or not aligned_of(c):
            return (None, 0, 0, 0, -2)
        nb = min((ldt + 63) // 64, 256)
        return ("lsres_bwd16<2>" if C <= 512 else "lsres_bwd16<4>", nb, 1, nb, 0)
    if L == "act_bwd":
        if R <= 0:
            return (None, 0, 0, 0, 0)
        if R & 3:
            return (None, 0, 0, 0, -2)
        return ("act_bwd", min((R // 4 + 255) // 256, 4096), 1, 0, 0)
    if L == "dropout":
        if R <= 0:
            return (None, 0, 0, 0, 0)
        return ("dropout", min((R + 255) // 256, 8192), 1, 0, 0)
    raise KeyError(L)


def _c(launcher, R, C, kernel, members, **kw):
    d = dict(launcher=launcher, R=R, C=C, kernel=kernel, members=members, **kw)
    d["id"] = f"{launcher}-R{R}-C{C}" + "".join(f"-{k}{v}" for k, v in kw.items())
    return d


# ---- spe_colsum ------------------------------------------------------------------------------------------------------------------
COLSUM = (
    # wide: al4 && R <= 64 && C >= 4096; C = 4100: the last workgroup is partly idle
    [_c("colsum", R, C, "colsum_wide", 0) for R in (1, 64) for C in (4096, 4100)]
    + [_c("colsum", 8, 4096, "colsum_wide", 0, pad=8)]                                   # strided view, canaries behind C
    # the neighbours that must not take it
    + [_c("colsum", 65, 4096, "colsum_tall4", 2), _c("colsum", 64, 4092, "colsum_tall4", 1)]
    # tall4: column edges (one, 15, 16, 17 quads; 32 column blocks), 4 members
    + [_c("colsum", 200, C, "colsum_tall4", 4) for C in (4, 60, 64, 68, 2048)]
    # tall4: 1, 2, 16, 17 members; the looping second level (257)
    + [_c("colsum", R, 64, "colsum_tall4", m) for R, m in ((64, 1), (65, 2), (1024, 16), (1025, 17), (16448, 257))]
    # tall4: the cap (2048 / 32 column blocks = 64 row segments), then grid-stride rows
    + [_c("colsum", 4096, 2048, "colsum_tall4", 64), _c("colsum", 4160, 2048, "colsum_tall4", 64)]
    + [_c("colsum", 200, 64, "colsum_tall4", 4, pad=8)]                                  # strided view
    # generic: C % 4 != 0
    + [_c("colsum", 300, C, "colsum", 2) for C in (91, 1, 63, 65)]
    + [_c("colsum", 300, 64, "colsum", 2, off=1)]                                        # aligned shape, view one float off alignment
    + [_c("colsum", 300, 64, "colsum", 2, pad=2)]                                        # ld % 4 != 0
    + [_c("colsum", R, 91, "colsum", m) for R, m in ((1, 1), (3, 1), (256, 1), (257, 2), (4097, 17), (16640, 64))]
    + [_c("colsum", 200, 91, "colsum", 1, pad=6)]                                        # strided view
)

# ---- spe_layerscale_residual_fwd -------------------------------------------------------------------------------------------------
LSRES_FWD = (
    # R C / 4 below, at and above 256 (one workgroup / two), above 4096 * 256 (grid-stride)
    [_c("lsres_fwd", R, C, "lsres_fwd", 0) for R, C in ((255, 4), (256, 4), (257, 4), (1, 1024), (2, 1024), (4100, 1024))]
    + [_c("lsres_fwd", 150, 64, "lsres_fwd", 0, rps=50), _c("lsres_fwd", 130, 1024, "lsres_fwd", 0, rps=50)]
)

# ---- spe_layerscale_residual_bwd -------------------------------------------------------------------------------------------------
LSRES_BWD = (
    [_c("lsres_bwd", 100, C, "lsres_bwd_rows", 7) for C in (4, 252, 256, 260, 512, 1020, 1024)]
    + [_c("lsres_bwd", R, 256, "lsres_bwd_rows", m) for R, m in ((1, 1), (15, 1), (16, 1), (17, 2), (256, 16), (257, 17), (2048, 128), (2049, 128))]
    + [_c("lsres_bwd", 257, 64, "lsres_bwd_rows", 17, rps=50), _c("lsres_bwd", 100, 192, "lsres_bwd_rows", 7, rps=23, prefill=1)]
    + [_c("lsres_bwd", 100, 1028, "lsres_bwd", 2), _c("lsres_bwd", 100, 91, "lsres_bwd", 2, prefill=1),
       _c("lsres_bwd", 100, 64, "lsres_bwd", 2, off=1)]
    + [_c("lsres_bwd", R, 91, "lsres_bwd", m) for R, m in ((1, 1), (64, 1), (65, 2), (16385, 256))]
    + [_c("lsres_bwd", 150, 91, "lsres_bwd", 3, rps=50)]
)

# ---- spe_layerscale_residual_bwd16 / _bwd16d -------------------------------------------------------------------------------------
LSRES_BWD16 = (
    [_c("lsres_bwd16", 129, C, "lsres_bwd16<2>" if C <= 512 else "lsres_bwd16<4>", 3) for C in (4, 508, 512, 516, 1024)]
    + [_c("lsres_bwd16", R, 64, "lsres_bwd16<2>", m) for R, m in ((1, 1), (63, 1), (64, 1), (65, 2))]
    + [_c("lsres_bwd16", 65, 1024, "lsres_bwd16<4>", 2, f16=1)]
    # ldt beyond the rounded R: all-padding tiles
    + [_c("lsres_bwd16", R, C, k, m, ldt_extra=e) for R, C, k, m, e in ((129, 64, "lsres_bwd16<2>", 4, 64), (129, 64, "lsres_bwd16<2>", 5, 128),
                                                                        (63, 516, "lsres_bwd16<4>", 3, 128), (1, 64, "lsres_bwd16<2>", 2, 64))]
    # more than 256 tiles: several tiles per workgroup
    + [_c("lsres_bwd16", 16385, 64, "lsres_bwd16<2>", 256), _c("lsres_bwd16", 1100, 192, "lsres_bwd16<2>", 18, f16=1, prefill=1)]
    + [_c("lsres_bwd16", 129, 192, "lsres_bwd16<2>", 3, f16=f, outs=o) for f in (0, 1) for o in ("row", "T")]
    + [_c("lsres_bwd16", 129, 192, "lsres_bwd16<2>", 3, prefill=1)]
    # the dropout / DropPath entry
    + [_c("lsres_bwd16", 150, 192, "lsres_bwd16<2>", 3, entry="bwd16d", p=0.1), _c("lsres_bwd16", 150, 192, "lsres_bwd16<2>", 3, entry="bwd16d", p=0.1, rps=50),
       _c("lsres_bwd16", 150, 1024, "lsres_bwd16<4>", 3, entry="bwd16d", p=0.1, rps=50, f16=1, prefill=1),
       _c("lsres_bwd16", 150, 64, "lsres_bwd16<2>", 3, entry="bwd16d", p=0.0, rps=50),
       _c("lsres_bwd16", 150, 64, "lsres_bwd16<2>", 4, entry="bwd16d", p=0.5, ldt_extra=64, outs="T")]
)
# refusals (-2; the outputs must remain canaries): what is wrong -> the arguments
BWD16_REFUSALS = (
    dict(id="C%4", R=65, C=66), dict(id="C1028", R=65, C=1028), dict(id="ldt%64", R=65, C=64, ldt=160), dict(id="ldt<R", R=65, C=64, ldt=64),
    dict(id="misaligned", R=65, C=64, off=1), dict(id="p>=1", R=65, C=64, p=1.0), dict(id="p<0", R=65, C=64, p=-0.1),
    dict(id="rps<=0", R=65, C=64, p=0.1, rps=0),
)

# ---- spe_act_bwd / spe_dropout ---------------------------------------------------------------------------------------------------
ACT_N = (4, 1020, 1024, 1028, 4096 * 1024 + 4)          # one lane; below / at / above one workgroup; grid-stride
ACT_BWD = [_c("act_bwd", n, 0, "act_bwd", 0) for n in ACT_N]
DROPOUT_N = (1, 255, 256, 257, 8192 * 256 + 1)
DROPOUT_P = (0.0, 0.1, 0.5)
DROPOUT = [_c("dropout", n, 0, "dropout", 0) for n in DROPOUT_N]

GPU_CASES = {"colsum": COLSUM, "lsres_fwd": LSRES_FWD, "lsres_bwd": LSRES_BWD, "lsres_bwd16": LSRES_BWD16, "act_bwd": ACT_BWD, "dropout": DROPOUT}
# refused shapes of the other launchers (status -2)
REFUSED = (_c("lsres_fwd", 10, 6, None, 0), _c("lsres_fwd", 10, 1, None, 0), _c("act_bwd", 1022, 0, None, 0), _c("act_bwd", 1, 0, None, 0))

# (launcher, regime) pairs the cases must reach: every launcher with a cross-workgroup sum reaches every regime its grid cap allows
REQUIRED_REGIMES = (
    [("colsum_tall4", r) for r in REGIMES] + [("colsum", r) for r in REGIMES[:3]] + [("lsres_bwd_rows", r) for r in REGIMES[:3]]
    + [("lsres_bwd", r) for r in REGIMES[:3]] + [("lsres_bwd16<2>", r) for r in REGIMES[:3]] + [("lsres_bwd16<4>", "2-16")]
)
