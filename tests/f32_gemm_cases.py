"""Problems of the fp32-operand strided GEMM (spe_gemm_f32 / spe_gemm_ex, csrc/gemm.hip) and the kernel instance each must run on.

The selection is gemm_f32_select in csrc/gemm.hip, visible through kernels.gemm_plan (spe_gemm_f32_plan, host only).  This file holds data and
pure-Python arithmetic on it (no torch, no device):

  INSTANCES   the 12 instances spe_gemm_kernel<T, TA, TB, SPLIT> the library compiles, by the name a profiler prints
  PINNED      (plan arguments, expected fields or status) written out BY HAND from the rules of gemm.hip and gemm_tiles.h:
                  T = 128 iff ceil(M / 128) * ceil(N / 128) * batch0 * batch1 * splitk >= 256 and M > 64 and N > 64 ;
                  a direction is bound to XCDs from 16 panels on (the one with more rows first) and then padded to 8 panels ;
                  splitk > k-tiles is clamped (atomics) or refused with -5 (slabs) ; -3 split with an epilogue ; -2 both transposes ; -4 K <= 0
              - never regenerate it from the function under test
  GPU_CASES   the problems of tests/test_f32_gemm_gpu.py: one list of templates per tile size, run on every layout and precision
  layout()    where a case puts its operands: leading dimensions, batch strides, offsets from a 16-byte boundary (in elements)
  states()    which paths of the kernel a case reaches, computed from the plan and the shape; REQUIRED lists what every instance must see
              (tests/test_f32_gemm_plan_cpu.py demands it)
"""

BK = 32                                          # contraction elements per k-tile
LAYOUTS = {"NT": (0, 1), "NN": (0, 0), "TN": (1, 0)}          # name -> (transA, transB)
GUARD = 8                                        # NaN elements in front of every operand block (keeps 16-byte alignment for fp32 and bf16)


def instance(T, TA, TB, SPLIT):
    b = ("false", "true")
    return f"spe_gemm_kernel<{T}, {b[TA]}, {b[TB]}, {b[SPLIT]}>"


def kernel_name(plan):
    """gemm_plan's answer -> kernel name (None stays None)."""
    return None if plan is None else instance(plan["T"], plan["TA"], plan["TB"], plan["SPLIT"])


INSTANCES = [instance(T, ta, tb, s) for T in (64, 128) for (ta, tb) in LAYOUTS.values() for s in (0, 1)]


def pad4(n):
    return (n + 3) & ~3


# ---- pinned choices ---------------------------------------------------------------------------------------------------------------
# (keyword arguments of kernels.gemm_plan besides lda / ldb / ldc, which the CPU test fills in as contiguous ; expected fields, or a status)
def _p(M, N, K, **kw):
    return dict(M=M, N=N, K=K, **kw)


PINNED = [
    # tile edge: 128-tiles x batches x splits = 255 | 256, and the M > 64, N > 64 conditions
    (_p(1920, 2176, 64), dict(T=64)),                                      # 15 x 17 = 255
    (_p(2048, 2048, 64), dict(T=128)),                                     # 16 x 16 = 256
    (_p(129, 130, 40, batch0=8, batch1=8), dict(T=128)),                   # 4 x 64 = 256
    (_p(129, 130, 40, batch0=8, batch1=7), dict(T=64)),                    # 4 x 56 = 224
    (_p(128, 128, 32, batch0=16, batch1=16), dict(T=128)),                 # 1 x 256
    (_p(128, 128, 32, batch0=17, batch1=15), dict(T=64)),                  # 1 x 255
    (_p(129, 129, 2048, splitk=64), dict(T=128, splitk=64, kt_per_split=1)),          # 4 x 64: splits count
    (_p(129, 129, 2048, splitk=63), dict(T=64, splitk=63, kt_per_split=2)),           # 4 x 63 = 252 (and the last 31 splits are empty)
    (_p(129, 129, 2048, splitk=-64), dict(T=128, splitk=64, slab=129 * 129)),
    (_p(64, 4096, 64, batch0=16), dict(T=64)),                             # 32 x 16 = 512 wide tiles, but M <= 64
    (_p(65, 4096, 64, batch0=16), dict(T=128)),
    (_p(4096, 64, 64, batch0=16), dict(T=64)),                             # N <= 64: the per-head attention contractions
    (_p(4096, 65, 64, batch0=16), dict(T=128)),
    (_p(1, 4, 384), dict(T=64, xcd_bind=0, grid_x=1)),
    # tile order at T = 64: 15 | 16 | 17 panels
    (_p(960, 8, 8), dict(T=64, xcd_bind=0, grid_x=15)),
    (_p(1024, 8, 8), dict(T=64, xcd_bind=1, grid_x=16)),
    (_p(1025, 8, 8), dict(T=64, xcd_bind=1, grid_x=24)),                   # 17 panels padded to 24
    (_p(8, 960, 8), dict(T=64, xcd_bind=0, grid_x=15)),
    (_p(8, 1024, 8), dict(T=64, xcd_bind=2, grid_x=16)),
    (_p(8, 1025, 8), dict(T=64, xcd_bind=2, grid_x=24)),
    (_p(1025, 130, 8), dict(T=64, xcd_bind=1, grid_x=24 * 3)),
    (_p(1025, 1025, 8), dict(T=64, xcd_bind=1, grid_x=24 * 17)),           # M >= N: M is bound
    (_p(1025, 1089, 8), dict(T=64, xcd_bind=2, grid_x=24 * 17)),           # N > M: N is bound (18 panels -> 24)
    (_p(1100, 960, 8), dict(T=64, xcd_bind=1, grid_x=24 * 15)),
    (_p(960, 1100, 8), dict(T=64, xcd_bind=2, grid_x=24 * 15)),
    (_p(1100, 900, 8, batch0=2), dict(T=64, xcd_bind=1, grid_x=24 * 15)),  # 9 x 8 x 2 = 144 wide tiles: 18 x 15 tiles of 64, M bound
    # tile order at T = 128
    (_p(2049, 129, 8, batch0=8), dict(T=128, xcd_bind=1, grid_x=24 * 2)),  # 17 x 2 x 8 = 272 ; 17 panels padded to 24
    (_p(129, 2049, 8, batch0=8), dict(T=128, xcd_bind=2, grid_x=24 * 2)),
    (_p(2048, 129, 8, batch0=8), dict(T=128, xcd_bind=1, grid_x=16 * 2)),
    (_p(1920, 129, 8, batch0=9), dict(T=128, xcd_bind=0, grid_x=15 * 2)),  # 15 x 2 x 9 = 270, 15 panels: plain
    # split-K: the clamp, empty splits, slabs
    (_p(66, 70, 160, splitk=4), dict(splitk=4, kt_per_split=2, slab=0)),   # 5 k-tiles: 2 2 1 0
    (_p(66, 70, 160, splitk=-4, ldc=72), dict(splitk=4, kt_per_split=2, slab=66 * 72)),
    (_p(66, 70, 160, splitk=5), dict(splitk=5, kt_per_split=1)),
    (_p(66, 70, 160, splitk=6), dict(splitk=5, kt_per_split=1)),           # clamped to the 5 k-tiles
    (_p(66, 70, 160, splitk=1000), dict(splitk=5, kt_per_split=1)),
    (_p(66, 70, 160, splitk=-5), dict(splitk=5, kt_per_split=1)),
    (_p(66, 70, 160, splitk=-6), -5),                                      # more slabs than k-tiles
    (_p(66, 70, 1, splitk=-2), -5),
    (_p(66, 70, 1, splitk=2), dict(splitk=1, kt_per_split=1)),
    (_p(66, 70, 160, splitk=0), dict(splitk=1, kt_per_split=5)),
    (_p(66, 70, 160, splitk=-1), dict(splitk=1, kt_per_split=5, slab=66 * 70)),
    # the slab of a batched launch: the extent formula of kernels.gemm_splitk_into, rounded up to 4
    (_p(37, 41, 96, splitk=-3, ldc=44, batch0=2, batch1=2, sC=(4000, 1900)), dict(splitk=3, slab=(4000 + 1900 + 36 * 44 + 41 + 3) & ~3)),
    (_p(37, 41, 96, splitk=-3, ldc=44, batch0=2, batch1=1, sC=(4000, 0)), dict(splitk=3, slab=(4000 + 36 * 44 + 41 + 3) & ~3)),
    # refusals
    (_p(66, 70, 160, splitk=2, epilogue=True), -3),
    (_p(66, 70, 160, splitk=-2, epilogue=True), -3),
    (_p(66, 70, 160, splitk=1, epilogue=True), dict(splitk=1)),
    (_p(66, 70, 20, splitk=2, epilogue=True), dict(splitk=1)),             # one k-tile: clamped to no split first, so the epilogue is fine
    (_p(66, 70, 160, transA=True, transB=True), -2),
    (_p(66, 70, 0), -4),
    (_p(66, 70, -1), -4),
    (_p(66, 70, 0, transA=True, transB=True), -4),                         # K <= 0 is reported first
    # nothing to do: status 0, an all-zero plan
    (_p(0, 70, 160), dict(T=0, splitk=0, grid_x=0)),
    (_p(66, 0, 160), dict(T=0, splitk=0, grid_x=0)),
    (_p(0, 70, 0), dict(T=0, splitk=0, grid_x=0)),
    (_p(66, 70, 160, batch0=0), dict(T=0, splitk=0, grid_x=0)),
    # the vector flags: base alignment (16 bytes; 8 for a bf16 A), leading dimension and batch strides multiples of 4 (NT: lda = ldb = K)
    (_p(66, 70, 160, transB=True), dict(vecA=1, vecB=1)),
    (_p(66, 70, 160, transB=True, a_mod16=4), dict(vecA=0, vecB=1)),
    (_p(66, 70, 160, transB=True, b_mod16=8), dict(vecA=1, vecB=0)),
    (_p(66, 70, 160, transB=True, lda=161), dict(vecA=0, vecB=1)),
    (_p(66, 70, 160, transB=True, ldb=162), dict(vecA=1, vecB=0)),
    (_p(66, 70, 160, transB=True, batch0=2, sA=(66 * 160 + 2, 0), sB=(70 * 160, 0), sC=(66 * 70, 0)), dict(vecA=0, vecB=1)),
    (_p(66, 70, 160, transB=True, batch0=2, batch1=2, sA=(2 * 66 * 160, 66 * 160), sB=(2 * 70 * 160, 70 * 160 + 1), sC=(2 * 66 * 70, 66 * 70)), dict(vecA=1, vecB=0)),
    (_p(66, 70, 160, transB=True, a_bf16=True, a_mod16=8), dict(vecA=1)),
    (_p(66, 70, 160, transB=True, a_bf16=True, a_mod16=2), dict(vecA=0)),
    (_p(66, 70, 160, transB=True, a_bf16=True, a_mod16=4), dict(vecA=0)),
]


# ---- GPU cases --------------------------------------------------------------------------------------------------------------------
# A template: M, N, K and
#   b0, b1        batch counts
#   splitk        as the entry takes it: 1, n > 1 (atomics), -n (slabs)
#   a, b          operand placement: "vec" (rows 16-byte aligned and padded to 4: the vector flag is set), "ld" (leading dimension no
#                 multiple of 4), "off" (base one element behind a 16-byte boundary), "bs" (a batch stride no multiple of 4; needs batches)
#   c             "vec" | "ld" (ldc no multiple of 4) | "off" (C one float behind a 16-byte boundary) | "c2off" (only C2 is) |
#                 "sc0" (sC0 = 2 mod 4: C of the odd batches is not 16-byte aligned, that of the even ones is)
#   epi           "none" | "bias" | "relu" | "gelu" (all but "none": bias and C2 as well)
#   a16           A is stored as bf16 (spe_gemm_ex, a_bf16 = 1)
#   ops           "int" (the default exact operands) | "ties" (plain instances: 16-bit integers with exact bf16 ties) |
#                 "both10" (SPLIT instances: both operands 10-bit) | "random" (normal, bounded not exact)
#   only          0 / 1: the template runs on the plain / the SPLIT instances only
def _t(name, M, N, K, **kw):
    d = dict(name=name, M=M, N=N, K=K, b0=1, b1=1, splitk=1, a="vec", b="vec", c="vec", epi="none", a16=False, ops="int", only=None)
    assert set(kw) <= set(d), kw
    d.update(kw)
    return d


TEMPLATES = {
    64: [
        _t("m1", 1, 5, 1),
        _t("ksmall", 7, 9, 13, a="ld", b="off", c="ld"),
        _t("k32", 64, 64, 32, epi="bias"),
        _t("t+1", 65, 65, 40, c="off", epi="relu"),
        _t("k3", 70, 66, 100, b0=2, b1=3, a="bs", c="sc0"),
        _t("c2off", 33, 20, 64, b="ld", c="c2off", epi="gelu"),
        _t("gelu", 70, 66, 40, a="off", epi="gelu"),
        _t("at_empty", 66, 70, 160, splitk=4),
        _t("at_clamp", 20, 36, 40, splitk=7, c="off"),
        _t("sl_empty", 66, 70, 150, splitk=-4, c="ld"),
        _t("sl_batched", 37, 41, 96, splitk=-3, b0=2, b1=2, b="bs"),
        _t("ord_m", 1025, 8, 8),
        _t("ord_n", 8, 1025, 8),
        _t("a16_vec", 70, 66, 72, a16=True),
        _t("a16_sc", 65, 33, 40, a16=True, a="off", c="ld"),
        _t("ties", 66, 37, 60, ops="ties", only=0),
        _t("wide12", 20, 24, 1000, only=1),
        _t("both10", 40, 33, 15, ops="both10", only=1),
        _t("random", 77, 53, 200, ops="random"),
    ],
    # the same states on the 128-tile instances, which take 256 tiles: reached through batch and split counts, not size
    128: [
        _t("k1", 129, 130, 1, b0=8, b1=8),
        _t("ksmall", 129, 129, 13, b0=8, b1=8, a="ld", b="off", c="ld"),
        _t("k32", 128, 128, 32, b0=16, b1=16, epi="bias"),
        _t("t+1", 129, 130, 40, b0=8, b1=8, c="off", epi="relu"),
        _t("k3", 130, 134, 100, b0=8, b1=8, a="bs", c="sc0"),
        _t("c2off", 129, 130, 64, b0=8, b1=8, b="ld", c="c2off", epi="gelu"),
        _t("at_empty", 129, 129, 160, b0=4, b1=4, splitk=4),
        _t("at_64", 129, 129, 2048, splitk=64),
        _t("at_clamp", 129, 130, 40, b0=8, b1=8, splitk=7, b="bs", c="off"),
        _t("sl_empty", 129, 130, 150, b0=4, b1=4, splitk=-4, c="ld"),
        _t("ord_m", 2049, 129, 8, b0=8),
        _t("ord_n", 129, 2049, 8, b0=8),
        _t("a16_vec", 130, 134, 72, b0=8, b1=8, a16=True),
        _t("a16_sc", 129, 130, 40, b0=8, b1=8, a16=True, a="off", c="ld"),
        _t("ties", 130, 133, 60, b0=8, b1=8, ops="ties", only=0),
        _t("wide12", 129, 130, 520, b0=8, b1=8, only=1),
        _t("both10", 129, 130, 15, b0=8, b1=8, ops="both10", only=1),
        _t("random", 150, 131, 200, b0=8, b1=8, ops="random"),
    ],
}


def _cases():
    out = []
    for T, temps in TEMPLATES.items():
        for lay in LAYOUTS:
            for prec in (0, 1):
                for t in temps:
                    if t["only"] is not None and t["only"] != prec:
                        continue
                    c = dict(t, T=T, layout=lay, prec=prec)
                    c["id"] = f"{T}-{lay}-{'split' if prec else 'plain'}-{t['name']}"
                    c["swap"] = len(out) % 2 == 1          # the wide and the narrow operand change roles in every second case
                    out.append(c)
    return out


GPU_CASES = _cases()


def layout(c):
    """Where case c keeps its operands.  All figures in elements of the operand's type.  A is stored as [RA rows, CA contiguous] per batch
    (TA: [K, M], else [M, K]), B likewise (TB: [N, K], else [K, N]).  Rows of a "vec" operand are padded to a multiple of 4 plus 4 more NaN
    elements; every block starts GUARD elements (+ 1 for "off") into a 16-byte aligned buffer."""
    ta, tb = LAYOUTS[c["layout"]]
    M, N, K, b0, b1 = c["M"], c["N"], c["K"], c["b0"], c["b1"]
    L = {}
    for x, (R, C), mode in (("a", (K, M) if ta else (M, K), c["a"]), ("b", (N, K) if tb else (K, N), c["b"])):
        ld = pad4(C) + (5 if mode == "ld" else 4)
        s1 = R * ld + 8 + (1 if mode == "bs" else 0)
        s0 = b1 * s1 + 16
        off = GUARD + (1 if mode == "off" else 0)
        L[x] = dict(R=R, C=C, ld=ld, s0=s0, s1=s1, off=off, numel=off + (b0 - 1) * s0 + (b1 - 1) * s1 + R * ld + GUARD)
        assert mode != "bs" or b0 * b1 > 1
    ldc = pad4(N) + (5 if c["c"] == "ld" else 4)
    s1 = M * ldc + 8
    s0 = b1 * s1 + (10 if c["c"] == "sc0" else 16)
    assert c["c"] != "sc0" or b0 > 1
    L["c"] = dict(ld=ldc, s0=s0, s1=s1, off=GUARD + (1 if c["c"] == "off" else 0), off2=GUARD + (1 if c["c"] == "c2off" else 0))
    return L


def plan_args(c):
    """Keyword arguments of kernels.gemm_plan for case c, as tests/test_f32_gemm_gpu.py launches it."""
    L = layout(c)
    ta, tb = LAYOUTS[c["layout"]]
    esz = 2 if c["a16"] else 4
    return dict(M=c["M"], N=c["N"], K=c["K"], lda=L["a"]["ld"], ldb=L["b"]["ld"], ldc=L["c"]["ld"], transA=ta, transB=tb,
                batch0=c["b0"], batch1=c["b1"], sA=(L["a"]["s0"], L["a"]["s1"]), sB=(L["b"]["s0"], L["b"]["s1"]),
                sC=(L["c"]["s0"], L["c"]["s1"]), splitk=c["splitk"], precision=c["prec"], a_bf16=c["a16"], epilogue=c["epi"] != "none",
                a_mod16=(L["a"]["off"] * esz) % 16, b_mod16=(L["b"]["off"] * 4) % 16)


def kt_per_split(c, plan):
    """k-tiles of each split, as the kernel divides them."""
    ktiles, kt = -(-c["K"] // BK), plan["kt_per_split"]
    return [max(0, min(ktiles, (z + 1) * kt) - z * kt) for z in range(plan["splitk"])]


def states(c, plan):
    """The paths of spe_gemm_kernel case c reaches, from the plan and the shape (the conditions are those of the kernel source)."""
    T, M, N, K = plan["T"], c["M"], c["N"], c["K"]
    L = layout(c)
    s = set()
    nts = kt_per_split(c, plan)
    for x, rows, vec in (("A", M, plan["vecA"]), ("B", N, plan["vecB"])):
        if not vec:
            s.add(f"{x}:masked-scalar")          # rowsX_in is false without the vector flag: every tile takes the masked loader
            continue
        if rows >= T and K >= BK:
            s.add(f"{x}:interior")               # a tile fully inside and a full k-tile (every k-tile belongs to some split)
        if rows % T or K % BK:
            s.add(f"{x}:masked-vector")
    if c["a16"]:
        s.add("a16:vector" if plan["vecA"] else "a16:scalar")
    if K == 1:
        s.add("K=1")
    if K < BK and K % 4:
        s.add("K<32,K%4")
    if K == BK:
        s.add("K=32")
    if BK < K < 2 * BK and max(nts) == 2:
        s.add("K=full+ragged")
    if max(nts) >= 3:
        s.add("k-tiles>=3")
    if M == 1:
        s.add("M=1")
    if M % 4 and N % 4:
        s.add("M%4,N%4")
    for x, v in (("M", M), ("N", N)):
        if v == T:
            s.add(f"{x}=T")
        if v == T + 1:
            s.add(f"{x}=T+1")
    # stores: vst of the kernel, per batch (the slab offset is a multiple of 4 wherever ldc is: M * ldc, or the rounded extent)
    ldc4 = L["c"]["ld"] % 4 == 0
    c_al = [(L["c"]["off"] + i * L["c"]["s0"] + j * L["c"]["s1"]) % 4 == 0 for i in range(c["b0"]) for j in range(c["b1"])]
    c2_al = [(L["c"]["off2"] + i * L["c"]["s0"] + j * L["c"]["s1"]) % 4 == 0 for i in range(c["b0"]) for j in range(c["b1"])]
    has_c2 = c["epi"] != "none"
    atomic = plan["splitk"] > 1 and c["splitk"] > 0
    if not atomic:                               # the atomic path has one (scalar) form
        if not ldc4:
            s.add("store:scalar-ldc")
        elif not any(c_al):
            s.add("store:scalar-C")
        elif has_c2 and all(c_al) and not any(c2_al):
            s.add("store:scalar-C2-only")
        elif all(c_al) and N >= 4:
            s.add("store:vector")
        if ldc4 and any(c_al) and not all(c_al):
            s.add("batch:sC0-mixed-alignment")
    if c["b0"] > 1 and c["b1"] > 1:
        s.add("batch:b1>1")
    if c["splitk"] > 1:
        s.add("atomic:adds-onto-C")
        if c["splitk"] > -(-K // BK):
            s.add("atomic:clamped")
        if plan["splitk"] > 1 and nts[-1] == 0:
            s.add("atomic:empty-split")
    if c["splitk"] < -1:
        if nts[-1] == 0:
            s.add("slab:empty-split")
        if c["b0"] * c["b1"] > 1:
            s.add("slab:batched")
    tiles_m, tiles_n = -(-M // T), -(-N // T)
    if plan["xcd_bind"] == 0:
        assert plan["grid_x"] == tiles_m * tiles_n
        s.add("order:plain")
    else:
        d = "M" if plan["xcd_bind"] == 1 else "N"
        s.add(f"order:{d}-bound")
        if plan["grid_x"] > tiles_m * tiles_n:
            s.add(f"order:{d}-bound-padded")
    return s


REQUIRED = {
    "A:interior", "A:masked-vector", "A:masked-scalar", "B:interior", "B:masked-vector", "B:masked-scalar",
    "K=1", "K<32,K%4", "K=32", "K=full+ragged", "k-tiles>=3",
    "M%4,N%4", "M=T", "N=T", "M=T+1", "N=T+1",
    "store:vector", "store:scalar-ldc", "store:scalar-C", "store:scalar-C2-only",
    "batch:b1>1", "batch:sC0-mixed-alignment",
    "atomic:adds-onto-C", "atomic:clamped", "atomic:empty-split", "slab:empty-split", "slab:batched",
    "order:plain", "order:M-bound", "order:N-bound", "order:M-bound-padded", "order:N-bound-padded",
    "a16:vector", "a16:scalar",
}
REQUIRED_64_ONLY = {"M=1"}                       # a 128-tile instance needs M > 64
