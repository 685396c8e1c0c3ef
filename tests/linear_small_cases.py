"""Shapes of the small-row Linear kernels (csrc/linear_small.hip: spe_linear_small_fwd / _bwd / _group_fwd / _group_bwd), the kernel
instance each must run on and the edges ("states") each reaches.  Data and plain arithmetic only: nothing here calls the library.

The launch choices are ls_plan in csrc/linear_small.hip, visible through kernels.linear_small_plan (spe_linear_small_plan, host only):
    forward        tiles = ceil(R / 32) * ceil(N / 32)   (group: ceil(R / 32) * nblk * N / 32) ;  tiles <= 320 -> KC 384, else KC 128
    backward       tiles_dx = dx ? ceil(R / 32) * ceil(K / 32) : 0 ;  tiles_dw = dW ? ceil(N / 32) * ceil(K / 32) : db ? ceil(N / 32) : 0
                   tiles_dx + tiles_dw <= 320 -> <384, 512>, else <128, 256>
    group backward tiles_dw = (some output has a dy and a dW or db) ? nblk * N / 32 * ceil(K / 32) : 0 ;  <384, 512> only when N % 384 == 0 too

  INSTANCES   the six kernel instances, by the name a profiler prints
  PINNED      (entry, problem, instance, tiles_dx, tiles_dw) written out BY HAND from the launchers as they stood before the choice became
              one function - never regenerate it from the plan
  FWD_CASES, BWD_CASES, GROUP_FWD_CASES, GROUP_BWD_CASES (GPU_CASES: the four lists by entry)
              the problems of tests/test_linear_small_gpu.py
  STATES      every edge the GPU cases must reach, by name; tests/test_linear_small_plan_cpu.py demands each from states_of()
  states_of   case -> the states it reaches
"""

LS_T, WIDE_MAX, MAXBLK = 32, 320, 16


def fwd_name(KC, split):
    return f"linear_small_fwd_kernel<{KC}, {'true' if split else 'false'}>"


def bwd_name(KC, RC):
    return f"linear_small_bwd_kernel<{KC}, {RC}>"


def kernel_name(entry, plan):
    """linear_small_plan's answer -> kernel name."""
    return fwd_name(plan["KC"], plan["SPLIT"]) if entry in ("fwd", "group_fwd") else bwd_name(plan["KC"], plan["RC"])


INSTANCES = [fwd_name(384, True), fwd_name(384, False), fwd_name(128, True), fwd_name(128, False), bwd_name(384, 512), bwd_name(128, 256)]

# (entry, problem, instance, tiles_dx, tiles_dw); problem: fwd (R, N, K, split) ; bwd (R, N, K, wants) with wants a subset of "xwb" (dx, dW, db) ;
# group_fwd (R, nblk, N, K, split) ; group_bwd (R, nblk, N, K, dx, any_dw).  The product runs R = 400 (cfg2: 2 x 200 queries) and 600 rows at
# d = 384, an FFN of 2048, heads of 4 (padded to 8), 24 and 96 columns and groups of 2, 3 and 13 Linears.
PINNED = [
    ("fwd", (400, 384, 384, True), fwd_name(384, True), 0, 0),            # 13 x 12 = 156
    ("fwd", (400, 384, 384, False), fwd_name(384, False), 0, 0),
    ("fwd", (600, 384, 384, True), fwd_name(384, True), 0, 0),            # 19 x 12 = 228
    ("fwd", (400, 2048, 384, True), fwd_name(128, True), 0, 0),           # FFN linear1: 13 x 64 = 832
    ("fwd", (400, 384, 2048, True), fwd_name(384, True), 0, 0),           # FFN linear2: 156 tiles, six chunks of 384 with a tail of 128
    ("fwd", (600, 2048, 384, False), fwd_name(128, False), 0, 0),         # 19 x 64 = 1216
    ("fwd", (600, 8, 384, True), fwd_name(384, True), 0, 0),              # box head, 4 columns padded to 8: 19 tiles
    ("fwd", (600, 24, 384, True), fwd_name(384, True), 0, 0),             # class head
    ("fwd", (600, 96, 384, False), fwd_name(384, False), 0, 0),           # 19 x 3 = 57
    ("fwd", (5, 10240, 8, False), fwd_name(384, False), 0, 0),            # 320 | 321
    ("fwd", (5, 10248, 8, False), fwd_name(128, False), 0, 0),
    ("bwd", (400, 384, 384, "xwb"), bwd_name(384, 512), 156, 144),        # 300
    ("bwd", (600, 384, 384, "xwb"), bwd_name(128, 256), 228, 144),        # 372
    ("bwd", (400, 2048, 384, "xwb"), bwd_name(128, 256), 156, 768),
    ("bwd", (400, 384, 2048, "xwb"), bwd_name(128, 256), 832, 768),
    ("bwd", (600, 24, 384, "xwb"), bwd_name(384, 512), 228, 12),          # 240: <384, 512> with R > 512
    ("bwd", (600, 8, 384, "xwb"), bwd_name(384, 512), 228, 12),
    ("bwd", (600, 96, 384, "xwb"), bwd_name(384, 512), 228, 36),
    ("bwd", (400, 384, 384, "wb"), bwd_name(384, 512), 0, 144),           # no input gradient wanted
    ("bwd", (400, 384, 384, "x"), bwd_name(384, 512), 156, 0),
    ("bwd", (400, 384, 384, "b"), bwd_name(384, 512), 0, 12),             # bias gradient only: the k-tile-0 workgroups
    ("bwd", (400, 384, 384, ""), None, 0, 0),                             # nothing wanted: nothing launched
    ("bwd", (32, 10208, 32, "xwb"), bwd_name(384, 512), 1, 319),          # 320 | 321
    ("bwd", (32, 10240, 32, "xwb"), bwd_name(128, 256), 1, 320),
    ("group_fwd", (400, 2, 384, 384, True), fwd_name(384, True), 0, 0),   # 13 x 24 = 312
    ("group_fwd", (400, 3, 384, 384, True), fwd_name(128, True), 0, 0),   # 13 x 36 = 468
    ("group_fwd", (400, 13, 384, 384, False), fwd_name(128, False), 0, 0),
    ("group_fwd", (600, 2, 384, 384, True), fwd_name(128, True), 0, 0),   # 19 x 24 = 456
    ("group_fwd", (5, 1, 10240, 8, False), fwd_name(384, False), 0, 0),
    ("group_fwd", (5, 1, 10272, 8, False), fwd_name(128, False), 0, 0),
    ("group_bwd", (400, 3, 384, 384, True, True), bwd_name(128, 256), 156, 432),
    ("group_bwd", (400, 13, 384, 384, True, True), bwd_name(128, 256), 156, 1872),
    ("group_bwd", (400, 2, 384, 384, False, True), bwd_name(384, 512), 0, 288),
    ("group_bwd", (300, 2, 256, 256, True, True), bwd_name(128, 256), 80, 128),      # 208 <= 320, but N % 384 != 0
    ("group_bwd", (400, 3, 384, 384, True, False), bwd_name(384, 512), 156, 0),      # no dy with a dW / db: the dx program alone
    ("group_bwd", (400, 3, 384, 384, False, False), None, 0, 0),
]


# ---- the GPU cases ------------------------------------------------------------------------------------------------------------------------
# forward: (R, N, K, act, flags); flags: b bias, p pre, x x16_out, s ldx = K + 12, u the scalar-store variants (ldc = N + 1 ; y one float behind
# a 16-byte boundary) on top of ldc = N and N + 4, t "ties" operands, r random-normal operands (bounded).  Each is run split and plain.
_FWD_384 = [
    (1, 8, 8, 0, "bpx"), (31, 24, 16, 1, "bpxsu"), (32, 32, 24, 0, "x"), (33, 40, 32, 2, "bps"), (33, 40, 40, 1, "bu"),
    (65, 24, 376, 0, "bx"), (33, 40, 384, 1, "bpxs"), (33, 24, 392, 0, "pu"), (33, 40, 400, 1, "bx"), (33, 40, 792, 0, "bxs"),
    (5, 10240, 8, 0, "bx"), (33, 40, 72, 0, "bxt"), (70, 72, 424, 0, "bxr"),
]
_FWD_128 = [
    (1, 10272, 8, 0, "bpx"), (31, 10272, 16, 1, "bxs"), (32, 10272, 24, 0, "x"), (33, 5152, 32, 2, "bps"), (10241, 8, 40, 1, "bxu"),
    (10241, 24, 16, 0, "pxsu"), (10271, 32, 8, 0, "b"), (5153, 40, 24, 0, "bpxu"),
    (33, 5152, 120, 0, "bx"), (33, 5152, 128, 1, "bpxs"), (33, 5152, 136, 0, "px"), (33, 5152, 144, 0, "bp"), (33, 5152, 280, 0, "bxs"),
    (5, 10248, 8, 0, "bx"), (33, 5152, 72, 0, "bxt"), (70, 5152, 168, 0, "bxr"),
]
FWD_CASES = [dict(entry="fwd", R=R, N=N, K=K, split=sp, act=act, flags=fl, id=f"fwd-{'split' if sp else 'plain'}-{R}x{N}x{K}-a{act}-{fl}")
             for sp in (True, False) for (R, N, K, act, fl) in _FWD_384 + _FWD_128]

# backward: (R, N, K, wants, act, flags); wants: subset of "xwb" ; flags: r random-normal (bounded), w wide dy for the bias sum (integers of 12
# significant bits: only where db is the one output)
_BWD_384 = [
    (511, 40, 64, "xwb", 0, ""), (512, 64, 40, "xwb", 1, ""), (513, 40, 40, "wb", 0, ""), (1055, 64, 64, "xwb", 0, ""), (1055, 40, 32, "w", 1, ""),
    (33, 8, 8, "xwb", 0, ""), (31, 24, 24, "xwb", 1, ""), (65, 40, 40, "xwb", 0, ""), (63, 24, 8, "x", 1, ""), (33, 40, 24, "b", 1, "w"),
    (33, 392, 24, "xwb", 0, ""), (33, 400, 8, "x", 0, ""), (33, 408, 40, "xwb", 1, ""), (65, 792, 24, "x", 0, ""),
    (32, 10208, 32, "xwb", 0, ""), (1, 40, 8, "b", 2, "w"), (600, 24, 384, "xwb", 0, ""), (600, 40, 72, "xwb", 0, "r"), (600, 40, 72, "b", 0, "w"),
    (97, 40, 24, "", 0, ""),
]
_BWD_128 = [
    (255, 5160, 40, "xwb", 0, ""), (256, 5160, 40, "wb", 1, ""), (257, 5160, 40, "xwb", 1, ""), (543, 5160, 40, "xwb", 0, ""), (543, 5160, 40, "w", 0, ""),
    (33, 8, 10248, "xwb", 0, ""), (31, 24, 10248, "xwb", 1, ""), (33, 40, 5128, "x", 0, ""), (33, 10280, 8, "xwb", 0, ""), (63, 10280, 24, "wb", 1, ""),
    (33, 136, 2080, "xwb", 0, ""), (33, 144, 2080, "xwb", 1, ""), (33, 152, 2080, "xwb", 0, ""), (65, 280, 1040, "xwb", 0, ""),
    (32, 10240, 32, "xwb", 0, ""), (1, 10272, 8, "b", 2, "w"), (33, 10272, 8, "b", 1, "w"), (300, 5160, 40, "xwb", 0, "r"), (300, 10272, 8, "b", 0, "w"),
]
BWD_CASES = [dict(entry="bwd", R=R, N=N, K=K, wants=w, act=act, flags=fl, id=f"bwd-{R}x{N}x{K}-{w or 'none'}-a{act}{'-' + fl if fl else ''}")
             for (R, N, K, w, act, fl) in _BWD_384 + _BWD_128]

# group forward: (R, nblk, N, K, split, add, bias, flags); add: "none" (array NULL), "all", "mixed" (NULL elements) ; bias likewise ; flags: x, s as above
_GFWD = [
    (33, 1, 32, 24, True, "none", "all", "x"), (33, 2, 96, 40, False, "all", "all", "xs"), (65, 16, 32, 392, True, "mixed", "mixed", "x"),
    (31, 2, 384, 792, False, "mixed", "none", ""), (33, 16, 96, 16, False, "all", "mixed", "x"), (1, 2, 384, 8, True, "all", "all", "xs"),
    (5, 1, 10240, 8, False, "none", "all", "x"), (5, 1, 10272, 8, False, "all", "all", "x"), (5, 1, 10272, 8, True, "all", "none", ""),
    (33, 16, 352, 136, True, "all", "all", "xs"), (70, 16, 96, 280, False, "mixed", "mixed", "x"), (33, 2, 5152, 24, True, "none", "mixed", "x"),
    (33, 16, 320, 24, True, "mixed", "all", "x"),
]
GROUP_FWD_CASES = [dict(entry="group_fwd", R=R, nblk=nb, N=N, K=K, split=sp, add=add, bias=bias, flags=fl,
                        id=f"gfwd-{'split' if sp else 'plain'}-{R}x{nb}x{N}x{K}-add:{add}-bias:{bias}{'-' + fl if fl else ''}")
                   for (R, nb, N, K, sp, add, bias, fl) in _GFWD]

# group backward: (R, nblk, N, K, dy, dW, db, dx); dy: which outputs have NO gradient - "none", "first", "middle", "last", "all" ; dW / db: "all",
# "none" (array NULL), "mixed" (NULL elements) ; dx: wanted
_GBWD = [
    (511, 1, 384, 32, "none", "all", "all", True), (512, 3, 384, 8, "first", "all", "mixed", True), (513, 3, 768, 24, "none", "mixed", "all", True),
    (1055, 3, 384, 40, "middle", "all", "all", True), (33, 3, 768, 8, "last", "all", "none", False), (65, 3, 384, 24, "all", "all", "all", True),
    (33, 1, 384, 24, "none", "none", "none", True),
    (255, 1, 128, 40, "none", "all", "all", True), (256, 3, 256, 24, "first", "mixed", "all", True), (257, 16, 128, 8, "middle", "all", "mixed", True),
    (543, 3, 512, 40, "last", "all", "all", True), (33, 16, 384, 64, "none", "all", "all", True), (33, 16, 256, 8, "all", "all", "all", True),
    (65, 3, 512, 24, "none", "none", "all", False), (31, 3, 128, 8, "all", "all", "all", False), (97, 1, 768, 392, "none", "all", "all", True),
]
GROUP_BWD_CASES = [dict(entry="group_bwd", R=R, nblk=nb, N=N, K=K, dy=dy, dW=dW, db=db, dx=dx,
                        id=f"gbwd-{R}x{nb}x{N}x{K}-nody:{dy}-dW:{dW}-db:{db}-{'dx' if dx else 'nodx'}")
                   for (R, nb, N, K, dy, dW, db, dx) in _GBWD]
GPU_CASES = {"fwd": FWD_CASES, "bwd": BWD_CASES, "group_fwd": GROUP_FWD_CASES, "group_bwd": GROUP_BWD_CASES}


def mixed_null(i):
    """The "mixed" pattern of a pointer table: which elements are NULL (every third, from the second on; mixed tables have nblk >= 2)."""
    return i % 3 == 1


def no_grad(which, i, nblk):
    """Does output i of a group backward case have no gradient (dy[i] NULL)?"""
    return {"none": False, "all": True, "first": i == 0, "last": i == nblk - 1, "middle": i == nblk // 2 and 0 < i < nblk - 1}[which]


# ---- the choice and the states of a case, by arithmetic ----------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def tiles_of(c):
    """-> (tiles_dx, tiles_dw, grid) as the launchers count them."""
    e, tr = c["entry"], _cdiv(c["R"], LS_T)
    if e == "fwd":
        return 0, 0, tr * _cdiv(c["N"], LS_T)
    if e == "group_fwd":
        return 0, 0, tr * (c["nblk"] * c["N"] // LS_T)
    tk = _cdiv(c["K"], LS_T)
    if e == "bwd":
        tn = _cdiv(c["N"], LS_T)
        tdx = tr * tk if "x" in c["wants"] else 0
        tdw = tn * tk if "w" in c["wants"] else (tn if "b" in c["wants"] else 0)
        return tdx, tdw, tdx + tdw
    tdx = tr * tk if c["dx"] else 0
    tdw = c["nblk"] * c["N"] // LS_T * tk if any_dw(c) else 0
    return tdx, tdw, tdx + tdw


def any_dw(c):
    """group backward: does some output have a dy and a wanted dW or db?"""
    nb = c["nblk"]
    for i in range(nb):
        if no_grad(c["dy"], i, nb):
            continue
        has_w = c["dW"] == "all" or (c["dW"] == "mixed" and not mixed_null(i))
        has_b = c["db"] == "all" or (c["db"] == "mixed" and not mixed_null(i))
        if has_w or has_b:
            return True
    return False


def instance_of(c):
    """The kernel a case must run on (None: nothing is launched)."""
    _, _, grid = tiles_of(c)
    if grid == 0:
        return None
    wide = grid <= WIDE_MAX
    if c["entry"] in ("fwd", "group_fwd"):
        return fwd_name(384 if wide else 128, c["split"])
    if c["entry"] == "group_bwd":
        wide = wide and c["N"] % 384 == 0
    return bwd_name(384, 512) if wide else bwd_name(128, 256)


_FWD_I = [(384, True), (384, False), (128, True), (128, False)]
_BWD_I = [(384, 512), (128, 256)]
STATES = (
    [f"{fwd_name(kc, sp)}: {s}" for kc, sp in _FWD_I for s in
     ["R=1", "R=31", "R=32", "R=33", "R%32=1 after a full row tile", "N=8", "N=24", "N=32", "N=40", "K=8", "K=16", "K=24", "K=32", "K=40",
      "K=KC-8", "K=KC", "K=KC+8", "K=2KC+24", "tail 8 after a full chunk", "tail 16 after a full chunk", "tail 24 after a full chunk",
      "ldx=K", "ldx=K+12", "ldc=N+1 and y+1float", "pre", "pre=NULL", "bias", "bias=NULL", "act=0", "act=1", "act=2", "x16_out", "x16_out=NULL",
      "ties", "random", "tiles=320" if kc == 384 else "tiles=321"]]
    + [f"{bwd_name(kc, rc)}: {s}" for kc, rc in _BWD_I for s in
       ["want=x", "want=w", "want=b", "want=wb", "want=xwb", "R=RC-1", "R=RC", "R=RC+1", "R=2RC+31", "R%32=1", "R%32=31", "N=8", "N=24", "N=40",
        "K=8", "K=24", "K=40", "dx: N=KC+8", "dx: N=KC+16", "dx: N=KC+24", "dx: N=2KC+24", "act=0", "act=1", "act=2", "random", "wide dy for db",
        "grid=320" if kc == 384 else "grid=321"]]
    + ["bwd: nothing wanted"]
    + [f"group_fwd: {s}" for s in
       ["nblk=1", "nblk=2", "nblk=16", "N=32", "N=96", "N=384", "add=none", "add=all", "add=mixed", "bias=none", "bias=mixed", "bias=all",
        "split", "plain", "tiles=320", "tiles=321", "x16_out", "x16_out=NULL", "ldx=K+12", "KC=384", "KC=128", "K=KC+8 at KC=128", "K=2KC+24 at KC=384"]]
    + [f"group_bwd: {s}" for s in
       ["N=128", "N=256", "N=384", "N=512", "N=768", "N=384 on <128, 256>", "nblk=1", "nblk=3", "nblk=16", "dy NULL: first", "dy NULL: middle",
        "dy NULL: last", "dy NULL: all with dx", "dy NULL: all without dx", "dW=none", "dW=mixed", "db=none", "db=mixed", "dx=NULL",
        "nothing but dx"]]
    + [f"group_bwd {bwd_name(kc, rc)}: {s}" for kc, rc in _BWD_I for s in ["R=RC-1", "R=RC", "R=RC+1", "R=2RC+31"]]
)


def states_of(c):
    """The states a case reaches, by arithmetic on its shape and switches."""
    inst, e, R, N, K = instance_of(c), c["entry"], c["R"], c["N"], c["K"]
    out = []
    tdx, tdw, grid = tiles_of(c)
    if e == "fwd":
        kc, fl = (384 if "<384" in inst else 128), c["flags"]
        s = [f"R={R}"] if R in (1, 31, 32, 33) else []
        s += ["R%32=1 after a full row tile"] if R > 32 and R % 32 == 1 else []
        s += [f"N={N}"] if N in (8, 24, 32, 40) else []
        s += [f"K={K}"] if K in (8, 16, 24, 32, 40) else []
        s += [{kc - 8: "K=KC-8", kc: "K=KC", kc + 8: "K=KC+8", 2 * kc + 24: "K=2KC+24"}[K]] if K in (kc - 8, kc, kc + 8, 2 * kc + 24) else []
        s += [f"tail {K % kc % 32} after a full chunk"] if K > kc and K % kc % 32 else []
        s += ["ldx=K+12" if "s" in fl else "ldx=K", "pre" if "p" in fl else "pre=NULL", "bias" if "b" in fl else "bias=NULL", f"act={c['act']}",
              "x16_out" if "x" in fl else "x16_out=NULL"]
        s += ["ldc=N+1 and y+1float"] if "u" in fl else []
        s += ["ties"] if "t" in fl else []
        s += ["random"] if "r" in fl else []
        s += [f"tiles={grid}"] if grid in (320, 321) else []
        out = [f"{inst}: {x}" for x in s]
    elif e == "bwd":
        if inst is None:
            return ["bwd: nothing wanted"]
        kc, rc = (384, 512) if "<384" in inst else (128, 256)
        w, fl = c["wants"], c["flags"]
        s = [f"want={w}", f"act={c['act']}"]
        s += [{rc - 1: "R=RC-1", rc: "R=RC", rc + 1: "R=RC+1", 2 * rc + 31: "R=2RC+31"}[R]] if R in (rc - 1, rc, rc + 1, 2 * rc + 31) and "w" in w else []
        s += [f"R%32={R % 32}"] if R % 32 in (1, 31) else []
        s += [f"N={N}"] if N in (8, 24, 40) else []
        s += [f"K={K}"] if K in (8, 24, 40) and ("x" in w or "w" in w) else []
        if "x" in w and N in (kc + 8, kc + 16, kc + 24, 2 * kc + 24):
            s += ["dx: N=" + {kc + 8: "KC+8", kc + 16: "KC+16", kc + 24: "KC+24", 2 * kc + 24: "2KC+24"}[N]]
        s += ["random"] if "r" in fl else []
        s += ["wide dy for db"] if "w" in fl else []
        s += [f"grid={grid}"] if grid in (320, 321) else []
        out = [f"{inst}: {x}" for x in s]
    elif e == "group_fwd":
        kc, fl, nb = (384 if "<384" in inst else 128), c["flags"], c["nblk"]
        s = [f"nblk={nb}"] if nb in (1, 2, 16) else []
        s += [f"N={N}"] if N in (32, 96, 384) else []
        s += [f"add={c['add']}", f"bias={c['bias']}", "split" if c["split"] else "plain", f"KC={kc}"]
        s += [f"tiles={grid}"] if grid in (320, 321) else []
        s += ["x16_out" if "x" in fl else "x16_out=NULL"] + (["ldx=K+12"] if "s" in fl else [])
        s += ["K=KC+8 at KC=128"] if kc == 128 and K == 136 else []
        s += ["K=2KC+24 at KC=384"] if kc == 384 and K == 792 else []
        out = [f"group_fwd: {x}" for x in s]
    else:
        nb = c["nblk"]
        if inst is None:
            return ["group_bwd: dy NULL: all without dx"]
        kc, rc = (384, 512) if "<384" in inst else (128, 256)
        s = [f"N={N}"] + ([f"nblk={nb}"] if nb in (1, 3, 16) else [])
        s += ["N=384 on <128, 256>"] if N == 384 and kc == 128 else []
        s += [f"dy NULL: {c['dy']}"] if c["dy"] in ("first", "middle", "last") else []
        s += ["dy NULL: all with dx"] if c["dy"] == "all" and c["dx"] else []
        s += [f"dW={c['dW']}"] if c["dW"] != "all" else []
        s += [f"db={c['db']}"] if c["db"] != "all" else []
        s += ["dx=NULL"] if not c["dx"] else []
        s += ["nothing but dx"] if tdw == 0 else []
        out = [f"group_bwd: {x}" for x in s]
        if R in (rc - 1, rc, rc + 1, 2 * rc + 31) and tdw:
            out.append(f"group_bwd {inst}: " + {rc - 1: "R=RC-1", rc: "R=RC", rc + 1: "R=RC+1", 2 * rc + 31: "R=2RC+31"}[R])
    return out
