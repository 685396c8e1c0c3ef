"""Shapes of the weight-gradient TN GEMM (spe_gemm_bf16tn, csrc/gemm_bf16tn.hip) and the kernel instance each must run on.

The selection is tn_gemm_select in csrc/gemm_bf16tn.hip, visible through kernels.gemm16_tn_plan (spe_gemm_bf16tn_plan, host only).  This
file holds data only; a problem is (M, N, R, splitk) with splitk as the entry takes it (1, or -n for n slabs):

  INSTANCES   the three kernel instances the library compiles, by the name a profiler prints
  PINNED      (problem, (BM, BN)) written out BY HAND from the dispatch code as it stood before the selection became one function:
                  t128 = ceil(M / 128) * ceil(N / 128) * splits ;  t128 < 256 -> 64 x 64 ;  else M > 64 and N > 64 -> 128 x 128 ;
                  else M > 64 -> 128 x 64 ;  else 64 x 64
              - never regenerate it from the function under test
  GPU_SITES   the problems of tests/test_tn_gemm_gpu.py by the launch site they must reach (the 64 x 64 kernel has two: the small-tile
              rule and M <= 64); tests/test_tn_gemm_plan_cpu.py demands that each site sees a split with 0, 1, 2, 3 and >= 4 row tiles
  GPU_CASES   the same problems as one list
"""


def tn(BM, BN):
    return f"gemm_bf16tn_kernel<{BM}, {BN}>"


def kernel_name(plan):
    """gemm16_tn_plan's answer -> kernel name (None stays None)."""
    return None if plan is None else tn(plan["BM"], plan["BN"])


INSTANCES = [tn(128, 128), tn(128, 64), tn(64, 64)]

PINNED = [
    # the weight gradients of a cfg2 step (8300 tokens, width 384) with the split kernels._dw16_tn gives them; profiles/r06_final_kernel_stats.csv
    # names exactly these two instances for the step: gemm_bf16tn_kernel<128, 128> and gemm_bf16tn_kernel<64, 64>, never <128, 64>
    ((384, 384, 8300, -14), (64, 64)),          # proj, decoder blocks: 9 x 14 = 126 < 256; 36 tiles of 64: 512 // 36 = 14 splits
    ((1536, 384, 8300, -14), (128, 128)),       # fc1: 36 x 14 = 504
    ((384, 1536, 8300, -14), (128, 128)),       # fc2
    ((1152, 384, 8300, -16), (128, 128)),       # qkv: 27 x 16 = 432
    ((4608, 384, 8300, -4), (128, 128)),        # 108 x 4 = 432
    # 128-tiles x splits = 255 | 256
    ((1920, 2176, 400, 1), (64, 64)),           # 15 x 17 = 255
    ((2048, 2048, 400, 1), (128, 128)),         # 16 x 16 = 256
    ((384, 2176, 1100, -5), (64, 64)),          # 3 x 17 x 5 = 255
    ((512, 1024, 1100, -8), (128, 128)),        # 4 x 8 x 8 = 256
    ((1920, 56, 1100, -17), (64, 64)),          # 15 x 1 x 17 = 255: the small-tile rule comes before the narrow ones
    ((56, 1920, 1100, -17), (64, 64)),
    # M = 64 | 72 at N > 64, 16 x 16 = 256 wide tiles
    ((64, 2048, 1100, -16), (64, 64)),
    ((72, 2048, 1100, -16), (128, 128)),
    # N = 64 | 72 at M > 64
    ((2048, 64, 1100, -16), (128, 64)),
    ((2048, 72, 1100, -16), (128, 128)),
    # decoder-size problems, no split
    ((384, 384, 400, 1), (64, 64)),
    ((8, 8, 5, 1), (64, 64)),
]

# (M, N, R, splitk) by launch site.  Row tiles per split are given where they matter.  Every shape is ragged in the tile it runs on except
# the "whole tiles" ones.  The 3-tile cases of the two narrow sites are additions to the list this file was first specified with, which
# reached 0, 1, 2 and 4 tiles there but never 3.
GPU_SITES = {
    "small": [                                   # launch_tn<64, 64> by the small-tile rule
        (8, 8, 5, 1),
        (72, 136, 1, 1), (72, 136, 63, 1), (72, 136, 64, 1), (72, 136, 65, 1), (72, 136, 129, 1), (72, 136, 200, 1), (72, 136, 321, 1),   # 1 1 1 2 3 4 6
        (136, 72, 700, -11),                     # 1 each
        (136, 72, 641, -6),                      # 2 2 2 2 2 1
        (392, 392, 1100, -14),                   # nine splits of 2 tiles, five empty
    ],
    "128x128": [                                 # tiles of 128, 128, 8 rows and 9 x 128 + 8 columns
        (264, 1160, 579, -10),                   # 1 each
        (264, 1160, 600, -9),                    # 2 x 5, four empty
        (264, 1160, 1667, -9),                   # 3 each, the last tile has 3 rows
        (264, 1160, 2500, -9),                   # 5 x 8, one empty
        (384, 1152, 1667, -10),                  # whole tiles
    ],
    "128x64": [
        (2048, 64, 1100, -16),                   # whole tiles: 2 x 9, seven empty
        (2056, 56, 1030, -16),                   # 2 x 8, 1, seven empty
        (2056, 56, 3100, -16),                   # 4 x 12, 1, three empty
        (2056, 56, 2100, -16),                   # 3 x 11, five empty
    ],
    "m64": [                                     # launch_tn<64, 64> by M <= 64
        (64, 2048, 1100, -16),
        (56, 2056, 1030, -16),
        (56, 2056, 3100, -16),
        (56, 2056, 2100, -16),
    ],
}
SITE_INSTANCE = {"small": (64, 64), "128x128": (128, 128), "128x64": (128, 64), "m64": (64, 64)}
GPU_CASES = [c for site in GPU_SITES.values() for c in site]
# one case per launch site for the scalar-store variants (ldc = N + 1 ; C one float behind a 16-byte boundary)
SCALAR_STORE_CASES = [(72, 136, 129, 1), (264, 1160, 600, -9), (2056, 56, 1030, -16), (56, 2056, 1030, -16)]
