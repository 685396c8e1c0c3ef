"""Shapes of the 16-bit NT GEMM family (spe_gemm_bf16nt, spe_gemm_bf16nt_ex) and the kernel instance each must run on.

The selection lives in csrc/gemm_nt_select.h and is visible through kernels.gemm16_plan (spe_gemm_bf16nt_plan, host only).  This file
holds data only:

  INSTANCES   the 14 + 10 kernel instances the library compiles, by the name a profiler prints
  PINNED      (problem, expected kernel) written out BY HAND from the dispatch code as it stood before the selection became one function
              (spe_nt2_dispatch / spe_gemm_bf16nt / gemm_bf16nt_ex_impl with their shipped constants), cross-checked against the kernel
              names of profiles/r06_final_kernel_stats.csv - never regenerate it from the function under test
  GPU_CASES   the problems tests/test_kernels_gpu.py::test_nt_gemm_every_instance runs; tests/test_nt_gemm_plan_cpu.py demands that
              they reach every instance at least once, so no compiled kernel is untested and a test can tell which kernel it exercises
  STEP_SHAPES the NT products of a cfg2 training step (8300 tokens, width 384), for tools/nt_gemm_digest.py

A problem is a dict of gemm16_plan's keyword arguments plus M, N, K.
"""


def P(M, N, K, **kw):
    return dict(M=M, N=N, K=K, **kw)


def _b(v):
    return "true" if v else "false"


def nt2(BM, BN, BK, SPLIT, EX, F16, NST=2):
    return f"gemm_nt2_kernel<{BM}, {BN}, {BK}, {NST}, {_b(SPLIT)}, {_b(EX)}, {_b(F16)}>"


def b16(BM, BN, EX, NTS=0, SPLIT=False):
    return f"gemm_bf16nt_kernel<{BM}, {BN}, {_b(EX)}, {NTS}, {_b(SPLIT)}>"


def kernel_name(plan):
    """gemm16_plan's answer -> kernel name (None stays None)."""
    if plan is None:
        return None
    if plan["family"] == "nt2":
        return nt2(plan["BM"], plan["BN"], plan["BK"], plan["SPLIT"], plan["EX"], plan["F16"], plan["NST"])
    return b16(plan["BM"], plan["BN"], plan["EX"], plan["NTS"], plan["SPLIT"])


T, F = True, False
INSTANCES = [
    nt2(128, 128, 64, F, T, T), nt2(128, 64, 64, F, T, T), nt2(160, 128, 64, F, F, T), nt2(128, 128, 64, F, F, T),
    nt2(160, 128, 32, T, F, F), nt2(160, 128, 64, F, F, F), nt2(64, 64, 64, F, F, F), nt2(64, 64, 64, F, T, F),
    nt2(128, 64, 32, T, F, F), nt2(128, 64, 32, T, T, F), nt2(128, 128, 32, T, F, F), nt2(128, 128, 32, T, T, F),
    nt2(128, 128, 64, F, F, F), nt2(128, 128, 64, F, T, F),
    b16(128, 128, F), b16(128, 128, T), b16(128, 64, F), b16(128, 64, T), b16(64, 64, F), b16(64, 64, T),
    b16(64, 64, F, SPLIT=T), b16(64, 64, T, SPLIT=T), b16(64, 64, F, NTS=6), b16(64, 64, F, NTS=7),
]

PINNED = [
    # the products of a cfg2 step (kernel names: profiles/r06_final_kernel_stats.csv)
    (P(8300, 1152, 384, split=T), nt2(160, 128, 32, T, F, F)),                  # qkv forward: 52 x 9 tall tiles fit one round
    (P(8300, 384, 384, split=T), nt2(128, 64, 32, T, F, F)),
    (P(8300, 384, 1152), nt2(64, 64, 64, F, F, F)),                             # qkv dx
    (P(8300, 384, 1536), nt2(64, 64, 64, F, F, F)),                             # fc1 dx
    (P(8300, 384, 384, split=T, ex=T), nt2(128, 64, 32, T, T, F)),              # proj + residual
    (P(8300, 1536, 384, ex=T), nt2(64, 64, 64, F, T, F)),                       # fc2 dh
    (P(8300, 1536, 384, ex=T, op_f16=T, lo_f16=T), nt2(128, 128, 64, F, T, T)),  # fc1 + GELU on fp16 operands
    (P(8300, 1536, 384, ex=T, op_f16=T), nt2(128, 128, 64, F, T, T)),
    (P(8300, 384, 1536, ex=T, op_f16=T), nt2(128, 64, 64, F, T, T)),            # fc2 + residual on fp16 operands
    (P(8300, 4608, 384, op_f16=T), nt2(128, 128, 64, F, F, T)),                 # decoder memory side: 5 rounds of 128 = 4 rounds of 160 rows
    (P(8300, 2304, 384, op_f16=T), nt2(160, 128, 64, F, F, T)),                 # 52 x 18 = 936: 2 rounds of 160 < 3 rounds of 128
    (P(4150, 1536, 384, split=T), nt2(128, 128, 32, T, F, F)),                  # 33 x 12 = 396 tiles: one round, no gain from tall tiles
    (P(4150, 1536, 384), nt2(128, 128, 64, F, F, F)),
    (P(8300, 1152, 384), nt2(160, 128, 64, F, F, F)),
    (P(8300, 1536, 384, split=T, ex=T), nt2(128, 64, 32, T, T, F)),             # split + extended epilogue: wide from N = 2048 only
    (P(8300, 2048, 384, split=T, ex=T), nt2(128, 128, 32, T, T, F)),
    (P(8300, 2048, 384, ex=T), nt2(128, 128, 64, F, T, F)),
    (P(8300, 2047, 384, ex=T), nt2(64, 64, 64, F, T, F)),
    (P(8300, 1023, 384), nt2(64, 64, 64, F, F, F)),                             # plain: wide from N = 1024
    (P(8300, 1024, 384), nt2(160, 128, 64, F, F, F)),                           # 65 x 8 = 520: 2 rounds of 128 ; 52 x 8 = 416: 1 of 160
    (P(2048, 1024, 384), nt2(128, 128, 64, F, F, F)),                           # one round either way
    (P(8300, 1023, 384, ex=T, op_f16=T), nt2(128, 64, 64, F, T, T)),
    (P(8300, 1024, 384, ex=T, op_f16=T), nt2(128, 128, 64, F, T, T)),
    # the edges of the nt2 domain: below each, the register-pipelined family
    (P(2047, 384, 384), b16(64, 64, F, NTS=6)),                                 # 16 x 3 = 48 wide tiles, 16 x 6 = 96 < 256, 6 K tiles
    (P(2048, 384, 384), nt2(64, 64, 64, F, F, F)),
    (P(2048, 384, 64), b16(64, 64, F)),                                         # bf16: one ring stage is not worth it
    (P(2048, 384, 64, op_f16=T), nt2(128, 128, 64, F, F, T)),                   # fp16 operands have no other family
    (P(2048, 384, 128), nt2(64, 64, 64, F, F, F)),
    (P(2048, 384, 192), nt2(64, 64, 64, F, F, F)),
    (P(2048, 384, 200), b16(64, 64, F)),                                        # K % 64 != 0
    (P(2048, 384, 200, op_f16=T), None),
    (P(2048, 56, 384), b16(64, 64, F)),
    (P(2048, 64, 384), nt2(64, 64, 64, F, F, F)),
    (P(2048, 56, 384, op_f16=T), None),
    (P(2047, 384, 384, op_f16=T), None),
    (P(2048, 384, 384, ex=T, lo_f16=T), None),                                  # the fp16 second copy needs fp16 operands
    (P(8300, 384, 384, splitk=-2), b16(128, 128, F)),                           # K slabs: 65 x 3 x 2 = 390 wide tiles fill the chip
    (P(8300, 384, 384, ex=T, out16T=T, ld16t=8320), b16(64, 64, T)),
    (P(8300, 384, 384, split=T, ex=T, out16T=T, ld16t=8320), b16(64, 64, T, SPLIT=T)),
    (P(2047, 384, 384, split=T), b16(64, 64, F, SPLIT=T)),
    (P(2047, 384, 384, split=T, ex=T), b16(64, 64, T, SPLIT=T)),
    # the shapes the removed LDS-DMA variant of gemm_bf16nt_kernel could still reach (N < 64, or a transposed copy): the next rule
    (P(2051, 56, 1024), b16(64, 64, F)),
    (P(2051, 384, 1024, ex=T, out16T=T, ld16t=2112), b16(64, 64, T)),
    # fewer than 2048 rows (decoder-size problems, weight-gradient-shaped slabs)
    (P(400, 2048, 384), b16(64, 64, F, NTS=6)),                                 # 4 x 16 = 64 wide tiles, 4 x 32 = 128 < 256
    (P(300, 384, 384), b16(64, 64, F, NTS=6)),
    (P(384, 384, 448), b16(64, 64, F, NTS=7)),
    (P(384, 384, 512), b16(64, 64, F)),
    (P(1536, 384, 8320, splitk=-16), b16(128, 128, F)),                         # 12 x 3 x 16 = 576 >= 384
    (P(1000, 3000, 384), b16(128, 64, F)),                                      # 8 x 24 = 192 < 384 ; 8 x 47 = 376 >= 256
    (P(2000, 3072, 384), b16(128, 128, F)),                                     # 16 x 24 = 384
    (P(2000, 3072, 384, ex=T), b16(128, 128, T)),
    (P(1000, 3000, 384, ex=T), b16(128, 64, T)),
    (P(300, 384, 384, ex=T), b16(64, 64, T)),
    (P(300, 384, 384, ex=T, out16T=T, ld16t=384), b16(128, 64, T)),             # only the 128-row tiles reach column 383 of the transposed copy
    (P(300, 384, 384, ex=T, out16T=T, ld16t=448), None),
]

# Problems of the GPU test: the smallest shapes that reach each instance (ragged rows and columns everywhere; more than one workgroup per
# direction).  7169 rows = the fewest at which 9 column tiles of 160-row tiles need one round and 128-row tiles two (45 x 9 = 405, 57 x 9 = 513).
GPU_CASES = [
    P(2051, 1032, 64, ex=T, op_f16=T, lo_f16=T), P(2051, 72, 64, ex=T, op_f16=T, lo_f16=T),
    P(7169, 1152, 64, op_f16=T), P(2051, 72, 64, op_f16=T),
    P(7169, 1152, 128, split=T), P(7169, 1152, 128),
    P(2051, 72, 128), P(2051, 72, 128, ex=T), P(2051, 72, 128, split=T), P(2051, 72, 128, split=T, ex=T),
    P(2051, 1032, 128, split=T), P(2051, 1032, 128),
    P(2051, 2056, 128, split=T, ex=T), P(2051, 2056, 128, ex=T),
    # register-pipelined family: above 2048 rows (K no multiple of 64 ; N < 64 ; a transposed copy) ...
    P(2051, 72, 200), P(2051, 72, 200, ex=T), P(2051, 72, 200, split=T), P(2051, 72, 200, split=T, ex=T),
    P(2051, 56, 1024), P(2051, 384, 1024, ex=T, out16T=T, ld16t=2112),
    # ... and below
    P(2047, 3072, 72), P(2047, 3072, 72, ex=T), P(2047, 1000, 72), P(2047, 1000, 72, ex=T),
    P(130, 72, 200), P(130, 72, 448),
]

# NT products of a cfg2 training step (B * N = 8300 tokens, width 384, MLP 1536; decoder memory side 6 layers stacked), bf16s mode
STEP_SHAPES = [
    P(8300, 1152, 384, split=T), P(8300, 384, 384, split=T, ex=T), P(8300, 1536, 384, ex=T, op_f16=T, lo_f16=T), P(8300, 384, 1536, ex=T, op_f16=T),
    P(8300, 384, 1152), P(8300, 384, 384), P(8300, 1536, 384, ex=T), P(8300, 384, 1536),
    P(8300, 4608, 384, op_f16=T), P(8300, 2304, 384, op_f16=T), P(8300, 384, 4608), P(8300, 384, 2304),
    P(8300, 384, 384, split=T), P(8300, 1536, 384, split=T, ex=T), P(8300, 384, 1536, split=T, ex=T),
]
