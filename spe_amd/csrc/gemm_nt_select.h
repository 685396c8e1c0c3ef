// Kernel selection of the 16-bit NT GEMM family (spe_gemm_bf16nt, spe_gemm_bf16nt_ex(d)): ONE pure function from the problem to the kernel
// instance that runs it, and the list of the instances that exist.  Host only, no HIP types: the launcher (gemm_bf16.hip) switches over
// the list, spe_gemm_bf16nt_plan hands the same answer to tests and tools (tests/test_nt_gemm_plan_cpu.py pins it).
//
//   nt2     gemm_nt2.hip   gemm_nt2_kernel<BM, BN, BK, NST, SPLIT, EX, F16>     LDS-DMA ring, activation-sized products (>= 2048 rows)
//   bf16nt  gemm_bf16.hip  gemm_bf16nt_kernel<BM, BN, EX, NTS, SPLIT>           register-pipelined loop (BK = 64), everything else
//
// The thresholds below were developer knobs while they were tuned; the shipped library has none, so each is a constant
// with the measurement that set it.  What the removed alternatives measured: profiles/HISTORY_r05.md section 3.
#pragma once

enum NtFamily { NT_FAMILY_NT2 = 0, NT_FAMILY_BF16NT = 1 };

struct NtProblem {
    int M, N, K;
    bool split;        // (hi, lo) operand pairs: three-term product
    bool ex;           // extended epilogue (spe_gemm_bf16nt_ex / _exd)
    bool f16;          // the operands hold IEEE fp16 (single-term product)
    bool f16_second;   // extended epilogue: the second 16-bit copy of the result is IEEE fp16 (fp16 operands only)
    int splitk;        // K slices (>= 1; slab mode of spe_gemm_bf16nt)
    bool out16t;       // extended epilogue: a transposed 16-bit copy [N][ld16t] is requested
    long ld16t;
};

struct NtPlan {
    int err;           // 0, or the status the GEMM entry returns for this problem (-2: no kernel covers it)
    int family;        // NtFamily
    int BM, BN, BK;    // workgroup tile; BK = contraction depth of one stage
    int NST;           // nt2: ring stages (bf16nt: 0 - two LDS buffers behind a register stage)
    int NTS;           // bf16nt: > 0 = every K tile in flight at once, NTS tiles at most (nt2: 0)
    bool SPLIT, EX, F16;
};

// ---- nt2 domain.  Fewer rows, a K split, a transposed copy or a contraction that is no multiple of the stage depth run on bf16nt.
constexpr int NT2_MIN_ROWS = 2048;
constexpr int NT2_MIN_COLS = 64;
constexpr int NT2_K_STEP = 64;
// bf16 products of a contraction of ONE stage are faster on the register-pipelined kernels; fp16 operands have no other kernel family, so
// their domain reaches down to one stage (K = 64: the ring's refill clamps to the last tile)
constexpr int NT2_MIN_K = 128, NT2_MIN_K_F16 = 64;
// plain epilogue: 128-wide column tiles from N = 1024 on; narrower outputs keep more workgroups in flight (8300 x 384: 390 tiles of 128 x 64)
constexpr int NT2_WIDE_MIN = 1024;
// single-term + extended epilogue (fc2 dh: GELU derivative from the saved pre-activation, bf16 output, column sums) is bound by that
// epilogue: narrow tiles overlap it with other workgroups' main loops (8300 x 1536 x 384: 63 -> 51 us)
constexpr int NT2_WIDE_MIN_EX_SINGLE = 2048;
// split + extended epilogue (fc1 + GELU: pre-activation + hi / lo bf16 outputs): 85 -> 73 us INSIDE the step on 128 x 64 tiles (the
// isolated launch prefers the wide tiles, 69 vs 76 us: measured in the step)
constexpr int NT2_WIDE_MIN_EX_SPLIT = 2048;
// 512 = resident workgroup slots (256 CUs x 2).  Tile quantisation: 8300 rows make 65 row tiles of 128; 65 x 9 = 585 tiles (qkv forward)
// take 2 rounds for 1.14 rounds of work, 160-row tiles (52 x 9 = 468) fit ONE round of 1.25x larger tiles.  Plain epilogue only (the
// staged epilogue of a 160 x 128 tile does not fit two workgroups per CU).
constexpr long NT2_SLOTS = 512;
inline bool nt2_tall_wins(int M, int N) {
    const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128), t160 = (long)((M + 159) / 160) * ((N + 127) / 128);
    return ((t160 + NT2_SLOTS - 1) / NT2_SLOTS) * 160 < ((t128 + NT2_SLOTS - 1) / NT2_SLOTS) * 128;
}

inline NtPlan nt_plan_make(int family, int BM, int BN, int BK, int NST, int NTS, bool SPLIT, bool EX, bool F16) {
    return NtPlan{0, family, BM, BN, BK, NST, NTS, SPLIT, EX, F16};
}
inline NtPlan nt_plan_error(int err) { return NtPlan{err, -1, 0, 0, 0, 0, 0, false, false, false}; }

inline NtPlan nt_gemm_select(const NtProblem& q) {
    const int M = q.M, N = q.N, K = q.K;
    auto nt2 = [&](int BM, int BN, int BK, bool SPLIT, bool F16) { return nt_plan_make(NT_FAMILY_NT2, BM, BN, BK, 2, 0, SPLIT, q.ex, F16); };
    auto b16 = [&](int BM, int BN, int NTS, bool SPLIT) { return nt_plan_make(NT_FAMILY_BF16NT, BM, BN, 64, 0, NTS, SPLIT, q.ex, false); };
    const bool in_nt2 = M >= NT2_MIN_ROWS && q.splitk == 1 && !q.out16t && (K % NT2_K_STEP) == 0 && K >= (q.f16 ? NT2_MIN_K_F16 : NT2_MIN_K) &&
                        N >= NT2_MIN_COLS;
    if (in_nt2) {
        if (q.f16_second && !q.f16) return nt_plan_error(-2);      // the fp16 second copy comes with fp16 operands only
        if (q.f16) {
            if (q.split) return nt_plan_error(-2);
            // extended epilogue (round 5: the backbone MLP's forward products in precision mode bf16s - fc1 + GELU emitting the bf16 copy for
            // the backward and the fp16 copy for fc2, fc2 + LayerScale residual)
            if (q.ex) return nt2(128, N >= NT2_WIDE_MIN ? 128 : 64, 64, false, true);
            // plain (the decoder's memory-side projections): wide tiles
            return nt2(nt2_tall_wins(M, N) ? 160 : 128, 128, 64, false, true);
        }
        const bool wide = N >= (q.ex ? (q.split ? NT2_WIDE_MIN_EX_SPLIT : NT2_WIDE_MIN_EX_SINGLE) : NT2_WIDE_MIN);
        if (!q.ex && wide && nt2_tall_wins(M, N)) return nt2(160, 128, q.split ? 32 : 64, q.split, false);
        // Narrow outputs, single-term (N = 384: the input-gradient products; fc2 dh): 8300 x 384 is 390 tiles of 128 x 64 - 1.5 workgroups per
        // CU.  64 x 64 tiles (780 workgroups, three to four per CU) hide each other's load latency: qkv dx 19.4 -> 17.0 us, fc1 dx 24.0 ->
        // 21.5, the stacked decoder dx (K = 4608) 59.3 -> 53.1; in the step fc2 dh 64.5 -> 56.3 us.  The split products gain nothing from them.
        if (!wide && !q.split) return nt2(64, 64, 64, false, false);
        return nt2(128, wide ? 128 : 64, q.split ? 32 : 64, q.split, false);      // split: BK = 32 keeps the (hi, lo) stage at 32 KB
    }
    if (q.f16 || q.f16_second) return nt_plan_error(-2);           // fp16 operands / fp16 second copy: the LDS-DMA kernels only
    const long ktiles = (K + 63) / 64;
    if (!q.ex) {
        // split operands: 64 x 64 tiles at two workgroups per CU (73 KB of LDS each)
        if (q.split) return q.splitk == 1 ? b16(64, 64, 0, true) : nt_plan_error(-3);
        // Activation-sized products outside the nt2 domain: 64 x 64 tiles (2000-3000 small workgroups at 4 per CU overlap one's stores with
        // another's loads).  The weight-gradient-shaped products (few output tiles, K slabs) keep the wide tiles.
        if (q.splitk == 1 && M >= 2048) return b16(64, 64, 0, false);
        // 128 x 128 when that already fills the chip, else narrower tiles (more workgroups in flight)
        const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128) * q.splitk;
        if (t128 >= 384 && N > 64) return b16(128, 128, 0, false);
        const long t64n = (long)((M + 127) / 128) * ((N + 63) / 64) * q.splitk;
        if (t64n >= 256 && M > 64) return b16(128, 64, 0, false);
        // decoder-size problems (few workgroups, short contraction): every K tile in flight at once
        if (q.splitk == 1 && ktiles <= 6) return b16(64, 64, 6, false);
        if (q.splitk == 1 && ktiles == 7) return b16(64, 64, 7, false);
        return b16(64, 64, 0, false);
    }
    // the transposed copy's zero columns M .. ld16t - 1 are written by the last row tile: it must reach ld16t
    const bool reach128 = !q.out16t || q.ld16t <= (long)((M + 127) / 128) * 128;
    const bool reach64 = !q.out16t || q.ld16t <= (long)((M + 63) / 64) * 64;
    if (!reach128 && !reach64) return nt_plan_error(-2);
    if (q.split) return reach64 ? b16(64, 64, 0, true) : nt_plan_error(-2);
    if (M >= 2048 && reach64) return b16(64, 64, 0, false);
    const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128);
    if (reach128 && t128 >= 384 && N > 64) return b16(128, 128, 0, false);
    const long t64n = (long)((M + 127) / 128) * ((N + 63) / 64);
    if (reach128 && ((t64n >= 256 && M > 64) || !reach64)) return b16(128, 64, 0, false);
    return b16(64, 64, 0, false);
}

// ---- the instances that exist: X(BM, BN, BK, NST, SPLIT, EX, F16) / X(BM, BN, EX, NTS, SPLIT).  nt_gemm_select returns nothing else
// (tests/test_nt_gemm_plan_cpu.py), and the launcher's switch and the explicit instantiations of gemm_nt2.hip are generated from these lists.
#define NT2_INSTANCES(X)                                                                                                      \
    X(128, 128, 64, 2, false, true, true)   X(128, 64, 64, 2, false, true, true)                                              \
    X(160, 128, 64, 2, false, false, true)  X(128, 128, 64, 2, false, false, true)                                            \
    X(160, 128, 32, 2, true, false, false)  X(160, 128, 64, 2, false, false, false)                                           \
    X(64, 64, 64, 2, false, false, false)   X(64, 64, 64, 2, false, true, false)                                              \
    X(128, 64, 32, 2, true, false, false)   X(128, 64, 32, 2, true, true, false)                                              \
    X(128, 128, 32, 2, true, false, false)  X(128, 128, 32, 2, true, true, false)                                             \
    X(128, 128, 64, 2, false, false, false) X(128, 128, 64, 2, false, true, false)
#define BF16NT_INSTANCES(X)                                                                                                   \
    X(128, 128, false, 0, false) X(128, 128, true, 0, false) X(128, 64, false, 0, false) X(128, 64, true, 0, false)           \
    X(64, 64, false, 0, false)   X(64, 64, true, 0, false)   X(64, 64, false, 0, true)   X(64, 64, true, 0, true)             \
    X(64, 64, false, 6, false)   X(64, 64, false, 7, false)

// one integer per instance: the `case` labels of the launcher's switch
constexpr int nt_key(int family, int BM, int BN, int BK, int NST, int NTS, bool SPLIT, bool EX, bool F16) {
    return (((((((family * 256 + BM) * 256 + BN) * 2 + (BK == 64)) * 4 + NST) * 8 + NTS) * 2 + SPLIT) * 2 + EX) * 2 + F16;
}
inline int nt_key(const NtPlan& s) { return nt_key(s.family, s.BM, s.BN, s.BK, s.NST, s.NTS, s.SPLIT, s.EX, s.F16); }
