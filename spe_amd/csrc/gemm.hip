// MFMA GEMM for every Linear / batched contraction on the SPE hot path (gfx950).
//
//   C[z][m][n] = act( alpha * sum_k opA(z)[m][k] * opB(z)[k][n] + bias[n] )
//
// fp32 tensors in HBM (A optionally bf16 bits); operands are rounded to bf16 while they are staged into LDS and
// multiplied with v_mfma_f32_16x16x32_bf16 (fp32 accumulate).  `precision == 1` selects the
// 3-term split (hi*hi + hi*lo + lo*hi) which recovers ~fp32 accuracy at 3x the MFMA work; it is
// what the 1e-3 parity mode uses.  Replaces the implicit ATen GEMMs behind nn.Linear / torch.bmm
// in reference models/cait.py:374-393, models/transformer.py:355-427, models/attention.py:353,375.
//
// One kernel, spe_gemm_kernel<T, TA, TB, SPLIT>, in the 12 instances of F32_GEMM_INSTANCES: block tile T x T x 32 with T = 128
// or 64 (spe_gemm_tile chooses), NT / NN / TN operand layouts, plain or split.  Block = 256 threads = 4 waves (2x2); wave tile
// T/2 x T/2 = (T/32)^2 MFMA tiles.  Register-staged double buffering: tile t+1 is in flight from HBM while tile t is multiplied.
//   load   load_tile<KC, R, MASK>: HBM -> registers for either contiguous index, one overload per element type (fp32; A stored
//          as bf16 bits).  Its contract when `vec` is set: rows are 16-B aligned (8-B for bf16) and padded to a multiple of 4 elements.
//   stage  stage_kc / stage_rc: the two register -> LDS layouts, both through store_bf16 (rounding, hi / lo split).
//   mult   the MFMAs are issued as (B-frag, A-frag), so they produce C^T tiles: each lane ends up with four CONSECUTIVE
//          columns of one row of C, which the epilogue stores as one 16-B quad.
//   store  alpha, bias, C2, activation; K splits add atomically or store their own slab.
#include "common.h"
#include "gemm_tiles.h"
#include <stdlib.h>

#define BK 32
#define LDSLD 40  // bf16 per LDS row: 32 + 8 pad -> 80 B rows keep ds_read_b128 16-B aligned

struct GemmArgs {
    const float* A; const float* B; float* C; float* C2; const float* bias;
    int M, N, K;
    long lda, ldb, ldc;
    int nb1;
    long sA0, sA1, sB0, sB1, sC0, sC1;
    float alpha;
    int act;       // 0 none, 1 relu, 2 gelu(erf)
    int splitk;    // >1: K split over workgroups (no bias/act): atomically added into pre-zeroed C, or, when
    long slab;     //     slab != 0, split z stores its partial tile into C + z*slab (reduced by the caller)
    int kt_per_split;
    int vecA, vecB;
    int xcd_bind;  // 0: plain tile order, 1: M-panels bound to XCDs, 2: N-panels bound to XCDs
    int a_bf16;    // A operand is stored as bf16 (spe_gemm_ex: a 16-bit tensor such as a transposed score tensor)
};

// ---- HBM -> registers -------------------------------------------------------------------
// All loads are UNCONDITIONAL on clamped addresses and masked afterwards: a branch around a load
// makes hipcc serialise it behind an s_waitcnt vmcnt(0) (one round trip per element).
// `vec` (wave-uniform): rows are 16-B aligned and padded to a multiple of 4 floats, so a float4
// at any 4-aligned in-row offset is inside the allocation even when it straddles the logical edge.
//
// Thread t of the 256 owns NI = R / 32 quads of an R x 32 operand tile: elements (s + STEP * i, c .. c + 3), i < NI, with c along the
// contiguous index of the tensor and s along the strided one; the loaders read them into v[i][0..3].
//   "KC", the contraction index is the contiguous one, X(r,k) = base[r*ld + k]:  k-quad t&7 of rows (t>>3) + 32 i
//   "RC", the row (m or n) index is contiguous, X(r,k) = base[k*ld + r]:  R = 128: row-quad t>>3 at k = (t&7)*4 + i (i < 4)
//                                                                         R =  64: row-quad (t>>3)&15 at k = (t&7)*4 + 2*(t>>7) + i (i < 2)
// The clamp-then-mask rule of both loaders: the strided index is clamped to its last valid value, a quad starts at
// min(c, (climit - 1) & ~3) (>= 0 since climit >= 1; without `vec` each element is clamped and loaded on its own), the mask tests the
// UNCLAMPED indices.  !MASK: interior tile, 16-B aligned rows: no clamps, no selects (the staging VALU work bounds this kernel).
template <bool KC, int R, bool MASK>
__device__ __forceinline__ void load_tile(const float* __restrict__ base, long ld, int row0, int nrows, int k0, int kend, bool vec, float v[4][4]) {
    const int t = threadIdx.x;
    constexpr int NI = R / 32, STEP = KC ? 32 : 1;
    const int c = KC ? k0 + (t & 7) * 4 : row0 + ((R == 128) ? (t >> 3) : ((t >> 3) & 15)) * 4;
    const int sRC = KC ? 0 : k0 + (t & 7) * 4 + ((R == 128) ? 0 : 2 * (t >> 7));
    auto s0 = [&]() { return KC ? row0 + (t >> 3) : sRC; };      // KC: formed where it is used, which keeps hipcc's instruction order
    const int climit = KC ? kend : nrows, slimit = KC ? nrows : kend;
    if (!MASK) {
        const float* p0 = base + (long)s0() * ld + c;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const float4 q = *reinterpret_cast<const float4*>(p0 + (long)(STEP * i) * ld);
            v[i][0] = q.x; v[i][1] = q.y; v[i][2] = q.z; v[i][3] = q.w;
        }
        return;
    }
    const int cq = min(c, (climit - 1) & ~3);
    if (vec) {      // the branch on `vec` stands outside the row loop: the rows' loads issue back to back
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int s = s0() + STEP * i;
            const float4 q = *reinterpret_cast<const float4*>(base + (long)min(s, slimit - 1) * ld + cq);
            const bool sv = s < slimit;
            v[i][0] = (sv && c + 0 < climit) ? q.x : 0.f; v[i][1] = (sv && c + 1 < climit) ? q.y : 0.f;
            v[i][2] = (sv && c + 2 < climit) ? q.z : 0.f; v[i][3] = (sv && c + 3 < climit) ? q.w : 0.f;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int s = s0() + STEP * i;
            const float* p = base + (long)min(s, slimit - 1) * ld;
            float q[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) q[j] = p[min(c + j, climit - 1)];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[i][j] = (s < slimit && c + j < climit) ? q[j] : 0.f;
        }
    }
}
// bf16-stored A operand: same mapping and rule, 8-B vector loads of 4 elements.  Here the branch on `vec` sits inside the row loop: no
// product path uses this overload, and its code is kept instruction for instruction.
template <bool KC, int R, bool MASK>
__device__ __forceinline__ void load_tile(const unsigned short* __restrict__ base, long ld, int row0, int nrows, int k0, int kend, bool vec, float v[4][4]) {
    const int t = threadIdx.x;
    constexpr int NI = R / 32, STEP = KC ? 32 : 1;
    const int c = KC ? k0 + (t & 7) * 4 : row0 + ((R == 128) ? (t >> 3) : ((t >> 3) & 15)) * 4;
    const int sRC = KC ? 0 : k0 + (t & 7) * 4 + ((R == 128) ? 0 : 2 * (t >> 7));
    auto s0 = [&]() { return KC ? row0 + (t >> 3) : sRC; };
    const int climit = KC ? kend : nrows, slimit = KC ? nrows : kend;
    if (!MASK) {
        const unsigned short* p0 = base + (long)s0() * ld + c;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const uint2 u = *reinterpret_cast<const uint2*>(p0 + (long)(STEP * i) * ld);
            v[i][0] = __uint_as_float(u.x << 16); v[i][1] = __uint_as_float(u.x & 0xffff0000u);
            v[i][2] = __uint_as_float(u.y << 16); v[i][3] = __uint_as_float(u.y & 0xffff0000u);
        }
        return;
    }
    const int cq = min(c, (climit - 1) & ~3);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int s = s0() + STEP * i;
        const unsigned short* p = base + (long)min(s, slimit - 1) * ld;
        unsigned short q[4];
        if (vec) {
            const uint2 u = *reinterpret_cast<const uint2*>(p + cq);
            q[0] = u.x & 0xffff; q[1] = u.x >> 16; q[2] = u.y & 0xffff; q[3] = u.y >> 16;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) q[j] = p[min(c + j, climit - 1)];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = (s < slimit && c + j < climit) ? spe_bf2f(q[j]) : 0.f;
    }
}

// ---- registers -> LDS (bf16 via v_cvt_pk_bf16_f32, optionally hi/lo split) -------------------
template <int N, bool SPLIT>
__device__ __forceinline__ void store_bf16(unsigned short* hi, unsigned short* lo, int off, const float (&x)[N]) {
    typedef __bf16 bf16xN_t __attribute__((ext_vector_type(N)));
    bf16xN_t h, l;
#pragma unroll
    for (int k = 0; k < N; ++k) h[k] = (__bf16)x[k];
    *reinterpret_cast<bf16xN_t*>(hi + off) = h;
    if (SPLIT) {
#pragma unroll
        for (int k = 0; k < N; ++k) l[k] = (__bf16)(x[k] - (float)h[k]);
        *reinterpret_cast<bf16xN_t*>(lo + off) = l;
    }
}
template <int R, bool SPLIT>
__device__ __forceinline__ void stage_kc(unsigned short* hi, unsigned short* lo, const float v[4][4]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < R / 32; ++i) store_bf16<4, SPLIT>(hi, lo, ((t >> 3) + 32 * i) * LDSLD + (t & 7) * 4, v[i]);
}
template <int R, bool SPLIT>
__device__ __forceinline__ void stage_rc(unsigned short* hi, unsigned short* lo, const float v[4][4]) {
    const int t = threadIdx.x;
    constexpr int NI = R / 32;       // the NI quads of a thread are consecutive k: row j takes element j of each
    const int off = ((R == 128) ? (t >> 3) : ((t >> 3) & 15)) * 4 * LDSLD + (t & 7) * 4 + ((R == 128) ? 0 : 2 * (t >> 7));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float x[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) x[i] = v[i][j];
        store_bf16<NI, SPLIT>(hi, lo, off + j * LDSLD, x);
    }
}

// TA: opA(m,k) = A[k*lda+m] (else A[m*lda+k]).  TB: opB(k,n) = B[n*ldb+k] (else B[k*ldb+n]).
template <int T, bool TA, bool TB, bool SPLIT>
__global__ __launch_bounds__(256) void spe_gemm_kernel(GemmArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned short smem[];
    constexpr int TILE = T * LDSLD;            // elements per operand tile
    constexpr int NF = T / 32;                 // 16x16 MFMA tiles per wave in each direction (wave tile = T/2)
    constexpr int WT = T / 2;
    constexpr int NPL = SPLIT ? 2 : 1;         // planes (hi, lo)
    // layout: [buf][A hi, A lo, B hi, B lo]
    auto sA = [&](int buf, int pl) { return smem + (buf * 2 * NPL + pl) * TILE; };
    auto sB = [&](int buf, int pl) { return smem + (buf * 2 * NPL + NPL + pl) * TILE; };

    const int tiles_m = (p.M + T - 1) / T, tiles_n = (p.N + T - 1) / T;
    int tm, tn;
    if (!tile_decode(p.xcd_bind, tiles_m, tiles_n, tm, tn)) return;      // XCD-aware tile order: gemm_tiles.h
    const int zb = blockIdx.z / p.splitk, zs = blockIdx.z % p.splitk;
    const int b0 = zb / p.nb1, b1 = zb % p.nb1;
    const float* A = p.a_bf16 ? nullptr : p.A + b0 * p.sA0 + b1 * p.sA1;
    const unsigned short* A16 = p.a_bf16 ? reinterpret_cast<const unsigned short*>(p.A) + b0 * p.sA0 + b1 * p.sA1 : nullptr;
    const float* B = p.B + b0 * p.sB0 + b1 * p.sB1;
    float* C = p.C + b0 * p.sC0 + b1 * p.sC1 + (long)zs * p.slab;
    float* C2 = p.C2 ? p.C2 + b0 * p.sC0 + b1 * p.sC1 : nullptr;

    const int m0 = tm * T, n0 = tn * T;
    const int ktiles = (p.K + BK - 1) / BK;
    const int kt_begin = zs * p.kt_per_split;
    int kt_end = kt_begin + p.kt_per_split; if (kt_end > ktiles) kt_end = ktiles;
    const int nt = kt_end - kt_begin;

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wm = w >> 1, wn = w & 1;
    const int fr = lane & 15, fk = (lane >> 4) * 8;

    f32x4_t acc[NF][NF];
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    float va[4][4], vb[4][4];
    // interior fast path: the whole operand tile is in bounds and rows are vector-aligned -> unmasked loads
    const bool rowsA_in = p.vecA && (m0 + T <= p.M), rowsB_in = p.vecB && (n0 + T <= p.N);
    auto gload = [&](int kt) {
        const int k0 = kt * BK;
        const bool k_in = k0 + BK <= p.K;
        auto loadA = [&](auto MASK, bool vec) {      // interior / masked is the outer choice, the element type the inner one, for A as for B
            if (p.a_bf16) load_tile<!TA, T, MASK()>(A16, p.lda, m0, p.M, k0, p.K, vec, va);
            else          load_tile<!TA, T, MASK()>(A, p.lda, m0, p.M, k0, p.K, vec, va);
        };
        if (rowsA_in && k_in) loadA(std::false_type(), true); else loadA(std::true_type(), p.vecA);
        if (rowsB_in && k_in) load_tile<TB, T, false>(B, p.ldb, n0, p.N, k0, p.K, true, vb);
        else                  load_tile<TB, T, true>(B, p.ldb, n0, p.N, k0, p.K, p.vecB, vb);
    };
    auto stage = [&](int buf) {
        if (TA) stage_rc<T, SPLIT>(sA(buf, 0), sA(buf, NPL - 1), va); else stage_kc<T, SPLIT>(sA(buf, 0), sA(buf, NPL - 1), va);
        if (TB) stage_kc<T, SPLIT>(sB(buf, 0), sB(buf, NPL - 1), vb); else stage_rc<T, SPLIT>(sB(buf, 0), sB(buf, NPL - 1), vb);
    };

    // one MFMA operand fragment: lane (fr, fk) reads 8 consecutive k of row `row` of an LDS plane
    auto frag = [&](const unsigned short* plane, int row) {
        return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8_t*>(plane + row * LDSLD + fk));
    };
    if (nt > 0) {
        gload(kt_begin);
        stage(0);
        __syncthreads();
        for (int t = 0; t < nt; ++t) {
            const int buf = t & 1;
            if (t + 1 < nt) gload(kt_begin + t + 1);
            bf16x8_t a[NF], b[NF];
#pragma unroll
            for (int i = 0; i < NF; ++i)
                a[i] = frag(sA(buf, 0), wm * WT + i * 16 + fr);
#pragma unroll
            for (int j = 0; j < NF; ++j)
                b[j] = frag(sB(buf, 0), wn * WT + j * 16 + fr);
#pragma unroll
            for (int i = 0; i < NF; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
            if (SPLIT) {
                bf16x8_t al[NF], bl[NF];
#pragma unroll
                for (int i = 0; i < NF; ++i)
                    al[i] = frag(sA(buf, 1), wm * WT + i * 16 + fr);
#pragma unroll
                for (int j = 0; j < NF; ++j)
                    bl[j] = frag(sB(buf, 1), wn * WT + j * 16 + fr);
#pragma unroll
                for (int i = 0; i < NF; ++i)
#pragma unroll
                    for (int j = 0; j < NF; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bl[j], a[i], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], al[i], acc[i][j], 0, 0, 0);
                    }
            }
            if (t + 1 < nt) stage(buf ^ 1);
            __syncthreads();
        }
    }

    // ---- epilogue.  The MFMAs were issued as (B-frag, A-frag), i.e. they produced C^T tiles, so
    // acc[i][j][r] = C[m0 + wm*T/2 + i*16 + (lane&15)][n0 + wn*T/2 + j*16 + (lane>>4)*4 + r]:
    // every lane owns 4 consecutive columns of one row -> one 16-B store per tile.
    const bool vst = ((p.ldc & 3) == 0) && ((reinterpret_cast<uintptr_t>(C) & 15) == 0) &&
                     (!C2 || (reinterpret_cast<uintptr_t>(C2) & 15) == 0);
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const int n = n0 + wn * WT + j * 16 + (lane >> 4) * 4;
        if (n >= p.N) continue;
        float bv[4] = {0.f, 0.f, 0.f, 0.f};
        if (p.bias && p.splitk == 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) bv[r] = p.bias[min(n + r, p.N - 1)];
        }
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int m = m0 + wm * WT + i * 16 + fr;
            if (m >= p.M) continue;
            const long off = (long)m * p.ldc + n;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = acc[i][j][r] * p.alpha;
            if (p.splitk > 1) {
                if (p.slab != 0) {      // private slab of this split: plain (vector) stores, zeros if the split was empty
                    if (vst && n + 3 < p.N) *reinterpret_cast<float4*>(C + off) = make_float4(v[0], v[1], v[2], v[3]);
                    else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) if (n + r < p.N) C[off + r] = v[r];
                    }
                } else if (nt > 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) if (n + r < p.N) atomicAdd(C + off + r, v[r]);
                }
                continue;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += bv[r];
            const bool full = vst && (n + 3 < p.N);
            if (C2) {
                if (full) *reinterpret_cast<float4*>(C2 + off) = make_float4(v[0], v[1], v[2], v[3]);
                else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) if (n + r < p.N) C2[off + r] = v[r];
                }
            }
            if (p.act == 1) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
            } else if (p.act == 2) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = spe_gelu_erf(v[r]);
            }
            if (full) *reinterpret_cast<float4*>(C + off) = make_float4(v[0], v[1], v[2], v[3]);
            else {
#pragma unroll
                for (int r = 0; r < 4; ++r) if (n + r < p.N) C[off + r] = v[r];
            }
        }
    }
}

// Tile choice: every GEMM of this model is HBM/latency bound, so what matters is enough workgroups in flight.
// 128x128 tiles when they already give >= 1 workgroup per CU (split-K slices count), 64x64 tiles (4x the
// workgroups, half the registers, twice the L2 re-reads) otherwise and for skinny outputs (N <= 64: the per-head attention contractions).
extern "C" int spe_gemm_tile(int M, int N, int nbatch) {
    static int forced = -1;
    if (forced < 0) forced = SPE_KNOB("SPE_GEMM_TILE", 0);
    if (forced == 64 || forced == 128) return forced;
    const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128) * nbatch;
    return (t128 >= 256 && N > 64 && M > 64) ? 128 : 64;
}

// The argument checks and every launch choice of spe_gemm_ex, in one place: the launcher fills GemmArgs and the grid from the answer,
// spe_gemm_f32_plan hands it to tests and tools (tests/test_f32_gemm_plan_cpu.py pins it).  Status as the launcher returns it; 1 = nothing
// to do (an empty M, N or batch: the launcher returns 0 without a launch).  epilogue: bias, activation or C2 asked for.  a_mod16 / b_mod16:
// the operand addresses modulo 16.
struct GemmPlan { int T, TA, TB, SPLIT, splitk, kt_per_split; long slab; int vecA, vecB, xcd_bind, grid; };
static int gemm_f32_select(int M, int N, int K, long lda, long ldb, long ldc, int transA, int transB, int batch0, int batch1,
                           long sA0, long sA1, long sB0, long sB1, long sC0, long sC1, int splitk, int precision, int a_bf16,
                           int epilogue, int a_mod16, int b_mod16, GemmPlan* s) {
    if (M <= 0 || N <= 0 || K <= 0 || batch0 <= 0 || batch1 <= 0) return K <= 0 && M > 0 && N > 0 ? -4 : 1;
    if (transA && transB) return -2;  // not needed on this path
    s->TA = transA ? 1 : 0; s->TB = transB ? 1 : 0; s->SPLIT = precision == 1;
    s->slab = 0;
    const int ktiles = (K + BK - 1) / BK;
    if (splitk < 0) {           // slab mode: C must hold |splitk| slabs (M*ldc floats; batched: the extent of all batches)
        splitk = -splitk;
        s->slab = (batch0 * batch1 == 1) ? (long)M * ldc
                                         : ((((long)(batch0 - 1) * sC0 + (long)(batch1 - 1) * sC1 + (long)(M - 1) * ldc + N) + 3) & ~3L);
        if (splitk > ktiles) return -5;
    }
    if (splitk < 1) splitk = 1;
    if (splitk > ktiles) splitk = ktiles > 0 ? ktiles : 1;
    s->kt_per_split = (ktiles + splitk - 1) / splitk;
    s->splitk = splitk;
    if (splitk > 1 && epilogue) return -3;
    auto m4 = [](long v) { return (v & 3) == 0; };
    // float4 loads need 16-B aligned rows; quads that straddle an edge fall back to scalars
    s->vecA = ((a_bf16 ? (a_mod16 & 7) : (a_mod16 & 15)) == 0) && m4(lda) && m4(sA0) && m4(sA1);
    s->vecB = ((b_mod16 & 15) == 0) && m4(ldb) && m4(sB0) && m4(sB1);
    s->T = spe_gemm_tile(M, N, batch0 * batch1 * splitk);
    const TileOrder order = tile_order(M, N, (M + s->T - 1) / s->T, (N + s->T - 1) / s->T);
    s->xcd_bind = order.xcd_bind;
    s->grid = order.grid;
    return 0;
}

// ---- the instances that exist: X(T, TA, TB, SPLIT).  gemm_f32_select names nothing else (it refuses TA && TB); the launcher's switch is
// generated from this list.
#define F32_GEMM_INSTANCES(X)                                                                                       \
    X(64, false, true, false)  X(64, false, true, true)  X(64, false, false, false)  X(64, false, false, true)      \
    X(64, true, false, false)  X(64, true, false, true)  X(128, false, true, false)  X(128, false, true, true)      \
    X(128, false, false, false) X(128, false, false, true) X(128, true, false, false) X(128, true, false, true)
constexpr int f32_gemm_key(int T, int TA, int TB, int SPLIT) { return ((T * 2 + TA) * 2 + TB) * 2 + SPLIT; }

template <int T, bool TA, bool TB, bool SPLIT>
static int launch_gemm(const GemmArgs& p, int grid_x, int nbatch, hipStream_t stream) {
    constexpr int smem = 2 * 2 * (SPLIT ? 2 : 1) * T * LDSLD * (int)sizeof(unsigned short);
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&spe_gemm_kernel<T, TA, TB, SPLIT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, smem);
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    dim3 grid(grid_x, 1, nbatch * p.splitk);
    hipLaunchKernelGGL((spe_gemm_kernel<T, TA, TB, SPLIT>), grid, dim3(256), smem, stream, p);
    SPE_CHECK_LAUNCH();
    return 0;
}

// C-ABI: see include/spe_hip.h (spe_gemm_f32_plan).  Host only: the selection for a problem, no device needed.
extern "C" int spe_gemm_f32_plan(int M, int N, int K, long lda, long ldb, long ldc, int transA, int transB, int batch0, int batch1,
                                 long sA0, long sA1, long sB0, long sB1, long sC0, long sC1, int splitk, int precision, int a_bf16,
                                 int epilogue, int a_mod16, int b_mod16, long* v) {
    GemmPlan s;
    const int rc = gemm_f32_select(M, N, K, lda, ldb, ldc, transA, transB, batch0, batch1, sA0, sA1, sB0, sB1, sC0, sC1, splitk, precision,
                                   a_bf16, epilogue, a_mod16, b_mod16, &s);
    if (rc < 0) return rc;
    if (rc > 0) s = GemmPlan{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};             // nothing to do: no kernel runs
    if (v) { v[0] = s.T; v[1] = s.TA; v[2] = s.TB; v[3] = s.SPLIT; v[4] = s.splitk; v[5] = s.kt_per_split; v[6] = s.slab;
             v[7] = s.vecA; v[8] = s.vecB; v[9] = s.xcd_bind; v[10] = s.grid; }
    return 0;
}

// C-ABI: see include/spe_hip.h (spe_gemm_ex): the contraction with the A operand optionally stored as bf16 (a_bf16 = 1; lda / sA* in elements).
extern "C" int spe_gemm_ex(const void* A, int a_bf16, const float* B, float* C, const float* bias, float* C2,
                           int M, int N, int K, long lda, long ldb, long ldc, int transA, int transB,
                           int batch0, int batch1, long sA0, long sA1, long sB0, long sB1, long sC0, long sC1,
                           float alpha, int act, int splitk, int precision, hipStream_t stream) {
    GemmPlan s;
    const int rc = gemm_f32_select(M, N, K, lda, ldb, ldc, transA, transB, batch0, batch1, sA0, sA1, sB0, sB1, sC0, sC1, splitk, precision,
                                   a_bf16, act != 0 || C2 != nullptr || bias != nullptr, (int)(reinterpret_cast<uintptr_t>(A) & 15),
                                   (int)(reinterpret_cast<uintptr_t>(B) & 15), &s);
    if (rc != 0) return rc > 0 ? 0 : rc;
    GemmArgs p;
    p.A = reinterpret_cast<const float*>(A); p.a_bf16 = a_bf16; p.B = B; p.C = C; p.C2 = C2; p.bias = bias;
    p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    p.nb1 = batch1; p.sA0 = sA0; p.sA1 = sA1; p.sB0 = sB0; p.sB1 = sB1; p.sC0 = sC0; p.sC1 = sC1;
    p.alpha = alpha; p.act = act; p.slab = s.slab;
    p.kt_per_split = s.kt_per_split; p.splitk = s.splitk;
    p.vecA = s.vecA; p.vecB = s.vecB; p.xcd_bind = s.xcd_bind;
    switch (f32_gemm_key(s.T, s.TA, s.TB, s.SPLIT)) {
#define F32_GEMM_CASE(T, TA, TB, SPLIT) \
    case f32_gemm_key(T, TA, TB, SPLIT): return launch_gemm<T, TA, TB, SPLIT>(p, s.grid, batch0 * batch1, stream);
        F32_GEMM_INSTANCES(F32_GEMM_CASE)
#undef F32_GEMM_CASE
    }
    return -2;          // unreachable while gemm_f32_select names members of the list (tests/test_f32_gemm_plan_cpu.py)
}

// C-ABI: see include/spe_hip.h (spe_gemm_f32).
extern "C" int spe_gemm_f32(const float* A, const float* B, float* C, const float* bias, float* C2,
                            int M, int N, int K, long lda, long ldb, long ldc, int transA, int transB,
                            int batch0, int batch1, long sA0, long sA1, long sB0, long sB1, long sC0, long sC1,
                            float alpha, int act, int splitk, int precision, hipStream_t stream) {
    return spe_gemm_ex(A, 0, B, C, bias, C2, M, N, K, lda, ldb, ldc, transA, transB, batch0, batch1, sA0, sA1, sB0, sB1, sC0, sC1,
                       alpha, act, splitk, precision, stream);
}
