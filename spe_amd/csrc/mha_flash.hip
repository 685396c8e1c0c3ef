// Flash-style multi-head attention for the encoder / decoder / cross-attention of the SPE transformer
// (reference models/attention.py:277-383 `multi_head_attention_forward`: softmax(scale q k^T + key_padding_mask),
// dropout on the probabilities, . v, with q/k head dim != v head dim in the decoder cross-attention; and the
// nn.MultiheadAttention core of the encoder, models/transformer.py:275-277) - forward and backward without ever
// writing the [B,H,Lq,Lk] score tensor (the materialising path moves 4 such fp32 tensors per layer: 53 MB each for
// the decoder's 200 x 4150 cross-attention, 1.1 GB each for an encoder layer at N = 4150).
//
// Element formats as in the talking-heads kernels (attn_pack.h, attn_flash.hip): the FORWARD operands - q * scale * log2(e), k (Qf, Kf), v (V16) and the probabilities of
// the P.V product - are O(1) and go through fp16 (3 more mantissa bits than bf16, same size and MFMA rate: the bf16 version of
// this kernel alone cost 1.1e-3 of pred_logits at cfg2, tools/error_budget.py); the backward recomputes S from the same fp16
// fragments and keeps bf16 wherever a gradient is an operand (Vf.dOf, P^T dO16, dS K16, dS^T Q16).
//
// Same building blocks as the talking-heads kernels: 16-bit MFMA operand fragments packed by spe_attn_pack_multi, the
// swapped orientation S^T = K_tile . Q_tile^T so that a lane owns one query and 4 keys, and the 16x16 C tile reused
// directly as the B operand of v_mfma_f32_16x16x16_bf16 for the second contraction (P.V, dS.K, P^T.dO, dS^T.Q).
// A wave owns one 16-row tile of the non-streamed axis; the 4 waves of a workgroup share the streamed tile's fragments
// through a double-buffered LDS stage:
//   forward   item = (b, h, 16-query tile, key chunk): online softmax in the log2 domain, O += P_drop V; partial
//             (O, m, l) per chunk, combined by mha_merge_kernel (few query tiles -> many key chunks keep the chip busy)
//   backward  dq  item = (b, h, query tile, key chunk): dS = P (keep dPd - D), dQ = dS K into the chunk's own slab (the caller
//             adds the slabs in chunk order), or straight into dq when there is one chunk
//             dkv item = (b, h, 16-key tile): loops over all query tiles in the non-swapped orientation, dV += Pd^T dO,
//             dK += dS^T Q, plain stores
// Head dims are run-time (<= 96 for q/k, <= 64 for v); fragments are full 32-wide steps (kind 2 of spe_attn_pack_multi).
//
// The stage (MhaStream, mha_fetch, mha_commit).  A kernel names the operands it streams - forward: Kf, V16; dq: Kf, Vf, K16; dkv: Qf, dOf,
// Q16, dO16 and the 48-float LSE / D / NaN-marker row - each as (global array, first tile, elements per tile = 64 per fragment unit, LDS
// array [2][..]).  Per streamed tile and in this order: fetch tile t + 1 into registers (thread tid holds element tid, and element
// tid + 256 of a five- or six-unit tile), compute on buffer t & 1, commit the registers to the other buffer, one barrier.  Buffer 0 is
// filled the same way before the loop.  Nothing but mha_commit writes the stage, nothing reads a buffer between its commit and the barrier.
//
// The store rule (mha_store_tiles: dq, dk, dv).  A lane holds 4 consecutive columns of its row: one float4 when the row length is a
// multiple of 4 (the quad is then inside the row and aligned), scalar stores of the columns below the row length otherwise.  Every
// output element is written exactly once, by a plain store - no atomics, nothing to zero beforehand.
#include "attn_flash_common.h"

#define MHA_DSK 3          // max 32-steps of the q/k head dim
#define MHA_DSV 2          // max 32-steps of the v head dim
#define MHA_DVT 4          // max 16-tiles of the v head dim
#define MHA_DKT 6          // max 16-tiles of the q/k head dim
#define MHA_LN2 0.6931471805599453f
#ifndef MHA_TARGET
#define MHA_TARGET 1024    // developer knob (tools/ab.py): workgroups spe_mha_plan aims at
#endif

struct MhaArgs {
    const flu32x4_t* Qf; const flu32x4_t* Kf; const flu32x4_t* Vf; const flu32x4_t* dOf;   // 32-wide fragment records [B,H,nt][ds][64]
    const uint2* V16; const uint2* K16; const uint2* Q16; const uint2* dO16;            // 16-wide fragments [B,H,nt][dt][64]
    const unsigned char* mask;                 // [B, Lk] key padding (1 = padded) or null
    float* Opart; float* ML;                   // forward partials: [item][dvt][64][4], [item][16][2]
    const float* LSE; const float* Dd;         // [B,H,Lq] log2-domain log-sum-exp, D = rowsum(dO . O)
    float* dq; float* dk; float* dv;           // [B,L,H,d] fp32, overwritten (dq only when nch == 1)
    float* dq_ws;                              // nch > 1: [nch][B,Lq,H,dk] slabs, one private partial dq per key chunk
    unsigned long long* keepbits;              // dropout keep flags [B*H*ntq*ntk][4] (written by the forward, p_drop > 0)
    int B, H, Lq, Lk, dk_dim, dv_dim, ntq, ntk, nch, ch_len;
    float scale, p_drop; uint64_t seed, offset;
};

__device__ __forceinline__ flu32x4_t mha_frag(const flu32x4_t* base, long rec, int ds, int st, int lane) {
    return base[(rec * ds + st) * 64 + lane];
}
// second contraction: a 16-wide fragment of the stage (uint2) against the wave's own C tile packed to 16 bits.  F16: P.V of the forward
// (probabilities relative to the running maximum are in [0, 1]: fl_pack4_f16, plain conversion); bf16 (fl_pack4<false>): every gradient
template <bool F16>
__device__ __forceinline__ f32x4_t mha_mfma16(uint2 a, fls16x4_t b, f32x4_t c) {
    return fl_mfma16<F16>(__builtin_bit_cast(fls16x4_t, a), b, c);
}

// Workgroup = 4 waves working on 4 consecutive tiles of the NON-streamed axis (query tiles in the forward / dQ
// kernels, key tiles in the dK/dV kernel); the fragments of the streamed tile are fetched once per workgroup into a
// double-buffered LDS stage (one barrier per step) instead of once per wave: a quarter of the L2 traffic.
// One streamed operand: tile t is the n elements (64 per fragment unit) at g + (rec0 + t) * n, its stage lds[2][ROW].  The 256 threads hold one
// element each in r[0]; a tile of five or six units (the 16-wide q / k fragments above head dim 64) has its elements 256.. in r[1].
template <typename T, int ROW>
struct MhaStream {
    const T* g; long rec0; int n; T (*lds)[ROW];
    T r[ROW > 256 ? 2 : 1];
    __device__ __forceinline__ MhaStream(const T* g_, long rec0_, int n_, T (*lds_)[ROW]) : g(g_), rec0(rec0_), n(n_), lds(lds_) {}
    __device__ __forceinline__ void fetch(int t, int tid) {
        if (tid < n) r[0] = g[(rec0 + t) * n + tid];
        if constexpr (ROW > 256) { if (tid + 256 < n) r[1] = g[(rec0 + t) * n + tid + 256]; }
    }
    __device__ __forceinline__ void commit(int buf, int tid) const {
        if (tid < n) lds[buf][tid] = r[0];
        if constexpr (ROW > 256) { if (tid + 256 < n) lds[buf][tid + 256] = r[1]; }
    }
};
// the two steps of the stage, over the operands a kernel streams (in the order given)
template <typename... S> __device__ __forceinline__ void mha_fetch(int t, int tid, S&... s) { (s.fetch(t, tid), ...); }
template <typename... S> __device__ __forceinline__ void mha_commit(int buf, int tid, const S&... s) { (s.commit(buf, tid), ...); }

// The one first contraction: sum over the ns 32-wide head-dim steps of (streamed tile in the stage) . (the wave's own fragments), one accumulate
// chain in step order.  F16: the scores K.Q^T / Q.K^T of all three kernels; bf16: dP = V.dO^T / dO.V^T of the backward.
template <bool F16, int NS>
__device__ __forceinline__ f32x4_t mha_dot(const flu32x4_t* stage, const flu32x4_t (&own)[NS], int ns, int lane) {
    f32x4_t s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < NS; ++st)
        if (st < ns) s = fl_mfma32<F16>(stage[st * 64 + lane], own[st], s);
    return s;
}
// a key takes part: inside Lk and not padded
__device__ __forceinline__ bool mha_key_ok(const MhaArgs& a, int b, int key) {
    return key < a.Lk && !(a.mask && a.mask[(long)b * a.Lk + min(key, a.Lk - 1)]);
}
// Backward, both orientations: the keep words of tile (qt, kt) - all ones without dropout - and dS = P (keep dP - D) of one element
__device__ __forceinline__ void mha_keep_words(const MhaArgs& a, long tile, unsigned long long (&kbits)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) kbits[r] = ~0ull;
    if (a.p_drop > 0.f) {
#pragma unroll
        for (int r = 0; r < 4; ++r) kbits[r] = a.keepbits[tile * 4 + r];
    }
}
__device__ __forceinline__ float mha_ds(float p, float dp, float keep, float D) { return p * (dp * keep - D); }

// keep bits of a 16x16 tile, written by the forward: word r, bit l = keep flag of the element lane l holds in register r
// of the swapped-orientation tile (query l & 15, key 4*(l >> 4) + r)
__device__ __forceinline__ float mha_keep_swapped(const unsigned long long* kb, int lane, int r, float inv) {
    return ((kb[r] >> lane) & 1ull) ? inv : 0.f;
}
// the same element seen from the non-swapped orientation: lane holds key (lane & 15) and query 4*(lane >> 4) + r
__device__ __forceinline__ float mha_keep_plain(const unsigned long long* kb, int lane, int r, float inv) {
    const int key = lane & 15, ql = 4 * (lane >> 4) + r;
    return ((kb[key & 3] >> (ql + 16 * (key >> 2))) & 1ull) ? inv : 0.f;
}

// The one result store of the backward (dq_store, dk_store, dv_store): f * g, the [16 rows][dim] accumulator tiles of a wave, to the lane's row
// `dst` of a [.., H, dim] fp32 tensor.  A lane holds columns dc .. dc + 3 of tile d: one float4 (:vector) where dim % 4 == 0 - then the
// quad is inside the row and 16-B aligned - and the columns below dim one by one (:scalar) otherwise.
template <int NT>
__device__ __forceinline__ void mha_store_tiles(float* dst, const f32x4_t (&g)[NT], int nt, int dim, float f, int lane) {
#pragma unroll
    for (int d = 0; d < NT; ++d)
        if (d < nt) {
            const int dc = d * 16 + 4 * (lane >> 4);
            if (dc + 3 < dim && (dim & 3) == 0) {
                *reinterpret_cast<float4*>(dst + dc) = make_float4(g[d][0] * f, g[d][1] * f, g[d][2] * f, g[d][3] * f);
                continue;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (dc + r < dim) dst[dc + r] = g[d][r] * f;
        }
}

// ---- forward ---------------------------------------------------------------------------------------
// TDK / TDV: head dims fixed at compile time (0: taken from the arguments - every step guard is then a branch around an
// MFMA; the instantiated pairs fold them away: 131 -> 12 branches, 192 -> ~120 registers in the dK/dV kernel)
template <int TDK, int TDV>
__global__ __launch_bounds__(256) void mha_fwd_kernel(MhaArgs a) {
    __shared__ flu32x4_t sK[2][MHA_DSK * 64];
    __shared__ uint2 sV[2][MHA_DVT * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
    const int nqg = (a.ntq + 3) / 4;
    const int ch = blockIdx.x % a.nch; const int qg = (blockIdx.x / a.nch) % nqg; const long bh = blockIdx.x / ((long)a.nch * nqg);
    const int b = (int)(bh / a.H);
    const int dkd = TDK ? TDK : a.dk_dim, dvd = TDV ? TDV : a.dv_dim;
    const int dsk = (dkd + 31) / 32, dvt = (dvd + 15) / 16;
    const int qt = qg * 4 + wave;
    const bool active = qt < a.ntq;
    const int qtc = min(qt, a.ntq - 1);
    const int q = qtc * 16 + (lane & 15);
    const long ld4 = (a.Lk + 3) & ~3;

    flu32x4_t qf[MHA_DSK];
#pragma unroll
    for (int st = 0; st < MHA_DSK; ++st) qf[st] = (st < dsk) ? mha_frag(a.Qf, bh * a.ntq + qtc, dsk, st, lane) : (flu32x4_t){0u, 0u, 0u, 0u};
    f32x4_t o[MHA_DVT];
#pragma unroll
    for (int d = 0; d < MHA_DVT; ++d) o[d] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    const int kt0 = ch * a.ch_len, kt1 = min(kt0 + a.ch_len, a.ntk);
    MhaStream<flu32x4_t, MHA_DSK * 64> stK(a.Kf, bh * a.ntk, dsk * 64, sK);
    MhaStream<uint2, MHA_DVT * 64> stV(a.V16, bh * a.ntk, dvt * 64, sV);
    mha_fetch(kt0, tid, stK, stV); mha_commit(0, tid, stK, stV);
    __syncthreads();
    for (int kt = kt0; kt < kt1; ++kt) {
        const int buf = (kt - kt0) & 1;
        if (kt + 1 < kt1) mha_fetch(kt + 1, tid, stK, stV);
        const f32x4_t s = mha_dot<true>(sK[buf], qf, dsk, lane);
        const int kb = kt * 16 + 4 * (lane >> 4);
        float sv[4], tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sv[r] = mha_key_ok(a, b, kb + r) ? s[r] : -INFINITY;
            tmax = fmaxf(tmax, sv[r]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));           // max over the tile's 16 keys of this lane's query
        const float mn = fmaxf(m, tmax);
        // branch-free (the MFMAs below must run for the whole wave): m = -inf means o = l = 0, so alpha is moot
        const float alpha = (m > -INFINITY) ? __builtin_amdgcn_exp2f(m - mn) : 0.f;
        float p[4], pd[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { p[r] = (sv[r] > -INFINITY) ? __builtin_amdgcn_exp2f(sv[r] - mn) : 0.f; pd[r] = p[r]; }
        if (a.p_drop > 0.f) {
            // one Philox block per lane: element index (row * ld4 + key), 4 consecutive keys, ld4 % 4 == 0
            float ks[4];
            spe_drop_scale4(a.seed, a.offset, (uint64_t)((bh * a.Lq + min(q, a.Lq - 1)) * ld4 + kb), a.p_drop, ks);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pd[r] *= ks[r];
                const unsigned long long w = __ballot(ks[r] != 0.f);
                if (active && lane == r) a.keepbits[((bh * a.ntq + qt) * a.ntk + kt) * 4 + r] = w;
            }
        }
        l = l * alpha + (p[0] + p[1] + p[2] + p[3]);
        m = mn;
#pragma unroll
        for (int d = 0; d < MHA_DVT; ++d)
            if (d < dvt) {
                o[d] *= alpha;
                o[d] = mha_mfma16<true>(sV[buf][d * 64 + lane], fl_pack4_f16(pd[0], pd[1], pd[2], pd[3]), o[d]);
            }
        if (kt + 1 < kt1) mha_commit(buf ^ 1, tid, stK, stV);
        __syncthreads();
    }
    if (!active) return;
    // partials: O (relative to m), and per query m and the lane-group-summed l
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const long item = (bh * a.ntq + qt) * a.nch + ch;
#pragma unroll
    for (int d = 0; d < MHA_DVT; ++d)
        if (d < dvt) *reinterpret_cast<f32x4_t*>(a.Opart + ((item * dvt + d) * 64 + lane) * 4) = o[d];
    if (lane < 16) { a.ML[(item * 16 + lane) * 2] = m; a.ML[(item * 16 + lane) * 2 + 1] = l; }
}

// O[b, q, h, :] = sum_c Opart_c * 2^(m_c - M) / L ; LSE = M + log2(L)
__global__ __launch_bounds__(256) void mha_merge_kernel(const float* __restrict__ Opart, const float* __restrict__ ML, float* __restrict__ O,
                                                        float* __restrict__ LSE, int B, int H, int Lq, int ntq, int nch, int dv_dim) {
    const int dvt = (dv_dim + 15) / 16;
    const long total = (long)B * H * ntq * dvt * 64;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int lane = (int)(i & 63); long t = i >> 6;
    const int d = (int)(t % dvt); t /= dvt;
    const int qt = (int)(t % ntq); const long bh = t / ntq;
    const int b = (int)(bh / H), h = (int)(bh % H);
    const int ql = lane & 15, q = qt * 16 + ql;
    if (q >= Lq) return;
    const long item0 = (bh * ntq + qt) * nch;
    float M = -INFINITY;
    for (int c = 0; c < nch; ++c) M = fmaxf(M, ML[((item0 + c) * 16 + ql) * 2]);
    float L = 0.f; f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < nch; ++c) {
        const float mc = ML[((item0 + c) * 16 + ql) * 2];
        if (mc == -INFINITY) continue;
        const float w = __builtin_amdgcn_exp2f(mc - M);
        L += ML[((item0 + c) * 16 + ql) * 2 + 1] * w;
        acc += *reinterpret_cast<const f32x4_t*>(Opart + (((item0 + c) * dvt + d) * 64 + lane) * 4) * w;
    }
    const float inv = 1.f / L;
    const int dc = d * 16 + 4 * (lane >> 4);
    float* dst = O + ((long)b * Lq + q) * ((long)H * dv_dim) + (long)h * dv_dim;
#pragma unroll
    for (int r = 0; r < 4; ++r) if (dc + r < dv_dim) dst[dc + r] = acc[r] * inv;
    if (d == 0 && lane < 16) LSE[bh * Lq + q] = M + __builtin_amdgcn_logf(L);
}

// ---- backward: dQ ------------------------------------------------------------------------------------
template <int TDK, int TDV>
__global__ __launch_bounds__(256) void mha_bwd_dq_kernel(MhaArgs a) {
    __shared__ flu32x4_t sK[2][MHA_DSK * 64];
    __shared__ flu32x4_t sV[2][MHA_DSV * 64];
    __shared__ uint2 sK16[2][MHA_DKT * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
    const int nqg = (a.ntq + 3) / 4;
    const int ch = blockIdx.x % a.nch; const int qg = (blockIdx.x / a.nch) % nqg; const long bh = blockIdx.x / ((long)a.nch * nqg);
    const int b = (int)(bh / a.H), h = (int)(bh % a.H);
    const int dkd = TDK ? TDK : a.dk_dim, dvd = TDV ? TDV : a.dv_dim;
    const int dsk = (dkd + 31) / 32, dsv = (dvd + 31) / 32, dkt = (dkd + 15) / 16;
    const int qt = qg * 4 + wave;
    const bool active = qt < a.ntq;
    const int qtc = min(qt, a.ntq - 1);
    const int q = qtc * 16 + (lane & 15);
    const bool qv = active && q < a.Lq;
    const float inv_keep = 1.f / (1.f - a.p_drop);

    flu32x4_t qf[MHA_DSK], dof[MHA_DSV];
#pragma unroll
    for (int st = 0; st < MHA_DSK; ++st) qf[st] = (st < dsk) ? mha_frag(a.Qf, bh * a.ntq + qtc, dsk, st, lane) : (flu32x4_t){0u, 0u, 0u, 0u};
#pragma unroll
    for (int st = 0; st < MHA_DSV; ++st) dof[st] = (st < dsv) ? mha_frag(a.dOf, bh * a.ntq + qtc, dsv, st, lane) : (flu32x4_t){0u, 0u, 0u, 0u};
    const float lse = qv ? a.LSE[bh * a.Lq + q] : 0.f, Dq = qv ? a.Dd[bh * a.Lq + q] : 0.f;
    f32x4_t g[MHA_DKT];
#pragma unroll
    for (int d = 0; d < MHA_DKT; ++d) g[d] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    const int kt0 = ch * a.ch_len, kt1 = min(kt0 + a.ch_len, a.ntk);
    MhaStream<flu32x4_t, MHA_DSK * 64> stK(a.Kf, bh * a.ntk, dsk * 64, sK);
    MhaStream<flu32x4_t, MHA_DSV * 64> stV(a.Vf, bh * a.ntk, dsv * 64, sV);
    MhaStream<uint2, MHA_DKT * 64> stK16(a.K16, bh * a.ntk, dkt * 64, sK16);
    mha_fetch(kt0, tid, stK, stV, stK16); mha_commit(0, tid, stK, stV, stK16);
    __syncthreads();
    for (int kt = kt0; kt < kt1; ++kt) {
        const int buf = (kt - kt0) & 1;
        if (kt + 1 < kt1) mha_fetch(kt + 1, tid, stK, stV, stK16);
        const f32x4_t s = mha_dot<true>(sK[buf], qf, dsk, lane), dp = mha_dot<false>(sV[buf], dof, dsv, lane);
        unsigned long long kbits[4];
        mha_keep_words(a, (bh * a.ntq + qtc) * a.ntk + kt, kbits);
        const int kb = kt * 16 + 4 * (lane >> 4);
        float ds[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = (qv && mha_key_ok(a, b, kb + r)) ? __builtin_amdgcn_exp2f(s[r] - lse) : 0.f;
            const float keep = (a.p_drop > 0.f) ? mha_keep_swapped(kbits, lane, r, inv_keep) : 1.f;
            ds[r] = mha_ds(p, dp[r], keep, Dq);
        }
        const fls16x4_t db = fl_pack4<false>(ds[0], ds[1], ds[2], ds[3]);
#pragma unroll
        for (int d = 0; d < MHA_DKT; ++d)
            if (d < dkt) g[d] = mha_mfma16<false>(sK16[buf][d * 64 + lane], db, g[d]);
        if (kt + 1 < kt1) mha_commit(buf ^ 1, tid, stK, stV, stK16);
        __syncthreads();
    }
    if (!qv) return;
    // scale * g, lane = (query, 4 consecutive d): into the chunk's private slab (dq_slab; the caller adds the slabs in chunk order),
    // or straight into dq when one chunk covers every key.  spe_mha_bwd refuses nch > 1 without slabs.
    float* dst = (a.nch > 1 ? a.dq_ws + (long)ch * a.B * a.Lq * a.H * dkd : a.dq) + (((long)b * a.Lq + q) * a.H + h) * dkd;
    mha_store_tiles(dst, g, dkt, dkd, a.scale, lane);
}

// ---- backward: dK, dV ----------------------------------------------------------------------------------
template <int TDK, int TDV>
__global__ __launch_bounds__(256) void mha_bwd_dkv_kernel(MhaArgs a) {
    __shared__ flu32x4_t sQ[2][MHA_DSK * 64];
    __shared__ flu32x4_t sdO[2][MHA_DSV * 64];
    __shared__ uint2 sQ16[2][MHA_DKT * 64];
    __shared__ uint2 sdO16[2][MHA_DVT * 64];
    __shared__ float sLD[2][48];                           // LSE[16], D[16] of the query tile, and what P is at an excluded key [16]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
    const int nkg = (a.ntk + 3) / 4;
    const int kg = blockIdx.x % nkg; const long bh = blockIdx.x / nkg;
    const int b = (int)(bh / a.H), h = (int)(bh % a.H);
    const int dkd = TDK ? TDK : a.dk_dim, dvd = TDV ? TDV : a.dv_dim;
    const int dsk = (dkd + 31) / 32, dsv = (dvd + 31) / 32, dkt = (dkd + 15) / 16, dvt = (dvd + 15) / 16;
    const int kt = kg * 4 + wave;
    const bool active = kt < a.ntk;
    const int ktc = min(kt, a.ntk - 1);
    const int key = ktc * 16 + (lane & 15);                // non-swapped orientation: a lane owns one key and 4 queries
    const bool kv = active && mha_key_ok(a, b, key);
    const float inv_keep = 1.f / (1.f - a.p_drop);

    flu32x4_t kf[MHA_DSK], vf[MHA_DSV];
#pragma unroll
    for (int st = 0; st < MHA_DSK; ++st) kf[st] = (st < dsk) ? mha_frag(a.Kf, bh * a.ntk + ktc, dsk, st, lane) : (flu32x4_t){0u, 0u, 0u, 0u};
#pragma unroll
    for (int st = 0; st < MHA_DSV; ++st) vf[st] = (st < dsv) ? mha_frag(a.Vf, bh * a.ntk + ktc, dsv, st, lane) : (flu32x4_t){0u, 0u, 0u, 0u};
    f32x4_t gk[MHA_DKT], gv[MHA_DVT];
#pragma unroll
    for (int d = 0; d < MHA_DKT; ++d) gk[d] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d < MHA_DVT; ++d) gv[d] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    MhaStream<flu32x4_t, MHA_DSK * 64> stQ(a.Qf, bh * a.ntq, dsk * 64, sQ);
    MhaStream<flu32x4_t, MHA_DSV * 64> stdO(a.dOf, bh * a.ntq, dsv * 64, sdO);
    MhaStream<uint2, MHA_DKT * 64> stQ16(a.Q16, bh * a.ntq, dkt * 64, sQ16);
    MhaStream<uint2, MHA_DVT * 64> stdO16(a.dO16, bh * a.ntq, dvt * 64, sdO16);
    MhaStream<float, 48> stLD(nullptr, 0, 48, sLD);            // not a copy: its 48 values are made here, the commit is the stage's
    auto fetch = [&](int qt) {
        mha_fetch(qt, tid, stQ, stdO, stQ16, stdO16);
        if (tid < 48) {
            // third block: 0, or NaN for a query without any key (LSE = -inf: every key of the batch padded) - softmax over an empty
            // set is NaN, as in torch and the materialising path, and dV of that batch is NaN like O, dQ and dK (which D carries there)
            const int qq = min(qt * 16 + (tid & 15), a.Lq - 1);
            const float x = (tid >= 16 && tid < 32) ? a.Dd[bh * a.Lq + qq] : a.LSE[bh * a.Lq + qq];
            stLD.r[0] = (tid < 32) ? x : (x == -INFINITY ? __builtin_nanf("") : 0.f);
        }
    };
    fetch(0); mha_commit(0, tid, stQ, stdO, stQ16, stdO16, stLD);
    __syncthreads();
    for (int qt = 0; qt < a.ntq; ++qt) {
        const int buf = qt & 1;
        if (qt + 1 < a.ntq) fetch(qt + 1);
        const f32x4_t s = mha_dot<true>(sQ[buf], kf, dsk, lane), dp = mha_dot<false>(sdO[buf], vf, dsv, lane);      // C[q, key]
        unsigned long long kbits[4];
        mha_keep_words(a, (bh * a.ntq + qt) * a.ntk + ktc, kbits);
        const int qb = qt * 16 + 4 * (lane >> 4);
        float pd[4], ds[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool ok = kv && qb + r < a.Lq;
            const float lse = sLD[buf][4 * (lane >> 4) + r], Dq = sLD[buf][16 + 4 * (lane >> 4) + r];
            const float p = ok ? __builtin_amdgcn_exp2f(s[r] - lse) : sLD[buf][32 + 4 * (lane >> 4) + r];
            const float keep = (a.p_drop > 0.f) ? mha_keep_plain(kbits, lane, r, inv_keep) : 1.f;
            pd[r] = p * keep;
            ds[r] = mha_ds(p, dp[r], keep, Dq);
        }
        const fls16x4_t pb = fl_pack4<false>(pd[0], pd[1], pd[2], pd[3]), db = fl_pack4<false>(ds[0], ds[1], ds[2], ds[3]);
#pragma unroll
        for (int d = 0; d < MHA_DVT; ++d)
            if (d < dvt) gv[d] = mha_mfma16<false>(sdO16[buf][d * 64 + lane], pb, gv[d]);
#pragma unroll
        for (int d = 0; d < MHA_DKT; ++d)
            if (d < dkt) gk[d] = mha_mfma16<false>(sQ16[buf][d * 64 + lane], db, gk[d]);
        if (qt + 1 < a.ntq) mha_commit(buf ^ 1, tid, stQ, stdO, stQ16, stdO16, stLD);
        __syncthreads();
    }
    if (!active || key >= a.Lk) return;
    float* dk_ = a.dk + (((long)b * a.Lk + key) * a.H + h) * dkd;
    float* dv_ = a.dv + (((long)b * a.Lk + key) * a.H + h) * dvd;
    // the Q fragments carry scale * log2(e): dK = dS^T (scale q) = dS^T Qpacked * ln 2
    mha_store_tiles(dk_, gk, dkt, dkd, MHA_LN2, lane);
    mha_store_tiles(dv_, gv, dvt, dvd, 1.f, lane);
}

// ---- C ABI ----------------------------------------------------------------------------------------------
static int mha_fill(MhaArgs& a, int B, int H, int Lq, int Lk, int dk, int dv, int nch) {
    if (dk < 1 || dk > 32 * MHA_DSK || dv < 1 || dv > 16 * MHA_DVT) return -2;
    a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk; a.dk_dim = dk; a.dv_dim = dv;
    a.ntq = (Lq + 15) / 16; a.ntk = (Lk + 15) / 16;
    if (nch < 1) nch = 1; if (nch > a.ntk) nch = a.ntk;
    a.ch_len = (a.ntk + nch - 1) / nch;
    a.nch = (a.ntk + a.ch_len - 1) / a.ch_len;
    return 0;
}

// The (TDK, TDV) instances, listed once: f(integral_constant<int, TDK>, integral_constant<int, TDV>) for the head dims of the call
template <typename F>
static void mha_dispatch(int dk, int dv, F&& f) {
    using D0 = std::integral_constant<int, 0>;
    using D48 = std::integral_constant<int, 48>;
    using D96 = std::integral_constant<int, 96>;
    if (dk == 96 && dv == 48) f(D96{}, D48{});                 // decoder cross-attention
    else if (dk == 48 && dv == 48) f(D48{}, D48{});            // encoder, decoder self-attention
    else f(D0{}, D0{});                                        // run-time head dims
}
#define MHA_LAUNCH(kernel, wgs)                                                                                                       \
    mha_dispatch(dk, dv, [&](auto tdk, auto tdv) {                                                                                    \
        hipLaunchKernelGGL((kernel<decltype(tdk)::value, decltype(tdv)::value>), dim3((unsigned)(wgs)), dim3(256), 0, st, a);         \
    });                                                                                                                               \
    SPE_CHECK_LAUNCH()

// see include/spe_hip.h
extern "C" int spe_mha_plan(int B, int H, int Lq, int Lk, int* nch) {
    const int ntq = (Lq + 15) / 16, ntk = (Lk + 15) / 16;
    long items = (long)B * H * ((ntq + 3) / 4);                // workgroups of 4 query tiles
    int c = (int)((MHA_TARGET + items - 1) / items);           // ~4 workgroups per CU
    if (c > ntk / 4) c = ntk / 4;                              // at least 4 key tiles per chunk
    if (c < 1) c = 1;
    const int len = (ntk + c - 1) / c;
    *nch = (ntk + len - 1) / len;
    return 0;
}
extern "C" int spe_mha_fwd(const void* Qf, const void* Kf, const void* V16, const void* mask, float* Opart, float* ML, float* O,
                           float* LSE, void* keepbits, int B, int H, int Lq, int Lk, int dk, int dv, int nch, float p_drop,
                           uint64_t seed, uint64_t offset, hipStream_t st) {
    if (B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0) return 0;
    MhaArgs a = {};
    const int rc = mha_fill(a, B, H, Lq, Lk, dk, dv, nch);
    if (rc) return rc;
    if (a.nch != nch) return -5;                               // the caller sized the workspaces with spe_mha_plan
    a.Qf = (const flu32x4_t*)Qf; a.Kf = (const flu32x4_t*)Kf; a.V16 = (const uint2*)V16; a.mask = (const unsigned char*)mask;
    a.Opart = Opart; a.ML = ML; a.p_drop = p_drop; a.seed = seed; a.offset = offset;
    a.keepbits = (unsigned long long*)keepbits;
    if (p_drop > 0.f && !keepbits) return -2;
    MHA_LAUNCH(mha_fwd_kernel, (long)B * H * ((a.ntq + 3) / 4) * a.nch);
    const long total = (long)B * H * a.ntq * ((dv + 15) / 16) * 64;
    hipLaunchKernelGGL(mha_merge_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, Opart, ML, O, LSE, B, H, Lq, a.ntq,
                       a.nch, dv);
    SPE_CHECK_LAUNCH();
    return 0;
}
extern "C" int spe_mha_bwd(const void* Qf, const void* Kf, const void* Vf, const void* dOf, const void* K16, const void* Q16,
                           const void* dO16, const void* mask, const float* LSE, const float* D, const void* keepbits, float* dq,
                           float* dq_ws, float* dk_, float* dv_, int B, int H, int Lq, int Lk, int dk, int dv, int nch, float scale, float p_drop,
                           hipStream_t st) {
    if (B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0) return 0;
    MhaArgs a = {};
    const int rc = mha_fill(a, B, H, Lq, Lk, dk, dv, nch);
    if (rc) return rc;
    a.Qf = (const flu32x4_t*)Qf; a.Kf = (const flu32x4_t*)Kf; a.Vf = (const flu32x4_t*)Vf; a.dOf = (const flu32x4_t*)dOf;
    a.K16 = (const uint2*)K16; a.Q16 = (const uint2*)Q16; a.dO16 = (const uint2*)dO16; a.mask = (const unsigned char*)mask;
    a.LSE = LSE; a.Dd = D; a.dq = dq; a.dq_ws = dq_ws; a.dk = dk_; a.dv = dv_;
    a.scale = scale; a.p_drop = p_drop;
    a.keepbits = (unsigned long long*)const_cast<void*>(keepbits);
    if (p_drop > 0.f && !keepbits) return -2;
    if (a.nch > 1 && !dq_ws) return -2;                        // chunks never add into one dq: each needs its slab
    MHA_LAUNCH(mha_bwd_dq_kernel, (long)B * H * ((a.ntq + 3) / 4) * a.nch);
    MHA_LAUNCH(mha_bwd_dkv_kernel, (long)B * H * ((a.ntk + 3) / 4));
    return 0;
}
