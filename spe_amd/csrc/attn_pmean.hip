// Head-mean of the talking-heads attention probabilities, accumulated block by block (reference models/cait.py:384, 392 keep a clone of
// softmax(proj_l(q k^T)) [B, H, N, N] per block; the woct0head backbone stacks all of them and takes mean(dim=2).mean(dim=0) for
// cams_cls_patch, cait.py:993-994).  No [B, H, N, N] tensor exists here: one fp32 [B, N, N] accumulator receives every block's head sum,
//
//   M[b][q][k] += alpha * sum_g P_g[b][q][k],   P_g = exp2(sum_h Wl[g][h] S_h + c0[b][q][g])     (alpha = 1 / (depth * H))
//
// with S_h the raw scores recomputed from the fused forward's fp16 fragment records (spe_attn_pack_multi kind 0 + 16; Qf carries
// scale * log2(e)) and c0 the row constants of spe_attn_merge_rows - the first half ("H1") of the flash forward's step (attn_flash.hip)
// without the proj_w mix and the P' V product.  P is taken before proj_w and before dropout: the reference's `weights`.
//
// Work: one wave per (b, q-tile, chunk of PM_KT key tiles); each 16 x 16 tile of M is owned by exactly one wave of a launch, which reads, adds
// and writes it back (plain vector loads and stores, no atomics); the blocks' launches are ordered on the stream - deterministic.
// spe_attn_pmean_dense is the same accumulation from a materialised P [B, H, N, ld] (the fp32 path: bf16x3, unsupported head geometries).
#include "attn_flash_common.h"

#define PM_KT 8                      // key tiles per wave

template <int H, int DSTEPS, bool TAIL16>
__global__ __launch_bounds__(256) void attn_pmean_kernel(const flu32x4_t* __restrict__ Qf, const flu32x4_t* __restrict__ Kf,
                                                         const float* __restrict__ Wl, const float* __restrict__ c0, int Np, float* __restrict__ M,
                                                         float alpha, int B, int N, int nt, int nkc) {
    const int lane = threadIdx.x & 63;
    const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= (long)B * nt * nkc) return;                        // whole wave; no barrier in this kernel
    const int kc = (int)(wid % nkc), qt = (int)((wid / nkc) % nt), b = (int)(wid / ((long)nkc * nt));
    // S^T = K Q^T (M = keys, N = queries): lane = (query qt * 16 + (lane & 15), keys 4 (lane >> 4) + r of the key tile)
    const int q = qt * 16 + (lane & 15);
    flu32x4_t qreg[H * DSTEPS];
#pragma unroll
    for (int h = 0; h < H; ++h)
#pragma unroll
        for (int st = 0; st < DSTEPS; ++st) qreg[h * DSTEPS + st] = fl_frag_global<DSTEPS, TAIL16>(Qf, ((long)b * H + h) * nt + qt, st, lane);
    // the fp32 Wl mix on v_mfma_f32_4x4x1_16b_f32 (attn_stats.hip, mix_keys_f32): register i of a lane accumulates output head 4 gh + i of the
    // lane's own (query, key) element; it starts from that head's row constant
    float A[H / 4][H];
    fl_mixA_f32<H, false>(Wl, lane, A);
    f32x4_t cq[H / 4];                                            // rows N .. Np - 1 of c0 are zero: q < nt * 16 <= Np
#pragma unroll
    for (int gh = 0; gh < H / 4; ++gh) cq[gh] = *reinterpret_cast<const f32x4_t*>(c0 + ((long)b * Np + q) * H + 4 * gh);
    float* Mrow = M + ((long)b * N + (q < N ? q : 0)) * N;
    const int kt_end = min(nt, (kc + 1) * PM_KT);
    for (int kt = kc * PM_KT; kt < kt_end; ++kt) {
        f32x4_t s[H];
#pragma unroll
        for (int h = 0; h < H; ++h) {
            f32x4_t c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int st = 0; st < DSTEPS; ++st) c = fl_mfma32<true>(fl_frag_global<DSTEPS, TAIL16>(Kf, ((long)b * H + h) * nt + kt, st, lane), qreg[h * DSTEPS + st], c);
            s[h] = c;
        }
        f32x4_t sp[4][H / 4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int gh = 0; gh < H / 4; ++gh) sp[r][gh] = cq[gh];
#pragma unroll
        for (int h = 0; h < H; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int gh = 0; gh < H / 4; ++gh) sp[r][gh] = __builtin_amdgcn_mfma_f32_4x4x1f32(A[gh][h], s[h][r], sp[r][gh], 0, 0, 0);
        f32x4_t pv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float t = 0.f;
#pragma unroll
            for (int g = 0; g < H; ++g) t += __builtin_amdgcn_exp2f(sp[r][g >> 2][g & 3]);
            pv[r] = alpha * t;
        }
        const int k0 = kt * 16 + 4 * (lane >> 4);
        if (q < N) {
            if ((N & 3) == 0) {                                   // rows 16-B aligned: the lane's 4 keys are all valid or all padding
                if (k0 < N) {
                    f32x4_t m = *reinterpret_cast<const f32x4_t*>(Mrow + k0);
                    *reinterpret_cast<f32x4_t*>(Mrow + k0) = m + pv;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (k0 + r < N) Mrow[k0 + r] += pv[r];
            }
        }
    }
}

__global__ __launch_bounds__(256) void attn_pmean_dense_kernel(const float* __restrict__ P, float* __restrict__ M, float alpha, int H, int N,
                                                               long ld, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;           // over B * N * N
    if (i >= total) return;
    const int k = (int)(i % N);
    const long bq = i / N;
    const int q = (int)(bq % N), b = (int)(bq / N);
    float s = 0.f;
    for (int h = 0; h < H; ++h) s += P[(((long)b * H + h) * N + q) * ld + k];
    M[i] += alpha * s;
}

// C-ABI: see include/spe_hip.h.  -2 for unsupported (H, head dim).
extern "C" int spe_attn_pmean(const void* Qf, const void* Kf, const float* Wl, const float* c0, int Np, float* M, float alpha, int B, int H, int N,
                              int dh, hipStream_t st) {
    const int nt = (N + 15) / 16;
    if ((long)B * nt <= 0) return 0;
    if (dh < 1 || dh > 64 || Np < nt * 16) return -2;
    const int nkc = (nt + PM_KT - 1) / PM_KT;
    const long waves = (long)B * nt * nkc;
    const dim3 grid((unsigned)((waves + 3) / 4));
    const flu32x4_t* q4 = reinterpret_cast<const flu32x4_t*>(Qf);
    const flu32x4_t* k4 = reinterpret_cast<const flu32x4_t*>(Kf);
    return attn_dispatch(H, dh, [&](auto h, auto ds, auto tl) {
        hipLaunchKernelGGL((attn_pmean_kernel<decltype(h)::value, decltype(ds)::value, decltype(tl)::value>), grid, dim3(256), 0, st, q4, k4, Wl, c0, Np, M,
                           alpha, B, N, nt, nkc);
        SPE_CHECK_LAUNCH();
        return 0;
    });
}

extern "C" int spe_attn_pmean_dense(const float* P, float* M, float alpha, int B, int H, int N, long ld, hipStream_t st) {
    const long total = (long)B * N * N;
    if (total <= 0) return 0;
    if (H < 1 || ld < N) return -2;
    hipLaunchKernelGGL(attn_pmean_dense_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, P, M, alpha, H, N, ld, total);
    SPE_CHECK_LAUNCH();
    return 0;
}
