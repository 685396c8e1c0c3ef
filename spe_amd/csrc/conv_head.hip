// 3x3 convolutional class head of the woct0head TSCAM backbones (reference models/cait.py:971-974, 1142-1145, 1309-1312:
// conv_head = Conv2d(C, K, 3, padding=1) over the normalised patch tokens, then AdaptiveAvgPool2d(1)) and its autograd.
//
// The token tensor is read as it is: x [B, h*w, C] fp32, channels-last - no permute, no contiguous copy, no im2col.  Every product is an
// implicit GEMM on the exact-fp32 matrix instruction v_mfma_f32_16x16x4_f32 (lane l: A[l & 15][k = l >> 4], B[k = l >> 4][l & 15];
// D[row = 4 (l >> 4) + r][col = l & 15]); the zero padding of the convolution is a masked load.  fp32 throughout, in every precision mode.
//
//   forward : map[b][k][p] = bias[k] + sum_{c, tap} W[k][c][tap] x[b][p + off(tap)][c],  logits[b][k] = mean_p map[b][k][p]
//             (M = classes, N = positions, contraction = 9 C).  The spatial sums cross workgroups: det_reduce.h (fixed order, no atomics).
//   backward: g = dmap + dlogits / (h w) (either may be absent: the pooled gradient is one case of a general dmap)
//             dx[b][q][c] = sum_{k, tap} W[k][c][tap] g[b][k][q - off(tap)]       (M = positions, N = channels, contraction = 9 K)
//             dW[k][c][tap] = sum_{b, p} g[b][k][p] x[b][p + off(tap)][c],  db[k] = sum_{b, p} g[b][k][p]
//             (M = classes, N = channels, contraction = positions): split over position ranges into private partial rows of a caller-owned
//             workspace, summed in split order by a second kernel - the split-K slab scheme of spe_gemm_f32, bitwise reproducible.
#include "common.h"
#include "det_reduce.h"

#define CH_KG 8                      // class tiles (16 classes each) per pass of the forward kernel

__device__ __forceinline__ f32x4_t ch_mfma(float a, float b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// gradient at (b, k, p): dmap and / or the pooled gradient spread over the positions
__device__ __forceinline__ float ch_grad(const float* __restrict__ dmap, const float* __restrict__ dlog, int b, int k, int p, int K, int hw,
                                         float inv_hw) {
    float v = 0.f;
    if (dmap) v = dmap[((long)b * K + k) * hw + p];
    if (dlog) v += dlog[(long)b * K + k] * inv_hw;
    return v;
}

// Forward: one wave per 16-position tile (4 per workgroup), all classes in passes of CH_KG tiles.
__global__ __launch_bounds__(256) void conv_head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                                                            float* __restrict__ map, float* __restrict__ logits, int h, int w, int C, int K,
                                                            DetWs ws) {
    extern __shared__ float ch_red[];                 // [4 waves][K]: per-wave sums over the wave's positions
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
    const int hw = h * w, j = lane & 15, g = lane >> 4;
    const int pt = blockIdx.x * 4 + wave;
    const int p = pt * 16 + j;                        // this lane's position in the B operand
    const int py = p / w, px = p % w;
    const float* xb = x + (long)b * hw * C;
    const int nkt = (K + 15) / 16;
    for (int kg = 0; kg < nkt; kg += CH_KG) {
        f32x4_t acc[CH_KG];
#pragma unroll
        for (int t = 0; t < CH_KG; ++t) acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        for (int tap = 0; tap < 9; ++tap) {
            const int sy = py + tap / 3 - 1, sx = px + tap % 3 - 1;
            const bool pv = p < hw && sy >= 0 && sy < h && sx >= 0 && sx < w;
            const float* xs = xb + ((long)sy * w + sx) * C;
            for (int c0 = 0; c0 < C; c0 += 16) {
                const int c = c0 + 4 * g;                 // lane group g: channels c .. c + 3 (C % 4 == 0: all four or none)
                f32x4_t xv = (f32x4_t){0.f, 0.f, 0.f, 0.f};
                if (pv && c < C) xv = *reinterpret_cast<const f32x4_t*>(xs + c);
#pragma unroll
                for (int t = 0; t < CH_KG; ++t) {
                    if (kg + t >= nkt) break;             // wave-uniform
                    const int k = (kg + t) * 16 + j;
                    const bool wv = k < K && c < C;
                    const float* wp = W + ((long)k * C + c) * 9 + tap;
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc[t] = ch_mfma(wv ? wp[s * 9] : 0.f, xv[s], acc[t]);
                }
            }
        }
        // D: class (kg + t) * 16 + 4 g + r, position pt * 16 + j
#pragma unroll
        for (int t = 0; t < CH_KG; ++t) {
            if (kg + t >= nkt) break;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = (kg + t) * 16 + 4 * g + r;
                float v = acc[t][r];
                if (k < K && p < hw) map[((long)b * K + k) * hw + p] = v + bias[k];
                // the wave's sum over its 16 positions (masked positions hold exact zeros)
                v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
                if (j == 0 && k < K) ch_red[wave * K + k] = v;
            }
        }
    }
    __syncthreads();
    const float inv_hw = 1.0f / (float)hw;
    det_reduce(ws, b, blockIdx.x, gridDim.x, K, threadIdx.x, 256,
               [&](int k) { return ((ch_red[k] + ch_red[K + k]) + ch_red[2 * K + k]) + ch_red[3 * K + k]; },
               [&](int k, float s) { logits[(long)b * K + k] = bias[k] + s * inv_hw; });
}

// dx: one wave per (16-position tile, 4 channel tiles); 4 waves per workgroup along the positions.
__global__ __launch_bounds__(256) void conv_head_dx_kernel(const float* __restrict__ W, const float* __restrict__ dmap, const float* __restrict__ dlog,
                                                           float* __restrict__ dx, int h, int w, int C, int K) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.z;
    const int hw = h * w, j = lane & 15, g = lane >> 4;
    const int qt = blockIdx.x * 4 + wave, ct0 = blockIdx.y * 4;
    if (qt * 16 >= hw) return;                        // whole wave: no barrier in this kernel
    const float inv_hw = 1.0f / (float)hw;
    const int q = qt * 16 + j;                        // A operand row: the dx position
    const int qy = q / w, qx = q % w;
    f32x4_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    for (int tap = 0; tap < 9; ++tap) {
        const int sy = qy - (tap / 3 - 1), sx = qx - (tap % 3 - 1);          // the output position that read q through this tap
        const bool pv = q < hw && sy >= 0 && sy < h && sx >= 0 && sx < w;
        const int sp = sy * w + sx;
        for (int k0 = 0; k0 < K; k0 += 4) {
            const int ka = k0 + g;                    // A column / B row: class
            const float av = (pv && ka < K) ? ch_grad(dmap, dlog, b, ka, sp, K, hw, inv_hw) : 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int c = (ct0 + t) * 16 + j;
                const float bv = (ka < K && c < C) ? W[((long)ka * C + c) * 9 + tap] : 0.f;
                acc[t] = ch_mfma(av, bv, acc[t]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int c = (ct0 + t) * 16 + j;
        if (c >= C) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qq = qt * 16 + 4 * g + r;
            if (qq < hw) dx[((long)b * hw + qq) * C + c] = acc[t][r];
        }
    }
}

// dW / db partials: workgroup = (class tile, 4 channel tiles - one per wave), split s over the flattened (b, p) positions.  Row s of ws holds
// split s's partial dW [K][C][9] followed by its partial db [K].
__global__ __launch_bounds__(256) void conv_head_dw_kernel(const float* __restrict__ x, const float* __restrict__ dmap, const float* __restrict__ dlog,
                                                           float* __restrict__ ws, int B, int h, int w, int C, int K, int pos_per_split) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hw = h * w, j = lane & 15, g = lane >> 4;
    const int ncg = (C + 63) / 64;
    const int kt = blockIdx.x / ncg, ct = (blockIdx.x % ncg) * 4 + wave, split = blockIdx.y;
    const long L = (long)K * C * 9 + K;
    float* row = ws + (long)split * L;
    const float inv_hw = 1.0f / (float)hw;
    const long P0 = (long)split * pos_per_split;
    long P1 = P0 + pos_per_split; if (P1 > (long)B * hw) P1 = (long)B * hw;
    const int k = kt * 16 + j;                        // A operand row: class
    const int c = ct * 16 + j;                        // B operand column: channel
    const bool cv = c < C;
    f32x4_t acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    float dbs = 0.f;
    if (ct * 16 < C) {                                // wave-uniform
        for (long P = P0; P < P1; P += 4) {
            const long Pl = P + g;                    // A column / B row: position
            const bool pv = Pl < P1;
            const int b = pv ? (int)(Pl / hw) : 0, p = pv ? (int)(Pl % hw) : 0;
            const float av = (pv && k < K) ? ch_grad(dmap, dlog, b, k, p, K, hw, inv_hw) : 0.f;
            dbs += av;
            const int py = p / w, px = p % w;
            const float* xb = x + (long)b * hw * C + c;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int sy = py + tap / 3 - 1, sx = px + tap % 3 - 1;
                const bool v = pv && cv && sy >= 0 && sy < h && sx >= 0 && sx < w;
                const float bv = v ? xb[((long)sy * w + sx) * C] : 0.f;
                acc[tap] = ch_mfma(av, bv, acc[tap]);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kk = kt * 16 + 4 * g + r;
            if (kk < K && cv) {
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) row[((long)kk * C + c) * 9 + tap] = acc[tap][r];
            }
        }
    }
    // db: the class's sum over the 4 position lanes of its column (lanes j, j + 16, j + 32, j + 48), written by one wave of the class tile
    dbs += __shfl_xor(dbs, 16, 64);
    dbs += __shfl_xor(dbs, 32, 64);
    if (blockIdx.x % ncg == 0 && wave == 0 && g == 0 && k < K) row[(long)K * C * 9 + k] = dbs;
}

// out[e] = sum_s ws[s][e] in split order (dW then db; NULL destinations skipped).  Overwrites.
__global__ __launch_bounds__(256) void conv_head_wsum_kernel(const float* __restrict__ ws, int nsplit, long KC9, int K, float* __restrict__ dW,
                                                             float* __restrict__ db) {
    const long L = KC9 + K;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= L) return;
    float s = 0.f;
    for (int i = 0; i < nsplit; ++i) s += ws[(long)i * L + e];
    if (e < KC9) { if (dW) dW[e] = s; }
    else if (db) db[e - KC9] = s;
}

static bool ch_shape_ok(int B, int h, int w, int C, int K) {
    return B >= 1 && h >= 1 && w >= 1 && K >= 1 && C >= 4 && (C & 3) == 0 && (long)h * w < (1L << 30) && (long)K * C * 9 < (1L << 30);
}

// position splits of the weight-gradient pass: enough workgroups for the chip, >= 64 positions per split, <= 64 splits
static int ch_nsplit(int B, int h, int w, int C, int K) {
    const long npos = (long)B * h * w;
    const long tiles = (long)((K + 15) / 16) * ((C + 63) / 64);
    long s = (1024 + tiles - 1) / tiles;
    const long smax = (npos + 63) / 64;
    if (s > smax) s = smax;
    if (s > 64) s = 64;
    return s < 1 ? 1 : (int)s;
}

// C-ABI: see include/spe_hip.h.
extern "C" int spe_conv_head_fwd(const float* x, const float* W, const float* bias, float* map, float* logits, int B, int h, int w, int C, int K,
                                 hipStream_t st) {
    if (!ch_shape_ok(B, h, w, C, K)) return -2;
    const int hw = h * w, nwg = ((hw + 15) / 16 + 3) / 4;
    DetWs ws = spe_detws();
    ws.defer = nullptr;
    DET_CHECK(ws, B, nwg, K);
    hipLaunchKernelGGL(conv_head_fwd_kernel, dim3((unsigned)nwg, (unsigned)B), dim3(256), 4 * K * (int)sizeof(float), st, x, W, bias, map, logits,
                       h, w, C, K, ws);
    SPE_CHECK_LAUNCH();
    return 0;
}

extern "C" int spe_conv_head_plan(int B, int h, int w, int C, int K, long* ws_floats) {
    if (!ch_shape_ok(B, h, w, C, K)) return -2;
    *ws_floats = (long)ch_nsplit(B, h, w, C, K) * ((long)K * C * 9 + K);
    return 0;
}

extern "C" int spe_conv_head_bwd(const float* x, const float* W, const float* dmap, const float* dlogits, float* dx, float* dW, float* db,
                                 float* ws, long ws_floats, int B, int h, int w, int C, int K, hipStream_t st) {
    if (!ch_shape_ok(B, h, w, C, K)) return -2;
    const int hw = h * w;
    if (dx) {
        hipLaunchKernelGGL(conv_head_dx_kernel, dim3((unsigned)(((hw + 15) / 16 + 3) / 4), (unsigned)((C + 63) / 64), (unsigned)B), dim3(256), 0, st,
                           W, dmap, dlogits, dx, h, w, C, K);
        SPE_CHECK_LAUNCH();
    }
    if (dW || db) {
        const int ns = ch_nsplit(B, h, w, C, K);
        const long L = (long)K * C * 9 + K;
        if (!ws || ws_floats < ns * L) return -4;
        const long npos = (long)B * hw;
        const int pps = (int)(((npos + ns - 1) / ns + 3) / 4 * 4);
        const int ntiles = ((K + 15) / 16) * ((C + 63) / 64);
        hipLaunchKernelGGL(conv_head_dw_kernel, dim3((unsigned)ntiles, (unsigned)ns), dim3(256), 0, st, x, dmap, dlogits, ws, B, h, w, C, K, pps);
        SPE_CHECK_LAUNCH();
        hipLaunchKernelGGL(conv_head_wsum_kernel, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, st, ws, ns, L - K, K, dW, db);
        SPE_CHECK_LAUNCH();
    }
    return 0;
}
