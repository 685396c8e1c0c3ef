// Optimiser step of the SPE training loop on flat buffers: reference
// engine.py:161-165 (`clip_grad_norm_(model.parameters(), 0.1)` then `optimizer.step()`) with the AdamW parameter
// groups of main.py:177-191.  Gradients already live in the flat all-reduce buckets (spe_amd/dp.py); parameters and
// the two moment buffers use the same layout, so the whole step is two launches per bucket - a squared-norm pass and
// one fused clip + decoupled-weight-decay + Adam update - instead of ~20 multi-tensor launches over ~600 tensors.
#include "common.h"

// partials[b] = sum of g[i]^2 over the b-th contiguous chunk (fixed order: deterministic)
__global__ __launch_bounds__(256) void sqnorm_partials_kernel(const float* __restrict__ g, long n, float* __restrict__ partials) {
    __shared__ float red[16];
    const long per = ((n + gridDim.x - 1) / gridDim.x + 3) & ~3L;
    long beg = (long)blockIdx.x * per; if (beg > n) beg = n;       // chunks past the end are empty (end - beg must not go negative)
    long end = beg + per; if (end > n) end = n;
    float acc = 0.f;
    const bool al = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
    if (al) {
        for (long i = beg + threadIdx.x * 4; i + 3 < end; i += 1024) {
            const float4 v = *reinterpret_cast<const float4*>(g + i);
            acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
        const long tail = beg + ((end - beg) & ~3L);
        for (long i = tail + threadIdx.x; i < end; i += 256) acc += g[i] * g[i];
    } else {
        for (long i = beg + threadIdx.x; i < end; i += 256) acc += g[i] * g[i];
    }
    acc = spe_block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

extern "C" int spe_sqnorm_partials(const float* g, long n, float* partials, int nblocks, hipStream_t st) {
    if (nblocks <= 0) return 0;
    hipLaunchKernelGGL(sqnorm_partials_kernel, dim3(nblocks), dim3(256), 0, st, g, n, partials);
    SPE_CHECK_LAUNCH();
    return 0;
}

// Gradient accumulation beside the buckets (spe_amd/dp.py, accum_steps > 1): dst = a + b, or the bit copy dst = a when b is
// NULL (not a + 0: -0.0 survives).  dst may alias a or b - every lane reads its own elements before it writes them, hence no
// __restrict__.  No atomics, no cross-lane sums: bitwise deterministic.
template <bool ADD>
__global__ __launch_bounds__(256) void accum_flat_kernel(float* dst, const float* a, const float* b, long n) {
    const long n4 = n & ~3L;
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < n4; i += (long)gridDim.x * 1024) {
        float4 v = *reinterpret_cast<const float4*>(a + i);
        if (ADD) {
            const float4 w = *reinterpret_cast<const float4*>(b + i);
            v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
        }
        *reinterpret_cast<float4*>(dst + i) = v;
    }
    if (blockIdx.x == 0 && threadIdx.x < n - n4) {           // scalar tail: n % 4 elements
        const long i = n4 + threadIdx.x;
        const float x = a[i];
        dst[i] = ADD ? x + b[i] : x;
    }
}

// C-ABI: see include/spe_hip.h (spe_accum_flat).
extern "C" int spe_accum_flat(float* dst, const float* a, const float* b, long n, hipStream_t st) {
    if (n <= 0) return 0;
    if ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) return -2;
    long nb = (n + 1023) / 1024; if (nb > 2048) nb = 2048;           // the grid cap of spe_adamw_flat
    if (b != nullptr) hipLaunchKernelGGL(accum_flat_kernel<true>, dim3((unsigned)nb), dim3(256), 0, st, dst, a, b, n);
    else hipLaunchKernelGGL(accum_flat_kernel<false>, dim3((unsigned)nb), dim3(256), 0, st, dst, a, b, n);
    SPE_CHECK_LAUNCH();
    return 0;
}

// Exchange of two flat buffers (FlatAdamW.ema_weights(): parameters <-> their moving average).  Loads and stores only - no
// arithmetic touches the values, so NaN payloads and -0.0 survive.  Every lane reads both of its elements before it writes either.
__global__ __launch_bounds__(256) void swap_flat_kernel(float* __restrict__ a, float* __restrict__ b, long n) {
    const long n4 = n & ~3L;
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < n4; i += (long)gridDim.x * 1024) {
        const float4 x = *reinterpret_cast<const float4*>(a + i), y = *reinterpret_cast<const float4*>(b + i);
        *reinterpret_cast<float4*>(a + i) = y;
        *reinterpret_cast<float4*>(b + i) = x;
    }
    if (blockIdx.x == 0 && threadIdx.x < n - n4) {           // scalar tail: n % 4 elements
        const long i = n4 + threadIdx.x;
        const float x = a[i], y = b[i];
        a[i] = y; b[i] = x;
    }
}

// C-ABI: see include/spe_hip.h (spe_swap_flat).
extern "C" int spe_swap_flat(float* a, float* b, long n, hipStream_t st) {
    if (n <= 0) return 0;
    if (a == nullptr || b == nullptr || a == b || ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15)) return -2;
    long nb = (n + 1023) / 1024; if (nb > 2048) nb = 2048;           // the grid cap of spe_adamw_flat
    hipLaunchKernelGGL(swap_flat_kernel, dim3((unsigned)nb), dim3(256), 0, st, a, b, n);
    SPE_CHECK_LAUNCH();
    return 0;
}

#define ADAMW_MAXSEG 64
struct AdamwArgs {
    float* p; float* g; float* m; float* v; long n;
    const long* seg_end; const float* seg_lr; const float* seg_wd; int nseg;
    float beta1, beta2, eps, bc1, bc2sqrt;
    const float* partials; int npartials; float max_norm; int write_grad; float gscale;
    const int* guard;                  // GUARDED only: the guard block, in place of bc1, bc2sqrt, partials, max_norm and gscale
    float* e; double ema_decay; int ema_warmup; float ema_t;       // EMA only: the average, its decay, warm-up on / off, applied steps (unguarded)
};

// Sum of the squared-norm partials of ALL buckets: lane-strided, then spe_block_sum.  The one reduction behind the clip factor of the
// unguarded update (every workgroup's prologue) and behind the gate's decision, so both paths clip by the same bits.
__device__ __forceinline__ float adamw_sqnorm_total(const float* partials, int npartials, float* red) {
    float acc = 0.f;
    for (int i = threadIdx.x; i < npartials; i += 256) acc += partials[i];
    return spe_block_sum(acc, red);
}
// norm of the scaled gradient and clip * gscale from that sum (max_norm <= 0: no clipping)
__device__ __forceinline__ float adamw_clip_scale(float sqsum, float max_norm, float gscale, float* norm) {
    const float tot = gscale * sqrtf(sqsum);
    *norm = tot;
    const float clip = max_norm > 0.f ? fminf(max_norm / (tot + 1e-6f), 1.f) : 1.f;
    return clip * gscale;
}

// Guard block words (include/spe_hip.h, SPE_ADAMW_GUARD_*)
enum { GW_APPLIED = 0, GW_SKIPPED = 1, GW_FIRST = 2, GW_APPLY = 3, GW_CLIP = 4, GW_BC1 = 5, GW_BC2SQRT = 6, GW_NORM = 7, GW_STEP_F = 8 };

// One workgroup per optimizer step, after the spe_sqnorm_partials launches of every bucket: the decision and the step's constants.
// apply = isfinite(sum of squares) - a NaN or an infinity anywhere in the buckets, or a squared norm past FLT_MAX, skips the step.
// The bias corrections follow the APPLIED count t (a skipped step must not shift the later ones): beta^t in fp64, rounded once.
__global__ __launch_bounds__(256) void adamw_gate_kernel(int* guard, const float* __restrict__ partials, int npartials, float max_norm,
                                                         float gscale, double beta1, double beta2) {
    __shared__ float red[16];
    const float sqsum = adamw_sqnorm_total(partials, npartials, red);
    if (threadIdx.x != 0) return;
    float norm;
    const float cs = adamw_clip_scale(sqsum, max_norm, gscale, &norm);
    const int apply = isfinite(sqsum) ? 1 : 0;
    const int applied = guard[GW_APPLIED] + apply, skipped = guard[GW_SKIPPED] + 1 - apply;
    const double t = (double)applied;
    float* gf = reinterpret_cast<float*>(guard);
    guard[GW_APPLIED] = applied;
    guard[GW_SKIPPED] = skipped;
    if (!apply && guard[GW_FIRST] == 0) guard[GW_FIRST] = applied + skipped;       // 1-based index of this attempt
    guard[GW_APPLY] = apply;
    gf[GW_CLIP] = apply ? cs : 0.f;
    gf[GW_BC1] = (float)(1.0 - pow(beta1, t));
    gf[GW_BC2SQRT] = (float)sqrt(1.0 - pow(beta2, t));
    gf[GW_NORM] = norm;
    gf[GW_STEP_F] = (float)applied;
}

// C-ABI: see include/spe_hip.h (spe_adamw_gate).
extern "C" int spe_adamw_gate(void* guard, const float* partials, int npartials, float max_norm, float grad_scale, double beta1,
                              double beta2, hipStream_t st) {
    if (guard == nullptr || (reinterpret_cast<uintptr_t>(guard) & 15) || partials == nullptr || npartials < 1) return -2;
    hipLaunchKernelGGL(adamw_gate_kernel, dim3(1), dim3(256), 0, st, static_cast<int*>(guard), partials, npartials, max_norm, grad_scale,
                       beta1, beta2);
    SPE_CHECK_LAUNCH();
    return 0;
}

// The weight-EMA stream of the update (EMA instantiations): e' = e + w * (p' - e) in three fp32 operations, each rounded - the file is
// built with contraction on, so the switch is scoped to these two helpers and the update's own bits stay what they were.
// w = (float)(1 - d), d = warmup ? min(decay, (1 + t) / (10 + t)) : decay in fp64, t the 1-based count of applied steps.
__device__ __forceinline__ float adamw_ema_weight(double decay, int warmup, double t) {
#pragma clang fp contract(off)
    const double d = warmup ? fmin(decay, (1.0 + t) / (10.0 + t)) : decay;
    return (float)(1.0 - d);
}
__device__ __forceinline__ float adamw_ema(float e, float p, float w) {
#pragma clang fp contract(off)
    const float d = p - e;
    const float s = w * d;
    return e + s;
}

// torch.optim.AdamW (amsgrad = False, maximize = False):
//   p *= 1 - lr*wd ; m = lerp(m, g, 1-beta1) ; v = beta2*v + (1-beta2) g^2 ;
//   p -= (lr / (1-beta1^t)) * m / (sqrt(v)/sqrt(1-beta2^t) + eps)
// with g first scaled by clip = min(1, max_norm / (||g||_2 + 1e-6)) over ALL parameters (torch clip_grad_norm_).
// Element i belongs to the segment s with seg_end[s-1] <= i < seg_end[s] (parameter group: lr, weight decay).
// GUARDED (spe_adamw_flat_guarded): clip * gscale and the bias corrections come from the guard block the gate launch left, and a
// workgroup that reads apply == 0 returns before its first store - p, m, v and g keep their bits.  Everything after the prologue is
// the one body of every instantiation.
// EMA (spe_adamw_flat_ema): one more fp32 stream of the same layout, e' = adamw_ema(e, p', w) with the p' this lane has just computed;
// t comes from the argument (unguarded) or from the guard block's applied count (guarded: a skipped step leaves e and the warm-up alone).
template <bool GUARDED, bool EMA>
__global__ __launch_bounds__(256) void adamw_flat_kernel(AdamwArgs a) {
    __shared__ float red[16];
    __shared__ long s_end[ADAMW_MAXSEG];
    __shared__ float s_lr[ADAMW_MAXSEG], s_wd[ADAMW_MAXSEG];
    float clip, bc1, bc2sqrt, ema_t = a.ema_t;
    if (GUARDED) {                                       // the record in one round trip, ahead of the decision that waits for it
        const float* gf = reinterpret_cast<const float*>(a.guard);
        const int apply = a.guard[GW_APPLY];
        clip = gf[GW_CLIP]; bc1 = gf[GW_BC1]; bc2sqrt = gf[GW_BC2SQRT];
        if (EMA) ema_t = gf[GW_STEP_F];
        if (apply == 0) return;                          // the same word for every lane: the whole workgroup leaves
    }
    const float ema_w = EMA ? adamw_ema_weight(a.ema_decay, a.ema_warmup, (double)ema_t) : 0.f;
    for (int i = threadIdx.x; i < a.nseg; i += 256) { s_end[i] = a.seg_end[i]; s_lr[i] = a.seg_lr[i]; s_wd[i] = a.seg_wd[i]; }
    if (!GUARDED) {
        float norm;
        const float sqsum = a.max_norm > 0.f ? adamw_sqnorm_total(a.partials, a.npartials, red) : 0.f;
        clip = adamw_clip_scale(sqsum, a.max_norm, a.gscale, &norm);
        bc1 = a.bc1; bc2sqrt = a.bc2sqrt;
    }
    __syncthreads();
    // grid-stride over float4 chunks: the prologue above (segment table, clip factor from the norm partials) is paid once
    // per workgroup, not once per 1024 elements (26 K workgroups for the 27 M parameters of cfg2: 0.41 -> 0.2x ms)
    for (long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i0 < a.n; i0 += (long)gridDim.x * 1024) {
    int lo = 0, hi = a.nseg - 1;                         // first segment whose end is > i0
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_end[mid] > i0) hi = mid; else lo = mid + 1; }
    int seg = lo;
    float pv[4], gv[4], mv[4], vv[4], ev[4];
    const bool full = i0 + 3 < a.n;
    if (full) {
        const float4 P = *reinterpret_cast<const float4*>(a.p + i0), G = *reinterpret_cast<const float4*>(a.g + i0);
        const float4 M = *reinterpret_cast<const float4*>(a.m + i0), V = *reinterpret_cast<const float4*>(a.v + i0);
        pv[0] = P.x; pv[1] = P.y; pv[2] = P.z; pv[3] = P.w; gv[0] = G.x; gv[1] = G.y; gv[2] = G.z; gv[3] = G.w;
        mv[0] = M.x; mv[1] = M.y; mv[2] = M.z; mv[3] = M.w; vv[0] = V.x; vv[1] = V.y; vv[2] = V.z; vv[3] = V.w;
        if (EMA) { const float4 E = *reinterpret_cast<const float4*>(a.e + i0); ev[0] = E.x; ev[1] = E.y; ev[2] = E.z; ev[3] = E.w; }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = i0 + j < a.n;
            pv[j] = in ? a.p[i0 + j] : 0.f; gv[j] = in ? a.g[i0 + j] : 0.f; mv[j] = in ? a.m[i0 + j] : 0.f; vv[j] = in ? a.v[i0 + j] : 0.f;
            if (EMA) ev[j] = in ? a.e[i0 + j] : 0.f;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        while (seg < a.nseg - 1 && s_end[seg] <= i0 + j) ++seg;
        const float lr = s_lr[seg], wd = s_wd[seg];
        const float g = gv[j] * clip;
        float p = pv[j] * (1.f - lr * wd);
        const float m = mv[j] + (g - mv[j]) * (1.f - a.beta1);
        const float v = a.beta2 * vv[j] + (1.f - a.beta2) * g * g;
        const float denom = sqrtf(v) / bc2sqrt + a.eps;
        p -= (lr / bc1) * (m / denom);
        pv[j] = p; gv[j] = g; mv[j] = m; vv[j] = v;
        if (EMA) ev[j] = adamw_ema(ev[j], p, ema_w);
    }
    if (full) {
        *reinterpret_cast<float4*>(a.p + i0) = make_float4(pv[0], pv[1], pv[2], pv[3]);
        *reinterpret_cast<float4*>(a.m + i0) = make_float4(mv[0], mv[1], mv[2], mv[3]);
        *reinterpret_cast<float4*>(a.v + i0) = make_float4(vv[0], vv[1], vv[2], vv[3]);
        if (a.write_grad) *reinterpret_cast<float4*>(a.g + i0) = make_float4(gv[0], gv[1], gv[2], gv[3]);
        if (EMA) *reinterpret_cast<float4*>(a.e + i0) = make_float4(ev[0], ev[1], ev[2], ev[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < a.n) {
                a.p[i0 + j] = pv[j]; a.m[i0 + j] = mv[j]; a.v[i0 + j] = vv[j];
                if (a.write_grad) a.g[i0 + j] = gv[j];
                if (EMA) a.e[i0 + j] = ev[j];
            }
    }
    }
}

// The launch of every entry: status codes, grid (one workgroup per 1024 elements, 2048 at most) and the shared arguments.
template <bool GUARDED, bool EMA>
static int adamw_flat_launch(AdamwArgs a, hipStream_t st) {
    if (a.n <= 0) return 0;
    if (a.nseg < 1 || a.nseg > ADAMW_MAXSEG) return -2;
    if ((reinterpret_cast<uintptr_t>(a.p) | reinterpret_cast<uintptr_t>(a.g) | reinterpret_cast<uintptr_t>(a.m) | reinterpret_cast<uintptr_t>(a.v)) & 15) return -2;
    if (GUARDED && (a.guard == nullptr || (reinterpret_cast<uintptr_t>(a.guard) & 15))) return -2;
    if (EMA && (a.e == nullptr || (reinterpret_cast<uintptr_t>(a.e) & 15) || !(a.ema_decay >= 0.0 && a.ema_decay < 1.0))) return -2;   // NaN: refused
    long nb = (a.n + 1023) / 1024; if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL((adamw_flat_kernel<GUARDED, EMA>), dim3((unsigned)nb), dim3(256), 0, st, a);
    SPE_CHECK_LAUNCH();
    return 0;
}

// The arguments the entries share; the EMA fields stay off unless spe_adamw_flat_ema sets them.
static AdamwArgs adamw_args(float* p, float* g, float* m, float* v, long n, const long* seg_end, const float* seg_lr, const float* seg_wd,
                            int nseg, float beta1, float beta2, float eps, int write_grad) {
    AdamwArgs a;
    a.p = p; a.g = g; a.m = m; a.v = v; a.n = n; a.seg_end = seg_end; a.seg_lr = seg_lr; a.seg_wd = seg_wd; a.nseg = nseg;
    a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.bc1 = 0.f; a.bc2sqrt = 0.f;
    a.partials = nullptr; a.npartials = 0; a.max_norm = 0.f; a.write_grad = write_grad; a.gscale = 0.f;
    a.guard = nullptr;
    a.e = nullptr; a.ema_decay = 0.0; a.ema_warmup = 0; a.ema_t = 0.f;
    return a;
}
static void adamw_args_unguarded(AdamwArgs& a, float bias_c1, float bias_c2, const float* partials, int npartials, float max_norm,
                                 float grad_scale) {
    a.bc1 = bias_c1; a.bc2sqrt = sqrtf(bias_c2);
    a.partials = partials; a.npartials = npartials; a.max_norm = max_norm; a.gscale = grad_scale;
}

// C-ABI: see include/spe_hip.h (spe_adamw_flat).  All flat buffers 16-B aligned, n elements.
extern "C" int spe_adamw_flat(float* p, float* g, float* m, float* v, long n, const long* seg_end, const float* seg_lr,
                              const float* seg_wd, int nseg, float beta1, float beta2, float eps, float bias_c1, float bias_c2,
                              const float* partials, int npartials, float max_norm, int write_grad, float grad_scale,
                              hipStream_t st) {
    AdamwArgs a = adamw_args(p, g, m, v, n, seg_end, seg_lr, seg_wd, nseg, beta1, beta2, eps, write_grad);
    adamw_args_unguarded(a, bias_c1, bias_c2, partials, npartials, max_norm, grad_scale);
    return adamw_flat_launch<false, false>(a, st);
}

// C-ABI: see include/spe_hip.h (spe_adamw_flat_guarded).
extern "C" int spe_adamw_flat_guarded(float* p, float* g, float* m, float* v, long n, const long* seg_end, const float* seg_lr,
                                      const float* seg_wd, int nseg, float beta1, float beta2, float eps, const void* guard,
                                      int write_grad, hipStream_t st) {
    AdamwArgs a = adamw_args(p, g, m, v, n, seg_end, seg_lr, seg_wd, nseg, beta1, beta2, eps, write_grad);
    a.guard = static_cast<const int*>(guard);
    return adamw_flat_launch<true, false>(a, st);
}

// C-ABI: see include/spe_hip.h (spe_adamw_flat_ema).  guard != NULL: the guarded update (bias_c1 .. grad_scale and t are ignored).
extern "C" int spe_adamw_flat_ema(float* p, float* g, float* m, float* v, float* e, long n, const long* seg_end, const float* seg_lr,
                                  const float* seg_wd, int nseg, float beta1, float beta2, float eps, float bias_c1, float bias_c2,
                                  const float* partials, int npartials, float max_norm, int write_grad, float grad_scale,
                                  const void* guard, double decay, int warmup, long t, hipStream_t st) {
    AdamwArgs a = adamw_args(p, g, m, v, n, seg_end, seg_lr, seg_wd, nseg, beta1, beta2, eps, write_grad);
    a.e = e; a.ema_decay = decay; a.ema_warmup = warmup != 0; a.ema_t = (float)t;
    if (guard != nullptr) {
        a.guard = static_cast<const int*>(guard);
        return adamw_flat_launch<true, true>(a, st);
    }
    adamw_args_unguarded(a, bias_c1, bias_c2, partials, npartials, max_norm, grad_scale);
    return adamw_flat_launch<false, true>(a, st);
}
