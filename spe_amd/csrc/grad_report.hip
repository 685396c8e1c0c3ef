// Per-parameter gradient report on the flat buckets of the optimizer (FlatAdamW(skip_report=...), FlatAdamW.grad_stats()): which
// parameter carried the NaN / infinity / overflowing square behind a skipped step, and the gradient and weight norms of every
// parameter.  No reference site: the reference exits on a non-finite loss (engine.py:147-159) and logs no per-layer norms.
// Contract, record layout and the summation order: include/spe_hip.h (spe_grad_report); the numpy restatement of the order is
// tests/grad_report_ref.py.  The file is built with -ffp-contract=off: every product and every addition below is rounded on its own.
//
// Two launches.  A parameter is cut into chunks of GR_CHUNK elements counted from ITS OWN first element; one workgroup reduces one
// chunk (a streaming pass: 16-B loads, four passes in flight per lane) and leaves a partial record in the reduction workspace; the
// second launch, one workgroup per parameter, folds that parameter's partial records in chunk order.  So a record is a function of the
// parameter's values and length alone - nothing depends on the grid, on the neighbours or on where the parameter sits in the bucket -
// while the big parameters (1.6 M elements at cfg2) still spread over the chip.  The tables are on the device and the host never reads
// them: the grid of the first launch is the upper bound n / GR_CHUNK + npar of the chunk count, and every workgroup finds the
// (parameter, chunk) of its slot by a prefix sum over the table of lengths.  The kernel boundary orders the partial records before
// their fold: plain stores, no tickets, no atomics.
#include "det_reduce.h"
#include <limits.h>

#define GR_THREADS 256
#define GR_SPAN (4L * GR_THREADS)          // elements one pass of the workgroup covers
#define GR_CHUNK (16L * GR_SPAN)           // elements of one chunk: 16 passes
#define GR_WORDS 8

// running state of one lane; after the block reductions, a chunk's partial record
struct GrPart {
    float gsq, gmax, psq, pmax;
    int nan, inf, first;                   // first: INT_MAX while no non-finite element was met
};

__device__ __forceinline__ int gr_chunks(long len) { return len > 0 ? (int)((len + GR_CHUNK - 1) / GR_CHUNK) : 0; }

// the gate: true when this launch has nothing to write (every lane reads the same words: the whole workgroup leaves together)
__device__ __forceinline__ bool gr_gated_out(const int* __restrict__ guard, int when, int& attempt) {
    attempt = 0;
    if (guard == nullptr) return false;
    const int applied = guard[0], skipped = guard[1], apply = guard[3];
    attempt = applied + skipped;
    return when != 0 && (apply != 0 || (when == 2 && skipped != 1));
}

// vector q of a chunk = its elements 4q .. 4q + 3, elements past the end read as +0.0.  16-B load where the parameter starts on a
// 16-B boundary (always, in the optimizer's buckets), scalar loads otherwise: the values - and so the record - are the same.
__device__ __forceinline__ void gr_load4(const float* __restrict__ x, long i, long len, bool vec, float (&v)[4]) {
    if (vec && i + 3 < len) {
        const float4 t = *reinterpret_cast<const float4*>(x + i);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i + j < len ? x[i + j] : 0.f;
    }
}

// four gradient elements starting at index i of the parameter: a non-finite one is counted and then taken as +0.0
__device__ __forceinline__ void gr_take_g(GrPart& s, const float (&v)[4], long i, float scale) {
    float q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float x = v[j];
        const uint32_t b = __float_as_uint(x);
        if ((b & 0x7f800000u) == 0x7f800000u) {
            if (b & 0x007fffffu) ++s.nan; else ++s.inf;
            if (s.first == INT_MAX) s.first = (int)(i + j);          // a lane meets its elements in ascending order
            x = 0.f;
        }
        const float t = scale * x;
        q[j] = t * t;
        s.gmax = fmaxf(s.gmax, fabsf(t));
    }
    s.gsq = s.gsq + ((q[0] + q[1]) + (q[2] + q[3]));
}
__device__ __forceinline__ void gr_take_p(GrPart& s, const float (&v)[4]) {
    float q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        q[j] = v[j] * v[j];
        s.pmax = fmaxf(s.pmax, fabsf(v[j]));
    }
    s.psq = s.psq + ((q[0] + q[1]) + (q[2] + q[3]));
}

// integer block reductions in the shape of spe_block_sum (`red`: GR_THREADS / 64 ints of LDS); exact, so their order is free
template <bool MIN>
__device__ __forceinline__ int gr_block_int(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int w = __shfl_xor(v, o, 64);
        v = MIN ? min(v, w) : v + w;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    int r = MIN ? INT_MAX : 0;
    for (int i = 0; i < GR_THREADS / 64; ++i) r = MIN ? min(r, red[i]) : r + red[i];
    return r;
}
// inclusive prefix sum of v over the lanes of the workgroup; `total`: the sum over all of them
__device__ __forceinline__ int gr_block_scan(int v, int* red, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    __syncthreads();
    if (lane == 63) red[w] = v;
    __syncthreads();
    int before = 0;
    total = 0;
    for (int i = 0; i < GR_THREADS / 64; ++i) {
        if (i < w) before += red[i];
        total += red[i];
    }
    return v + before;
}

// First launch: slot blockIdx.x of nslots -> the partial record of one chunk, at part + 8 * slot.  The chunks of parameter 0 take the
// first slots, those of parameter 1 the next ones, ...; slots past the last chunk have no work.
template <bool HAS_P>
__global__ __launch_bounds__(GR_THREADS) void grad_report_chunk_kernel(const float* __restrict__ g, const float* __restrict__ p,
                                                                       const long* __restrict__ par_beg, const long* __restrict__ par_len,
                                                                       int npar, float scale, const int* __restrict__ guard, int when,
                                                                       uint32_t* __restrict__ part) {
    __shared__ float red[16];
    __shared__ int redi[GR_THREADS / 64];
    __shared__ int s_own[2];
    int attempt;
    if (gr_gated_out(guard, when, attempt)) return;
    const int slot = blockIdx.x;
    if (threadIdx.x == 0) s_own[0] = -1;                 // (ordered before the owner's store by the barriers of the scan)
    int base = 0;
    for (int t0 = 0; t0 < npar; t0 += GR_THREADS) {      // workgroup-uniform: base and slot are the same in every lane
        const int j = t0 + threadIdx.x;
        const int cnt = j < npar ? gr_chunks(par_len[j]) : 0;
        int total;
        const int incl = base + gr_block_scan(cnt, redi, total);
        if (cnt > 0 && incl - cnt <= slot && slot < incl) { s_own[0] = j; s_own[1] = slot - (incl - cnt); }
        base += total;
        if (base > slot) break;
    }
    __syncthreads();
    const int par = s_own[0];
    if (par < 0) return;
    const long c0 = (long)s_own[1] * GR_CHUNK;           // the chunk's first element, counted from the parameter's
    const long beg = par_beg[par] + c0;
    long len = par_len[par] - c0; if (len > GR_CHUNK) len = GR_CHUNK;
    const float* __restrict__ gp = g + beg;
    const float* __restrict__ pp = HAS_P ? p + beg : nullptr;
    const bool vec = (reinterpret_cast<uintptr_t>(gp) & 15) == 0;          // p is aligned like g: the same offset into an aligned buffer
    GrPart s = {0.f, 0.f, 0.f, 0.f, 0, 0, INT_MAX};
    long i = 4L * threadIdx.x;
    if (vec) {                                           // four passes per trip, all loads issued ahead of the sums; the sums keep pass order
        for (; i + 3 * GR_SPAN + 3 < len; i += 4 * GR_SPAN) {
            float4 G[4], P[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                G[u] = *reinterpret_cast<const float4*>(gp + i + u * GR_SPAN);
                if (HAS_P) P[u] = *reinterpret_cast<const float4*>(pp + i + u * GR_SPAN);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float gv[4] = {G[u].x, G[u].y, G[u].z, G[u].w};
                gr_take_g(s, gv, c0 + i + u * GR_SPAN, scale);
                if (HAS_P) {
                    const float pv[4] = {P[u].x, P[u].y, P[u].z, P[u].w};
                    gr_take_p(s, pv);
                }
            }
        }
    }
    for (; i < len; i += GR_SPAN) {
        float gv[4], pv[4];
        gr_load4(gp, i, len, vec, gv);
        gr_take_g(s, gv, c0 + i, scale);
        if (HAS_P) {
            gr_load4(pp, i, len, vec, pv);
            gr_take_p(s, pv);
        }
    }
    const float gsq = spe_block_sum(s.gsq, red);
    const float psq = HAS_P ? spe_block_sum(s.psq, red) : 0.f;
    const float gmax = spe_block_max(s.gmax, red);
    const float pmax = HAS_P ? spe_block_max(s.pmax, red) : 0.f;
    const int nan = gr_block_int<false>(s.nan, redi);
    const int inf = gr_block_int<false>(s.inf, redi);
    const int first = gr_block_int<true>(s.first, redi);
    if (threadIdx.x == 0) {
        uint4* o = reinterpret_cast<uint4*>(part + (long)slot * GR_WORDS);
        o[0] = make_uint4(__float_as_uint(gsq), __float_as_uint(gmax), __float_as_uint(psq), __float_as_uint(pmax));
        o[1] = make_uint4((uint32_t)nan, (uint32_t)inf, (uint32_t)first, 0u);
    }
}

// Second launch: workgroup i folds the partial records of parameter i, chunk 0 first, and stores record i.
__global__ __launch_bounds__(GR_THREADS) void grad_report_fold_kernel(const long* __restrict__ par_len, const int* __restrict__ guard, int when,
                                                                      const uint32_t* __restrict__ part, int nslots, uint32_t* __restrict__ out) {
    __shared__ int redi[GR_THREADS / 64];
    __shared__ uint4 s_rec[GR_THREADS][2];
    int attempt;
    if (gr_gated_out(guard, when, attempt)) return;
    const int par = blockIdx.x;
    int before = 0;                                      // the slots of the parameters in front of this one
    for (int j = threadIdx.x; j < par; j += GR_THREADS) before += gr_chunks(par_len[j]);
    const int slot0 = gr_block_int<false>(before, redi);
    const int nch = gr_chunks(par_len[par]);
    GrPart s = {0.f, 0.f, 0.f, 0.f, 0, 0, INT_MAX};
    for (int c0 = 0; c0 < nch; c0 += GR_THREADS) {
        const int slot = slot0 + c0 + threadIdx.x;
        if (c0 + threadIdx.x < nch && slot < nslots) {   // (slot < nslots holds for tables that keep the contract; no read past the workspace otherwise)
            const uint4* r = reinterpret_cast<const uint4*>(part + (long)slot * GR_WORDS);
            s_rec[threadIdx.x][0] = r[0]; s_rec[threadIdx.x][1] = r[1];
        } else {
            s_rec[threadIdx.x][0] = make_uint4(0u, 0u, 0u, 0u); s_rec[threadIdx.x][1] = make_uint4(0u, 0u, (uint32_t)INT_MAX, 0u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = min(GR_THREADS, nch - c0);
            for (int k = 0; k < m; ++k) {
                const uint4 a = s_rec[k][0], b = s_rec[k][1];
                s.gsq = s.gsq + __uint_as_float(a.x);
                s.gmax = fmaxf(s.gmax, __uint_as_float(a.y));
                s.psq = s.psq + __uint_as_float(a.z);
                s.pmax = fmaxf(s.pmax, __uint_as_float(a.w));
                s.nan += (int)b.x; s.inf += (int)b.y;
                s.first = min(s.first, (int)b.z);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        uint4* o = reinterpret_cast<uint4*>(out + (long)par * GR_WORDS);
        o[0] = make_uint4(__float_as_uint(s.gsq), __float_as_uint(s.gmax), __float_as_uint(s.psq), __float_as_uint(s.pmax));
        o[1] = make_uint4((uint32_t)s.nan, (uint32_t)s.inf, (uint32_t)(s.first == INT_MAX ? -1 : s.first), (uint32_t)attempt);
    }
}

// C-ABI: see include/spe_hip.h (spe_grad_report).
extern "C" int spe_grad_report(const float* g, const float* p, long n, const long* par_beg, const long* par_len, int npar,
                               float grad_scale, const void* guard, int when, void* out, hipStream_t st) {
    if (g == nullptr || out == nullptr || ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(out)) & 15)) return -2;
    if (reinterpret_cast<uintptr_t>(p) & 15) return -2;
    if (par_beg == nullptr || par_len == nullptr || npar < 1 || when < 0 || when > 2) return -2;
    if ((when != 0 && guard == nullptr) || (reinterpret_cast<uintptr_t>(guard) & 15)) return -2;
    if (n <= 0) return 0;
    const long nslots = (n + GR_CHUNK - 1) / GR_CHUNK + npar;          // >= the number of chunks: sum of ceil(len / GR_CHUNK) over disjoint ranges of [0, n)
    const DetWs ws = spe_detws();
    if (ws.slab == nullptr || nslots * GR_WORDS > ws.slab_floats || nslots > INT_MAX) return -4;
    const int* gd = static_cast<const int*>(guard);
    uint32_t* part = reinterpret_cast<uint32_t*>(ws.slab);
    if (p != nullptr)
        hipLaunchKernelGGL(grad_report_chunk_kernel<true>, dim3((unsigned)nslots), dim3(GR_THREADS), 0, st, g, p, par_beg, par_len, npar,
                           grad_scale, gd, when, part);
    else
        hipLaunchKernelGGL(grad_report_chunk_kernel<false>, dim3((unsigned)nslots), dim3(GR_THREADS), 0, st, g, p, par_beg, par_len, npar,
                           grad_scale, gd, when, part);
    SPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(grad_report_fold_kernel, dim3((unsigned)npar), dim3(GR_THREADS), 0, st, par_len, gd, when, part, (int)nslots,
                       static_cast<uint32_t*>(out));
    SPE_CHECK_LAUNCH();
    return 0;
}
