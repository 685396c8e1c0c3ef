// Multi-label classification AP on the device (reference cams_deit.py:493-574, AveragePrecisionMeter.average_precision; DESIGN.md
// section 8m): per class column the samples are walked in descending score, at every positive pos_count / total_count is added in
// fp64, in walk order, and the sum is divided by the number of positives.
//
// There is no sort.  The term of a positive depends only on two counts - how many counted samples, and how many positives among
// them, rank at or before it - so cls_ap_rank_kernel counts them by streaming the class row through LDS (one thread per sample, one
// 64-bit comparison per pair), and, the positives' ranks among the positives being a permutation of 1 .. P, drops the term at slot
// pos - 1 of the class's workspace row.  cls_ap_sum_kernel then adds the P slots of a class sequentially, in slot order - the
// reference's order of additions, which is the point: the result equals the Python loop bit for bit.
//
// The order: higher score first; scores that compare equal in fp32 (+0.0 and -0.0 included) by ascending sample index; NaN before
// every number, NaNs among themselves by index.  It is folded into one unsigned 64-bit word per sample (cls_ap_word), larger = earlier.
// Compiled with -ffp-contract=off like the other evaluators (spe_amd/build.py EXTRA_FLAGS); the only floating-point operations are the
// fp64 divisions and the sequential fp64 additions.  No atomics of any kind; nothing synchronises the host.
#include "det_eval_common.h"
#include <math.h>

#define CLS_AP_MAX_N (1 << 24)       // samples per class: the index takes 24 bits of the order word
#define CLS_AP_TILE EV_THREADS       // samples staged per step, and the workgroup of both kernels
#define CLS_AP_CHUNK 1024            // workspace slots staged per step of the sequential sum

// Order word of sample j: bits 63 .. 32 the score as an unsigned integer that ascends with it (all NaNs the largest value, -0.0
// read as +0.0), bits 31 .. 8 (2^24 - 1 - j), so that among equal scores the lower index is larger, bit 1 "positive", bit 0 "counted".
// Sample j ranks before sample i  <=>  word(j) > (word(i) | 0xff): the flag bits never decide, and j = i is never "before".
__device__ __forceinline__ unsigned long long cls_ap_word(float s, int t, int j, int difficult) {
    unsigned key;
    if (s != s) key = 0xffffffffu;
    else {
        const unsigned u = __float_as_uint(s == 0.0f ? 0.0f : s);
        key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    const unsigned counted = (difficult && t == 0) ? 0u : 1u, positive = t == 1 ? 2u : 0u;
    return ((unsigned long long)key << 32) | ((unsigned long long)(unsigned)(CLS_AP_MAX_N - 1 - j) << 8) | positive | counted;
}

// grid (ceil(n / 256), C): thread t of block b owns sample i = b * 256 + t of class blockIdx.y and meets every sample of the row.
__global__ __launch_bounds__(CLS_AP_TILE) void cls_ap_rank_kernel(const float* __restrict__ scores, const signed char* __restrict__ targets,
                                                                  int n, long ld, int difficult, double* __restrict__ ws) {
    __shared__ unsigned long long tile[CLS_AP_TILE];
    const int c = blockIdx.y, tid = threadIdx.x;
    const float* s = scores + (long)c * ld;
    const signed char* t = targets + (long)c * ld;
    const int i = blockIdx.x * CLS_AP_TILE + tid;
    const unsigned long long own = i < n ? cls_ap_word(s[i], t[i], i, difficult) : 0ull;
    const bool positive = (own & 2ull) != 0ull;
    const bool wave_works = __any(positive);                                // a wave without a positive only helps staging
    const unsigned long long bar = own | 0xffull;
    int tot = 1, pos = 1;                                                    // "at or before": the positive itself
    for (int base = 0; base < n; base += CLS_AP_TILE) {
        const int j = base + tid;
        tile[tid] = j < n ? cls_ap_word(s[j], t[j], j, difficult) : 0ull;    // past the row: neither counted nor before anything
        __syncthreads();
        if (wave_works) {
#pragma unroll 8
            for (int k = 0; k < CLS_AP_TILE; ++k) {
                const unsigned long long w = tile[k];                        // one address for the whole wave: a broadcast
                const bool before = w > bar;
                tot += before ? (int)(w & 1ull) : 0;
                pos += before ? (int)((w >> 1) & 1ull) : 0;
            }
        }
        __syncthreads();
    }
    if (positive) ws[(long)c * n + (pos - 1)] = (double)pos / (double)tot;
}

// One workgroup per class: the counts, then the P terms in slot order, staged through LDS and added by one thread.
__global__ __launch_bounds__(CLS_AP_TILE) void cls_ap_sum_kernel(const signed char* __restrict__ targets, int n, long ld, int difficult,
                                                                 const double* __restrict__ ws, double* __restrict__ ap,
                                                                 int* __restrict__ npos, int* __restrict__ ncounted) {
    __shared__ int iws[CLS_AP_TILE / 64];
    __shared__ double buf[CLS_AP_CHUNK];
    const int c = blockIdx.x, tid = threadIdx.x;
    const signed char* t = targets + (long)c * ld;
    int p = 0, q = 0;
    for (int j = tid; j < n; j += CLS_AP_TILE) {
        const int v = t[j];
        p += v == 1;
        q += !(difficult && v == 0);
    }
    const int P = ev_isum(p, iws);
    const int Q = ev_isum(q, iws);
    const double* w = ws + (long)c * n;
    double sum = 0.;
    for (int base = 0; base < P; base += CLS_AP_CHUNK) {
        const int m = min(CLS_AP_CHUNK, P - base);
        __syncthreads();
        for (int k = tid; k < m; k += CLS_AP_TILE) buf[k] = w[base + k];
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < m; ++k) sum += buf[k];                       // precision_at_i += pos_count / total_count, in walk order
    }
    if (tid == 0) {
        ap[c] = P > 0 ? sum / (double)P : (double)NAN;                       // the reference divides by zero here (ZeroDivisionError)
        npos[c] = P;
        ncounted[c] = Q;
    }
}

// C-ABI: see include/spe_hip.h (spe_cls_ap).
extern "C" int spe_cls_ap_workspace(int n, int C, size_t* bytes) {
    if (!bytes || n < 0 || n > CLS_AP_MAX_N || C < 1 || C > 65535) return -2;
    *bytes = (size_t)n * (size_t)C * sizeof(double);
    return 0;
}

extern "C" int spe_cls_ap(const float* scores, const signed char* targets, int n, int C, long ld, int difficult, double* workspace,
                          double* ap, int* npos, int* ncounted, hipStream_t st) {
    if (n < 0 || n > CLS_AP_MAX_N || C < 1 || C > 65535 || ld < n) return -2;
    if (n > 0 && !workspace) return -4;
    if (n > 0) {
        hipLaunchKernelGGL(cls_ap_rank_kernel, dim3((unsigned)((n + CLS_AP_TILE - 1) / CLS_AP_TILE), (unsigned)C), dim3(CLS_AP_TILE), 0, st,
                           scores, targets, n, ld, difficult, workspace);
        SPE_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(cls_ap_sum_kernel, dim3((unsigned)C), dim3(CLS_AP_TILE), 0, st, targets, n, ld, difficult, workspace, ap, npos,
                       ncounted);
    SPE_CHECK_LAUNCH();
    return 0;
}
