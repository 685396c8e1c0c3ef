// What the two detection meters share on the device (voc_eval.hip, coco_eval.hip; DESIGN.md sections 8g and 8i): the limits, the
// search for an (image, class) segment, one step of the ground-truth compaction and the workgroup primitives of the curve kernels.
// Both files promise bit-for-bit agreement with numpy and are compiled with -ffp-contract=off.  Each helper here is the expression
// its callers used to spell out (the rule of common.h's float4 helpers), so every fp64 operation keeps its operand order; nothing in
// this header multiplies and adds.
#pragma once
#include "common.h"

#define EV_MAXDET 4096       // detections per image (the convention of spe_nms_sorted)
#define EV_THREADS 256       // workgroup of the curve kernels: the width of a chunk and of its carries

// first index in [lo, hi) whose key is >= v (class labels / category indices ascend inside an image)
__device__ __forceinline__ int ev_lower_bound(const long* __restrict__ key, int lo, int hi, long v) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (key[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// [s, e): the detections with key v among those of one image, [d0, d1)
__device__ __forceinline__ void ev_segment(const long* __restrict__ key, int d0, int d1, long v, int& s, int& e) {
    s = ev_lower_bound(key, d0, d1, v);
    e = ev_lower_bound(key, s, d1, v + 1);
}

// One 64-wide step of a compaction that keeps the incoming order: -> the slot of this lane's item (meaningful where `member`),
// count advanced by the members of the step.  Holds a ballot: the whole wave calls it, never a divergent branch.
__device__ __forceinline__ int ev_compact_slot(bool member, int lane, int& count) {
    const unsigned long long mask = __ballot(member);
    const int p = count + __popcll(mask & ((1ull << lane) - 1ull));
    count += __popcll(mask);
    return p;
}

// ---- workgroup primitives of the curve kernels (EV_THREADS threads; ws: EV_THREADS / 64 words of LDS) ----------------------------
// inclusive sum over the workgroup of (tp count | fp count << 16) - at most 256 of each per chunk; total: the chunk's sum
__device__ __forceinline__ int ev_scan(int v, int* ws, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(v, o, 64); if (lane >= o) v += t; }
    __syncthreads();
    if (lane == 63) ws[w] = v;
    __syncthreads();
    int off = 0; total = 0;
#pragma unroll
    for (int k = 0; k < EV_THREADS / 64; ++k) { if (k < w) off += ws[k]; total += ws[k]; }
    return v + off;
}
// v -> max over the threads >= this one (the precision envelope inside a chunk); total: the chunk's maximum
__device__ __forceinline__ double ev_suffix_max(double v, double* ws, double& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const double t = __shfl_down(v, o, 64); if (lane + o < 64) v = fmax(v, t); }
    __syncthreads();
    if (lane == 0) ws[w] = v;
    __syncthreads();
    total = ws[0];
#pragma unroll
    for (int k = 1; k < EV_THREADS / 64; ++k) { if (k > w) v = fmax(v, ws[k]); total = fmax(total, ws[k]); }
    return v;
}
// op over the workgroup in an order fixed by the thread layout: xor butterfly per wave, then the waves in index order
template <typename T, typename Op>
__device__ __forceinline__ T ev_reduce(T v, T* ws, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = ws[0];
#pragma unroll
    for (int k = 1; k < EV_THREADS / 64; ++k) r = op(r, ws[k]);
    return r;
}
__device__ __forceinline__ double ev_sum(double v, double* ws) { return ev_reduce(v, ws, [](double a, double b) { return a + b; }); }
__device__ __forceinline__ int ev_isum(int v, int* ws) { return ev_reduce(v, ws, [](int a, int b) { return a + b; }); }
__device__ __forceinline__ int ev_imin(int v, int* ws) { return ev_reduce(v, ws, [](int a, int b) { return min(a, b); }); }
