// Training targets on the device (include/spe_hip.h: spe_cam_targets, spe_refine_pick): what the training loop
// does between the forward and the criterion, where the data already is.
//
//   spe_cam_targets   the packed result of spe_cam_boxes_device (counts, then integer boxes [x, y, x+w, y+h]) -> the stage-0 target rows
//                     of the whole batch: normalised cxcywh boxes, labels, and the row offset of every map.  The reference builds them on
//                     the host (engine.py:356-398: a list per class, torch.cat, the division by [W, H, W, H]).  ONE workgroup: an exclusive
//                     scan of the row counts over the M maps in chunks of TT_THREADS with a carry, then one thread per output row.
//   spe_refine_pick   PostProcessRefine (reference models/conditional_detr.py:641-677) behind its sigmoid: for every (image, present class)
//                     pair the best query by torch.max's rule, its probability and its box.  One wave per pair, the lanes stride over
//                     the queries; no atomics, every tie broken by the query index, so the result is a function of the input alone.
//
// This file is compiled without FMA contraction (spe_amd/build.py), and the arithmetic that must match the host's elementwise composition
// is spelled with the _rn intrinsics besides: one rounding per operation.
#include "common.h"

#define TT_THREADS 256
#define TT_WAVES (TT_THREADS / SPE_WAVE)
#define TT_MAXM 65535             // the map limit of spe_cam_boxes_device
#define TT_MAXBOXES 2048          // its max_boxes limit

// rows a map contributes: a negative count is a status (0 rows), `single` keeps the first box only
__device__ __forceinline__ int tt_rows(int n, int max_boxes, int single) {
    if (n <= 0) return 0;
    if (single) return 1;
    return n < max_boxes ? n : max_boxes;
}

__global__ __launch_bounds__(TT_THREADS) void cam_targets_kernel(const int* __restrict__ packed, const int* __restrict__ cls0, int M,
                                                                 int max_boxes, int single, float Wf, float Hf, int cap,
                                                                 float* __restrict__ out_boxes, long* __restrict__ out_labels, int* off) {
    __shared__ int wsum[TT_WAVES];
    __shared__ int carry_s;
    const int tid = threadIdx.x, lane = tid & (SPE_WAVE - 1), wave = tid / SPE_WAVE;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    // exclusive scan of the row counts, TT_THREADS maps at a time
    for (int base = 0; base < M; base += TT_THREADS) {
        const int m = base + tid;
        const int r = m < M ? tt_rows(packed[m], max_boxes, single) : 0;
        int incl = r;
#pragma unroll
        for (int o = 1; o < SPE_WAVE; o <<= 1) {
            const int t = __shfl_up(incl, o, SPE_WAVE);
            if (lane >= o) incl += t;
        }
        if (lane == SPE_WAVE - 1) wsum[wave] = incl;
        __syncthreads();
        int before = carry_s, total = 0;
#pragma unroll
        for (int w = 0; w < TT_WAVES; ++w) {
            if (w < wave) before += wsum[w];
            total += wsum[w];
        }
        if (m < M) off[m] = before + incl - r;
        __syncthreads();                                  // everyone has read carry_s and wsum
        if (tid == 0) carry_s += total;
        __syncthreads();
    }
    const int T = carry_s;
    if (tid == 0) off[M] = T;
    __threadfence_block();
    __syncthreads();                                      // off[] is read back below by other threads of this workgroup
    const int* boxes = packed + M;
    for (int row = tid; row < T && row < cap; row += TT_THREADS) {
        int lo = 0, hi = M;                               // the last m with off[m] <= row: maps without rows share their successor's offset
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (off[mid] <= row) lo = mid; else hi = mid;
        }
        const int m = lo, j = row - off[m];
        const int* bp = boxes + ((size_t)m * max_boxes + j) * 4;           // 4-byte aligned only: M counts lie in front
        const int4 b = make_int4(bp[0], bp[1], bp[2], bp[3]);
        // _xyxy_to_cxcywh on integers, true division, then / [W, H, W, H] in fp32 (spe_amd/camboxes.py)
        const float cx = __fdiv_rn(__fdiv_rn(__int2float_rn(b.x + b.z), 2.f), Wf);
        const float cy = __fdiv_rn(__fdiv_rn(__int2float_rn(b.y + b.w), 2.f), Hf);
        const float w = __fdiv_rn(__int2float_rn(b.z - b.x), Wf);
        const float h = __fdiv_rn(__int2float_rn(b.w - b.y), Hf);
        *reinterpret_cast<float4*>(out_boxes + (size_t)row * 4) = make_float4(cx, cy, w, h);
        out_labels[row] = (long)cls0[m] + 1;
    }
}

// (value, query) of the better candidate by torch.max's rule: a NaN beats every number, the first NaN wins; the largest value wins; equal
// values: the lowest query.  q < 0: no candidate.
__device__ __forceinline__ bool tt_better(float av, int aq, float bv, int bq) {
    if (bq < 0) return aq >= 0;
    if (aq < 0) return false;
    const bool an = av != av, bn = bv != bv;
    if (an || bn) return an && (!bn || aq < bq);
    if (av != bv) return av > bv;
    return aq < bq;
}

__global__ __launch_bounds__(TT_THREADS) void refine_pick_kernel(const float* __restrict__ prob, const float* __restrict__ pred_boxes,
                                                                 const int* __restrict__ cls, const int* __restrict__ cls_off, int B, int Q,
                                                                 int Kc, int U, float* __restrict__ scores, int* __restrict__ queries,
                                                                 float* __restrict__ boxes) {
    const int lane = threadIdx.x & (SPE_WAVE - 1);
    const int u = blockIdx.x * TT_WAVES + threadIdx.x / SPE_WAVE;              // wave-uniform
    if (u >= U) return;
    int lo = 0, hi = B;                                                         // the last image with cls_off[b] <= u
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cls_off[mid] <= u) lo = mid; else hi = mid;
    }
    const int b = lo, c = cls[u];
    if (c < 0 || c >= Kc) return;                                               // refused on the host where it can see the table; never read
    const float* p = prob + (size_t)b * Q * Kc + c;
    float bv = 0.f;
    int bq = -1;
    for (int q = lane; q < Q; q += SPE_WAVE) {
        const float v = p[(size_t)q * Kc];
        if (tt_better(v, q, bv, bq)) { bv = v; bq = q; }
    }
#pragma unroll
    for (int o = SPE_WAVE / 2; o > 0; o >>= 1) {
        const int ov = __shfl_xor(__float_as_int(bv), o, SPE_WAVE), oq = __shfl_xor(bq, o, SPE_WAVE);
        if (tt_better(__int_as_float(ov), oq, bv, bq)) { bv = __int_as_float(ov); bq = oq; }
    }
    if (lane == 0) {
        scores[u] = bv;                                                         // the winner's own bits, a NaN's payload included
        queries[u] = bq;
    }
    if (lane < 4) boxes[(size_t)u * 4 + lane] = pred_boxes[((size_t)b * Q + bq) * 4 + lane];
}

// C-ABI: see include/spe_hip.h
extern "C" int spe_cam_targets(const int* packed, const int* cls0, int M, int max_boxes, int single, int W, int H, int cap, float* boxes,
                               long* labels, int* off, hipStream_t st) {
    if (M < 0 || max_boxes < 1 || W < 1 || H < 1 || cap < 0) return -3;
    if (M > TT_MAXM || max_boxes > TT_MAXBOXES) return -2;
    if ((long)cap < (long)M * (single ? 1 : max_boxes)) return -3;              // the worst case must fit: the counts are not known here
    if (!off || (M > 0 && (!packed || !cls0 || !boxes || !labels))) return -3;   // no map: only off[0] = 0 is written
    if ((uintptr_t)boxes & 15) return -3;                                       // a row is stored as one float4
    hipLaunchKernelGGL(cam_targets_kernel, dim3(1), dim3(TT_THREADS), 0, st, packed, cls0, M, max_boxes, single, (float)W, (float)H, cap,
                       boxes, labels, off);
    SPE_CHECK_LAUNCH();
    return 0;
}

extern "C" int spe_refine_pick(const float* prob, const float* pred_boxes, const int* cls, const int* cls_off, const int* cls_host,
                               const int* cls_off_host, int B, int Q, int Kc, int U, float* scores, int* queries, float* boxes,
                               hipStream_t st) {
    if (B < 0 || Q < 1 || Kc < 1 || U < 0) return -3;                            // torch.max over an empty query axis raises too
    if (cls_off_host) {
        if (cls_off_host[0] != 0 || cls_off_host[B] != U) return -3;
        for (int b = 0; b < B; ++b)
            if (cls_off_host[b + 1] < cls_off_host[b]) return -3;
    }
    if (cls_host)
        for (int u = 0; u < U; ++u)
            if (cls_host[u] < 0 || cls_host[u] >= Kc) return -3;
    if (U == 0) return 0;
    if (B < 1 || !prob || !pred_boxes || !cls || !cls_off || !scores || !queries || !boxes) return -3;
    hipLaunchKernelGGL(refine_pick_kernel, dim3((U + TT_WAVES - 1) / TT_WAVES), dim3(TT_THREADS), 0, st, prob, pred_boxes, cls, cls_off,
                       B, Q, Kc, U, scores, queries, boxes);
    SPE_CHECK_LAUNCH();
    return 0;
}
