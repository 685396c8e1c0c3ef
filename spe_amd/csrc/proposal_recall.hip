// Proposal recall on the device (include/spe_hip.h: spe_proposal_recall): are the Q sparse proposals of a stage on
// the objects, or is the pick among them wrong?  PseudoLabelMeter (pseudo_quality.hip) scores only the one query per (image, class) that
// PostProcessRefine picks; this meter scores every ground-truth row against ALL Q query boxes of its image and counts, per class, the
// recall-at-k curve under the class's own ordering (k = 1 is exactly the refine pick) and the ceiling with all Q queries.  The reference
// has no route to these numbers: its evaluator sees only NMS survivors.  Counter-only: 2 + T + T * K 64-bit counters per class,
// accumulated in place, nothing read back.
//
// Rules (the package's own).  A ground-truth row g of image b with label c:
//   1. c outside [0, min(C, Kc)): gts[C] += 1 and nothing else.  Otherwise gts[c] += 1.
//   2. iou[q] for all Q queries of image b: util.box_ops.box_iou on box_cxcywh_to_xyxy of both rows in fp32, operation for operation -
//      box_iou_f32.h, shared with pseudo_quality.hip; this file is compiled without FMA contraction (spe_amd/build.py).
//   3. best = the maximum over the non-NaN iou[q].  Finite and > 0: iou_q[c] += llrint(min(best, 1) * 2^20).
//   4. Per threshold t the covering set S_t = { q : iou[q] > thr[t] } - strict, a NaN never covers.  Empty: nothing is counted for t.
//      Otherwise ceil[t][c] += 1; lead = the first element of S_t in CLASS c's ORDER of the image's queries by prob[b][q][c]: a NaN comes
//      before every number, NaNs among themselves by lower q, larger values first, equal values (+0.0 and -0.0 are equal) by lower q - a
//      total order whose first element is torch.max's and spe_refine_pick's pick.  r = the number of queries of the image that precede
//      lead in that order; hit[t][k][c] += 1 for every k with r < ks[k].
//   Counter rows [2 + T + T * K][C + 1]: 0 gts, 1 iou_q, 2 + t ceil[t], 2 + T + t * K + k hit[t][k].
//
//   ONE workgroup of PR_THREADS per image.  The image's Q boxes are staged once in LDS as corners plus area (20 bytes per query).  The four
//   waves stride over the image's ground-truth rows; per row a lane keeps the IoUs and the class's probabilities of its ceil(Q / 64) <= 16
//   queries in registers.  Per threshold: one wave-wide reduction to the order-first covering query, comparing (is-NaN, value, index),
//   then one counting pass for its rank - no sort and no rank of every query, O(T * Q) per row.  The thresholds ascend, so the covering
//   sets shrink: the first empty one ends the row.  Integer atomics only: the counters are a function of the input alone.
#include "common.h"
#include "box_iou_f32.h"

#define PR_THREADS 256
#define PR_MAX_Q 1024              // queries per image: the LDS staging (-2 beyond)
#define PR_MAX_TABLE 8             // thresholds, and cut-offs
#define PR_LANE_Q (PR_MAX_Q / SPE_WAVE)

// the two small tables travel by value in the launch arguments
struct PrTables {
    float thr[PR_MAX_TABLE];
    int ks[PR_MAX_TABLE];
};

// a query as the order sees it: its probability for the class and its index; q < 0: none
struct PrKey {
    float v;
    int q;
};

// a comes before b in the class's order (both are queries)
__device__ __forceinline__ bool pr_before(float av, int aq, float bv, int bq) {
    const bool an = av != av, bn = bv != bv;
    if (an || bn) return an && (!bn || aq < bq);
    return av > bv || (av == bv && aq < bq);
}

__device__ __forceinline__ PrKey pr_first(PrKey a, PrKey b) {
    if (a.q < 0) return b;
    if (b.q < 0) return a;
    return pr_before(a.v, a.q, b.v, b.q) ? a : b;
}

__device__ __forceinline__ void pr_add(long* counters, int C, int row, int c, long v) {
    atomicAdd(reinterpret_cast<unsigned long long*>(counters + (size_t)row * (C + 1) + c), (unsigned long long)v);
}

__global__ __launch_bounds__(PR_THREADS) void proposal_recall_kernel(const float* __restrict__ prob, const float* __restrict__ boxes,
                                                                     const float* __restrict__ gboxes, const long* __restrict__ glabels,
                                                                     const int* __restrict__ goff, int Q, int Kc, int C, int G, int T, int K,
                                                                     PrTables tab, long* counters) {
    __shared__ float4 q_xyxy[PR_MAX_Q];
    __shared__ float q_area[PR_MAX_Q];
    const int tid = threadIdx.x, b = blockIdx.x, lane = tid % SPE_WAVE, wave = tid / SPE_WAVE;
    const int g0 = goff[b], g1 = goff[b + 1];
    if (g0 < 0 || g1 < g0 || g1 > G || g0 == g1) return;                     // refused on the host, which knows the table; an image without rows
    for (int q = tid; q < Q; q += PR_THREADS) {
        const float4 c = pq_corners(boxes + ((size_t)b * Q + q) * 4);
        q_xyxy[q] = c;
        q_area[q] = pq_area(c);
    }
    __syncthreads();
    const int limit = C < Kc ? C : Kc;
    for (int g = g0 + wave; g < g1; g += PR_THREADS / SPE_WAVE) {           // everything below is uniform over the wave
        const long label = glabels[g];
        if (label < 0 || label >= (long)limit) {
            if (lane == 0) pr_add(counters, C, 0, C, 1);
            continue;
        }
        const int c = (int)label;
        const float4 gt = pq_corners(gboxes + (size_t)g * 4);
        const float ga = pq_area(gt);
        const float* col = prob + (size_t)b * Q * Kc + c;
        float iou[PR_LANE_Q], p[PR_LANE_Q];
        float best = -INFINITY;                                              // below every IoU: a row whose IoUs are all NaN keeps it
#pragma unroll
        for (int i = 0; i < PR_LANE_Q; ++i) {
            const int q = i * SPE_WAVE + lane;
            iou[i] = NAN;                                                    // past Q: never covers, never the best
            p[i] = 0.f;
            if (q < Q) {
                iou[i] = pq_iou(q_xyxy[q], q_area[q], gt, ga);
                p[i] = col[(size_t)q * Kc];
                if (iou[i] > best) best = iou[i];                            // a NaN never wins
            }
        }
#pragma unroll
        for (int s = SPE_WAVE / 2; s > 0; s >>= 1) {
            const float o = __shfl_xor(best, s);
            if (o > best) best = o;
        }
        if (lane == 0) {
            pr_add(counters, C, 0, c, 1);
            if (best > 0.f && best < INFINITY) pr_add(counters, C, 1, c, pq_iou_quantum(best));
        }
        for (int t = 0; t < T; ++t) {
            const float thr = tab.thr[t];
            if (!(best > thr)) break;                                        // S_t is empty, and so is every later one
            PrKey lead = {0.f, -1};
#pragma unroll
            for (int i = 0; i < PR_LANE_Q; ++i)                              // ascending q inside a lane: an equal value keeps the earlier
                if (iou[i] > thr && (lead.q < 0 || pr_before(p[i], i * SPE_WAVE + lane, lead.v, lead.q))) lead = {p[i], i * SPE_WAVE + lane};
#pragma unroll
            for (int s = SPE_WAVE / 2; s > 0; s >>= 1) {
                const PrKey o = {__shfl_xor(lead.v, s), __shfl_xor(lead.q, s)};
                lead = pr_first(lead, o);
            }
            int r = 0;
#pragma unroll
            for (int i = 0; i < PR_LANE_Q; ++i) {
                const int q = i * SPE_WAVE + lane;
                if (q < Q && pr_before(p[i], q, lead.v, lead.q)) ++r;
            }
#pragma unroll
            for (int s = SPE_WAVE / 2; s > 0; s >>= 1) r += __shfl_xor(r, s);
            if (lane == PR_MAX_TABLE) pr_add(counters, C, 2 + t, c, 1);
            for (int k = 0; k < K; ++k)                                      // lane k adds hit[t][k]; the table is read with a uniform index
                if (lane == k && r < tab.ks[k]) pr_add(counters, C, 2 + T + t * K + k, c, 1);
        }
    }
}

// C-ABI: see include/spe_hip.h
extern "C" int spe_proposal_recall(const float* prob, const float* boxes, const float* gboxes, const long* glabels, const int* goff,
                                   const int* goff_host, int B, int Q, int Kc, int G, int C, const float* thr, int T, const int* ks, int K,
                                   long* counters, hipStream_t st) {
    if (B < 0 || G < 0 || Q < 1 || Kc < 1 || C < 1 || T < 1 || T > PR_MAX_TABLE || K < 1 || K > PR_MAX_TABLE) return -3;
    if (!goff_host || !thr || !ks || !counters) return -3;
    for (int t = 0; t < T; ++t)
        if (!(thr[t] - thr[t] == 0.f) || (t > 0 && !(thr[t] > thr[t - 1]))) return -3;       // finite, strictly ascending
    for (int k = 0; k < K; ++k)
        if (ks[k] < 1 || (k > 0 && ks[k] <= ks[k - 1])) return -3;
    if (goff_host[0] != 0 || goff_host[B] != G) return -3;
    for (int b = 0; b < B; ++b)
        if (goff_host[b + 1] < goff_host[b]) return -3;
    if (Q > PR_MAX_Q) return -2;
    if (B == 0 || G == 0) return 0;                                              // nothing to count
    if (!prob || !boxes || !gboxes || !glabels || !goff) return -3;
    PrTables tab = {};
    for (int t = 0; t < T; ++t) tab.thr[t] = thr[t];
    for (int k = 0; k < K; ++k) tab.ks[k] = ks[k];
    hipLaunchKernelGGL(proposal_recall_kernel, dim3(B), dim3(PR_THREADS), 0, st, prob, boxes, gboxes, glabels, goff, Q, Kc, C, G, T, K, tab,
                       counters);
    SPE_CHECK_LAUNCH();
    return 0;
}
