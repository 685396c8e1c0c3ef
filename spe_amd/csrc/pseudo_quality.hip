// Pseudo-label quality on the device (include/spe_hip.h: spe_pseudo_quality): how good the boxes are that the
// training loop feeds its criteria - the CAM boxes of stage 0, PostProcessRefine's picks of the later stages - measured against the
// loader's ground-truth rows while training runs.  The reference only has the route through its evaluator (engine_loc.py:204-220,
// pseudo_label_to_det_out); this is a counter-only meter: ten 64-bit counters per class, accumulated in place, nothing read back.
//
//   ONE workgroup of PQ_THREADS per image.  The image's ground-truth rows (as corners and areas), both label vectors, a hit flag per pseudo
//   row and a covered flag per ground-truth row live in LDS.  Three phases with a barrier between them:
//     1. stage: corners / areas / labels of the ground truth, labels of the pseudo rows; `rows` and `gts` are counted here, a label
//        outside [0, C) in column C, and such a row takes no further part (its staged label is -1);
//     2. one thread per pseudo row walks the ground-truth rows of its label: best IoU, hit, orphan, the quantised IoU; it marks the
//        ground-truth rows it covers;
//     3. one thread per ground-truth row: covered; the FIRST row of a class in the image stands for the (image, class) pair and walks
//        the pseudo rows of the class: lead row, any hit, empty.
//   Integer atomics only: the counters are a function of the input alone.
//
// The IoU is util.box_ops.box_iou on box_cxcywh_to_xyxy of both rows in fp32, operation for operation (corners, areas, max / min,
// clamp(min=0), inter, (area1 + area2) - inter, the division): box_iou_f32.h, shared with proposal_recall.hip.  This file is compiled
// without FMA contraction (spe_amd/build.py) and the header spells the arithmetic with the _rn intrinsics besides: one rounding per operation.
#include "common.h"
#include "box_iou_f32.h"

#define PQ_THREADS 256
#define PQ_MAX_ROWS 1024           // pseudo rows and ground-truth rows per image (-2 beyond)
#define PQ_COUNTERS 10

enum { PQ_PAIRS = 0, PQ_PAIRS_LEAD_HIT, PQ_PAIRS_ANY_HIT, PQ_PAIRS_EMPTY, PQ_ROWS, PQ_ROWS_HIT, PQ_ROWS_ORPHAN, PQ_GTS, PQ_GTS_COVERED, PQ_IOU_Q };

__device__ __forceinline__ void pq_add(long* counters, int C, int k, int c, long v) {
    atomicAdd(reinterpret_cast<unsigned long long*>(counters + (size_t)k * (C + 1) + c), (unsigned long long)v);
}

// a label as the kernel keeps it: the class, or -1 for one outside [0, C)
__device__ __forceinline__ int pq_class(long l, int C) { return (l < 0 || l >= (long)C) ? -1 : (int)l; }

__global__ __launch_bounds__(PQ_THREADS) void pseudo_quality_kernel(const float* __restrict__ boxes, const long* __restrict__ labels,
                                                                    const float* __restrict__ scores, const int* __restrict__ off,
                                                                    const float* __restrict__ gboxes, const long* __restrict__ glabels,
                                                                    const int* __restrict__ goff, int C, float thr, long* counters) {
    __shared__ float4 g_xyxy[PQ_MAX_ROWS];
    __shared__ float g_area[PQ_MAX_ROWS];
    __shared__ int g_cls[PQ_MAX_ROWS];
    __shared__ int p_cls[PQ_MAX_ROWS];
    __shared__ unsigned char g_cov[PQ_MAX_ROWS];
    __shared__ unsigned char p_hit[PQ_MAX_ROWS];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int t0 = off[b], T = off[b + 1] - t0, g0 = goff[b], G = goff[b + 1] - g0;
    if (T < 0 || T > PQ_MAX_ROWS || G < 0 || G > PQ_MAX_ROWS) return;       // refused on the host, which knows both tables; never staged
    // 1. stage
    for (int g = tid; g < G; g += PQ_THREADS) {
        const float4 c = pq_corners(gboxes + (size_t)(g0 + g) * 4);
        const int cls = pq_class(glabels[g0 + g], C);
        g_xyxy[g] = c;
        g_area[g] = pq_area(c);
        g_cls[g] = cls;
        g_cov[g] = 0;
        pq_add(counters, C, PQ_GTS, cls < 0 ? C : cls, 1);
    }
    for (int t = tid; t < T; t += PQ_THREADS) {
        const int cls = pq_class(labels[t0 + t], C);
        p_cls[t] = cls;
        p_hit[t] = 0;
        pq_add(counters, C, PQ_ROWS, cls < 0 ? C : cls, 1);
    }
    __syncthreads();
    // 2. the pseudo rows
    for (int t = tid; t < T; t += PQ_THREADS) {
        const int cls = p_cls[t];
        if (cls < 0) continue;
        const float4 p = pq_corners(boxes + (size_t)(t0 + t) * 4);
        const float pa = pq_area(p);
        float best = -INFINITY;                                              // below every IoU: a row whose IoUs are all NaN keeps it
        bool same = false;
        for (int g = 0; g < G; ++g) {
            if (g_cls[g] != cls) continue;
            same = true;
            const float iou = pq_iou(p, pa, g_xyxy[g], g_area[g]);
            if (iou > best) best = iou;                                      // a NaN never wins
            if (iou > thr) g_cov[g] = 1;                                     // every writer stores the same 1
        }
        if (!same) {
            pq_add(counters, C, PQ_ROWS_ORPHAN, cls, 1);
            continue;
        }
        if (best > thr) {
            p_hit[t] = 1;
            pq_add(counters, C, PQ_ROWS_HIT, cls, 1);
        }
        if (best > 0.f && best < INFINITY) {
            pq_add(counters, C, PQ_IOU_Q, cls, pq_iou_quantum(best));
        }
    }
    __syncthreads();
    // 3. the ground-truth rows, and the pairs through the first row of every class
    for (int g = tid; g < G; g += PQ_THREADS) {
        const int cls = g_cls[g];
        if (cls < 0) continue;
        if (g_cov[g]) pq_add(counters, C, PQ_GTS_COVERED, cls, 1);
        bool first = true;
        for (int e = 0; e < g && first; ++e) first = g_cls[e] != cls;
        if (!first) continue;
        int lead = -1;
        float lead_s = 0.f;
        bool any = false;
        for (int t = 0; t < T; ++t) {
            if (p_cls[t] != cls) continue;
            any = any || p_hit[t];
            if (lead < 0) {
                lead = t;
                if (scores) lead_s = scores[t0 + t];
            } else if (scores && lead_s == lead_s) {                         // the first NaN goes before everything
                const float s = scores[t0 + t];
                if (s != s || s > lead_s) { lead = t; lead_s = s; }          // equal scores: the lowest row stays
            }
        }
        pq_add(counters, C, PQ_PAIRS, cls, 1);
        if (lead < 0) pq_add(counters, C, PQ_PAIRS_EMPTY, cls, 1);
        else if (p_hit[lead]) pq_add(counters, C, PQ_PAIRS_LEAD_HIT, cls, 1);
        if (any) pq_add(counters, C, PQ_PAIRS_ANY_HIT, cls, 1);
    }
}

// C-ABI: see include/spe_hip.h
extern "C" int spe_pseudo_quality(const float* boxes, const long* labels, const float* scores, const int* off, const float* gboxes,
                                  const long* glabels, const int* goff, const int* off_host, const int* goff_host, int B, int T, int G, int C,
                                  float iou_thresh, long* counters, hipStream_t st) {
    if (B < 0 || T < 0 || G < 0 || C < 1 || !off_host || !goff_host || !counters) return -3;
    if (off_host[0] != 0 || off_host[B] != T || goff_host[0] != 0 || goff_host[B] != G) return -3;
    for (int b = 0; b < B; ++b)
        if (off_host[b + 1] < off_host[b] || goff_host[b + 1] < goff_host[b]) return -3;
    for (int b = 0; b < B; ++b)
        if (off_host[b + 1] - off_host[b] > PQ_MAX_ROWS || goff_host[b + 1] - goff_host[b] > PQ_MAX_ROWS) return -2;
    if (B == 0 || (T == 0 && G == 0)) return 0;                                  // nothing to count
    if (!off || !goff || (T > 0 && (!boxes || !labels)) || (G > 0 && (!gboxes || !glabels))) return -3;
    hipLaunchKernelGGL(pseudo_quality_kernel, dim3(B), dim3(PQ_THREADS), 0, st, boxes, labels, scores, off, gboxes, glabels, goff, C,
                       iou_thresh, counters);
    SPE_CHECK_LAUNCH();
    return 0;
}
