// util.box_ops.box_iou on box_cxcywh_to_xyxy of two rows in fp32, operation for operation (corners, areas, max / min, clamp(min=0), inter,
// (area1 + area2) - inter, the division): what pseudo_quality.hip and proposal_recall.hip score their boxes with.  Both files are compiled
// without FMA contraction (spe_amd/build.py); the arithmetic is spelled with the _rn intrinsics besides: one rounding per operation.
#pragma once
#include "common.h"

// torch.max / torch.min of two numbers: a NaN on either side is the result
__device__ __forceinline__ float pq_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
__device__ __forceinline__ float pq_min(float a, float b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
// clamp(min=0): a NaN stays
__device__ __forceinline__ float pq_clamp0(float v) { return v < 0.f ? 0.f : v; }

// box_cxcywh_to_xyxy: [cx - 0.5 w, cy - 0.5 h, cx + 0.5 w, cy + 0.5 h]
__device__ __forceinline__ float4 pq_corners(const float* __restrict__ row) {
    const float cx = row[0], cy = row[1], hw = __fmul_rn(0.5f, row[2]), hh = __fmul_rn(0.5f, row[3]);
    return make_float4(__fsub_rn(cx, hw), __fsub_rn(cy, hh), __fadd_rn(cx, hw), __fadd_rn(cy, hh));
}

__device__ __forceinline__ float pq_area(float4 b) { return __fmul_rn(__fsub_rn(b.z, b.x), __fsub_rn(b.w, b.y)); }

__device__ __forceinline__ float pq_iou(float4 a, float aa, float4 b, float ab) {
    const float w = pq_clamp0(__fsub_rn(pq_min(a.z, b.z), pq_max(a.x, b.x)));
    const float h = pq_clamp0(__fsub_rn(pq_min(a.w, b.w), pq_max(a.y, b.y)));
    const float inter = __fmul_rn(w, h);
    return __fdiv_rn(inter, __fsub_rn(__fadd_rn(aa, ab), inter));
}

// the best IoU of a row as the meters sum it: llrint(min(best, 1) * 2^20) - a power of two, the product is exact; the caller has checked
// that best is finite and positive
__device__ __forceinline__ long pq_iou_quantum(float best) { return __float2ll_rn(__fmul_rn(best < 1.f ? best : 1.f, 1048576.f)); }
