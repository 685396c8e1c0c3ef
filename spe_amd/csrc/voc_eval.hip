// PASCAL VOC detection metrics on the device (reference engine_loc.py:176-197, datasets/voc_eval.py, datasets/dis_eval.py;
// DESIGN.md section 8g): what turns the per-class NMS survivors into AP / mAP and CorLoc.
//
// The reference walks one global, score-sorted list per class.  Whether a detection is a true or a false positive depends only on
// the detections of the SAME image and class that come before it, so the greedy matching is done per (image, class) segment as soon
// as a batch leaves the NMS (voc_match_kernel), and the end of the run is one sort (torch), two scans and a short sum per class
// (voc_ap_kernel).  Everything here is fp64 in numpy's operation order.  This file is compiled with -ffp-contract=off
// (spe_amd/build.py EXTRA_FLAGS): no multiply-add of the overlap is contracted into an FMA, so with equal inputs the overlaps - and
// with them every threshold and tie decision - are bit-identical to numpy's.  Counters are 32-bit integer atomics (order-free, bitwise
// reproducible); there are no floating-point atomics and nothing synchronises the host.
// The limits, the segment search, the compaction step and the workgroup primitives are det_eval_common.h's, shared with coco_eval.hip.
#include "det_eval_common.h"
#include <float.h>

#define VOC_MAXGT 1024       // ground-truth boxes per image: what one workgroup keeps in LDS

// The decimal round trip of the reference's result files (voc_voc.py:383-386): '{:.3f}' of the score, '{:.1f}' of the fp32
// coordinate + 1.  double(fp32) * 1000 (* 10) is exact in fp64 and rint is half-even, so rint(.) / scale is the correctly rounded
// decimal Python prints, parsed back.  scale 0: no quantisation.
__device__ __forceinline__ double voc_score(float s, double scale) {
    const double d = (double)s;
    return scale != 0.0 ? rint(d * scale) / scale : d;
}
__device__ __forceinline__ double voc_coord(float x, double scale) {
    return scale != 0.0 ? rint((double)(x + 1.0f) * scale) / scale : (double)x + 1.0;
}

// One wave per (image, class).  The class's ground truth of the image is compacted into LDS in its incoming order (so "lowest index"
// below is numpy's argmax), the detections of the segment are visited in order, each visit is one lane-strided pass over the ground
// truth and one wave arg-max.
__global__ __launch_bounds__(64) void voc_match_kernel(const float* __restrict__ det_box, const float* __restrict__ det_score,
                                                       const long* __restrict__ det_label, const int* __restrict__ det_off,
                                                       const double* __restrict__ gt_box, const long* __restrict__ gt_label,
                                                       const unsigned char* __restrict__ gt_diff, const int* __restrict__ gt_off,
                                                       int C, double ovthresh, double sscale, double cscale,
                                                       unsigned char* __restrict__ flag, double* __restrict__ score_out,
                                                       int* __restrict__ npos, int* __restrict__ nimgs, int* __restrict__ hits) {
    __shared__ double gb[VOC_MAXGT][4];
    __shared__ unsigned char gd[VOC_MAXGT], used[VOC_MAXGT];
    const int img = blockIdx.x / C, c = blockIdx.x - img * C, lane = threadIdx.x;
    const int d0 = det_off[img], d1 = det_off[img + 1], g0 = gt_off[img], g1 = gt_off[img + 1];
    if (d1 - d0 < 0 || d1 - d0 > EV_MAXDET || g1 - g0 < 0 || g1 - g0 > VOC_MAXGT) return;       // the entry point refuses these (-2)
    const long want = (long)c + 1;

    int ng = 0, nnd = 0;                                                                        // wave-uniform
    for (int base = g0; base < g1; base += 64) {
        const int j = base + lane;
        const bool m = j < g1 && gt_label[j] == want;
        const bool df = m && gt_diff[j] != 0;
        const int p = ev_compact_slot(m, lane, ng);
        if (m) {
            gb[p][0] = gt_box[(long)j * 4]; gb[p][1] = gt_box[(long)j * 4 + 1];
            gb[p][2] = gt_box[(long)j * 4 + 2]; gb[p][3] = gt_box[(long)j * 4 + 3];
            gd[p] = df; used[p] = 0;
        }
        nnd += __popcll(__ballot(m && !df));
    }
    if (lane == 0) {
        if (nnd) atomicAdd(npos + c, nnd);
        if (ng) atomicAdd(nimgs + c, 1);
    }
    __syncthreads();

    int s, e;
    ev_segment(det_label, d0, d1, want, s, e);
    // labels outside 1 .. C belong to no class (engine_loc.py:184): flag 0, written by the first / last wave of the image
    if (c == 0) for (int i = d0 + lane; i < s; i += 64) { flag[i] = 0; score_out[i] = voc_score(det_score[i], sscale); }
    if (c == C - 1) for (int i = e + lane; i < d1; i += 64) { flag[i] = 0; score_out[i] = voc_score(det_score[i], sscale); }

    for (int i = s; i < e; ++i) {
        const double b0 = voc_coord(det_box[(long)i * 4], cscale), b1 = voc_coord(det_box[(long)i * 4 + 1], cscale);
        const double b2 = voc_coord(det_box[(long)i * 4 + 2], cscale), b3 = voc_coord(det_box[(long)i * 4 + 3], cscale);
        const double area = (b2 - b0 + 1.) * (b3 - b1 + 1.);
        double best = -INFINITY;
        int idx = 0x7fffffff;
        bool isnan_ = false;
        for (int j = lane; j < ng; j += 64) {                                                  // voc_eval.py:169-182, term by term
            const double ixmin = fmax(gb[j][0], b0), iymin = fmax(gb[j][1], b1);
            const double ixmax = fmin(gb[j][2], b2), iymax = fmin(gb[j][3], b3);
            const double iw = fmax(ixmax - ixmin + 1., 0.), ih = fmax(iymax - iymin + 1., 0.);
            const double inters = iw * ih;
            const double uni = area + (gb[j][2] - gb[j][0] + 1.) * (gb[j][3] - gb[j][1] + 1.) - inters;
            const double ov = inters / uni;
            if (ov != ov) isnan_ = true;
            else if (ov > best) { best = ov; idx = j; }                                        // strict: the first maximum of this lane
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {                                                     // wave arg-max, lowest index on equal values
            const double ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(idx, o, 64);
            if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
        }
        // np.max propagates a NaN overlap (0/0 of degenerate boxes) and NaN > ovthresh is False: a false positive
        const bool over = !__any(isnan_) && best > ovthresh;
        unsigned char f = 2;
        if (over && gd[idx]) f = 0;                                                            // difficult: neither, nothing marked
        else if (over && !used[idx]) { f = 1; used[idx] = 1; }                                 // every lane stores the same byte it reads back
        if (lane == 0) {
            flag[i] = f;
            score_out[i] = voc_score(det_score[i], sscale);
            if (i == s && over) atomicAdd(hits + c, 1);                                        // CorLoc: the top survivor against ANY box of the class
        }
    }
}

// C-ABI: see include/spe_hip.h (spe_voc_match).
extern "C" int spe_voc_match(const float* det_boxes, const float* det_scores, const long* det_labels, const int* det_off,
                             const double* gt_boxes, const long* gt_labels, const unsigned char* gt_difficult, const int* gt_off,
                             int nimg, int num_classes, int max_det, int max_gt, double ovthresh, double score_scale,
                             double coord_scale, unsigned char* flags, double* scores_out, int* npos, int* nimgs, int* hits,
                             hipStream_t st) {
    if (nimg <= 0) return 0;
    if (num_classes < 1 || max_det < 0 || max_gt < 0 || max_det > EV_MAXDET || max_gt > VOC_MAXGT ||
        (long)nimg * num_classes > 0x7fffffffL)
        return -2;
    hipLaunchKernelGGL(voc_match_kernel, dim3((unsigned)(nimg * num_classes)), dim3(64), 0, st, det_boxes, det_scores, det_labels,
                       det_off, gt_boxes, gt_labels, gt_difficult, gt_off, num_classes, ovthresh, score_scale, coord_scale, flags,
                       scores_out, npos, nimgs, hits);
    SPE_CHECK_LAUNCH();
    return 0;
}

// ---- precision / recall curve and both APs of one class per workgroup ---------------------------------------------------------
__global__ __launch_bounds__(EV_THREADS) void voc_ap_kernel(const unsigned char* __restrict__ flag, const int* __restrict__ seg_off,
                                                            const int* __restrict__ npos, double* __restrict__ ap07,
                                                            double* __restrict__ ap_area, double* __restrict__ rec,
                                                            double* __restrict__ prec) {
    __shared__ int iws[EV_THREADS / 64];
    __shared__ double dws[EV_THREADS / 64];
    const int c = blockIdx.x, tid = threadIdx.x;
    const long s = seg_off[c];
    const long n = max((long)seg_off[c + 1] - s, 0l);
    const double np_ = (double)npos[c];                                     // rec = tp / float(npos): NaN / inf when npos = 0, as numpy gives
    const unsigned char* fl = flag + s;

    // forward: running counts, rec / prec, the 11 maxima of AP07 (prec >= 0, so "0 when rec >= t is empty" is the start value)
    int ctp = 0, cfp = 0;
    double pm[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) pm[k] = 0.;
    for (long base = 0; base < n; base += EV_THREADS) {
        const long i = base + tid;
        const int f = i < n ? fl[i] : 0;
        int tot;
        const int inc = ev_scan((f == 1) | ((f == 2) << 16), iws, tot);
        if (i < n) {
            const int tp = ctp + (inc & 0xffff), fp = cfp + (inc >> 16);
            const double r = (double)tp / np_, p = (double)tp / fmax((double)tp + (double)fp, DBL_EPSILON);
            if (rec) rec[s + i] = r;
            if (prec) prec[s + i] = p;
#pragma unroll
            for (int k = 0; k < 11; ++k) if (r >= (double)k * 0.1) pm[k] = fmax(pm[k], p);      // np.arange(0., 1.1, 0.1)[k] = k * 0.1
        }
        ctp += tot & 0xffff; cfp += tot >> 16;
    }
    double ap = 0.;
    for (int k = 0; k < 11; ++k) {                                          // a maximum does not depend on the order it is taken in
        double t;
        ev_suffix_max(pm[k], dws, t);
        ap = ap + t / 11.;
    }
    if (tid == 0) ap07[c] = ap;

    // backward: precision envelope (reverse running maximum) and sum (mrec[i+1] - mrec[i]) * mpre[i+1] where mrec changes, the
    // sentinels mrec = [0, rec, 1], mpre = [0, prec, 0] of voc_eval.py:44-56 included.  Counts at i: totals minus what follows i.
    const double last = n > 0 ? (double)ctp / np_ : 0.;
    double area = 0.;
    if (1. != last) area = (1. - last) * 0.;                                // the sentinel term: 0, or the NaN numpy gets from rec = NaN / inf
    double env = 0.;
    for (long base = n > 0 ? (n - 1) / EV_THREADS * EV_THREADS : -1; base >= 0; base -= EV_THREADS) {
        const long i = base + tid;
        const int f = i < n ? fl[i] : 0;
        int tot;
        const int inc = ev_scan((f == 1) | ((f == 2) << 16), iws, tot);
        const int tp = ctp - (tot & 0xffff) + (inc & 0xffff), fp = cfp - (tot >> 16) + (inc >> 16);
        const double p = i < n ? (double)tp / fmax((double)tp + (double)fp, DBL_EPSILON) : 0.;
        double cmax;
        const double m = fmax(ev_suffix_max(p, dws, cmax), env);
        double term = 0.;
        if (i < n) {
            const double r = (double)tp / np_, rp = i > 0 ? (double)(tp - (f == 1)) / np_ : 0.;
            if (r != rp) term = (r - rp) * m;
        }
        area += ev_sum(term, dws);
        env = fmax(env, cmax);
        ctp -= tot & 0xffff; cfp -= tot >> 16;
    }
    if (tid == 0) ap_area[c] = area;
}

// C-ABI: see include/spe_hip.h (spe_voc_ap).
extern "C" int spe_voc_ap(const unsigned char* flags, const int* seg_off, const int* npos, int num_classes, double* ap07,
                          double* ap_area, double* rec, double* prec, hipStream_t st) {
    if (num_classes <= 0) return 0;
    hipLaunchKernelGGL(voc_ap_kernel, dim3((unsigned)num_classes), dim3(EV_THREADS), 0, st, flags, seg_off, npos, ap07, ap_area,
                       rec, prec);
    SPE_CHECK_LAUNCH();
    return 0;
}
