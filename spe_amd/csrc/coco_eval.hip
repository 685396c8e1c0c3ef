// COCO detection metrics on the device (reference engine.evaluate -> datasets/coco_eval.py CocoEvaluator, i.e. the published COCOeval
// algorithm for iouType 'bbox', useCats = 1): what turns the per-class NMS survivors into the twelve AP / AR numbers.
//
// As with the VOC meter (voc_eval.hip), whether a detection is matched depends only on the higher-scoring detections of the SAME image
// and category, so the greedy matching runs per (image, category) as soon as a batch leaves the NMS (coco_match_kernel) and only flag
// words, ranks, scores and integer counters are kept; the end of the run is one sort (torch) and one launch (coco_accumulate_kernel).
// The IoU thresholds, area ranges, recall thresholds and maxDets are numpy's values, uploaded by the caller - nothing here recomputes
// them.  Everything is fp64 in the operation order of COCOeval; the file is compiled with -ffp-contract=off (spe_amd/build.py
// EXTRA_FLAGS), so no multiply-add of the IoU is contracted into an FMA and every threshold and tie decision is the host's, bit for
// bit.  Counters are 32-bit integer atomics; there are no floating-point atomics and nothing synchronises the host.
// The limits, the segment search, the compaction step and the workgroup primitives are det_eval_common.h's, shared with voc_eval.hip.
#include "det_eval_common.h"
#include <float.h>

#define COCO_MAXGT 512       // ground-truth boxes per image: what one wave keeps in LDS
#define COCO_T 10            // IoU thresholds: the matched / ignore bit fields of a flag word are 10 wide
#define COCO_A 4             // area ranges: one flag word each
#define COCO_MAXR 128        // recall thresholds spe_coco_accumulate takes (COCOeval has 101)

// One wave per (image, category).  The category's ground truth of the image is compacted into LDS in its incoming order.  The
// detections of the segment are visited in order; per visit the IoUs are computed ONCE, one box per lane, into LDS, and then lane
// p = a * 10 + t (40 of the 64) walks the boxes for its own (area range, threshold) pair exactly as COCOeval does: the non-ignored
// boxes first, then - only while nothing is matched - the ignored ones, `iou < best` skips, so among equal IoUs the LAST box wins.
// A walk is as long as the category has boxes in the image (typically 1 to 10), and the 40 walks run side by side: spreading the
// boxes over the lanes instead would cost 40 wave reductions per detection and would have to rebuild "last of the equal" from them.
// Which boxes a pair has matched is bit p of the box's 64-bit word in LDS (set by an LDS integer atomic; every lane owns its bit).
__global__ __launch_bounds__(64) void coco_match_kernel(const float* __restrict__ det_box, const long* __restrict__ det_cat,
                                                        const int* __restrict__ det_off, const double* __restrict__ gt_box,
                                                        const long* __restrict__ gt_cat, const unsigned char* __restrict__ gt_crowd,
                                                        const double* __restrict__ gt_area, const int* __restrict__ gt_off,
                                                        const double* __restrict__ iou_thrs, const double* __restrict__ area_rng,
                                                        int K, int top, int* __restrict__ rank, unsigned* __restrict__ words,
                                                        int* __restrict__ npig) {
    __shared__ double gb[COCO_MAXGT][4];
    __shared__ double iou[COCO_MAXGT];
    __shared__ unsigned long long gm[COCO_MAXGT];       // bit p: matched by an earlier detection at pair p
    __shared__ unsigned char gf[COCO_MAXGT];            // bit a: ignored in area range a; bit 4: crowd
    const int img = blockIdx.x / K, c = blockIdx.x - img * K, lane = threadIdx.x;
    const int d0 = det_off[img], d1 = det_off[img + 1], g0 = gt_off[img], g1 = gt_off[img + 1];
    if (d1 - d0 < 0 || d1 - d0 > EV_MAXDET || g1 - g0 < 0 || g1 - g0 > COCO_MAXGT) return;      // the entry point refuses these (-2)
    const double r00 = area_rng[0], r01 = area_rng[1], r10 = area_rng[2], r11 = area_rng[3];
    const double r20 = area_rng[4], r21 = area_rng[5], r30 = area_rng[6], r31 = area_rng[7];

    int ng = 0, n0 = 0, n1 = 0, n2 = 0, n3 = 0;                                                 // wave-uniform
    for (int base = g0; base < g1; base += 64) {
        const int j = base + lane;
        const bool m = j < g1 && gt_cat[j] == (long)c;
        unsigned f = 0;
        if (m) {
            const bool crowd = gt_crowd[j] != 0;
            const double ar = gt_area[j];
            f = (unsigned)(crowd || ar < r00 || ar > r01) | ((unsigned)(crowd || ar < r10 || ar > r11) << 1) |
                ((unsigned)(crowd || ar < r20 || ar > r21) << 2) | ((unsigned)(crowd || ar < r30 || ar > r31) << 3) |
                ((unsigned)crowd << 4);
        }
        const int p = ev_compact_slot(m, lane, ng);
        if (m) {
            gb[p][0] = gt_box[(long)j * 4]; gb[p][1] = gt_box[(long)j * 4 + 1];
            gb[p][2] = gt_box[(long)j * 4 + 2]; gb[p][3] = gt_box[(long)j * 4 + 3];
            gf[p] = (unsigned char)f; gm[p] = 0ull;
        }
        n0 += __popcll(__ballot(m && !(f & 1u))); n1 += __popcll(__ballot(m && !(f & 2u)));
        n2 += __popcll(__ballot(m && !(f & 4u))); n3 += __popcll(__ballot(m && !(f & 8u)));
    }
    if (lane < COCO_A) {
        const int n = lane == 0 ? n0 : lane == 1 ? n1 : lane == 2 ? n2 : n3;
        if (n) atomicAdd(npig + c * COCO_A + lane, n);
    }
    __syncthreads();

    int s, e;
    ev_segment(det_cat, d0, d1, (long)c, s, e);
    const int ev = min(e, s + top);
    // categories outside 0 .. K-1 belong to nobody and detections past the first `top` of a segment are never evaluated: rank -1
    if (c == 0) for (int i = d0 + lane; i < s; i += 64) { rank[i] = -1; *(uint4*)(words + (long)i * 4) = make_uint4(0u, 0u, 0u, 0u); }
    for (int i = ev + lane; i < (c == K - 1 ? d1 : e); i += 64) { rank[i] = -1; *(uint4*)(words + (long)i * 4) = make_uint4(0u, 0u, 0u, 0u); }

    const bool pair = lane < COCO_A * COCO_T;
    const int a = pair ? lane / COCO_T : 0, t = pair ? lane - a * COCO_T : 0;
    const double thr = fmin(iou_thrs[t], 1. - 1e-10);
    const double a0 = area_rng[2 * a], a1 = area_rng[2 * a + 1];
    const unsigned long long bit = 1ull << lane;

    for (int i = s; i < ev; ++i) {
        // convert_to_xywh: the widths are fp32 differences, then everything is double
        const float x0 = det_box[(long)i * 4], y0 = det_box[(long)i * 4 + 1], x1 = det_box[(long)i * 4 + 2], y1 = det_box[(long)i * 4 + 3];
        const double dx = (double)x0, dy = (double)y0, dw = (double)(x1 - x0), dh = (double)(y1 - y0);
        const double darea = dw * dh;
        for (int j = lane; j < ng; j += 64) {                                                   // bbIou, term by term
            const double gx = gb[j][0], gy = gb[j][1], gw = gb[j][2], gh = gb[j][3];
            const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
            const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
            double o = 0.;
            if (w > 0. && h > 0.) {
                const double in = w * h;
                const double un = (gf[j] & 16u) ? darea : darea + gw * gh - in;
                o = in / un;
            }
            iou[j] = o;
        }
        __syncthreads();
        int m = -1;
        if (pair) {
            double best = thr;
            for (int j = 0; j < ng; ++j) {                                                      // the non-ignored group
                const unsigned f = gf[j];
                if ((f >> a) & 1u) continue;
                if ((gm[j] & bit) && !(f & 16u)) continue;
                const double o = iou[j];
                if (o < best) continue;
                best = o; m = j;
            }
            if (m < 0)                                                                          // else: the walk stops at the ignored group
                for (int j = 0; j < ng; ++j) {
                    const unsigned f = gf[j];
                    if (!((f >> a) & 1u)) continue;
                    if ((gm[j] & bit) && !(f & 16u)) continue;
                    const double o = iou[j];
                    if (o < best) continue;
                    best = o; m = j;
                }
        }
        const bool dm = m >= 0;
        const bool dig = pair && (dm ? ((gf[m] >> a) & 1u) != 0 : (darea < a0 || darea > a1));
        if (dm) atomicOr(&gm[m], bit);
        const unsigned long long mb = __ballot(dm), ib = __ballot(dig);
        if (lane < COCO_A)
            words[(long)i * 4 + lane] = (unsigned)((mb >> (lane * COCO_T)) & 0x3ffull) | ((unsigned)((ib >> (lane * COCO_T)) & 0x3ffull) << COCO_T);
        if (lane == 0) rank[i] = i - s;
        __syncthreads();
    }
}

// C-ABI: see include/spe_hip.h (spe_coco_match).
extern "C" int spe_coco_match(const float* det_boxes, const long* det_cats, const int* det_off, const double* gt_boxes,
                              const long* gt_cats, const unsigned char* gt_iscrowd, const double* gt_area, const int* gt_off,
                              const double* iou_thrs, const double* area_rng, int nimg, int num_cats, int max_det, int max_gt,
                              int top, int* rank, unsigned* words, int* npig, hipStream_t st) {
    if (nimg <= 0) return 0;
    if (num_cats < 1 || max_det < 0 || max_gt < 0 || max_det > EV_MAXDET || max_gt > COCO_MAXGT || top < 1 ||
        (long)nimg * num_cats > 0x7fffffffL)
        return -2;
    hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)(nimg * num_cats)), dim3(64), 0, st, det_boxes, det_cats, det_off, gt_boxes,
                       gt_cats, gt_iscrowd, gt_area, gt_off, iou_thrs, area_rng, num_cats, top, rank, words, npig);
    SPE_CHECK_LAUNCH();
    return 0;
}

// ---- precision / recall tables of one (category, area range, maxDets entry) per workgroup ------------------------------------------
// Records of category k: seg_off[k] .. seg_off[k+1], in curve order (score descending, image id ascending, rank).  A record takes
// part when its rank is below the maxDets entry; COCOeval removes the others before its cumulative sums, here they stay in place and
// add to neither count (their precision enters the envelope as 0 and no look-up may land on them).  Per threshold t: a forward pass
// for the totals and the first participating record, then ONE backward pass over 256-wide chunks with carries - integer scans give
// the running tp / fp of every record (totals minus what follows), rc = tp / npig, pr = tp / ((fp + tp) + eps), the envelope is the
// running maximum from the end, and np.searchsorted(rc, recThrs, side='left') is turned round: rc only grows at a true positive, so
// the first record with rc >= thr is a true positive (or the first record of all, for the thresholds its rc already reaches) and
// that record writes the thresholds in (rc before it, its rc].  Every threshold is written by at most one record.
__global__ __launch_bounds__(EV_THREADS) void coco_accumulate_kernel(const unsigned* __restrict__ words, const int* __restrict__ rank,
                                                                      const float* __restrict__ score, const int* __restrict__ seg_off,
                                                                      const int* __restrict__ npig, const int* __restrict__ max_dets,
                                                                      const double* __restrict__ rec_thrs, int K, int R, int M,
                                                                      double* __restrict__ precision, double* __restrict__ recall,
                                                                      double* __restrict__ scores) {
    __shared__ int iws[EV_THREADS / 64];
    __shared__ double dws[EV_THREADS / 64];
    __shared__ double thr[COCO_MAXR], pbuf[COCO_MAXR], sbuf[COCO_MAXR];
    const int tid = threadIdx.x;
    const int m = blockIdx.x % M, a = (blockIdx.x / M) % COCO_A, k = blockIdx.x / (M * COCO_A);
    const long s = seg_off[k];
    const int n = (int)max((long)seg_off[k + 1] - s, 0l);
    const int np_i = npig[k * COCO_A + a], lim = max_dets[m];
    const long kam = ((long)k * COCO_A + a) * M + m;                        // [T,R,K,A,M] and [T,K,A,M]: the trailing three
    const long KAM = (long)K * COCO_A * M;
    if (np_i == 0) {                                                        // COCOeval skips the category: its init value stays
        for (int q = tid; q < COCO_T * R; q += EV_THREADS) { precision[(long)q * KAM + kam] = -1.; scores[(long)q * KAM + kam] = -1.; }
        if (tid < COCO_T) recall[(long)tid * KAM + kam] = -1.;
        return;
    }
    const double npd = (double)np_i;
    for (int r = tid; r < R; r += EV_THREADS) thr[r] = rec_thrs[r];
    const unsigned* wd = words + s * 4 + a;
    const int* rk = rank + s;
    const float* sc = score + s;

    for (int t = 0; t < COCO_T; ++t) {
        for (int r = tid; r < R; r += EV_THREADS) { pbuf[r] = 0.; sbuf[r] = 0.; }
        int ltp = 0, lfp = 0, lfirst = n;
        for (int i = tid; i < n; i += EV_THREADS) {
            if (rk[i] < lim) {
                const unsigned w = wd[(long)i * 4];
                const bool mt = (w >> t) & 1u, ig = (w >> (COCO_T + t)) & 1u;
                ltp += mt && !ig; lfp += !mt && !ig;
                lfirst = min(lfirst, i);
            }
        }
        int ctp = ev_isum(ltp, iws), cfp = ev_isum(lfp, iws);
        const int first = ev_imin(lfirst, iws);
        const int ttp = ctp;

        double env = 0.;
        for (int base = n > 0 ? (n - 1) / EV_THREADS * EV_THREADS : -1; base >= 0; base -= EV_THREADS) {
            const int i = base + tid;
            const bool valid = i < n && rk[i] < lim;
            bool istp = false, isfp = false;
            if (valid) {
                const unsigned w = wd[(long)i * 4];
                const bool mt = (w >> t) & 1u, ig = (w >> (COCO_T + t)) & 1u;
                istp = mt && !ig; isfp = !mt && !ig;
            }
            int tot;
            const int inc = ev_scan((int)istp | ((int)isfp << 16), iws, tot);
            const int tp = ctp - (tot & 0xffff) + (inc & 0xffff), fp = cfp - (tot >> 16) + (inc >> 16);
            const double p = valid ? (double)tp / (((double)fp + (double)tp) + DBL_EPSILON) : 0.;      // np.spacing(1) = 2^-52
            double cmax;
            const double en = fmax(ev_suffix_max(p, dws, cmax), env);
            if (valid && (istp || i == first)) {
                const double rc = (double)tp / npd;
                int r = 0;
                if (i != first) {                                           // first threshold above the recall before this record
                    const double rp = (double)(tp - 1) / npd;
                    int lo = 0, hi = R;
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (thr[mid] > rp) hi = mid; else lo = mid + 1; }
                    r = lo;
                }
                const double sd = (double)sc[i];
                for (; r < R && thr[r] <= rc; ++r) { pbuf[r] = en; sbuf[r] = sd; }
            }
            env = fmax(env, cmax);
            ctp -= tot & 0xffff; cfp -= tot >> 16;
        }
        __syncthreads();
        for (int r = tid; r < R; r += EV_THREADS) {
            precision[((long)t * R + r) * KAM + kam] = pbuf[r];
            scores[((long)t * R + r) * KAM + kam] = sbuf[r];
        }
        if (tid == 0) recall[(long)t * KAM + kam] = first < n ? (double)ttp / npd : 0.;
        __syncthreads();
    }
}

// C-ABI: see include/spe_hip.h (spe_coco_accumulate).
extern "C" int spe_coco_accumulate(const unsigned* words, const int* rank, const float* det_scores, const int* seg_off, const int* npig,
                                   const int* max_dets, const double* rec_thrs, int num_cats, int num_rec, int num_max_dets,
                                   double* precision, double* recall, double* scores, hipStream_t st) {
    if (num_cats <= 0) return 0;
    if (num_rec < 1 || num_rec > COCO_MAXR || num_max_dets < 1 || (long)num_cats * COCO_A * num_max_dets > 0x7fffffffL) return -2;
    hipLaunchKernelGGL(coco_accumulate_kernel, dim3((unsigned)(num_cats * COCO_A * num_max_dets)), dim3(EV_THREADS), 0, st, words,
                       rank, det_scores, seg_off, npig, max_dets, rec_thrs, num_cats, num_rec, num_max_dets, precision, recall, scores);
    SPE_CHECK_LAUNCH();
    return 0;
}
