// Detection head (include/spe_hip.h: spe_detect): the detections of a batch in one launch.  What PostProcess
// (reference models/conditional_detr.py:592-623: sigmoid, topk over Q * Kc, div, mod, box conversion, gather, scale) followed by the per-class
// NMS of the evaluation loops (engine_loc.py:154-174, engine.py:662-680) computes, with nothing read back on the host and nothing written
// to HBM between the steps.  One workgroup of 1024 threads per image:
//
//   select    8-bit radix select over an order-preserving uint32 image of the logit (four histogram passes in LDS find the k-th key),
//             compaction of everything above the k-th key plus the LOWEST-INDEXED elements equal to it, bitonic sort of the k
//             (key, ~index) pairs - logit descending, equal logits by flat index ascending.  Selecting on the logit is a valid topk of
//             the probabilities (sigmoid is monotone) and fixes the tie order torch.topk leaves open.
//   decode    label, query, PostProcess's fp32 box arithmetic with one rounding per operation.
//   order     stable by label: every element counts the elements that go before it (labels are not bounded by anything that fits a
//             histogram: Kc <= 2^20), so the list becomes (label ascending, score descending) - per_class_nms's order.
//   suppress  greedy, per class.  Classes do not interact, so one WAVE takes one class: lane l owns the detections l, l + 64, ... of
//             the class and keeps their dead bits in a register; the visit order is serial, the flag of the visited detection is
//             fetched from its owner's register, no barrier and no LDS write inside a class.  The IoU test is spe_nms_sorted's
//             (csrc/loss.hip nms_kernel; torchvision's arithmetic), one rounding per operation.
//
// Integer LDS atomics only; wherever their arrival order decides a slot, the slot is re-ordered afterwards by a unique key, so the
// result is a function of the input alone.  This file is compiled without FMA contraction (spe_amd/build.py), and the arithmetic that
// must match an elementwise composition is spelled with the _rn intrinsics besides.
#include "common.h"

#define DET_THREADS 1024
#define DET_WAVES (DET_THREADS / SPE_WAVE)
#define DET_MAXK 1024
#define DET_MAXN (1 << 20)

// Order-preserving image of a float: a < b <=> key(a) < key(b); -0.0 is +0.0, every NaN is the greatest key (torch.topk's order).
__device__ __forceinline__ unsigned det_key(float x) {
    unsigned u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long det_pair(unsigned key, int idx) {       // greater pair = earlier in the result
    return ((unsigned long long)key << 32) | (unsigned)~(unsigned)idx;
}

// f(index, value) for every element of a row that starts at an arbitrary 4-byte address: 16-byte loads over the aligned middle, scalar
// loads for the <= 3 elements in front of it and the <= 3 behind.  The order of the calls is not defined.
template <class F>
__device__ __forceinline__ void det_for_each(const float* __restrict__ row, int N, F f) {
    const int tid = threadIdx.x;
    int head = (int)(((16 - ((uintptr_t)row & 15)) & 15) >> 2);
    if (head > N) head = N;
    const int nv = (N - head) >> 2, tail0 = head + 4 * nv;
    const float4* v = reinterpret_cast<const float4*>(row + head);
    for (int g = tid; g < nv; g += DET_THREADS) {
        const float4 x = v[g];
        const int i = head + 4 * g;
        f(i, x.x); f(i + 1, x.y); f(i + 2, x.z); f(i + 3, x.w);
    }
    if (tid < head) f(tid, row[tid]);
    else if (tid - head < N - tail0) f(tail0 + tid - head, row[tail0 + tid - head]);
}

// ++hist[bucket] for the calling lanes.  The logits of a detector crowd into a few exponents, so in the first pass most waves agree on
// the bucket: then one lane adds the count (an LDS atomic on one address is serialised lane by lane otherwise).
__device__ __forceinline__ void det_hist_add(int* hist, unsigned bucket) {
    const unsigned long long act = __ballot(1);
    const unsigned first = __builtin_amdgcn_readfirstlane(bucket);
    if (__ballot(bucket == first) == act) {
        if ((int)(threadIdx.x & 63) == __ffsll((long long)act) - 1) atomicAdd(hist + first, (int)__popcll(act));
    } else {
        atomicAdd(hist + bucket, 1);
    }
}

__global__ __launch_bounds__(DET_THREADS) void detect_kernel(const float* __restrict__ logits, const float* __restrict__ boxes,
                                                             const float* __restrict__ sizes, int Q, int Kc, int k, float thr, int do_nms,
                                                             float* __restrict__ out_logit, long* __restrict__ out_label,
                                                             float* __restrict__ out_box, int* __restrict__ out_query,
                                                             int* __restrict__ out_count) {
    __shared__ unsigned long long s_pair[DET_MAXK];
    __shared__ float4 s_box[DET_MAXK];                   // from here on: in (label, score) order
    __shared__ float s_logit[DET_MAXK];
    __shared__ int s_label[DET_MAXK], s_query[DET_MAXK], s_keep[DET_MAXK], s_seg[DET_MAXK];
    __shared__ int s_lab0[DET_MAXK];                     // labels in score order
    __shared__ int s_hist[256], s_wave[DET_WAVES], s_sel[3], s_cnt[3];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = Q * Kc;
    const float* row = logits + (long)b * N;

    // ---- select: the k-th key, one byte per pass, most significant first ------------------------------------------------------------
    unsigned prefix = 0u, mask = 0u;
    int remaining = k, eq_total = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) s_hist[tid] = 0;
        __syncthreads();
        det_for_each(row, N, [&](int, float x) {
            const unsigned key = det_key(x);
            if ((key & mask) == prefix) det_hist_add(s_hist, (key >> shift) & 255u);
        });
        __syncthreads();
        if (tid < 256) {                                  // the bucket that holds the remaining-th greatest of the candidates
            int above = 0;
            for (int j = tid + 1; j < 256; ++j) above += s_hist[j];
            const int h = s_hist[tid];
            if (above < remaining && remaining <= above + h) { s_sel[0] = tid; s_sel[1] = above; s_sel[2] = h; }
        }
        __syncthreads();
        prefix |= (unsigned)s_sel[0] << shift;
        mask |= 255u << shift;
        remaining -= s_sel[1];
        eq_total = s_sel[2];
    }
    // prefix: the k-th key; `remaining` of the eq_total elements equal to it are taken, the lowest-indexed ones
    const unsigned kth = prefix;
    const int r = remaining, nabove = k - r;
    const bool eq_all = eq_total == r;
    int P = 1;
    while (P < k) P <<= 1;
    for (int i = tid; i < P; i += DET_THREADS) s_pair[i] = 0ull;                       // below every real pair (the least key is -inf's)
    if (tid < 3) s_cnt[tid] = 0;
    __syncthreads();
    det_for_each(row, N, [&](int i, float x) {
        const unsigned key = det_key(x);
        if (key > kth) {
            const int slot = atomicAdd(&s_cnt[0], 1);
            if (slot < nabove) s_pair[slot] = det_pair(key, i);
        } else if (eq_all && key == kth) {
            const int slot = atomicAdd(&s_cnt[1], 1);
            if (slot < r) s_pair[nabove + slot] = det_pair(key, i);
        }
    });
    if (!eq_all) {
        // more equal elements than places: every wave walks one contiguous range in index order, counts its equal elements, and after
        // a prefix over the waves files those whose rank among all equal elements is below r
        const int per = (N + DET_WAVES - 1) / DET_WAVES;
        const int w0 = min(N, wave * per), w1 = min(N, w0 + per);
        int cnt = 0;
        for (int i0 = w0; i0 < w1; i0 += 64) {
            const int i = i0 + lane;
            cnt += (int)__popcll(__ballot(i < w1 && det_key(row[i < w1 ? i : w0]) == kth));
        }
        if (lane == 0) s_wave[wave] = cnt;
        __syncthreads();
        int off = 0;
        for (int j = 0; j < wave; ++j) off += s_wave[j];
        for (int i0 = w0; i0 < w1 && off < r; i0 += 64) {
            const int i = i0 + lane;
            const bool eq = i < w1 && det_key(row[i < w1 ? i : w0]) == kth;
            const unsigned long long m = __ballot(eq);
            const int rank = off + (int)__popcll(m & ((1ull << lane) - 1ull));
            if (eq && rank < r) s_pair[nabove + rank] = det_pair(kth, i);
            off += (int)__popcll(m);
        }
    }
    // bitonic sort of the P pairs, descending
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            if (tid < (P >> 1)) {
                const int pos = 2 * tid - (tid & (stride - 1)), q = pos + stride;
                const unsigned long long a = s_pair[pos], c = s_pair[q];
                const bool desc = (pos & size) == 0;
                if ((a < c) == desc) { s_pair[pos] = c; s_pair[q] = a; }
            }
        }
    }
    __syncthreads();

    // ---- decode: thread i owns the i-th best ----------------------------------------------------------------------------------------
    int label = 0, query = 0;
    float logit = 0.f;
    float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < k) {
        unsigned idx = ~(unsigned)s_pair[tid];
        if (idx >= (unsigned)N) idx = (unsigned)N - 1u;                               // cannot happen; keeps every address inside the row
        label = (int)(idx % (unsigned)Kc);
        query = (int)(idx / (unsigned)Kc);
        logit = row[idx];
        const float* bp = boxes + ((long)b * Q + query) * 4;
        const float cx = bp[0], cy = bp[1], w = bp[2], h = bp[3];
        const float img_h = sizes[2 * b], img_w = sizes[2 * b + 1];
        const float hw = __fmul_rn(0.5f, w), hh = __fmul_rn(0.5f, h);
        float x0 = __fsub_rn(cx, hw), y0 = __fsub_rn(cy, hh), x1 = __fadd_rn(cx, hw), y1 = __fadd_rn(cy, hh);
        x0 = x0 < 0.f ? 0.f : x0; y0 = y0 < 0.f ? 0.f : y0; x1 = x1 < 0.f ? 0.f : x1; y1 = y1 < 0.f ? 0.f : y1;     // clamp(min=0): NaN stays
        box = make_float4(__fmul_rn(x0, img_w), __fmul_rn(y0, img_h), __fmul_rn(x1, img_w), __fmul_rn(y1, img_h));
        s_lab0[tid] = label;
    }
    __syncthreads();

    // ---- order: stable by label -----------------------------------------------------------------------------------------------------
    if (tid < k) {
        int rank = 0;
        for (int j = 0; j < k; ++j) {
            const int lj = s_lab0[j];
            rank += (lj < label || (lj == label && j < tid)) ? 1 : 0;
        }
        s_box[rank] = box; s_logit[rank] = logit; s_label[rank] = label; s_query[rank] = query; s_keep[rank] = 1;
    }
    __syncthreads();

    // ---- suppress: one wave per class ---------------------------------------------------------------------------------------------------
    if (do_nms) {
        if (tid < k && (tid == 0 || s_label[tid - 1] != s_label[tid])) s_seg[atomicAdd(&s_cnt[2], 1)] = tid;
        __syncthreads();
        const int nseg = s_cnt[2];
        for (int sg = wave; sg < nseg; sg += DET_WAVES) {
            const int s = s_seg[sg], li = s_label[s];
            int L = 0;
            for (int t = 0; t < DET_MAXK / 64; ++t) {
                const int p = s + lane + 64 * t;
                const int c = (int)__popcll(__ballot(p < k && s_label[p < k ? p : s] == li));
                L += c;
                if (c < 64) break;
            }
            unsigned dead = 0u;                            // bit t: detection lane + 64 t of the class is suppressed
            for (int i = 0; i < L; ++i) {
                const unsigned dm = (unsigned)__shfl((int)dead, i & 63, 64);
                if ((dm >> (i >> 6)) & 1u) continue;
                const float4 bi = s_box[s + i];
                const float ai = __fmul_rn(__fsub_rn(bi.z, bi.x), __fsub_rn(bi.w, bi.y));
                for (int t = i >> 6; t * 64 < L; ++t) {
                    const int j = lane + 64 * t;
                    if (j > i && j < L) {
                        const float4 bj = s_box[s + j];
                        const float w = fmaxf(__fsub_rn(fminf(bi.z, bj.z), fmaxf(bi.x, bj.x)), 0.f);
                        const float h = fmaxf(__fsub_rn(fminf(bi.w, bj.w), fmaxf(bi.y, bj.y)), 0.f);
                        const float inter = __fmul_rn(w, h), aj = __fmul_rn(__fsub_rn(bj.z, bj.x), __fsub_rn(bj.w, bj.y));
                        if (__fdiv_rn(inter, __fsub_rn(__fadd_rn(ai, aj), inter)) > thr) dead |= 1u << t;
                    }
                }
            }
            for (int t = 0; t * 64 < L; ++t)
                if (lane + 64 * t < L) s_keep[s + lane + 64 * t] = ((dead >> t) & 1u) ? 0 : 1;
        }
        __syncthreads();
    }

    // ---- compact: survivors to the front, the fill behind them ----------------------------------------------------------------------
    const bool kp = tid < k && s_keep[tid] != 0;
    const unsigned long long km = __ballot(kp);
    if (lane == 0) s_wave[wave] = (int)__popcll(km);
    __syncthreads();
    int base = 0, count = 0;
    for (int j = 0; j < DET_WAVES; ++j) { const int c = s_wave[j]; base += j < wave ? c : 0; count += c; }
    const long o = (long)b * k;
    if (kp) {
        const long d = o + base + (int)__popcll(km & ((1ull << lane) - 1ull));
        const float4 bx = s_box[tid];
        out_logit[d] = s_logit[tid]; out_label[d] = (long)s_label[tid]; out_query[d] = s_query[tid];
        out_box[d * 4] = bx.x; out_box[d * 4 + 1] = bx.y; out_box[d * 4 + 2] = bx.z; out_box[d * 4 + 3] = bx.w;
    }
    if (tid >= count && tid < k) {
        const long d = o + tid;
        out_logit[d] = -INFINITY; out_label[d] = -1; out_query[d] = -1;
        out_box[d * 4] = 0.f; out_box[d * 4 + 1] = 0.f; out_box[d * 4 + 2] = 0.f; out_box[d * 4 + 3] = 0.f;
    }
    if (tid == 0) out_count[b] = count;
}

// C-ABI: see include/spe_hip.h
extern "C" int spe_detect(const float* logits, const float* boxes, const float* sizes, int B, int Q, int Kc, int k, float iou_threshold,
                          int do_nms, float* out_logit, long* out_label, float* out_box, int* out_query, int* out_count, hipStream_t st) {
    if (B <= 0) return 0;
    const long N = (long)Q * (long)Kc;
    if (Q < 0 || Kc < 0 || k < 1 || k > N) return -3;
    if (k > DET_MAXK || N > DET_MAXN) return -2;
    hipLaunchKernelGGL(detect_kernel, dim3(B), dim3(DET_THREADS), 0, st, logits, boxes, sizes, Q, Kc, k, iou_threshold, do_nms, out_logit,
                       out_label, out_box, out_query, out_count);
    SPE_CHECK_LAUNCH();
    return 0;
}
