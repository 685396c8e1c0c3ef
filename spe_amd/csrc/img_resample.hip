// Device-side input transforms (reference datasets/transforms.py + util/misc.collate_fn): Pillow's bilinear
// Image.resize restated bit for bit, with the crop box and the horizontal flip folded into the source index map, and ToTensor +
// Normalize + the batch padding as the epilogue of the last pass.
//
// Pillow resamples separably: per axis a table (first tap, tap count, coefficients) computed in fp64 and rounded to 22-bit fixed
// point, a horizontal pass that writes uint8, a vertical pass that reads that uint8.  The intermediate rounding is part of the
// result.  rs_tables_kernel restates the fp64 arithmetic in Pillow's operation order; this file is compiled with -ffp-contract=off
// (spe_amd/build.py EXTRA_FLAGS) so that no multiply-add of it is contracted into an FMA.  Everything after the tables is 32-bit
// integer arithmetic.  An axis whose length does not change gets taps (1 << 22, 0): the same bytes as Pillow's copy.
//
// Every launch serves the whole batch through a descriptor table, RS_DESC longs per image (include/spe_hip.h).
#include "common.h"

#define RS_DESC 16
#define RS_MAX_TAPS 65          // ksize = 2 * ceil(max(inS / outS, 1)) + 1: a 32x downscale (a 4x one needs 9)
#define RS_MAX_SIDE 32768       // any source, box or output side
#define RS_BITS 22

enum { D_SRC, D_SRCW, D_SRCH, D_X0, D_Y0, D_CW, D_CH, D_FLIP, D_OW, D_OH, D_DST, D_TMP, D_TABX, D_TABY, D_KX, D_KY };

static inline int rs_ksize(long inS, long outS) {
    const double scale = (double)inS / (double)outS;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs;
    return (int)ceil(support) * 2 + 1;
}
static inline long rs_pitch(long ow) { return (ow + 3) & ~3l; }

// 0, or the status of the first bad descriptor: -2 empty / oversized box or output, -3 crop outside the source, -5 more taps than RS_MAX_TAPS
static int rs_validate(const long* d, int n) {
    for (int i = 0; i < n; ++i, d += RS_DESC) {
        if (d[D_CW] < 1 || d[D_CH] < 1 || d[D_OW] < 1 || d[D_OH] < 1 || d[D_SRCW] < 1 || d[D_SRCH] < 1 || d[D_SRC] == 0 ||
            d[D_SRCW] > RS_MAX_SIDE || d[D_SRCH] > RS_MAX_SIDE || d[D_OW] > RS_MAX_SIDE || d[D_OH] > RS_MAX_SIDE)
            return -2;
        if (d[D_X0] < 0 || d[D_Y0] < 0 || d[D_X0] + d[D_CW] > d[D_SRCW] || d[D_Y0] + d[D_CH] > d[D_SRCH]) return -3;
        if (rs_ksize(d[D_CW], d[D_OW]) > RS_MAX_TAPS || rs_ksize(d[D_CH], d[D_OH]) > RS_MAX_TAPS) return -5;
    }
    return 0;
}
// the planned fields must be what spe_resample_plan wrote (a launch never trusts offsets it cannot bound)
static int rs_planned(const long* d, int n, long* tmp_bytes, long* table_ints, long* mow, long* moh, long* mch) {
    long tmp = 0, tab = 0;
    *mow = *moh = *mch = 0;
    for (int i = 0; i < n; ++i, d += RS_DESC) {
        const int kx = rs_ksize(d[D_CW], d[D_OW]), ky = rs_ksize(d[D_CH], d[D_OH]);
        if (d[D_TMP] != tmp || d[D_TABX] != tab || d[D_KX] != kx || d[D_TABY] != tab + d[D_OW] * (2 + kx) || d[D_KY] != ky) return -2;
        tmp += 3 * d[D_CH] * rs_pitch(d[D_OW]);
        tab += d[D_OW] * (2 + kx) + d[D_OH] * (2 + ky);
        if (d[D_OW] > *mow) *mow = d[D_OW];
        if (d[D_OH] > *moh) *moh = d[D_OH];
        if (d[D_CH] > *mch) *mch = d[D_CH];
    }
    *tmp_bytes = tmp + 16;       // the vertical pass reads 4 bytes at any x below the row pitch
    *table_ints = tab;
    return 0;
}

// C-ABI: see include/spe_hip.h (spe_resample_plan).  Host only.
extern "C" int spe_resample_plan(long* desc, int n, long* totals) {
    if (n <= 0) return -2;
    const int rc = rs_validate(desc, n);
    if (rc) return rc;
    long tmp = 0, tab = 0;
    long* d = desc;
    for (int i = 0; i < n; ++i, d += RS_DESC) {
        const int kx = rs_ksize(d[D_CW], d[D_OW]), ky = rs_ksize(d[D_CH], d[D_OH]);
        d[D_TMP] = tmp; d[D_TABX] = tab; d[D_KX] = kx; d[D_TABY] = tab + d[D_OW] * (2 + kx); d[D_KY] = ky;
        tmp += 3 * d[D_CH] * rs_pitch(d[D_OW]);
        tab += d[D_OW] * (2 + kx) + d[D_OH] * (2 + ky);
    }
    return rs_planned(desc, n, totals, totals + 1, totals + 2, totals + 3, totals + 4);
}

// ---- tables: one thread per (image, axis, output index) -------------------------------------------------------------------------
// Layout of one axis: xmin[outS], n[outS], k[outS][ksize].  The weights are evaluated twice (once for their sum, once to divide)
// instead of being kept: the same operations on the same operands give the same values, and no per-thread array is needed.
__device__ __forceinline__ double rs_weight(int x, int xmin, double center, double ss) {
    double t = ((double)(x + xmin) - center + 0.5) * ss;
    if (t < 0.0) t = -t;
    return t < 1.0 ? 1.0 - t : 0.0;
}
__global__ __launch_bounds__(256) void rs_tables_kernel(const long* __restrict__ desc, int* __restrict__ tables) {
    const long* d = desc + (long)blockIdx.z * RS_DESC;
    const int axis = blockIdx.y;
    const int inS = (int)d[axis ? D_CH : D_CW], outS = (int)d[axis ? D_OH : D_OW], ksize = (int)d[axis ? D_KY : D_KX];
    const int xx = blockIdx.x * 256 + threadIdx.x;
    if (xx >= outS) return;
    int* tab = tables + d[axis ? D_TABY : D_TABX];
    const double scale = (double)inS / (double)outS;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs;
    const double center = ((double)xx + 0.5) * scale;
    const double ss = 1.0 / fs;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > inS) xmax = inS;
    int n = xmax - xmin;
    n = n < 0 ? 0 : (n > ksize ? ksize : n);            // never taken (support >= 1): keeps every later read inside the tables
    double ww = 0.0;
    for (int x = 0; x < n; ++x) ww += rs_weight(x, xmin, center, ss);
    tab[xx] = xmin;
    tab[outS + xx] = n;
    int* k = tab + 2 * (long)outS + (long)xx * ksize;
    for (int x = 0; x < ksize; ++x) {
        int v = 0;
        if (x < n) {
            double w = rs_weight(x, xmin, center, ss);
            if (ww != 0.0) w /= ww;
            v = (int)(0.5 + w * (double)(1 << RS_BITS));
        }
        k[x] = v;
    }
}

__device__ __forceinline__ unsigned rs_clip8(int acc) {
    const int v = acc >> RS_BITS;
    return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ---- horizontal pass: uint8 HWC view (crop box, flip) -> planar uint8 [3][ch][pitch], pitch = ow rounded up to 4 -------------------
// One lane: four consecutive outputs of one row, all three channels, three 4-byte stores (the pad bytes of a row are written as 0).
__global__ __launch_bounds__(256) void rs_h_kernel(const long* __restrict__ desc, const int* __restrict__ tables,
                                                   unsigned char* __restrict__ tmp) {
    const long* d = desc + (long)blockIdx.z * RS_DESC;
    const int ow = (int)d[D_OW], ch = (int)d[D_CH], pitch = (ow + 3) & ~3;
    const int x4 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x4 >= pitch || y >= ch) return;
    const int kx = (int)d[D_KX], cw = (int)d[D_CW], x0 = (int)d[D_X0];
    const bool flip = d[D_FLIP] != 0;
    const int* tab = tables + d[D_TABX];
    const int* kt = tab + 2 * (long)ow;
    const unsigned char* row = (const unsigned char*)d[D_SRC] + (d[D_Y0] + y) * d[D_SRCW] * 3;
    unsigned o0 = 0, o1 = 0, o2 = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int x = x4 + i;
        if (x >= ow) break;
        const int xmin = tab[x], n = tab[ow + x];
        const int* k = kt + (long)x * kx;
        int a0 = 1 << (RS_BITS - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < n; ++t) {
            const int sx = flip ? x0 + cw - 1 - (xmin + t) : x0 + xmin + t;
            const unsigned char* p = row + sx * 3;
            const int kk = k[t];
            a0 += (int)p[0] * kk; a1 += (int)p[1] * kk; a2 += (int)p[2] * kk;
        }
        o0 |= rs_clip8(a0) << (8 * i); o1 |= rs_clip8(a1) << (8 * i); o2 |= rs_clip8(a2) << (8 * i);
    }
    unsigned char* t0 = tmp + d[D_TMP] + (long)y * pitch + x4;
    const long plane = (long)ch * pitch;
    *reinterpret_cast<unsigned*>(t0) = o0;
    *reinterpret_cast<unsigned*>(t0 + plane) = o1;
    *reinterpret_cast<unsigned*>(t0 + 2 * plane) = o2;
}

// ---- vertical pass ------------------------------------------------------------------------------------------------------------
// four consecutive x (from byte x, any alignment) of output row y of one plane: the 22-bit sums before the shift
__device__ __forceinline__ void rs_vsum4(const unsigned char* __restrict__ plane, int pitch, int x, int ymin, int n,
                                         const int* __restrict__ k, int (&acc)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = 1 << (RS_BITS - 1);
    const unsigned char* p = plane + (long)ymin * pitch + x;
    for (int t = 0; t < n; ++t, p += pitch) {
        unsigned w;
        __builtin_memcpy(&w, p, 4);
        const int kk = k[t];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += (int)((w >> (8 * i)) & 255u) * kk;
    }
}

// epilogue (a): a uint8 HWC image that feeds another resize.  One lane: four x of one row, three channels.
__global__ __launch_bounds__(256) void rs_v_u8_kernel(const long* __restrict__ desc, const int* __restrict__ tables,
                                                      const unsigned char* __restrict__ tmp) {
    const long* d = desc + (long)blockIdx.z * RS_DESC;
    const int ow = (int)d[D_OW], oh = (int)d[D_OH], ch = (int)d[D_CH], pitch = (ow + 3) & ~3;
    const int x4 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x4 >= ow || y >= oh) return;
    const int* tab = tables + d[D_TABY];
    const int ymin = tab[y], n = tab[oh + y];
    const int* k = tab + 2 * (long)oh + (long)y * (int)d[D_KY];
    const unsigned char* base = tmp + d[D_TMP];
    unsigned char* dst = (unsigned char*)d[D_DST] + ((long)y * ow + x4) * 3;
    const int cnt = ow - x4 < 4 ? ow - x4 : 4;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int acc[4];
        rs_vsum4(base + (long)c * ch * pitch, pitch, x4, ymin, n, k, acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) if (i < cnt) dst[i * 3 + c] = (unsigned char)rs_clip8(acc[i]);
    }
}

// epilogue (b): byte -> fp32 through the 3 x 256 table, planar into the padded batch, the padding mask with it.  The kernel owns
// every element of out[b] and mask[b].  One workgroup: 256 lanes of one (image, channel) plane; one lane: four consecutive x of one
// row and one 16-byte store.  A row of the batch starts at any float address, so lane 0 of a row takes the 0 .. 3 elements in front
// of the first 16-byte aligned address with scalar stores, lane j >= 1 the j-th aligned group, and a group cut off by the end of
// the row is stored element by element.
__global__ __launch_bounds__(256) void rs_v_norm_kernel(const long* __restrict__ desc, const int* __restrict__ tables,
                                                        const unsigned char* __restrict__ tmp, const float* __restrict__ lut,
                                                        float* __restrict__ out, unsigned char* __restrict__ mask, int Hmax,
                                                        int Wmax, int lpr) {
    __shared__ float slut[256];
    const int b = blockIdx.y / 3, c = blockIdx.y - b * 3;
    slut[threadIdx.x] = lut[c * 256 + threadIdx.x];                          // the channel's row of the table
    __syncthreads();
    const long* d = desc + (long)b * RS_DESC;
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;                    // < RS_MAX_SIDE * (RS_MAX_SIDE / 4 + 2) < 2^31
    const int y = (int)(idx / (unsigned)lpr), j = (int)(idx - (unsigned)y * (unsigned)lpr);
    if (y >= Hmax) return;
    const int r = c * Hmax + y;
    const int ow = (int)d[D_OW], oh = (int)d[D_OH], ch = (int)d[D_CH], pitch = (ow + 3) & ~3;
    const long rowoff = ((long)b * 3 * Hmax + r) * Wmax;                     // float index of out[b, c, y, 0]
    int head = (int)(((16 - ((uintptr_t)(out + rowoff) & 15)) & 15) >> 2);  // floats up to the first 16-byte aligned address
    if (head > Wmax) head = Wmax;
    const int xs = j == 0 ? 0 : head + 4 * (j - 1);
    const int cnt = j == 0 ? head : (Wmax - xs < 4 ? Wmax - xs : 4);
    if (cnt <= 0) return;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (y < oh && xs < ow) {
        const int* tab = tables + d[D_TABY];
        int acc[4];
        rs_vsum4(tmp + d[D_TMP] + (long)c * ch * pitch, pitch, xs, tab[y], tab[oh + y],
                 tab + 2 * (long)oh + (long)y * (int)d[D_KY], acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) if (xs + i < ow) v[i] = slut[rs_clip8(acc[i])];
    }
    float* o = out + rowoff + xs;
    if (j > 0 && cnt == 4) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    else
        for (int i = 0; i < cnt; ++i) o[i] = v[i];
    if (c == 0) {                                                             // True on padding
        unsigned char* m = mask + ((long)b * Hmax + y) * Wmax + xs;
        unsigned bits = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) bits |= (unsigned)(y >= oh || xs + i >= ow) << (8 * i);
        if (cnt == 4 && (((uintptr_t)m) & 3) == 0) *reinterpret_cast<unsigned*>(m) = bits;
        else
            for (int i = 0; i < cnt; ++i) m[i] = (unsigned char)((bits >> (8 * i)) & 1u);
    }
}

// C-ABI: see include/spe_hip.h.  Each launcher validates the HOST copy of the descriptors (it also sizes the grid from it) and
// launches nothing when a descriptor is bad.
static int rs_check(const long* desc_host, int n, long* mow, long* moh, long* mch) {
    long tmp_bytes, table_ints;
    if (n <= 0 || n > 65535) return -2;                                       // one grid dimension counts the images
    const int rc = rs_validate(desc_host, n);
    return rc ? rc : rs_planned(desc_host, n, &tmp_bytes, &table_ints, mow, moh, mch);
}
extern "C" int spe_resample_tables(const long* desc_host, const long* desc_dev, int n, int* tables, hipStream_t st) {
    long mow, moh, mch;
    const int rc = rs_check(desc_host, n, &mow, &moh, &mch);
    if (rc) return rc;
    const long mo = mow > moh ? mow : moh;
    hipLaunchKernelGGL(rs_tables_kernel, dim3((unsigned)((mo + 255) / 256), 2, (unsigned)n), dim3(256), 0, st, desc_dev, tables);
    SPE_CHECK_LAUNCH();
    return 0;
}

extern "C" int spe_resample_h(const long* desc_host, const long* desc_dev, int n, const int* tables, unsigned char* tmp,
                              hipStream_t st) {
    long mow, moh, mch;
    const int rc = rs_check(desc_host, n, &mow, &moh, &mch);
    if (rc) return rc;
    hipLaunchKernelGGL(rs_h_kernel, dim3((unsigned)((rs_pitch(mow) / 4 + 63) / 64), (unsigned)((mch + 3) / 4), (unsigned)n), dim3(256),
                       0, st, desc_dev, tables, tmp);
    SPE_CHECK_LAUNCH();
    return 0;
}

extern "C" int spe_resample_v(const long* desc_host, const long* desc_dev, int n, const int* tables, const unsigned char* tmp,
                              const float* lut, float* out, unsigned char* mask, int Hmax, int Wmax, hipStream_t st) {
    long mow, moh, mch;
    const int rc = rs_check(desc_host, n, &mow, &moh, &mch);
    if (rc) return rc;
    if (!out) {                                                               // epilogue (a): every image to its own D_DST
        for (int i = 0; i < n; ++i) if (desc_host[(long)i * RS_DESC + D_DST] == 0) return -2;
        hipLaunchKernelGGL(rs_v_u8_kernel, dim3((unsigned)((mow + 255) / 256), (unsigned)((moh + 3) / 4), (unsigned)n), dim3(256), 0,
                           st, desc_dev, tables, tmp);
        SPE_CHECK_LAUNCH();
        return 0;
    }
    if (!lut || !mask || mow > Wmax || moh > Hmax || Hmax > RS_MAX_SIDE || Wmax > RS_MAX_SIDE) return -2;
    if (n > 65535 / 3) return -2;
    const int lpr = 1 + (Wmax + 3) / 4;
    const long lanes = (long)Hmax * lpr;                                      // per (image, channel) plane
    hipLaunchKernelGGL(rs_v_norm_kernel, dim3((unsigned)((lanes + 255) / 256), (unsigned)(3 * n)), dim3(256), 0, st, desc_dev, tables, tmp,
                       lut, out, mask, Hmax, Wmax, lpr);
    SPE_CHECK_LAUNCH();
    return 0;
}
