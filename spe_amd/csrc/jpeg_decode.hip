// Baseline JPEG decoding, device side: quantised coefficients -> the uint8 [H][W][3] image DeviceImage takes,
// equal to libjpeg-turbo's default decode (what Pillow gives) bit for bit.  The serial part - markers and Huffman codes - runs on the
// host (jpeg_entropy.h, exported from here); everything that touches a pixel is the two launches below, for a whole batch:
//   pass A  jd_idct_kernel   dequantise + jidctint.c's "islow" inverse DCT + range limit -> uint8 component planes (padded block grid)
//   pass B  jd_colour_kernel "fancy" triangle upsampling of 2x1 / 2x2 chroma + jdcolor.c's 16-bit fixed-point YCbCr -> RGB -> dst
// All arithmetic is 32-bit integer.  Every launch serves n images through a descriptor table (JD_DESC longs per image) that exists
// twice, as with spe_resample_*: the host copy is validated and sizes the grids, the device copy is what the kernels read.  Every
// index a kernel forms comes from the descriptor, never from coefficient data.
#include "common.h"
#include "jpeg_entropy.h"

#define JD_DESC 16
#define JD_MAX_SIDE 32768        // what the resample kernels take
#define JD_QT 192                // shorts in front of an image's coefficients: its 3 x 64 quantisation tables

enum { J_W, J_H, J_NCOMP, J_HS, J_VS, J_MCUX, J_MCUY, J_COEF, J_PLANES, J_DST };

static inline long jd_blocks(const long* d) { return d[J_MCUX] * d[J_MCUY] * (d[J_NCOMP] == 1 ? 1 : d[J_HS] * d[J_VS] + 2); }

// 0, or -2 for the first bad descriptor.  Records and plane sets must lie inside the two buffers, in order, without overlap.
static int jd_validate(const long* d, int n, long coef_elems, long planes_bytes, long* max_blocks, long* max_lanes) {
    long coef_end = 0, planes_end = 0;
    *max_blocks = *max_lanes = 0;
    for (int i = 0; i < n; ++i, d += JD_DESC) {
        if (d[J_W] < 1 || d[J_H] < 1 || d[J_W] > JD_MAX_SIDE || d[J_H] > JD_MAX_SIDE || d[J_DST] == 0) return -2;
        const long hs = d[J_HS], vs = d[J_VS];
        if (d[J_NCOMP] == 1) { if (hs != 1 || vs != 1) return -2; }
        else if (d[J_NCOMP] != 3 || !((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return -2;
        if (d[J_MCUX] != (d[J_W] + 8 * hs - 1) / (8 * hs) || d[J_MCUY] != (d[J_H] + 8 * vs - 1) / (8 * vs)) return -2;
        const long nb = jd_blocks(d);
        if (d[J_COEF] < coef_end || (d[J_COEF] & 7) || d[J_COEF] + JD_QT + nb * 64 > coef_elems) return -2;
        if (d[J_PLANES] < planes_end || (d[J_PLANES] & 15) || d[J_PLANES] + nb * 64 > planes_bytes) return -2;
        coef_end = d[J_COEF] + JD_QT + nb * 64;
        planes_end = d[J_PLANES] + nb * 64;
        if (nb > *max_blocks) *max_blocks = nb;
        const long lanes = d[J_H] * (1 + (d[J_W] + 3) / 4);
        if (lanes > *max_lanes) *max_lanes = lanes;
    }
    return 0;
}

// ---- pass A ----------------------------------------------------------------------------------------------------------------
// jidctint.c's 8-point pass (CONST_BITS 13): the even part on i0, i2, i4, i6, the odd part on i1, i3, i5, i7; descale by s
template <int S>
__device__ __forceinline__ void jd_pass8(const int (&i)[8], int (&o)[8]) {
    int z1 = (i[2] + i[6]) * 4433;
    const int t2 = z1 - i[6] * 15137, t3 = z1 + i[2] * 6270;
    const int t0 = (i[0] + i[4]) << 13, t1 = (i[0] - i[4]) << 13;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a = i[7], b = i[5], c = i[3], d = i[1];
    z1 = a + d;
    int z2 = b + c, z3 = a + c, z4 = b + d;
    const int z5 = (z3 + z4) * 9633;
    a *= 2446; b *= 16819; c *= 25172; d *= 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    a += z1 + z3; b += z2 + z4; c += z2 + z3; d += z1 + z4;
    const int r = 1 << (S - 1);
    o[0] = (t10 + d + r) >> S; o[7] = (t10 - d + r) >> S;
    o[1] = (t11 + c + r) >> S; o[6] = (t11 - c + r) >> S;
    o[2] = (t12 + b + r) >> S; o[5] = (t12 - b + r) >> S;
    o[3] = (t13 + a + r) >> S; o[4] = (t13 - a + r) >> S;
}

// libjpeg's range-limit table in closed form: index (v + 128) & 1023 -> 0..255 identity, then 384 x 255, then 384 x 0
__device__ __forceinline__ unsigned jd_limit(int v) {
    const int t = (v + 128) & 1023;
    return (unsigned)(t < 256 ? t : (t < 640 ? 255 : 0));
}

// One workgroup: 32 blocks, 8 lanes each.  Lane r of a block loads row r (16 bytes, coalesced) and dequantises it into LDS; as lane c it
// transforms column c in place; as lane r again it transforms row r and stores 8 samples with one 8-byte store.  The 8 lanes of a
// block sit in one wave; rows of the LDS tile are 9 ints apart, so the 32 lanes of a half wave touch 32 different banks both ways.
#define JD_LDS_ROW 9
__global__ __launch_bounds__(256) void jd_idct_kernel(const long* __restrict__ desc, const short* __restrict__ coef,
                                                      unsigned char* __restrict__ planes) {
    __shared__ int tile[32][8 * JD_LDS_ROW];
    const long* d = desc + (long)blockIdx.y * JD_DESC;
    const int lb = threadIdx.x >> 3, l = threadIdx.x & 7;
    const long blk = (long)blockIdx.x * 32 + lb;                              // block of the image, components one after the other
    const int mcux = (int)d[J_MCUX], mcuy = (int)d[J_MCUY], hs = (int)d[J_HS], vs = (int)d[J_VS];
    const long n0 = (long)mcux * mcuy * hs * vs, n1 = (long)mcux * mcuy;
    const bool live = blk < (d[J_NCOMP] == 1 ? n0 : n0 + 2 * n1);
    const int c = blk < n0 ? 0 : (blk < n0 + n1 ? 1 : 2);
    int* t = tile[lb];
    if (live) {
        const short* rec = coef + d[J_COEF];
        const int4 raw = *reinterpret_cast<const int4*>(rec + JD_QT + blk * 64 + l * 8);
        const int4 qraw = *reinterpret_cast<const int4*>(rec + c * 64 + l * 8);
        const int w[4] = {raw.x, raw.y, raw.z, raw.w}, q[4] = {qraw.x, qraw.y, qraw.z, qraw.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            t[l * JD_LDS_ROW + 2 * k] = (int)(short)(w[k] & 0xFFFF) * (q[k] & 0xFFFF);
            t[l * JD_LDS_ROW + 2 * k + 1] = (w[k] >> 16) * (int)((unsigned)q[k] >> 16);
        }
    }
    __syncthreads();
    int in[8], out[8];
    if (live) {
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = t[k * JD_LDS_ROW + l];
        jd_pass8<11>(in, out);
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k * JD_LDS_ROW + l] = out[k];
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = t[l * JD_LDS_ROW + k];
        jd_pass8<18>(in, out);
        const long cb = c == 0 ? blk : (c == 1 ? blk - n0 : blk - n0 - n1);   // block of the component, raster order
        const int bw = c == 0 ? mcux * hs : mcux;
        const int by = (int)(cb / bw), bx = (int)(cb - (long)by * bw);
        const long plane = c == 0 ? 0 : (c == 1 ? n0 : n0 + n1) * 64;
        uint2 v;
        v.x = jd_limit(out[0]) | (jd_limit(out[1]) << 8) | (jd_limit(out[2]) << 16) | (jd_limit(out[3]) << 24);
        v.y = jd_limit(out[4]) | (jd_limit(out[5]) << 8) | (jd_limit(out[6]) << 16) | (jd_limit(out[7]) << 24);
        *reinterpret_cast<uint2*>(planes + d[J_PLANES] + plane + ((long)(by * 8 + l) * bw + bx) * 8) = v;
    }
}

// ---- pass B ----------------------------------------------------------------------------------------------------------------
// the chroma sample of output pixel (x, y): p is the component's plane (pitch bytes a row), of which dw x dh samples are real
__device__ __forceinline__ int jd_chroma(const unsigned char* __restrict__ p, int pitch, int x, int y, int hs, int vs, int dw, int dh) {
    if (hs == 1) return p[(long)y * pitch + x];
    const int i = x >> 1;
    if (dw <= 2) return p[(long)(vs == 2 ? y >> 1 : y) * pitch + i];          // libjpeg-turbo replicates below three samples a row
    const int nx = (x & 1) ? (i + 1 < dw ? i + 1 : dw - 1) : (i > 0 ? i - 1 : 0);
    if (vs == 1) {
        const unsigned char* r = p + (long)y * pitch;
        return (3 * r[i] + r[nx] + 1 + (x & 1)) >> 2;
    }
    const int j = y >> 1;
    const int ny = (y & 1) ? (j + 1 < dh ? j + 1 : dh - 1) : (j > 0 ? j - 1 : 0);
    const unsigned char *r0 = p + (long)j * pitch, *r1 = p + (long)ny * pitch;
    const int s = 3 * r0[i] + r1[i], sn = 3 * r0[nx] + r1[nx];
    return (3 * s + sn + 8 - (x & 1)) >> 4;
}

__device__ __forceinline__ unsigned jd_clamp8(int v) { return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// One lane: up to four consecutive pixels of one row.  A row of dst starts at any byte address (3 W is arbitrary).  Pixel x lies at a
// 4-byte aligned address when x = (row address) mod 4, so lane 0 of a row takes the 0 .. 3 pixels in front of the first such pixel
// with byte stores, lane j >= 1 the j-th group of four with three 4-byte stores, and a group the row's end cuts off goes byte by byte.
__global__ __launch_bounds__(256) void jd_colour_kernel(const long* __restrict__ desc, const unsigned char* __restrict__ planes) {
    const long* d = desc + (long)blockIdx.y * JD_DESC;
    const int W = (int)d[J_W], H = (int)d[J_H], lpr = 1 + (W + 3) / 4;
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;                     // < JD_MAX_SIDE * (JD_MAX_SIDE / 4 + 1) < 2^31
    const int y = (int)(idx / (unsigned)lpr), j = (int)(idx - (unsigned)y * (unsigned)lpr);
    if (y >= H) return;
    unsigned char* row = (unsigned char*)d[J_DST] + (long)y * W * 3;
    int head = (int)((uintptr_t)row & 3);
    if (head > W) head = W;
    const int xs = j == 0 ? 0 : head + 4 * (j - 1);
    const int cnt = j == 0 ? head : (W - xs < 4 ? W - xs : 4);
    if (cnt <= 0) return;
    const int hs = (int)d[J_HS], vs = (int)d[J_VS], mcux = (int)d[J_MCUX], mcuy = (int)d[J_MCUY];
    const bool grey = d[J_NCOMP] == 1;
    const unsigned char* py = planes + d[J_PLANES];
    const long n0 = (long)mcux * mcuy * hs * vs * 64, n1 = (long)mcux * mcuy * 64;
    const unsigned char *pcb = py + n0, *pcr = pcb + n1;
    const int ypitch = mcux * hs * 8, cpitch = mcux * 8;
    const int dw = (W + hs - 1) / hs, dh = (H + vs - 1) / vs;
    unsigned char px[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int x = xs + i < W ? xs + i : W - 1;                            // lanes past the end repeat the last pixel, unstored
        const int yv = py[(long)y * ypitch + x];
        int r = yv, g = yv, b = yv;
        if (!grey) {
            const int cb = jd_chroma(pcb, cpitch, x, y, hs, vs, dw, dh) - 128, cr = jd_chroma(pcr, cpitch, x, y, hs, vs, dw, dh) - 128;
            r = yv + ((91881 * cr + 32768) >> 16);
            g = yv + ((-22554 * cb - 46802 * cr + 32768) >> 16);
            b = yv + ((116130 * cb + 32768) >> 16);
        }
        px[3 * i] = (unsigned char)jd_clamp8(r); px[3 * i + 1] = (unsigned char)jd_clamp8(g); px[3 * i + 2] = (unsigned char)jd_clamp8(b);
    }
    unsigned char* o = row + (long)xs * 3;
    if (j > 0 && cnt == 4) {
        unsigned* o4 = reinterpret_cast<unsigned*>(o);
#pragma unroll
        for (int k = 0; k < 3; ++k) o4[k] = px[4 * k] | (px[4 * k + 1] << 8) | (px[4 * k + 2] << 16) | ((unsigned)px[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 3 * cnt; ++k) o[k] = px[k];
    }
}

// C-ABI: see include/spe_hip.h
extern "C" int spe_jpeg_probe(const unsigned char* data, long n, int* info) { return spe_jpeg_probe_impl(data, n, info); }
extern "C" int spe_jpeg_entropy(const unsigned char* data, long n, short* coef, long coef_elems, int* reason) {
    return spe_jpeg_entropy_impl(data, n, coef, coef_elems, reason);
}

extern "C" int spe_jpeg_reconstruct(const long* desc_host, const long* desc_dev, int n, const short* coef, long coef_elems,
                                    unsigned char* planes, long planes_bytes, hipStream_t st) {
    if (n <= 0 || n > 65535 || !desc_host || !desc_dev || !coef || !planes || ((uintptr_t)coef & 15) || ((uintptr_t)planes & 15)) return -2;
    long max_blocks, max_lanes;
    const int rc = jd_validate(desc_host, n, coef_elems, planes_bytes, &max_blocks, &max_lanes);
    if (rc) return rc;
    hipLaunchKernelGGL(jd_idct_kernel, dim3((unsigned)((max_blocks + 31) / 32), (unsigned)n), dim3(256), 0, st, desc_dev, coef, planes);
    SPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(jd_colour_kernel, dim3((unsigned)((max_lanes + 255) / 256), (unsigned)n), dim3(256), 0, st, desc_dev, planes);
    SPE_CHECK_LAUNCH();
    return 0;
}
