// Learned position embedding of the patch grid (reference models/position_encoding.py:60-85: two nn.Embedding(50, npf) tables
// indexed by the column and the row of a cell, concatenated column features first) and its adjoint.
#include "common.h"

#define POS_TABLE_ROWS 50        // rows of each table: the largest grid side the reference can embed

// V floats per lane: float4 when npf % 4 == 0 and every pointer is 16-B aligned, else one float (any npf)
template <int V> struct PosVec;
template <> struct PosVec<4> {
    typedef float4 T;
    static __device__ __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
    static __device__ __forceinline__ T add(T a, T b) { return spe_add4(a, b); }
};
template <> struct PosVec<1> {
    typedef float T;
    static __device__ __forceinline__ T zero() { return 0.f; }
    static __device__ __forceinline__ T add(T a, T b) { return a + b; }
};

// out[b][y][x][c] = col[x][c] for c < npf, row[y][c - npf] above: a copy, one lane per V consecutive channels of a cell (a group of V
// never straddles the two halves: V divides npf).  The layout of spe_pos_sine's output, so the transformer's [B, hw, d] view stays copy-free.
template <int V>
__global__ __launch_bounds__(256) void pos_learned_fwd_kernel(const float* __restrict__ col, const float* __restrict__ row,
                                                              float* __restrict__ out, int B, int h, int w, int npf) {
    typedef typename PosVec<V>::T vec_t;
    const int CW = 2 * npf / V;
    const long total = (long)B * h * w * CW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % CW) * V; long t = i / CW;
        const int x = (int)(t % w); t /= w;
        const int y = (int)(t % h);
        const float* src = c < npf ? col + (long)x * npf + c : row + (long)y * npf + (c - npf);
        reinterpret_cast<vec_t*>(out)[i] = *reinterpret_cast<const vec_t*>(src);
    }
}

// Adjoint.  Workgroup r < 50 owns row r of d_col, workgroup 50 + r row r of d_row: no sum crosses workgroups, nothing is added to what the
// destination held, every one of the 2 x 50 rows is stored (zeros for the table rows the grid does not reach).
//   d_col[x][c] = sum_b sum_y g[b][y][x][c]            d_row[y][c] = sum_b sum_x g[b][y][x][npf + c]
// The B * h (B * w) terms of an output are numbered t = b * n + k (k = y or x) and dealt to the S = 256 / tps slices of the workgroup, slice s
// adding t = s, s + S, .. in ascending order; a slice is tps lanes reading V consecutive channels each (coalesced rows over c).  The first
// slice then adds the S partial sums in slice order from LDS.  tps depends on npf alone: the order of every sum is fixed by the shape.
template <int V>
__global__ __launch_bounds__(256) void pos_learned_bwd_kernel(const float* __restrict__ g, float* __restrict__ d_col, float* __restrict__ d_row,
                                                              int B, int h, int w, int npf, int tps) {
    typedef typename PosVec<V>::T vec_t;
    __shared__ vec_t part[256];
    const bool is_row = blockIdx.x >= POS_TABLE_ROWS;
    const int r = blockIdx.x - (is_row ? POS_TABLE_ROWS : 0);
    float* dst = is_row ? d_row : d_col;
    if (!dst) return;                                    // the whole workgroup: this table is not wanted
    vec_t* drow = reinterpret_cast<vec_t*>(dst + (long)r * npf);
    const int CW = npf / V;
    if (r >= (is_row ? h : w)) {
        for (int cu = threadIdx.x; cu < CW; cu += 256) drow[cu] = PosVec<V>::zero();
        return;
    }
    const long d = 2L * npf;
    const int n = is_row ? w : h;                        // terms per image
    const long kstride = is_row ? d : (long)w * d;       // from term k to k + 1
    const long img = (long)h * w * d;
    const float* base = g + (is_row ? (long)r * w * d + npf : (long)r * d);
    const int S = 256 / tps, s = threadIdx.x / tps, l = threadIdx.x % tps;
    const int terms = B * n;
    for (int c0 = 0; c0 < CW; c0 += tps) {               // one pass unless npf > 256 * V
        const int cu = c0 + l;
        vec_t acc = PosVec<V>::zero();
        if (cu < CW) {
            for (int t = s; t < terms; t += S) {
                const int b = t / n, k = t - b * n;
                acc = PosVec<V>::add(acc, *reinterpret_cast<const vec_t*>(base + b * img + k * kstride + (long)cu * V));
            }
        }
        part[threadIdx.x] = acc;
        __syncthreads();
        if (s == 0 && cu < CW) {
            vec_t tot = part[l];
            for (int j = 1; j < S; ++j) tot = PosVec<V>::add(tot, part[j * tps + l]);
            drow[cu] = tot;
        }
        __syncthreads();
    }
}

static bool pos_aligned16(const void* a, const void* b, const void* c) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}
static bool pos_grid_ok(int B, int h, int w, int npf) {
    return B >= 1 && npf >= 1 && h >= 1 && h <= POS_TABLE_ROWS && w >= 1 && w <= POS_TABLE_ROWS;
}

// C-ABI: see include/spe_hip.h
extern "C" int spe_pos_learned_fwd(const float* col, const float* row, float* out, int B, int h, int w, int npf, hipStream_t st) {
    if (!pos_grid_ok(B, h, w, npf)) return -2;
    const bool v4 = (npf & 3) == 0 && pos_aligned16(col, row, out);
    const long total = (long)B * h * w * (2 * npf / (v4 ? 4 : 1));
    long nb = (total + 255) / 256; if (nb > 4096) nb = 4096;
    if (v4) hipLaunchKernelGGL(pos_learned_fwd_kernel<4>, dim3((unsigned)nb), dim3(256), 0, st, col, row, out, B, h, w, npf);
    else hipLaunchKernelGGL(pos_learned_fwd_kernel<1>, dim3((unsigned)nb), dim3(256), 0, st, col, row, out, B, h, w, npf);
    SPE_CHECK_LAUNCH();
    return 0;
}

extern "C" int spe_pos_learned_bwd(const float* g, float* d_col, float* d_row, int B, int h, int w, int npf, hipStream_t st) {
    if (!pos_grid_ok(B, h, w, npf)) return -2;
    if (!d_col && !d_row) return 0;
    const bool v4 = (npf & 3) == 0 && pos_aligned16(g, d_col, d_row);
    const int CW = npf / (v4 ? 4 : 1);
    int tps = 16;                                        // lanes per slice: the power of two covering a row, 16 .. 256
    while (tps < CW && tps < 256) tps <<= 1;
    const dim3 grid(2 * POS_TABLE_ROWS);
    if (v4) hipLaunchKernelGGL(pos_learned_bwd_kernel<4>, grid, dim3(256), 0, st, g, d_col, d_row, B, h, w, npf, tps);
    else hipLaunchKernelGGL(pos_learned_bwd_kernel<1>, grid, dim3(256), 0, st, g, d_col, d_row, B, h, w, npf, tps);
    SPE_CHECK_LAUNCH();
    return 0;
}
