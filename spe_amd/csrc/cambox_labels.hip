// CAM -> pseudo boxes on the device (reference cams_deit.py:61-96 get_multi_bboxes from the
// thresholded image on: cv2.findContours(RETR_TREE), contourArea, boundingRect, keep area >= ratio * largest).  The host path
// (csrc/cambox.hip, spe_cam_contour_boxes) walks every border serially; here no border is walked: areas, boxes and discovery
// order of all borders come from two connected-component labellings of the zero-padded image, one 2x2 window per pixel and
// integer atomics - the formulation and its index arithmetic are in cambox_index.h.  All M maps share every launch (map index
// in grid.y):
//   init      each pixel links to the start of its horizontal run of its own class inside its 64-pixel segment (one ballot)
//   merge     union-find with atomicMin on roots: run to the run left of the segment boundary, run to the runs above it
//             (foreground 8-connected, background 4-connected; one union per run overlap, not per pixel)
//   compress  every pixel takes its root = the smallest index of its component (unique end state, whatever the execution
//             order); root pixels zero their accumulators, which live at the root's own index
//   count     one lane per column of 8 cells: half-unit area increments, kept in registers while the root stays the same and
//             then pre-reduced in the wave when its lanes share the root (one atomic per 8 x 64 cells of a large blob), and
//             atomicMin / atomicMax boxes from the pixels that touch the other class
//   fold      every border adds its own count to each of its ancestors in the border tree (parent = label of the pixel west of
//             the root: strictly decreasing, so the walk ends at the frame); after the counts are complete: its own launch
//   top       the largest area over the roots of each map (wave maximum, one atomicMax per wave)
//   collect   the roots with area >= ratio * largest go to the map's survivor list (slots by one atomicAdd per wave)
//   rank      one workgroup per map: rank the survivors by (area descending, key ascending) by counting, write boxes and count
// (one workgroup per map scanning all labels for the top and the survivors took 0.23 ms for six 1333 x 800 maps, these three
// launches take 0.03; the count kernel with one atomic per wave of 64 cells took 0.24 ms there, with the 8-row columns 0.08)
// Integer atomics only: the result is bitwise reproducible.  Every find loop follows strictly decreasing labels; all loops are
// bounded by a multiple of the pixel count and set a flag on overrun (status -6 for that map) instead of spinning.
#include "common.h"
#include "cambox_index.h"
#include <limits.h>

namespace {
struct CamPlanes { int* lab; int* own2; int* area2; int* x0; int* y0; int* x1; int* y1; int* flag; int* list; };
__device__ __forceinline__ CamPlanes cam_planes(int* ws, int rows, int cols) {
    const long pl = cambox_plane_ints(rows, cols);
    int* base = ws + (long)blockIdx.y * cambox_map_ints(rows, cols);
    CamPlanes p; p.lab = base; p.own2 = base + pl; p.area2 = base + 2 * pl; p.x0 = base + 3 * pl; p.y0 = base + 4 * pl; p.x1 = base + 5 * pl;
    p.y1 = base + 6 * pl; p.flag = base + 7 * pl; p.list = p.flag + 4;
    return p;
}
// one wave = one 64-pixel segment of one padded row; 4 waves per workgroup
struct CamPix { bool valid; int y, x, p; };
__device__ __forceinline__ CamPix cam_pix(int rows, int cols) {
    const int W = cols + 2, Hh = rows + 2, segsx = (W + 63) >> 6;
    const long seg = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    CamPix q;
    q.y = (int)(seg / segsx); q.x = (int)(seg % segsx) * 64 + (threadIdx.x & 63);
    q.valid = q.y < Hh && q.x < W;
    q.p = q.y * W + q.x;
    return q;
}
__device__ __forceinline__ int cam_ld(const int* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// A stale label read is harmless: a label only ever decreases and every former value is still an ancestor; atomicMin decides.
__device__ bool cam_union(int* lab, int a, int b, long limit) {
    long steps = 0;
    while (true) {
        for (int t; (t = cam_ld(lab + a)) != a; a = t) if (++steps > limit) return false;
        for (int t; (t = cam_ld(lab + b)) != b; b = t) if (++steps > limit) return false;
        if (a == b) return true;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(lab + a, b);
        if (old == a) return true;              // a was a root and now hangs under b
        a = old;                                // a had a parent already: that parent and b still have to meet
        if (++steps > limit) return false;
    }
}

__global__ __launch_bounds__(256) void cam_label_init_kernel(const unsigned char* __restrict__ imgs, int* __restrict__ ws, int rows, int cols) {
    const CamPlanes P = cam_planes(ws, rows, cols);
    const unsigned char* img = imgs + (long)blockIdx.y * rows * cols;
    const CamPix q = cam_pix(rows, cols);
    const int lane = threadIdx.x & 63;
    const bool fg = q.valid && cambox_fg(img, rows, cols, q.y, q.x);
    const unsigned long long fm = __ballot(fg), vm = __ballot(q.valid);
    if (q.valid) P.lab[q.p] = q.p - lane + cambox_run_start(fg ? fm : (vm & ~fm), lane);
    if (blockIdx.x == 0 && threadIdx.x == 0) { P.flag[0] = 0; P.flag[1] = -1; P.flag[2] = 0; }     // chain overrun, top area2, survivors
}

__global__ __launch_bounds__(256) void cam_label_merge_kernel(const unsigned char* __restrict__ imgs, int* __restrict__ ws, int rows, int cols) {
    const CamPlanes P = cam_planes(ws, rows, cols);
    const unsigned char* img = imgs + (long)blockIdx.y * rows * cols;
    const CamPix q = cam_pix(rows, cols);
    if (!q.valid) return;
    const int W = cols + 2;
    const long limit = 4 * cambox_padded_pixels(rows, cols) + 64;
    const bool fg = cambox_fg(img, rows, cols, q.y, q.x);
    const bool w = q.x > 0 && cambox_fg(img, rows, cols, q.y, q.x - 1) == fg;
    bool ok = true;
    if ((threadIdx.x & 63) == 0 && w) ok = cam_union(P.lab, q.p, q.p - 1, limit);          // the run goes on across the segment boundary
    if (q.y > 0) {
        const bool nw = q.x > 0 && cambox_fg(img, rows, cols, q.y - 1, q.x - 1) == fg;
        const bool n = cambox_fg(img, rows, cols, q.y - 1, q.x) == fg;
        const bool ne = q.x < W - 1 && cambox_fg(img, rows, cols, q.y - 1, q.x + 1) == fg;
        const CamboxLinks l = cambox_links(fg, w, nw, n, ne, W);
        for (int k = 0; k < l.n; ++k) ok = cam_union(P.lab, q.p, q.p + l.off[k], limit) && ok;
    }
    if (!ok) atomicOr(P.flag, 1);
}

__global__ __launch_bounds__(256) void cam_label_compress_kernel(int* __restrict__ ws, int rows, int cols) {
    const CamPlanes P = cam_planes(ws, rows, cols);
    const CamPix q = cam_pix(rows, cols);
    if (!q.valid) return;
    const long limit = cambox_padded_pixels(rows, cols);
    long steps = 0;
    int r = q.p;
    for (int t; (t = cam_ld(P.lab + r)) != r; r = t) if (++steps > limit) { atomicOr(P.flag, 1); return; }
    if (r != q.p) { __hip_atomic_store(P.lab + q.p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
    P.own2[r] = 0; P.area2[r] = 0; P.x0[r] = INT_MAX; P.y0[r] = INT_MAX; P.x1[r] = -1; P.y1[r] = -1;
}

// own2[root] += v for the lanes with root >= 0 and v > 0; one atomic for the wave when they all name the same root.  Every
// lane of the wave calls this.
__device__ __forceinline__ void cam_wave_add(int* own2, int root, int v) {
    const bool has = root >= 0 && v > 0;
    const unsigned long long m = __ballot(has);
    if (m == 0) return;
    const int first = __ffsll((long long)m) - 1;
    const int r0 = __shfl(root, first, 64);
    if (__ballot(has && root == r0) == m) {
        int s = has ? v : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if ((int)(threadIdx.x & 63) == first) atomicAdd(own2 + r0, s);
    } else if (has) atomicAdd(own2 + root, v);
}

// lane-local run of increments for one root: flushed with one atomic when the root changes
__device__ __forceinline__ void cam_run_add(int* own2, int& run_root, int& run_sum, int root, int v) {
    if (root < 0 || v <= 0) return;
    if (root == run_root) { run_sum += v; return; }
    if (run_sum > 0) atomicAdd(own2 + run_root, run_sum);
    run_root = root; run_sum = v;
}

// One wave = CAM_COUNT_ROWS cell rows of one 64-pixel segment: a lane walks down its column, carries the lower pixel pair of a
// cell over as the upper pair of the next, and keeps its increments in registers while the root stays the same; the wave then
// sums them.  A large blob gets one atomic per CAM_COUNT_ROWS x 64 cells instead of one per cell.
#define CAM_COUNT_ROWS 8
__global__ __launch_bounds__(256) void cam_count_kernel(const unsigned char* __restrict__ imgs, int* __restrict__ ws, int rows, int cols) {
    const CamPlanes P = cam_planes(ws, rows, cols);
    const unsigned char* img = imgs + (long)blockIdx.y * rows * cols;
    const int W = cols + 2, Hh = rows + 2, segsx = (W + 63) >> 6;
    const long seg = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long ybase = (seg / segsx) * CAM_COUNT_ROWS;                          // wave-uniform
    const int x = (int)(seg % segsx) * 64 + (threadIdx.x & 63);
    const bool xcell = x < W - 1;
    int own_r = -1, own_s = 0, hole_r = -1, hole_s = 0;
    int lab[4] = {0, 0, 0, 0};
    bool fg[4] = {false, false, false, false};
    if (xcell && ybase < Hh - 1) {
        const int p = (int)ybase * W + x;
        lab[2] = P.lab[p]; lab[3] = P.lab[p + 1];
        fg[2] = cambox_fg(img, rows, cols, (int)ybase, x); fg[3] = cambox_fg(img, rows, cols, (int)ybase, x + 1);
    }
    for (int r = 0; r < CAM_COUNT_ROWS; ++r) {
        const long yl = ybase + r;
        if (yl >= Hh - 1) break;                                                // the last padded row owns no cell (wave-uniform exit)
        if (!xcell) continue;
        const int y = (int)yl, p = y * W + x;
        lab[0] = lab[2]; lab[1] = lab[3]; fg[0] = fg[2]; fg[1] = fg[3];
        lab[2] = P.lab[p + W]; lab[3] = P.lab[p + W + 1];
        fg[2] = cambox_fg(img, rows, cols, y + 1, x); fg[3] = cambox_fg(img, rows, cols, y + 1, x + 1);
        const CamboxCell c = cambox_cell(lab, fg);
        cam_run_add(P.own2, own_r, own_s, c.own, c.own_add);
        cam_run_add(P.own2, hole_r, hole_s, c.hole[0], c.hole_add[0]);
        if (c.hole[1] >= 0) atomicAdd(P.own2 + c.hole[1], c.hole_add[1]);       // a second hole across the diagonal: rare
        // boxes: extreme pixels of a component always touch the other class.  A foreground or hole pixel is never on the padded
        // border (that is the frame, label 0), so it owns a cell and its four neighbours exist.
        if (fg[0] || lab[0] != 0) {
            const bool me = fg[0];
            if (fg[1] != me || fg[2] != me || cambox_fg(img, rows, cols, y, x - 1) != me || cambox_fg(img, rows, cols, y - 1, x) != me) {
                atomicMin(P.x0 + lab[0], x); atomicMin(P.y0 + lab[0], y);
                atomicMax(P.x1 + lab[0], x); atomicMax(P.y1 + lab[0], y);
            }
        }
    }
    cam_wave_add(P.own2, own_r, own_s);
    cam_wave_add(P.own2, hole_r, hole_s);
}

__global__ __launch_bounds__(256) void cam_fold_kernel(int* __restrict__ ws, int rows, int cols) {
    const CamPlanes P = cam_planes(ws, rows, cols);
    const CamPix q = cam_pix(rows, cols);
    if (!q.valid || q.p == 0 || P.lab[q.p] != q.p) return;
    // The pixel west of a hole's raster-first pixel is foreground (a background one would belong to the hole and come first), the
    // one west of a component's is background: the hole around it, or the frame (label 0), where the walk ends.
    const int own = P.own2[q.p];
    atomicAdd(P.area2 + q.p, own);
    if (own == 0) return;
    const long limit = cambox_padded_pixels(rows, cols);
    long steps = 0;
    for (int a = P.lab[q.p - 1]; a != 0; a = P.lab[a - 1]) {
        atomicAdd(P.area2 + a, own);
        if (++steps > limit) { atomicOr(P.flag, 1); return; }
    }
}

// largest area2 over the border roots of a map (pixel 0 is the frame's root: no border) -> flag[1]
__global__ __launch_bounds__(256) void cam_top_kernel(int* __restrict__ ws, int rows, int cols) {
    const CamPlanes P = cam_planes(ws, rows, cols);
    const CamPix q = cam_pix(rows, cols);
    const bool root = q.valid && q.p != 0 && P.lab[q.p] == q.p;
    if (__ballot(root) == 0) return;
    int v = root ? P.area2[q.p] : -1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(P.flag + 1, v);
}

// the survivors of a map, in arrival order, into its list (6 ints each: area2, key, box); flag[2] counts all of them, also those
// beyond max_boxes, which are not stored
__global__ __launch_bounds__(256) void cam_collect_kernel(const unsigned char* __restrict__ imgs, int* __restrict__ ws, int rows, int cols,
                                                          float area_ratio, int max_boxes) {
    const CamPlanes P = cam_planes(ws, rows, cols);
    const unsigned char* img = imgs + (long)blockIdx.y * rows * cols;
    const CamPix q = cam_pix(rows, cols);
    const int lane = threadIdx.x & 63;
    int a2 = 0;
    bool keep = q.valid && q.p != 0 && P.lab[q.p] == q.p;
    if (keep) { a2 = P.area2[q.p]; keep = cambox_keep(a2, cam_ld(P.flag + 1), area_ratio); }
    const unsigned long long m = __ballot(keep);
    if (m == 0) return;
    const int first = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == first) base = atomicAdd(P.flag + 2, __popcll(m));
    base = __shfl(base, first, 64);
    const int slot = base + __popcll(m & ((1ull << lane) - 1ull));
    if (!keep || slot >= max_boxes) return;
    const bool fg = cambox_fg(img, rows, cols, q.y, q.x);
    int* e = P.list + 6 * slot;
    e[0] = a2; e[1] = cambox_key(q.p, fg);
    cambox_emit(fg, P.x0[q.p], P.y0[q.p], P.x1[q.p], P.y1[q.p], e + 2);
}

#define CAM_RANK_THREADS 1024
__global__ __launch_bounds__(CAM_RANK_THREADS) void cam_rank_kernel(const int* __restrict__ ws_c, int rows, int cols, int* __restrict__ boxes,
                                                                   int* __restrict__ nboxes, int max_boxes) {
    __shared__ int s_area[CAMBOX_MAX_BOXES], s_key[CAMBOX_MAX_BOXES];
    const CamPlanes P = cam_planes(const_cast<int*>(ws_c), rows, cols);
    const int m = blockIdx.y, n = P.flag[2];
    int* out = boxes + (long)m * max_boxes * 4;
    if (P.flag[0] != 0 || P.flag[1] < 0 || n > max_boxes) {
        if (threadIdx.x == 0) {
            if (P.flag[0] != 0) nboxes[m] = CAMBOX_STATUS_CHAIN;
            else if (P.flag[1] < 0) { out[0] = 0; out[1] = 0; out[2] = 1; out[3] = 1; nboxes[m] = 1; }      // no border at all
            else nboxes[m] = CAMBOX_STATUS_OVERFLOW;
        }
        return;
    }
    for (int s = threadIdx.x; s < n; s += CAM_RANK_THREADS) { s_area[s] = P.list[6 * s]; s_key[s] = P.list[6 * s + 1]; }
    __syncthreads();
    for (int s = threadIdx.x; s < n; s += CAM_RANK_THREADS) {
        int rank = 0;
        for (int t = 0; t < n; ++t) rank += cambox_before(s_area[t], s_key[t], s_area[s], s_key[s]) ? 1 : 0;
        const int* e = P.list + 6 * s + 2;
        int* b = out + 4 * rank;
        b[0] = e[0]; b[1] = e[1]; b[2] = e[2]; b[3] = e[3];
    }
    if (threadIdx.x == 0) nboxes[m] = n;
}
}  // namespace

// C-ABI: see include/spe_hip.h.
extern "C" int spe_cam_boxes_device_workspace(int M, int rows, int cols, size_t* bytes) {
    if (!bytes || M < 0 || rows < 1 || cols < 1 || cambox_padded_pixels(rows, cols) > (1L << 30)) return -2;
    *bytes = (size_t)M * (size_t)cambox_map_ints(rows, cols) * sizeof(int);
    return 0;
}

extern "C" int spe_cam_boxes_device(const unsigned char* img, int M, int rows, int cols, float area_ratio, void* workspace,
                                    size_t workspace_bytes, int* boxes, int* nboxes, int max_boxes, hipStream_t st) {
    if (M == 0) return 0;
    size_t need = 0;
    if (spe_cam_boxes_device_workspace(M, rows, cols, &need) != 0 || M > 65535 || max_boxes < 1 || max_boxes > CAMBOX_MAX_BOXES ||
        ((uintptr_t)workspace & 15) != 0)
        return -2;
    if (!workspace || workspace_bytes < need) return -4;
    int* ws = static_cast<int*>(workspace);
    const long segs = (long)((cols + 2 + 63) / 64) * (rows + 2);
    const dim3 grid((unsigned)((segs + 3) / 4), (unsigned)M), block(256);
    hipLaunchKernelGGL(cam_label_init_kernel, grid, block, 0, st, img, ws, rows, cols);
    SPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(cam_label_merge_kernel, grid, block, 0, st, img, ws, rows, cols);
    SPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(cam_label_compress_kernel, grid, block, 0, st, ws, rows, cols);
    SPE_CHECK_LAUNCH();
    const long csegs = (long)((cols + 2 + 63) / 64) * ((rows + 2 + CAM_COUNT_ROWS - 1) / CAM_COUNT_ROWS);
    hipLaunchKernelGGL(cam_count_kernel, dim3((unsigned)((csegs + 3) / 4), (unsigned)M), block, 0, st, img, ws, rows, cols);
    SPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(cam_fold_kernel, grid, block, 0, st, ws, rows, cols);
    SPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(cam_top_kernel, grid, block, 0, st, ws, rows, cols);
    SPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(cam_collect_kernel, grid, block, 0, st, img, ws, rows, cols, area_ratio, max_boxes);
    SPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(cam_rank_kernel, dim3(1, (unsigned)M), dim3(CAM_RANK_THREADS), 0, st, ws, rows, cols, boxes, nboxes, max_boxes);
    SPE_CHECK_LAUNCH();
    return 0;
}
