// Tile order of the GEMM kernels (gemm.hip, gemm_bf16.hip, gemm_nt2.hip) and the LDS-DMA load they share.
//
// Workgroup b runs on XCD b % 8 (8 private L2s).  The panels of the operand with more rows (same K: more bytes) are bound to XCDs - all
// tiles that read one such panel run on the same XCD - so that operand is fetched into one L2 only; the other one is re-fetched by each
// XCD.  The bound direction is padded to a multiple of 8 panels; the padding workgroups return at once.
#pragma once

struct TileOrder {
    int xcd_bind;      // 0: plain tile order, 1: M-panels bound to XCDs, 2: N-panels bound to XCDs
    int grid;          // workgroups in grid.x (tiles + padding)
};

// host: bind the operand with more rows if it has enough panels to balance 8 XCDs
static inline TileOrder tile_order(int M, int N, int tiles_m, int tiles_n) {
    TileOrder o{0, tiles_m * tiles_n};
    if (M >= N && tiles_m >= 16) o.xcd_bind = 1;
    else if (N > M && tiles_n >= 16) o.xcd_bind = 2;
    else if (tiles_m >= 16) o.xcd_bind = 1;
    else if (tiles_n >= 16) o.xcd_bind = 2;
    if (o.xcd_bind == 1) o.grid = 8 * ((tiles_m + 7) / 8) * tiles_n;
    if (o.xcd_bind == 2) o.grid = 8 * ((tiles_n + 7) / 8) * tiles_m;
    return o;
}

// device: blockIdx.x -> (tm, tn); false = a padding workgroup (nothing to do)
__device__ __forceinline__ bool tile_decode(int xcd_bind, int tiles_m, int tiles_n, int& tm, int& tn) {
    if (xcd_bind == 0) { tm = blockIdx.x % tiles_m; tn = blockIdx.x / tiles_m; }
    else {
        const int no = (xcd_bind == 1) ? tiles_n : tiles_m;
        const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
        const int tb = xcd + 8 * (idx / no), to = idx % no;
        tm = (xcd_bind == 1) ? tb : to; tn = (xcd_bind == 1) ? to : tb;
        if (tm >= tiles_m || tn >= tiles_n) return false;
    }
    return true;
}

// global -> LDS without staging registers: lane l's 16 B land at lds_dst + 16 l (lds_dst wave-uniform, M0 restored)
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
