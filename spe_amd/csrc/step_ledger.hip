// Step ledger: the loss bookkeeping of one training step on the device (reference engine.py:134-169 with util/misc.py:34-93,
// 139-253 behind it).  The reference forms the weighted total with one multiply and one add launch per loss
// key, reads it back before the backward for its isfinite guard, and reads ~95 more scalars back after the optimizer step for its
// meters.  Here ONE launch per step (ledger_record_kernel) forms the total and files every value in device-resident meters, and
// nothing is read back before a log line is due (ledger_summary_kernel: one launch, one [M, 5] table).
//
// This file is compiled with -ffp-contract=off (spe_amd/build.py EXTRA_FLAGS): total = ((0 + v0*w0) + v1*w1) + ... is Python's
// sum() over fp32 tensors only while every product is rounded before it is added - a fused multiply-add gives other bits.
// One workgroup per record launch, one thread per meter, fixed order: no atomics, bitwise reproducible.
//
// State block (caller-owned, zero-initialised = an empty ledger; D = 64 ring rows):
//   long steps, long bad_plus1 (first step with a non-finite total, + 1; 0: none), long reserved[2]
//   double totals [2K + 1 + E]          running sums: K unscaled, K scaled, loss, E extras
//   double ring_e [D][E]                extras of the last D steps
//   float  ring_v [D][K], ring_w [D][K] values and weights of the last D steps (row = step % D)
//   uchar  mask   [K rounded up to 8]   the newest mask
#include "common.h"
#include <math.h>

#define LG_D 64
#define LG_MAXK 256
#define LG_MAXE 8
#define LG_THREADS 256

struct LedgerExtras { double e[LG_MAXE]; };

struct LedgerView {
    long* head;
    double* totals;
    double* ring_e;
    float* ring_v;
    float* ring_w;
    unsigned char* mask;
};

__host__ __device__ static inline size_t ledger_bytes(int K, int E) {
    return 32 + 8 * (size_t)(2 * K + 1 + E) + 8 * (size_t)LG_D * E + 8 * (size_t)LG_D * K + (size_t)((K + 7) & ~7);
}

__device__ __forceinline__ LedgerView ledger_view(void* state, int K, int E) {
    LedgerView s;
    char* p = (char*)state;
    s.head = (long*)p; p += 32;
    s.totals = (double*)p; p += 8 * (size_t)(2 * K + 1 + E);
    s.ring_e = (double*)p; p += 8 * (size_t)LG_D * E;
    s.ring_v = (float*)p; p += 4 * (size_t)LG_D * K;
    s.ring_w = (float*)p; p += 4 * (size_t)LG_D * K;
    s.mask = (unsigned char*)p;
    return s;
}

__global__ __launch_bounds__(LG_THREADS) void ledger_record_kernel(const float* __restrict__ vals, const float* __restrict__ weights,
                                                                   const unsigned char* __restrict__ mask, LedgerExtras ex, int K, int E,
                                                                   void* state, float* __restrict__ total_out) {
    __shared__ float sv[LG_MAXK], ss[LG_MAXK];
    __shared__ unsigned char sm[LG_MAXK];
    __shared__ float stotal;
    const int tid = threadIdx.x;
    const LedgerView s = ledger_view(state, K, E);
    const long step = s.head[0];                                   // read by everyone before thread 0 advances it (after the barriers)
    const int row = (int)(step % LG_D);
    if (tid < K) {
        const float v = vals[tid], w = weights[tid];
        const unsigned char m = mask[tid] != 0;
        sv[tid] = v; ss[tid] = v * w; sm[tid] = m;
        s.ring_v[(size_t)row * K + tid] = v;
        s.ring_w[(size_t)row * K + tid] = w;
        s.mask[tid] = m;
    }
    if (tid < E) s.ring_e[(size_t)row * E + tid] = ex.e[tid];
    __syncthreads();
    if (tid == 0) {                                                // engine.py:144: sum() starts from the int 0 and adds in key order
        float t = 0.0f;
        for (int k = 0; k < K; ++k)
            if (sm[k]) t = t + ss[k];
        stotal = t;
    }
    __syncthreads();
    const float total = stotal;
    const int M = 2 * K + 1 + E;
    for (int i = tid; i < M; i += LG_THREADS) {                    // one thread owns a meter: SmoothedValue.update's total += value
        double add;
        bool on = true;
        if (i < K) add = (double)sv[i];
        else if (i < 2 * K) { add = (double)ss[i - K]; on = sm[i - K]; }
        else if (i == 2 * K) add = (double)total;
        else add = ex.e[i - 2 * K - 1];
        if (on) s.totals[i] = s.totals[i] + add;
    }
    if (tid == 0) {
        total_out[0] = total;
        if (!isfinite(total) && s.head[1] == 0) s.head[1] = step + 1;      // sticky: only the first bad step is kept
        s.head[0] = step + 1;
    }
}

__global__ __launch_bounds__(LG_THREADS) void ledger_total_bwd_kernel(const float* __restrict__ g, const float* __restrict__ weights,
                                                                      const unsigned char* __restrict__ mask, int K,
                                                                      float* __restrict__ dvals) {
    const int k = threadIdx.x;
    if (k < K) dvals[k] = mask[k] ? weights[k] * g[0] : 0.0f;
}

// One wave per meter; lane i holds the i-th oldest of the last n = min(steps, window) values.
__global__ __launch_bounds__(64) void ledger_summary_kernel(void* state, int K, int E, const int* __restrict__ windows,
                                                            const float* __restrict__ ring_override, const int* __restrict__ order,
                                                            double* __restrict__ out) {
    const int m = blockIdx.x, lane = threadIdx.x;
    const LedgerView s = ledger_view(state, K, E);
    const long steps = s.head[0];
    double* o = out + (size_t)m * 5;
    if (m == 0 && lane == 0) {                                     // the header rides along: one copy tells the host everything
        out[(size_t)(2 * K + 1 + E) * 5] = (double)steps;
        out[(size_t)(2 * K + 1 + E) * 5 + 1] = (double)s.head[1];
    }
    const int win = min(max(windows[m], 1), LG_D);                 // the entry point refuses anything else
    const int n = (int)(steps < (long)win ? steps : (long)win);
    if (n <= 0) {                                                  // an empty meter has no statistics
        if (lane < 5) o[lane] = NAN;
        return;
    }
    const float* rv = ring_override ? ring_override : s.ring_v;
    double xd = 0.0;
    if (lane < n) {
        const int row = (int)((steps - n + lane) % LG_D);
        const float* v = rv + (size_t)row * K;
        const float* w = s.ring_w + (size_t)row * K;
        if (m < K) xd = (double)v[m];
        else if (m < 2 * K) xd = (double)(v[m - K] * w[m - K]);
        else if (m == 2 * K) {
            float t = 0.0f;
            for (int q = 0; q < K; ++q) {
                const int k = order ? order[q] : q;
                if ((unsigned)k < (unsigned)K && s.mask[k]) t = t + v[k] * w[k];       // (a bad index is skipped, never followed)
            }
            xd = (double)t;
        } else xd = s.ring_e[(size_t)row * E + (m - 2 * K - 1)];
    }
    const float xf = (float)xd;                                    // the median is taken over a float32 tensor (misc.py:67)
    const bool anynan = __any(lane < n && xd != xd) != 0;
    int rank = 0;
    double sum = 0.0, mx = 0.0;
    for (int j = 0; j < n; ++j) {
        const float fj = __shfl(xf, j, 64);
        const double dj = __shfl(xd, j, 64);
        rank += (fj < xf || (fj == xf && j < lane)) ? 1 : 0;       // ties by position: a stable sort
        sum = sum + dj;                                            // in order, fp64
        if (j == 0 || dj > mx) mx = dj;                            // Python's max(): the first of equal maxima
    }
    const int want = (n - 1) / 2;                                  // torch.median: the lower median
    const unsigned long long hit = __ballot(lane < n && rank == want);
    const int src = hit ? (int)__builtin_ctzll(hit) : 0;
    const double med = (double)__shfl(xf, src, 64);
    const double newest = __shfl(xd, n - 1, 64);
    if (lane == 0) {
        o[0] = anynan ? (double)NAN : med;
        o[1] = (double)(float)(sum / (double)n);
        o[2] = s.totals[m] / (double)steps;
        o[3] = anynan ? (double)NAN : mx;
        o[4] = newest;
    }
}

static int ledger_args_ok(int K, int E) { return K >= 1 && K <= LG_MAXK && E >= 0 && E <= LG_MAXE; }

// C-ABI: see include/spe_hip.h (spe_ledger_*).
extern "C" int spe_ledger_state_bytes(int K, int E, size_t* bytes) {
    if (!ledger_args_ok(K, E) || !bytes) return -2;
    *bytes = ledger_bytes(K, E);
    return 0;
}

extern "C" int spe_ledger_record(const float* vals, const float* weights, const unsigned char* mask, const double* extras_host,
                                 int K, int E, void* state, size_t state_bytes, float* total, hipStream_t st) {
    if (!ledger_args_ok(K, E) || (E > 0 && !extras_host) || !vals || !weights || !mask || !total) return -2;
    if (!state || state_bytes < ledger_bytes(K, E) || ((uintptr_t)state & 7)) return -4;
    LedgerExtras ex;
    for (int i = 0; i < LG_MAXE; ++i) ex.e[i] = i < E ? extras_host[i] : 0.0;
    hipLaunchKernelGGL(ledger_record_kernel, dim3(1), dim3(LG_THREADS), 0, st, vals, weights, mask, ex, K, E, state, total);
    SPE_CHECK_LAUNCH();
    return 0;
}

extern "C" int spe_ledger_total_bwd(const float* g, const float* weights, const unsigned char* mask, int K, float* dvals,
                                    hipStream_t st) {
    if (K < 1 || K > LG_MAXK || !g || !weights || !mask || !dvals) return -2;
    hipLaunchKernelGGL(ledger_total_bwd_kernel, dim3(1), dim3(LG_THREADS), 0, st, g, weights, mask, K, dvals);
    SPE_CHECK_LAUNCH();
    return 0;
}

extern "C" int spe_ledger_summary(void* state, size_t state_bytes, int K, int E, const int* windows_host, const int* windows_dev,
                                  const float* ring_override, const int* order, double* out, hipStream_t st) {
    if (!ledger_args_ok(K, E) || !windows_host || !windows_dev || !out) return -2;
    const int M = 2 * K + 1 + E;
    for (int i = 0; i < M; ++i)
        if (windows_host[i] < 1 || windows_host[i] > LG_D) return -2;
    if (!state || state_bytes < ledger_bytes(K, E) || ((uintptr_t)state & 7)) return -4;
    hipLaunchKernelGGL(ledger_summary_kernel, dim3((unsigned)M), dim3(64), 0, st, state, K, E, windows_dev, ring_override, order, out);
    SPE_CHECK_LAUNCH();
    return 0;
}
