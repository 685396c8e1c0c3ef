"""Cases shared by test_grad_report_cpu.py and test_grad_report_gpu.py: parameter lengths and gradient value sets of spe_grad_report."""
import numpy as np

THREADS = 256                       # lanes of the workgroup that reduces one chunk of a parameter (csrc/grad_report.hip)
PASS_SPAN = 4 * THREADS             # elements one pass of that workgroup covers: a longer chunk wraps the lane-strided sweep
TRIP_PASSES = 4                     # passes the unrolled loop takes per trip; lane 0 enters it from (TRIP_PASSES - 1) * PASS_SPAN + 4 elements on
CHUNK = 16 * PASS_SPAN              # elements of one chunk: a longer parameter spreads over several workgroups, folded in chunk order
LENGTHS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257,
           PASS_SPAN - 1, PASS_SPAN, PASS_SPAN + 1,          # 1023, 1024, 1025: the last vector of a pass partial / full; one element into the second pass
           2 * PASS_SPAN + 5,                                # three passes, none of them through the unrolled loop
           TRIP_PASSES * PASS_SPAN - 1, TRIP_PASSES * PASS_SPAN, TRIP_PASSES * PASS_SPAN + 1,   # one unrolled trip (not for the last lane / for all / and a fifth pass)
           9 * PASS_SPAN + 1,                                # two trips and a ninth pass of one element
           CHUNK - 1, CHUNK, CHUNK + 1,                      # one chunk of four trips; a second chunk of one element
           2 * CHUNK + 5 * PASS_SPAN + 5]                    # three chunks, the last one partial
FOLD_TILE = 256                     # chunk records the folding workgroup stages per round
LONG_LENGTH = FOLD_TILE * CHUNK + 3 # 257 chunks: the fold wraps (one case of its own, 4.2 M elements)

# the six-tensor, two-bucket (bucket_bytes=4096), two-group setup of test_adamw_guard_gpu.py / test_adamw_ema_gpu.py
SHAPES = [(64, 32), (64,), (7, 5, 3), (1,), (300, 17), (33,)]
BETAS, EPS = (0.9, 0.999), 1e-8

BIG = 3e19                          # finite, its square (9e38) is beyond FLT_MAX = 3.4e38
NEAR = 1.3e19                       # its square (1.69e38) is finite, the sum of three is not
NAN, INF = float("nan"), float("inf")

VALUE_SETS = ["normal", "negzero_denormal", "zeros", "nan_first", "inf_last", "neginf_middle", "nan_then_inf", "inf_then_nan",
              "big_finite", "sum_overflow"]
# sets whose finite elements overflow the fp32 sum of squares (from the stated length on): no fp64 comparison there
OVERFLOWS = {"big_finite": 1, "sum_overflow": 3}


def grad_values(name, L, seed=0):
    """The gradient of one parameter of L elements, fp32."""
    rng = np.random.default_rng(1000 * VALUE_SETS.index(name) + L + seed)
    g = rng.standard_normal(L).astype(np.float32)
    mid = L // 2
    if name == "negzero_denormal":
        pool = np.array([-0.0, 0.0, 1e-40, -3e-42, 1.4e-45, -1.1754942e-38, 1e-20, -1e-19, 2.5], dtype=np.float32)
        g = pool[rng.integers(0, len(pool), L)]
        g[0] = np.float32(-0.0)
    elif name == "zeros":
        g[:] = 0.0
    elif name == "nan_first":
        g[0] = NAN
    elif name == "inf_last":
        g[L - 1] = INF
    elif name == "neginf_middle":
        g[mid] = -INF
    elif name == "nan_then_inf":                 # several non-finite elements: the first is a NaN (L = 1: that NaN alone)
        g[L - 1] = INF
        g[mid] = INF
        g[L // 3] = NAN
        if L > 8:
            g[L // 3 + 1] = -INF
            g[L - 2] = NAN
    elif name == "inf_then_nan":
        g[L - 1] = NAN
        g[mid] = NAN
        g[L // 3] = -INF
        if L > 8:
            g[L // 3 + 1] = NAN
    elif name == "big_finite":
        g[mid] = BIG if L % 2 else -BIG
    elif name == "sum_overflow":
        g = (NEAR * (1.0 + 0.01 * rng.standard_normal(L))).astype(np.float32) * rng.choice(np.float32([-1.0, 1.0]), L)
    return np.ascontiguousarray(g, dtype=np.float32)


def weight_values(L, seed=0):
    return np.random.default_rng(77 + L + seed).standard_normal(L).astype(np.float32)
