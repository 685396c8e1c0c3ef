"""Cases shared by test_adamw_ema_cpu.py and test_adamw_ema_gpu.py."""
GRID_CAP = 2048                     # workgroups of spe_adamw_flat(_guarded / _ema) at most; each sweeps 1024 elements per pass
SIZES = [1, 3, 4, 5, 255, 256, 1023, 1024, 1025, GRID_CAP * 1024 + 7]          # those of test_adamw_guard_gpu.py; the last one wraps the grid-stride

# (decay, warmup, t).  (1 + t) / (10 + t) first EXCEEDS decay at t = 44991 for 0.9998 (it equals it at 44990) and at t = 81 for 0.9.
TRIPLES = [
    (0.9998, True, 1), (0.9998, True, 5),                                   # warm-up active
    (0.9998, True, 44989), (0.9998, True, 44990), (0.9998, True, 44991),    # the crossover
    (0.9, True, 79), (0.9, True, 80), (0.9, True, 81),
    (0.9998, True, 10 ** 6),                                                # warm-up saturated
    (0.9998, False, 1), (0.9, False, 5),                                    # warm-up off
    (0.0, True, 1), (0.0, True, 10 ** 6), (0.0, False, 3),                  # decay = 0: w = 1, the EMA is the parameter
]

# w of the triples above as float32 bit patterns, worked out by hand from the contract (exact rationals, then one rounding each):
#   t = 1: 1 - 2/11 = 9/11;  t = 5: 1 - 6/15 = 0.6;  t = 79: 1 - 80/89 = 9/89;  t = 44989: 1 - 44990/44999 = 9/44999
WEIGHT_BITS = {
    (0.9998, True, 1): 0x3F51745D, (0.9998, True, 5): 0x3F19999A, (0.9998, True, 10 ** 6): 0x3951B717, (0.9998, False, 1): 0x3951B717,
    (0.9, True, 80): 0x3DCCCCCD, (0.9, True, 81): 0x3DCCCCCD, (0.9, False, 5): 0x3DCCCCCD,
    (0.0, True, 1): 0x3F800000, (0.0, True, 10 ** 6): 0x3F800000, (0.0, False, 3): 0x3F800000,
}

# the six-tensor, two-bucket (bucket_bytes=4096), two-group setup of test_adamw_guard_gpu.py
SHAPES = [(64, 32), (64,), (7, 5, 3), (1,), (300, 17), (33,)]
BETAS, EPS = (0.9, 0.999), 1e-8
