"""Data of the 16-bit operand conversion tests (tests/test_cvt16_gpu.py, tests/test_cvt16_ref_cpu.py): the geometry cases of
spe_cvt_bf16 / spe_cvt_bf16_h and the fp32 bit patterns every conversion is fed.  No project code is imported here.

A geometry case is a dict
  name, entry ("cvt" = spe_cvt_bf16, "h" = spe_cvt_bf16_h), R, C,
  ldx      row stride of x in floats (>= C),
  xoff     0: x starts at the allocation (16-byte aligned); 1: one float past a 16-byte boundary,
  off, ldo the row-major outputs are the column block [off, off + C) of a [R, ldo] matrix (off = 0 and ldo = C: a fresh tensor);
           both outputs share the geometry, as the entry points demand,
  ldt      row stride of the transposed copy (>= R),
  outputs  which of "out", "lo" (the low part; the fp16 copy for entry "h"), "T", "colsum" are passed (the others are NULL).
The tiles of cvt_bf16_tile (csrc/gemm_bf16.hip) are 64 x 64 with 16 row lanes and 16 column quads; every case stays inside the
contract of include/spe_hip.h (out / out_lo 8-byte aligned when ldo % 4 == 0, outT when ldt % 4 == 0) and is tiny."""
import itertools

import numpy as np

R_VALUES = (1, 15, 16, 17, 63, 64, 65, 129)
C_VALUES = (1, 3, 4, 5, 63, 64, 65, 67, 132)
MAX_ELEMS = 132 * 200


def rup(n, m):
    return (n + m - 1) // m * m


def _case(name, R, C, ldx=None, xoff=0, off=0, ldo=None, ldt=None, outputs=("out", "lo", "T"), entry="cvt"):
    return dict(name=name, entry=entry, R=R, C=C, ldx=C if ldx is None else ldx, xoff=xoff, off=off, ldo=C if ldo is None else ldo,
                ldt=R if ldt is None else ldt, outputs=tuple(outputs))


def _subsets(names):
    return [s for n in range(1, len(names) + 1) for s in itertools.combinations(names, n)]


CVT_OUTPUTS = ("out", "lo", "T", "colsum")
H_OUTPUTS = ("out", "lo", "T")          # spe_cvt_bf16_h has no column sum

GEOMETRY = []
# every R and every C once, everything contiguous: the vector paths wherever C % 4 == 0, and the ragged last quad / row lane
for R, C in ((1, 1), (15, 3), (16, 4), (17, 5), (63, 63), (64, 64), (65, 65), (129, 67), (1, 132), (129, 132)):
    GEOMETRY.append(_case("rc-%dx%d" % (R, C), R, C))
# the row stride and the base of x: ldx = C rounded up to 4, an odd ldx > C, a base one float past a 16-byte boundary
GEOMETRY += [
    _case("ldx-up4-17x5", 17, 5, ldx=8), _case("ldx-odd-17x5", 17, 5, ldx=7), _case("ldx-up4-65x67", 65, 67, ldx=68),
    _case("ldx-odd-65x67", 65, 67, ldx=69), _case("ldx-odd-64x64", 64, 64, ldx=65), _case("xoff-16x4", 16, 4, xoff=1),
    _case("xoff-65x132", 65, 132, xoff=1), _case("xoff-ldx-up4-63x63", 63, 63, ldx=64, xoff=1), _case("xoff-ldx-odd-15x3", 15, 3, ldx=5, xoff=1),
]
# the row-major outputs as a column block at offset 0, 4 or 64 of a wider matrix (ldo % 4 == 0), and with an odd ldo
GEOMETRY += [
    _case("block0-65x64", 65, 64, off=0, ldo=200), _case("block4-65x5", 65, 5, off=4, ldo=16), _case("block64-17x67", 17, 67, off=64, ldo=136),
    _case("block64-64x64", 64, 64, off=64, ldo=128), _case("block4-129x4", 129, 4, off=4, ldo=12), _case("block4-63x132", 63, 132, off=4, ldo=140),
    _case("oddldo-17x5", 17, 5, ldo=7), _case("oddldo-65x64", 65, 64, ldo=67), _case("oddldo-16x4", 16, 4, ldo=5),
    _case("oddldo-63x132", 63, 132, ldo=133),
]
# the transposed copy: ldt = R rounded up to 64, R + 1, R + 3, R + 68 (one whole padding tile and a partial one)
for R, C in ((1, 5), (17, 64), (64, 4), (65, 65)):
    for tag, ldt in (("up64", rup(R, 64)), ("+1", R + 1), ("+3", R + 3), ("+68", R + 68)):
        GEOMETRY.append(_case("ldt%s-%dx%d" % (tag, R, C), R, C, ldt=ldt))
# every subset of the outputs, on one geometry with all the fall-back paths at once
for s in _subsets(CVT_OUTPUTS):
    GEOMETRY.append(_case("subset-ragged-" + "+".join(s), 65, 67, ldx=69, xoff=1, off=4, ldo=76, ldt=65 + 68, outputs=s))
GEOMETRY.append(_case("all-vector-64x64", 64, 64, ldt=64, outputs=CVT_OUTPUTS))
# spe_cvt_bf16_h: every subset, and the edges again with the fp16 second copy
for s in _subsets(H_OUTPUTS):
    GEOMETRY.append(_case("h-subset-" + "+".join(s), 17, 64, ldt=64, outputs=s, entry="h"))
GEOMETRY += [
    _case("h-rc-65x65", 65, 65, entry="h"), _case("h-rc-129x132", 129, 132, entry="h"), _case("h-xoff-63x63", 63, 63, ldx=64, xoff=1, entry="h"),
    _case("h-block4-65x5", 65, 5, off=4, ldo=16, entry="h"), _case("h-block64-17x67", 17, 67, off=64, ldo=136, ldt=17 + 68, entry="h"),
    _case("h-oddldo-65x64", 65, 64, ldo=67, ldt=65 + 3, entry="h"), _case("h-ldx-odd-1x132", 1, 132, ldx=133, ldt=64, entry="h"),
]

# the column sum on finite data (R, C, ldt or None): every R / C of the issue, and ldt > R + 64 so that padding tiles exist and add nothing
COLSUM = [(R, C, None) for R in (1, 63, 64, 65, 129, 200) for C in (5, 64, 132)] + [(1, 5, 1 + 68), (65, 64, 65 + 68), (129, 132, 129 + 68), (63, 67, 63 + 130)]

# the activation backward folded into the read (act, R, C, ldx): aux shares ldx with x, ldx > C
ACT = [(1, 17, 64, 68), (1, 65, 67, 69), (2, 65, 67, 69), (2, 64, 132, 136), (2, 129, 5, 7)]

# spe_cvt_f16 (R, C, ldx, ldo)
F16 = [(R, C, C + dx, C + do) for R in (1, 7, 300) for C, dx, do in ((4, 4, 8), (8, 0, 4), (132, 8, 0), (132, 4, 12))]

# ---- values -------------------------------------------------------------------------------------------------------------------------
def _f32_bits(v):
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


NAMED = {
    "zero": [0x00000000, 0x80000000],
    # exact ties between bf16 neighbours: lower neighbour even (0x3F80) and odd (0x3F81), and one ulp either side of each
    "tie_even": [0x3F808000, 0xBF808000], "tie_odd": [0x3F818000, 0xBF818000],
    "tie_ulp": [0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0xBF807FFF, 0xBF808001],
    "bf16_max": [0x7F7F0000, 0xFF7F0000, 0x7F7F7FFF],
    "to_inf": [0x7F7F8000, 0xFF7F8000, 0x7F7FFFFF, 0xFF7FFFFF],            # the first fp32 that rounds to bf16 infinity, and FLT_MAX
    "inf": [0x7F800000, 0xFF800000],
    "nan": [0x7FC00000, 0xFFC00001],
    "f16_sat": [_f32_bits(v) for v in (65504.0, 65519.99, 65520.0, 1e9, -65504.0, -65519.99, -65520.0, -1e9)],
    # fp16 subnormal range (below 2^-14 = 6.10e-5), its ties (2^-25, 3 x 2^-25) and the underflow to zero
    "f16_sub": [_f32_bits(v) for v in (6.1e-5, 6.0e-8, 2.9e-8, 1e-10, -6.1e-5, -6.0e-8, -2.9e-8, -1e-10, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14,
                                       2.0 ** -14 - 2.0 ** -26)],
    "f32_sub": [0x00000001, 0x00008000, 0x00018000, 0x00400000, 0x007FFFFF, 0x80000001, 0x80008000, 0x807FFFFF],
}


def _random_bits(n=4096, seed=0xC7716):
    """n patterns from a seeded integer generator: exponent field i % 256 (every exponent 16 times), random sign and mantissa."""
    g = np.random.Generator(np.random.PCG64(seed))
    sign = g.integers(0, 2, n, dtype=np.int64) << 31
    man = g.integers(0, 1 << 23, n, dtype=np.int64)
    exp = (np.arange(n, dtype=np.int64) % 256) << 23
    return [int(v) for v in (sign | exp | man)]


RANDOM_BITS = _random_bits()
VALUE_BITS = [b for k in NAMED for b in NAMED[k]] + RANDOM_BITS


def is_f32_subnormal(b):
    return (b & 0x7F800000) == 0 and (b & 0x007FFFFF) != 0


def is_finite_moderate(b):
    """Finite, not an fp32 subnormal, magnitude below 2^40: what a column sum test may add up without overflow."""
    e = (b >> 23) & 0xFF
    return (e == 0 and (b & 0x007FFFFF) == 0) or 0 < e < 127 + 40


# the conversions' main value list leaves the fp32 subnormals to their own named case (the device may flush them)
MAIN_BITS = [b for b in VALUE_BITS if not is_f32_subnormal(b)]
SUBNORMAL_BITS = [b for b in VALUE_BITS if is_f32_subnormal(b)]
FINITE_BITS = [b for b in VALUE_BITS if is_finite_moderate(b)]
