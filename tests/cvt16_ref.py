"""Host restatement of the 16-bit operand conversions (include/spe_hip.h: spe_cvt_bf16, spe_cvt_bf16_h, spe_cvt_bf16_multi, spe_cvt_f16):
the definitions the GPU tests of tests/test_cvt16_gpu.py compare the kernels with, bit for bit.  Plain torch and numpy on the CPU, no
project code is imported here.

Both roundings are written on the integer pattern of the fp32 value and NOT with tensor.to(bfloat16) / tensor.half(), so that
tests/test_cvt16_ref_cpu.py can check one against the other.  16-bit results are raw patterns in int16 tensors; a NaN result is the
canonical quiet NaN of the format (the tests compare NaNs by position, never by payload)."""
import math

import numpy as np
import torch

BF16_NAN = 0x7FC0
F16_NAN = 0x7E00
F16_MAX_F32_BITS = 0x477FE000            # 65504.0f


def _u32(x):
    """fp32 tensor -> its bit patterns as non-negative int64 (same shape)."""
    assert x.dtype == torch.float32
    return x.detach().cpu().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def _to_i16(p):
    """int64 patterns 0 .. 0xFFFF -> int16 tensor with the same bits."""
    return torch.where(p >= 0x8000, p - 0x10000, p).to(torch.int16)


def bits_to_f32(u):
    """int64 / int32 bit patterns -> fp32 tensor."""
    u = torch.as_tensor(u, dtype=torch.int64) & 0xFFFFFFFF
    return torch.where(u >= 0x80000000, u - 0x100000000, u).to(torch.int32).view(torch.float32)


def bf16_bits_to_f32(b):
    """int16 bf16 patterns -> the fp32 values they stand for (exact)."""
    return bits_to_f32((b.to(torch.int64) & 0xFFFF) << 16)


def is_nan16(b, fmt):
    """Positions of NaN patterns in an int16 tensor of bf16 (fmt 'bf16') or fp16 ('f16') patterns."""
    p = b.to(torch.int64) & 0x7FFF
    return p > (0x7F80 if fmt == "bf16" else 0x7C00)


def bf16_rne_bits(x):
    """bf16(x), round to nearest even, on the uint32 pattern: add 0x7FFF + (bit 16), shift right by 16.  NaN -> quiet NaN."""
    u = _u32(x)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return _to_i16(torch.where(nan, (u >> 16) & 0x8000 | BF16_NAN, r))


def lo_bits(x):
    """The low part of the split operand: bf16(x - float(bf16(x))).  The subtraction is exact in fp32 (Sterbenz / the difference has at
    most 16 significant bits); inf - inf = NaN and finite - inf = -inf fall out of the same expression."""
    hi = bf16_bits_to_f32(bf16_rne_bits(x))
    return bf16_rne_bits(x.detach().cpu() - hi)


def f16_sat_bits(x):
    """IEEE fp16 of clamp(x, -65504, 65504), round to nearest even, subnormals kept, NaN kept - in integer arithmetic."""
    u = _u32(x).numpy()
    sign = (u >> 16) & 0x8000
    a = u & 0x7FFFFFFF
    nan = a > 0x7F800000
    a = np.minimum(a, F16_MAX_F32_BITS)                         # the clamp: the patterns of non-negative floats order like the floats
    # normal results (|x| >= 2^-14): rebias the exponent, round 13 mantissa bits away (65504 is exact: no carry into infinity)
    rn = a - (112 << 23)
    normal = (rn + 0xFFF + ((rn >> 13) & 1)) >> 13
    # subnormal results: |x| = m 2^(e - 150) in units of 2^-24 is m >> (126 - e); 25 or more bits away is less than half a unit
    e = a >> 23
    m = np.where(e > 0, (a & 0x7FFFFF) | 0x800000, 0)
    sh = np.clip(126 - e, 14, 25)
    q = m >> sh
    rem = m & ((np.int64(1) << sh) - 1)
    half = np.int64(1) << (sh - 1)
    sub = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    mag = np.where(a >= 0x38800000, normal, sub)
    out = np.where(nan, sign | F16_NAN, sign | mag)
    return _to_i16(torch.from_numpy(out.astype(np.int64)))


def transposeT(bits, ldt):
    """[R, C] patterns -> the zero-padded transpose [C, ldt]: columns R .. ldt-1 are zero."""
    R, C = bits.shape
    assert ldt >= R
    out = torch.zeros((C, ldt), dtype=bits.dtype)
    out[:, :R] = bits.t()
    return out


def untransposeT(bitsT, R):
    """-> ([R, C] patterns, the padding columns [C, ldt - R])."""
    return bitsT[:, :R].t().contiguous(), bitsT[:, R:]


def colsum64(x):
    """fp64 column sums of an fp32 [R, C]."""
    return x.detach().cpu().double().sum(0)


def gelu_grad64(h):
    """d/dh of the exact-erf GELU, h Phi(h): Phi(h) + h phi(h), in fp64."""
    h = h.double()
    return 0.5 * (1.0 + torch.erf(h * (1.0 / math.sqrt(2.0)))) + h * torch.exp(-0.5 * h * h) * (1.0 / math.sqrt(2.0 * math.pi))


def act_bwd64(x, aux, act):
    """x * act'(aux) in fp64: act 1 = ReLU (aux > 0, so both zeros switch the element off), act 2 = exact-erf GELU."""
    x, aux = x.detach().cpu().double(), aux.detach().cpu().double()
    if act == 1:
        return x * (aux > 0).double()
    assert act == 2
    return x * gelu_grad64(aux)


def gelu_bwd_f32_formula(x, aux):
    """The kernels' own formula x * (cdf + h * pdf) evaluated in fp32 with torch.erf / torch.exp on the host: what the interval of the
    GELU test is measured from (delta = 4 x its worst |fp32 - fp64| / |x|)."""
    x, h = x.detach().cpu().float(), aux.detach().cpu().float()
    cdf = 0.5 * (1.0 + torch.erf(h * 0.70710678118654752))
    pdf = 0.3989422804014327 * torch.exp(-0.5 * h * h)
    return x * (cdf + h * pdf)
