"""CPU restatement of the two bf16 parameter stores of mh_adamw_split / mh_adamw_sr (include/merlin_hip.h, optimizer section), on integer
bit patterns, for tests/test_adamw_rounding_cpu.py and tests/test_adamw_rounding_gpu.py.  Works on tensors of any device."""
import numpy as np
import torch

from merlin_amd.weights import MASK64, _splitmix64_np, splitmix64_scalar

M32 = 0xFFFFFFFF


def f32_bits(x):
    """fp32 tensor -> its bit patterns as non-negative int64."""
    assert x.dtype == torch.float32
    return x.contiguous().view(torch.int32).to(torch.int64) & M32


def bits_f32(u):
    """int64 bit patterns (mod 2^32) -> fp32 tensor."""
    u = u & M32
    return ((u ^ 0x80000000) - 0x80000000).to(torch.int32).view(torch.float32)


def _u16_to_bf16(h):
    return ((h ^ 0x8000) - 0x8000).to(torch.int16).view(torch.bfloat16)


def bf16_bits(p):
    assert p.dtype == torch.bfloat16
    return p.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def split_bits(master):
    """fp32 master -> (p bf16, lo int16): hi = (u + 0x8000) >> 16 (round to nearest, ties away from zero), lo = u - (hi << 16)."""
    u = f32_bits(master)
    hi = ((u + 0x8000) & M32) >> 16
    lo = (u - (hi << 16)) & 0xFFFF
    return _u16_to_bf16(hi), ((lo ^ 0x8000) - 0x8000).to(torch.int16)


def join_bits(p, lo):
    """(p bf16, lo int16) -> the fp32 master with bits (p << 16) + lo (mod 2^32)."""
    assert lo.dtype == torch.int16
    return bits_f32((bf16_bits(p) << 16) + lo.to(torch.int64))


def sr_key(seed, step):
    """FusedAdamW(rounding="stochastic", seed=seed): the hash key of its step number `step` (1-based)."""
    return splitmix64_scalar((seed & MASK64) ^ ((step * 0xD1342543DE82EF95) & MASK64))


def sr_fields(n, key, index0):
    """The 16-bit random field of each of n elements from arena index index0: field (j & 3) of splitmix64(key + (j >> 2)).  int64 numpy."""
    j = np.arange(index0, index0 + n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = _splitmix64_np(np.uint64(key) + (j >> np.uint64(2)))
    return ((z >> (np.uint64(16) * (j & np.uint64(3)))) & np.uint64(0xFFFF)).astype(np.int64)


def sr_store(values, key, index0):
    """fp32 values -> bf16 (u + r) >> 16; exponent field 255 truncated."""
    u = f32_bits(values)
    r = torch.from_numpy(sr_fields(values.numel(), key, index0)).to(u.device).view(u.shape)
    special = (u & 0x7F800000) == 0x7F800000
    return _u16_to_bf16(torch.where(special, u, u + r) >> 16)


def nearest_store(values):
    """What adamw_k does today: round to nearest even."""
    return values.to(torch.bfloat16)


def bf16_floor(x):
    """Largest bf16-representable value <= x (fp32 tensor, finite), as fp32."""
    u = f32_bits(x)
    t = u & 0xFFFF0000
    return bits_f32(torch.where((u >> 31 == 1) & (u != t), t + 0x10000, t))  # negative and inexact: one step up in magnitude


def bf16_ceil(x):
    return -bf16_floor(-x)


def bf16_spacing(x):
    """Distance between the two bf16 neighbours of |x| (x's own binade), as float64."""
    t = f32_bits(x) & 0x7FFF0000
    return bits_f32(t + 0x10000).double() - bits_f32(t).double()
