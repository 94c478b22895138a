"""CPU restatement of the compact AdamW moments of mh_adamw_compact (include/merlin_hip.h, optimizer section) on integer bit patterns and an
explicit table of the e4m3 grid, for tests/test_adamw_compact_cpu.py and tests/test_adamw_compact_gpu.py, and a small numpy AdamW simulator
on synthetic gradient streams that measures what the format costs.  numpy throughout: device tensors come here through .cpu().numpy()."""
import math

import numpy as np

from merlin_amd.weights import MASK64, _splitmix64_np, splitmix64_scalar

BLOCK = 128
E4M3_MAX = 448.0


def _e4m3_value(code):
    e, f = (code >> 3) & 15, code & 7
    return f * 2.0 ** -9 if e == 0 else (1 + f / 8) * 2.0 ** (e - 7)


# the 127 non-negative finite e4m3 magnitudes, by code 0x00 .. 0x7E (0x7F is NaN): 0, 2^-9 .. 7 * 2^-9 (subnormal), 2^-6 .. 448
E4M3 = np.array([_e4m3_value(c) for c in range(127)], dtype=np.float64)


def state_key(seed, step):
    """FusedAdamW(states="compact", seed=seed): the moments' hash key of step number `step` (1-based)."""
    return splitmix64_scalar((seed & MASK64) ^ ((step * 0xA0761D6478BD642F) & MASK64))


def state_fields(n, key, index0):
    """(r_v, r_m) of each of n elements from arena index index0: element j takes the 32-bit half (j & 1) of splitmix64(key + (j >> 1)); r_v is
    its low 16 bits, r_m its high 16.  int64 numpy."""
    j = np.arange(index0, index0 + n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = _splitmix64_np(np.uint64(key) + (j >> np.uint64(1)))
    half = (z >> (np.uint64(32) * (j & np.uint64(1)))) & np.uint64(0xFFFFFFFF)
    return (half & np.uint64(0xFFFF)).astype(np.int64), (half >> np.uint64(16)).astype(np.int64)


def scale_exp(amax):
    """e of one block maximum (fp32 array, >= 0): the smallest integer with amax * 2^-e <= 448, e >= -126, 0 for amax = 0 (mh_kv8_fill's rule)."""
    amax = np.asarray(amax, dtype=np.float32).astype(np.float64)
    m, ex = np.frexp(amax)  # amax = m * 2^ex, m in [0.5, 1)
    e = np.maximum(np.where(m <= 0.875, ex - 9, ex - 8), -126)
    return np.where(amax == 0, 0, e).astype(np.int64)


def _blocks(x, fill):
    """[n] -> [ceil(n / 128), 128], the last block padded with `fill`."""
    nb = -(-x.size // BLOCK)
    out = np.full(nb * BLOCK, fill, dtype=x.dtype)
    out[: x.size] = x
    return out.reshape(nb, BLOCK)


def m_prob_up(y):
    """For y = |m'| * 2^-e in [0, 448] (float64 array holding fp32 values): (index of lo in E4M3, 65536 t).  y = 448 has no successor: t = 0."""
    idx = np.searchsorted(E4M3, y, side="right") - 1
    lo = E4M3[idx]
    hi = E4M3[np.minimum(idx + 1, 126)]
    t = np.where(hi > lo, (y - lo) / np.where(hi > lo, hi - lo, 1.0), 0.0)  # exact: y - lo has at most 20 bits under the spacing
    return idx, 65536.0 * t


def m_code(y, r_m):
    """The e4m3 magnitude byte of y under the 16-bit field r_m: hi when r_m < 65536 t, else lo."""
    idx, t16 = m_prob_up(np.asarray(y, dtype=np.float64))
    return idx + (np.asarray(r_m) < t16)


def v_bits(u, r_v):
    """bf16 bit pattern of the fp32 bit pattern u under the 16-bit field r_v: (u + r_v) >> 16; exponent field 255 truncated."""
    u = np.asarray(u, dtype=np.int64)
    return (np.where((u & 0x7F800000) == 0x7F800000, u, u + r_v) >> 16).astype(np.uint16)


def m_store(m, key, index0):
    """fp32 m' [n] from arena index index0 (a multiple of 128) -> (e4m3 bytes uint8 [n], scale bytes uint8 [ceil(n / 128)])."""
    m = np.ascontiguousarray(m, dtype=np.float32)
    assert index0 % BLOCK == 0 and m.ndim == 1
    n = m.size
    e = scale_exp(np.abs(_blocks(m, np.float32(0))).max(axis=1))
    inv = np.ldexp(np.float32(1), -e).astype(np.float32)  # 2^-e, a normal fp32 for e in [-126, 120]
    y = (np.abs(_blocks(m, np.float32(0))) * inv[:, None]).astype(np.float32).reshape(-1)[:n].astype(np.float64)  # the fp32 product
    assert float(y.max(initial=0.0)) <= E4M3_MAX
    code = m_code(y, state_fields(n, key, index0)[1])
    sign = (m.view(np.uint32) >> np.uint32(24)) & np.uint32(0x80)
    return (code.astype(np.uint32) | sign).astype(np.uint8), (e + 127).astype(np.uint8)


def m_decode(codes, scales):
    """(e4m3 bytes [n], scale bytes) -> fp32 [n]: code * 2^e, exact."""
    codes = np.asarray(codes, dtype=np.uint8)
    n = codes.size
    e = np.repeat(np.asarray(scales, dtype=np.int64)[: -(-n // BLOCK)] - 127, BLOCK)[:n]
    mag = np.ldexp(E4M3[np.minimum(codes & 0x7F, 126)], e)
    out = np.where(codes & 0x80, -mag, mag)
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)  # exact in fp32
    return out.astype(np.float32)


def v_store(v, key, index0):
    """fp32 v' [n] -> bf16 bit patterns uint16 [n]: (u + r_v) >> 16; exponent field 255 truncated (mh_adamw_sr's store)."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.int64)
    return v_bits(u, state_fields(u.size, key, index0)[0])


def v_decode(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def pack(m, v, key, index0):
    """-> (m8, mscale, v16 bits)."""
    m8, ms = m_store(m, key, index0)
    return m8, ms, v_store(v, key, index0)


def unpack(m8, mscale, v16):
    return m_decode(m8, mscale), v_decode(v16)


# ---- simulator -----------------------------------------------------------------------------------------------------------------------------
def stream(n, steps, decades, seed, drop_at=None, drop=1e-3):
    """A synthetic gradient stream [steps, n] (fp32): element i is mu_i + sigma_i * N(0, 1) with sigma_i log-uniform over `decades` decades
    below 1e-4 and mu_i / sigma_i drawn from {0, 0.1, 1}; from step `drop_at` (1-based) on everything is scaled by `drop`."""
    rng = np.random.default_rng(seed)
    sig = 10.0 ** rng.uniform(-4 - decades, -4, n)
    mu = sig * rng.choice([0, 0.1, 1.0], n)
    g = mu + sig * rng.standard_normal((steps, n))
    if drop_at is not None:
        g[drop_at - 1:] *= drop
    return g.astype(np.float32)


def simulate(g, m_mode="e4m3", v_mode="sr", seed=0, b1=0.9, b2=0.999, eps=1e-8):
    """AdamW's update direction u_t = (m / bc1) / (sqrt(v / bc2) + eps) on the stream g [steps, n], once with fp32 moments and once with stored
    moments (m_mode "fp32" | "e4m3"; v_mode "fp32" | "sr" | "nearest": bf16 by stochastic rounding or to nearest even), the update taken from
    the unrounded moments as the kernel does.  The moment recurrences run in fp32 in adamw_value's operation order.  -> dict:
      step_rms   sqrt(sum |u_q - u|^2 / sum |u|^2) over all steps and elements
      acc_l1     sum_i |sum_t u_q - sum_t u| / sum_i sum_t |u|
      acc_l2     || sum_t u_q - sum_t u ||_2 / || sum_t u ||_2
      v_mean, vq_mean   [steps] mean over the elements of the fp32 and of the stored v after each step
      v_rel      [steps] mean over the elements of stored v / fp32 v - 1"""
    steps, n = g.shape
    f = np.float32
    c1, c2 = f(b1), f(b2)
    d1, d2 = f(1) - c1, f(1) - c2
    m = np.zeros(n, f)
    v = np.zeros(n, f)
    mq, vq = m.copy(), v.copy()
    su, suq, sa = np.zeros(n), np.zeros(n), np.zeros(n)
    err2 = ref2 = 0.0
    v_mean, vq_mean, v_rel = np.zeros(steps), np.zeros(steps), np.zeros(steps)
    for t in range(1, steps + 1):
        gt = g[t - 1]
        m, v = c1 * m + d1 * gt, c2 * v + d2 * gt * gt
        mq, vq = c1 * mq + d1 * gt, c2 * vq + d2 * gt * gt
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        u = (m.astype(np.float64) / bc1) / (np.sqrt(v.astype(np.float64) / bc2) + eps)
        uq = (mq.astype(np.float64) / bc1) / (np.sqrt(vq.astype(np.float64) / bc2) + eps)
        su += u
        suq += uq
        sa += np.abs(u)
        err2 += float(((uq - u) ** 2).sum())
        ref2 += float((u ** 2).sum())
        key = state_key(seed, t)
        if m_mode == "e4m3":
            mq = m_decode(*m_store(mq, key, 0))
        if v_mode == "sr":
            vq = v_decode(v_store(vq, key, 0))
        elif v_mode == "nearest":
            u32 = vq.view(np.uint32).astype(np.int64)
            vq = v_decode(((u32 + 0x7FFF + ((u32 >> 16) & 1)) >> 16).astype(np.uint16))
        v_mean[t - 1], vq_mean[t - 1] = v.astype(np.float64).mean(), vq.astype(np.float64).mean()
        v_rel[t - 1] = (vq.astype(np.float64) / np.where(v > 0, v, 1).astype(np.float64) - (v > 0)).mean()
    return dict(step_rms=math.sqrt(err2 / ref2), acc_l1=float(np.abs(suq - su).sum() / sa.sum()),
                acc_l2=float(np.linalg.norm(suq - su) / np.linalg.norm(su)), v_mean=v_mean, vq_mean=vq_mean, v_rel=v_rel)
