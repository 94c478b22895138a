"""The MXFP4 weight format of the decode step (include/merlin_hip.h "MXFP4 weight path", csrc/decode.hip) restated in torch, and the
float64 reference + bound of the GEMV that reads it (same structure as numerics.gemv_fp8w, 32-wide blocks).

Format: q uint8 [N, K/2], byte j of a row = element 2j in the low nibble and 2j + 1 in the high one; a code is s e e m with magnitudes
0, 0.5, 1, 1.5, 2, 3, 4, 6; scales uint8 [N, K/32] = e + 127, one power of two per 32 consecutive k.
Scale rule: e = the smallest integer with amax 2^-e <= 6 (amax = m 2^ex with m in [0.5, 1): e = ex - 3 if m <= 0.75 else ex - 2),
clamped to >= -126, 0 for an all-zero block.  Value rule: w 2^-e, exact in fp32, rounded to the nearest magnitude, a tie to the code whose
mantissa bit is 0."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(__file__))
import numerics as N  # noqa: E402

MAGNITUDES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
BLOCK = 32


def block_exponent(amax):
    """amax fp32 [...] >= 0 -> int e [...] by the rule above (torch.frexp: amax = m 2^ex, m in [0.5, 1), fp32 subnormals included)."""
    amax = amax.float().cpu()
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.75, ex - 3, ex - 2).clamp(min=-126)
    return torch.where(amax == 0, torch.zeros_like(e), e).to(torch.int32)


def round_e2m1(a):
    """a float64 [...] in [0, 6] -> code magnitude index [...] 0..7: the nearest of MAGNITUDES, a tie to the even index (mantissa bit 0)."""
    mags = torch.tensor(MAGNITUDES, dtype=torch.float64)
    d = (a.double()[..., None] - mags).abs()
    near = d == d.amin(-1, keepdim=True)
    even = torch.tensor([i % 2 == 0 for i in range(8)])
    near_even = near & even
    return torch.where(near_even.any(-1), near_even.to(torch.uint8).argmax(-1), near.to(torch.uint8).argmax(-1))


def quant(w):
    """w [N, K] (bf16 / fp16, K % 32 == 0) -> (q uint8 [N, K/2], scales uint8 [N, K/32]) on the CPU."""
    w = w.detach().cpu()
    Nr, K = w.shape
    assert K % BLOCK == 0
    wb = w.double().view(Nr, K // BLOCK, BLOCK)
    e = block_exponent(wb.abs().amax(-1).float())
    x = torch.ldexp(wb, -e[..., None])  # exact
    assert float(x.abs().max()) <= 6.0
    code = round_e2m1(x.abs()).to(torch.uint8) | (torch.signbit(wb).to(torch.uint8) << 3)
    code = code.view(Nr, K // 2, 2)
    return (code[..., 0] | (code[..., 1] << 4)).contiguous(), (e + 127).to(torch.uint8).contiguous()


def codes64(q):
    """q uint8 [N, K/2] -> float64 [N, K]: the e2m1 values without their block scales."""
    q = q.cpu()
    c = torch.stack([q & 15, q >> 4], dim=-1).view(q.shape[0], -1).long()
    mag = torch.tensor(MAGNITUDES, dtype=torch.float64)[c & 7]
    return torch.where((c & 8) != 0, -mag, mag)


def scales64(scales):
    """E8M0 bytes [N, K/32] -> float64 2^e."""
    return torch.ldexp(torch.ones(scales.shape, dtype=torch.float64), scales.cpu().to(torch.int32) - 127)


def dequant(q, scales):
    """(q, scales) -> float64 [N, K], exact."""
    return codes64(q) * scales64(scales).repeat_interleave(BLOCK, dim=1)


def _block_sums(X, Q):
    """X [M, K], Q [N, K] -> [M, N, K / 32]: the sum of x q over each 32-k block."""
    nb = X.shape[1] // BLOCK
    return torch.einsum("mbk,nbk->mnb", X.view(X.shape[0], nb, BLOCK), Q.view(Q.shape[0], nb, BLOCK))


def gemv_fp4w(x, q, scales, resid=None, *, out_dtype=None, model=None):
    """mh_gemv_fp4w: y[m, n] = sum_kb 2^e[n, kb] sum_{k in block kb} q[n, k] x[m, k] (+ resid), the scale applied to the block sum as the
    kernels do.  -> (ref64, B) for numerics.componentwise: the products of an e2m1 value and a 16-bit activation are exact (the kernels widen
    the codes to 16 bits and multiply in dot2 / MFMA instructions), the scales are powers of two and the sums are fp32, so as in numerics.gemm
    B = (sum_kb 2^e sum |q| |x| + |resid|) (sqrt(K) + 4) 2^-24 / eps(out).
    model=dtype: fp32 block sums, fp32 scale and add, ONE rounding at the store."""
    wt = torch.float64 if model is None else torch.float32
    od = x.dtype if out_dtype is None else out_dtype
    X, Q, S = x.detach().cpu().to(wt), codes64(q).to(wt), scales64(scales).to(wt)
    K = X.shape[1]
    acc = (_block_sums(X, Q) * S[None]).sum(-1)
    if resid is not None:
        acc = acc + resid.detach().cpu().to(wt)
    if model is not None:
        return N.r16(acc, None if od == torch.float32 else od)
    cond = (_block_sums(X.abs(), Q.abs()) * S[None]).sum(-1)
    if resid is not None:
        cond = cond + resid.detach().cpu().to(wt).abs()
    return acc, cond * ((math.sqrt(K) + 4) * N.EPS16[torch.float32] / N.EPS16[od])
