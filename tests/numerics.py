"""Per-element error bounds for the kernel tests: fp64 references with their condition magnitudes, rounding models, and the checker.

A kernel output `got` is held to

    |got - ref64| <= c * (eps16 * (|ref64| + B) + tiny)            for every element,

where ref64 is the operation evaluated in float64 from the 16-bit inputs, B is its condition magnitude (the same sums with the terms in
absolute value: what one rounding of an operand or of a partial sum can move the result by, in units of eps16), eps16 the unit roundoff of
the output type (EPS16) and tiny the absolute rounding floor of that type (TINY: half the subnormal spacing; where the reference is exactly
zero AND B is zero the output must be exactly zero, asserted separately).  One large element no longer sets the scale of a whole tensor.

The LIMIT on c never comes from a kernel.  Every operation has a ROUNDING MODEL here (`model=dtype`): the same reference evaluated in fp32
with the intermediates rounded to the 16-bit type where the kernels hold 16-bit MFMA operands (include/merlin_hip.h and the kernel
comments: P before P V and P^T dO, dS before dS K and dS^T Q, o as stored before delta, and every stored output).  A test evaluates the
model on ITS OWN inputs, measures the model's c (`c_model`) and allows `limit(c_model) = max(2, 2 * c_model)`: the factor 2 covers a
different summation order (MFMA tiles, split-K, online softmax) and the exp2-based softmax of the kernels, both of which move a result by
about as much again as the roundings the model performs; the floor of 2 is two roundings of the output type.

Measured c, worst over the shapes of tests/test_componentwise_gpu.py and tests/test_entry_points_gpu.py on an MI355X (the model evaluated with torch on
the same inputs in the same run; on the CPU shapes of tests/test_numerics_cpu.py the models score the same to two digits):

    operation                         bf16 model  bf16 kernel   fp16 model  fp16 kernel
    --------------------------------  ----------  -----------   ----------  -----------
    accumulate, 4-wave staged              0.984        0.984        0.971        0.971
    adamw m                                0.861        0.861        1.045        1.045
    adamw p                                0.996        0.996        0.995        0.995
    adamw v                                2.178        2.178        2.727        2.727
    add                                    0.996        0.996        1.000        1.000
    attention decode                       0.394        0.331        0.465        0.327
    attention dk 5-product                 0.726        0.726        0.939        0.939
    attention dk 7-product                 0.726        0.726        0.969        0.969
    attention dq 5-product                 0.361        0.361        0.322        0.322
    attention dq 7-product                 0.425        0.425        0.384        0.384
    attention dv 5-product                 0.781        0.781        0.919        0.919
    attention dv 7-product                 0.874        0.874        0.919        0.919
    attention o (3 forward forms)          0.729        0.729        0.732        0.732
    ce gradient                            0.996        0.996        1.000        1.000
    conv3x3 col2im                         0.996        0.996        0.998        0.998
    gemm 16-bit store, all epilogues       0.995        0.995        0.994        0.994
    gemm fp32 store                        0.182        0.134        0.389        0.143
    gemm split-K + epilogue                0.976        0.976        0.897        0.897
    gemm+gelu act                          1.008        1.008        0.991        0.991
    gemm+gelu bwd                          0.951        0.951        0.999        0.999
    gemm+gelu f1                           0.993        0.993        0.992        0.992
    gemm+rope                              0.990        0.990        0.980        0.980
    gemm+swiglu act                        0.966        0.966        0.996        0.996
    gemm+swiglu bwd                        0.977        0.977        0.999        0.999
    gemm+swiglu gu                         0.995        0.995        0.988        0.988
    gemv 16-bit                            0.992        0.992        0.981        0.981
    gemv fp32                              0.112        0.044        0.192        0.043
    gemv fp8w 16-bit                       0.993        0.993        0.982        0.982
    gemv fp8w fp32                         0.042        0.057        0.080        0.062
    layernorm db                           0.222        0.222        0.221        0.221
    layernorm dw                           0.315        0.315        0.279        0.279
    layernorm dx                           0.441        0.441        0.445        0.445
    layernorm y                            0.498        0.498        0.500        0.500
    quick-gelu bwd                         0.996        0.996        0.999        0.999
    quick-gelu fwd                         0.996        0.996        0.997        0.997
    reduce_partials                        0.980        0.980        0.980        0.980
    reduce_partials (fp32 out)             0.252        0.252          nan          nan
    rmsnorm dw                             0.453        0.453        0.422        0.422
    rmsnorm dx                             0.496        0.496        0.497        0.497
    rmsnorm y                              0.996        0.996        0.999        0.999
    rope fwd / inverse                     1.274        1.274        1.479        1.471
    swiglu bwd                             0.996        0.998        0.999        0.999
    swiglu fwd                             0.996        0.996        0.999        0.999
    wgrad split-K 16-bit                   0.995        0.995        0.992        0.992
    wgrad split-K fp32                     0.131        0.109        0.336        0.131

(Model and kernel mostly agree to three digits: the worst element is one whose error is the rounding of the output itself, and both round the
same fp32 value.  Where the summation order matters - decode attention, fp32 stores - they differ.)

(The two "gemv fp8w" rows: fp8 weights with per-128-block scales, worst over every arm of mh_gemv_fp8w and the shapes of
tests/test_fp8_componentwise_gpu.py, 16-bit stores with and without a residual.)

Structured softmax rows (tests/attn_inputs.py; tests/test_attention_structured_gpu.py), measured on an MI355X on 2026-10-19, worst over the
three prefill shapes, the forward forms 0 / 1 / 2, the fused-kv modes 0 / 1 / 2 and, for the cache kernels, over every placement and arm
(16-bit and fp8 cache, merge launch / fused merge / one block).  F3 = the one-hot placements together, F4 = the sink with its two shifted
copies.  A one-hot row's o IS a row of v and its dS cancels to nothing, so model and kernel both score 0.000 there: what those rows can show
is a wrong reference or weight, which scores in the thousands (tests/test_attention_structured_cpu.py).  lse is held to
|lse - lse64| <= c 2^-24 (|lse64| + A_row + 1) (`lse_c`), its model being fp32 scores and an fp32 logsumexp (`attention_lse_model`):

    operation                         bf16 model  bf16 kernel   fp16 model  fp16 kernel
    --------------------------------  ----------  -----------   ----------  -----------
    F1 attention o                         0.626        0.750        0.653        0.653
    F1 attention lse                       1.663        1.580        2.562        1.482
    F1 attention dq 7-product              0.403        0.403        0.319        0.302
    F1 attention dq 5-product              0.284        0.284        0.263        0.263
    F1 attention dk 7-product              0.423        0.423        0.559        0.559
    F1 attention dk 5-product              0.348        0.320        0.328        0.296
    F1 attention dv 7-product              0.835        0.835        0.777        0.777
    F1 attention dv 5-product              0.835        0.835        0.651        0.651
    F2 attention o                         0.574        0.574        0.608        0.608
    F2 attention lse                       1.663        1.580        1.662        1.482
    F2 attention dq 7-product              0.344        0.344        0.299        0.299
    F2 attention dq 5-product              0.284        0.284        0.263        0.263
    F2 attention dk 7-product              0.556        0.556        0.857        0.857
    F2 attention dk 5-product              0.484        0.484        0.118        0.118
    F2 attention dv 7-product              0.871        0.871        0.970        0.970
    F2 attention dv 5-product              0.871        0.871        0.268        0.268
    F3 attention o                         0.000        0.000        0.000        0.000
    F3 attention lse                       3.251        2.100        6.649        2.054
    F3 attention dq 7-product              0.000        0.000        0.000        0.000
    F3 attention dq 5-product              0.000        0.000        0.000        0.000
    F3 attention dk 7-product              0.328        0.328        0.000        0.000
    F3 attention dk 5-product              0.277        0.277        0.000        0.000
    F3 attention dv 7-product              0.731        0.731        0.164        0.164
    F3 attention dv 5-product              0.662        0.662        0.088        0.088
    F4 attention o                         0.471        0.471        0.897        0.897
    F4 attention lse                       9.939        2.866        8.169        3.793
    F4 attention dq 7-product              0.003        0.003        0.021        0.021
    F4 attention dq 5-product              0.003        0.003        0.021        0.021
    F4 attention dk 7-product              0.324        0.324        0.975        0.975
    F4 attention dk 5-product              0.252        0.252        0.960        0.960
    F4 attention dv 7-product              0.782        0.782        0.972        0.972
    F4 attention dv 5-product              0.661        0.661        0.914        0.914
    placed one-hot key, all cache kernels  0.000        0.000        0.000        0.000
    placed sink: attention decode          0.740        0.446        0.849        0.495
    placed sink: attention decode multi    0.857        0.490        0.813        0.493
    placed sink: attention extend          0.811        0.799        0.883        0.773
    placed sink: attention extend branches 0.773        0.656        0.762        0.685
    placed sink: attention decode beams    0.844        0.495        2.170        0.489

The norm kernels' dispatch arms and row partitions (tests/norm_inputs.py with its edge rows; tests/test_norm_arms_gpu.py), measured on an MI355X
on 2026-10-20, worst over the shapes of each check (every limit is the floor of 2, except 7.272 for the bf16 summed column-sum partials, whose
model - torch's fp32 column sum - scores 3.636).  "partials summed" = the raw fp32 partial rows summed in fp64, held to eps = 2^-24; rstd is in
fp32 ulps from fp64 against a bound of 4:

    operation                                         bf16 model  bf16 kernel   fp16 model  fp16 kernel
    ------------------------------------------------  ----------  -----------   ----------  -----------
    colsum                                                 0.435        0.435        0.231        0.231
    colsum accumulate                                      0.439        0.439        0.173        0.173
    colsum partials summed, fp32 bound                     3.636        0.739        0.525        0.093
    layernorm_bwd db                                       0.457        0.457        0.487        0.487
    layernorm_bwd db accumulate                            0.446        0.446        0.477        0.477
    layernorm_bwd db partials summed, fp32 bound           0.038        0.001        0.136        0.002
    layernorm_bwd dw                                       0.470        0.470        0.473        0.473
    layernorm_bwd dw accumulate                            0.490        0.490        0.469        0.469
    layernorm_bwd dw partials summed, fp32 bound           0.274        0.096        0.336        0.097
    layernorm_bwd dx                                       0.447        0.447        0.428        0.428
    layernorm_bwd dx accumulate                            0.464        0.464        0.494        0.494
    layernorm_f32_to_f32 y (fp32)                          0.425        0.571        0.387        0.559
    layernorm_fwd y                                        0.497        0.497        0.500        0.500
    norm_fwd_f32in ln y                                    0.498        0.498        0.498        0.498
    norm_fwd_f32in rms y                                   0.994        0.994        0.992        0.992
    rmsnorm_bwd dw                                         0.493        0.493        0.476        0.476
    rmsnorm_bwd dw accumulate                              0.484        0.484        0.471        0.471
    rmsnorm_bwd dw partials summed, fp32 bound             0.287        0.095        0.123        0.104
    rmsnorm_bwd dx                                         0.498        0.498        0.496        0.496
    rmsnorm_bwd dx accumulate                              0.495        0.495        0.498        0.498
    rmsnorm_fwd rstd (fp32 ulps, bound 4)                  1.310        2.505        0.816        1.504
    rmsnorm_fwd y                                          0.996        0.996        0.998        0.998
    rmsnorm_fwd_q8 y                                       0.996        0.996        0.996        0.996

Their mutants (tests/test_numerics_cpu.py, on the same inputs): a dw without the row's last 8-element chunk, a block that skips its last row, a
reduce that skips a partial row score 85 to 1000 against 2 in the 16-bit dw / db at 9 rows and 1e4 to 7e5 under the fp32 bound at 4097 rows (a 16-bit
dw cannot see one row of 4097); a LayerNorm variance taken as E[x^2] - mu^2 in fp32 is invisible in a 16-bit y (c = 0.5, the model's own) and is
rejected in the fp32 y of mh_layernorm_f32_to_f32 (c = 8 to 12 against 2).

The scaled-fp8 GEMMs are held to |got - want| <= ulp_out(want) + C_ACC 2^-24 sum|ab| instead (see the fp8 section below).  Worst observed
(|got - want| - ulp) / (2^-24 sum|ab|) on an MI355X, against C_ACC = 512: the 4-wave kernel ~140 (K = 256, fp32 store); the 8-wave kernel over
the shapes, weight forms and epilogues of tests/test_fp8_componentwise_gpu.py 167 (bf16 store), 185 (fp16 store), 175 (fp32 store), 71 / 104
(dgrad with block exponents, bf16 / fp16), 36 / 61 (wgrad over 1000 tokens).

The mutants of tests/test_numerics_cpu.py (a tile of keys dropped, a causal mask off by one, AdamW without bias correction, ...) score
c between 5 and several thousand against limits of 2 to 4; the max-norm metric of tests/test_ops_gpu.py lets most of them pass in bf16.
"""
import math

import torch

EPS16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
# absolute rounding floor of a stored value: half the spacing of the subnormals (fp16: 2^-24 apart; bf16 and fp32 share an exponent range)
TINY = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -150}
F16_SUB = 2.0 ** -25  # half the spacing of fp16 subnormals: what rounding P (or dS) below 2^-14 to fp16 moves it by


def limit(c_model):
    """2 x the rounding model's own c: a different summation order and the exp2-based softmax move a result by about as much again as the
    model's roundings do.  Floor 2 = two roundings of the output type.  Widening this factor is not an option (see the module docstring)."""
    return max(2.0, 2.0 * float(c_model))


def r16(x, dtype):
    """x rounded to the 16-bit type, back in x's own type (dtype None / fp32 on an fp32 tensor: unchanged)."""
    return x if dtype is None else x.to(dtype).to(x.dtype)


def componentwise(got, ref64, B, eps16, tiny=0.0):
    """-> (worst |got - ref64| / (eps16 * (|ref64| + B) + tiny'), index of that element).  Elements with ref64 == 0 and B == 0 (masked query
    rows, zero padding, untouched cache rows) are not scored: they must be EXACTLY zero, which is asserted here."""
    ref64 = ref64.double()
    got = got.double().reshape(ref64.shape)
    Bt = (B if isinstance(B, torch.Tensor) else torch.full_like(ref64, float(B))).double().expand_as(ref64)
    exact = (ref64 == 0) & (Bt == 0)
    bad = exact & (got != 0)
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"element {_unravel(i, ref64.shape)} must be exactly zero, got {float(got.reshape(-1)[i])!r} ({int(bad.sum())} such elements)")
    assert bool(torch.isfinite(got).all()), f"{int((~torch.isfinite(got)).sum())} non-finite elements"
    ratio = (got - ref64).abs() / (eps16 * (ref64.abs() + Bt) + max(tiny, 1e-300))
    ratio = torch.where(exact, torch.zeros_like(ratio), ratio)
    c, i = ratio.reshape(-1).max(0)
    return float(c), _unravel(int(i), ref64.shape)


def _unravel(i, shape):
    idx = []
    for n in reversed(shape):
        idx.append(i % n)
        i //= n
    return tuple(reversed(idx))


# ---- GEMM / GEMV ------------------------------------------------------------------------------------------------------------------------
QUICK_GELU_SLOPE = 1.1  # max |d/dx x sigmoid(1.702 x)| = 1.0998: an error of the pre-activation is amplified by at most this


def gemm(a, b, *, bias=None, resid=None, c_old=None, gelu=False, a_t=False, b_t=False, model=None, out_dtype=None, staged_accumulate=False):
    """C = op(A) op(B)^T (+ bias) (quick-GELU) (+ resid) (+ C_old), the epilogue order of mh_gemm; out_dtype (default: a's) is the type C is
    stored in.  -> (ref64, B) or, with model=dtype, the rounding model (fp32 product, ONE rounding to out_dtype at the store).
    The condition magnitude is |A| |B|^T + |bias| (x 1.1 through quick-GELU) + |resid| + |C_old|, but NO term of it is rounded to 16 bits:
    products of two 16-bit values are exact in fp32 and the sum is accumulated in fp32 (include/merlin_hip.h: "bf16/f16 MFMA, fp32
    accumulate"), so a K-term sum moves only by the fp32 roundings of its partial sums.  Each is at most 2^-24 of that magnitude; they are
    independent in sign, so K of them add up like sqrt(K), not K (the worst case K would let an fp32-stored result that was rounded to 16 bits on
    the way pass in fp16: the mutant "fp32 store rounded to 16 bits first" of tests/test_numerics_cpu.py) - and the magnitude itself already
    overstates every partial sum.  B is therefore that magnitude times (sqrt(K) + 4) * 2^-24 / eps(out_dtype), 4 for the epilogue's adds.
    With the plain magnitude, eps16 * B exceeds a whole bias at K = 512 and the mutant "bias added twice" passes too.
    staged_accumulate: the 4-wave kernel's 16-bit MH_EPI_ACCUM (csrc/gemm_w4.hip w4_store, "Staged epilogue": line 239 packs the quadrant to
    16 bits into LDS - `pack2<DT>` in `stage8` - and line 463, `a[e] += o[e]`, adds C_old to those packed values on the way out) rounds the product BEFORE it adds C_old -
    the arithmetic of torch's own `grad += new_grad` on 16-bit gradients.  The model then rounds there too and B gains the product's
    magnitude once (one eps16 rounding of it).  The 8-wave and 128-tile kernels add in fp32 and are held to the form without it."""
    wt = torch.float64 if model is None else torch.float32
    od = a.dtype if out_dtype is None else out_dtype
    A = (a.t() if a_t else a).to(wt)
    Bm = (b if b_t else b.t()).to(wt)
    K = A.shape[1]
    acc = A @ Bm
    cond = A.abs() @ Bm.abs() if model is None else None
    if bias is not None:
        acc = acc + bias.to(wt)
        if model is None:
            cond = cond + bias.to(wt).abs()
    if gelu:
        acc = acc * torch.sigmoid(1.702 * acc)
        if model is None:
            cond = cond * QUICK_GELU_SLOPE
    staged = None
    if staged_accumulate:
        staged = acc.abs() if model is None else None
        acc = r16(acc, None if model is None else od)
    for extra in (resid, c_old):
        if extra is not None:
            acc = acc + extra.to(wt)
            if model is None:
                cond = cond + extra.to(wt).abs()
    if model is None:
        cond = cond * ((math.sqrt(K) + 4) * EPS16[torch.float32] / EPS16[od])
        return acc, (cond if staged is None else cond + staged)
    return r16(acc, None if od == torch.float32 else od)


# ---- fp8 (OCP e4m3) operands: exact dequantisers, the scaled-fp8 GEMM and the fp8-weight GEMV ---------------------------------------------
# The scaled fp8 MFMA (v_mfma_scale_f32_16x16x128_f8f6f4) sums a 128-k block's products at LESS than fp32 precision, so the fp8 GEMMs are not
# held to the (sqrt(K) + 4) 2^-24 form of `gemm` but, per element, to
#     |got - want| <= ulp_out(want) + C_ACC 2^-24 sum_k |a_k b_k| + epilogue terms
# with want the float64 product of the EXACTLY dequantised operands (an e4m3 value times an fp32 scale needs 28 bits: `q.float() * s` is itself
# rounded).  C_ACC is the project's figure for this MFMA (worst observed on an MI355X: ~140 on the 4-wave kernel, K = 256, fp32 store; see the
# table in the module docstring for the 8-wave kernel); C_OP 2^-24 times the magnitude of the terms an fp32 element-wise op adds is that op's
# own arithmetic, TINY_OP its flush-to-zero floor.  The fp8-weight GEMV multiplies in dot2 / 16-bit MFMA instructions (exact products, fp32
# sums) and IS held to `componentwise` with the (sqrt(K) + 4) form.
C_ACC = 512
C_OP = 64
TINY_OP = 2.0 ** -100
U24 = 2.0 ** -24
_MANT = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}
_ULP_FLOOR = {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24, torch.float32: 2.0 ** -149}
E4M3_MAX = 448.0


def ulp(x, dtype):
    """Spacing of `dtype` at |x| (float64 tensor), floored at the subnormal spacing."""
    _, e = torch.frexp(x.abs())
    return torch.ldexp(torch.ones_like(x), (e - 1 - _MANT[dtype]).to(torch.int32)).clamp_min(_ULP_FLOOR[dtype])


def bound_ratio(got, want, err, dtype):
    """-> (worst |got - want| / (ulp_dtype(want) + err), flat index of that element)."""
    r = (got.double() - want).abs() / (ulp(want, dtype) + err)
    c, i = r.reshape(-1).max(0)
    return float(c), int(i)


def check(name, got, want, err, dtype):
    """every element: |got - want| <= ulp_dtype(want) + err"""
    d = (got.double() - want).abs()
    tol = ulp(want, dtype) + err
    assert torch.isfinite(got.float()).all(), name
    bad = d > tol
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        r, c = divmod(i, want.shape[1])
        import pytest

        pytest.fail(f"{name}: {int(bad.sum())} of {bad.numel()} elements outside the bound, first [{r}, {c}]: got {float(got.flatten()[i])} "
                    f"want {float(want.flatten()[i])} bound {float(tol.flatten()[i]):.3e}")


def e4m3(q):
    """uint8 e4m3 bytes -> their values in float64 (exact)."""
    return q.view(torch.float8_e4m3fn).double()


def deq64(q8):
    """(q uint8 [R, K], s fp32 [R]) of quant_fp8_rows / quant_fp8_rows_t -> float64 [R, K] = q s, exact."""
    return e4m3(q8[0]) * q8[1].double()[:, None]


def exp_group_bytes(K):
    return ((K // 128) * 64 + 4095) // 4096 * 4096


def exp_nibbles(ex, n_rows, K):
    """Exponent image of quant_fp8_rows_e4 / _rows_t_e4 (include/merlin_hip.h: 16-byte header, then [row / 128][G bytes], a group = [K / 128
    blocks][64 B], two rows per byte, low nibble = even row) -> int64 [n_rows, K / 128].  The header flag must say whether any exponent is
    non-zero: the GEMM takes its constant-scale loop while it is 0."""
    nkb, G = K // 128, exp_group_bytes(K)
    assert int(ex[:4].view(torch.int32)) == int(bool(ex[16:].any())), "the header flag says whether any exponent is non-zero"
    img = ex[16:].view(-1, G)
    rows = torch.arange(n_rows, device=ex.device)
    byte = img[(rows >> 7)[:, None], torch.arange(nkb, device=ex.device)[None, :] * 64 + ((rows & 127) >> 1)[:, None]]
    return ((byte >> ((rows & 1) * 4)[:, None]) & 15).long()


def exp_image(e, device=None):
    """The inverse of exp_nibbles: int [N, K / 128] exponents in [0, 15] -> the uint8 image with its header, sized as ops._exp_image sizes it."""
    Nr, nkb = e.shape
    device = e.device if device is None else device
    G = exp_group_bytes(nkb * 128)
    img = torch.zeros(((Nr + 255) // 256) * 2, G, dtype=torch.uint8)
    ec = e.cpu().to(torch.uint8)
    rows = torch.arange(Nr)
    col = torch.arange(nkb)[None, :] * 64 + ((rows & 127) >> 1)[:, None]
    grp = (rows >> 7)[:, None].expand(Nr, nkb)
    for par in (0, 1):  # even rows: low nibble, odd rows: high nibble (two passes: the two rows of a pair share every byte)
        sel = (rows & 1) == par
        img[grp[sel], col[sel]] |= ec[sel] << (4 * par)
    head = torch.zeros(16, dtype=torch.uint8)
    head[:4] = torch.tensor([int(bool(ec.any()))], dtype=torch.int32).view(torch.uint8)
    return torch.cat([head, img.reshape(-1)]).to(device)


def deq64_e4(q, s, ex, n_rows=None, K=None):
    """(q [N, K], s [N], exponent image) -> (float64 [N, K] = q s 2^-e per 128-k block, e int64 [N, K / 128]), exact."""
    n_rows = q.shape[0] if n_rows is None else n_rows
    K = q.shape[1] if K is None else K
    e = exp_nibbles(ex, n_rows, K)
    scale = torch.ldexp(s.double()[:n_rows, None].expand(n_rows, K // 128).contiguous(), (-e).to(torch.int32))
    return (e4m3(q[:n_rows, :K]).view(n_rows, K // 128, 128) * scale[:, :, None]).view(n_rows, K), e


def deq64_any(b8):
    """(q, s) or (q, s, exponent image or None) -> float64, exact."""
    if len(b8) > 2 and b8[2] is not None:
        return deq64_e4(b8[0], b8[1], b8[2])[0]
    return deq64(b8)


def deq64_b128(q, scales):
    """(q [N, K], scales fp32 [N, ceil(K / 128)]) of quant_fp8_b128 -> float64 [N, K]; the last block may be partial."""
    K = q.shape[1]
    return e4m3(q) * scales.double().repeat_interleave(128, dim=1)[:, :K]


def exact_block_exp(rowmax, bmax):
    """floor(log2(rowmax / blockmax)) clamped to [0, 15], 15 for an all-zero block, from the binary exponents and significands (no log2):
    rowmax [N, 1] and bmax [N, nkb] fp32, as csrc/fp8_quant.hip block_exp computes it."""
    ma, ea = torch.frexp(rowmax.float())
    mb, eb = torch.frexp(bmax.float())
    e = (ea - eb - (ma < mb).to(ea.dtype)).clamp(0, 15)
    return torch.where(bmax > 0, e, torch.full_like(e, 15)).long()


def quant_rows(x):
    """torch emulation of mh_quant_fp8_rows: s = max|row| (1 / 448) in fp32 (1 for a zero row), bytes = e4m3_rne(x (1 / s))."""
    amax = x.float().abs().amax(1)
    s = torch.where(amax > 0, amax * torch.tensor(1.0 / E4M3_MAX, dtype=torch.float32, device=x.device), torch.ones_like(amax))
    return (x.float() * (1.0 / s)[:, None]).to(torch.float8_e4m3fn).view(torch.uint8), s


def quant_b128(w):
    """torch emulation of mh_quant_fp8_b128: one scale per 128 consecutive k (the last block may be partial)."""
    Nr, K = w.shape
    nb = (K + 127) // 128
    wp = torch.nn.functional.pad(w.float(), (0, nb * 128 - K)).view(Nr, nb, 128)
    amax = wp.abs().amax(2)
    s = torch.where(amax > 0, amax * torch.tensor(1.0 / E4M3_MAX, dtype=torch.float32, device=w.device), torch.ones_like(amax))
    q = (wp * (1.0 / s)[:, :, None]).to(torch.float8_e4m3fn).view(torch.uint8).view(Nr, nb * 128)[:, :K].contiguous()
    return q, s


def gemm_fp8(a8, b8, *, bias=None, gelu=False, resid=None, c_old=None, out_dtype=torch.bfloat16, model=False):
    """mh_gemm_fp8: C = (sa qa) (sb 2^-e qb)^T (+ bias) (quick-GELU) (+ resid) (+ C_old), the epilogue order of mh_gemm.  a8 = (qa, sa), b8 = (qb,
    sb[, exponent image]).  -> (want64, err): a kernel's output is held to |got - want64| <= ulp_out(want64) + err (`check`), err = C_ACC 2^-24
    |A| |B|^T carried through the epilogue: every fp32 add of the store phase contributes C_OP 2^-24 times the magnitude of its two terms,
    quick-GELU multiplies the error of its argument by QUICK_GELU_SLOPE and adds its own arithmetic - x / (1 + exp(-1.702 x)) with the
    argument of exp rounded to fp32, which moves the result by |out| (1 - sigmoid) |1.702 x| 2^-24 - plus TINY_OP where it flushes.  C_old is added
    in fp32 BEFORE the one rounding of the store (csrc/gemm_common.h epi_store4 / EpiStoreFast: `v += o` ahead of pack2 - the 8-wave and
    128-tile kernels; the 4-wave kernel's staged form is `gemm(..., staged_accumulate=True)`).
    model=True: the rounding model instead - the integer-valued products summed in fp32, the two row scales multiplied in fp32 and applied
    once (csrc/gemm256.hip: `acc *= sm * sc_n`), the epilogue in fp32, ONE rounding to out_dtype."""
    A, Bd = deq64(a8), deq64_any(b8)
    if model:
        qb = e4m3(b8[0])
        if len(b8) > 2 and b8[2] is not None:
            e = exp_nibbles(b8[2], *b8[0].shape)
            qb = (qb.view(qb.shape[0], -1, 128) * torch.ldexp(torch.ones_like(e, dtype=torch.float64), (-e).to(torch.int32))[:, :, None]).view(qb.shape)
        acc = (e4m3(a8[0]).float() @ qb.float().t()) * (a8[1].float()[:, None] * b8[1].float()[None, :])
        if bias is not None:
            acc = acc + bias.float()
        if gelu:
            acc = acc * torch.sigmoid(1.702 * acc)
        for extra in (resid, c_old):
            if extra is not None:
                acc = acc + extra.float()
        return r16(acc, None if out_dtype == torch.float32 else out_dtype)
    want = A @ Bd.t()
    err = C_ACC * U24 * (A.abs() @ Bd.abs().t())
    if bias is not None:
        b64 = bias.double()
        err = err + C_OP * U24 * (want.abs() + b64.abs())
        want = want + b64
    if gelu:
        z = 1.702 * want
        sg = torch.sigmoid(z)
        want = want * sg
        err = QUICK_GELU_SLOPE * err + C_OP * U24 * want.abs() * (1 + z.abs() * (1 - sg)) + TINY_OP
    for extra in (resid, c_old):
        if extra is not None:
            x64 = extra.double()
            err = err + C_OP * U24 * (want.abs() + x64.abs())
            want = want + x64
    return want, err


def _block_sums(X, Q):
    """X [M, K], Q [N, K] -> [M, N, ceil(K / 128)]: sum of x q over each 128-k block (a partial last block padded with zeros)."""
    K = X.shape[1]
    nb = (K + 127) // 128
    Xp, Qp = (torch.nn.functional.pad(t, (0, nb * 128 - K)) for t in (X, Q))
    return torch.einsum("mbk,nbk->mnb", Xp.view(X.shape[0], nb, 128), Qp.view(Q.shape[0], nb, 128))


def gemv_fp8w(x, q, scales, resid=None, *, out_dtype=None, model=None):
    """mh_gemv_fp8w: y[m, n] = sum_kb s[n, kb] sum_{k in block kb} q[n, k] x[m, k] (+ resid), (q, scales) from quant_fp8_b128, the scale
    applied to the block sum as the kernels do (csrc/decode.hip: `acc = fmaf(s, p, acc)`).  -> (ref64, B) for `componentwise`: the products
    of an e4m3 value and a 16-bit activation are exact (the kernels widen the bytes to 16 bits and multiply in dot2 / MFMA instructions) and the
    sums are fp32, so as in `gemm` B = (sum_kb |s| sum |q| |x| + |resid|) (sqrt(K) + 4) 2^-24 / eps(out).
    model=dtype: fp32 block sums, fp32 scale and add, ONE rounding at the store."""
    wt = torch.float64 if model is None else torch.float32
    od = x.dtype if out_dtype is None else out_dtype
    X, Q, S = x.to(wt), e4m3(q).to(wt), scales.to(wt)
    K = X.shape[1]
    acc = (_block_sums(X, Q) * S[None]).sum(-1)
    if resid is not None:
        acc = acc + resid.to(wt)
    if model is not None:
        return r16(acc, None if od == torch.float32 else od)
    cond = (_block_sums(X.abs(), Q.abs()) * S.abs()[None]).sum(-1)
    if resid is not None:
        cond = cond + resid.to(wt).abs()
    return acc, cond * ((math.sqrt(K) + 4) * EPS16[torch.float32] / EPS16[od])


# ---- attention (one head) -----------------------------------------------------------------------------------------------------------------
def attention(q, k, v, do=None, *, causal, n_valid=None, model=None, allowed=None, chunk=2048, keep=False):
    """One (batch, head): q, k, v, do [S, D] in the 16-bit type.  Semantics of mh_attn_fwd2 / mh_attn_bwd2: keys >= n_valid excluded, query
    rows >= n_valid zero.  Chunked over queries (the fp64 score matrix of S = 8192 is never held whole).
    model=None: fp64 reference -> dict o, lse, B_o and, with do: dq, dk, dv, B_dq, B_dk, B_dv, abs_dv, abs_dk, abs_dq.
        B_o = P |V|;  B_dv = P^T |dO|;  |dS|_bound = P o (|dP| + sum_d |o||dO|),  B_dq = |dS|_bound |K| scale,  B_dk = |dS|_bound^T |Q| scale.
        abs_* = sum_i |dO_i| (resp. scale sum_i |Q_i|, scale sum_j |K_j|) over the ATTENDED pairs: multiplied by F16_SUB it is what rounding P / dS
        to fp16 subnormals can move dV / dK / dQ by (see `f16_subnormal_B`).
    model=dtype: the rounding model in fp32 - P rounded before P V (csrc/attn_fwd2.hip packs exp2 of the scores into the MFMA A operand) and
        before P^T dO, dS rounded before dS K and dS^T Q (csrc/attn_bwd2.hip; the five-product form stores that 16-bit dS), delta taken from
        the o that was stored, every output rounded.
    allowed(q0, q1) -> bool [q1 - q0, S] replaces the mask (the mutants of tests/test_numerics_cpu.py)."""
    wt = torch.float64 if model is None else torch.float32
    rd = (lambda x: x) if model is None else (lambda x: r16(x, model))
    S, D = q.shape
    scale = 1.0 / math.sqrt(D)
    n = S if n_valid is None else int(n_valid)
    Q, K, V = q.to(wt), k.to(wt), v.to(wt)
    dO = None if do is None else do.to(wt)
    ar = torch.arange(S, device=q.device)
    out = {"o": torch.zeros(S, D, dtype=wt, device=q.device), "lse": torch.zeros(S, dtype=wt, device=q.device)}
    names = ["B_o"] if do is None else ["B_o", "dq", "dk", "dv", "B_dq", "B_dk", "B_dv", "abs_dv", "abs_dk", "abs_dq"]
    for nm in names:
        if model is None or nm in ("dq", "dk", "dv"):
            out[nm] = torch.zeros(S, D, dtype=wt, device=q.device)
    for q0 in range(0, S, chunk):
        q1 = min(S, q0 + chunk)
        if allowed is not None:
            ok = allowed(q0, q1)
        else:
            ok = (ar[None, :] < n) & (ar[q0:q1, None] < n)
            if causal:
                ok = ok & (ar[None, :] <= ar[q0:q1, None])
        s = ((Q[q0:q1] @ K.t()) * scale).masked_fill(~ok, float("-inf"))
        m = s.amax(1, keepdim=True)
        m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        e = torch.exp(s - m)
        l = e.sum(1, keepdim=True)
        linv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
        o = rd((rd(e) @ V) * linv)
        P = e * linv
        out["o"][q0:q1] = o
        out["lse"][q0:q1] = torch.where(l > 0, m + torch.log(l.clamp_min(1e-300)), torch.zeros_like(l))[:, 0]
        if model is None:
            out["B_o"][q0:q1] = P @ V.abs()
        if dO is None:
            continue
        g = dO[q0:q1]
        delta = (o * g).sum(1, keepdim=True)
        dP = g @ V.t()
        out["dv"] += rd(P).t() @ g
        dS = P * (dP - delta)
        dS16 = rd(dS)
        out["dq"][q0:q1] = (dS16 @ K) * scale
        out["dk"] += (dS16.t() @ Q[q0:q1]) * scale
        if model is None:
            out["B_dv"] += P.t() @ g.abs()
            dSb = P * (dP.abs() + (o.abs() * g.abs()).sum(1, keepdim=True))
            out["B_dq"][q0:q1] = (dSb @ K.abs()) * scale
            out["B_dk"] += (dSb.t() @ Q[q0:q1].abs()) * scale
            okf = ok.to(wt)
            out["abs_dv"] += okf.t() @ g.abs()
            out["abs_dk"] += (okf.t() @ Q[q0:q1].abs()) * scale
            out["abs_dq"][q0:q1] = (okf @ K.abs()) * scale
        if keep:
            out["P"], out["dS"], out["ok"] = P, dS, ok
    if dO is not None:
        for nm in ("dq", "dk", "dv"):
            out[nm] = rd(out[nm])
    return out


def attention_magnitude(q, k, *, causal, n_valid=None):
    """A_row [S]: the row's largest scale sum_d |q_id k_jd| over the pairs it attends (0 for a row that attends nothing): what one fp32
    rounding of a partial sum of the score can move that score - and with it lse - by, in units of 2^-24."""
    S, D = q.shape
    n = S if n_valid is None else int(n_valid)
    ar = torch.arange(S, device=q.device)
    ok = (ar[None, :] < n) & (ar[:, None] < n)
    if causal:
        ok = ok & (ar[None, :] <= ar[:, None])
    A = (q.double().abs() @ k.double().abs().t()) / math.sqrt(D)
    return A.masked_fill(~ok, 0.0).amax(1)


def attention_lse_model(q, k, *, causal, n_valid=None):
    """The rounding model of lse: fp32 scores (one fp32 matmul, one multiply by scale), fp32 logsumexp; 0 for a row that attends nothing."""
    S, D = q.shape
    n = S if n_valid is None else int(n_valid)
    ar = torch.arange(S, device=q.device)
    ok = (ar[None, :] < n) & (ar[:, None] < n)
    if causal:
        ok = ok & (ar[None, :] <= ar[:, None])
    s = ((q.float() @ k.float().t()) * torch.tensor(1.0 / math.sqrt(D), dtype=torch.float32, device=q.device)).masked_fill(~ok, float("-inf"))
    any_ok = ok.any(1)
    s = torch.where(any_ok[:, None], s, torch.zeros_like(s))
    return torch.where(any_ok, torch.logsumexp(s, 1), torch.zeros_like(s[:, 0]))


def lse_c(got, lse64, A_row):
    """lse (fp32, nats) is held to |lse - lse64| <= c 2^-24 (|lse64| + A_row + 1): lse is a score plus log l with l in [1, S], so it carries the
    fp32 roundings of the score's partial sums (A_row), of its own magnitude, and of log l (the + 1).  -> (worst c, row).  Rows that attend
    nothing (A_row == 0 and lse64 == 0) must be exactly zero."""
    lse64 = lse64.double()
    got = got.double().reshape(lse64.shape)
    A_row = A_row.double().reshape(lse64.shape)
    exact = (lse64 == 0) & (A_row == 0)
    assert not bool((exact & (got != 0)).any()), "lse of a row that attends nothing must be exactly zero"
    assert bool(torch.isfinite(got).all()), f"{int((~torch.isfinite(got)).sum())} non-finite lse values"
    ratio = (got - lse64).abs() / (EPS16[torch.float32] * (lse64.abs() + A_row + 1.0))
    ratio = torch.where(exact, torch.zeros_like(ratio), ratio)
    c, i = ratio.reshape(-1).max(0)
    return float(c), _unravel(int(i), lse64.shape)


def f16_subnormal_B(ref, name, dtype):
    """B of dq / dk / dv with the fp16 subnormal term folded in.  P (and with it dS) below 2^-14 is subnormal in fp16: rounding it moves it by
    up to F16_SUB ABSOLUTELY, not by eps16 relatively, and at S = 4096 most of a softmax row is that small.  The 16-bit MFMA operand P of
    P^T dO therefore moves dV[j] by up to F16_SUB * sum_i |dO_i| over the queries i that attend key j; dS in dS^T Q moves dK likewise with the
    Q sum.  dQ = dS K has the same operand, so it gets the K sum.  In units of eps16 that is abs_* * F16_SUB / eps16.  bf16 has fp32's exponent range: no term."""
    B = ref["B_" + name]
    if dtype == torch.float16:
        B = B + ref["abs_" + name] * (F16_SUB / EPS16[dtype])
    return B


# ---- norms ---------------------------------------------------------------------------------------------------------------------------------
def rmsnorm(x, w, eps, dy=None, *, dx_old=None, model=None):
    """LlamaRMSNorm y = w x rstd, rstd = rsqrt(mean x^2 + eps).  -> dict y, B_y (0: the sum of squares has no cancellation, one rounding at the
    store) and, with dy: dx = rstd (w dy - xh mean(xh w dy)) (+ dx_old), dw = sum_rows dy xh, with B_dx, B_dw = the same sums of absolute values."""
    wt = torch.float64 if model is None else torch.float32
    X, W = x.to(wt), w.to(wt)
    rstd = torch.rsqrt((X * X).mean(1, keepdim=True) + eps)
    xh = X * rstd
    out = {"y": r16(xh * W, model), "B_y": 0.0}
    if dy is not None:
        G = dy.to(wt) * W
        proj = (xh * G).mean(1, keepdim=True)
        dx = rstd * (G - xh * proj)
        Bdx = rstd * (G.abs() + xh.abs() * (xh * G).abs().mean(1, keepdim=True))
        if dx_old is not None:
            dx, Bdx = dx + dx_old.to(wt), Bdx + dx_old.to(wt).abs()
        out.update(dx=r16(dx, model), B_dx=Bdx, dw=(dy.to(wt) * xh).sum(0), B_dw=(dy.to(wt) * xh).abs().sum(0))
    return out


def layernorm(x, w, b, eps, dy=None, *, dx_old=None, model=None):
    """nn.LayerNorm.  y = xh w + b, B_y = |xh w| + |b|; dx = rstd (g - mean g - xh mean(g xh)), g = w dy; dw = sum dy xh, db = sum dy."""
    wt = torch.float64 if model is None else torch.float32
    X, W, Bb = x.to(wt), w.to(wt), b.to(wt)
    mu = X.mean(1, keepdim=True)
    rstd = torch.rsqrt(((X - mu) ** 2).mean(1, keepdim=True) + eps)
    xh = (X - mu) * rstd
    out = {"y": r16(xh * W + Bb, model), "B_y": (xh * W).abs() + Bb.abs()}
    if dy is not None:
        DY = dy.to(wt)
        G = DY * W
        dx = rstd * (G - G.mean(1, keepdim=True) - xh * (G * xh).mean(1, keepdim=True))
        Bdx = rstd * (G.abs() + G.abs().mean(1, keepdim=True) + xh.abs() * (G * xh).abs().mean(1, keepdim=True))
        if dx_old is not None:
            dx, Bdx = dx + dx_old.to(wt), Bdx + dx_old.to(wt).abs()
        out.update(dx=r16(dx, model), B_dx=Bdx, dw=(DY * xh).sum(0), B_dw=(DY * xh).abs().sum(0), db=DY.sum(0), B_db=DY.abs().sum(0))
    return out


def reduce_rows(partial, old=None, *, model=None):
    """mh_reduce_partials: out[d] = sum_r partial[r, d] (+ old).  -> (ref64, B = sum |partial| + |old|) or the model (fp32 sum, one rounding)."""
    wt = torch.float64 if model is None else torch.float32
    s = partial.to(wt).sum(0)
    Bc = partial.to(wt).abs().sum(0)
    if old is not None:
        s, Bc = s + old.to(wt), Bc + old.to(wt).abs()
    return (s, Bc) if model is None else r16(s, None if model == torch.float32 else model)


def colsum(x, old=None, *, model=None):
    """mh_colsum_partial + mh_reduce_partials: out[d] = sum_r x[r, d] (+ old), x 16-bit (any row stride).  -> (ref64, B = sum |x| + |old|) like
    `reduce_rows`, or the model: every term is exact in fp32, the sum is fp32, ONE rounding at the store (model=torch.float32: none)."""
    return reduce_rows(x, old, model=model)


def norm_f32in(x32, w, b, eps, *, y_dtype, model=None):
    """mh_norm_fwd_f32in (y_dtype = w's 16-bit type) and mh_layernorm_f32_to_f32 (y_dtype = fp32): the fp32 stream's reader.  x32 fp32 [rows, d],
    b None: RMSNorm, else LayerNorm.  -> dict y, B_y, x16; x16 = x32 rounded to nearest-even in w's type, which the kernel must reproduce
    exactly (torch.equal).  model=w's dtype: the same in fp32, y rounded once to y_dtype (not at all when that is fp32).
    The input is not a 16-bit value here and y may be stored in fp32, so the fp32 arithmetic itself is what B_y measures, in units of
    eps(y_dtype): F = 4 (rstd |w| mean|x| + |xh w| / 2) + |xh w| + |b|, times 2^-24 / eps(y_dtype).  Its terms: the row sums are trees (a
    lane's d / 64 terms, then a 64-lane butterfly; torch's pairwise sum in the model), so only their last levels round at the size of the
    result - 4 roundings of mean|x| allowed for the mean with its divide, not the sqrt(K) of `gemm`'s sequential K loop - and an error of
    the mean moves every y of the row by rstd |w| times itself (LayerNorm only); the variance is such a sum of non-negative terms and rstd
    carries half its relative error into xh w; the last multiply-add rounds |xh w| and |b| once each.  A 16-bit LayerNorm y keeps
    `layernorm`'s own B_y = |xh w| + |b| on top (the two may cancel), a 16-bit RMSNorm y none, as in `rmsnorm`."""
    wt = torch.float64 if model is None else torch.float32
    X, W = x32.to(wt), w.to(wt)
    mu = X.mean(1, keepdim=True) if b is not None else torch.zeros_like(X[:, :1])
    rstd = torch.rsqrt(((X - mu) ** 2).mean(1, keepdim=True) + eps)
    xh = (X - mu) * rstd
    y = xh * W if b is None else xh * W + b.to(wt)
    x16 = x32.to(w.dtype)
    if model is not None:
        return {"y": r16(y, None if y_dtype == torch.float32 else y_dtype), "x16": x16}
    k = 4.0
    F = (k / 2 + 1) * (xh * W).abs()
    if b is not None:
        F = F + k * rstd * W.abs() * X.abs().mean(1, keepdim=True) + b.to(wt).abs()
    By = F * (EPS16[torch.float32] / EPS16[y_dtype])
    if b is not None and y_dtype != torch.float32:
        By = By + (xh * W).abs() + b.to(wt).abs()
    return {"y": y, "B_y": By, "x16": x16}


# ---- elementwise: single roundings of a short expression, B = 0 ----------------------------------------------------------------------------
def _wt(model):
    return torch.float64 if model is None else torch.float32


def swiglu_fwd(gu, *, model=None):
    ff = gu.shape[1] // 2
    g, u = gu[:, :ff].to(_wt(model)), gu[:, ff:].to(_wt(model))
    return r16(g * torch.sigmoid(g) * u, model)


def swiglu_bwd(gu, dout, *, model=None):
    ff = gu.shape[1] // 2
    g, u, d = gu[:, :ff].to(_wt(model)), gu[:, ff:].to(_wt(model)), dout.to(_wt(model))
    sg = torch.sigmoid(g)
    return r16(torch.cat([d * u * sg * (1 + g * (1 - sg)), d * g * sg], 1), model)


def quick_gelu_fwd(x, *, model=None):
    X = x.to(_wt(model))
    return r16(X * torch.sigmoid(1.702 * X), model)


def quick_gelu_bwd(x, dy, *, model=None):
    X, d = x.to(_wt(model)), dy.to(_wt(model))
    sg = torch.sigmoid(1.702 * X)
    return r16(d * sg * (1 + 1.702 * X * (1 - sg)), model)


def add(a, b, *, model=None):
    return r16(a.to(_wt(model)) + b.to(_wt(model)), model)


def rope_table(S, D, theta, device="cpu"):
    """[S, D/2, 2] (cos, sin) in fp32 from fp64 angles (layout of mh_rope_table)."""
    inv = theta ** (-torch.arange(0, D, 2, dtype=torch.float64, device=device) / D)
    ang = torch.arange(S, dtype=torch.float64, device=device)[:, None] * inv[None, :]
    return torch.stack([ang.cos(), ang.sin()], -1).float()


def rope(x, table, S, *, inverse=False, model=None):
    """Rotate-half RoPE of x [T, nheads, D] at position t % S with the fp32 table the kernel itself reads: out1 = x1 c - x2 s, out2 = x2 c + x1 s
    (inverse: s -> -s)."""
    wt = _wt(model)
    T, _, D = x.shape
    X = x.to(wt)
    pos = torch.arange(T, device=x.device) % S
    c, s = table[pos, :, 0].to(wt)[:, None, :], table[pos, :, 1].to(wt)[:, None, :]
    if inverse:
        s = -s
    x1, x2 = X[..., :D // 2], X[..., D // 2:]
    return r16(torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1), model)


# ---- the same element maths behind a GEMM (fused epilogues): the argument itself carries one 16-bit rounding ---------------------------------
# mh_gemm_swiglu_fwd / mh_gemm_gelu_fwd / mh_gemm_nt_rope store the projection AND a function of it; the 8-wave kernel applies the function
# to the ROUNDED 16-bit tile (include/merlin_hip.h: "bit-identical to the unfused sequence"), the 4-wave kernel to the fp32 accumulators.
# Against the fp64 function of the fp64 projection, the result may therefore move by eps16 |x f'(x)| per argument x on top of its own store.
def swiglu_fwd_cond(gu64, B_gu=None):
    """B of act = silu(gate) * up when gate | up come out of a GEMM: |d act / d gate| (|gate| + B_gate) + |d act / d up| (|up| + B_up), B_gu the
    GEMM's own B (a gate that cancels to ~ 0 in the product is uncertain by B_gate, not by eps16 |gate|)."""
    ff = gu64.shape[1] // 2
    g, u = gu64[:, :ff], gu64[:, ff:]
    Bg, Bu = (0.0, 0.0) if B_gu is None else (B_gu[:, :ff], B_gu[:, ff:])
    sg = torch.sigmoid(g)
    return (u * sg * (1 + g * (1 - sg))).abs() * (g.abs() + Bg) + (g * sg).abs() * (u.abs() + Bu)


def quick_gelu_fwd_cond(x64, B_x=0.0):
    sg = torch.sigmoid(1.702 * x64)
    return (sg * (1 + 1.702 * x64 * (1 - sg))).abs() * (x64.abs() + B_x)


def rope_cond(x64, table, S):
    """|x1 c| + |x2 s| per output: what a rounding of x1 and of x2 moves the rotated pair by."""
    T, _, D = x64.shape
    pos = torch.arange(T, device=x64.device) % S
    c, s = table[pos, :, 0].double()[:, None, :].abs(), table[pos, :, 1].double()[:, None, :].abs()
    x1, x2 = x64[..., :D // 2].abs(), x64[..., D // 2:].abs()
    return torch.cat([x1 * c + x2 * s, x2 * c + x1 * s], -1)


def attention_decode(q, kc, vc, n, *, model=None):
    """One sequence of mh_attn_decode: q [H, D], caches [Smax, H, D], keys [0, n).  -> (o [H, D], B = P |V|); the model rounds P like the
    prefill kernels do (the decode kernels keep P in fp32: one rounding fewer than the model allows)."""
    wt = _wt(model)
    H, D = q.shape
    Q, K, V = q.to(wt)[:, None, :], kc[:n].to(wt).permute(1, 0, 2), vc[:n].to(wt).permute(1, 0, 2)
    P = torch.softmax((Q @ K.transpose(1, 2)) / math.sqrt(D), -1)
    o = (r16(P, model) @ V)[:, 0]
    return r16(o, model) if model is not None else (o, (P @ V.abs())[:, 0])


# ---- shifted cross-entropy -----------------------------------------------------------------------------------------------------------------
def shifted_labels(labels):
    """Row (b, s) is scored against labels[b, s + 1]; the last position of a sample and -100 are ignored (-100 here)."""
    sh = torch.full_like(labels, -100)
    sh[:, :-1] = labels[:, 1:]
    return sh.reshape(-1)


def cross_entropy(logits, labels, V, gscale=1.0, *, model=None):
    """logits fp32 [T, >= V], labels int64 [B, S].  -> dict lse [T], row_loss [T], count, mean (NaN when count == 0, like torch), dlogits [T, V] =
    gscale / count (softmax - onehot) on scored rows, 0 elsewhere.  B = 0 per element: softmax entries of 1e-6 are held to their own size."""
    wt = _wt(model)
    x = logits[:, :V].to(wt)
    lab = shifted_labels(labels)
    scored = (lab >= 0) & (lab < V)
    lse = torch.logsumexp(x, 1)
    safe = lab.clamp(0, V - 1)
    row_loss = torch.where(scored, lse - x.gather(1, safe[:, None])[:, 0], torch.zeros_like(lse))
    count = int(scored.sum())
    sm = torch.exp(x - lse[:, None])
    sm.scatter_add_(1, safe[:, None], -scored.to(wt)[:, None])
    d = sm * scored.to(wt)[:, None] * ((gscale / count) if count else 0.0)
    return {"lse": lse, "row_loss": row_loss, "count": count, "mean": (row_loss.sum() / count) if count else torch.tensor(float("nan")),
            "dlogits": r16(d, model)}


# ---- AdamW: ONE step from the kernel's own previous state -----------------------------------------------------------------------------------
def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def adamw_step(p, g, m, v, *, lr, beta1, beta2, eps, wd, step, gscale=1.0, gscale_dev=None, model=None):
    """torch.optim.AdamW (decoupled decay, bias-corrected) with g scaled by gscale (* gscale_dev).  p, g 16-bit, m, v fp32: the state BEFORE the
    step, as the kernel left it, so the only accumulated error of p is its single 16-bit store (B_p: fp32 effects only).  The hyper-parameters are the C ABI's
    `float` arguments: their fp32 values are the inputs of the reference too (1 - beta is then exact in fp32 as well).
    -> dict p, m, v, B_p, B_m (= |beta1 m| + |(1 - beta1) g|).  The model multiplies gscale by the device-side factor in fp32 first, as
    csrc/elementwise.hip adamw_k does (`gscale *= *gscale_dev`), and takes the bias corrections as fp32 values (mh_adamw: 1.0f - powf(beta, step))."""
    wt = _wt(model)
    lr, beta1, beta2, eps, wd, gscale = (_f32(x) for x in (lr, beta1, beta2, eps, wd, gscale))
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    if gscale_dev is not None:
        gscale = gscale * _f32(gscale_dev)
    if model is not None:
        gscale, bc1, bc2 = _f32(gscale), _f32(bc1), _f32(bc2)
    P, G, M, Vv = p.to(wt), g.to(wt) * gscale, m.to(wt), v.to(wt)
    mn = beta1 * M + (1 - beta1) * G
    vn = beta2 * Vv + (1 - beta2) * G * G
    decayed, upd = P * (1 - lr * wd), lr * (mn / bc1) / (torch.sqrt(vn / bc2) + eps)
    # B_p: nothing in the update is rounded to 16 bits, but its two terms can cancel (a weight crossing zero): each carries a few fp32
    # roundings (products, quotient, square root: 8 in all), which count against a result far smaller than either term
    Bp = (decayed.abs() + upd.abs()) * (8 * EPS16[torch.float32] / EPS16.get(p.dtype, EPS16[torch.float32]))
    return {"p": r16(decayed - upd, model), "m": mn, "v": vn, "B_p": Bp, "B_m": (beta1 * M).abs() + ((1 - beta1) * G).abs()}


def resolvable(p_new64, p_old, tol):
    """Fraction of elements whose reference step |p_new - p_old| exceeds 8 x the tolerance they are checked with: below that a kernel that does
    nothing at all passes.  tol: tensor, the absolute tolerance per element."""
    return float(((p_new64 - p_old.double()).abs() > 8 * tol).double().mean())


# Hyper-parameters chosen so that ONE step is resolvable in bf16 (a step must exceed 8 x 2 x 2^-8 = 6 % of |p|) and so that the decay alone
# (lr * wd = 5 % of |p| per step) is: the model's real weights (sigma 0.02) and a tensor of ones standing for norm weights.
ADAMW_CASES = {"weights": dict(sigma=0.02, offset=0.0, lr=4e-3, wd=12.5), "norm weights (ones)": dict(sigma=0.0, offset=1.0, lr=0.1, wd=0.5)}


def adamw_inputs(case, n, dtype, step):
    c = ADAMW_CASES[case]
    gen = torch.Generator().manual_seed(n)
    p0 = (c["offset"] + c["sigma"] * torch.randn(n, generator=gen)).to(dtype)
    base = torch.randn(n, generator=gen).abs() * 1e-2 * torch.where(p0.float() < 0, -1.0, 1.0)
    # a consistent direction, towards zero: |m^| / sqrt(v^) stays near 1, every step is a full lr, and |p| (the scale of the tolerance) never grows
    g = (base * (1 + 0.1 * math.sin(step))).to(dtype)
    return p0, g
