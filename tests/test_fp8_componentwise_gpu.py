"""The 8-wave scaled-fp8 GEMM (csrc/gemm256.hip, mh_gemm_force_kernel(256)) and the fp8-weight GEMV of the decode step (csrc/decode.hip
mh_gemv_fp8w) element by element against float64 references built from the EXACTLY dequantised operands (tests/numerics.py, fp8 section).
The fused fp8 forms (RoPE, SwiGLU forward / backward, amax, rmsnorm + q8; gemv_fp8w_norm, SwiGLU, q|k|v + RoPE with fp8 weights) are tied bit
for bit to "unfused product + stand-alone kernel" elsewhere in the suite; this file is what holds the unfused products themselves.

GEMM:  |got - want| <= ulp_out(want) + C_ACC 2^-24 sum_k |a_k b_k| + epilogue terms (numerics.gemm_fp8), every epilogue kind, three forms of
       weight scales (per row; exponent image all zero = the constant-scale loop; exponents 2^-((n + kb) % 4) that differ between neighbouring
       rows and blocks), the training products (dgrad, wgrad over a zero-filled token tail, SwiGLU backward with maxima).
GEMV:  numerics.componentwise with limit(c_model), every arm of the launcher, which arm a case takes asserted from the launcher's own conditions.
Every launch runs twice and must repeat its bits.  Lines printed: `F8 | ...` (GEMM: worst (|d| - ulp) / (2^-24 sum|ab|)) and `CW | ...` (GEMV)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import numerics as N  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
F32 = torch.float32


def dev():
    return torch.device("cuda:0")


def rnd(*shape, dtype=torch.bfloat16, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev())


@pytest.fixture(scope="module")
def ops():
    from merlin_amd import ops as O

    assert O.arch_ok(0), "not a gfx950 device"
    return O


@pytest.fixture
def eight_wave(ops):
    ops.gemm_force_kernel(256)
    try:
        yield ops
    finally:
        ops.gemm_force_kernel(0)


def twice(fn):
    """fn() two times: the launches must be bit-identical."""
    a, b = fn(), fn()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert torch.equal(x, y), "two launches of the same product differ"
    return a


def hold_f8(name, got, want, err, od, cond=None):
    """Print the worst excess over the output's own ulp in units of 2^-24 sum|ab| (the figure C_ACC bounds), then assert the bound."""
    if cond is not None:
        d = ((got.double() - want).abs() - N.ulp(want, od)).clamp_min(0) / (N.U24 * cond).clamp_min(1e-300)
        print(f"F8 | {name} | {str(od)[6:]} | worst (|d| - ulp) / (2^-24 sum|ab|) = {float(d.max()):.1f} | C_ACC = {N.C_ACC}")
    N.check(name, got, want, err, od)


def block_pow2(Nr, nkb):
    """e[n, kb] = (n + kb) % 4: neighbouring rows and neighbouring blocks differ."""
    return (torch.arange(Nr)[:, None] + torch.arange(nkb)[None, :]) % 4


def weight_forms(ops, w, form):
    """-> b8 for gemm_fp8.  rows: per-row scales only.  e0: the quantiser's exponent image with every exponent zero (each block holds an element
    as large as the row's maximum), header flag 0 = the constant-scale loop.  exp: exponents (n + kb) % 4 written into the image by hand,
    block scale sb[n] 2^-e (any bytes with any exponents are a valid operand; one wrong exponent moves a whole row of outputs)."""
    Nr, K = w.shape
    if form == "rows":
        return ops.quant_fp8_rows(w)
    if form == "e0":
        w = w.clone()
        w[:, ::128] = w.float().abs().amax(1, keepdim=True).to(w.dtype)
        q, s, ex = ops.quant_fp8_rows_e4(w)
        assert int(ex[:4].view(torch.int32)) == 0 and not bool(ex[16:].any()), "every block reaches the row maximum: no exponent, flag 0"
        return q, s, ex
    q, s = ops.quant_fp8_rows(w)
    ex = N.exp_image(block_pow2(Nr, K // 128), dev())
    assert ex.numel() == ops._exp_image(Nr, K, dev()).numel() and int(ex[:4].view(torch.int32)) == 1
    return q, s, ex


# (M, N, K): one K-tile (the K loop is prologue and epilogue only); one full tile; an odd K-tile count with ragged M and N; N % 4 != 0 (the scalar
# store path); 65 blocks (the exponent group is padded from 4160 to 8192 bytes)
GEMM_SHAPES = [(1, 8, 128), (256, 256, 256), (300, 264, 384), (72, 262, 256), (64, 136, 8320)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["rows", "e0", "exp"])
@pytest.mark.parametrize("M,Nn,K", GEMM_SHAPES)
def test_fp8_gemm_8wave_every_epilogue_per_element(eight_wave, dtype, form, M, Nn, K):
    ops = eight_wave
    x, w = rnd(M, K, dtype=dtype), rnd(Nn, K, dtype=dtype, seed=1, scale=K ** -0.5)  # pre-activations of order 1: quick-GELU in its curved region
    bias, resid, old = rnd(Nn, dtype=dtype, seed=2), rnd(M, Nn, dtype=dtype, seed=3), rnd(M, Nn, dtype=dtype, seed=4)
    old32 = old.float() * 3
    a8, b8 = ops.quant_fp8_rows(x), weight_forms(ops, w, form)
    cond = N.deq64(a8).abs() @ N.deq64_any(b8).abs().t()
    tag = f"{M}x{Nn}x{K} {form}"

    def check(name, run, od=dtype, **kw):
        want, err = N.gemm_fp8(a8, b8, out_dtype=od, **kw)
        hold_f8(f"8-wave {name} {tag}", twice(run), want, err, od, cond if not kw else None)

    check("plain", lambda: ops.gemm_fp8(a8, b8, out_dtype=dtype))
    check("bias", lambda: ops.gemm_fp8(a8, b8, out_dtype=dtype, bias=bias), bias=bias)
    check("bias+gelu", lambda: ops.gemm_fp8(a8, b8, out_dtype=dtype, bias=bias, act="quick_gelu"), bias=bias, gelu=True)
    check("residual", lambda: ops.gemm_fp8(a8, b8, out_dtype=dtype, resid=resid), resid=resid)
    check("bias+residual", lambda: ops.gemm_fp8(a8, b8, out_dtype=dtype, bias=bias, resid=resid), bias=bias, resid=resid)
    check("accumulate", lambda: ops.gemm_fp8(a8, b8, out=old.clone(), accum=True), c_old=old)
    check("fp32 store", lambda: ops.gemm_fp8(a8, b8, out=torch.empty(M, Nn, dtype=F32, device=dev()), dt16=dtype), od=F32)
    check("fp32 accumulate", lambda: ops.gemm_fp8(a8, b8, out=old32.clone(), accum=True, dt16=dtype), od=F32, c_old=old32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_gemm_8wave_second_tile_of_a_persistent_block_restages_its_exponents(eight_wave, dtype):
    """17 x 17 = 289 tiles for 256 CUs: a persistent block takes a second tile, whose exponent image it stages under the first tile's store
    phase.  Per element, and bit for bit against the one-block-per-tile launch."""
    ops = eight_wave
    M = Nn = 4352
    K = 256
    x, w = rnd(M, K, dtype=dtype), rnd(Nn, K, dtype=dtype, seed=1, scale=K ** -0.5)
    a8, b8 = ops.quant_fp8_rows(x), weight_forms(ops, w, "exp")
    try:
        ops.gemm_persistent(0)
        one_per_tile = ops.gemm_fp8(a8, b8, out_dtype=dtype)
        ops.gemm_persistent(1)
        got = twice(lambda: ops.gemm_fp8(a8, b8, out_dtype=dtype))
    finally:
        ops.gemm_persistent(1)
    assert torch.equal(got, one_per_tile)
    want, err = N.gemm_fp8(a8, b8, out_dtype=dtype)
    hold_f8(f"8-wave plain {M}x{Nn}x{K} exp persistent", got, want, err, dtype, err / N.C_ACC / N.U24)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_training_products_8wave_per_element(eight_wave, dtype):
    """dgrad against the transposed weight with block exponents, wgrad over T = 1000 tokens (Tp = 1024: the zero-filled tail contributes
    nothing), fresh and accumulating."""
    ops = eight_wave
    T, No, Ki = 1000, 384, 264
    dy, x = rnd(T, No, dtype=dtype, scale=0.3), rnd(T, Ki, dtype=dtype, seed=1, scale=0.5)
    w = rnd(No, Ki, dtype=dtype, seed=2, scale=0.05).float()
    # transposed form: row = input channel c, block = 128 output channels; scale them so that the quantiser itself finds exponents that matter
    w = (w.view(No // 128, 128, Ki) * torch.ldexp(torch.ones(No // 128, Ki), -block_pow2(Ki, No // 128).t().to(torch.int32)).to(dev())[:, None, :]).view(No, Ki).to(dtype)
    dy8, wT8 = ops.quant_fp8_rows(dy), ops.quant_fp8_rows_t_e4(w)
    assert wT8[0].shape == (Ki, No) and int(wT8[2][:4].view(torch.int32)) == 1
    _, e = N.deq64_e4(*wT8)
    assert int(e.max()) >= 2 and bool((e[:, 0] != e[:, 1]).any()) and bool((e[1] != e[2]).any())
    want, err = N.gemm_fp8(dy8, wT8, out_dtype=dtype)
    assert float((want - dy.double() @ w.double()).abs().max()) < 6e-2 * float(want.abs().max())  # ... and it is the product it claims to be
    hold_f8(f"8-wave dgrad {T}x{Ki}x{No}", twice(lambda: ops.gemm_fp8(dy8, wT8, out_dtype=dtype)), want, err, dtype, err / N.C_ACC / N.U24)
    # wgrad dW = dy^T x over the tokens
    dyT8, xT8 = ops.quant_fp8_rows_t(dy), ops.quant_fp8_rows_t(x)
    assert dyT8[0].shape == (No, 1024) and xT8[0].shape == (Ki, 1024) and int(dyT8[0][:, T:].max()) == 0 and int(xT8[0][:, T:].max()) == 0
    valid = lambda q8: (q8[0][:, :T].contiguous(), q8[1])  # noqa: E731  the reference never sees the tail
    want, err = N.gemm_fp8(valid(dyT8), valid(xT8), out_dtype=dtype)
    assert float((want - dy.double().t() @ x.double()).abs().max()) < 6e-2 * float(want.abs().max())
    fresh = twice(lambda: ops.gemm_fp8(dyT8, xT8, out=torch.empty(No, Ki, dtype=dtype, device=dev()), out_dtype=dtype))
    hold_f8(f"8-wave wgrad fresh {No}x{Ki}xT={T}", fresh, want, err, dtype, err / N.C_ACC / N.U24)
    old = rnd(No, Ki, dtype=dtype, seed=5)
    want, err = N.gemm_fp8(valid(dyT8), valid(xT8), out_dtype=dtype, c_old=old)
    hold_f8(f"8-wave wgrad accumulate {No}x{Ki}xT={T}", twice(lambda: ops.gemm_fp8(dyT8, xT8, out=old.clone(), accum=True)), want, err, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,d,ff", [(253, 128, 264), (300, 384, 520)])
def test_fp8_swiglu_backward_with_maxima_8wave_per_element(eight_wave, dtype, T, d, ff):
    """gemm_fp8_swiglu_bwd(..., want_amax=True) behind the 8-wave kernel: dgu = swiglu_bwd(gu, dact) with dact = dy Wd rounded once to the
    16-bit stage, against float64; the maxima are exactly those of the stored tensor."""
    ops = eight_wave
    dy, wd, gu = rnd(T, d, dtype=dtype, scale=0.3), rnd(d, ff, dtype=dtype, seed=1, scale=0.05), rnd(T, 2 * ff, dtype=dtype, seed=2)
    gu[:, 3] = 0
    dy[5] = 0
    dy8, wdT8 = ops.quant_fp8_rows(dy), ops.quant_fp8_rows_t(wd)
    assert wdT8[0].shape == (ff, d)
    dgu, amax = twice(lambda: ops.gemm_fp8_swiglu_bwd(dy8, wdT8, gu, want_amax=True))
    assert torch.equal(dgu, ops.gemm_fp8_swiglu_bwd(dy8, wdT8, gu))
    a = amax.view(torch.float32)
    assert torch.equal(a[:T], dgu.float().abs().amax(1)) and torch.equal(a[T:], dgu.float().abs().amax(0))
    dact, e = N.gemm_fp8(dy8, wdT8, out_dtype=dtype)
    ed = e + N.ulp(dact, dtype)  # the staged 16-bit dact
    g, u = gu[:, :ff].double(), gu[:, ff:].double()
    s = torch.sigmoid(g)
    dsilu = s * (1 + g * (1 - s))
    want = torch.cat([dact * u * dsilu, dact * g * s], 1)
    err = torch.cat([(u * dsilu).abs() * ed + N.C_OP * N.U24 * (dact * u * s).abs() * (1 + (g * (1 - s)).abs()),
                     (g * s).abs() * ed + N.C_OP * N.U24 * (dact * g * s).abs()], 1) + N.TINY_OP
    hold_f8(f"8-wave swiglu backward {T}x{ff}x{d}", dgu, want, err, dtype)
    assert float(dgu[5].abs().max()) == 0.0 and float(dgu[:, ff + 3].abs().max()) == 0.0  # zero dact row; zero gate column -> du = 0


# ---- the fp8-weight GEMV ---------------------------------------------------------------------------------------------------------------------
def gemv_arm(M, Nn, K, mfma_min, ksplit):
    """The kernel csrc/decode.hip gemv_fp8w_impl launches for a plain projection, from its own conditions (mfma_min = 3 by default, 17 = never)."""
    if M >= mfma_min and K % 64 == 0:
        return "mfma"
    assert M <= 8
    if ksplit and M <= 2 and Nn <= 8192 and K >= 2048:
        return "k-split"
    if M >= 3 and Nn >= 8192:
        return "wave per row pair"   # two weight rows per wave, activations through LDS
    return "wave per row, LDS" if M >= 3 else "wave per row"  # 1-2 rows read the activations straight from memory


# (M, N, K, MFMA row threshold, k-split, 16-wave MFMA blocks, the arm that must run).  K = 144 and 272 end in a partial 128-block; K = 2064 and
# 4112 also cross the GEMV_KC = 2048 chunk of the K loop; N = 515 leaves the last block of waves ragged; N = 8200 gives two rows per wave.
GEMV_CASES = [
    (1, 515, 272, 17, True, True, "wave per row"),
    (2, 515, 144, 17, True, True, "wave per row"),
    (1, 515, 4112, 17, False, True, "wave per row"),
    (2, 264, 2064, 17, False, True, "wave per row"),
    (2, 264, 4096, 17, False, True, "wave per row"),
    (3, 515, 272, 17, True, True, "wave per row, LDS"),
    (8, 515, 2064, 17, True, True, "wave per row, LDS"),
    (3, 515, 4112, 17, True, True, "wave per row, LDS"),
    (5, 264, 144, 0, True, True, "wave per row, LDS"),      # default threshold, K % 64 != 0: no MFMA form
    (3, 8200, 272, 17, True, True, "wave per row pair"),
    (1, 264, 2048, 0, True, True, "k-split"),
    (2, 264, 4096, 0, True, True, "k-split"),
    (1, 515, 2064, 0, True, True, "k-split"),
    (2, 515, 4112, 0, True, True, "k-split"),
    (3, 515, 2112, 0, True, True, "mfma"),
    (3, 515, 2112, 0, True, False, "mfma"),
    (8, 264, 4096, 0, True, True, "mfma"),
    (9, 515, 192, 0, True, False, "mfma"),
    (16, 515, 2112, 0, True, True, "mfma"),
    (16, 264, 4096, 0, True, False, "mfma"),
]


def block_scaled_weights(Nn, K, dtype):
    """Blocks scaled by 2^-((n + kb) % 4), one all-zero row (7) and one all-zero block (row 9, the last block)."""
    nb = (K + 127) // 128
    w = rnd(Nn, K, dtype=dtype, seed=1, scale=0.5).float()
    f = torch.ldexp(torch.ones(Nn, nb), -block_pow2(Nn, nb).to(torch.int32)).to(dev())
    w = w * f.repeat_interleave(128, dim=1)[:, :K]
    w[7] = 0
    w[9, (nb - 1) * 128:] = 0
    return w.to(dtype)


def hold(name, dtype, got, ref, B, model, od):
    cm, _ = N.componentwise(model, ref, B, N.EPS16[od], N.TINY[od])
    ck, at = N.componentwise(got, ref, B, N.EPS16[od], N.TINY[od])
    lim = N.limit(cm)
    print(f"CW | {name} | {str(dtype)[6:]} -> {str(od)[6:]} | {cm:.3f} | {ck:.3f} | {lim:.3f} | worst at {at}")
    assert ck <= lim, f"{name} {dtype}: kernel c = {ck:.3f} at {at} exceeds {lim:.3f} (model c = {cm:.3f})"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,Nn,K,mfma_min,ksplit,wide,arm", GEMV_CASES)
def test_fp8_weight_gemv_every_arm_per_element(ops, dtype, M, Nn, K, mfma_min, ksplit, wide, arm):
    assert gemv_arm(M, Nn, K, mfma_min or 3, ksplit) == arm
    nb = (K + 127) // 128
    x, resid = rnd(M, K, dtype=dtype), rnd(M, Nn, dtype=dtype, seed=2)
    qw = ops.quant_fp8_b128(block_scaled_weights(Nn, K, dtype))
    q, sc = qw
    assert float(sc[7].min()) == 1.0 == float(sc[7].max()) == float(sc[9, nb - 1]) and int(q[7].max()) == 0
    if nb >= 4:  # the scales of a row really differ from block to block (nominally by 8; a block's own maximum varies by far less)
        assert bool((sc[16:32].max(1).values >= 3 * sc[16:32].min(1).values).all())
    tag = f"gemv fp8w {arm}{'' if wide else ' (8 waves)'} {M}x{Nn}x{K}"
    try:
        ops.gemv_mfma_min_rows(mfma_min)
        ops.gemv_ksplit(ksplit)
        ops.gemv_mfma_wide(wide)
        assert M <= ops._gemv_rows_per_launch(K)  # one launch
        got16 = twice(lambda: ops.gemv_fp8w(x, qw))
        gotr = twice(lambda: ops.gemv_fp8w(x, qw, resid=resid))
        got32 = twice(lambda: ops.gemv_fp8w(x, qw, out_f32=True))
    finally:
        ops.gemv_mfma_min_rows(0)
        ops.gemv_ksplit(True)
        ops.gemv_mfma_wide(True)
    ref, B = N.gemv_fp8w(x, q, sc)
    hold(f"{tag} 16-bit", dtype, got16, ref, B, N.gemv_fp8w(x, q, sc, model=dtype), dtype)
    assert float(got16[:, 7].abs().max()) == 0.0  # the all-zero weight row
    ref, B = N.gemv_fp8w(x, q, sc, resid)
    hold(f"{tag} +resid", dtype, gotr, ref, B, N.gemv_fp8w(x, q, sc, resid, model=dtype), dtype)
    ref, B = N.gemv_fp8w(x, q, sc, out_dtype=F32)
    hold(f"{tag} fp32", dtype, got32, ref, B, N.gemv_fp8w(x, q, sc, out_dtype=F32, model=dtype), F32)
