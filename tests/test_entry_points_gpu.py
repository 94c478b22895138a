"""Exact tests of the C-ABI entry points no other GPU test calls directly (include/merlin_hip.h): the flag / index / validation kernels, the
clip coefficient, the partial-sum reduce, the conv-projector gathers, mh_gemm_nt itself, and the A/B setters documented as bit-identical."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import numerics as N  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


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


# ---- mh_any_nonzero -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 5, 8, 13, 4096, 4096 + 7, (1 << 21) + 3])
def test_any_nonzero_is_exact_on_the_bit_patterns(ops, dtype, n):
    def flag(t):
        f = torch.zeros(1, dtype=torch.int32, device=dev())
        ops.any_nonzero(t, f)
        return int(f[0])

    z = torch.zeros(n, dtype=dtype, device=dev())
    assert flag(z) == 0
    assert flag(-z) == 0 and bool((-z).view(torch.int16).ne(0).all())  # only -0: every bit pattern is 0x8000, every value is zero
    sub = torch.tensor([1], dtype=torch.int16, device=dev()).view(dtype)  # the smallest subnormal: its square underflows fp32
    for val in (sub, torch.tensor([float("nan")], dtype=dtype, device=dev()), torch.tensor([float("-inf")], dtype=dtype, device=dev())):
        for where in sorted({0, n // 2, n - 1}):  # n - 1: the last element of a length that is not a multiple of 8
            t = z.clone()
            t[where] = val[0]
            assert flag(t) == 1, (n, where, val)
    f = torch.ones(1, dtype=torch.int32, device=dev())  # the flag is OR-ed: a raised flag stays raised on zeros
    ops.any_nonzero(z, f)
    assert int(f[0]) == 1


# ---- mh_mask_lens ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 255, 256, 257, 4096])
def test_mask_lens_is_one_plus_the_last_set_position(ops, S):
    g = torch.Generator().manual_seed(S)
    rows = [torch.zeros(S, dtype=torch.bool), torch.ones(S, dtype=torch.bool)]
    for n in sorted({1, S // 2, S - 1, S} - {0}):
        m = torch.zeros(S, dtype=torch.bool)
        m[:n] = True
        rows.append(m)                                   # a prefix
        h = m.clone()
        h[torch.randint(0, n, (max(1, n // 3),), generator=g)] = False
        rows.append(h)                                   # the same with holes (possibly at position 0 or n - 1)
    one = torch.zeros(S, dtype=torch.bool)
    one[S - 1] = True
    rows.append(one)                                     # left padding down to one token
    rows.append(torch.rand(S, generator=g) < 0.01)       # sparse
    mask = torch.stack(rows)
    idx = torch.arange(1, S + 1)
    want = (mask.long() * idx).amax(1).to(torch.int32)
    for m in (mask.to(dev()), mask.to(torch.uint8).to(dev()), (mask.to(torch.uint8) * 255).to(dev())):
        assert torch.equal(ops.mask_lens(m).cpu(), want)


# ---- mh_check_inputs ---------------------------------------------------------------------------------------------------------------------
def test_check_inputs_every_slot_alone(ops):
    B, S, V = 3, 300, 1000
    g = torch.Generator().manual_seed(1)
    ids0 = torch.randint(0, V, (B, S), generator=g)
    ids0[0, 0], ids0[1, 5] = 0, V - 1                    # the two ends of the valid range
    lab0 = torch.randint(0, V, (B, S), generator=g)
    lab0[0, :7] = -100
    lab0[2, 10], lab0[2, 11] = 0, V - 1
    full = torch.ones(B, S, dtype=torch.bool)

    def run(ids=ids0, labels=lab0, mask=full, lens=None):
        err = torch.zeros(12, dtype=torch.int32, device=dev())
        d = lambda t: None if t is None else t.to(dev())  # noqa: E731
        lens_t = None if mask is None else (ops.mask_lens(mask.to(dev())) if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev()))
        ops.check_inputs(d(ids), d(labels), d(mask), lens_t, err, V)
        return err.cpu().tolist()

    clean = [0] * 12
    assert run() == clean
    for bad, (b, s) in ((V, (1, 299)), (-1, (0, 0)), (1 << 40, (2, 256)), (V + 5, (2, 17))):  # positions in every 256-thread stride
        ids = ids0.clone()
        ids[b, s] = bad
        want = list(clean)
        want[4], want[5] = 1, b * S + s
        assert run(ids=ids) == want, (bad, b, s)
        assert run(ids=ids, labels=None, mask=None) == want
        assert run(ids=None) == clean                    # NULL ids: skipped
    for bad, (b, s) in ((V, (0, 3)), (-1, (1, 299)), (-99, (2, 0)), (-101, (1, 257))):
        lab = lab0.clone()
        lab[b, s] = bad
        want = list(clean)
        want[6], want[7] = 1, b * S + s
        assert run(labels=lab) == want, (bad, b, s)
        assert run(ids=None, labels=lab, mask=None) == want
        assert run(labels=None) == clean                 # NULL labels: skipped
    # a right-padded batch: only "the batch carries padding"
    pad = full.clone()
    pad[1, 200:] = False
    want = list(clean)
    want[10] = 1
    assert run(mask=pad) == want
    assert run(ids=None, labels=None, mask=pad) == want
    assert run(mask=None) == clean                       # NULL mask: skipped (lens is not read)
    # a hole: not a prefix (popcount != 1 + last set position) - and therefore padding too
    hole = full.clone()
    hole[2, 100] = False
    want = list(clean)
    want[8], want[9], want[10] = 1, 2, 1
    assert run(mask=hole) == want
    left = full.clone()
    left[0, :50] = False                                 # left padding of sample 0
    want[9] = 0
    assert run(mask=left) == want
    # slot 8 alone: a full mask against lengths that disagree with it
    want = list(clean)
    want[8], want[9] = 1, 1
    assert run(lens=[S, S - 1, S]) == want
    # bad id AND bad label AND a hole at once: the slots do not disturb each other
    ids, lab = ids0.clone(), lab0.clone()
    ids[1, 1], lab[0, 9] = V, V
    assert run(ids=ids, labels=lab, mask=hole) == [0, 0, 0, 0, 1, S + 1, 1, 9, 1, 2, 1, 0]


# ---- mh_clip_scale -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gscale", [1.0, 0.125, -0.5, 3.0])
@pytest.mark.parametrize("max_norm", [1.0, 0.3, 1e3])
def test_clip_scale_is_torch_clip_grad_norm_coefficient(ops, gscale, max_norm):
    gen = torch.Generator().manual_seed(3)
    grads = [torch.randn(n, generator=gen) * s for n, s in ((1000, 0.01), (77, 0.1), (4096, 0.02))]
    params = [torch.nn.Parameter(torch.zeros_like(g, dtype=torch.float64)) for g in grads]
    for p_, g in zip(params, grads):
        p_.grad = g.double() * gscale
    total = float(torch.nn.utils.clip_grad_norm_(params, max_norm))           # the norm of the SCALED gradients, in fp64
    coef = min(1.0, max_norm / (total + 1e-6))
    sumsq = torch.tensor([float(sum((g.double() ** 2).sum() for g in grads))], dtype=torch.float32, device=dev())
    out2 = torch.full((2,), -1.0, dtype=torch.float32, device=dev())
    ops.clip_scale(sumsq, gscale, max_norm, out2)
    got_coef, got_norm = float(out2[0]), float(out2[1])
    # sqrtf, a product, an add and a quotient in fp32 on an fp32 input: 8 ulps
    assert abs(got_norm - total) <= 8 * 2.0 ** -24 * total
    assert abs(got_coef - coef) <= 8 * 2.0 ** -24 * coef and got_coef <= 1.0
    assert (got_coef == 1.0) == (total + 1e-6 <= max_norm) or abs(total - max_norm) < 1e-5 * max_norm
    applied = float(params[0].grad.abs().max() / (grads[0].double() * gscale).abs().max())  # what torch multiplied the gradients by
    assert abs(applied - got_coef) <= 1e-6 * coef


# ---- mh_reduce_partials, called directly ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("nblk,d", [(1, 8), (7, 264), (33, 40), (128, 4096), (1000, 1024), (1024, 100)])
def test_reduce_partials_fresh_and_accumulating(ops, out_dtype, nblk, d):
    part = (torch.randn(nblk, d, generator=torch.Generator().manual_seed(nblk + d)) * 2).to(dev())
    part[:, 0] = part[:, 0].abs()                        # one column without cancellation, the rest with
    old = rnd(d, dtype=out_dtype, seed=1) if out_dtype != torch.float32 else torch.randn(d, generator=torch.Generator().manual_seed(2)).to(dev())
    mdt = out_dtype
    for acc in (False, True):
        out = old.clone()
        ops.reduce_partials(part, nblk, d, out, acc)
        ref, Bc = N.reduce_rows(part, old if acc else None)
        mod = N.reduce_rows(part, old if acc else None, model=mdt)
        # in units of the output type: a 16-bit output is ONE rounding of an fp32 sum (B enters with nblk fp32 roundings), an fp32 output is the sum itself
        scale = (nblk + 1) * N.EPS16[torch.float32] / N.EPS16[out_dtype]
        cm = N.componentwise(mod, ref, Bc * scale, N.EPS16[out_dtype], N.TINY[out_dtype])[0]
        ck, at = N.componentwise(out, ref, Bc * scale, N.EPS16[out_dtype], N.TINY[out_dtype])
        print(f"CW | reduce_partials {nblk}x{d}{' accumulate' if acc else ''} | {str(out_dtype)[6:]} | {cm:.3f} | {ck:.3f} | {N.limit(cm):.3f} | worst at {at}")
        assert ck <= N.limit(cm), (ck, cm, at)


# ---- mh_conv3x3_cols / mh_conv3x3_col2im -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N_,G,C,stride,row0,extra", [(2, 5, 8, 1, 1, 0), (1, 6, 24, 2, 1, 0), (3, 7, 16, 2, 1, 0), (2, 4, 8, 1, 0, 0), (2, 24, 64, 2, 1, 0), (1, 5, 8, 2, 2, 3)])
def test_conv3x3_gathers_against_unfold_and_its_autograd(ops, dtype, N_, G, C, stride, row0, extra):
    rpi = row0 + G * G + extra                           # CLS rows in front, spare rows behind
    Go = (G + 2 - 3) // stride + 1
    x = rnd(N_ * rpi, C, dtype=dtype)
    cols = ops.conv3x3_cols(x, N_, G, C, stride, rpi, row0)
    img = x.view(N_, rpi, C)[:, row0:row0 + G * G].reshape(N_, G, G, C).permute(0, 3, 1, 2).double().requires_grad_()
    unf = torch.nn.functional.unfold(img, 3, padding=1, stride=stride)          # [N, C * 9, Go * Go], k = c * 9 + ky * 3 + kx
    want = unf.transpose(1, 2).reshape(N_ * Go * Go, C * 9)
    assert cols.shape == want.shape and torch.equal(cols.double(), want.detach())  # a gather: bit for bit
    dcols = rnd(N_ * Go * Go, C * 9, dtype=dtype, seed=3)
    dx = ops.conv3x3_col2im(dcols, N_, G, C, stride, rpi, row0).view(N_, rpi, C)

    def fold(dc):                                         # autograd of that unfold, channels last
        gimg, = torch.autograd.grad(unf, img, dc.view(N_, Go * Go, C * 9).transpose(1, 2), retain_graph=True)
        return gimg.permute(0, 2, 3, 1).reshape(N_, G * G, C)
    ref, Bc = fold(dcols.double()), fold(dcols.double().abs())
    mod = N.r16(ref.float(), dtype)                       # at most nine 16-bit terms: exact in fp32, ONE rounding
    patch = dx[:, row0:row0 + G * G]
    Bc = Bc * (9 * N.EPS16[torch.float32] / N.EPS16[dtype])  # nine fp32 additions of exact terms
    cm = N.componentwise(mod, ref, Bc, N.EPS16[dtype], N.TINY[dtype])[0]
    ck, at = N.componentwise(patch, ref, Bc, N.EPS16[dtype], N.TINY[dtype])
    print(f"CW | conv3x3 col2im G={G} C={C} stride={stride} | {str(dtype)[6:]} | {cm:.3f} | {ck:.3f} | {N.limit(cm):.3f} | worst at {at}")
    assert ck <= N.limit(cm), (ck, cm, at)
    rest = torch.ones(rpi, dtype=torch.bool)
    rest[row0:row0 + G * G] = False
    assert float(dx[:, rest.to(dev())].float().abs().max() if bool(rest.any()) else 0.0) == 0.0  # non-patch rows exactly zero


# ---- mh_gemm_nt itself (ops.gemm_nt goes through the general mh_gemm) ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N_,K", [(200, 328, 512), (613, 4096, 1024), (300, 103, 64)])
def test_gemm_nt_entry_point(ops, dtype, M, N_, K):
    from merlin_amd import _lib as L

    a, b = rnd(M, K, dtype=dtype), rnd(N_, K, dtype=dtype, seed=1, scale=0.5)
    bias, resid = rnd(N_, dtype=dtype, seed=2), rnd(M, N_, dtype=dtype, seed=3)
    for kw, epi in (({}, 0), ({"bias": bias, "resid": resid}, ops.EPI_BIAS | ops.EPI_RESIDUAL)):
        if kw and N_ % 4:
            continue  # (the staged epilogues take N % 4 == 0, as everywhere in tests/test_ops_gpu.py)
        out = torch.empty(M, N_, dtype=dtype, device=dev())
        L.call("mh_gemm_nt", a, K, b, K, out, N_, kw.get("bias"), kw.get("resid"), N_ if kw else 0, M, N_, K, ops.dt_of(a), epi, ops._stream())
        ref, Bc = N.gemm(a, b, **kw)
        mod = N.gemm(a, b, model=dtype, **kw)
        cm = N.componentwise(mod, ref, Bc, N.EPS16[dtype], N.TINY[dtype])[0]
        ck, at = N.componentwise(out, ref, Bc, N.EPS16[dtype], N.TINY[dtype])
        print(f"CW | mh_gemm_nt {M}x{N_}x{K}{' bias+resid' if kw else ''} | {str(dtype)[6:]} | {cm:.3f} | {ck:.3f} | {N.limit(cm):.3f} | worst at {at}")
        assert ck <= N.limit(cm), (ck, cm, at)
        L.call("mh_gemm", a, K, 0, b, K, 0, (same := torch.empty_like(out)), N_, kw.get("bias"), kw.get("resid"), N_ if kw else 0, M, N_, K, ops.dt_of(a), epi, ops._stream())
        assert torch.equal(out.view(torch.int16), same.view(torch.int16))  # the NT form IS mh_gemm with both operands K-contiguous


# ---- the A/B setters documented as bit-identical arms ----------------------------------------------------------------------------------------
def _gemm_results(ops, dtype):
    """A few products with edge tiles, below and above 256 output tiles (one persistent round of the 256 CUs), through the auto selection and
    each forced kernel, with a plain and a staged epilogue."""
    res = []
    for M, N_, K in ((1000, 520, 256), (200, 328, 512), (4104, 4360, 128), (8200, 2056, 64)):
        a, b = rnd(M, K, dtype=dtype), rnd(N_, K, dtype=dtype, seed=1, scale=0.5)
        bias, resid = rnd(N_, dtype=dtype, seed=2), rnd(M, N_, dtype=dtype, seed=3)
        bt = b.t().contiguous()
        for which in (0, 128, 256, 4):
            try:
                ops.gemm_force_kernel(which)
                res += [ops.gemm_nt(a, b), ops.gemm_nt(a, b, bias=bias, resid=resid), ops.gemm_nt(a, bt, b_t=True), ops.gemm_nt(a, b, out_f32=True)]
            finally:
                ops.gemm_force_kernel(0)
    return res


def _same_bits(xs, ys):
    return len(xs) == len(ys) and all(x.dtype == y.dtype and torch.equal(x.view(torch.int32 if x.dtype == torch.float32 else torch.int16),
                                                                         y.view(torch.int32 if y.dtype == torch.float32 else torch.int16)) for x, y in zip(xs, ys))


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_persistent_and_raster_group_arms_are_bit_identical(ops, dtype):
    base = _gemm_results(ops, dtype)
    assert _same_bits(base, _gemm_results(ops, dtype))   # run to run first
    try:
        ops.gemm_persistent(False)
        assert _same_bits(base, _gemm_results(ops, dtype)), "gemm_persistent(False)"
    finally:
        ops.gemm_persistent(True)
    for gm in (1, 2, 8, 16):
        try:
            ops.gemm_raster_group(gm)
            assert _same_bits(base, _gemm_results(ops, dtype)), f"gemm_raster_group({gm})"
            ops.gemm_persistent(False)
            assert _same_bits(base, _gemm_results(ops, dtype)), f"gemm_raster_group({gm}) + gemm_persistent(False)"
        finally:
            ops.gemm_raster_group(0)
            ops.gemm_persistent(True)
    assert _same_bits(base, _gemm_results(ops, dtype))   # and the defaults are back


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,S,H,D,causal,lens", [(2, 613, 2, 128, True, None), (3, 577, 2, 64, False, None), (1, 1024, 1, 128, True, None), (2, 300, 2, 128, True, [300, 177]),
                                                    (2, 300, 2, 128, False, [300, 177]), (2, 200, 2, 64, True, [200, 130])])
def test_attn_wide_stores_arm_is_bit_identical(ops, dtype, B, S, H, D, causal, lens):
    qkv = rnd(B * S, 3 * H * D, dtype=dtype)
    q, k, v = (qkv[:, i * H * D:(i + 1) * H * D] for i in range(3))
    do = rnd(B * S, H * D, dtype=dtype, seed=9)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev()) if lens else None

    def run():
        o, lse = ops.attn_fwd2(q, k, v, B, S, H, D, causal, seqlens=lens_t)
        out = [o, lse]
        for spill in (False, True):
            out += list(ops.attn_bwd2(q, k, v, o, do, lse, B, S, H, D, causal, seqlens=lens_t, spill=spill))
        return out
    base = run()
    try:
        ops.attn_wide_stores(False)
        narrow = run()
    finally:
        ops.attn_wide_stores(True)
    assert _same_bits(base, narrow)
    assert _same_bits(base, run())
