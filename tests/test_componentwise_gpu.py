"""Every kernel family against its fp64 reference PER ELEMENT (tests/numerics.py): |got - ref| <= limit * eps16 * (|ref| + B), the limit taken
from the rounding model evaluated here, on the same inputs, with torch - never from a kernel.  Shapes are the suite's own (test_ops_gpu.py,
test_geometry_gpu.py); bf16 and fp16.  Each check prints `CW | operation | dtype | c_model | c_kernel | limit` before it asserts."""
import math
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


def hold(name, dtype, got, ref, B, model, out_dtype=None):
    """Measure the model's c and the kernel's c with the same reference and B, print both, assert kernel <= limit(model)."""
    od = dtype if out_dtype is None else out_dtype
    cm, _ = N.componentwise(model, ref, B, N.EPS16[od], N.TINY[od])
    ck, at = N.componentwise(got, ref, B, N.EPS16[od], N.TINY[od])
    lim = N.limit(cm)
    print(f"CW | {name} | {str(dtype)[6:]} | {cm:.3f} | {ck:.3f} | {lim:.3f} | worst at {at}")
    assert ck <= lim, f"{name} {dtype}: kernel c = {ck:.3f} at {at} exceeds {lim:.3f} (model c = {cm:.3f})"
    return ck


# ---- attention ------------------------------------------------------------------------------------------------------------------------
def _heads(t, B, S, H, D):
    """[B*S, H*D] view -> list of per-(b, h) [S, D] slices, (b, h) order."""
    return [t[b * S:(b + 1) * S, h * D:(h + 1) * D] for b in range(B) for h in range(H)]


def _attention_refs(q, k, v, do, B, S, H, D, causal, lens, dtype):
    refs, mods = [], []
    lens = lens if lens else [S] * B
    for i, (qq, kk, vv, dd) in enumerate(zip(*(_heads(t, B, S, H, D) for t in (q, k, v, do)))):
        n = lens[i // H]
        refs.append(N.attention(qq, kk, vv, dd, causal=causal, n_valid=n))
        mods.append(N.attention(qq, kk, vv, dd, causal=causal, n_valid=n, model=dtype))
    return refs, mods


def _hold_heads(name, dtype, got, refs, mods, nm, B, S, H, D):
    ref = torch.stack([r[nm] for r in refs])
    Bc = torch.stack([r["B_o"] if nm == "o" else N.f16_subnormal_B(r, nm, dtype) for r in refs])
    mod = torch.stack([m[nm] for m in mods])
    return hold(name, dtype, torch.stack(_heads(got, B, S, H, D)), ref, Bc, mod)


def _mask_tag(D, causal):
    """The mask in a printed name, where it is not the model's own for this head dim (causal at D = 128, none at D = 64)."""
    return "" if causal == (D == 128) else (" causal" if causal else " non-causal")


ATTN_CASES = [
    # the causal D = 128 shapes of test_attention_fwd_bwd (with its ragged lengths), the non-causal D = 64 tower shape, the benchmark lengths
    (1, 128, 1, 128, True, None), (2, 613, 2, 128, True, None), (2, 300, 2, 128, True, [300, 177]), (2, 40, 2, 128, True, [29, 40]),
    (1, 1024, 1, 128, True, None), (3, 577, 2, 64, False, None), (1, 17, 2, 64, False, None), (2, 577, 2, 64, False, [577, 300]),
    (1, 4096, 2, 128, True, None), (1, 8192, 1, 128, True, None), (1, 4096, 1, 128, True, [4001]),
    # the other two (head dim, mask) combinations the library dispatches: D = 128 without a mask (a tower with 128-wide heads), D = 64 causal
    # (a decoder with 64-wide heads) - ragged, one row past a 128- / 256-row block, fewer rows than one tile
    (2, 300, 2, 128, False, [300, 177]), (1, 257, 2, 128, False, None), (2, 200, 2, 64, True, [200, 130]), (1, 129, 2, 64, True, None),
    (1, 17, 2, 64, True, None)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,S,H,D,causal,lens", ATTN_CASES)
def test_attention_forward_and_backward_per_element(ops, dtype, B, S, H, D, causal, lens):
    qkv = rnd(B * S, 3 * H * D, dtype=dtype)
    q, k, v = (qkv[:, i * H * D:(i + 1) * H * D] for i in range(3))
    do = rnd(B * S, H * D, dtype=dtype, seed=9)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev()) if lens else None
    refs, mods = _attention_refs(q, k, v, do, B, S, H, D, causal, lens, dtype)
    tag = f"S={S} D={D}{_mask_tag(D, causal)}{' ragged' if lens else ''}"
    o, lse = ops.attn_fwd2(q, k, v, B, S, H, D, causal, seqlens=lens_t)
    _hold_heads(f"attention o {tag}", dtype, o, refs, mods, "o", B, S, H, D)
    if D == 128:  # all three forward forms (mh_attn_fwd_pingpong 0 / 1 / 2)
        try:
            for form in (1, 2):
                ops.attn_fwd_pingpong(form)
                of, _ = ops.attn_fwd2(q, k, v, B, S, H, D, causal, seqlens=lens_t)
                _hold_heads(f"attention o form {form} {tag}", dtype, of, refs, mods, "o", B, S, H, D)
        finally:
            ops.attn_fwd_pingpong(0)
    five = causal and D == 128 and S % 128 == 0 and not lens
    for spill in ((False, True) if five else (False,)):
        dq, dk, dv = ops.attn_bwd2(q, k, v, o, do, lse, B, S, H, D, causal, seqlens=lens_t, spill=spill)
        if D == 128 and causal:
            assert ops.LAST_ATTN_BWD_FORM == ("five-product" if spill else "seven-product")
        form = "5-product" if spill else "7-product"
        for nm, g in (("dv", dv), ("dk", dk), ("dq", dq)):
            _hold_heads(f"attention {nm} {form} {tag}", dtype, g, refs, mods, nm, B, S, H, D)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,D,Smax,lens", [(2, 2, 128, 40, [17, 40]), (3, 4, 64, 700, [1, 333, 700]), (1, 32, 128, 4200, [4100])])
def test_decode_attention_per_element(ops, dtype, B, H, D, Smax, lens):
    d = H * D
    kc, vc, q = rnd(B, Smax, d, dtype=dtype, seed=3), rnd(B, Smax, d, dtype=dtype, seed=4), rnd(B, d, dtype=dtype, seed=5)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev())
    pairs = [N.attention_decode(q[b].view(H, D), kc[b].view(Smax, H, D), vc[b].view(Smax, H, D), lens[b]) for b in range(B)]
    ref, Bc = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    mod = torch.stack([N.attention_decode(q[b].view(H, D), kc[b].view(Smax, H, D), vc[b].view(Smax, H, D), lens[b], model=dtype) for b in range(B)])
    for split in (True, False):
        o = ops.attn_decode(q, kc, vc, lens_t, H, D, split_kv=split)
        hold(f"attention decode {'split-KV' if split else 'one block'} Smax={Smax}", dtype, o.view(B, H, D), ref, Bc, mod)


# ---- GEMM / GEMV ------------------------------------------------------------------------------------------------------------------------
def four_wave_kernel_ran(ops, run):
    """Did the automatic kernel selection send run() (-> its result tensor) to the 4-wave 256 x 256 kernel?  Its result then has the bits of the
    forced 4-wave run and not those of the forced 8-wave run (their 16-bit accumulate epilogues round differently, see numerics.gemm)."""
    try:
        ops.gemm_force_kernel(0)
        auto = run()
        ops.gemm_force_kernel(4)
        w4 = run()
        ops.gemm_force_kernel(256)
        w8 = run()
    finally:
        ops.gemm_force_kernel(0)
    return torch.equal(auto, w4) and not torch.equal(auto, w8)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", [0, 128, 256, 4])
@pytest.mark.parametrize("M,Nn,K", [(200, 328, 512), (1000, 520, 256), (304, 520, 256), (2064, 1288, 128), (616, 4096, 1024)])
def test_gemm_layouts_and_epilogues_per_element(ops, dtype, which, M, Nn, K):
    """NT / NN / TN / TT, every epilogue, edge tiles in both dimensions; automatic selection and the forced 128 / 256 / 4-wave kernels."""
    a, b = rnd(M, K, dtype=dtype), rnd(Nn, K, dtype=dtype, seed=1, scale=0.5)
    bias, resid, old = rnd(Nn, dtype=dtype, seed=2), rnd(M, Nn, dtype=dtype, seed=3), rnd(M, Nn, dtype=dtype, seed=4)
    old32 = old.float() * 3
    at, bt = a.t().contiguous(), b.t().contiguous()
    tag = f"{M}x{Nn}x{K} kernel {which or 'auto'}"

    def check(name, got, out_dtype=None, **kw):
        ref, Bc = N.gemm(a, b, out_dtype=out_dtype, **kw)
        hold(f"gemm {name} {tag}", dtype, got, ref, Bc, N.gemm(a, b, model=dtype, out_dtype=out_dtype, **kw), out_dtype=out_dtype)
    try:
        ops.gemm_force_kernel(which)
        check("NT", ops.gemm_nt(a, b))
        check("NN", ops.gemm_nt(a, bt, b_t=True))
        check("TN", ops.gemm_nt(at, bt, a_t=True, b_t=True))
        check("TT", ops.gemm_nt(at, b, a_t=True))
        check("bias", ops.gemm_nt(a, b, bias=bias), bias=bias)
        check("bias+gelu", ops.gemm_nt(a, b, bias=bias, act="quick_gelu"), bias=bias, gelu=True)
        check("NN resid", ops.gemm_nt(a, bt, b_t=True, resid=resid), resid=resid)
        check("bias+resid", ops.gemm_nt(a, b, bias=bias, resid=resid), bias=bias, resid=resid)
        # The 4-wave kernel's staged 16-bit accumulate rounds the product before it adds C_old (csrc/gemm_w4.hip:239 and :463; numerics.gemm,
        # staged_accumulate); every other kernel is held to the one-rounding form.  Which one the automatic selection ran is found out, not assumed.
        def accumulate():
            acc = old.clone()
            return ops.gemm_nt(at, bt, a_t=True, b_t=True, out=acc, accum=True)
        staged = which == 4 or (which == 0 and four_wave_kernel_ran(ops, accumulate))
        ops.gemm_force_kernel(which)
        check(f"TN accumulate{' (4-wave staged)' if staged else ''}", accumulate(), c_old=old, staged_accumulate=staged)
        check("fp32 store", ops.gemm_nt(a, b, out_f32=True), out_dtype=F32)
        acc32 = old32.clone()
        check("fp32 accumulate+bias", ops.gemm_nt(a, b, bias=bias, out=acc32, accum=True), out_dtype=F32, bias=bias, c_old=old32)
    finally:
        ops.gemm_force_kernel(0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,No,Ki", [(27696, 1024, 1024), (1731, 1024, 256), (130, 512, 264), (64, 256, 256), (4100, 4096, 4096), (37, 256, 8)])
def test_wgrad_split_k_per_element(ops, dtype, T, No, Ki):
    dy, x = rnd(T, No, dtype=dtype, scale=0.5), rnd(T, Ki, dtype=dtype, seed=1, scale=0.5)
    old = rnd(No, Ki, dtype=dtype, seed=5)
    from merlin_amd import _lib as L

    splits = int(L.lib().mh_gemm_splitk_max(No, Ki, T))
    tag = f"T={T} {No}x{Ki} splits={splits}"
    out = torch.empty(No, Ki, dtype=dtype, device=dev())
    ops.wgrad_tn(dy, x, out, accum=False)
    ref, Bc = N.gemm(dy, x, a_t=True, b_t=True)
    hold(f"wgrad fresh {tag}", dtype, out, ref, Bc, N.gemm(dy, x, a_t=True, b_t=True, model=dtype))
    def accumulate():
        acc = old.clone()
        return ops.wgrad_tn(dy, x, acc, accum=True)
    # (weight gradients over >= 4096 tokens go to the 4-wave kernel by default - mh_gemm_w4_policy bit 0 - whose 16-bit accumulate is the staged form)
    staged = four_wave_kernel_ran(ops, accumulate)
    ref, Bc = N.gemm(dy, x, a_t=True, b_t=True, c_old=old, staged_accumulate=staged)
    hold(f"wgrad accumulate{' (4-wave staged)' if staged else ''} {tag}", dtype, accumulate(), ref, Bc,
         N.gemm(dy, x, a_t=True, b_t=True, c_old=old, model=dtype, staged_accumulate=staged))
    acc32 = torch.ones(No, Ki, device=dev())
    ops.wgrad_tn(dy, x, acc32, accum=True)
    one = torch.ones(No, Ki, device=dev())
    ref, Bc = N.gemm(dy, x, a_t=True, b_t=True, c_old=one, out_dtype=F32)
    hold(f"wgrad fp32 accumulate {tag}", dtype, acc32, ref, Bc, N.gemm(dy, x, a_t=True, b_t=True, c_old=one, model=dtype, out_dtype=F32), out_dtype=F32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,Nn,K", [(613, 4096, 4096), (577, 1024, 4096), (40, 4096, 12288)])
def test_skinny_gemm_split_k_with_epilogue_per_element(ops, dtype, M, Nn, K):
    """ops.gemm_nt's split-K path for few output tiles (bf16 by default), epilogue applied by the reduce pass."""
    a, b = rnd(M, K, dtype=dtype), rnd(Nn, K, dtype=dtype, seed=1, scale=0.5)
    bias, resid = rnd(Nn, dtype=dtype, seed=2), rnd(M, Nn, dtype=dtype, seed=3)
    ref, Bc = N.gemm(a, b, bias=bias, resid=resid)
    hold(f"gemm skinny bias+resid {M}x{Nn}x{K}", dtype, ops.gemm_nt(a, b, bias=bias, resid=resid), ref, Bc, N.gemm(a, b, bias=bias, resid=resid, model=dtype))
    ref, Bc = N.gemm(a, b, bias=bias, gelu=True)
    hold(f"gemm skinny bias+gelu {M}x{Nn}x{K}", dtype, ops.gemm_nt(a, b, bias=bias, act="quick_gelu"), ref, Bc, N.gemm(a, b, bias=bias, gelu=True, model=dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,Nn,K", [(1, 4096, 4096), (2, 515, 264), (8, 12288, 4096), (5, 32003, 256), (11, 1024, 11008), (16, 4096, 4096)])
def test_gemv_both_forms_per_element(ops, dtype, M, Nn, K):
    """The wave-per-row form (1-2 rows, and every row count with the MFMA threshold at 17) and the MFMA form (3-16 rows)."""
    x, w, resid = rnd(M, K, dtype=dtype), rnd(Nn, K, dtype=dtype, seed=1, scale=0.5), rnd(M, Nn, dtype=dtype, seed=2)
    ref, Bc = N.gemm(x, w, resid=resid)
    mod = N.gemm(x, w, resid=resid, model=dtype)
    ref32, B32 = N.gemm(x, w, out_dtype=F32)
    mod32 = N.gemm(x, w, model=dtype, out_dtype=F32)
    try:
        for thr, form in ((0, "default"), (17, "wave-per-row")):
            if thr == 17 and M > 8 and K % 32:
                continue
            ops.gemv_mfma_min_rows(thr)
            hold(f"gemv {form} +resid {M}x{Nn}x{K}", dtype, ops.gemv(x, w, resid=resid), ref, Bc, mod)
            hold(f"gemv {form} fp32 {M}x{Nn}x{K}", dtype, ops.gemv(x, w, out_f32=True), ref32, B32, mod32, out_dtype=F32)
    finally:
        ops.gemv_mfma_min_rows(0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", [0, 256, 4])
def test_gemm_fused_epilogues_per_element(ops, dtype, which):
    """RoPE, SwiGLU (forward, backward) and quick-GELU (forward, backward) in the GEMM's store phase, against the fp64 function of the fp64 product."""
    try:
        ops.gemm_force_kernel(which)
        tag = f"kernel {which or 'auto'}"
        # RoPE: q|k|v projection, q and k heads rotated at row % S
        Bn, S, H, D, K = 2, 96, 2, 128, 256
        x, w = rnd(Bn * S, K, dtype=dtype), rnd(3 * H * D, K, dtype=dtype, seed=1, scale=0.5)
        tab = ops.rope_table(S, D, 10000.0, dev())
        got = ops.gemm_nt_rope(x, w, tab, S, H, D)
        y64, By = N.gemm(x, w)
        qk64 = y64[:, :2 * H * D].reshape(Bn * S, 2 * H, D)
        ref = torch.cat([N.rope(qk64, tab, S).reshape(Bn * S, -1), y64[:, 2 * H * D:]], 1)
        Bc = torch.cat([N.rope_cond(qk64, tab, S).reshape(Bn * S, -1), By[:, 2 * H * D:]], 1)
        y16 = N.gemm(x, w, model=dtype)
        mod = torch.cat([N.rope(y16[:, :2 * H * D].reshape(Bn * S, 2 * H, D).to(dtype), tab, S, model=dtype).reshape(Bn * S, -1), y16[:, 2 * H * D:]], 1)
        hold(f"gemm+rope {tag}", dtype, got, ref, Bc, mod)
        # SwiGLU forward and backward
        M, ff, K = 1000, 1408, 256
        x, wgu = rnd(M, K, dtype=dtype), rnd(2 * ff, K, dtype=dtype, seed=1, scale=0.5)
        gu, act = ops.gemm_swiglu_fwd(x, wgu)
        gu64, Bgu = N.gemm(x, wgu)
        hold(f"gemm+swiglu gu {tag}", dtype, gu, gu64, Bgu, N.gemm(x, wgu, model=dtype))
        hold(f"gemm+swiglu act {tag}", dtype, act, N.swiglu_fwd(gu64), N.swiglu_fwd_cond(gu64, Bgu), N.swiglu_fwd(N.gemm(x, wgu, model=dtype).to(dtype), model=dtype))
        dy, wd = rnd(M, K, dtype=dtype, seed=2, scale=0.5), rnd(K, ff, dtype=dtype, seed=3, scale=0.5)
        dgu = ops.gemm_swiglu_bwd(dy, wd, gu)
        dact64, Bd = N.gemm(dy, wd, b_t=True)
        ref = N.swiglu_bwd(gu, dact64)  # (gu is an INPUT here, as stored; only dact carries a rounding, and the result is linear in dact)
        hold(f"gemm+swiglu bwd {tag}", dtype, dgu, ref, N.swiglu_bwd(gu, dact64.abs() + Bd).abs(), N.swiglu_bwd(gu, N.gemm(dy, wd, b_t=True, model=dtype).to(dtype), model=dtype))
        # quick-GELU forward and backward (CLIP MLP)
        T, vd, vff = 1154, 128, 256
        x, w1, b1 = rnd(T, vd, dtype=dtype), rnd(vff, vd, dtype=dtype, seed=1, scale=0.5), rnd(vff, dtype=dtype, seed=2)
        f1, a1 = ops.gemm_gelu_fwd(x, w1, b1)
        f64, Bf = N.gemm(x, w1, bias=b1)
        f16 = N.gemm(x, w1, bias=b1, model=dtype)
        hold(f"gemm+gelu f1 {tag}", dtype, f1, f64, Bf, f16)
        hold(f"gemm+gelu act {tag}", dtype, a1, N.quick_gelu_fwd(f64), N.quick_gelu_fwd_cond(f64, Bf), N.quick_gelu_fwd(f16.to(dtype), model=dtype))
        dy, w2 = rnd(T, vd, dtype=dtype, seed=3, scale=0.5), rnd(vd, vff, dtype=dtype, seed=4, scale=0.5)
        df1 = ops.gemm_gelu_bwd(dy, w2, f1)
        d64, Bd = N.gemm(dy, w2, b_t=True)
        ref = N.quick_gelu_bwd(f1, d64)
        hold(f"gemm+gelu bwd {tag}", dtype, df1, ref, N.quick_gelu_bwd(f1, d64.abs() + Bd).abs(), N.quick_gelu_bwd(f1, N.gemm(dy, w2, b_t=True, model=dtype).to(dtype), model=dtype))
    finally:
        ops.gemm_force_kernel(0)


# ---- norms, elementwise, RoPE -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,d", [(613, 4096), (37, 256), (1000, 1024), (5, 128)])
def test_rmsnorm_forward_and_backward_per_element(ops, dtype, rows, d):
    eps = 1e-5
    x, dy, old = rnd(rows, d, dtype=dtype), rnd(rows, d, dtype=dtype, seed=2), rnd(rows, d, dtype=dtype, seed=4)
    w = (1 + 0.1 * torch.randn(d, generator=torch.Generator().manual_seed(5))).to(dtype).to(dev())
    x[rows // 2] = (x[rows // 2].float() * 1e-3).to(dtype)  # a near-zero row: eps decides its scale
    tag = f"{rows}x{d}"
    for acc in (False, True):
        o = old if acc else None
        ref, mod = N.rmsnorm(x, w, eps, dy, dx_old=o), N.rmsnorm(x, w, eps, dy, dx_old=o, model=dtype)
        if not acc:
            hold(f"rmsnorm y {tag}", dtype, ops.rmsnorm_fwd(x, w, eps), ref["y"], ref["B_y"], mod["y"])
        dw = rnd(d, dtype=dtype, seed=6)
        dw_old = dw.clone()
        dx = ops.rmsnorm_bwd(x, w, dy, eps, dx=old.clone() if acc else None, accumulate_dx=acc, dw_out=dw, dw_accumulate=acc)
        hold(f"rmsnorm dx{' accumulate' if acc else ''} {tag}", dtype, dx, ref["dx"], ref["B_dx"], mod["dx"])
        dwr, dwB, dwm = ref["dw"], ref["B_dw"], mod["dw"]
        if acc:
            dwr, dwB, dwm = dwr + dw_old.double(), dwB + dw_old.double().abs(), dwm + dw_old.float()
        hold(f"rmsnorm dw{' accumulate' if acc else ''} {tag}", dtype, dw, dwr, dwB, N.r16(dwm, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,d", [(577 * 2, 1024), (34, 128)])
def test_layernorm_forward_and_backward_per_element(ops, dtype, rows, d):
    eps = 1e-5
    x, dy, old = rnd(rows, d, dtype=dtype), rnd(rows, d, dtype=dtype, seed=2), rnd(rows, d, dtype=dtype, seed=4)
    w = (1 + 0.1 * torch.randn(d, generator=torch.Generator().manual_seed(5))).to(dtype).to(dev())
    b = rnd(d, dtype=dtype, seed=6, scale=0.1)
    tag = f"{rows}x{d}"
    for acc in (False, True):
        o = old if acc else None
        ref, mod = N.layernorm(x, w, b, eps, dy, dx_old=o), N.layernorm(x, w, b, eps, dy, dx_old=o, model=dtype)
        if not acc:
            hold(f"layernorm y {tag}", dtype, ops.layernorm_fwd(x, w, b, eps), ref["y"], ref["B_y"], mod["y"])
        dw, db = rnd(d, dtype=dtype, seed=7), rnd(d, dtype=dtype, seed=8)
        dw_old, db_old = dw.clone(), db.clone()
        dx = ops.layernorm_bwd(x, w, dy, eps, dx=old.clone() if acc else None, accumulate_dx=acc, dw_out=dw, db_out=db, accumulate=acc)
        hold(f"layernorm dx{' accumulate' if acc else ''} {tag}", dtype, dx, ref["dx"], ref["B_dx"], mod["dx"])
        for nm, got, prev in (("dw", dw, dw_old), ("db", db, db_old)):
            r, Bc, m = ref[nm], ref["B_" + nm], mod[nm]
            if acc:
                r, Bc, m = r + prev.double(), Bc + prev.double().abs(), m + prev.float()
            hold(f"layernorm {nm}{' accumulate' if acc else ''} {tag}", dtype, got, r, Bc, N.r16(m, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_elementwise_and_rope_per_element(ops, dtype):
    rows, ff = 613, 11008
    gu, dout = rnd(rows, 2 * ff, dtype=dtype), rnd(rows, ff, dtype=dtype, seed=1)
    # saturated and vanishing gates.  (Not beyond -87: sigmoid(g) is then below 2^-126 and the fast reciprocal returns 0 for it, so silu(g) * up is 0
    # instead of ~ 1e-37 - an absolute error no 16-bit consumer can see, but an infinite relative one.)
    gu[0, :8] = torch.tensor([0.0, -0.0, 30.0, -30.0, 1e-4, -1e-4, 80.0, -80.0], dtype=dtype)
    hold("swiglu fwd", dtype, ops.swiglu_fwd(gu), N.swiglu_fwd(gu), 0.0, N.swiglu_fwd(gu, model=dtype))
    hold("swiglu bwd", dtype, ops.swiglu_bwd(gu, dout), N.swiglu_bwd(gu, dout), 0.0, N.swiglu_bwd(gu, dout, model=dtype))
    x, dy = rnd(577 * 2, 4096, dtype=dtype, seed=2, scale=2.0), rnd(577 * 2, 4096, dtype=dtype, seed=3)
    hold("quick-gelu fwd", dtype, ops.quick_gelu_fwd(x), N.quick_gelu_fwd(x), 0.0, N.quick_gelu_fwd(x, model=dtype))
    hold("quick-gelu bwd", dtype, ops.quick_gelu_bwd(x, dy), N.quick_gelu_bwd(x, dy), 0.0, N.quick_gelu_bwd(x, dy, model=dtype))
    hold("add", dtype, ops.add(x, dy), N.add(x, dy), 0.0, N.add(x, dy, model=dtype))
    for Bn, S, H, D in ((2, 50, 4, 128), (1, 577, 2, 64), (1, 4096, 1, 128)):
        T = Bn * S
        qkv = rnd(T, 3 * H * D, dtype=dtype, seed=4)
        tab = ops.rope_table(S, D, 10000.0, dev())
        tab64 = N.rope_table(S, D, 10000.0, dev())
        assert float((tab - tab64).abs().max()) < 2e-4 * max(1.0, S / 512)  # fp32 angles up to S rad: the table itself against fp64 angles
        for inverse in (False, True):
            got = ops.rope_qk_(qkv.clone(), tab, S, H, D, inverse=inverse)
            qk = qkv[:, :2 * H * D].reshape(T, 2 * H, D)
            hold(f"rope{' inverse' if inverse else ''} S={S} D={D}", dtype, got[:, :2 * H * D].reshape(T, 2 * H, D), N.rope(qk, tab, S, inverse=inverse), 0.0,
                 N.rope(qk, tab, S, inverse=inverse, model=dtype))
            assert torch.equal(got[:, 2 * H * D:], qkv[:, 2 * H * D:])  # v untouched


# ---- loss ----------------------------------------------------------------------------------------------------------------------------------
def _ce_inputs(V, ldl, Bn=2, S=37):
    g = torch.Generator().manual_seed(V + ldl)
    logits = (torch.randn(Bn * S, ldl, generator=g) * 3).to(dev())
    labels = torch.randint(0, V, (Bn, S), generator=g).to(dev())
    labels[0, :5] = -100
    labels[1, 10:20] = -100
    return logits, labels


def _hold_ce(ops, name, logits, labels, V, Vpad, gscale):
    """ce_fwd against fp64 (lse, row losses, count, mean) and ce_bwd per element in both dtypes.  Returns (lse, out2)."""
    ref = N.cross_entropy(logits, labels, V, gscale)
    row_loss, lse, out2 = ops.ce_fwd(logits, labels, V)
    # lse = m + log(sum exp(x - m)): the fast exp / log of the kernel are good to a few fp32 ulps of the SUM, i.e. of 1 in lse: 16 ulps of
    # max(1, |lse|), and the same for a row's loss lse - x[label] on the scale of its two terms
    e32 = N.EPS16[F32]
    assert bool(torch.isfinite(lse).all()), f"{name}: non-finite lse in rows {(~torch.isfinite(lse)).nonzero().flatten().tolist()[:8]}"
    assert float(((lse.double() - ref["lse"]).abs() / (16 * e32 * ref["lse"].abs().clamp_min(1.0))).max()) <= 1.0, name
    scale = ref["lse"].abs().clamp_min(1.0) + ref["row_loss"].abs()
    assert float(((row_loss.double() - ref["row_loss"]).abs() / (32 * e32 * scale)).max()) <= 1.0, name
    assert float(row_loss[N.shifted_labels(labels) < 0].abs().max()) == 0.0
    assert float(out2[1]) == ref["count"]
    assert abs(float(out2[0]) - float(ref["row_loss"].sum())) <= 64 * e32 * float(ref["row_loss"].sum()) * max(1.0, math.log2(len(lse))), name
    assert float(out2[2]) == float(out2[0] / out2[1])
    for dtype in DTYPES:
        dl = ops.ce_bwd(logits, labels, lse, out2, V, Vpad, gscale, dtype)
        hold(f"ce gradient {name}", dtype, dl[:, :V], ref["dlogits"], 0.0, N.cross_entropy(logits, labels, V, gscale, model=dtype)["dlogits"])
        if Vpad > V:
            assert float(dl[:, V:].abs().max()) == 0.0
    return lse, out2


@pytest.mark.parametrize("V", [103, 32003])
def test_cross_entropy_per_element(ops, V):
    Vpad = (V + 63) // 64 * 64
    for ldl, gscale in ((Vpad, 1.0), (Vpad + 64, 0.37), (Vpad + 3, 1.0)):  # ldl > Vpad; gscale != 1; rows that are not 16-byte aligned
        logits, labels = _ce_inputs(V, ldl)
        lse, out2 = _hold_ce(ops, f"V={V} ldl={ldl} gscale={gscale}", logits, labels, V, Vpad, gscale)
        # the compact form: the selected rows of ce_bwd bit for bit, negative indices give zero rows
        T = labels.numel()
        rows = torch.tensor([0, 5, -1, T - 1, 36, 37, -7, 20, 5], dtype=torch.int64, device=dev())
        for dtype in DTYPES:
            full = ops.ce_bwd(logits, labels, lse, out2, V, Vpad, gscale, dtype)
            part = ops.ce_bwd_rows(logits, labels, lse, out2, rows, V, Vpad, gscale, dtype)
            want = torch.where((rows >= 0)[:, None], full[rows.clamp_min(0)], torch.zeros_like(full[:1]))
            assert torch.equal(part.view(torch.int16), want.view(torch.int16))
            assert float(part[rows < 0].abs().max()) == 0.0 and float(part[rows >= 0].abs().max()) > 0.0


def test_cross_entropy_all_ignored_batch(ops):
    V, Vpad = 103, 128
    logits, labels = _ce_inputs(V, Vpad)
    labels[:] = -100
    row_loss, lse, out2 = ops.ce_fwd(logits, labels, V)
    assert float(out2[1]) == 0.0 and float(out2[0]) == 0.0 and math.isnan(float(out2[2]))  # like torch's mean over no rows
    assert math.isnan(float(torch.nn.functional.cross_entropy(logits[:, :V], labels.view(-1), ignore_index=-100)))
    assert float(row_loss.abs().max()) == 0.0
    for dtype in DTYPES:
        dl = ops.ce_bwd(logits, labels, lse, out2, V, Vpad, 1.0, dtype)
        assert float(dl.float().abs().max()) == 0.0 and not bool(torch.isnan(dl.float()).any())


@pytest.mark.parametrize("V,ldl", [(103, 128), (103, 131), (32003, 32064)])
def test_cross_entropy_rows_with_minus_inf_logits(ops, V, ldl):
    """Masked-out vocabulary entries (-inf logits): torch's logsumexp is finite there and so must the kernel's be - whole 16-byte groups of
    -inf at the start of a thread's stride, scattered single ones, and a row whose only finite logit is the label's."""
    Vpad = (V + 63) // 64 * 64
    logits, labels = _ce_inputs(V, ldl)
    ninf = float("-inf")
    logits[3, :64] = ninf             # the first element of 16 threads' strides
    logits[4, 8:12] = ninf            # one aligned group of four
    logits[5, ::7] = ninf             # scattered
    logits[6, V - 3:V] = ninf         # the tail
    labels.view(-1)[5:8] = 1          # rows 4-6 are scored against labels[0, 5..7]: a finite column of each (a -inf label logit is an infinite loss)
    lab7 = int(labels.view(-1)[8])    # row 7 is scored against labels[0, 8]
    keep = logits[7, lab7].clone()
    logits[7, :] = ninf
    logits[7, lab7] = keep
    ref = torch.logsumexp(logits[:, :V].double(), 1)
    assert bool(torch.isfinite(ref).all())
    sh = N.shifted_labels(labels)
    assert bool(torch.isfinite(logits[sh >= 0, sh[sh >= 0]]).all())  # every scored label sits on a finite logit
    _hold_ce(ops, f"-inf logits V={V} ldl={ldl}", logits, labels, V, Vpad, 1.0)


IDLE_REDUCERS = list(range(100, 200)) + list(range(1000, 1024))  # threads of the 1024-thread reduction that get no scored row


def _ce_many_rows(V, ldl, Bn, S, offset=0):
    """More rows than the reduction has threads (T = Bn * S around and beyond 1024, 2048): thread i of it sums rows i, i + 1024, ...  Every row
    of the threads in IDLE_REDUCERS is ignored (row t is scored against the flat label t + 1), the others keep a random label.
    offset: the logits are a view that starts `offset` floats into their buffer."""
    T = Bn * S
    g = torch.Generator().manual_seed(V + T)
    buf = (torch.randn(T * ldl + 4, generator=g) * 3).to(dev())
    logits = buf[offset:offset + T * ldl].view(T, ldl)
    labels = torch.randint(0, V, (Bn, S), generator=g)
    t = torch.arange(T - 1)
    labels.view(-1)[1:][torch.isin(t % 1024, torch.tensor(IDLE_REDUCERS))] = -100
    return logits, labels.to(dev())


@pytest.mark.parametrize("V,Bn,S,offset", [(103, 1, 1024, 0), (103, 1, 1025, 0), (103, 3, 700, 0), (103, 2, 2049, 0), (32003, 1, 1100, 0),
                                           (103, 3, 700, 1)])
def test_cross_entropy_more_rows_than_reducer_threads(ops, V, Bn, S, offset):
    """The final reduction's strided loop over T > 1024 rows (second and third pass, threads with and without a row in the last pass, threads
    with nothing to add), and, offset = 1, logits whose rows are 4 bytes off a 16-byte boundary although ldl % 4 == 0: the 16-byte loads of
    the row pass would be misaligned there, so mh_ce_fwd takes them only when the base pointer allows it too."""
    Vpad = (V + 63) // 64 * 64
    logits, labels = _ce_many_rows(V, Vpad, Bn, S, offset)
    assert Vpad % 4 == 0 and logits.data_ptr() % 16 == 4 * offset
    sh = N.shifted_labels(labels).cpu()
    scored = (sh >= 0).nonzero().flatten() % 1024
    assert set(scored.tolist()) == set(range(min(1024, Bn * S - 1))) - set(IDLE_REDUCERS)  # (the very last row is never scored)
    _hold_ce(ops, f"V={V} T={Bn}x{S} offset={offset}", logits, labels, V, Vpad, 0.5 if offset else 1.0)


# ---- optimizer ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(N.ADAMW_CASES))
@pytest.mark.parametrize("n", [8, 4096, 4096 + 5, 2 ** 20 + 3])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("decay", [True, False])
def test_adamw_ten_steps_one_at_a_time(ops, dtype, case, n, clip, decay):
    """mh_adamw / mh_adamw_clip, every step checked from the state the KERNEL left (p, m, v): the only accumulated error of p is its single
    16-bit store.  Before a step is compared it is shown to be resolvable (numerics.resolvable): a kernel that does nothing fails."""
    hp = dict(beta1=0.9, beta2=0.95, eps=1e-8)
    lr, wd = N.ADAMW_CASES[case]["lr"], N.ADAMW_CASES[case]["wd"] if decay else 0.0
    gscale, factor = 0.5, 0.8
    fdev = torch.tensor([factor], dtype=torch.float32, device=dev())
    p = N.adamw_inputs(case, n, dtype, 1)[0].to(dev())
    m, v = torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    worst = {"p": (0.0, 0.0), "m": (0.0, 0.0), "v": (0.0, 0.0)}
    for step in range(1, 11):
        g = N.adamw_inputs(case, n, dtype, step)[1].to(dev())
        p0, m0, v0 = p.clone(), m.clone(), v.clone()
        kw = dict(lr=lr, wd=wd, step=step, gscale=gscale, gscale_dev=factor if clip else None, **hp)
        ref, mod = N.adamw_step(p0, g, m0, v0, **kw), N.adamw_step(p0, g, m0, v0, model=dtype, **kw)
        cp = N.componentwise(mod["p"], ref["p"], ref["B_p"], N.EPS16[dtype], N.TINY[dtype])[0]
        tol = N.limit(cp) * N.EPS16[dtype] * ref["p"].abs()
        frac = N.resolvable(ref["p"], p0, tol)
        assert frac >= 0.9, f"step {step}: only {frac:.2f} of the reference steps are resolvable"
        if clip:
            ops.adamw_clip_(p, g, m, v, lr, hp["beta1"], hp["beta2"], hp["eps"], wd, step, gscale, fdev)
        else:
            ops.adamw_(p, g, m, v, lr, hp["beta1"], hp["beta2"], hp["eps"], wd, step, gscale)
        e32, t32 = N.EPS16[F32], 1e-37
        for nm, got, Bc, eps, tiny in (("p", p, ref["B_p"], N.EPS16[dtype], N.TINY[dtype]), ("m", m, ref["B_m"], e32, t32), ("v", v, 0.0, e32, t32)):
            cm = N.componentwise(mod[nm], ref[nm], Bc, eps, tiny)[0]
            ck, at = N.componentwise(got, ref[nm], Bc, eps, tiny)
            lim = N.limit(cm)
            assert ck <= lim, f"adamw {nm} step {step}: kernel c = {ck:.3f} at {at} exceeds {lim:.3f} (model {cm:.3f})"
            if ck >= worst[nm][1]:
                worst[nm] = (cm, ck)
    for nm, (cm, ck) in worst.items():
        print(f"CW | adamw{'_clip' if clip else ''} {nm} {case} n={n} wd={wd} | {str(dtype)[6:]} | {cm:.3f} | {ck:.3f} | {N.limit(cm):.3f} | worst of 10 steps")
