"""The per-element checker of tests/numerics.py against itself, without a GPU: for every operation it must ACCEPT the rounding model (the fp32
evaluation with the kernels' 16-bit roundings) and REJECT every mutant - a plain fp64 reference with one deliberate defect, stored in the 16-bit
type like a kernel's output - at c >= 2 x the limit the kernels are held to.  Every line printed is `mutant dtype: c vs limit`.

The fp8 cases also print what the metric they replace gives for the same mutant: relerr = max|got - ref| / max|ref| in units of eps16, which
tests/test_fp8_training_gpu.py and tests/test_ops_gpu.py hold below 3 to 4.  Any error below 1.2 % of the LARGEST output of the tensor passes
it in bf16.  Of the mutants below it lets through, in bf16, "bias added twice in one column" at the weight size its own tests use (sigma 0.3:
1.1 eps16 against a limit of 4; 7.5 x the per-element bound) and comes within 10 % of passing it at sigma 0.05 (4.45 eps16; 44 x the bound); it
scores "one lane's 16 values skipped" of the GEMV at 5.3 to 7.4 eps16 against its limit of 3 (c = 20 to 31 against 2).  The other
mutants are built on weights whose block scales differ by powers of two and move a whole row or block by more than that metric's limit too;
in fp16, whose eps is 8 times smaller, it catches all of them."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import numerics as N  # noqa: E402

DTYPES = [torch.bfloat16, torch.float16]


def rnd(*shape, dtype, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def score(got, ref, B, dtype):
    """c of `got`; inf when an element that must be exactly zero is not (the checker raises there)."""
    try:
        return N.componentwise(got, ref, B, N.EPS16[dtype], N.TINY[dtype])[0]
    except AssertionError:
        return float("inf")


def accept(name, dtype, model, ref, B, cap):
    """The checker accepts the model: its c is finite and small (cap: what the rounding analysis of the operation allows), so the limit
    derived from it is tight enough to mean something."""
    c = score(model, ref, B, dtype)
    print(f"model  {name:34s} {str(dtype)[6:]:9s} c = {c:8.3f}  limit = {N.limit(c):.3f}")
    assert c <= cap, (name, dtype, c)
    return N.limit(c)


def reject(name, dtype, got, ref, B, lim):
    c = score(got.to(dtype) if got.dtype == torch.float64 else got, ref, B, dtype)
    print(f"mutant {name:34s} {str(dtype)[6:]:9s} c = {c:8.1f}  limit = {lim:.3f}")
    assert c >= 2 * lim, (name, dtype, c, lim)


# ---- attention ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", [1024, 2048])
def test_attention_model_accepted_and_tile_mutants_rejected(dtype, S):
    D = 128
    qkv = rnd(S, 3 * D, dtype=dtype)  # one head of the suite's fused q|k|v rows
    q, k, v = (qkv[:, i * D:(i + 1) * D] for i in range(3))
    do = rnd(S, D, dtype=dtype, seed=9)
    ref = N.attention(q, k, v, do, causal=True, keep=True)
    mod = N.attention(q, k, v, do, causal=True, model=dtype)
    lim = {}
    for nm in ("o", "dv", "dq", "dk"):
        B = ref["B_o"] if nm == "o" else N.f16_subnormal_B(ref, nm, dtype)
        # one rounding of the 16-bit operand and one of the output, each at most eps16 * (|ref| + B): c <= 2 before fp32 effects
        lim[nm] = accept(f"attention {nm} S={S}", dtype, mod[nm], ref[nm], B, cap=2.0)
    Bs = {nm: N.f16_subnormal_B(ref, nm, dtype) for nm in ("dq", "dk", "dv")}
    scale = 1.0 / math.sqrt(D)
    ar = torch.arange(S)

    dv = ref["dv"].clone(); dv[-64:] = 0
    reject(f"dV last 64-key tile zero S={S}", dtype, dv, ref["dv"], Bs["dv"], lim["dv"])
    dk = ref["dk"].clone(); dk[-64:] = 0
    reject(f"dK last 64-key tile zero S={S}", dtype, dk, ref["dk"], Bs["dk"], lim["dk"])
    dq = ref["dq"].clone(); dq[-64:] -= (ref["dS"][-64:, -64:] @ k[-64:].double()) * scale
    reject(f"dQ loses the diagonal tile S={S}", dtype, dq, ref["dq"], Bs["dq"], lim["dq"])

    def skip_tile(q0, q1):
        ok = ar[None, :] <= ar[q0:q1, None]
        hole = (ar[q0:q1, None] >= S - 64) & (ar[None, :] >= S // 2) & (ar[None, :] < S // 2 + 64)
        return ok & ~hole
    o = N.attention(q, k, v, causal=True, allowed=skip_tile)["o"]
    reject(f"fwd skips a 64-key tile S={S}", dtype, o, ref["o"], ref["B_o"], lim["o"])

    def off_by_one(q0, q1):
        i = ar[q0:q1, None]
        return ar[None, :] <= torch.where(i >= S // 2, i + 1, i)
    o = N.attention(q, k, v, causal=True, allowed=off_by_one)["o"]
    reject(f"causal mask off by one S={S}", dtype, o, ref["o"], ref["B_o"], lim["o"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_key_padding_off_by_one_rejected(dtype):
    S, D, n = 300, 128, 177  # the ragged shape of test_attention_fwd_bwd
    qkv = rnd(S, 3 * D, dtype=dtype)
    q, k, v = (qkv[:, i * D:(i + 1) * D] for i in range(3))
    ref = N.attention(q, k, v, causal=True, n_valid=n)
    lim = accept("attention o ragged", dtype, N.attention(q, k, v, causal=True, n_valid=n, model=dtype)["o"], ref["o"], ref["B_o"], cap=2.0)
    assert float(ref["o"][n:].abs().max()) == 0.0 and float(ref["B_o"][n:].abs().max()) == 0.0
    ar = torch.arange(S)
    # (a) one key too many, the padded query rows still zero: non-causal, so every valid row sees the extra key
    refn = N.attention(q, k, v, causal=False, n_valid=n)
    limn = accept("attention o ragged non-causal", dtype, N.attention(q, k, v, causal=False, n_valid=n, model=dtype)["o"], refn["o"], refn["B_o"], cap=2.0)
    o = N.attention(q, k, v, causal=False, allowed=lambda q0, q1: (ar[None, :] < n + 1) & (ar[q0:q1, None] < n))["o"]
    reject("key padding: one key too many", dtype, o, refn["o"], refn["B_o"], limn)
    # (b) the whole length off by one, causal: the only difference is query row n, which must be exactly zero
    o = N.attention(q, k, v, causal=True, n_valid=n + 1)["o"]
    reject("key padding: row n not zero", dtype, o, ref["o"], ref["B_o"], lim)


# ---- GEMM --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_model_accepted_and_tile_mutants_rejected(dtype):
    M, Nn, K = 200, 328, 512  # edge tiles in both dimensions of a 128- or 256-wide tiling
    a, b, bias, resid = rnd(M, K, dtype=dtype), rnd(Nn, K, dtype=dtype, seed=1), rnd(Nn, dtype=dtype, seed=2), rnd(M, Nn, dtype=dtype, seed=3)
    for kw in ({}, {"bias": bias}, {"bias": bias, "gelu": True}, {"bias": bias, "resid": resid}, {"c_old": resid}):
        ref, B = N.gemm(a, b, **kw)
        # fp32 accumulation: the one rounding at the store dominates
        accept(f"gemm {'+'.join(kw) or 'plain'}", dtype, N.gemm(a, b, model=dtype, **kw), ref, B, cap=1.5)
    ref32, B32 = N.gemm(a, b, out_dtype=torch.float32)
    c = N.componentwise(N.gemm(a, b, model=dtype, out_dtype=torch.float32), ref32, B32, N.EPS16[torch.float32])[0]
    print(f"model  gemm fp32 store {dtype}: c = {c:.3f}")
    assert c <= 1.0  # B is the worst-case bound of a K-term fp32 sum there
    rounded_first = N.gemm(a, b, model=dtype).float()  # the product stored in 16 bits, then widened: one rounding the fp32 store must not have
    c16 = N.componentwise(rounded_first, ref32, B32, N.EPS16[torch.float32])[0]
    print(f"mutant {'fp32 store rounded to 16 bits first':34s} {str(dtype)[6:]:9s} c = {c16:8.1f}  limit = {N.limit(c):.3f}")
    assert c16 >= 2 * N.limit(c)
    ref, B = N.gemm(a, b, bias=bias)
    lim = N.limit(score(N.gemm(a, b, bias=bias, model=dtype), ref, B, dtype))
    short = ref.clone()
    short[192:200, 256:] -= a[192:200, -32:].double() @ b[256:, -32:].double().t()
    reject("gemm omits the last 32 of K", dtype, short, ref, B, lim)
    twice = ref.clone()
    twice[:, 256:] += bias[256:].double()
    reject("gemm adds the bias twice", dtype, twice, ref, B, lim)


# ---- norms, elementwise, RoPE -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_norm_models_accepted_and_mutants_rejected(dtype):
    rows, d, eps = 37, 256, 1e-5
    x, w, dy = rnd(rows, d, dtype=dtype), (1 + 0.1 * torch.randn(d, generator=torch.Generator().manual_seed(5))).to(dtype), rnd(rows, d, dtype=dtype, seed=2)
    x[3] = (x[3].float() * 1e-3).to(dtype)  # a near-zero row: eps decides its scale
    old = rnd(rows, d, dtype=dtype, seed=4)
    ref, mod = N.rmsnorm(x, w, eps, dy, dx_old=old), N.rmsnorm(x, w, eps, dy, dx_old=old, model=dtype)
    ly = accept("rmsnorm y", dtype, mod["y"], ref["y"], ref["B_y"], cap=1.01)
    lx = accept("rmsnorm dx (accumulate)", dtype, mod["dx"], ref["dx"], ref["B_dx"], cap=1.01)
    accept("rmsnorm dw", dtype, N.r16(mod["dw"], dtype), ref["dw"], ref["B_dw"], cap=1.01)
    X, W, G = x.double(), w.double(), dy.double() * w.double()
    rstd = torch.rsqrt((X * X).mean(1, keepdim=True) + eps)
    reject("rmsnorm dx without the projection", dtype, rstd * G + old.double(), ref["dx"], ref["B_dx"], lx)
    y_noeps = ref["y"].clone()
    y_noeps[3] = X[3] * torch.rsqrt((X[3] * X[3]).mean()) * W
    reject("rmsnorm drops eps on a tiny row", dtype, y_noeps, ref["y"], ref["B_y"], ly)
    b = rnd(d, dtype=dtype, seed=6, scale=0.1)
    ref, mod = N.layernorm(x, w, b, eps, dy), N.layernorm(x, w, b, eps, dy, model=dtype)
    for nm in ("y", "dx", "dw", "db"):
        accept(f"layernorm {nm}", dtype, N.r16(mod[nm], dtype), ref[nm], ref["B_" + nm], cap=1.01)


@pytest.mark.parametrize("dtype", DTYPES)
def test_elementwise_and_rope_models_accepted_and_mutants_rejected(dtype):
    gu, dout = rnd(64, 512, dtype=dtype), rnd(64, 256, dtype=dtype, seed=1)
    # ONE rounding of an fp32 value: c <= 1 (+ fp32 effects)
    for name, ref, mod in (("swiglu fwd", N.swiglu_fwd(gu), N.swiglu_fwd(gu, model=dtype)),
                           ("swiglu bwd", N.swiglu_bwd(gu, dout), N.swiglu_bwd(gu, dout, model=dtype)),
                           ("quick-gelu fwd", N.quick_gelu_fwd(gu), N.quick_gelu_fwd(gu, model=dtype)),
                           ("quick-gelu bwd", N.quick_gelu_bwd(gu, gu.flip(0)), N.quick_gelu_bwd(gu, gu.flip(0), model=dtype)),
                           ("add", N.add(gu, gu.flip(0)), N.add(gu, gu.flip(0), model=dtype))):
        accept(name, dtype, mod, ref, 0.0, cap=1.0 + 1e-3)
    g, u, d = gu[:, :256].double(), gu[:, 256:].double(), dout.double()
    reject("swiglu bwd with plain sigmoid", dtype, torch.cat([d * u * torch.sigmoid(g), d * g * torch.sigmoid(g)], 1), N.swiglu_bwd(gu, dout), 0.0, 2.0)
    S, H, D = 50, 2, 128
    x = rnd(2 * S, H, D, dtype=dtype, seed=3)
    tab = N.rope_table(S, D, 10000.0)
    ref = N.rope(x, tab, S)
    lim = accept("rope", dtype, N.rope(x, tab, S, model=dtype), ref, 0.0, cap=1.0 + 1e-3)
    accept("rope inverse", dtype, N.rope(x, tab, S, inverse=True, model=dtype), N.rope(x, tab, S, inverse=True), 0.0, cap=1.0 + 1e-3)
    bad = ref.clone()
    bad[-1] = N.rope(x, tab, S, inverse=True)[-1]
    reject("rope inverse on the last row", dtype, bad, ref, 0.0, lim)


# ---- the norm kernels' dispatch arms and row partition, on the inputs of tests/test_norm_arms_gpu.py ----------------------------------------
def c_of(got, ref, B, od):
    try:
        return N.componentwise(got, ref, B, N.EPS16[od], N.TINY[od])[0]
    except AssertionError:
        return float("inf")


def above(name, dtype, c, lim):
    print(f"mutant {name:50s} {str(dtype)[6:]:9s} c = {c:10.1f}  limit = {lim:.3f}")
    assert c > lim, (name, dtype, c, lim)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ln", [False, True], ids=["rms", "ln"])
@pytest.mark.parametrize("rows,d", [(9, 520), (9, 1032), (9, 2056), (4097, 128)])
def test_norm_backward_partition_mutants_rejected(dtype, ln, rows, d):
    """What the GPU test holds dx, dw (db) and the raw partials to rejects: a dw without the row's last 8-element chunk, a block that skips its
    last row, a reduce that skips one partial row.  16-bit dw where the GPU test has few rows; at 4097 rows one row is below a bf16 rounding of
    the whole column (B_dw sums 4097 terms), and it is the fp32 bound on the summed partials that sees it."""
    import norm_inputs as NI

    F32 = torch.float32
    I = NI.norm_inputs(rows, d, dtype, ln)
    fn = (lambda **kw: N.layernorm(I["x"], I["w"], I["b"], NI.EPS, I["dy"], **kw)) if ln else (lambda **kw: N.rmsnorm(I["x"], I["w"], NI.EPS, I["dy"], **kw))
    ref, mod = fn(), fn(model=dtype)
    names = ("dw", "db") if ln else ("dw",)
    lim16 = {nm: N.limit(c_of(N.r16(mod[nm], dtype), ref[nm], ref["B_" + nm], dtype)) for nm in names}
    lim32 = {nm: N.limit(c_of(mod[nm], ref[nm], ref["B_" + nm], F32)) for nm in names}
    limx = N.limit(c_of(mod["dx"], ref["dx"], ref["B_dx"], dtype))
    print(f"model  backward {rows}x{d} {'ln' if ln else 'rms'} {str(dtype)[6:]}: limits dx {limx:.3f} 16-bit {lim16} fp32 {lim32}")
    big = rows >= 4097
    od = F32 if big else dtype
    lim = lim32 if big else lim16
    # the terms of dw (db) per row, and the partition the launcher makes of them
    X, DY = I["x"].double(), I["dy"].double()
    mu = X.mean(1, keepdim=True) if ln else 0.0
    xh = (X - mu) * torch.rsqrt(((X - mu) ** 2).mean(1, keepdim=True) + NI.EPS)
    terms = {"dw": DY * xh, "db": DY}
    nblk, rpb, ranges = NI.block_ranges(rows)
    for nm in names:
        T = terms[nm]
        partial = torch.stack([T[r0:r1].sum(0) for r0, r1 in ranges])
        assert c_of(partial.sum(0).to(od), ref[nm], ref["B_" + nm], od) <= 1.0  # the partition itself is the reference
        cut = ref[nm].clone()
        cut[-8:] = 0
        above(f"{nm} without the last 8-element chunk {rows}x{d}", dtype, c_of(cut.to(od), ref[nm], ref["B_" + nm], od), lim[nm])
        r0, r1 = ranges[0]
        above(f"{nm}: block 0 skips its last row {rows}x{d}", dtype, c_of((ref[nm] - T[r1 - 1]).to(od), ref[nm], ref["B_" + nm], od), lim[nm])
        last_full = max(b for b, (r0, r1) in enumerate(ranges) if r1 > r0)
        for b in (0, last_full):
            above(f"{nm}: reduce skips partial row {b} {rows}x{d}", dtype, c_of((ref[nm] - partial[b]).to(od), ref[nm], ref["B_" + nm], od), lim[nm])
    # the skipped row's dx is never written: whatever the buffer held (zeros here) is not the row's dx
    dx = ref["dx"].clone()
    dx[ranges[0][1] - 1] = 0
    above(f"dx: block 0 skips its last row {rows}x{d}", dtype, c_of(dx.to(dtype), ref["dx"], ref["B_dx"], dtype), limx)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [520, 1024, 4096])
def test_layernorm_one_pass_variance_rejected_on_the_shifted_row(dtype, d):
    """LayerNorm whose variance is E[x^2] - mu^2 in fp32: on a row of 30 + randn that difference keeps about 2^-24 x 900 of a variance of 1.
    A 16-bit y cannot show it (printed); the fp32 y of mh_layernorm_f32_to_f32 does, under numerics.norm_f32in's B_y."""
    import norm_inputs as NI

    F32 = torch.float32
    I = NI.f32_inputs(6, d, dtype, True)
    x, w, b = I["x32"], I["w"], I["b"]
    mu = x.mean(1, keepdim=True)
    var = (x * x).mean(1, keepdim=True) - mu * mu
    y_mut = (x - mu) * torch.rsqrt(var + torch.tensor(NI.EPS)) * w.float() + b.float()
    assert y_mut.dtype == F32
    for yd in (F32, dtype):
        ref, mod = N.norm_f32in(x, w, b, NI.EPS, y_dtype=yd), N.norm_f32in(x, w, b, NI.EPS, y_dtype=yd, model=dtype)
        assert torch.equal(ref["x16"], x.to(dtype))
        cm = c_of(mod["y"], ref["y"], ref["B_y"], yd)
        c = c_of(y_mut if yd == F32 else y_mut.to(yd), ref["y"], ref["B_y"], yd)
        if yd == F32:
            above(f"layernorm variance E[x^2] - mu^2, fp32 y d={d}", dtype, c, N.limit(cm))
        else:
            print(f"       (the same mutant in a 16-bit y d={d} {str(dtype)[6:]}: c = {c:.3f}, model {cm:.3f}: not visible)")


@pytest.mark.parametrize("dtype", DTYPES)
def test_colsum_and_f32in_models_accepted(dtype):
    import norm_inputs as NI

    for rows, d, ld, off in ((3, 8, 8, 0), (4097, 264, 272, 0), (4097, 260, 260, 0), (4097, 264, 272, 1)):
        buf, old = NI.colsum_inputs(rows, d, ld, dtype, offset=off)
        x = NI.colsum_view(buf, rows, d, ld, off)
        for o in (None, old):
            ref, B = N.colsum(x, o)
            accept(f"colsum {rows}x{d} ld {ld}{' accumulate' if o is not None else ''}", dtype, N.colsum(x, o, model=dtype), ref, B, cap=1.01)
    for ln in (False, True):
        for d in (8, 520, 1024, 4096):
            I = NI.f32_inputs(6, d, dtype, ln)
            for yd in (dtype, torch.float32) if ln else (dtype,):
                ref, mod = N.norm_f32in(I["x32"], I["w"], I["b"], NI.EPS, y_dtype=yd), N.norm_f32in(I["x32"], I["w"], I["b"], NI.EPS, y_dtype=yd, model=dtype)
                c = c_of(mod["y"], ref["y"], ref["B_y"], yd)
                print(f"model  norm_f32in {'ln' if ln else 'rms'} d={d} y {str(yd)[6:]:9s} {str(dtype)[6:]:9s} c = {c:8.3f}")
                assert c <= 1.01, (ln, d, yd, c)


# ---- loss ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [103, 32003])
def test_cross_entropy_model_accepted_and_count_mutant_rejected(dtype, V):
    Bn, S = 2, 17
    g = torch.Generator().manual_seed(V)
    logits = torch.randn(Bn * S, V, generator=g) * 3
    labels = torch.randint(0, V, (Bn, S), generator=g)
    labels[0, :5] = -100
    ref = N.cross_entropy(logits, labels, V, gscale=0.5)
    tref = torch.nn.functional.cross_entropy(logits.double().view(Bn, S, V)[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1), ignore_index=-100)
    assert abs(float(ref["mean"]) - float(tref)) < 1e-12 * float(tref)  # the reference itself against torch in fp64
    mod = N.cross_entropy(logits, labels, V, gscale=0.5, model=dtype)
    lim = accept(f"ce gradient V={V}", dtype, mod["dlogits"], ref["dlogits"], 0.0, cap=1.05)
    cnt = ref["count"]
    lab = N.shifted_labels(labels)
    onehot = torch.zeros_like(ref["dlogits"])
    sc = lab >= 0
    onehot[sc.nonzero()[:, 0], lab[sc]] = -0.5 / cnt
    soft = ref["dlogits"] - onehot
    reject(f"ce softmax part x count/(count+1) V={V}", dtype, soft * (cnt / (cnt + 1)) + onehot, ref["dlogits"], 0.0, lim)


# ---- AdamW ----------------------------------------------------------------------------------------------------------------------------------
ADAMW_CASES, adamw_inputs = N.ADAMW_CASES, N.adamw_inputs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(ADAMW_CASES))
def test_adamw_model_accepted_steps_resolvable_and_mutants_rejected(dtype, case):
    n, hp = 4096 + 5, dict(beta1=0.9, beta2=0.95, eps=1e-8)
    lr, wd, gscale = ADAMW_CASES[case]["lr"], ADAMW_CASES[case]["wd"], 0.5
    p, _ = adamw_inputs(case, n, dtype, 1)
    m, v = torch.zeros(n), torch.zeros(n)
    worst = {}
    for step in range(1, 11):
        _, g = adamw_inputs(case, n, dtype, step)
        kw = dict(lr=lr, wd=wd, step=step, gscale=gscale, **hp)
        ref, mod = N.adamw_step(p, g, m, v, **kw), N.adamw_step(p, g, m, v, model=dtype, **kw)
        cp = score(mod["p"], ref["p"], ref["B_p"], dtype)
        cm = N.componentwise(mod["m"], ref["m"], ref["B_m"], N.EPS16[torch.float32])[0]
        cv = N.componentwise(mod["v"], ref["v"], 0.0, N.EPS16[torch.float32], 1e-37)[0]
        assert cp <= 1.0 + 1e-3 and cm <= 2.0 and cv <= 4.0, (step, cp, cm, cv)  # one 16-bit store; two / four fp32 roundings
        lp, lm = N.limit(cp), N.limit(cm)
        tol = lp * N.EPS16[dtype] * ref["p"].abs()
        frac = N.resolvable(ref["p"], p, tol)
        assert frac >= 0.9, (case, dtype, step, frac)
        muts = {"does nothing": (p.double(), None),
                "no bias correction": (N.adamw_step(p, g, m, v, **{**kw, "step": 10 ** 6})["p"], None),
                "no weight decay": (N.adamw_step(p, g, m, v, **{**kw, "wd": 0.0})["p"], None),
                "ignores gscale": (None, N.adamw_step(p, g, m, v, **{**kw, "gscale": 1.0})["m"])}
        for name, (pm, mm) in muts.items():
            c = score(pm.to(dtype), ref["p"], ref["B_p"], dtype) if pm is not None else N.componentwise(mm.float(), ref["m"], ref["B_m"], N.EPS16[torch.float32])[0]
            worst[name] = max(worst.get(name, 0.0), c / (lp if pm is not None else lm))
        p, m, v = mod["p"].to(dtype), mod["m"], mod["v"]
    # every step is checked on its own, from the state the kernel itself left: a defect fails the test when ANY of the ten steps rejects it
    for name, ratio in worst.items():
        print(f"mutant adamw {name:22s} {case:20s} {str(dtype)[6:]:9s} largest c / limit over 10 steps = {ratio:10.1f}")
        assert ratio >= 2.0, (name, case, dtype, ratio)


def test_adamw_reference_is_torch_adamw_in_fp64():
    """numerics.adamw_step against torch.optim.AdamW itself, both in float64 and fed their own state over five steps: the reference the kernels
    are held to is not a formula of this suite's own.  (torch is given the fp32 values of the hyper-parameters, as adamw_step takes them.)"""
    n, hp = 513, dict(lr=4e-3, beta1=0.9, beta2=0.95, eps=1e-8, wd=12.5)
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731
    gen = torch.Generator().manual_seed(11)
    p = (0.02 * torch.randn(n, generator=gen)).to(torch.bfloat16).double()
    tp = p.clone().requires_grad_()
    opt = torch.optim.AdamW([tp], lr=f32(hp["lr"]), betas=(f32(hp["beta1"]), f32(hp["beta2"])), eps=f32(hp["eps"]), weight_decay=f32(hp["wd"]))
    m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 6):
        g = (1e-2 * torch.randn(n, generator=gen)).to(torch.bfloat16)
        tp.grad = g.double() * 0.5
        opt.step()
        out = N.adamw_step(p, g, m, v, step=step, gscale=0.5, **hp)
        p, m, v = out["p"], out["m"], out["v"]
        assert p.dtype == torch.float64 and float((p - tp.detach()).abs().max()) <= 1e-13 * float(tp.detach().abs().max()), step


# ---- fp8: the scaled-fp8 GEMM (|got - want| <= ulp + err) and the fp8-weight GEMV (componentwise) ----------------------------------------------
def old_metric(got, ref, dtype):
    """max|got - ref| / max|ref| in units of eps16: what the max-norm tests hold below 3 to 4."""
    return float((got.double() - ref).abs().max() / ref.abs().max()) / N.EPS16[dtype]


def block_scaled(w, zero_row=None, zero_block=None):
    """Block kb of row n scaled by 2^-((n + kb) % 4): adjacent rows and adjacent blocks differ by powers of two."""
    Nr, K = w.shape
    nb = (K + 127) // 128
    f = torch.ldexp(torch.ones(Nr, nb), -((torch.arange(Nr)[:, None] + torch.arange(nb)[None, :]) % 4).to(torch.int32))
    out = w.float() * f.repeat_interleave(128, dim=1)[:, :K]
    if zero_row is not None:
        out[zero_row] = 0
    if zero_block is not None:
        out[zero_block[0], zero_block[1] * 128:(zero_block[1] + 1) * 128] = 0
    return out.to(w.dtype)


def reject_bound(name, dtype, got, want, err, out_dtype=None, old_limit=4.0):
    od = dtype if out_dtype is None else out_dtype
    g = got.to(od) if got.dtype == torch.float64 else got
    r, _ = N.bound_ratio(g, want, err, od)
    om = old_metric(g, want, dtype)
    print(f"mutant {name:44s} {str(dtype)[6:]:9s} |d| / bound = {r:10.1f}   old metric = {om:8.2f} eps16 (limit {old_limit}: {'PASSES' if om < old_limit else 'caught'})")
    assert r >= 2.0, (name, dtype, r)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_gemm_model_accepted_and_mutants_rejected(dtype):
    M, Nn, K = 64, 136, 8320  # 65 blocks: the exponent group is padded; N is no multiple of the 128-row group
    nkb = K // 128
    x, w = rnd(M, K, dtype=dtype), rnd(Nn, K, dtype=dtype, seed=1, scale=0.05)
    bias, resid = rnd(Nn, dtype=dtype, seed=2), rnd(M, Nn, dtype=dtype, seed=3)
    a8, (qb, sb) = N.quant_rows(x), N.quant_rows(w)
    e = (torch.arange(Nn)[:, None] + torch.arange(nkb)[None, :]) % 4
    ex = N.exp_image(e)
    assert torch.equal(N.exp_nibbles(ex, Nn, K), e)  # the image builder and its reader are inverses
    b8 = (qb, sb, ex)
    for kw in ({}, {"bias": bias}, {"bias": bias, "gelu": True}, {"resid": resid}, {"bias": bias, "resid": resid}, {"c_old": resid}):
        for od in (dtype, torch.float32):
            if od == torch.float32 and kw and "c_old" not in kw:
                continue
            want, err = N.gemm_fp8(a8, b8, out_dtype=od, **kw)
            r, _ = N.bound_ratio(N.gemm_fp8(a8, b8, out_dtype=od, model=True, **kw), want, err, od)
            print(f"model  fp8 gemm {'+'.join(kw) or 'plain':16s} {str(dtype)[6:]:9s} -> {str(od)[6:]:9s} |d| / bound = {r:.3f}")
            assert r <= 1.0, (kw, od, r)
    A = N.deq64(a8)
    Bd, _ = N.deq64_e4(qb, sb, ex)
    Bq = N.deq64((qb, sb)).view(Nn, nkb, 128)  # without the exponents

    def with_exps(e2):
        return (Bq * torch.ldexp(torch.ones(Nn, nkb, dtype=torch.float64), (-e2).to(torch.int32))[:, :, None]).view(Nn, K)

    want, err = N.gemm_fp8(a8, b8, out_dtype=dtype)
    e2 = e.clone(); e2[5, 6] = 0  # (5 + 6) % 4 = 3
    reject_bound("one (row, block) exponent taken as 0", dtype, A @ with_exps(e2).t(), want, err)
    e2 = e.clone(); e2[[130, 131]] = e[[131, 130]]
    reject_bound("nibbles of an even/odd row pair swapped", dtype, A @ with_exps(e2).t(), want, err)
    short = want.clone(); short[48:64] -= A[48:64, -128:] @ Bd[:, -128:].t()
    reject_bound("last 128-k block missing for 16 rows", dtype, short, want, err)
    nb_sa = want.clone(); nb_sa[M - 1] *= float(a8[1][M - 2]) / float(a8[1][M - 1])
    assert float(a8[1][M - 2]) != float(a8[1][M - 1])
    reject_bound("last row of a tile uses its neighbour's sa", dtype, nb_sa, want, err)
    want, err = N.gemm_fp8(a8, b8, bias=bias, out_dtype=dtype)
    twice = want.clone(); twice[:, 77] += bias[77].double()
    reject_bound("bias added twice in one column", dtype, twice, want, err)
    # ... and with weights of the size the max-norm tests use (sigma 0.3: outputs of +-100, next to which one bias is 1 % of the largest)
    b8w = (*N.quant_rows(rnd(Nn, K, dtype=dtype, seed=1, scale=0.3)), ex)
    want, err = N.gemm_fp8(a8, b8w, bias=bias, out_dtype=dtype)
    twice = want.clone(); twice[:, 77] += bias[77].double()
    reject_bound("bias added twice in one column, sigma_w 0.3", dtype, twice, want, err)
    want, err = N.gemm_fp8(a8, b8, bias=bias, gelu=True, out_dtype=dtype)
    prod = A @ Bd.t()
    reject_bound("quick-GELU applied before the bias", dtype, prod * torch.sigmoid(1.702 * prod) + bias.double(), want, err)
    # C_old: N % 4 != 0 is the scalar store path
    M2, N2, K2 = 72, 262, 256
    x2, w2, old = rnd(M2, K2, dtype=dtype), rnd(N2, K2, dtype=dtype, seed=1, scale=0.05), rnd(M2, N2, dtype=dtype, seed=4)
    a2, b2 = N.quant_rows(x2), N.quant_rows(w2)
    want, err = N.gemm_fp8(a2, b2, c_old=old, out_dtype=dtype)
    r, _ = N.bound_ratio(N.gemm_fp8(a2, b2, c_old=old, out_dtype=dtype, model=True), want, err, dtype)
    assert r <= 1.0, r
    lost = want.clone(); lost[:, N2 - N2 % 4:] -= old[:, N2 - N2 % 4:].double()
    reject_bound("C_old ignored in the last N % 4 columns", dtype, lost, want, err)
    # the OLD reference - q.float() * s, an fp32 product that rounds (4 + 24 significant bits) - stays inside the bound: it must be accepted
    want, err = N.gemm_fp8(a8, b8, out_dtype=torch.float32)
    A32 = (N.e4m3(a8[0]).float() * a8[1][:, None]).double()
    B32 = (N.e4m3(qb).float().view(Nn, nkb, 128) * (sb[:, None] * torch.ldexp(torch.ones(Nn, nkb), (-e).to(torch.int32)))[:, :, None]).view(Nn, K).double()
    assert not torch.equal(A32, A)
    r, _ = N.bound_ratio(A32 @ B32.t(), want, err, torch.float32)
    print(f"accept fp32-rounded dequantised reference    {str(dtype)[6:]:9s} |d| / bound = {r:.4f} (fp32 store: margin {1 / r:.0f} x)")
    assert r <= 0.05, r  # two operand roundings of 2^-24 each against 512 2^-24 sum|ab|: at most 2 / 512


GEMV_SHAPES = [(1, 264, 4096), (3, 515, 272), (2, 256, 11008), (13, 515, 2112), (8, 72, 144)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,Nn,K", GEMV_SHAPES)
def test_fp8_weight_gemv_model_accepted_and_mutants_rejected(dtype, M, Nn, K):
    nb = (K + 127) // 128
    x, resid = rnd(M, K, dtype=dtype), rnd(M, Nn, dtype=dtype, seed=2)
    w = block_scaled(rnd(Nn, K, dtype=dtype, seed=1, scale=0.5), zero_row=7, zero_block=(9, nb - 1))
    q, sc = N.quant_b128(w)
    assert float(sc[7].min()) == 1.0 == float(sc[9, nb - 1]) and int(q[7].max()) == 0
    assert float((N.deq64_b128(q, sc) - w.double()).abs().max()) <= 2.0 ** -4 * float(w.float().abs().max())  # the dequantiser inverts the quantiser
    lims = {}
    for od, rs in ((dtype, None), (dtype, resid), (torch.float32, None), (torch.float32, resid)):
        ref, Bc = N.gemv_fp8w(x, q, sc, rs, out_dtype=od)
        c = N.componentwise(N.gemv_fp8w(x, q, sc, rs, out_dtype=od, model=dtype), ref, Bc, N.EPS16[od], N.TINY[od])[0]
        print(f"model  gemv fp8w {M}x{Nn}x{K} {'+resid' if rs is not None else '      '} {str(dtype)[6:]:9s} -> {str(od)[6:]:9s} c = {c:.3f}")
        assert c <= (1.0 if od == dtype else 0.5), (od, c)  # one rounding at a 16-bit store; fp32: B is the worst case of a K-term sum
        lims[(od, rs is not None)] = N.limit(c)
    X, Q, S = x.double(), N.e4m3(q), sc.double()
    bs = N._block_sums(X, Q)  # [M, N, nb]
    ref, Bc = N.gemv_fp8w(x, q, sc, resid)
    lim = lims[(dtype, True)]

    def rej(name, got, old_limit=3.0):
        g = got.to(dtype)
        c = score(g, ref, Bc, dtype)
        om = old_metric(g, ref, dtype)
        print(f"mutant {name:44s} {M}x{Nn}x{K} {str(dtype)[6:]:9s} c = {c:9.1f} limit = {lim:.2f}   old metric = {om:7.2f} eps16 "
              f"(limit {old_limit}: {'PASSES' if om < old_limit else 'caught'})")
        assert c >= 2 * lim, (name, c, lim)

    if K % 128:
        S2 = S.clone(); S2[:, nb - 1] = S[:, nb - 2]
        rej("partial last block takes the previous scale", (bs * S2[None]).sum(-1) + resid.double())
    n0 = 4  # a row whose first block has exponent 0
    lane = ref.clone(); lane[:, n0] -= S[n0, 0] * (X[:, 16:32] @ Q[n0, 16:32])
    rej("one lane's 16 values skipped", lane)
    S2 = S.clone(); S2[n0] = S[n0 + 1]
    rej("a row reads its neighbour's scales", (bs * S2[None]).sum(-1) + resid.double())
    nores = ref.clone(); nores[M - 1] -= resid[M - 1].double()
    rej("residual skipped for row M - 1", nores)
    if K > 2048:
        idx = torch.arange(nb)
        idx = torch.where(idx >= 16, idx - 16, idx)
        rej("second K chunk starts again at block 0", (bs * S[:, idx][None]).sum(-1) + resid.double())
