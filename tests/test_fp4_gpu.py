"""MXFP4 decode weights (csrc/decode.hip: mh_quant_fp4_b32, mh_gemv_fp4w, mh_gemv_fp4w_norm, mh_gemv_fp4w_qkv_rope; generate(fp4_weights=True)).

Quantiser:  dequantised values bit-exact against the torch restatement (tests/numerics_fp4.py), hand-built edge blocks included.
GEMV:       numerics.componentwise with limit(c_model) on every arm of the launcher, which arm a case takes asserted from the launcher's own
            conditions; every launch runs twice and must repeat its bits.  Lines printed: `CW | ...`.
Fused:      norm / SwiGLU / q|k|v + RoPE + append forms equal the separate launches bit for bit.
generate(): on the tiny model with its decoder weights snapped to the fp4 grid the fp4 path is the 16-bit path on the same weights: greedy
            against the CPU oracle, fp8 KV cache and beams against the 16-bit HIP path, seeded sampling repeatable."""
import dataclasses
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import numerics as N  # noqa: E402
import numerics_fp4 as F4  # noqa: E402

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


def twice(fn):
    """fn() two times: the launches must be bit-identical."""
    a, b = fn(), fn()
    assert torch.equal(a, b), "two launches of the same product differ"
    return a


def block_scaled_weights(Nn, K, dtype):
    """Blocks of 32 scaled by 2^-((n + kb) % 4), one all-zero row (7) and one all-zero block (row 9 where there is one, the last block)."""
    nb = K // 32
    w = rnd(Nn, K, dtype=dtype, seed=1, scale=0.5).float()
    f = torch.ldexp(torch.ones(Nn, nb), -((torch.arange(Nn)[:, None] + torch.arange(nb)[None, :]) % 4).to(torch.int32)).to(dev())
    w = w * f.repeat_interleave(32, dim=1)
    w[7] = 0
    if Nn > 9:
        w[9, (nb - 1) * 32:] = 0
    return w.to(dtype)


# ---- quantiser -----------------------------------------------------------------------------------------------------------------------------
TIES = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]


def edge_blocks(dtype):
    """Hand-built 32-element blocks (float64 values, all representable in `dtype`) and the scale byte each must get (None: not pinned here)."""
    fi = torch.finfo(dtype)
    z = lambda: torch.zeros(32, dtype=torch.float64)  # noqa: E731
    out = [(z(), 127)]                                                        # all-zero block: e = 0, codes 0
    for top, e in ((6.0, -3), (4.0, -3), (3.0, -4)):                          # amax exactly 6, 4, 3 times 2^-3
        b = z(); b[5] = -top * 2.0 ** -3; b[6:12] = torch.tensor([0.3, -0.2, 0.11, 0.05, -0.37, 0.01]).to(dtype).double(); out.append((b, e + 127))
    b = z(); b[0] = 0.75 * 2.0 ** -2; b[1] = 0.1; out.append((b.to(dtype).double(), -5 + 127))          # m exactly 0.75: e = ex - 3
    b = z(); b[0] = 0.1875 + 0.125 * fi.eps; b[1] = 0.1; out.append((b.to(dtype).double(), -4 + 127))  # one step above: e = ex - 2
    assert float(out[-1][0][0]) > 0.1875 and float(out[-1][0][0]) == float(torch.nextafter(torch.tensor(0.1875, dtype=dtype), torch.tensor(1.0, dtype=dtype)))
    b = z(); b[:7] = torch.tensor(TIES, dtype=torch.float64); b[7:14] = -b[:7]; b[31] = 6.0; out.append((b * 2.0 ** -4, -4 + 127))  # every tie, both signs
    tiny = 2.0 ** -130 if dtype == torch.bfloat16 else 2.0 ** -24                                     # clamped exponent (bf16) / smallest fp16 subnormal
    b = z(); b[3] = tiny; b[4] = -tiny / 2 if dtype == torch.bfloat16 else 0.0; out.append((b, 1 if dtype == torch.bfloat16 else -26 + 127))
    b = z(); b[0] = fi.max; b[1] = -fi.max / 2; b[2] = fi.max / 4; b[3] = 1.5 * 2.0 ** (math.floor(math.log2(fi.max)) - 2); out.append((b, None))           # the largest finite value
    if dtype == torch.bfloat16:
        b = z(); b[2] = 2.0 ** -127; b[3] = -2.0 ** -128; b[4] = 2.0 ** -126 * 1.5; out.append((b, 1))   # fp32-subnormal values at the clamped exponent
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Nn,K", [(9, 32), (515, 288), (264, 4096)])
def test_quantiser_values_bit_exact(ops, dtype, Nn, K):
    nb = K // 32
    w = block_scaled_weights(Nn, K, dtype).cpu().double().view(Nn * nb, 32)
    edges = edge_blocks(dtype)
    for i, (blk, _) in enumerate(edges):
        at = (i if i < 7 else i + 1) if (Nn, K) == (9, 32) else i  # (9, 32): one block per row, row 7 stays the all-zero row
        if at < Nn * nb:
            w[at] = blk
    w16 = w.view(Nn, K).to(dtype)
    assert torch.equal(w16.double(), w.view(Nn, K)), "an edge value is not representable"
    q, sc = ops.quant_fp4_b32(w16.to(dev()))
    assert q.shape == (Nn, K // 2) and sc.shape == (Nn, nb) and q.dtype == sc.dtype == torch.uint8
    qr, sr = F4.quant(w16)
    assert torch.equal(sc.cpu(), sr), f"{int((sc.cpu() != sr).sum())} scale bytes differ"
    got, want = F4.dequant(q, sc), F4.dequant(qr, sr)
    assert torch.equal(got, want), f"{int((got != want).sum())} values differ"   # (+0 and -0 compare equal)
    assert int(sc[7].min()) == int(sc[7].max()) == 127 and int((q[7] & 0x77).max()) == 0  # the all-zero row: scale byte 127, codes 0
    scf = sc.cpu().view(-1)
    for i, (_, byte) in enumerate(edges):
        at = (i if i < 7 else i + 1) if (Nn, K) == (9, 32) else i
        if byte is not None and at < Nn * nb:
            assert int(scf[at]) == byte, (i, int(scf[at]), byte)


def test_quantiser_refuses_partial_blocks(ops):
    with pytest.raises(ValueError, match="K = 40"):
        ops.quant_fp4_b32(rnd(4, 40))


# ---- the fp4-weight GEMV, every arm ------------------------------------------------------------------------------------------------------
def gemv_arm(M, Nn, K, mfma_min):
    """The kernel csrc/decode.hip gemv_fp4w_impl launches for a plain projection, from its own conditions (mfma_min = 3 by default, 17 = never)."""
    if M >= mfma_min and K % 64 == 0:
        return "mfma 64 rows" if Nn >= 30000 else "mfma 32 rows" if Nn >= 12000 else "mfma"
    assert M <= 8
    if M >= 3 and Nn >= 8192:
        return "wave per row pair"   # two weight rows per wave, activations through LDS
    return "wave per row, LDS" if M >= 3 else "wave per row"  # 1-2 rows read the activations straight from memory, K loop not chunked


# (M, N, K, MFMA row threshold, the arm that must run).  K = 2080 crosses one full wave step of 2048 values, 4128 two (and, with LDS staging,
# two chunks of the K loop); N = 515 leaves the last block of waves ragged; N = 8200 gives two rows per wave; K = 2112 and 192 leave the scale
# rows of the MFMA form unaligned (four byte loads per step), K = 4096 and 128 aligned (one dword load), 192 and 2112 end in a half step.
GEMV_CASES = [
    (1, 515, 288, 17, "wave per row"),
    (2, 264, 2080, 17, "wave per row"),
    (1, 515, 4128, 17, "wave per row"),
    (3, 515, 288, 17, "wave per row, LDS"),
    (8, 515, 2080, 17, "wave per row, LDS"),
    (3, 515, 4128, 17, "wave per row, LDS"),
    (5, 264, 288, 0, "wave per row, LDS"),      # default threshold, K % 64 != 0: no MFMA form
    (3, 8200, 288, 17, "wave per row pair"),
    (3, 515, 2112, 0, "mfma"),
    (5, 264, 4096, 0, "mfma"),
    (9, 515, 192, 0, "mfma"),
    (16, 515, 2112, 0, "mfma"),
    (4, 12040, 128, 0, "mfma 32 rows"),
    (3, 30010, 64, 0, "mfma 64 rows"),
]


def hold(name, dtype, got, ref, B, model, od):
    cm, _ = N.componentwise(model, ref, B, N.EPS16[od], N.TINY[od])
    ck, at = N.componentwise(got.cpu(), ref, B, N.EPS16[od], N.TINY[od])
    lim = N.limit(cm)
    print(f"CW | {name} | {str(dtype)[6:]} -> {str(od)[6:]} | {cm:.3f} | {ck:.3f} | {lim:.3f} | worst at {at}")
    assert ck <= lim, f"{name} {dtype}: kernel c = {ck:.3f} at {at} exceeds {lim:.3f} (model c = {cm:.3f})"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,Nn,K,mfma_min,arm", GEMV_CASES)
def test_fp4_weight_gemv_every_arm_per_element(ops, dtype, M, Nn, K, mfma_min, arm):
    assert gemv_arm(M, Nn, K, mfma_min or 3) == arm
    nb = K // 32
    x, resid = rnd(M, K, dtype=dtype), rnd(M, Nn, dtype=dtype, seed=2)
    qw = ops.quant_fp4_b32(block_scaled_weights(Nn, K, dtype))
    q, sc = qw
    assert int(sc[7].min()) == 127 == int(sc[7].max()) == int(sc[9, nb - 1]) and int((q[7] & 0x77).max()) == 0
    if nb >= 4:  # the scales of a row really differ from block to block
        assert bool((sc[16:32].max(1).values >= sc[16:32].min(1).values + 2).all())
    tag = f"gemv fp4w {arm} {M}x{Nn}x{K}"
    try:
        ops.gemv_mfma_min_rows(mfma_min)
        assert M <= ops._gemv_fp4_rows_per_launch(K)  # one launch
        got16 = twice(lambda: ops.gemv_fp4w(x, qw))
        gotr = twice(lambda: ops.gemv_fp4w(x, qw, resid=resid))
        got32 = twice(lambda: ops.gemv_fp4w(x, qw, out_f32=True))
    finally:
        ops.gemv_mfma_min_rows(0)
    ref, B = F4.gemv_fp4w(x, q, sc)
    hold(f"{tag} 16-bit", dtype, got16, ref, B, F4.gemv_fp4w(x, q, sc, model=dtype), dtype)
    assert float(got16[:, 7].abs().max()) == 0.0  # the all-zero weight row: exactly 0 ...
    assert torch.equal(gotr[:, 7], resid[:, 7])    # ... or exactly the residual
    ref, B = F4.gemv_fp4w(x, q, sc, resid)
    hold(f"{tag} +resid", dtype, gotr, ref, B, F4.gemv_fp4w(x, q, sc, resid, model=dtype), dtype)
    ref, B = F4.gemv_fp4w(x, q, sc, out_dtype=F32)
    hold(f"{tag} fp32", dtype, got32, ref, B, F4.gemv_fp4w(x, q, sc, out_dtype=F32, model=dtype), F32)


# ---- fused forms, bit for bit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K,mfma_min", [(1, 288, 0), (2, 2112, 0), (3, 288, 17), (8, 2112, 17), (8, 2112, 0), (16, 2112, 0)])
def test_fused_norm_and_swiglu_equal_the_separate_launches(ops, dtype, M, K, mfma_min):
    """gemv_fp4w_norm = rmsnorm_fwd + gemv_fp4w, and swiglu=True = swiglu_fwd of that projection.  17: every form one wave per row (pair);
    0: the default thresholds, where from 4 rows on both sides run the MFMA form (the same order of summation)."""
    ff = 264  # (swiglu_fwd takes whole 8-element groups)
    x, g = rnd(M, K, dtype=dtype), rnd(K, dtype=dtype, seed=3)
    qw = ops.quant_fp4_b32(block_scaled_weights(2 * ff, K, dtype))
    try:
        ops.gemv_mfma_min_rows(mfma_min)
        ref = ops.gemv_fp4w(ops.rmsnorm_fwd(x, g, 1e-6), qw)
        got = twice(lambda: ops.gemv_fp4w_norm(x, g, 1e-6, qw))
        act = twice(lambda: ops.gemv_fp4w_norm(x, g, 1e-6, qw, swiglu=True))
    finally:
        ops.gemv_mfma_min_rows(0)
    assert torch.equal(got, ref)
    assert act.shape == (M, ff) and torch.equal(act, ops.swiglu_fwd(ref))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("M", [1, 2, 5, 8, 9])
def test_qkv_rope_append_equals_the_three_launches(ops, dtype, D, M):
    """gemv_qkv_rope with the fp4 pair = rmsnorm_fwd + gemv_fp4w + decode_rope_append: qkv, the cache rows at pos; every other cache row
    untouched; the rotary position differs from the cache row.  9 rows: the fallback (the separate launches themselves)."""
    H, K, Smax = 2, 288, 12
    d = H * D
    x, g = rnd(M, K, dtype=dtype), rnd(K, dtype=dtype, seed=3)
    qw = ops.quant_fp4_b32(block_scaled_weights(3 * d, K, dtype))
    tab = ops.rope_table(Smax + 8, D, 10000.0, dev())
    pos = torch.tensor([(3 * i + 1) % Smax for i in range(M)], dtype=torch.int32, device=dev())
    rpos = (pos + torch.arange(M, dtype=torch.int32, device=dev()) % 3 + 2).to(torch.int32)
    kc0, vc0 = rnd(M, Smax, d, dtype=dtype, seed=5), rnd(M, Smax, d, dtype=dtype, seed=6)
    try:
        ops.gemv_mfma_min_rows(17)  # the reference projection as one wave per row: the summation order of the fused form
        ref = ops.gemv_fp4w(ops.rmsnorm_fwd(x, g, 1e-6), qw)
    finally:
        ops.gemv_mfma_min_rows(0)
    kc1, vc1 = kc0.clone(), vc0.clone()
    ops.decode_rope_append(ref, tab, pos, kc1, vc1, H, D, rope_pos=rpos)
    kc2, vc2 = kc0.clone(), vc0.clone()
    try:
        if M > 8:
            ops.gemv_mfma_min_rows(17)
        got = ops.gemv_qkv_rope(x, g, 1e-6, qw, tab, pos, kc2, vc2, H, D, rope_pos=rpos)
    finally:
        ops.gemv_mfma_min_rows(0)
    assert torch.equal(got, ref)
    assert torch.equal(kc2, kc1) and torch.equal(vc2, vc1)
    untouched = torch.ones(M, Smax, dtype=torch.bool, device=dev())
    untouched[torch.arange(M, device=dev()), pos.long()] = False
    assert torch.equal(kc2[untouched], kc0[untouched]) and torch.equal(vc2[untouched], vc0[untouched])
    assert not torch.equal(kc2[~untouched], kc0[~untouched])


# ---- engine and generate() on the tiny model, snapped to the grid -------------------------------------------------------------------------
GAIN, EOS = 25.0, 96


def _snap(m):
    """Every decoder Linear weight and lm_head replaced by dequant(quant(w)); -> {name: snapped fp32 cpu tensor}."""
    snapped = {}
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name == "lm_head.weight" or (name.startswith("model.layers.") and name.endswith("_proj.weight")):
                v = F4.dequant(*F4.quant(p.data)).to(p.dtype)
                p.copy_(v.to(p.device))
                snapped[name] = v.float()
    m.engine.weights_changed()
    return snapped


@pytest.fixture(scope="module")
def tiny():
    from test_generation_gpu import _model

    cfg, batch, m = _model("tiny_1img", GAIN)
    snapped = _snap(m)
    assert len(snapped) == 7 * cfg.num_hidden_layers + 1
    ids = batch["input_ids"][:, :22]
    return dict(cfg=cfg, batch=batch, m=m, snapped=snapped, ids_cpu=ids, ids=ids.cuda(), images=[im.cuda() for im in batch["images"]])


def _oracle_fn(t):
    from oracle import ref_cpu as R

    P = R.make_params(t["cfg"], seed=0)
    P["model.norm.weight"] = P["model.norm.weight"] * GAIN
    for name, v in t["snapped"].items():
        assert P[name].shape == v.shape or name == "lm_head.weight"
        P[name] = v[:P[name].shape[0]].to(P[name].dtype)
    images = t["batch"]["images"]

    def fn(x):
        with torch.no_grad():
            imgs = images * x.shape[0] if x.shape[0] > len(images) else images
            return R.forward(P, t["cfg"], x, None, None, imgs)[1][:, -1, :]
    return fn


def _same_or_16bit_tie(t, got, want, tag):
    """Equal tokens; or, at the first difference, the two candidates' scores on the 16-bit path (logits after the common prefix) are within
    the 2e-3 max|score| tie rule of test_generation_gpu._same_or_tie."""
    if got.tolist() == want.tolist():
        return
    n = min(got.shape[1], want.shape[1])
    diff = (got[:, :n] != want[:, :n]).any(0)
    assert bool(diff.any()), (tag, got.tolist(), want.tolist())
    k = int(diff.nonzero()[0])
    assert k >= t["ids"].shape[1], (tag, got.tolist(), want.tolist())
    b = int((got[:, k] != want[:, k]).nonzero()[0])
    with torch.no_grad():
        lg = t["m"](input_ids=want[b:b + 1, :k].cuda(), images=t["images"][b:b + 1]).logits[0, -1].float()
    gap = abs(float(lg[int(got[b, k])] - lg[int(want[b, k])]))
    assert gap < 2e-3 * float(lg.abs().max()), (tag, "diverged at", k, "without a tie", gap, got.tolist(), want.tolist())


def test_greedy_fp4_generate_matches_the_oracle_on_snapped_weights(tiny):
    from oracle import gen_ref as G
    from test_generation_gpu import _same_or_tie

    m, kw = tiny["m"], dict(images=tiny["images"], max_new_tokens=12, eos_token_id=EOS, pad_token_id=0)
    want = G.sample(_oracle_fn(tiny), tiny["ids_cpu"], 12, eos_ids=[EOS], pad=0)
    for extra in (dict(), dict(use_graph=False)):
        got = m.generate(tiny["ids"], fp4_weights=True, **kw, **extra).cpu()
        _same_or_tie(m, tiny["images"], got, want, 22, extra)
    assert m.engine._fp4 is not None and len(m.engine._fp4["layers"]) == tiny["cfg"].num_hidden_layers
    # the copies ARE the weights: quantising a snapped matrix gives the same values back
    W0, Q0 = m.engine.llama[0], m.engine._fp4["layers"][0]
    for a, b in ((W0.wqkv, Q0["wqkv"]), (W0.wo, Q0["wo"]), (W0.wgu, Q0["wgu"]), (W0.wd, Q0["wd"])):
        assert torch.equal(F4.dequant(*b), a.cpu().double())


def test_fp4_with_fp8_kv_beams_and_sampling(tiny):
    m, ids = tiny["m"], tiny["ids"]
    kw = dict(images=tiny["images"], max_new_tokens=10, eos_token_id=EOS, pad_token_id=0)
    for opt in (dict(fp8_kv=True), dict(fp8_kv=True, use_graph=False), dict(num_beams=5), dict(num_beams=5, fp8_kv=True)):
        want = m.generate(ids, **kw, **opt).cpu()
        got = m.generate(ids, fp4_weights=True, **kw, **opt).cpu()
        _same_or_16bit_tie(tiny, got, want, opt)
    skw = dict(images=tiny["images"], max_new_tokens=10, eos_token_id=-1, do_sample=True, temperature=1.5, seed=11)
    a, b = m.generate(ids, fp4_weights=True, **skw), m.generate(ids, fp4_weights=True, **skw)
    c = m.generate(ids, fp4_weights=True, use_graph=False, **skw)
    assert torch.equal(a, b) and torch.equal(a, c) and a.shape == (1, 32)


def test_fp4_copies_follow_the_weights(tiny):
    """After a weight changes and weights_changed() the fp4 path gives what a freshly built model with that weight gives."""
    from test_generation_gpu import _model

    m, ids = tiny["m"], tiny["ids"]
    kw = dict(images=tiny["images"], max_new_tokens=6, eos_token_id=-1, fp4_weights=True, use_graph=False)
    before = m.generate(ids, **kw)
    name = "model.layers.1.mlp.down_proj.weight"
    p = dict(m.named_parameters())[name]
    keep = p.detach().clone()
    g = torch.Generator().manual_seed(5)
    new = (torch.randn(p.shape, generator=g) * 0.08).to(p.dtype).to(p.device)
    try:
        with torch.no_grad():
            p.copy_(new)
        m.engine.weights_changed()
        assert m.engine._fp4 is None
        changed = m.generate(ids, **kw)
        _, _, fresh = _model("tiny_1img", GAIN)
        _snap(fresh)
        with torch.no_grad():
            dict(fresh.named_parameters())[name].copy_(new)
        fresh.engine.weights_changed()
        assert torch.equal(changed, fresh.generate(ids, **kw))
        assert not torch.equal(changed, before), "the changed weight did not reach the fp4 copies"
    finally:
        with torch.no_grad():
            p.copy_(keep)
        m.engine.weights_changed()
    assert torch.equal(m.generate(ids, **kw), before)


def test_fp4_errors(tiny, ops):
    from oracle import cases as C
    from test_model_gpu import _build

    m, ids = tiny["m"], tiny["ids"]
    kw = dict(images=tiny["images"], max_new_tokens=3)
    with pytest.raises(ValueError, match="fp4_weights"):
        m.generate(ids, fp4_weights=True, fp8_weights=True, **kw)
    with pytest.raises(ValueError, match="use_cache"):
        m.generate(ids, fp4_weights=True, use_cache=False, **kw)
    logits, cache = m.engine.prefill(ids, None, tiny["images"], 4)
    with pytest.raises(ValueError, match="fp8 and fp4"):
        m.engine.decode_step(logits.argmax(-1), cache, fp8=True, fp4=True)
    with pytest.raises(ValueError, match="fp8 and fp4"):
        m.engine.capture_decode_graph(cache, fp8=True, fp4=True)
    cfg, _ = C.get_case("tiny_1img")
    for field, value in (("hidden_size", 272), ("intermediate_size", 528)):
        odd = _build(dataclasses.replace(cfg, **{field: value}), torch.bfloat16)
        with pytest.raises(ValueError, match=f"{field} = {value}"):
            odd.engine.quantize_decode_weights_fp4()
