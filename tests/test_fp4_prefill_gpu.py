"""MXFP4 weights for the prompt: the many-row product mh_gemm_fp4w (csrc/gemm_fp4w.hip) and the prefill / full-sequence forward built on it
(engine.forward(fp4=True), prefill / extend(w_fp4=True), model.fp4_forward, generate(fp4_prefill=True)).

GEMM:       the harness of test_fp4_gpu.py (block_scaled_weights, twice, hold) with numerics_fp4.gemv_fp4w as reference, bound and model - the
            mathematics is that of the decode GEMV, M is free.  Both dtypes, the four store forms, shapes chosen for the tile edges.  Lines
            printed: `CW | ...`.
Placement:  one nonzero code per weight row and an x of ones: the stored nibble order and the scale block of every k position, exactly.
Engine:     on the tiny model with weights that are NOT on the e2m1 grid the fp4 forward / prefill is the 16-bit model on the snapped twin:
            logits and loss against the CPU oracle within the 16-bit path's own bounds, generate() against the twin, prefill against
            prefill + decode steps and against extend, sessions that remember which weight format wrote their rows."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import numerics_fp4 as F4  # noqa: E402
from test_fp4_gpu import DTYPES, EOS, F32, GAIN, _same_or_16bit_tie, _snap, block_scaled_weights, dev, hold, rnd, twice  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from merlin_amd import ops as O

    assert O.arch_ok(0), "not a gfx950 device"
    return O


# ---- the many-row product, per element -----------------------------------------------------------------------------------------------------
# (M, N, K): 17 x 515 x 288 - one ragged tile each way, K ends in a half K-tile; 130 / 264 - two M tiles, three N tiles, 2080 = 32 K-tiles and
# a half; 257 x 515 x 4128 - three M tiles, the longest contraction; 613 x 48 - the prompt length of the benchmark against less than one N
# tile; 8200 columns at a single scale block; 1 x 9 x 64 - a single row, a single whole K-tile.
GEMM_CASES = [(17, 515, 288), (130, 264, 2080), (257, 515, 4128), (613, 48, 4096), (33, 8200, 32), (1, 9, 64)]


def _refs(x, q, sc, extra, od):
    """(ref64, B, model) of numerics_fp4.gemv_fp4w for one store form (extra: the 16-bit resid / the prior fp32 out, or None)."""
    ref, B = F4.gemv_fp4w(x, q, sc, extra, out_dtype=od)
    return ref, B, F4.gemv_fp4w(x, q, sc, extra, out_dtype=od, model=x.dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,Nn,K", GEMM_CASES)
def test_fp4_weight_gemm_every_store_form_per_element(ops, dtype, M, Nn, K):
    nb = K // 32
    x, resid = rnd(M, K, dtype=dtype), rnd(M, Nn, dtype=dtype, seed=2)
    prior = rnd(M, Nn, dtype=F32, seed=4)
    qw = ops.quant_fp4_b32(block_scaled_weights(Nn, K, dtype))
    q, sc = qw
    assert int(sc[7].min()) == 127 == int(sc[7].max()) and int((q[7] & 0x77).max()) == 0  # the all-zero weight row
    if Nn > 9:
        assert int(sc[9, nb - 1]) == 127
    tag = f"gemm fp4w {M}x{Nn}x{K}"
    got16 = twice(lambda: ops.gemm_fp4w(x, qw))
    gotr = twice(lambda: ops.gemm_fp4w(x, qw, resid=resid))
    got32 = twice(lambda: ops.gemm_fp4w(x, qw, out_f32=True))
    gota = twice(lambda: ops.gemm_fp4w(x, qw, out=prior.clone(), accum=True))
    assert got16.dtype == gotr.dtype == dtype and got32.dtype == gota.dtype == F32
    hold(f"{tag} 16-bit", dtype, got16, *_refs(x, q, sc, None, dtype), dtype)
    hold(f"{tag} +resid", dtype, gotr, *_refs(x, q, sc, resid, dtype), dtype)
    hold(f"{tag} fp32", dtype, got32, *_refs(x, q, sc, None, F32), F32)
    hold(f"{tag} fp32 +=", dtype, gota, *_refs(x, q, sc, prior, F32), F32)
    assert float(got16[:, 7].abs().max()) == 0.0 and float(got32[:, 7].abs().max()) == 0.0  # the all-zero weight row: exactly 0 ...
    assert torch.equal(gotr[:, 7], resid[:, 7]) and torch.equal(gota[:, 7], prior[:, 7])    # ... or exactly the residual / the prior out


@pytest.mark.parametrize("dtype", DTYPES)
def test_five_rows_hold_the_bound_of_the_gemv(ops, dtype):
    """One launch of M = 5: the GEMM and the decode GEMV on the same operands, each within the same bound (not bit equality: the GEMV scales
    fp32 block sums, the GEMM sums scaled products)."""
    M, Nn, K = 5, 515, 2112
    x = rnd(M, K, dtype=dtype)
    qw = ops.quant_fp4_b32(block_scaled_weights(Nn, K, dtype))
    refs = _refs(x, *qw, None, dtype)
    hold(f"gemm fp4w {M}x{Nn}x{K}", dtype, twice(lambda: ops.gemm_fp4w(x, qw)), *refs, dtype)
    hold(f"gemv fp4w {M}x{Nn}x{K}", dtype, ops.gemv_fp4w(x, qw), *refs, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pad_n", [5, 8])  # out / resid rows of 520 elements: the vector stores and their ragged last quad; 523: element stores
def test_strided_operands_and_the_footprint(ops, dtype, pad_n):
    """x, out and resid as views of larger poisoned buffers (ld > width): the result is that of the contiguous call and the columns beyond N and
    the rows beyond M are unchanged."""
    M, Nn, K = 70, 515, 288
    xb = torch.full((M + 3, K + 8), float("nan"), dtype=dtype, device=dev())
    xb[:M, :K] = rnd(M, K, dtype=dtype)
    x = xb[:M, :K]
    rb = torch.full((M + 1, Nn + pad_n), 3.0, dtype=dtype, device=dev())
    rb[:M, :Nn] = rnd(M, Nn, dtype=dtype, seed=2)
    resid = rb[:M, :Nn]
    qw = ops.quant_fp4_b32(block_scaled_weights(Nn, K, dtype))
    q, sc = qw
    for form, od in (("16-bit", dtype), ("+resid", dtype), ("fp32", F32), ("fp32 +=", F32)):
        poison = -77.0
        ob = torch.full((M + 2, Nn + pad_n), poison, dtype=od, device=dev())
        extra = None
        if form == "fp32 +=":
            ob[:M, :Nn] = rnd(M, Nn, dtype=F32, seed=4)
            extra = ob[:M, :Nn].clone()
        elif form == "+resid":
            extra = resid
        before = ob.clone()
        ret = ops.gemm_fp4w(x, qw, out=ob[:M, :Nn], resid=resid if form == "+resid" else None, accum=form == "fp32 +=")
        assert ret.data_ptr() == ob.data_ptr()
        hold(f"gemm fp4w strided ld {Nn + pad_n} {form}", dtype, ob[:M, :Nn], *_refs(x.contiguous(), q, sc, extra, od), od)
        assert torch.equal(ob[:M, :Nn], ops.gemm_fp4w(x.contiguous(), qw, out=before[:M, :Nn].contiguous(), resid=extra if form == "+resid" else None,
                                                     accum=form == "fp32 +="))
        assert torch.equal(ob[M:], before[M:]) and torch.equal(ob[:, Nn:], before[:, Nn:]), f"{form}: the launch wrote outside [M, N]"
    assert float(rb[M:].min()) == 3.0 and float(rb[:, Nn:].min()) == 3.0


# ---- nibble and scale placement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("byte", [120, 131])
@pytest.mark.parametrize("K", [96, 128])  # 96: K - 1 lies in the half K-tile at the end
def test_single_code_lands_at_its_k_with_its_block_scale(ops, dtype, byte, K):
    """Weight row i holds ONE nonzero code, at k = ks[i], in a block whose scale byte is `byte` (every other block of the row carries another
    scale); x = 1: column i is exactly code * 2^(byte - 127), for both signs, and nothing else is nonzero.  A swapped nibble pair or byte
    order would move the code to a k whose x is 0 in the second pass (x = 1 at k alone), a wrong scale block would change the power of two."""
    ks = [0, 1, 7, 8, 31, 32, 33, 63, K - 1]
    Nn, M = 2 * len(ks) + 1, 3
    q = torch.zeros(Nn, K // 2, dtype=torch.uint8)
    sc = torch.full((Nn, K // 32), 127 + 9, dtype=torch.uint8)
    want = torch.zeros(M, Nn, dtype=torch.float64)
    for i, k in enumerate(ks):
        for sign in (0, 1):
            n = 2 * i + sign
            code = 3 | (sign << 3)  # +-1.5: exponent and mantissa bits both set
            q[n, k // 2] = code << (4 * (k % 2))
            sc[n, k // 32] = byte
            want[:, n] = (-1.5 if sign else 1.5) * 2.0 ** (byte - 127)
    qd, scd = q.to(dev()), sc.to(dev())
    assert torch.equal(F4.dequant(q, sc).sum(1), want[0])
    ones = torch.ones(M, K, dtype=dtype, device=dev())
    for f32 in (False, True):
        got = twice(lambda: ops.gemm_fp4w(ones, (qd, scd), out_f32=f32)).cpu().double()
        assert torch.equal(got, want), (f32, got[0].tolist(), want[0].tolist())
    for i, k in enumerate(ks):  # x = 1 at k alone: only columns 2 i, 2 i + 1 (and those of an equal k) answer
        e = torch.zeros(M, K, dtype=dtype, device=dev())
        e[:, k] = 1
        got = ops.gemm_fp4w(e, (qd, scd), out_f32=True).cpu().double()
        sel = torch.tensor([kk == k for kk in ks for _ in (0, 1)] + [False])
        assert torch.equal(got[:, sel], want[:, sel]) and float(got[:, ~sel].abs().max()) == 0.0, (k, got[0].tolist())


# ---- errors: raised, nothing launched ----------------------------------------------------------------------------------------------------
def test_gemm_refusals(ops):
    from merlin_amd import _lib as L

    x, x40 = rnd(4, 64), rnd(4, 40)
    qw = ops.quant_fp4_b32(rnd(16, 64))
    out32, out16 = torch.full((4, 16), 5.0, device=dev()), torch.full((4, 16), 5.0, dtype=torch.bfloat16, device=dev())
    q40 = (torch.zeros(16, 20, dtype=torch.uint8, device=dev()), torch.ones(16, 1, dtype=torch.uint8, device=dev()))
    with pytest.raises(ValueError, match="K = 40"):
        ops.gemm_fp4w(x40, q40)
    with pytest.raises(ValueError, match="accum"):
        ops.gemm_fp4w(x, qw, out=out16, accum=True)
    with pytest.raises(ValueError, match="resid"):
        ops.gemm_fp4w(x, qw, out=out32, resid=out16, accum=True)
    with pytest.raises(ValueError, match="resid"):
        ops.gemm_fp4w(x, qw, resid=out16, out_f32=True)
    # the launcher itself: MH_ERR_ARG and no launch for the same, and for null pointers
    err, s = L.DEFINES["MH_ERR_ARG"], torch.cuda.current_stream().cuda_stream
    q, sc = qw
    for args in ((x40, 40, q40[0], q40[1], out16, 16, None, 0, 4, 16, 40, L.MH_BF16, 0, 0),
                 (x, 64, q, sc, out16, 16, None, 0, 4, 16, 64, L.MH_BF16, 0, 1),
                 (x, 64, q, sc, out32, 16, out16, 16, 4, 16, 64, L.MH_BF16, 1, 1),
                 (x, 64, q, sc, out32, 16, out16, 16, 4, 16, 64, L.MH_BF16, 1, 0),
                 (None, 64, q, sc, out16, 16, None, 0, 4, 16, 64, L.MH_BF16, 0, 0),
                 (x, 64, None, sc, out16, 16, None, 0, 4, 16, 64, L.MH_BF16, 0, 0),
                 (x, 64, q, None, out16, 16, None, 0, 4, 16, 64, L.MH_BF16, 0, 0),
                 (x, 64, q, sc, None, 16, None, 0, 4, 16, 64, L.MH_BF16, 0, 0)):
        assert L.launch("mh_gemm_fp4w", *args, s) == err
    torch.cuda.synchronize()
    assert float(out32.min()) == 5.0 == float(out32.max()) and float(out16.float().min()) == 5.0 == float(out16.float().max())


# ---- engine and model on the tiny fixture, weights NOT on the e2m1 grid --------------------------------------------------------------------
def _pair(case, n_ids):
    """(raw, twin): the fixture model with its weights as generated, and a second build whose decoder Linear weights and lm_head are snapped
    to the grid - the 16-bit model that the raw model's MXFP4 copies are."""
    from test_generation_gpu import _model

    cfg, batch, raw = _model(case, GAIN)
    _, _, twin = _model(case, GAIN)
    snapped = _snap(twin)
    moved = max(float((dict(raw.named_parameters())[k].detach().float().cpu() - v).abs().max()) for k, v in snapped.items())
    assert moved > 0, "the raw weights already lie on the grid: the fixture shows nothing"
    ids = batch["input_ids"][:, :n_ids]
    return dict(cfg=cfg, batch=batch, raw=raw, m=twin, snapped=snapped, ids_cpu=ids, ids=ids.cuda(), images=[im.cuda() for im in batch["images"]])


@pytest.fixture(scope="module")
def tiny():
    return _pair("tiny_1img", 22)


def _oracle_params(t):
    """test_fp4_gpu._oracle_fn's construction: the CPU oracle's parameters with the snapped weights."""
    from oracle import ref_cpu as R

    P = R.make_params(t["cfg"], seed=0)
    P["model.norm.weight"] = P["model.norm.weight"] * GAIN
    for name, v in t["snapped"].items():
        assert P[name].shape == v.shape or name == "lm_head.weight"
        P[name] = v[:P[name].shape[0]].to(P[name].dtype)
    return P


def test_fp4_forward_is_the_oracle_on_snapped_weights(tiny):
    """model.fp4_forward = True on the RAW model: full-sequence logits and loss against the CPU oracle on the snapped weights, all positions,
    within the bounds the 16-bit path is held to on this fixture (test_model_gpu.TOL).  Measured on MI355X (fp16): logits 5.2e-4 of the
    largest magnitude (the 16-bit weights against the same oracle: 2.1e-1), loss 7.4e-5 relative, with the separate RoPE / SwiGLU launches."""
    from oracle import ref_cpu as R
    from test_model_gpu import TOL, _to_dev

    tol, raw, batch = TOL[torch.float16], tiny["raw"], tiny["batch"]
    with torch.no_grad():
        loss_ref, ref = R.forward(_oracle_params(tiny), tiny["cfg"], batch["input_ids"], batch["attention_mask"], batch["labels"], batch["images"])
        plain = raw(**_to_dev(batch))
        raw.fp4_forward = True
        try:
            out = raw(**_to_dev(batch))
        finally:
            raw.fp4_forward = False
    mask = batch["attention_mask"].bool()
    scale = float(ref[mask].abs().max())
    err = float((out.logits.float().cpu() - ref)[mask].abs().max()) / scale
    err16 = float((plain.logits.float().cpu() - ref)[mask].abs().max()) / scale
    dl = abs(float(out.loss) - float(loss_ref)) / abs(float(loss_ref))
    print(f"FP4FWD | logits rel err {err:.3e} (bound {tol['logits_tiny']:.1e}; the 16-bit weights against the same oracle: {err16:.3e}) | loss rel err {dl:.3e} "
          f"(bound {tol['loss']:.1e})")
    assert err16 > 10 * tol["logits_tiny"], "the 16-bit weights give the snapped oracle's logits: the fixture shows nothing"
    assert err < tol["logits_tiny"], f"logits rel err {err}"
    assert dl < tol["loss"], (float(out.loss), float(loss_ref))
    assert raw.engine._fp4 is not None and len(raw.engine._fp4["layers"]) == tiny["cfg"].num_hidden_layers


def test_fp4_forward_refuses_grad_and_fp8(tiny):
    from test_model_gpu import _to_dev

    raw, b = tiny["raw"], _to_dev(tiny["batch"])
    raw.fp4_forward = True
    try:
        with pytest.raises(RuntimeError, match="fp4_forward"):
            raw(**b)  # labels under grad
        raw.fp8_forward = True
        with torch.no_grad(), pytest.raises(RuntimeError, match="fp4 and fp8"):
            raw(**b)
    finally:
        raw.fp4_forward = raw.fp8_forward = False
    with torch.no_grad():
        assert torch.isfinite(raw(**b).loss)


@pytest.mark.parametrize("opt", [dict(), dict(num_beams=5), dict(num_beams=5, share_prompt_kv=True), dict(fp8_kv=True), dict(prompt_lookup_num_tokens=3),
                                 dict(guidance_scale=1.5)], ids=lambda o: "-".join(o) or "greedy")
def test_generate_with_fp4_prefill_is_the_snapped_twin(tiny, opt):
    """generate(fp4_weights=True, fp4_prefill=True) on the raw model = generate(fp4_weights=True) on the twin whose 16-bit weights ARE the
    grid values (its 16-bit prefill and the raw model's fp4 prefill are the same model), up to the tie rule."""
    kw = dict(images=tiny["images"], max_new_tokens=10, eos_token_id=EOS, pad_token_id=0)
    want = tiny["m"].generate(tiny["ids"], fp4_weights=True, **kw, **opt).cpu()
    got = tiny["raw"].generate(tiny["ids"], fp4_weights=True, fp4_prefill=True, **kw, **opt).cpu()
    _same_or_16bit_tie(tiny, got, want, opt)
    if not opt:  # without the option the raw model's prompt runs on other weights: a different model from the first token's logits on
        eng = tiny["raw"].engine
        a, _ = eng.prefill(tiny["ids"], None, tiny["images"], 1)
        b, _ = eng.prefill(tiny["ids"], None, tiny["images"], 1, w_fp4=True)
        c, _ = tiny["m"].engine.prefill(tiny["ids"], None, tiny["images"], 1)
        V = tiny["cfg"].vocab_size
        far, near = float((a - c)[:, :V].abs().max()), float((b - c)[:, :V].abs().max())
        print(f"FP4GEN | first logits against the twin's: 16-bit prefill {far:.3e}, fp4 prefill {near:.3e}, max |logit| {float(c[:, :V].abs().max()):.3e}")
        assert near < 2e-3 * float(c[:, :V].abs().max()) < far


def _close(name, got, want, V):
    d, top = float((got - want)[:, :V].abs().max()), float(want[:, :V].abs().max())
    print(f"FP4PRE | {name} | max dev {d:.3e} | 2e-3 max|logit| = {2e-3 * top:.3e}")
    assert d < 2e-3 * top, (name, d, top)


def test_fp4_prefill_equals_shorter_prefill_plus_decode_steps_and_extend(tiny):
    """Raw model, w_fp4=True: the prompt's last logits from one prefill of P tokens, from a prefill of P - 6 and six decode_step(fp4=True),
    and from a prefill of P - 6 and ONE extend(w_fp4=True) of the last six - one model, three schedules, within the tie width."""
    eng, images, V = tiny["raw"].engine, tiny["images"], tiny["cfg"].vocab_size
    ids = tiny["batch"]["input_ids"].cuda()  # the whole sample: the image span must lie in the shorter prompt
    P = ids.shape[1]
    assert ids.shape[0] == 1 and ids[0].tolist().index(tiny["raw"].im_end_token) < P - 6
    whole, _ = eng.prefill(ids, None, images, 2, w_fp4=True)
    whole = whole.clone()
    lg, cache = eng.prefill(ids[:, :P - 6], None, images, 8, w_fp4=True)
    for i in range(P - 6, P):
        lg = eng.decode_step(ids[:, i], cache, fp4=True)
    assert int(cache.lens[0]) == P
    _close("prefill(P - 6) + 6 decode steps", lg, whole, V)
    _, c2 = eng.prefill(ids[:, :P - 6], None, images, 8, w_fp4=True)
    le = eng.extend(c2, ids[:, P - 6:], w_fp4=True)
    assert int(c2.lens[0]) == P
    _close("prefill(P - 6) + extend(6)", le, whole, V)
    far, _ = eng.prefill(ids, None, images, 2)  # (the 16-bit prefill of the raw weights is NOT within that width: the switch is live)
    assert float((far - whole)[:, :V].abs().max()) > 2e-3 * float(whole[:, :V].abs().max())


def test_fp4_extend_with_an_image_in_the_tail():
    """tiny_2img: prefill up to the second image, then a 20-token tail holding that image through extend(w_fp4=True) - tower, projector and
    splice of the tail - against the fp4 prefill of the whole prompt."""
    from test_generation_gpu import _model

    cfg, batch, m = _model("tiny_2img", GAIN)
    eng, V = m.engine, cfg.vocab_size
    ids = batch["input_ids"][:, :47].cuda()
    imgs = batch["images"][0].cuda()
    row = ids[0].tolist()
    s2 = len(row) - 1 - row[::-1].index(m.im_start_token)
    assert s2 == 27 and row.index(m.im_end_token, s2) < 47 and imgs.shape[0] == 2
    whole, _ = eng.prefill(ids, None, [imgs], 2, w_fp4=True)
    whole = whole.clone()
    _, c = eng.prefill(ids[:, :s2], None, [imgs[:1]], 24, w_fp4=True)
    got = eng.extend(c, ids[:, s2:], [imgs[1:]], pos=s2, w_fp4=True)
    assert int(c.lens[0]) == 47
    _close("image in a 20-token tail", got, whole, V)


def _fp4_tie(m, ids, images, got, want):
    """Equal tokens, or at the first difference both candidates within 2e-3 max|logit| of the maximum of the fp4 model's own logits."""
    got, want = got.cpu(), want.cpu()
    if got.tolist() == want.tolist():
        return
    P, n = ids.shape[1], min(got.shape[1], want.shape[1])
    t = int((got[0, :n] != want[0, :n]).nonzero()[0])
    assert t >= P
    lg, cache = m.engine.prefill(ids, None, images, t - P + 2, w_fp4=True)
    for tok in want[0, P:t].tolist():
        lg = m.engine.decode_step(torch.tensor([tok], device=ids.device), cache, fp4=True)
    lg = lg[0, :m.config.vocab_size].float()
    tol = 2e-3 * float(lg.abs().max())
    assert float(lg.max() - lg[int(got[0, t])]) < tol and float(lg.max() - lg[int(want[0, t])]) < tol, ("diverged at", t, got.tolist(), want.tolist())


def test_session_keeps_the_two_weight_formats_apart(tiny):
    """A 16-bit call, then an fp4-prefill call on the same prefix through one session: nothing is reused.  A second fp4 call reuses the prefix
    and gives a sessionless call's tokens."""
    m, ids, images = tiny["raw"], tiny["ids"], tiny["images"]
    more = [17, 23, 9, 41, 5, 30]
    kw = dict(images=images, max_new_tokens=6, eos_token_id=-1, pad_token_id=0)
    f4 = dict(fp4_weights=True, fp4_prefill=True)
    s = m.new_session()
    out1 = m.generate(ids, session=s, **kw)
    assert s.last["reused_tokens"] == 0 and s.w_fp4 is False and len(s.tokens) == out1.shape[1] - 1
    ids2 = torch.cat([out1, torch.tensor([more], device=out1.device)], dim=1)
    out2 = m.generate(ids2, session=s, **f4, **kw)
    assert s.last == dict(reused_tokens=0, run_tokens=ids2.shape[1], images_encoded=1) and s.w_fp4 is True, s.last
    assert m.engine.last_generate_stats["reused_tokens"] == 0
    _fp4_tie(m, ids2, images, out2, m.generate(ids2, **f4, **kw))
    held = len(s.tokens)
    ids3 = torch.cat([out2, torch.tensor([more[::-1]], device=out2.device)], dim=1)
    out3 = m.generate(ids3, session=s, **f4, **kw)
    assert s.last == dict(reused_tokens=held, run_tokens=ids3.shape[1] - held, images_encoded=0) and held == out2.shape[1] - 1, s.last
    _fp4_tie(m, ids3, images, out3, m.generate(ids3, **f4, **kw))
    m.generate(ids3, session=s, **kw)  # and back: the 16-bit call does not build on the fp4 rows
    assert s.last["reused_tokens"] == 0 and s.w_fp4 is False
