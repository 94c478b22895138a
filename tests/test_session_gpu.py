"""Sessions for generate() on the GPU: mh_attn_extend / _kv8 per element against the fp64 reference and its rounding model (the rule of
tests/test_spec_gpu.py::test_attn_decode_multi_per_element), engine.extend against sequential decode steps with a bound measured in the
same run, an image in the extended tail against the prefill of the whole prompt, and generate(session=...) in every mode against the
goldens and the plain path."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import numerics as N  # noqa: E402
from test_kv8_cpu import kv8_dequantize, kv8_quantize  # noqa: E402
from test_kv8_gpu import GAIN, _dev, _tiny, hold, rnd_rows  # noqa: E402
from test_spec_gpu import _gold_model, _same_or_greedy_tie, _step_logits  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def O():
    from merlin_amd import ops

    assert ops.arch_ok(0), "not a gfx950 device"
    return ops


# ---- kernel ------------------------------------------------------------------------------------------------------------------------------
# (B, n, H, D, Smax, lens): one query, query 0 of sequence 0 sees a single key; one row past a 16-row MFMA tile; more than one 64-row query
# tile with the second partial, and a 300-row cache that ends in a partial key tile; the last query reads the last cache row exactly
# (137 + 63 = 200); three sequences of different lengths in one launch, every horizon inside the cache (690 + 4 < 700)
EXTEND_CASES = [(2, 1, 2, 128, 40, [1, 30]), (1, 17, 4, 64, 64, [5]), (2, 70, 2, 128, 300, [1, 200]), (1, 64, 2, 64, 200, [137]),
                (3, 5, 4, 64, 700, [1, 333, 690])]
FILL = 0.3125


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,n,H,D,Smax,lens", EXTEND_CASES)
def test_attn_extend_per_element(O, dtype, B, n, H, D, Smax, lens):
    """Query (b, t) is held to N.attention_decode(q[b, t], k, v, lens[b] + t) on the dequantised cache with the limit of the rounding model
    on the same inputs (hold() of tests/test_kv8_gpu.py): the fp8 form on the fp8 cache and the 16-bit form on the exactly cast
    dequantised cache.  The output [B*n, H*D] is carved out of a larger patterned buffer whose rows behind it must keep the pattern."""
    d = H * D
    assert all(ln + n - 1 <= Smax for ln in lens)
    q = rnd_rows(B * n * H, D, dtype, seed=5, lo=0.5, hi=2.0).view(B * n, d).to(dev())
    cache = []
    for seed in (3, 4):
        c8, cs = kv8_quantize(rnd_rows(B * Smax * H, D, dtype, seed=seed).view(B, Smax, H, D))
        cache += [c8.view(B, Smax, d).to(dev()), cs.permute(0, 2, 1).contiguous().to(dev()), kv8_dequantize(c8, cs).to(dev())]
    k8, ks, k64, v8, vs, v64 = cache
    k16, v16 = k64.to(dtype).view(B, Smax, d), v64.to(dtype).view(B, Smax, d)
    assert torch.equal(k16.double().view_as(k64), k64) and torch.equal(v16.double().view_as(v64), v64)  # the cast to the 16-bit type is exact
    rows = [(b, t) for b in range(B) for t in range(n)]
    pairs = [N.attention_decode(q[b * n + t].view(H, D), k64[b], v64[b], min(lens[b] + t, Smax)) for b, t in rows]
    ref, Bc = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    mod = torch.stack([N.attention_decode(q[b * n + t].view(H, D), k64[b], v64[b], min(lens[b] + t, Smax), model=dtype) for b, t in rows])
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev())
    tag = f"n={n} Smax={Smax} lens={lens}"
    guard = 3
    for name, run in (("kv8", lambda out: O.attn_extend_kv8(q, k8, v8, ks, vs, lens_t, n, H, D, out=out)),
                      ("16-bit", lambda out: O.attn_extend(q, k16, v16, lens_t, n, H, D, out=out))):
        buf = torch.full((B * n + guard, d), FILL, dtype=dtype, device=dev())
        o = run(buf[:B * n])
        assert o.data_ptr() == buf.data_ptr()
        hold(f"attention extend {name} {tag}", dtype, o.view(B * n, H, D), ref, Bc, mod)
        assert bool((buf[B * n:] == FILL).all()), f"{name}: rows behind the output were written"


def test_attn_extend_refuses_bad_arguments(O):
    from merlin_amd._lib import MerlinHipError

    H, D, Smax = 2, 64, 32
    q = torch.zeros(4, H * D, dtype=torch.float16, device=dev())
    k = torch.zeros(1, Smax, H * D, dtype=torch.float16, device=dev())
    lens = torch.ones(1, dtype=torch.int32, device=dev())
    with pytest.raises(MerlinHipError, match="bad argument"):
        O.attn_extend(q.view(-1)[1:1 + 3 * H * D].view(3, H * D), k, k, lens, 3, H, D)  # q rows not 16-byte aligned
    with pytest.raises(MerlinHipError, match="shape not supported"):
        O.attn_extend(torch.zeros(4, 2 * 32, dtype=torch.float16, device=dev()), torch.zeros(1, Smax, 64, dtype=torch.float16, device=dev()),
                      torch.zeros(1, Smax, 64, dtype=torch.float16, device=dev()), lens, 4, 2, 32)  # D = 32


# ---- engine ------------------------------------------------------------------------------------------------------------------------------
S_EXT = 40


def _toks(V, n=S_EXT, seed=11):
    return torch.randint(3, V, (n,), generator=torch.Generator().manual_seed(seed)).cuda()


@functools.lru_cache(maxsize=None)
def _measured(dtype, kv8):
    """On the tiny fixture, S_EXT teacher-forced tokens: (a = the logits of S_EXT sequential decode_steps, the logits of one more step of
    token `nxt`, d_pre, d_rows) - d_pre = dev(full-sequence forward() logits at those positions, a), d_rows = dev(row 0 of decode_step on
    the prompt replicated to six rows, a): the two deviations test_verify_step_reproduces_sequential_decode_steps measures, in this run."""
    cfg, m, ids, images = _tiny(dtype)
    eng = m.engine
    V, P = cfg.vocab_size, ids.shape[1]
    toks = _toks(V)
    nxt = _toks(V, 1, seed=12)
    _, ca = eng.prefill(ids, None, images, S_EXT + 2, kv_fp8=kv8)
    a = [eng.decode_step(toks[t:t + 1], ca).clone() for t in range(S_EXT)]
    a_next = eng.decode_step(nxt, ca).clone()
    with torch.no_grad():
        full = m(input_ids=torch.cat([ids, toks[None, :]], dim=1), images=images).logits[0, P:P + S_EXT].float()
    _, c6 = eng.prefill(ids.repeat(6, 1), None, images * 6, S_EXT + 2, kv_fp8=kv8)
    rows = [eng.decode_step(toks[t:t + 1].repeat(6), c6)[:1].clone() for t in range(S_EXT)]
    d_pre = _dev([full[t:t + 1] for t in range(S_EXT)], a, V)
    d_rows = _dev(rows, a, V)
    return a, a_next, d_pre, d_rows


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("kv8", [False, True], ids=["kv16", "kv8"])
def test_extend_reproduces_sequential_decode_steps(dtype, kv8):
    """40 teacher-forced tokens.  (a) 40 decode_steps; (b) one extend of the 40 on a fresh prefill: its last-row logits against (a)'s 40th,
    then one more decode_step on each cache; (c) an extend of the first 25, truncate back to 10 cached generated tokens, an extend of tokens
    10..39: the same logits again, i.e. the stale rows 10..24 are ignored and overwritten; (d) the same through grow_cache.  Every deviation
    <= 2 max(d_pre, d_rows), both measured in this run (the rule and the factor of test_verify_step_reproduces_sequential_decode_steps)."""
    cfg, m, ids, images = _tiny(dtype)
    eng = m.engine
    V, P = cfg.vocab_size, ids.shape[1]
    toks, nxt = _toks(V), _toks(V, 1, seed=12)
    a, a_next, d_pre, d_rows = _measured(dtype, kv8)
    _, cb = eng.prefill(ids, None, images, S_EXT + 2, kv_fp8=kv8)
    lb = eng.extend(cb, toks[None, :]).clone()
    assert lb.shape[0] == 1 and int(cb.lens[0]) == P + S_EXT
    lb_next = eng.decode_step(nxt, cb).clone()
    _, cc = eng.prefill(ids, None, images, S_EXT + 2, kv_fp8=kv8)
    eng.extend(cc, toks[None, :25], pos=P)
    assert int(cc.lens[0]) == P + 25
    cc.truncate(P + 10)
    assert int(cc.lens[0]) == P + 10
    lc = eng.extend(cc, toks[None, 10:]).clone()
    lc_next = eng.decode_step(nxt, cc).clone()
    _, cd = eng.prefill(ids, None, images, 0, kv_fp8=kv8)  # no room at all: the extend needs a grown cache
    with pytest.raises(ValueError, match="grow_cache"):
        eng.extend(cd, toks[None, :])
    cd = eng.grow_cache(cd, 256)
    assert cd.Smax == 256 and int(cd.lens[0]) == P
    ld = eng.extend(cd, toks[None, :]).clone()
    with pytest.raises(ValueError):
        eng.extend(eng.prefill(ids.repeat(2, 1), None, images * 2, 4, kv_fp8=kv8)[1], toks[None, :2])
    devs = dict(b=_dev([lb], a[-1:], V), b_next=_dev([lb_next], [a_next], V), c=_dev([lc], a[-1:], V), c_next=_dev([lc_next], [a_next], V),
                d=_dev([ld], a[-1:], V))
    bound = 2 * max(d_pre, d_rows)
    print(f"SESSION | extend | {'fp8' if kv8 else '16-bit'} cache | {str(dtype)[6:]} | d_pre = {d_pre:.3e} | d_rows = {d_rows:.3e} | "
          + " | ".join(f"dev({k}, a) = {v:.3e}" for k, v in devs.items()) + f" | bound = {bound:.3e}")
    assert max(devs.values()) <= bound, (devs, bound)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_extend_with_an_image_in_the_tail(dtype):
    """tiny_2img (text, image, text, image, text), 16-bit cache: (i) prefill of the 4 text tokens in front of the first image, extend of the
    rest with both images; (ii) prefill up to the second image with the first, extend of the rest with the second.  Last-position logits
    against the prefill of the whole prompt, under the bound of test_extend_reproduces_sequential_decode_steps (the tiny fixture's, the
    same decoder weights).  Through a session, the second call's images_encoded counts the tail's image only."""
    from test_generation_gpu import _model

    cfg, batch, m = _model("tiny_2img", GAIN, dtype)
    eng = m.engine
    V = cfg.vocab_size
    ids = batch["input_ids"][:, :48].cuda()
    imgs = batch["images"][0].cuda()
    row = ids[0].tolist()
    s1, s2 = row.index(m.im_start_token), len(row) - 1 - row[::-1].index(m.im_start_token)
    assert (s1, s2) == (4, 27) and imgs.shape[0] == 2
    whole, _ = eng.prefill(ids, None, [imgs], 2)
    whole = whole.clone()
    _, c1 = eng.prefill(ids[:, :s1], None, None, 48)
    l1 = eng.extend(c1, ids[:, s1:], [imgs]).clone()
    _, c2 = eng.prefill(ids[:, :s2], None, [imgs[:1]], 48)
    l2 = eng.extend(c2, ids[:, s2:], [imgs[1:]], pos=s2).clone()
    assert int(c1.lens[0]) == int(c2.lens[0]) == 48
    _, _, d_pre, d_rows = _measured(dtype, False)
    bound = 2 * max(d_pre, d_rows)
    d1, d2 = _dev([l1], [whole], V), _dev([l2], [whole], V)
    print(f"SESSION | image in the tail | {str(dtype)[6:]} | dev(i) = {d1:.3e} | dev(ii) = {d2:.3e} | bound = {bound:.3e}")
    assert max(d1, d2) <= bound, (d1, d2, bound)
    s = m.new_session()
    m.generate(ids[:, :s2], images=[imgs[:1]], max_new_tokens=1, eos_token_id=-1, pad_token_id=0, session=s)
    assert s.last == dict(reused_tokens=0, run_tokens=s2, images_encoded=1) and len(s.tokens) == s2
    m.generate(ids, images=[imgs], max_new_tokens=1, eos_token_id=-1, pad_token_id=0, session=s)
    assert s.last == dict(reused_tokens=s2, run_tokens=48 - s2, images_encoded=1), s.last
    assert m.engine.last_generate_stats["images_encoded"] == 1 and m.engine.last_generate_stats["reused_tokens"] == s2


# ---- generate(session=...) -----------------------------------------------------------------------------------------------------------------
def _holds(s, out, n=None):
    """The session holds out[0, :n] (default: all but the last emitted token), on the host and on the device."""
    n = out.shape[1] - 1 if n is None else n
    assert int(s.cache.lens[0]) == len(s.tokens) == n and s.tokens == out[0, :n].tolist(), (int(s.cache.lens[0]), len(s.tokens), n)


MORE = [17, 23, 9, 41, 5, 30]  # six more tokens of a second turn


@pytest.mark.parametrize("i", range(5))
def test_session_greedy_first_and_second_call(i):
    """(a) a first call through a fresh session gives the reference's tokens or a tie; (b) a second call whose prompt is the first output
    plus six tokens gives a plain generate()'s tokens or a tie, reusing exactly what the cache held; (e) the identical prompt again runs
    one token and gives the same output."""
    from test_generation_gpu import _same_or_tie

    rec, cfg, m, ids, images = _gold_model(i)
    kw = dict(images=images, max_new_tokens=rec["max_new_tokens"], do_sample=False, eos_token_id=rec["eos_token_id"], pad_token_id=0)
    s = m.new_session()
    out1 = m.generate(ids, session=s, **kw)
    _same_or_tie(m, images, out1.cpu(), torch.tensor(rec["greedy"]), rec["prompt_len"], "first call")
    assert s.last == dict(reused_tokens=0, run_tokens=ids.shape[1], images_encoded=sum(im.shape[0] for im in images))
    _holds(s, out1)
    held = len(s.tokens)
    ids2 = torch.cat([out1, torch.tensor([MORE], device=out1.device)], dim=1)
    kw2 = dict(kw, max_new_tokens=8, eos_token_id=-1)
    want2 = m.generate(ids2, **kw2)
    got2 = m.generate(ids2, session=s, **kw2)
    assert s.last == dict(reused_tokens=held, run_tokens=ids2.shape[1] - held, images_encoded=0), s.last
    st = m.engine.last_generate_stats
    assert st["reused_tokens"] == held and st["run_tokens"] == ids2.shape[1] - held and st["plain_steps"] == got2.shape[1] - ids2.shape[1] - 1
    _same_or_greedy_tie(m, ids2, None, images, got2, want2)
    _holds(s, got2)
    again = m.generate(ids2, session=s, **kw2)
    assert s.last == dict(reused_tokens=ids2.shape[1] - 1, run_tokens=1, images_encoded=0), s.last
    _same_or_greedy_tie(m, ids2, None, images, again, got2)
    _holds(s, again)
    s.reset()
    assert s.tokens == [] and int(s.cache.lens[0]) == 0
    m.generate(ids2, session=s, **kw2)
    assert s.last["reused_tokens"] == 0 and s.last["run_tokens"] == ids2.shape[1]


def test_session_divergence_in_text_and_in_the_image():
    """(c) a text prompt diverging at token 10 reuses exactly 10 tokens; (d) the same ids with a changed image reuse only the tokens in
    front of the image span (and encode the image again); both give the plain path's tokens or a tie."""
    rec, cfg, m, ids, images = _gold_model(4)
    kw = dict(max_new_tokens=6, eos_token_id=-1, pad_token_id=0)
    text = torch.randint(3, 90, (1, 24), generator=torch.Generator().manual_seed(5)).cuda()
    s = m.new_session()
    m.generate(text, session=s, **kw)
    text2 = text.clone()
    text2[0, 10:] = (text2[0, 10:] + 1 - 3) % 87 + 3
    assert bool((text2[0, 10:] != text[0, 10:]).all())
    got = m.generate(text2, session=s, **kw)
    assert s.last == dict(reused_tokens=10, run_tokens=14, images_encoded=0), s.last
    _same_or_greedy_tie(m, text2, None, None, got, m.generate(text2, **kw))
    _holds(s, got)
    # (d)
    s = m.new_session()
    m.generate(ids, images=images, session=s, **kw)
    other = [im.clone() for im in images]
    other[0][0, 1, 2, 3] += 0.5
    start = ids[0].tolist().index(m.im_start_token)
    assert start >= 1
    got = m.generate(ids, images=other, session=s, **kw)
    assert s.last == dict(reused_tokens=start, run_tokens=ids.shape[1] - start, images_encoded=1), s.last
    _same_or_greedy_tie(m, ids, None, other, got, m.generate(ids, images=other, **kw))
    same = m.generate(ids, images=[im.clone() for im in other], session=s, **kw)
    assert s.last == dict(reused_tokens=ids.shape[1] - 1, run_tokens=1, images_encoded=0), s.last
    _same_or_greedy_tie(m, ids, None, other, same, got)


def _second_turn(m, ids, images, s, **first_kw):
    """A first greedy call through the session, then the second turn's prompt: its output plus six tokens."""
    out1 = m.generate(ids, images=images, max_new_tokens=8, eos_token_id=-1, pad_token_id=0, session=s, **first_kw)
    return torch.cat([out1, torch.tensor([MORE], device=out1.device)], dim=1), len(s.tokens)


@pytest.mark.parametrize("flags", [dict(fp8_weights=True), dict(fp4_weights=True)], ids=lambda f: next(iter(f)))
def test_session_with_decode_weight_formats(flags):
    """(f) fp8 / fp4 decode weights: the second call equals the plain path under the same flags or a tie (the extend runs the 16-bit weights,
    like the plain path's prefill)."""
    rec, cfg, m, ids, images = _gold_model(4)
    s = m.new_session()
    ids2, held = _second_turn(m, ids, images, s)
    kw = dict(images=images, max_new_tokens=10, eos_token_id=-1, pad_token_id=0, **flags)
    got = m.generate(ids2, session=s, **kw)
    assert s.last["reused_tokens"] == held and s.last["run_tokens"] == ids2.shape[1] - held
    w = dict(fp8=bool(flags.get("fp8_weights")), fp4=bool(flags.get("fp4_weights")))
    _same_or_greedy_tie(m, ids2, None, images, got, m.generate(ids2, **kw), **w)
    _holds(s, got)


def test_session_seeded_sampling_with_prompt_lookup():
    """(f) do_sample with prompt_lookup_num_tokens=4 on the second call: the plain path's tokens under the same flags, or a divergence at a
    step where mh_select_tokens' uniform lies within 2e-3 of the inverse-CDF boundary between the two tokens (the rule of
    test_seeded_sampling_lookup_equals_plain_or_a_cdf_tie).  The session then holds out[:cache.lens], never the last emitted token."""
    import numpy as np

    from merlin_amd import ops
    from oracle import gen_ref as R

    rec, cfg, m, ids, images = _gold_model(4)
    V = cfg.vocab_size
    s = m.new_session()
    ids2, held = _second_turn(m, ids, images, s)
    P = ids2.shape[1]
    kw = dict(images=images, max_new_tokens=24, eos_token_id=-1, pad_token_id=0, do_sample=True, temperature=0.8, seed=4242, prompt_lookup_num_tokens=4)
    plain = m.generate(ids2, **kw).cpu()
    got = m.generate(ids2, session=s, **kw).cpu()
    assert s.last["reused_tokens"] == held and got.shape == plain.shape
    n = int(s.cache.lens[0])
    assert P <= n == len(s.tokens) <= got.shape[1] - 1 and s.tokens == got[0, :n].tolist()
    if got.tolist() != plain.tolist():
        t = int((got[0] != plain[0]).nonzero()[0])
        assert t >= P
        lg = _step_logits(m, ids2, None, images, plain[0, P:t].tolist())
        _, u = ops.select_tokens(lg[None].contiguous(), V, do_sample=True, temperature=0.8, top_k=50, top_p=1.0, seed=4242, step=t - P, return_u=True)
        u = float(u[0])
        cdf = np.cumsum(R.warp_probs(lg.cpu().numpy(), 0.8, 50, 1.0))
        for tok in (int(got[0, t]), int(plain[0, t])):
            lo, hi = (cdf[tok - 1] if tok else 0.0), cdf[tok]
            assert lo - 2e-3 <= u <= hi + 2e-3, ("diverged at", t, "away from a CDF boundary", tok, u, lo, hi, got.tolist(), plain.tolist())


@pytest.mark.parametrize("share", [False, True], ids=["copy", "share_prompt_kv"])
def test_session_beam_search(share):
    """(f) num_beams=3 on the second call, both cache paths: the plain path's hypothesis, or one whose length-normalised score under
    forward() lies within 2e-3 (relative) of it - a tie of the beam scores; the session's cache is read, not written: it holds the prompt."""
    rec, cfg, m, ids, images = _gold_model(4)
    s = m.new_session()
    ids2, held = _second_turn(m, ids, images, s)
    P = ids2.shape[1]
    kw = dict(images=images, max_new_tokens=8, num_beams=3, eos_token_id=-1, pad_token_id=0, share_prompt_kv=share)
    rows0 = [t[:, :P - 1].clone() for t in s.cache.k]
    want = m.generate(ids2, **kw)
    got = m.generate(ids2, session=s, **kw)
    assert s.last == dict(reused_tokens=held, run_tokens=P - held, images_encoded=0), s.last
    _holds(s, ids2, P)
    assert all(torch.equal(t[:, :held], r[:, :held]) for t, r in zip(s.cache.k, rows0))
    if got.tolist() != want.tolist():
        def score(seq):
            with torch.no_grad():
                lp = torch.log_softmax(m(input_ids=seq, images=images).logits[0, P - 1:-1, :cfg.vocab_size].float(), -1)
            return float(lp.gather(1, seq[0, P:, None]).sum()) / (seq.shape[1] - P)
        a, b = score(got), score(want)
        assert abs(a - b) <= 2e-3 * abs(b), ("beam outputs differ without a tie of their scores", a, b, got.tolist(), want.tolist())
    again = m.generate(ids2, session=s, **kw)  # the prompt is still there: one token runs
    assert s.last == dict(reused_tokens=P - 1, run_tokens=1, images_encoded=0) and again.shape[1] > P


def test_session_fp8_cache():
    """(g) fp8_kv=True: the second call reads its cached prefix quantised (the plain path's prefill reads it unquantised), so it is held to
    greedy decoding by teacher-forced decode_steps on an fp8 cache (test_spec_gpu._step_logits with kv8=True) by the tie rule, and must
    reproduce itself across two runs."""
    rec, cfg, m, ids, images = _gold_model(4)
    P0, V = ids.shape[1], cfg.vocab_size
    runs = []
    for _ in range(2):
        s = m.new_session(fp8_kv=True)
        ids2, held = _second_turn(m, ids, images, s, fp8_kv=True)
        got = m.generate(ids2, images=images, max_new_tokens=8, eos_token_id=-1, pad_token_id=0, fp8_kv=True, session=s)
        assert s.cache.fp8 and s.last["reused_tokens"] == held
        _holds(s, got)
        runs.append((ids2, got))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    ids2, got = runs[0]
    new = ids2[0, P0:].tolist()
    for _ in range(8):  # the reference continuation: every token of the second turn and every new one through decode_step
        new.append(int(_step_logits(m, ids, None, images, new, kv8=True)[:V].argmax()))
    want = torch.cat([ids, torch.tensor([new], device=ids.device)], dim=1)
    _same_or_greedy_tie(m, ids, None, images, got, want, True)


def test_session_grows_its_cache():
    """(h) capacity 64, then a call whose prompt + max_new_tokens exceeds it: the cache grows to a multiple of 256 with its rows (16-bit and
    fp8 form) and the call gives the tokens of a session created large enough."""
    rec, cfg, m, ids, images = _gold_model(4)
    for fp8 in (False, True):
        outs = []
        for cap in (64, 256):
            s = m.new_session(capacity=cap, fp8_kv=fp8)
            m.generate(ids, images=images, max_new_tokens=1, eos_token_id=-1, pad_token_id=0, session=s, fp8_kv=fp8)
            assert s.cache.Smax == cap and len(s.tokens) == ids.shape[1]
            ids2 = torch.cat([ids, torch.tensor([MORE], device=ids.device)], dim=1)
            outs.append(m.generate(ids2, images=images, max_new_tokens=40, eos_token_id=-1, pad_token_id=0, session=s, fp8_kv=fp8))
            assert s.cache.Smax == 256 and s.capacity == 256 and s.last["reused_tokens"] == ids.shape[1]
            _holds(s, outs[-1])
        assert torch.equal(outs[0], outs[1]), (fp8, outs[0].tolist(), outs[1].tolist())
