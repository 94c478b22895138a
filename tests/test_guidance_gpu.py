"""Classifier-free guidance on the GPU: mh_guidance_mix against transformers' formula in float64 (per-element bound from the kernel's fp32
roundings, torch's own fp32 evaluation as the yardstick), its footprint, argument checks and graph capture; engine.pair_cache; and
generate(guidance_scale=...) on the tiny model, teacher-forced against the model's own forwards on the conditional and the unconditional
sequence, with bans, sampling, prompt lookup and the default negative prompt; the launch symbols of calls without guidance."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from test_bans_cpu import hf_apply, hf_processors  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24    # unit roundoff of fp32
SENT = 7.25       # what the pad columns of an output buffer hold before (and after) a launch
PAD_IN = 1.0e30   # what the pad columns of the inputs hold: read as a logit it would be the row's maximum
SCALES = (0.5, 1.5, 3.0)


@pytest.fixture(scope="module")
def O():
    from merlin_amd import ops

    assert ops.arch_ok(0), "not a gfx950 device"
    return ops


def _ref64(c, u, g):
    """transformers' formula (UnbatchedClassifierFreeGuidanceLogitsProcessor.__call__) in float64 on fp32 inputs -> (scores, lc, lu)."""
    lc, lu = torch.log_softmax(c.double(), -1), torch.log_softmax(u.double(), -1)
    return g * (lc - lu) + lu, lc, lu


def _bound(lc, lu, g, V):
    """Per-element bound on |kernel - float64| from the fp32 roundings the kernel performs (csrc/sampling.hip guidance_mix_k), u = 2^-24.
    A log-probability is l = fl(fl(x - max) - fl(log S^)): the first subtraction moves it by u |x - max| <= u |l|, logf by one ulp of
    log S (<= 2 u |l|, as 0 <= log S <= |l|), the second subtraction by u |l|: 4 u |l|, plus the error of S^ itself, which enters log S
    absolutely.  S^ is a chain of L = ceil(V / 256) accumulations per thread and 8 more across the block; every link carries up to four
    roundings (the exponential, its argument, the add, a rescale of the running sum when the maximum moves), independent in sign, so they
    add up like sqrt (the rule of tests/numerics.py `gemm`), and the arguments' roundings weigh in with sum p |x - max| <= log V:
    K = 4 (sqrt(L) + 8) + log V units of u.  The mix g (lc - lu) + lu then amplifies the two rows' errors by |g| and |1 - g|, rounds
    lc - lu (u (|lc| + |lu|), times |g|) and rounds the result (u |out| <= u (|g| |lc| + |1 - g| |lu|)).  Collected, with every |l| term
    bounded by |lc| + |lu|:   bound_i = u (|g| + |1 - g|) (6 (|lc_i| + |lu_i|) + K)."""
    K = 4 * (math.sqrt(math.ceil(V / 256)) + 8) + math.log(V)
    return U * (abs(g) + abs(1 - g)) * (6 * (lc.abs() + lu.abs()) + K)


def _pairs(V, R, scaled, seed):
    """R pairs of N(0, 3) rows; scaled: pair R // 2 multiplied by 20 (N(0, 60): exp of it overflows fp32 unless the maximum is subtracted)."""
    gen = torch.Generator().manual_seed(seed)
    c, u = torch.randn(R, V, generator=gen) * 3, torch.randn(R, V, generator=gen) * 3
    if scaled:
        c[R // 2] *= 20
        u[R // 2] *= 20
    return c, u


_REF = {}


def _case(V, R, scaled, g):
    """Inputs, float64 reference, bound and torch's own fp32 error for one case - computed once, shared by the layouts, never written."""
    key = (V, R, scaled, g)
    if key not in _REF:
        from merlin_amd.generation import _guided_ref

        c, u = _pairs(V, R, scaled, 1000 * R + V % 997 + int(scaled))
        ref, lc, lu = _ref64(c, u, g)
        err_torch = float((_guided_ref(c, u, g).double() - ref).abs().max())  # torch's fp32 evaluation of the formula on the CPU
        _REF[key] = (c, u, ref, _bound(lc, lu, g, V), err_torch)
    return _REF[key]


def _launch(O, c, u, g, V, ld, one_buffer, in_place):
    """Run the kernel on copies of c, u [R, V] laid out with row stride ld (pad columns PAD_IN), as rows [1, 1 + R) and [1 + R, 1 + 2R) of
    one buffer or as two tensors, guard rows around them; -> (out [R, ld] on the host, the uncond rows before and after, everything else
    that must not have changed)."""
    R = c.shape[0]
    if one_buffer:
        buf = torch.full((2 * R + 2, ld), PAD_IN, dtype=torch.float32)
        buf[1:1 + R, :V], buf[1 + R:1 + 2 * R, :V] = c, u
        buf = buf.cuda()
        cd, ud = buf[1:1 + R], buf[1 + R:1 + 2 * R]
        guards = lambda: [buf[0].cpu(), buf[-1].cpu()]  # noqa: E731
    else:
        bc, bu = (torch.full((R + 2, ld), PAD_IN, dtype=torch.float32) for _ in range(2))
        bc[1:1 + R, :V], bu[1:1 + R, :V] = c, u
        bc, bu = bc.cuda(), bu.cuda()
        cd, ud = bc[1:1 + R], bu[1:1 + R]
        guards = lambda: [bc[0].cpu(), bc[-1].cpu(), bu[0].cpu(), bu[-1].cpu()]  # noqa: E731
    before = [t.clone() for t in guards()] + [ud.cpu().clone()]
    if in_place:
        out = O.guidance_mix(cd, ud, g, V, out=cd)
        assert out.data_ptr() == cd.data_ptr()
        pad = PAD_IN
    else:
        ob = torch.full((R + 2, ld), SENT, dtype=torch.float32, device="cuda")
        out = O.guidance_mix(cd, ud, g, V, out=ob[1:1 + R])
        assert bool((ob[0] == SENT).all()) and bool((ob[-1] == SENT).all()), "a row outside the launch was written"
        assert torch.equal(cd.cpu()[:, :V], c), "the cond rows changed in an out-of-place launch"
        pad = SENT
    torch.cuda.synchronize()
    after = guards() + [ud.cpu()]
    for a, b in zip(before, after):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the uncond rows or a guard row changed"
    got = out.cpu()
    assert bool((got[:, V:] == pad).all()), "columns >= V were written"
    return got[:, :V]


@pytest.mark.parametrize("V,ld", [(40, 40), (1000, 1008), (32003, 32064)])
@pytest.mark.parametrize("R", [1, 3])
def test_guidance_mix_vs_float64_within_the_bound_and_4x_torch(O, V, ld, R):
    """Every layout (rows of one buffer / two tensors, in place / third buffer), g in {0.5, 1.5, 3}, N(0, 3) rows without and with one
    pair scaled to N(0, 60): per element within the derived bound, and the maximum error at most 4 x the error of torch's fp32 evaluation
    of the same formula (the margin: the reduction order and the fused multiply-add of the last step differ from torch's)."""
    for scaled in (False, True):
        for g in SCALES:
            c, u, ref, bound, err_torch = _case(V, R, scaled, g)
            for one_buffer in (True, False):
                for in_place in (True, False):
                    got = _launch(O, c, u, g, V, ld, one_buffer, in_place)
                    assert bool(torch.isfinite(got).all())
                    err = (got.double() - ref).abs()
                    worst = float((err / bound).max())
                    print(f"GUIDANCE | V {V} R {R} scaled {int(scaled)} g {g} one_buffer {int(one_buffer)} in_place {int(in_place)} | "
                          f"kernel max err {float(err.max()):.3e} | torch fp32 max err {err_torch:.3e} | worst err / bound {worst:.3f}")
                    assert worst <= 1.0, (V, R, scaled, g, one_buffer, in_place, worst)
                    assert float(err.max()) <= 4 * err_torch, (V, R, scaled, g, one_buffer, in_place, float(err.max()), err_torch)


@pytest.mark.parametrize("V,ld", [(40, 40), (1000, 1008), (32003, 32064)])
def test_guidance_mix_of_a_row_with_itself_is_its_log_softmax(O, V, ld):
    c, _ = _pairs(V, 3, True, 5)
    want = torch.log_softmax(c.double(), -1)
    for g in SCALES:
        got = _launch(O, c, c.clone(), g, V, ld, False, False)
        assert float(((got.double() - want).abs() / _bound(want, want, g, V)).max()) <= 1.0, g


def test_guidance_mix_refuses_bad_arguments_and_writes_nothing(O):
    from merlin_amd import _lib as L

    V = 40
    c, u = (t.cuda() for t in _pairs(V, 2, False, 9))
    out = torch.full((2, V), SENT, device="cuda")
    bad = [(c, V, u, V, 2, 0, out, V),       # V < 1
           (c, V, u, V, -1, V, out, V),      # R < 0
           (None, V, u, V, 2, V, out, V), (c, V, None, V, 2, V, out, V), (c, V, u, V, 2, V, None, V),  # null pointers
           (c, V - 1, u, V, 2, V, out, V), (c, V, u, V - 1, 2, V, out, V), (c, V, u, V, 2, V, out, V - 1)]  # a leading dimension < V
    for cd, ldc, ud, ldu, R, v, o, ldo in bad:
        with pytest.raises(L.MerlinHipError, match="bad argument"):
            L.call("mh_guidance_mix", cd, ldc, ud, ldu, R, v, 1.5, o, ldo, None)
    with pytest.raises(AssertionError):
        O.guidance_mix(c, u, 1.5, V + 1)                       # the wrapper's own checks: more columns than the rows have
    with pytest.raises(AssertionError):
        O.guidance_mix(c, u.double(), 1.5, V)
    with pytest.raises(AssertionError):
        O.guidance_mix(c, u[:1], 1.5, V)
    L.call("mh_guidance_mix", c, V, u, V, 0, V, 1.5, out, V, None)  # no pairs: nothing to do, no error
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


def test_guidance_mix_is_capturable(O):
    """No allocation, no read-back: the launch (the decode step's layout: rows 0 and 1 of one buffer, in place) records into a HIP graph
    and replays on changed inputs."""
    V, ld = 1000, 1008
    x = torch.zeros(2, ld, device="cuda")
    O.guidance_mix(x[:1].clone(), x[1:], 1.5, V)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        O.guidance_mix(x[:1], x[1:], 1.5, V, out=x[:1])
    for seed in (1, 2):
        c, u = _pairs(V, 1, seed == 2, seed)
        x[0, :V], x[1, :V] = c[0].cuda(), u[0].cuda()
        gr.replay()
        ref, lc, lu = _ref64(c, u, 1.5)
        assert float(((x[:1, :V].cpu().double() - ref).abs() / _bound(lc, lu, 1.5, V)).max()) <= 1.0
        assert torch.equal(x[1, :V].cpu(), u[0]) and bool((x[:, V:] == 0).all())


# ---- generate() on the tiny model ----------------------------------------------------------------------------------------------------------
G_SCALE = 3.0
P0 = 22
_FP4 = {}


def _fixture():
    """tests/test_bans_gpu.py's tiny model (tiny_1img, V = 103, peaked logits), its 22-token prompt with one image, and the negative prompt:
    the same text without the image span."""
    from merlin_amd.generation import _image_spans
    from test_bans_gpu import _fixture as base

    m, cfg, ids, images, plain = base()
    row = ids[0].tolist()
    (s, e), = _image_spans(row, m.im_start_token, m.im_end_token)
    neg = torch.tensor([row[:s] + row[e:]], dtype=torch.int64, device="cuda")
    assert 1 <= neg.shape[1] < P0
    return m, cfg, ids, images, plain, neg


def _fp4_model():
    """A second tiny model whose decoder weights lie on the MXFP4 grid (tests/test_fp4_gpu.py::_snap): its fp4 copies ARE its weights, so
    its own 16-bit forward is the teacher of its fp4 decode steps."""
    if "m" not in _FP4:
        from test_bans_gpu import GAIN
        from test_fp4_gpu import _snap
        from test_generation_gpu import _model

        _FP4["m"] = _model("tiny_1img", GAIN)[2]
        _snap(_FP4["m"])
    return _FP4["m"]


def _last_logits(m, V, seq, images):
    with torch.no_grad():
        return m(input_ids=torch.tensor([seq], dtype=torch.int64, device="cuda"), images=images).logits[0, -1, :V].float().cpu()


def _teacher_forced(m, V, out, images, negative, neg_images, g, tag, procs=None, eos=()):
    """For EVERY generated position t: the model's own full forward on the conditional sequence out[:t] and on the unconditional one
    (negative prompt, or the prompt's last token, + the generated tokens), transformers' formula in float64 on those two rows (then the
    processors `procs`, which only write -inf), and: the emitted token lies within (|g| + |1 - g|) * 2e-3 * max|logit| of the guided
    maximum - tests/test_generation_gpu.py::_same_or_tie's 2e-3 of the largest logit magnitude (of the two rows that enter the mix),
    scaled by the mix's amplification of an input error.  -> (positions whose guided argmax differs from the conditional argmax,
    positions whose guided argmax is banned)."""
    from merlin_amd.generation import _uncond_context

    seq = out[0].tolist()
    neg = None if negative is None else negative[0].tolist()
    bites = banned = 0
    for t in range(P0, len(seq)):
        lc = _last_logits(m, V, seq[:t], images)
        lu = _last_logits(m, V, _uncond_context(neg, seq[:P0], seq[P0:t]), neg_images)
        s = _ref64(lc, lu, g)[0]
        raw_arg = int(s.argmax())
        if procs:
            s = hf_apply(procs, seq[:t], s.float()).double()
        tok = seq[t]
        assert torch.isfinite(s[tok]), (tag, "emitted a banned token", t, tok)
        gap = float(s.max() - s[tok])
        tol = (abs(g) + abs(1 - g)) * 2e-3 * max(float(lc.abs().max()), float(lu.abs().max()))
        print(f"GUIDANCE | {tag} | t {t} | tok {tok} | gap {gap:.3e} | tol {tol:.3e} | cond argmax {int(lc.argmax())} | guided argmax {raw_arg}")
        assert gap < tol, (tag, "not the guided maximum", t, tok, gap, tol)
        bites += int(raw_arg != int(lc.argmax()))
        banned += int(not math.isfinite(float(s[raw_arg])))
        if tok in eos:
            assert t == len(seq) - 1
    return bites, banned


def _plain_guided_scores(m, V, ids, images, neg, new):
    """The plain guided path's scores that choose new token number len(new): two prefills, the paired cache, teacher-forced B = 2 decode
    steps, one mix.  -> (scores fp32 [V] on the host, the largest magnitude of the two rows of logits that entered the mix)."""
    from merlin_amd import ops

    eng = m.engine
    lc, cc = eng.prefill(ids, None, images, 0)
    lu, cu = eng.prefill(neg, None, None, 0)
    lg, cache = torch.cat([lc, lu]), eng.pair_cache(cc, cu, len(new) + 2)
    for tok in new:
        lg = eng.decode_step(torch.tensor([tok, tok], device="cuda"), cache)
    return ops.guidance_mix(lg[:1], lg[1:], G_SCALE, V)[0].cpu(), float(lg[:, :V].abs().max())


MODES = dict(graph=dict(), no_graph=dict(use_graph=False), no_cache=dict(use_cache=False), fp8_kv=dict(fp8_kv=True), fp4_weights=dict(fp4_weights=True))


@pytest.mark.parametrize("mode", list(MODES))
def test_guided_greedy_teacher_forced_and_guidance_bites(mode):
    m, cfg, ids, images, plain, neg = _fixture()
    if mode == "fp4_weights":
        m = _fp4_model()
    out = m.generate(ids, images=images, max_new_tokens=12, eos_token_id=-1, pad_token_id=0, guidance_scale=G_SCALE, negative_prompt_ids=neg,
                     **MODES[mode]).cpu()
    assert out.shape == (1, P0 + 12) and torch.equal(out[:, :P0], ids.cpu())
    assert m.engine.last_generate_stats["guided_steps"] == 12
    bites, _ = _teacher_forced(m, cfg.vocab_size, out, images, neg, None, G_SCALE, mode)
    assert bites >= 1, "the guided argmax never differs from the conditional one: the test would pass with the mix skipped"


def test_guided_greedy_with_a_negative_image():
    """negative_images: the negative prompt is the whole prompt with ANOTHER image in its span."""
    m, cfg, ids, images, plain, neg = _fixture()
    other = [torch.flip(images[0], dims=(-1,)) * 0.5]
    out = m.generate(ids, images=images, max_new_tokens=12, eos_token_id=-1, pad_token_id=0, guidance_scale=G_SCALE, negative_prompt_ids=ids.clone(),
                     negative_prompt_attention_mask=torch.ones_like(ids), negative_images=other).cpu()
    _teacher_forced(m, cfg.vocab_size, out, images, ids, other, G_SCALE, "negative image")


def test_guided_greedy_with_the_default_negative_prompt():
    m, cfg, ids, images, plain, neg = _fixture()
    out = m.generate(ids, images=images, max_new_tokens=12, eos_token_id=-1, pad_token_id=0, guidance_scale=1.5).cpu()
    assert out.shape == (1, P0 + 12)
    _teacher_forced(m, cfg.vocab_size, out, images, None, None, 1.5, "default negative prompt")


@pytest.mark.parametrize("mode", ["graph", "no_cache", "lookup"])
def test_guided_greedy_with_bans(mode):
    """The options of tests/test_bans_gpu.py::_options behind the mix: no emitted token is banned, and the teacher-forced check holds on the
    guided, banned scores."""
    from test_bans_gpu import _options

    m, cfg, ids, images, plain, neg = _fixture()
    eos, opts, kw = _options(plain)
    extra = dict(graph=dict(), no_cache=dict(use_cache=False), lookup=dict(prompt_lookup_num_tokens=4))[mode]
    out = m.generate(ids, images=images, max_new_tokens=12, guidance_scale=G_SCALE, negative_prompt_ids=neg, **kw, **extra).cpu()
    assert out.shape[1] > P0 + 6  # min_new_tokens
    _teacher_forced(m, cfg.vocab_size, out, images, neg, None, G_SCALE, "bans " + mode, procs=hf_processors(P0, eos, **opts), eos=eos)


def test_guided_streamer_and_criteria_see_the_conditional_ids_only():
    m, cfg, ids, images, plain, neg = _fixture()
    seen, lens = [], []

    class Streamer:
        def put(self, x):
            seen.append(x.reshape(-1).tolist())

        def end(self):
            seen.append("end")

    def criterion(cur, scores):
        lens.append(tuple(cur.shape))
        assert torch.equal(cur[:, :P0].cpu(), ids.cpu())
        return cur.shape[1] >= P0 + 5

    out = m.generate(ids, images=images, max_new_tokens=12, eos_token_id=-1, pad_token_id=0, guidance_scale=G_SCALE, negative_prompt_ids=neg,
                     streamer=Streamer(), stopping_criteria=[criterion]).cpu()
    assert out.shape == (1, P0 + 5) and lens == [(1, P0 + i) for i in range(1, 6)]
    assert seen[0] == ids[0].tolist() and seen[-1] == "end" and [t for s in seen[1:-1] for t in s] == out[0, P0:].tolist()


def test_guided_sampling_is_replayable_and_prompt_lookup_gives_the_plain_guided_tokens():
    """Fixed seed twice: the same tokens.  prompt_lookup_num_tokens=4: the plain guided path's tokens, greedy and sampling (the invariant
    tests/test_spec_gpu.py holds for the unguided path: equal, or first different at a step where both tokens lie within the teacher-forced
    tolerance of the plain guided path's own scores); verify steps ran, accepted <= drafted."""
    m, cfg, ids, images, plain, neg = _fixture()
    V = cfg.vocab_size
    base = dict(images=images, max_new_tokens=24, eos_token_id=-1, pad_token_id=0, guidance_scale=G_SCALE, negative_prompt_ids=neg)
    for tag, skw in (("greedy", dict()), ("sampling", dict(do_sample=True, temperature=0.9, top_k=20, min_p=0.02, epsilon_cutoff=1e-3, seed=77))):
        want = m.generate(ids, **base, **skw).cpu()
        again = m.generate(ids, **base, **skw).cpu()
        assert torch.equal(want, again), tag
        assert m.engine.last_generate_stats["verify_steps"] == 0 and m.engine.last_generate_stats["guided_steps"] == 24
        for use_graph in (True, False):
            got = m.generate(ids, prompt_lookup_num_tokens=4, use_graph=use_graph, **base, **skw).cpu()
            st = dict(m.engine.last_generate_stats)
            assert st["verify_steps"] > 0 and st["accepted"] <= st["drafted"] and st["guided_steps"] == 1 + st["plain_steps"] + st["verify_steps"], st
            assert got.shape == want.shape
            if torch.equal(got, want):
                continue
            assert tag == "greedy", ("sampling diverged", got.tolist(), want.tolist())  # (a sampled tie has no argmax rule to fall back on)
            t = int((got[0] != want[0]).nonzero()[0])
            assert t >= P0
            s, mag = _plain_guided_scores(m, V, ids, images, neg, want[0, P0:t].tolist())
            tol = (abs(G_SCALE) + abs(1 - G_SCALE)) * 2e-3 * mag
            gaps = [float(s.max() - s[int(x[0, t])]) for x in (got, want)]
            assert max(gaps) < tol, ("diverged at", t, "without a tie", gaps, tol, got.tolist(), want.tolist())


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_pair_cache_rows_equal_their_sources_and_advance_together(fp8):
    m, cfg, ids, images, plain, neg = _fixture()
    eng = m.engine
    _, cc = eng.prefill(ids, None, images, 0, kv_fp8=fp8)
    _, cu = eng.prefill(neg, None, None, 3, kv_fp8=fp8)
    Pc, Pu = int(cc.lens[0]), int(cu.lens[0])
    assert (Pc, Pu) == (P0, neg.shape[1])
    pair = eng.pair_cache(cc, cu, 7)
    assert type(pair) is type(cc) and pair.B == 2 and pair.Smax == Pc + 7 and pair.fp8 == fp8 and pair.rpos is None
    assert pair.lens.tolist() == [Pc, Pu] and pair.lens.dtype == torch.int32
    for b, (src, n) in enumerate(((cc, Pc), (cu, Pu))):
        for li in range(len(src.k)):
            assert pair.k[li].dtype == src.k[li].dtype
            assert torch.equal(pair.k[li][b, :n], src.k[li][0, :n]) and torch.equal(pair.v[li][b, :n], src.v[li][0, :n])
            if fp8:
                assert torch.equal(pair.ks[li][b, :, :n], src.ks[li][0, :, :n]) and torch.equal(pair.vs[li][b, :, :n], src.vs[li][0, :, :n])
    for k in range(1, 4):
        eng.decode_step(torch.tensor([5, 5], device="cuda"), pair)
        assert pair.lens.tolist() == [Pc + k, Pu + k]
    assert cc.lens.tolist() == [Pc] and cu.lens.tolist() == [Pu]  # the sources are not written
    for bad in ((pair, cu), (cc, pair)):
        with pytest.raises(ValueError, match="pair_cache"):
            eng.pair_cache(*bad, 4)
    _, other = eng.prefill(neg, None, None, 0, kv_fp8=not fp8)
    with pytest.raises(ValueError, match="pair_cache"):
        eng.pair_cache(cc, other, 4)


def test_calls_without_guidance_launch_what_they_launched(monkeypatch):
    """The launch symbols at the library boundary: without guidance_scale, and with guidance_scale=1, every mode issues the same symbols
    in the same order and never mh_guidance_mix; with guidance every selected token is preceded by exactly one mix launch."""
    from merlin_amd import _lib as L

    m, cfg, ids, images, plain, neg = _fixture()
    names = []
    real = L.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(L, "call", recording)
    base = dict(images=images, max_new_tokens=6, eos_token_id=-1, pad_token_id=0)
    for extra in (dict(), dict(use_graph=False), dict(use_cache=False), dict(do_sample=True, temperature=0.8, seed=1), dict(prompt_lookup_num_tokens=4),
                  dict(no_repeat_ngram_size=2), dict(num_beams=3)):
        m.generate(ids, **base, **extra)  # (one-time work of a mode - tables, quantised copies - is not part of the comparison)
        runs = []
        for off in (dict(), dict(guidance_scale=1), dict(guidance_scale=1.0), dict(guidance_scale=None)):
            del names[:]
            m.generate(ids, **base, **extra, **off)
            runs.append(list(names))
        assert runs[0] and "mh_guidance_mix" not in runs[0] and all(r == runs[0] for r in runs[1:]), extra
    for extra, n_sel in ((dict(), 6), (dict(use_graph=False), 6), (dict(use_cache=False), 6)):
        del names[:]
        m.generate(ids, guidance_scale=2.0, negative_prompt_ids=neg, **base, **extra)
        assert names.count("mh_guidance_mix") == names.count("mh_select_tokens") == n_sel, extra
