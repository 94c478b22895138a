"""Assisted decoding on the GPU: the device-counter forms of the selection and ban launches against the scalar entry points (torch.equal,
and ONE captured graph that follows the counters), engine.capture_draft_graph against eager decode steps with scalar launches, and
generate(assistant_model=...) on the tiny multimodal fixture against its own plain path."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")


@pytest.fixture(scope="module")
def O():
    from merlin_amd import ops

    assert ops.arch_ok(0), "not a gfx950 device"
    return ops


# ---- kernels -----------------------------------------------------------------------------------------------------------------------------
def _logits(rows, V, ldl, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, ldl, generator=g) * 3.0
    x[:, V:] = 1e30  # (columns behind V are never read: a huge value there would win every selection)
    return x.cuda()


def _i64(v):
    return torch.tensor([v], dtype=torch.int64, device="cuda")


def _i32(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


SEL = [dict(), dict(do_sample=True, temperature=0.9, top_k=20, top_p=0.9, seed=77), dict(do_sample=True, temperature=1.3, top_k=0, top_p=1.0, seed=5, min_p=0.02, epsilon_cutoff=1e-4)]


@pytest.mark.parametrize("V,ldl", [(40, 40), (32003, 32064)])
@pytest.mark.parametrize("rows", [1, 5])
def test_select_tokens_dev_equals_the_scalar_entry_point(O, V, ldl, rows):
    """Same tokens and uniforms as select_tokens at step = counter + offset; the token also lands in ids[r, len + offset] and nowhere else
    in ids; a column outside the row writes nothing; greedy on a row of -inf gives 0 in both forms."""
    x = _logits(rows, V, ldl, seed=V + rows)
    x[rows - 1, 3:9] = NEG_INF
    cols = 12
    for sel in SEL:
        for base, off, length, len_off in ((0, 0, 0, 0), (7, 3, 4, 2), (2 ** 33, 5, 9, 2), (1, 0, 11, 0)):
            if sel.get("do_sample"):
                want, want_u = O.select_tokens(x, V, step=base + off, return_u=True, **sel)
            else:
                want, want_u = O.select_tokens(x, V, step=base + off, **sel), None
            ids = torch.full((rows + 1, cols), -7, dtype=torch.int64, device="cuda")
            out = torch.full((rows + 1,), -9, dtype=torch.int64, device="cuda")
            got = O.select_tokens_dev(x, V, _i64(base), off, out=out[:rows], ids=ids[:rows], len_base=_i32(length), len_off=len_off, return_u=bool(want_u is not None), **sel)
            got, got_u = got if want_u is not None else (got, None)
            assert torch.equal(got, want) and int(out[rows]) == -9, (sel, base, off)
            if want_u is not None:
                assert torch.equal(got_u, want_u)
            expect = torch.full_like(ids, -7)
            expect[:rows, length + len_off] = want
            assert torch.equal(ids, expect), (sel, length, len_off)
    # without ids: out alone; a cell outside the row: out alone
    assert torch.equal(O.select_tokens_dev(x, V, _i64(4), 1), O.select_tokens(x, V, step=5))
    ids = torch.full((rows, cols), -7, dtype=torch.int64, device="cuda")
    for length, len_off in ((cols, 0), (cols - 1, 1), (0, -1), (2 ** 31 - 1, 1)):
        assert torch.equal(O.select_tokens_dev(x, V, _i64(4), 1, ids=ids, len_base=_i32(length), len_off=len_off), O.select_tokens(x, V, step=5))
        assert bool((ids == -7).all())
    z = torch.full((rows, ldl), NEG_INF, device="cuda")
    assert O.select_tokens_dev(z, V, _i64(3), 0).tolist() == O.select_tokens(z, V, step=3).tolist() == [0] * rows


def _tables(V, P):
    """Every clause: 3-grams, a one-token and a two-token word, an always list, a begin list at length P, eos below P + 3."""
    t = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
    return dict(ngram=3, words=t([V - 1, 5, 6]), word_off=torch.tensor([0, 1, 3], dtype=torch.int32, device="cuda"), always=t([1, V + 4]), begin=t([2, 3]),
                begin_index=P, eos=t([4]), min_total=P + 3)


@pytest.mark.parametrize("V,ldl", [(40, 40), (32003, 32064)])
@pytest.mark.parametrize("rows", [1, 5])
def test_ban_tokens_dev_equals_the_scalar_entry_point(O, V, ldl, rows):
    """Bit-identical to ban_tokens at equal length, a batch step (one length for every row) and the rows of a verify step (ld_ids = 0,
    len_step = 1), a length of 0 and the all -inf row included; a length outside the history leaves the logits alone."""
    x0 = _logits(rows, V, ldl, seed=3)
    x0[0] = NEG_INF
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, 8, (rows, 24), generator=g).cuda()  # (a small alphabet: n-grams repeat, the word [5, 6] occurs)
    for P in (0, 6):
        kw = _tables(V, P)
        for length in (0, 1, 6, 7, 8, 9, 19):
            for base in (0, length, length + 3):  # the counter holds all of the length, part of it, or more (a negative offset)
                for layout in (dict(), dict(len_step=1, ld_ids=0)):
                    want = O.ban_tokens(x0.clone(), V, ids, len0=length, **layout, **kw)
                    got = O.ban_tokens_dev(x0.clone(), V, ids, _i32(base), len0=length - base, **layout, **kw)
                    assert torch.equal(got, want), (P, length, base, layout)
        assert int(torch.isinf(want[rows - 1, :V]).sum()) >= 2  # (the always list and the one-token word, whatever the history)
    for length in (25, 2 ** 31 - 1, -1):  # 25 > the row's 24 ids
        assert torch.equal(O.ban_tokens_dev(x0.clone(), V, ids, _i32(length), **kw), x0)
    assert torch.equal(O.ban_tokens_dev(x0.clone(), V, ids, _i32(24), **kw), O.ban_tokens(x0.clone(), V, ids, len0=24, **kw))
    # without a history (no n-gram, no words): the clauses keyed on the length alone still follow the counter
    nokw = {k: v for k, v in kw.items() if k not in ("ngram", "words", "word_off")}
    for length in (5, 6, 8, 9, 1000):
        want = O.ban_tokens(x0.clone(), V, None, len0=length, **nokw)
        assert torch.equal(O.ban_tokens_dev(x0.clone(), V, None, _i32(length - 2), len0=2, **nokw), want), length
    assert not torch.equal(want, x0) or rows == 1


@pytest.mark.parametrize("V,ldl", [(40, 40), (32003, 32064)])
def test_one_captured_graph_follows_the_device_counters(O, V, ldl):
    """The property the draft chain rests on: ONE graph holding a ban and a selection, replayed after nothing but the two counters changed,
    gives the scalar entry points' result for the new step and the new length - tokens, uniforms and the ids cell."""
    from merlin_amd import _lib as L

    rows, sel = 1, SEL[1]
    x0 = _logits(rows, V, ldl, seed=21)
    x = x0.clone()
    g = torch.Generator().manual_seed(2)
    hist = torch.randint(0, 8, (rows, 40), generator=g).cuda()
    ids = hist.clone()
    kw = _tables(V, 5)
    step, length = _i64(0), _i32(3)
    out = torch.zeros(rows, dtype=torch.int64, device="cuda")
    u = torch.zeros(rows, device="cuda")

    def body():
        x.copy_(x0)
        O.ban_tokens_dev(x, V, ids, length, len0=1, **kw)
        L.call("mh_select_tokens_dev", x, x.stride(0), rows, V, 1, sel["temperature"], sel["top_k"], sel["top_p"], 0.0, 0.0, sel["seed"], step, 2, out, u,
               ids, ids.stride(0), ids.shape[1], length, 1, O._stream())

    body()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    seen = set()
    for s, n in ((0, 3), (11, 4), (2 ** 40, 5), (6, 17), (6, 38)):
        ids.copy_(hist)
        step.fill_(s)
        length.fill_(n)
        graph.replay()
        want_x = O.ban_tokens(x0.clone(), V, hist, len0=n + 1, **kw)
        want, want_u = O.select_tokens(want_x, V, step=s + 2, return_u=True, **sel)
        assert torch.equal(x, want_x) and torch.equal(out, want) and torch.equal(u, want_u), (s, n)
        expect = hist.clone()
        expect[:, n + 1] = want
        assert torch.equal(ids, expect)
        seen.add((tuple(want.tolist()), float(want_u[0])))
    assert len(seen) > 2  # the replays did differ


def test_dev_forms_refuse_bad_arguments(O):
    from merlin_amd import _lib as L

    ERR = L.DEFINES["MH_ERR_ARG"]
    x = torch.zeros(2, 40, device="cuda")
    ids = torch.full((2, 8), -7, dtype=torch.int64, device="cuda")
    out = torch.full((2,), -9, dtype=torch.int64, device="cuda")
    step, length, one = _i64(0), _i32(4), _i64(3)
    st = O._stream()

    def select(logits=x, ldl=40, rows=2, V=40, step_base=step, out_=out, ids_=ids, ld=8, cols=8, len_base=length):
        return L.launch("mh_select_tokens_dev", logits, ldl, rows, V, 0, 1.0, 0, 1.0, 0.0, 0.0, 0, step_base, 0, out_, None, ids_, ld, cols, len_base, 0, st)

    def ban(logits=x, ldl=40, rows=2, V=40, ids_=ids, ld=8, cols=8, len_base=length, ngram=2):
        return L.launch("mh_ban_tokens_dev", logits, ldl, rows, V, ids_, ld, cols, len_base, 0, 0, ngram, None, None, 0, one, 1, None, 0, -1, None, 0, 0, st)

    for code in (select(step_base=None), select(len_base=None), select(V=0), select(ldl=39), select(rows=0), select(logits=None), select(out_=None), select(ld=7),
                 ban(len_base=None), ban(V=0), ban(ldl=39), ban(rows=0), ban(logits=None), ban(ids_=None), ban(ngram=-1), ban(ld=7)):
        assert code == ERR
    torch.cuda.synchronize()
    assert bool((x == 0).all()) and bool((ids == -7).all()) and bool((out == -9).all())
    assert select() == 0 and ban() == 0 and select(ids_=None, len_base=None) == 0 and ban(ids_=None, ngram=0) == 0
    assert out.tolist() == [0, 0] and ids[:, 4].tolist() == [0, 0] and bool(torch.isinf(x[:, 3]).all())


# ---- the draft chain ---------------------------------------------------------------------------------------------------------------------
GAIN = None
_CACHE = {}


def _fixture():
    """tests/test_bans_gpu.py's fixture (the tiny multimodal model, its prompt, its plain greedy continuation) and two drafts: a second
    instance with the target's weights, a different decoder - one layer, another seed, no vision tower (text-only) - and a third instance
    whose final norm weight is perturbed (a draft that agrees with the target at some positions and not at others)."""
    if "m" not in _CACHE:
        import test_bans_gpu as TB
        from oracle import cases as C
        from test_generation_gpu import _model
        from merlin_amd.model.llama_mmgpt import build_synthetic_model

        m, cfg, ids, images, plain = TB._fixture()
        _, _, twin = _model("tiny_1img", TB.GAIN)
        cfg1, _ = C.get_case("tiny_1img")
        llama = dict(vocab_size=cfg1.vocab_size - 3, hidden_size=cfg1.hidden_size, intermediate_size=cfg1.intermediate_size, num_hidden_layers=1,
                     num_attention_heads=cfg1.num_attention_heads, rms_norm_eps=cfg1.rms_norm_eps, rope_theta=cfg1.rope_theta, max_position_embeddings=8192)
        vision = dict(hidden_size=cfg1.v_hidden_size, intermediate_size=cfg1.v_intermediate_size, num_hidden_layers=1,
                      num_attention_heads=cfg1.v_num_attention_heads, image_size=cfg1.v_image_size, patch_size=cfg1.v_patch_size, layer_norm_eps=cfg1.v_layer_norm_eps)
        small = build_synthetic_model(llama, vision, projector=cfg1.projector, conv_stride=cfg1.conv_stride, dtype=torch.float16, device="cuda", seed=1)
        small.get_model().vision_tower = None  # text-only: the image-patch ids are ordinary embedding rows
        with torch.no_grad():
            small.model.norm.weight.mul_(TB.GAIN)
        small.engine.weights_changed()
        assert small.config.vocab_size == m.config.vocab_size and len(small.engine._ordered_params()) < len(twin.engine._ordered_params())
        _, _, near = _model("tiny_1img", TB.GAIN)
        with torch.no_grad():
            w = near.model.norm.weight
            w.mul_((1.0 + 0.35 * torch.randn(w.shape, generator=torch.Generator().manual_seed(5))).to(w))
        near.engine.weights_changed()
        _CACHE.update(m=m, cfg=cfg, ids=ids, images=images, plain=plain, twin=twin, small=small, near=near)
    c = _CACHE
    return c["m"], c["ids"], c["images"], c["plain"], c["twin"], c["small"]


@pytest.mark.parametrize("k", [1, 3, 15])
def test_capture_draft_graph_equals_eager_steps_with_scalar_selects(O, k):
    """The k drafted tokens of one replay are torch.equal to k eager decode steps with scalar bans and selects - greedy and sampling, with
    and without bans, and again after only the counters (and the input token) changed; the cache advanced by k."""
    from merlin_amd.generation import _ban_tables

    m, ids, images, plain, twin, small = _fixture()
    eng, V, P = small.engine, small.config.vocab_size, ids.shape[1]
    plan = dict(ngram=2, words=[[int(plain[0])], [7, 9]], always=[int(plain[1]), 5], begin=[int(plain[2])], min_new=3)
    eos = [int(plain[3])]
    for sel in (dict(do_sample=False, temperature=1.0, top_k=50, top_p=1.0, seed=0), dict(do_sample=True, temperature=0.9, top_k=50, top_p=1.0, seed=4242)):
        for bans in (False, True):
            tables = _ban_tables(plan, eos, P, ids.device) if bans else None
            _, cache = eng.prefill(ids, None, None, 2 * k + 2)
            seq = torch.zeros(1, P + 2 * k + 2, dtype=torch.int64, device="cuda")
            seq[0, :P] = ids[0]
            seq[0, P] = 11
            counters = torch.tensor([1, P + 1], dtype=torch.int64, device="cuda")
            graph, tok = eng.capture_draft_graph(cache, k, sel, tables, seq, (counters[:1], counters[1:].view(torch.int32)))
            assert int(cache.lens[0]) == P and tok.shape == (k + 1,)
            for rnd, (emitted, n) in enumerate(((1, P + 1), (2, P + 2))):  # the second round: one token more, the counters moved on
                if rnd:
                    cache.truncate(n - 1)
                    seq[0, n - 1] = 13
                counters.copy_(torch.tensor([emitted, n], dtype=torch.int64))
                tok[:1].copy_(seq[0, n - 1:n])
                graph.replay()
                got = tok[1:].clone()
                assert int(cache.lens[0]) == n - 1 + k
                assert torch.equal(seq[0, n:n + k], got) and int(seq[0, n - 1]) == (13 if rnd else 11)
                # the same k steps, eagerly, on a fresh cache
                _, ref = eng.prefill(ids, None, None, 2 * k + 2)
                hist = seq.clone()
                if rnd:
                    eng.decode_step(hist[0, P:P + 1], ref)
                want, t = [], hist[0, n - 1:n]
                for i in range(k):
                    lg = eng.decode_step(t, ref)
                    if bans:
                        O.ban_tokens(lg, V, hist, len0=n + i, **tables)
                    t = O.select_tokens(lg, V, step=emitted + i, **sel)
                    hist[0, n + i] = t[0]
                    want.append(int(t[0]))
                assert got.tolist() == want, (k, sel["do_sample"], bans, rnd)


# ---- generate() --------------------------------------------------------------------------------------------------------------------------
def _greedy_tie_ok(m, ids, images, got, want, kv8=False, **w):
    from test_spec_gpu import _same_or_greedy_tie

    _same_or_greedy_tie(m, ids, None, images, got, want, kv8, **w)


@pytest.mark.parametrize("arm", ["steps", "chain"])
def test_draft_with_the_targets_weights_is_accepted(arm):
    from test_generation_gpu import _same_or_tie

    m, ids, images, plain, twin, small = _fixture()
    P = ids.shape[1]
    kw = dict(images=images, max_new_tokens=24, eos_token_id=-1, pad_token_id=0)
    want = m.generate(ids, **kw).cpu()
    for k in (1, 5, 15):
        got = m.generate(ids, assistant_model=twin, num_assistant_tokens=k, **ARMS[arm], **kw).cpu()
        st = dict(m.engine.last_generate_stats)
        _same_or_tie(m, images, got, want, P, k)
        print(f"ASSISTED | twin | {arm} | k = {k} | {st}")
        assert got.shape == want.shape and st["verify_steps"] >= 1 and st["draft_steps"] >= st["drafted"] > 0
        # The twin's draft steps ARE the plain path's steps (same weights, same one-row kernels, same history), so its drafts are the plain
        # path's tokens bit for bit: the verify step rejects one only where its own many-row selection leaves the plain path - the step
        # _same_or_tie has just judged a tie.  Where the outputs are equal there was no such step.
        if got.tolist() == want.tolist():
            assert st["accepted"] == st["drafted"], st
            assert st["plain_steps"] + st["verify_steps"] + st["accepted"] == 23
    got = m.generate(ids, assistant_model=twin, **ARMS[arm], **kw)  # num_assistant_tokens=None: 5
    assert got.shape == want.shape and 0 < m.engine.last_generate_stats["drafted"] <= 5 * m.engine.last_generate_stats["verify_steps"]


ARMS = dict(steps=dict(), chain=dict(assistant_chain_graph=True), eager=dict(use_graph=False))


def test_a_different_draft_greedy_and_the_three_arms():
    """Greedy with the one-layer text-only draft and with the perturbed twin: the three arms - a single-step graph per draft step (the
    default), the chain graph, no graphs - emit identical tokens, which are the plain path's under _same_or_tie's rule."""
    from test_generation_gpu import _same_or_tie

    m, ids, images, plain, twin, small = _fixture()
    P = ids.shape[1]
    kw = dict(images=images, max_new_tokens=24, eos_token_id=-1, pad_token_id=0)
    want = m.generate(ids, **kw).cpu()
    for name, draft in (("small", small), ("near", _CACHE["near"])):
        outs, stats = {}, {}
        for arm, extra in ARMS.items():
            outs[arm] = m.generate(ids, assistant_model=draft, num_assistant_tokens=4, **extra, **kw).cpu()
            stats[arm] = dict(m.engine.last_generate_stats)
            print(f"ASSISTED | {name} greedy | {arm} | {stats[arm]}")
            assert stats[arm]["accepted"] < stats[arm]["drafted"] and stats[arm]["verify_steps"] >= 1
        assert torch.equal(outs["chain"], outs["steps"]) and torch.equal(outs["chain"], outs["eager"])
        assert stats["steps"] == stats["eager"]
        for key in ("plain_steps", "verify_steps", "drafted", "accepted"):  # (the chain also counts the steps it ran unused near max_length)
            assert stats["chain"][key] == stats["eager"][key]
        assert stats["chain"]["draft_steps"] >= stats["eager"]["draft_steps"]
        _same_or_tie(m, images, outs["chain"], want, P, name)
    # the perturbed twin is sometimes right: rounds end in the middle of a draft and the caches are rolled back to different lengths
    assert 0 < stats["eager"]["accepted"] < stats["eager"]["drafted"], stats["eager"]


@pytest.mark.parametrize("name", ["small", "near"])
def test_seeded_sampling_equals_plain_or_a_cdf_tie(name):
    """temperature 0.8, seed 4242 (the rule of tests/test_spec_gpu.py::test_seeded_sampling_lookup_equals_plain_or_a_cdf_tie): the three arms
    emit identical tokens; they are the plain path's, except from a step on where the selection's own uniform lies within 2e-3 of the
    inverse-CDF boundary between the two tokens, on the plain path's logits for the common prefix."""
    import numpy as np

    from merlin_amd import ops
    from oracle import gen_ref as R
    from test_spec_gpu import _step_logits

    m, ids, images, plain, twin, small = _fixture()
    draft = small if name == "small" else _CACHE["near"]
    P, V = ids.shape[1], m.config.vocab_size
    skw = dict(images=images, max_new_tokens=24, eos_token_id=-1, pad_token_id=0, do_sample=True, temperature=0.8, seed=4242)
    plain_s = m.generate(ids, **skw).cpu()
    outs = {}
    for arm, extra in ARMS.items():
        outs[arm] = m.generate(ids, assistant_model=draft, num_assistant_tokens=4, **extra, **skw).cpu()
        st = dict(m.engine.last_generate_stats)
        print(f"ASSISTED | {name} sampling | {arm} | {st}")
        assert st["accepted"] < st["drafted"]
    eager = outs["eager"]
    assert eager.shape == plain_s.shape and torch.equal(eager, outs["chain"]) and torch.equal(eager, outs["steps"]), {k: v.tolist() for k, v in outs.items()}
    if eager.tolist() != plain_s.tolist():
        t = int((eager[0] != plain_s[0]).nonzero()[0])
        assert t >= P
        lg = _step_logits(m, ids, None, images, plain_s[0, P:t].tolist())
        _, u = ops.select_tokens(lg[None].contiguous(), V, do_sample=True, temperature=0.8, top_k=50, top_p=1.0, seed=4242, step=t - P, return_u=True)
        u = float(u[0])
        cdf = np.cumsum(R.warp_probs(lg.cpu().numpy(), 0.8, 50, 1.0))
        for tok in (int(eager[0, t]), int(plain_s[0, t])):
            lo, hi = (cdf[tok - 1] if tok else 0.0), cdf[tok]
            assert lo - 2e-3 <= u <= hi + 2e-3, ("diverged at", t, "away from a CDF boundary", tok, u, lo, hi, eager.tolist(), plain_s.tolist())


@pytest.mark.parametrize("flags", [dict(fp8_kv=True), dict(fp8_weights=True), dict(fp4_weights=True), dict(fp4_weights=True, fp4_prefill=True)], ids=lambda f: "+".join(f))
def test_assisted_with_cache_and_weight_formats(flags):
    m, ids, images, plain, twin, small = _fixture()
    kw = dict(images=images, max_new_tokens=16, eos_token_id=-1, pad_token_id=0, **flags)
    want = m.generate(ids, **kw)
    got = m.generate(ids, assistant_model=small, num_assistant_tokens=4, **kw)
    assert got.shape == want.shape == (1, ids.shape[1] + 16) and m.engine.last_generate_stats["verify_steps"] >= 1
    if not flags.get("fp4_prefill"):  # (_step_logits prefills on the 16-bit weights: the rule's logits are those of the default prefill)
        _greedy_tie_ok(m, ids, images, got, want, bool(flags.get("fp8_kv")), fp8=bool(flags.get("fp8_weights")), fp4=bool(flags.get("fp4_weights")))
    else:
        n = int((got[0] == want[0]).long().cumprod(0).sum())
        assert n > ids.shape[1]  # the first token comes from the same prefill, whatever a later tie does
        if n < got.shape[1]:
            eng = m.engine
            lg, cache = eng.prefill(ids, None, images, 20, w_fp4=True)
            for t in want[0, ids.shape[1]:n].tolist():
                lg = eng.decode_step(torch.tensor([t], device="cuda"), cache, fp4=True)
            lg = lg[0, :m.config.vocab_size].float()
            assert float(lg.max() - lg[int(got[0, n])]) < 2e-3 * float(lg.abs().max())


def test_bans_hold_their_invariants():
    """With the options of tests/test_bans_gpu.py::_options: what the bans guarantee whatever the rounding, on both drafts, greedy, sampled
    and without graphs (the draft steps apply the bans too, through mh_ban_tokens_dev in the chain and mh_ban_tokens outside it)."""
    import test_bans_gpu as TB

    m, ids, images, plain, twin, small = _fixture()
    P = ids.shape[1]
    eos, opts, bkw = TB._options(plain)
    for extra in (dict(), dict(assistant_chain_graph=True), dict(do_sample=True, temperature=1.5, seed=4242), dict(do_sample=True, temperature=1.5, seed=4242, assistant_chain_graph=True),
                  dict(use_graph=False)):
        for draft in (twin, small):
            out = m.generate(ids, images=images, max_new_tokens=20, assistant_model=draft, num_assistant_tokens=4, **bkw, **extra).cpu()
            assert out.shape[1] > P + 6 and torch.equal(out[:, :P], ids.cpu())
            seq = out[0].tolist()
            if seq[-1] in eos:
                assert len(seq) - P > 6
            TB._assert_invariants(seq, P, eos, opts, ("assisted", extra))
            assert m.engine.last_generate_stats["verify_steps"] >= 1


def test_eos_inside_an_accepted_run_and_short_lengths():
    """EOS inside an accepted run stops there: the twin's drafts are the plain path's tokens, so the first round after the prefill's token
    accepts positions P + 1 .. P + 5; the EOS is the token the free-running continuation has there.  Then max_new_tokens of 1, 2, k + 1 and
    k + 3 (the last rounds use the drafts that still fit; the chain graph runs its k steps all the same).  All three arms."""
    from test_generation_gpu import _same_or_tie

    m, ids, images, plain, twin, small = _fixture()
    P = ids.shape[1]
    base = dict(images=images, max_new_tokens=12, pad_token_id=0)
    free = m.generate(ids, eos_token_id=-1, **base).cpu()
    for pos in (P + 2, P + 4):
        tok = int(free[0, pos])
        end = free[0].tolist().index(tok, P) + 1  # the first occurrence among the new tokens
        want = m.generate(ids, eos_token_id=tok, **base).cpu()
        assert want.shape[1] == end and int(want[0, -1]) == tok
        for arm, extra in ARMS.items():
            got = m.generate(ids, eos_token_id=tok, assistant_model=twin, num_assistant_tokens=5, **extra, **base).cpu()
            assert got.tolist() == want.tolist(), (pos, arm, got.tolist(), want.tolist())
            if end > P + 2:
                assert m.engine.last_generate_stats["accepted"] >= 1
    # lengths: max_new_tokens of 1, 2 and k + 1, both drafts, both arms - the plain path's first tokens
    k = 4
    for new in (1, 2, k + 1, k + 3):
        for draft in (twin, small):
            for arm, extra in ARMS.items():
                out = m.generate(ids, images=images, max_new_tokens=new, eos_token_id=-1, pad_token_id=0, assistant_model=draft, num_assistant_tokens=k, **extra).cpu()
                assert out.shape == (1, P + new) and torch.equal(out[:, :P], ids.cpu())
                _same_or_tie(m, images, out, free[:, :P + new], P, (new, arm))
    assert m.generate(ids, images=images, max_new_tokens=0, assistant_model=twin).shape == ids.shape


def test_streamer_receives_exactly_the_new_tokens():
    m, ids, images, plain, twin, small = _fixture()
    P = ids.shape[1]

    class Streamer:
        def __init__(self):
            self.puts, self.ended = [], False

        def put(self, t):
            self.puts.append(t.clone())

        def end(self):
            self.ended = True

    s = Streamer()
    got = m.generate(ids, images=images, max_new_tokens=12, eos_token_id=-1, pad_token_id=0, assistant_model=twin, num_assistant_tokens=4, streamer=s).cpu()
    st = m.engine.last_generate_stats
    assert s.ended and torch.equal(s.puts[0], ids.cpu())
    assert torch.cat([t.reshape(-1) for t in s.puts[1:]]).tolist() == got[0, P:].tolist()
    assert len(s.puts) - 1 == 1 + st["plain_steps"] + st["verify_steps"]


def test_without_an_assistant_nothing_new_is_launched(monkeypatch):
    """The launch symbols of generate() calls, recorded at the library boundary: assistant_model=None reaches neither device-counter form;
    with a draft, the default and use_graph=False select with the scalar launches (no device-counter launch either: those belong to the chain
    graph), and with assistant_chain_graph=True the device-counter launches are recorded once, at capture."""
    from merlin_amd import _lib as L

    m, ids, images, plain, twin, small = _fixture()
    names = []
    real = L.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(L, "call", recording)
    base = dict(images=images, max_new_tokens=6, eos_token_id=-1, pad_token_id=0)
    for extra in (dict(), dict(use_graph=False), dict(do_sample=True, temperature=0.8, seed=1), dict(prompt_lookup_num_tokens=4), dict(no_repeat_ngram_size=2)):
        for none in (dict(), dict(assistant_model=None, num_assistant_tokens=None), dict(assistant_model=None, num_assistant_tokens=7)):
            del names[:]
            m.generate(ids, **base, **extra, **none)
            assert "mh_select_tokens_dev" not in names and "mh_ban_tokens_dev" not in names, extra
            if not none:
                without = list(names)
            assert names == without, (extra, none)  # launch for launch what the call without the option launches
    del names[:]
    m.generate(ids, assistant_model=small, num_assistant_tokens=3, use_graph=False, **base)
    st = m.engine.last_generate_stats
    assert "mh_select_tokens_dev" not in names and "mh_ban_tokens_dev" not in names and st["draft_steps"] >= st["drafted"] > 0
    del names[:]
    m.generate(ids, assistant_model=small, num_assistant_tokens=3, no_repeat_ngram_size=2, **base)  # the default: a graph per draft step
    assert "mh_select_tokens_dev" not in names and "mh_ban_tokens_dev" not in names
    del names[:]
    m.generate(ids, assistant_model=small, num_assistant_tokens=3, no_repeat_ngram_size=2, assistant_chain_graph=True, **base)
    # one eager warm-up and one capture of the 3-step chain
    assert names.count("mh_select_tokens_dev") == names.count("mh_ban_tokens_dev") == 6
