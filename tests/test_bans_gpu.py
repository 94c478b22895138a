"""Token bans, min_p and epsilon sampling on the GPU: mh_ban_tokens against transformers' logits processors run on the CPU (exact equality
of the -inf set, every other element bit-identical), the selection kernel on rows that hold -inf and with the min_p / epsilon warpers against
transformers' warper chain, and generate() with the options: teacher-forced against the same processors, the invariants the bans
guarantee, the prompt-lookup path against the plain path, and beam search against transformers' own generate on the same decoder."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from test_bans_cpu import ban_cases, hf_apply, hf_processors, hf_width  # noqa: E402

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def O():
    from merlin_amd import ops

    assert ops.arch_ok(0), "not a gfx950 device"
    return ops


def _tables(eos_ids, P, ngram=0, words=None, always=None, begin=None, min_new=0):
    """The options -> the keyword arguments of ops.ban_tokens, through generate()'s own resolution (plan + device tables)."""
    from merlin_amd import generation as G

    o = G._resolve_options(None, dict(no_repeat_ngram_size=ngram, bad_words_ids=words, suppress_tokens=always, begin_suppress_tokens=begin,
                                      min_new_tokens=min_new))
    plan = G._ban_plan(o, eos_ids)
    return plan, (G._ban_tables(plan, eos_ids, P, torch.device("cuda:0")) if plan is not None else dict())


def _check(O, x0, V, hist_rows, P, eos_ids, opts, **layout):
    """Run mh_ban_tokens on a copy of x0 [R, ldl] (guard rows around it) and compare with transformers row by row: hist_rows[r] is the
    history row r is conditioned on (a list)."""
    from merlin_amd.generation import _banned

    R, ldl = x0.shape
    buf = torch.full((R + 2, ldl), 7.25, dtype=torch.float32, device="cuda")
    buf[1:R + 1] = x0.cuda()
    plan, kw = _tables(eos_ids, P, **opts)
    O.ban_tokens(buf[1:R + 1], V, layout.pop("ids"), **layout, **kw)
    got = buf.cpu()
    assert bool((got[0] == 7.25).all()) and bool((got[R + 1] == 7.25).all()), "a row outside the launch was written"
    got = got[1:R + 1]
    procs = hf_processors(P, eos_ids, **opts)
    w = max(hf_width(V, h, opts) for h in hist_rows)  # one width for all rows: the word processor sizes its tables at its first call
    for r in range(R):
        h = hist_rows[r]
        s = torch.zeros(w)
        s[:V] = x0[r, :V]
        want = hf_apply(procs, h, s)[:V] if procs else s[:V]
        want_inf = torch.isinf(want)
        got_inf = torch.isinf(got[r, :V])
        assert torch.equal(got_inf, want_inf), (r, len(h), opts, sorted(set(got_inf.nonzero().reshape(-1).tolist()) ^ set(want_inf.nonzero().reshape(-1).tolist()))[:10])
        assert bool((got[r, :V][got_inf] == float("-inf")).all())
        keep = ~got_inf
        assert torch.equal(got[r, :V][keep].view(torch.int32), x0[r, :V][keep].view(torch.int32)), (r, "an element that is not banned changed")
        assert torch.equal(got[r, V:].view(torch.int32), x0[r, V:].view(torch.int32)), (r, "columns [V, ldl) were written")
        assert {t for t in _banned(h, P, plan, eos_ids) if t < V} == set(got_inf.nonzero().reshape(-1).tolist())


def _logits(R, ldl, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(R, ldl, generator=g) * 3


def _histories(R, L, V, n, seed):
    """R histories of length L over a small alphabet (n-grams repeat with different continuations), with a constant run, an id >= V, and -
    where they fit - the tail's prefix planted at window 0 and just before the last window."""
    rng = np.random.RandomState(seed)
    hs = []
    for r in range(R):
        base = [3, 5, 11, V - 1, 17][:2 + r % 4]
        h = [int(base[i]) for i in rng.randint(0, len(base), size=L)]
        if r % 3 == 1 and L >= 8:
            h[L // 2:L // 2 + 4] = [5] * 4  # a constant run
        if r % 3 == 2 and L >= 8:
            h[L - 6:] = [11] * 6            # ... and one the history ends in: the last window matches
        if L >= 6:
            h[int(rng.randint(0, L))] = V + 4 + r  # an id the logits have no column for
        if n > 1 and L >= 3 * n:
            tail = h[L - n + 1:]
            h[0:n - 1] = tail            # a match at window 0 ...
            h[n - 1] = (7 + r) % V
            h[L - 2 * n + 1:L - n] = tail  # ... and one whose continuation is the first token of the tail (the last window but n - 1)
        hs.append(h)
    return hs


@pytest.mark.parametrize("V,ldl", [(32003, 32064), (40, 40)])
@pytest.mark.parametrize("R", [1, 5, 16])
def test_ngram_clause_vs_transformers(O, V, ldl, R):
    x0 = _logits(R, ldl, 1)
    for n in (1, 2, 3, 5):
        for L in sorted({0, max(n - 2, 0), n - 1, n, 300, 700}):
            hs = _histories(R, L, V, n, seed=100 * n + L)
            ids = torch.full((R, max(L, 1) + 3), V + 1, dtype=torch.int64)  # (cells behind the valid length hold an id that would match nothing)
            for r in range(R):
                ids[r, :L] = torch.tensor(hs[r], dtype=torch.int64).reshape(-1)[:L]
            _check(O, x0, V, hs, 0, [], dict(ngram=n), ids=ids.cuda(), len0=L)


@pytest.mark.parametrize("case", ban_cases(), ids=lambda c: c[0])
def test_ban_cases_of_the_cpu_restatement(O, case):
    """The edge cases tests/test_bans_cpu.py holds generation._banned to, on the kernel (V = 40: fewer columns than threads)."""
    tag, h, P, eos, opts = case
    x0 = _logits(1, 40, 2)
    ids = torch.full((1, len(h) + 2), 45, dtype=torch.int64)
    ids[0, :len(h)] = torch.tensor(h, dtype=torch.int64).reshape(-1)
    _check(O, x0, 40, [h], P, eos, opts, ids=ids.cuda(), len0=len(h))


@pytest.mark.parametrize("V,ldl", [(32003, 32064), (40, 40)])
def test_all_clauses_at_once_rows_and_lengths(O, V, ldl):
    """Every clause in one launch, 16 rows; len on both sides of begin_index and of min_total; words of 1, 2 and 4 tokens, one longer than
    the history, one equal to [eos], one with a token >= V; two eos ids."""
    eos = [V - 2, 9]
    words = [[13], [5, 14], [3, 5, 3, 15], [3, 3, 3, 3, 3, 3, 3, 3, 3, 16], [9], [V + 3], [11, V + 3], [5, 5], [V - 1, 2]]
    opts = dict(ngram=3, words=words, always=[0, V - 1, V, V + 9], begin=[21, V - 3], min_new=3)
    x0 = _logits(16, ldl, 3)
    for P, L in ((6, 6), (6, 7), (6, 8), (6, 9), (6, 10), (2, 300)):
        hs = _histories(16, L, V, 3, seed=L)
        for r in range(0, 16, 2):
            hs[r][L - 1] = 5  # the words that start with 5 fire in every other row
        ids = torch.tensor(hs, dtype=torch.int64)
        _check(O, x0, V, hs, P, eos, opts, ids=ids.cuda(), len0=L)
    # the short history: a word of 4 and of 10 tokens cannot fire (L = 2), the word of L + 1 = 3 tokens does not either (transformers)
    hs = [[3, 5]] * 16
    _check(O, x0, V, hs, 2, eos, dict(opts, words=words + [[3, 5, 17]]), ids=torch.tensor(hs, dtype=torch.int64).cuda(), len0=2)


@pytest.mark.parametrize("V,ldl", [(32003, 32064), (40, 40)])
def test_verify_layout_one_sequence_growing_prefix(O, V, ldl):
    """ld_ids = 0, len_step = 1, 16 rows: row t is conditioned on seq[:n + t] - per-row transformers calls on the growing prefix."""
    eos = [7]
    opts = dict(ngram=2, words=[[5, 14], [3, 5, 3, 15], [13]], always=[1], begin=[21], min_new=4)
    x0 = _logits(16, ldl, 4)
    for n, P in ((9, 9), (290, 288), (1, 0)):
        seq = _histories(1, n + 15, V, 2, seed=n)[0]
        ids = torch.tensor([seq], dtype=torch.int64).cuda()
        _check(O, x0, V, [seq[:n + t] for t in range(16)], P, eos, opts, ids=ids, len0=n, len_step=1, ld_ids=0)


def test_ban_tokens_refuses_bad_arguments(O):
    from merlin_amd._lib import MerlinHipError

    x = torch.zeros(2, 40, device="cuda")
    ids = torch.zeros(2, 8, dtype=torch.int64, device="cuda")
    one = torch.tensor([3], dtype=torch.int64, device="cuda")
    with pytest.raises(MerlinHipError, match="bad argument"):
        O.ban_tokens(x, 41, ids, len0=4, ngram=2)             # V > ldl
    with pytest.raises(MerlinHipError, match="bad argument"):
        O.ban_tokens(x, 40, None, len0=4, ngram=2)            # an n-gram clause without a history
    with pytest.raises(MerlinHipError, match="bad argument"):
        O.ban_tokens(x, 40, ids, len0=4, ngram=-1)
    with pytest.raises(AssertionError):
        O.ban_tokens(x, 40, ids, len0=8, len_step=1, ngram=2)  # row 1 would read 9 ids of 8
    with pytest.raises(AssertionError):
        O.ban_tokens(x, 40, ids.to(torch.int32), len0=4, ngram=2)
    assert bool((x == 0).all())
    O.ban_tokens(x, 40, None, always=one)                      # no history needed
    assert bool(torch.isinf(x[:, 3]).all()) and int(torch.isinf(x).sum()) == 2


def test_ban_tokens_is_capturable(O):
    """No allocation, no read-back, no synchronisation: the launch records into a HIP graph and replays on new logits and a longer history."""
    x = torch.zeros(2, 40, device="cuda")
    ids = torch.tensor([[3, 4, 3, 0], [5, 6, 7, 5]], dtype=torch.int64, device="cuda")
    O.ban_tokens(x.clone(), 40, ids, len0=3, ngram=2)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        O.ban_tokens(x, 40, ids, len0=3, ngram=2)
    x.zero_()
    g.replay()
    assert torch.isinf(x).nonzero().tolist() == [[0, 4]]
    x.zero_()
    ids[0, 2] = 9
    g.replay()
    assert torch.isinf(x).nonzero().tolist() == []


# ---- selection: -inf rows, min_p, epsilon ------------------------------------------------------------------------------------------------------
def _hf_probs(row, T, k, p, min_p, eps):
    """transformers' warper chain on one row -> (probabilities float64, the scores min_p saw, the scores epsilon saw)."""
    from transformers.generation import logits_process as lp

    s = row[None].clone()
    s = lp.TemperatureLogitsWarper(T)(None, s)
    if k:
        s = lp.TopKLogitsWarper(k)(None, s)
    if p < 1:
        s = lp.TopPLogitsWarper(p)(None, s)
    before_min_p = s.clone()
    if min_p is not None:
        s = lp.MinPLogitsWarper(min_p)(None, s)
    before_eps = s.clone()
    if 0 < eps < 1:
        s = lp.EpsilonLogitsWarper(eps)(None, s)
    return torch.softmax(s.double(), -1)[0].numpy(), before_min_p[0], before_eps[0]


def _away_from_thresholds(before_min_p, before_eps, min_p, eps):
    """The condition on the INPUTS: no logit within 1e-4 of the min_p threshold z_max + ln(min_p) or of the epsilon threshold
    (ln p_i = ln eps, p the softmax of what min_p left)."""
    if min_p:
        z = before_min_p[torch.isfinite(before_min_p)].double()
        assert float((z - (z.max() + np.log(min_p))).abs().min()) > 1e-4
    if eps:
        lp_ = torch.log_softmax(before_eps.double(), -1)
        lp_ = lp_[torch.isfinite(lp_)]
        assert float((lp_ - np.log(eps)).abs().min()) > 1e-4


WARP = [(0.7, 50, 1.0, 0.1, 0.0), (1.0, 0, 0.9, 0.05, 3e-3), (1.3, 0, 1.0, None, 0.01), (0.2, 50, 1.0, 0.3, 0.02), (1.0, 50, 0.95, 0.5, 0.0),
        (0.9, 0, 1.0, 0.0, 0.2)]


def _rows_with_inf(V):
    """Three rows of V logits: finite; with banned tokens, one thread's whole chunk among them; with only 30 allowed tokens (fewer than top_k =
    50 asks for), the chunk of the row's first thread banned."""
    rng = np.random.RandomState(8)
    C = (V + 255) // 256
    a = (rng.standard_normal(V) * 3).astype(np.float32)
    b = a.copy()
    b[rng.randint(0, V, size=V // 5)] = -np.inf
    b[5 * C:6 * C] = -np.inf
    c = np.full(V, -np.inf, dtype=np.float32)
    allowed = rng.choice(np.arange(C, V), size=30, replace=False)
    c[allowed] = (rng.standard_normal(30) * 2).astype(np.float32)
    return [torch.from_numpy(r) for r in (a, b, c)]


@pytest.mark.parametrize("cfg", WARP, ids=str)
def test_select_tokens_min_p_epsilon_and_banned_rows_vs_transformers(O, cfg):
    from oracle import gen_ref as G

    T, k, p, min_p, eps = cfg
    V = 1000  # chunks of 4 columns per thread
    for ri, row in enumerate(_rows_with_inf(V)):
        probs, s1, s2 = _hf_probs(row, T, k, p, min_p, eps)
        _away_from_thresholds(s1, s2, min_p, eps)
        assert (probs[torch.isinf(row).numpy()] == 0).all()
        cdf = np.cumsum(probs)
        lg = torch.full((64, V + 8), 50.0)  # (columns behind V hold the largest value of all: never looked at)
        lg[:, :V] = row
        lg = lg.cuda()
        assert torch.equal(O.select_tokens(lg, V).cpu(), row.argmax().expand(64))  # greedy = argmax, banned tokens or not
        for step in range(4):
            tok, u = O.select_tokens(lg, V, do_sample=True, temperature=T, top_k=k, top_p=p, min_p=min_p, epsilon_cutoff=eps, seed=99, step=step, return_u=True)
            tok, u = tok.cpu().numpy(), u.cpu().numpy()
            for r in range(64):
                assert abs(u[r] - G.counter_uniform(99, step, r)) < 1e-7
                t = int(tok[r])
                assert 0 <= t < V and probs[t] > 0, ("sampled a token the warpers removed", cfg, ri, r, t)
                lo = cdf[t - 1] if t > 0 else 0.0
                assert lo - 2e-5 <= u[r] <= cdf[t] + 2e-5, (cfg, ri, r, t, u[r], lo, cdf[t])


def test_select_tokens_neutral_warpers_are_todays_tokens_and_all_banned_row(O):
    from merlin_amd import _lib as L

    g = torch.Generator().manual_seed(3)
    x = (torch.randn(7, 32064, generator=g) * 2).cuda()
    V = 32003
    x[1, 100:20000] = float("-inf")
    for kw in (dict(temperature=0.8, top_k=50, top_p=1.0), dict(temperature=1.2, top_k=0, top_p=0.9), dict(temperature=0.3, top_k=5, top_p=0.5)):
        for step in (0, 3):
            old = O.select_tokens(x, V, do_sample=True, seed=5, step=step, **kw)
            assert torch.equal(old, O.select_tokens(x, V, do_sample=True, seed=5, step=step, min_p=None, epsilon_cutoff=0.0, **kw))
            assert torch.equal(old, O.select_tokens(x, V, do_sample=True, seed=5, step=step, min_p=0.0, **kw))  # the new entry point at its neutral values
            out = torch.empty(7, dtype=torch.int64, device="cuda")
            L.call("mh_select_tokens_warp", x, x.stride(0), 7, V, 1, kw["temperature"], kw["top_k"], kw["top_p"], 0.0, 0.0, 5, step, out, None, None)
            assert torch.equal(old, out)
    # select_tokens_multi with the warpers = one select_tokens per position
    y = x[:6].view(2, 3, -1)
    multi = O.select_tokens_multi(y, V, do_sample=True, temperature=0.9, top_k=0, top_p=1.0, seed=11, step0=4, min_p=0.2, epsilon_cutoff=1e-3)
    for t in range(3):
        assert torch.equal(multi[t], O.select_tokens(y[:, t].contiguous(), V, do_sample=True, temperature=0.9, top_k=0, top_p=1.0, seed=11, step=4 + t, min_p=0.2, epsilon_cutoff=1e-3))
    # greedy on a row of -inf only: index 0, like argmax
    z = torch.full((2, 300), float("-inf"), device="cuda")
    z[1, 299] = -3.0
    assert O.select_tokens(z).tolist() == [0, 299]
    with pytest.raises(L.MerlinHipError, match="bad argument"):
        O.select_tokens(x, V, do_sample=True, min_p=1.5)
    with pytest.raises(L.MerlinHipError, match="bad argument"):
        O.select_tokens(x, V, do_sample=True, epsilon_cutoff=1.0)


# ---- generate() --------------------------------------------------------------------------------------------------------------------------------
GAIN = 25.0
_CACHE = {}


def _fixture():
    """The tiny multimodal model (tiny_1img, V = 103, logits peaked with logit_gain as tests/test_generation_gpu.py::_model builds it), its
    prompt and the plain greedy continuation the options below are chosen from - built once."""
    if "m" not in _CACHE:
        from test_generation_gpu import _model

        cfg, batch, m = _model("tiny_1img", GAIN)
        ids = batch["input_ids"][:, :22].cuda()
        images = [im.cuda() for im in batch["images"]]
        plain = m.generate(ids, images=images, max_new_tokens=12, eos_token_id=-1, pad_token_id=0).cpu()[0, 22:].tolist()
        _CACHE.update(m=m, cfg=cfg, ids=ids, images=images, plain=plain)
    c = _CACHE
    return c["m"], c["cfg"], c["ids"], c["images"], c["plain"]


def _options(plain):
    """Options that bite on the plain continuation: its first token may not begin, its second is an eos that min_new_tokens holds back, no
    3-gram repeats (the tiny model loops), one token is suppressed and two words are bad."""
    eos = [int(plain[1]), 101]
    opts = dict(ngram=3, words=[[int(plain[2])], [int(plain[0]), int(plain[3])], [101]], always=[int(plain[5]), 102], begin=[int(plain[0])], min_new=6)
    kw = dict(no_repeat_ngram_size=3, bad_words_ids=opts["words"], suppress_tokens=opts["always"], begin_suppress_tokens=opts["begin"], min_new_tokens=6,
              eos_token_id=eos, pad_token_id=0)
    return eos, opts, kw


def _teacher_forced(m, V, out, am, images, P, eos, opts, tag):
    """For every generated position t of every row: the model's own forward logits on out[:, :t], transformers' processors for the options on
    the CPU, then: the emitted token is not banned and lies within _same_or_tie's bound (2e-3 of the largest logit magnitude) of the
    processed maximum.  -> the number of steps whose RAW argmax was banned."""
    out = out.cpu()
    procs = hf_processors(P, eos, **opts)
    hits = 0
    for b in range(out.shape[0]):
        done = False
        for t in range(P, out.shape[1]):
            if done:
                break
            a = None if am is None else torch.cat([am[b:b + 1].cuda(), torch.ones(1, t - P, dtype=am.dtype, device="cuda")], dim=1)
            with torch.no_grad():
                lg = m(input_ids=out[b:b + 1, :t].cuda(), attention_mask=a, images=images[b:b + 1] if images is not None else None).logits[0, -1, :V].float().cpu()
            s = hf_apply(procs, out[b, :t].tolist(), lg)
            tok = int(out[b, t])
            assert torch.isfinite(s[tok]), (tag, "emitted a banned token", b, t, tok)
            gap, tol = float(s.max() - s[tok]), 2e-3 * float(lg.abs().max())
            print(f"BANS | {tag} | row {b} | t {t} | tok {tok} | gap {gap:.3e} | tol {tol:.3e} | raw argmax banned {bool(torch.isinf(s[int(lg.argmax())]))}")
            assert gap < tol, (tag, "not the processed maximum", b, t, tok, gap, tol)
            hits += int(torch.isinf(s[int(lg.argmax())]))
            done = tok in eos
    return hits


@pytest.mark.parametrize("mode", ["graph", "no_graph", "no_cache", "fp8_kv"])
def test_greedy_with_bans_teacher_forced(mode):
    m, cfg, ids, images, plain = _fixture()
    eos, opts, kw = _options(plain)
    extra = dict(graph=dict(), no_graph=dict(use_graph=False), no_cache=dict(use_cache=False), fp8_kv=dict(fp8_kv=True))[mode]
    out = m.generate(ids, images=images, max_new_tokens=12, **kw, **extra)
    assert out.shape[1] > 22 + 6  # min_new_tokens
    assert _teacher_forced(m, cfg.vocab_size, out, None, images, 22, eos, opts, mode) >= 1


def test_greedy_with_bans_left_padded_batch():
    """Two left-padded prompts of different lengths: the history the bans see holds the pads (transformers' convention)."""
    m, cfg, ids, images, plain = _fixture()
    eos, opts, kw = _options(plain)
    pads = torch.zeros(1, 3, dtype=torch.int64, device="cuda")
    more = torch.tensor([[17, 23]], device="cuda")
    ids2 = torch.cat([torch.cat([pads[:, :1], ids, more], dim=1), torch.cat([pads, ids], dim=1)], dim=0)  # 1 pad + 22 + 2 text tokens | 3 pads + 22
    am = torch.ones_like(ids2)
    am[0, :1] = 0
    am[1, :3] = 0
    P = ids2.shape[1]
    out = m.generate(ids2, images=images * 2, attention_mask=am, max_new_tokens=10, **kw)
    assert torch.equal(out[:, :P], ids2)
    assert _teacher_forced(m, cfg.vocab_size, out, am, images * 2, P, eos, opts, "left-padded") >= 2


def test_greedy_with_bans_through_a_session():
    """The second call reuses a prefix from the session's cache; the history of the bans is the call's whole input_ids all the same."""
    m, cfg, ids, images, plain = _fixture()
    eos, opts, kw = _options(plain)
    s = m.new_session()
    out1 = m.generate(ids, images=images, max_new_tokens=4, session=s, **kw)
    ids2 = torch.cat([out1, torch.tensor([[17, 23, 9, 41]], device="cuda")], dim=1)
    P = ids2.shape[1]
    # the second turn's own plain continuation gives the options that bite there
    plain2 = m.generate(ids2, images=images, max_new_tokens=8, eos_token_id=-1, pad_token_id=0).cpu()[0, P:].tolist()
    eos2, opts2, kw2 = _options(plain2 + plain)
    out2 = m.generate(ids2, images=images, max_new_tokens=10, session=s, **kw2)
    assert s.last["reused_tokens"] >= 22 and s.last["run_tokens"] == P - s.last["reused_tokens"]
    assert _teacher_forced(m, cfg.vocab_size, out2, None, images, P, eos2, opts2, "session") >= 1


def _assert_invariants(seq, P, eos, opts, tag):
    """What the bans guarantee whatever the rounding: on the generated part of seq (a list) no n-gram ends that occurred before, no bad word,
    no suppressed id, no begin-suppressed id at position P, no eos before min_new_tokens."""
    n = opts["ngram"]
    words = [w for w in opts["words"] if not any(w == [e] for e in eos)]  # (a word equal to [eos] is no bad word)
    for t in range(P, len(seq)):
        if t + 1 >= n:
            gram = seq[t + 1 - n:t + 1]
            assert all(seq[i:i + n] != gram for i in range(0, t + 1 - n)), (tag, "repeated n-gram ending at", t, gram)
        for w in words:
            assert seq[t + 1 - len(w):t + 1] != w, (tag, "bad word ending at", t, w)  # (every word here is shorter than the prompt)
        assert seq[t] not in opts["always"], (tag, "suppressed id at", t)
        if t - P < opts["min_new"]:
            assert seq[t] not in eos, (tag, "eos at new token", t - P)
    assert seq[P] not in opts["begin"], (tag, "begin-suppressed id first")


@pytest.mark.parametrize("mode", ["greedy", "sample", "sample_min_p_eps", "beams", "beams_shared_fp8", "sample_lookup_fp4"])
def test_invariants_of_the_bans(mode):
    """Includes the combinations the docstring promises: bans with share_prompt_kv + fp8_kv + fp8_weights beams, and with
    prompt_lookup_num_tokens + fp4_weights sampling."""
    m, cfg, ids, images, plain = _fixture()
    eos, opts, kw = _options(plain)
    extra = dict(greedy=dict(), sample=dict(do_sample=True, temperature=1.5, seed=4242),
                 sample_min_p_eps=dict(do_sample=True, temperature=1.5, seed=7, min_p=0.02, epsilon_cutoff=1e-3, top_k=0),
                 beams=dict(num_beams=4), beams_shared_fp8=dict(num_beams=3, share_prompt_kv=True, fp8_kv=True, fp8_weights=True),
                 sample_lookup_fp4=dict(do_sample=True, temperature=0.7, seed=3, prompt_lookup_num_tokens=4, fp4_weights=True))[mode]
    out = m.generate(ids, images=images, max_new_tokens=20, **kw, **extra).cpu()
    assert out.shape[1] > 22 + 6 and torch.equal(out[:, :22], ids.cpu())
    seq = out[0].tolist()
    if seq[-1] in eos:
        assert len(seq) - 22 > 6
    _assert_invariants(seq, 22, eos, opts, mode)


def test_prompt_lookup_with_bans_gives_the_plain_paths_tokens():
    """prompt_lookup_num_tokens=4 with the options: the plain path's tokens, or first different at a step where both tokens lie within 2e-3
    of the largest magnitude of the PROCESSED maximum of the plain path's logits (the rule of tests/test_spec_gpu.py, applied behind the
    bans); verify steps ran."""
    from test_spec_gpu import _step_logits

    m, cfg, ids, images, plain = _fixture()
    V = cfg.vocab_size
    # 4-grams may not repeat: the tiny model's loops still give the drafter 2-grams to continue, and a draft's third token is banned
    eos = [101]
    opts = dict(ngram=4, words=[[int(plain[2])], [101]], always=[102], begin=[int(plain[0])], min_new=0)
    kw = dict(images=images, max_new_tokens=24, no_repeat_ngram_size=4, bad_words_ids=opts["words"], suppress_tokens=[102], begin_suppress_tokens=opts["begin"],
              eos_token_id=eos, pad_token_id=0)
    want = m.generate(ids, **kw).cpu()
    assert m.engine.last_generate_stats["verify_steps"] == 0
    for use_graph in (True, False):
        got = m.generate(ids, prompt_lookup_num_tokens=4, use_graph=use_graph, **kw).cpu()
        st = dict(m.engine.last_generate_stats)
        assert st["verify_steps"] > 0, st
        _assert_invariants(got[0].tolist(), 22, eos, opts, ("lookup", use_graph))
        if got.tolist() == want.tolist():
            continue
        n = min(got.shape[1], want.shape[1])
        diff = (got[0, :n] != want[0, :n]).nonzero()
        assert diff.numel(), ("one is a prefix of the other", got.tolist(), want.tolist())
        t = int(diff[0])
        assert t >= 22
        lg = _step_logits(m, ids, None, images, want[0, 22:t].tolist()).cpu()
        s = hf_apply(hf_processors(22, eos, **opts), want[0, :t].tolist(), lg)
        tol = 2e-3 * float(lg.abs().max())
        gaps = [float(s.max() - s[int(x[0, t])]) for x in (got, want)]
        assert max(gaps) < tol, ("diverged at", t, "without a tie", gaps, tol, got.tolist(), want.tolist())


# ---- beam search against transformers' own generate ------------------------------------------------------------------------------------------
PROMPTS = [[1, 66, 83, 94, 84, 58, 16, 79, 36], [1, 85, 27, 95, 51, 35, 48, 7, 37, 15, 4, 77], [1, 87, 84, 94, 27, 20, 70],
           [1, 46, 67, 82, 99, 26, 30, 73, 92, 13], [1, 30, 47, 17, 10, 58], [1, 67, 43, 30, 98, 8, 56, 74]]
# (logit gain, eos id, prompt, num_beams, the option): 16 new tokens each.  Chosen on the CPU model: with each of them transformers gives the
# same tokens in fp32 and after .to(torch.float16), and other tokens than without the option - both asserted below.
BEAM_CASES = [
    (25.0, 24, 0, 3, dict(no_repeat_ngram_size=2)),
    (15.0, 94, 3, 5, dict(no_repeat_ngram_size=3)),
    (30.0, 46, 4, 3, dict(no_repeat_ngram_size=2)),
    (25.0, 24, 0, 5, dict(bad_words_ids=[[76, 93]])),
    (40.0, 57, 2, 3, dict(bad_words_ids=[[76, 76]])),
    (15.0, 94, 3, 5, dict(bad_words_ids=[[85], [74, 74]])),
    (25.0, 24, 0, 3, dict(suppress_tokens=[40, 93])),
    (25.0, 52, 5, 5, dict(suppress_tokens=[57])),
    (15.0, 94, 3, 3, dict(begin_suppress_tokens=[85])),
    (25.0, 52, 5, 3, dict(begin_suppress_tokens=[57, 5])),
    (40.0, 76, 2, 3, dict(min_new_tokens=5)),
    (25.0, 46, 5, 5, dict(min_new_tokens=9)),
]
_HF = {}


def _hf_beam(gain, half, ids, nb, eos, **opt):
    from oracle import cases as C
    from oracle.make_gen_golden import hf_llama

    if (gain, half) not in _HF:
        cfg, _ = C.get_case("tiny_1img")
        mm = hf_llama(cfg, gain)
        _HF[(gain, half)] = mm.to(torch.float16) if half else mm
    with torch.no_grad():
        return _HF[(gain, half)].generate(ids, max_new_tokens=16, num_beams=nb, do_sample=False, eos_token_id=eos, pad_token_id=0, **opt).tolist()


def test_beam_cases_cover_every_ban_option():
    names = [next(iter(c[4])) for c in BEAM_CASES]
    assert len(BEAM_CASES) >= 6
    for k in ("no_repeat_ngram_size", "bad_words_ids", "suppress_tokens", "begin_suppress_tokens", "min_new_tokens"):
        assert names.count(k) >= 2, k


@pytest.mark.parametrize("i", range(len(BEAM_CASES)))
def test_beam_search_with_bans_matches_transformers(i):
    from test_generation_gpu import _model

    gain, eos, pi, nb, opt = BEAM_CASES[i]
    ids = torch.tensor([PROMPTS[pi]], dtype=torch.int64)
    want = _hf_beam(gain, False, ids, nb, eos, **opt)
    assert want == _hf_beam(gain, True, ids, nb, eos, **opt), "not admissible: transformers' fp32 and fp16 tokens differ"
    assert want != _hf_beam(gain, False, ids, nb, eos), "not admissible: the option changes nothing"
    key = ("beam", gain)
    if key not in _CACHE:
        _CACHE[key] = _model("tiny_1img", gain)[2]
    m = _CACHE[key]
    kw = dict(max_new_tokens=16, num_beams=nb, eos_token_id=eos, pad_token_id=0, **opt)
    copy = m.generate(ids.cuda(), **kw).cpu().tolist()
    share = m.generate(ids.cuda(), share_prompt_kv=True, **kw).cpu().tolist()
    sess = m.generate(ids.cuda(), session=m.new_session(), **kw).cpu().tolist()
    assert copy == want, (BEAM_CASES[i], copy, want)
    assert share == copy and sess == copy, (BEAM_CASES[i], copy, share, sess)


def test_calls_without_the_options_launch_nothing_new(monkeypatch):
    """The launch symbols of generate() calls, recorded at the library boundary: without the new options no mode reaches mh_ban_tokens or
    mh_select_tokens_warp; with bans every selected token is preceded by exactly one mh_ban_tokens launch."""
    from merlin_amd import _lib as L

    m, cfg, ids, images, plain = _fixture()
    names = []
    real = L.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(L, "call", recording)
    base = dict(images=images, max_new_tokens=6, eos_token_id=-1, pad_token_id=0)
    for extra in (dict(), dict(use_graph=False), dict(use_cache=False), dict(do_sample=True, temperature=0.8, seed=1), dict(prompt_lookup_num_tokens=4),
                  dict(num_beams=3), dict(num_beams=3, share_prompt_kv=True), dict(session=m.new_session())):
        m.generate(ids, **base, **extra)
    assert "mh_select_tokens" in names and "mh_log_softmax_rows" in names
    assert "mh_ban_tokens" not in names and "mh_select_tokens_warp" not in names
    del names[:]
    m.generate(ids, no_repeat_ngram_size=2, **base)
    assert names.count("mh_ban_tokens") == names.count("mh_select_tokens") == 6 and "mh_select_tokens_warp" not in names
    del names[:]
    m.generate(ids, do_sample=True, seed=1, min_p=0.1, **base)
    assert names.count("mh_select_tokens_warp") == 6 and "mh_select_tokens" not in names and "mh_ban_tokens" not in names
