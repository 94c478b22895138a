"""Token bans and the min_p / epsilon options of generate(), host side: option resolution and validation (before any device work), the
options that stay refused, generation._banned against transformers' logits processors chained on the CPU, and the word-table packer.
`hf_processors` / `hf_banned` / `ban_cases` are what tests/test_bans_gpu.py runs mh_ban_tokens against."""
import numpy as np
import pytest
import torch

V_SMALL = 40


def hf_processors(P, eos_ids, ngram=0, words=None, always=None, begin=None, min_new=0):
    """transformers' processors for the options, in the order of `_get_logits_processor` and under its conditions."""
    from transformers.generation import logits_process as lp

    procs = []
    if ngram > 0:
        procs.append(lp.NoRepeatNGramLogitsProcessor(ngram))
    if words:
        procs.append(lp.NoBadWordsLogitsProcessor(words, eos_ids if eos_ids else None))
    if min_new > 0 and eos_ids:
        procs.append(lp.MinNewTokensLengthLogitsProcessor(P, min_new, eos_ids))
    if always:
        procs.append(lp.SuppressTokensLogitsProcessor(always))
    if begin:
        procs.append(lp.SuppressTokensAtBeginLogitsProcessor(begin, P))
    return procs


def hf_apply(procs, ids_row, scores):
    """scores fp32 [V] -> processed scores after the processors saw the history ids_row (a list of ints)."""
    ids = torch.tensor([list(ids_row)], dtype=torch.int64).reshape(1, len(ids_row))
    s = scores[None].clone()
    for p in procs:
        s = p(ids, s)
    return s[0]


def hf_width(V, ids_row, opts):
    """transformers' processors index the scores with every id they ban, so an id >= V (the image placeholders of a padded vocabulary, say)
    needs scores that wide: they are run on max(V, largest id + 1) columns and the first V are compared."""
    ids = list(ids_row) + [t for w in (opts.get("words") or []) for t in w] + list(opts.get("always") or []) + list(opts.get("begin") or [])
    return max([V] + [int(t) + 1 for t in ids])


def hf_banned(ids_row, V, P, eos_ids, **opts):
    s = hf_apply(hf_processors(P, eos_ids, **opts), ids_row, torch.zeros(hf_width(V, ids_row, opts)))[:V]
    return set(torch.nonzero(torch.isinf(s)).reshape(-1).tolist())


def _opts_to_plan(eos_ids, ngram=0, words=None, always=None, begin=None, min_new=0):
    from merlin_amd.generation import _ban_plan, _resolve_options

    o = _resolve_options(None, dict(no_repeat_ngram_size=ngram, bad_words_ids=words, suppress_tokens=always, begin_suppress_tokens=begin,
                                    min_new_tokens=min_new))
    return _ban_plan(o, eos_ids)


def ban_cases(V=V_SMALL):
    """(tag, history, P, eos_ids, options): the edge cases of the five clauses, then random histories with every clause at once.  Ids may
    be >= V (they compare as history, they are never a target)."""
    c = []
    # no_repeat_ngram_size
    c.append(("ngram3 two continuations", [5, 6, 7, 5, 6, 9, 5, 6], 2, [], dict(ngram=3)))
    c.append(("ngram3 overlapping windows", [4, 4, 4, 4], 1, [], dict(ngram=3)))
    c.append(("ngram1 bans the history", [3, 9, 3, 11], 1, [], dict(ngram=1)))
    c.append(("ngram2 constant run", [8] * 12, 3, [], dict(ngram=2)))
    c.append(("ngram5 match at window 0 only", [1, 2, 3, 4, 30, 9, 9, 1, 2, 3, 4], 4, [], dict(ngram=5)))
    c.append(("ngram3 match at the last window", [9, 1, 2, 7, 1, 2], 2, [], dict(ngram=3)))
    c.append(("ngram2 history ids >= V", [V + 3, 5, V + 3, 6, V + 3], 2, [], dict(ngram=2)))
    c.append(("ngram2 banned id >= V", [5, V + 9, 5], 2, [], dict(ngram=2)))
    for n in (1, 2, 3, 5):
        for L in sorted({0, max(n - 2, 0), n - 1, n}):
            c.append((f"ngram{n} L={L}", [7] * L, 0, [], dict(ngram=n)))
    # bad words
    words = [[11], [3, 12], [1, 2, 3, 13], [2, 3, 14], [V + 5], [6, V + 1]]
    c.append(("words len 1/2/4 fire", [9, 1, 2, 3], 1, [], dict(words=words)))
    c.append(("word longer than L + 1", [3], 1, [], dict(words=[[1, 2, 3, 13], [5, 3, 14]])))
    c.append(("word of length L + 1 (transformers: longer than the context)", [2, 3], 1, [], dict(words=[[2, 3, 14], [1, 2, 3, 13], [3, 15]])))
    c.append(("words on an empty history", [], 0, [], dict(words=words)))
    c.append(("word equal to [eos] is dropped", [9, 3], 1, [12, 11], dict(words=[[11], [3, 12], [12], [17]])))
    # min_new_tokens / begin_suppress_tokens on both sides of their thresholds, two eos ids
    for L in (4, 5, 6, 7):
        c.append((f"min_new 2 begin L={L} P=5", list(range(20, 20 + L)), 5, [7, 31], dict(min_new=2, begin=[4, 33], always=[0, V - 1, V, V + 7])))
    c.append(("min_new without eos", [1, 2], 2, [], dict(min_new=3)))
    # everything at once on random histories (small alphabet: n-grams repeat, words fire)
    rng = np.random.RandomState(5)
    for t in range(24):
        L = int(rng.choice([0, 1, 2, 3, 6, 17, 40, 90]))
        P = int(rng.randint(0, L + 1))
        h = rng.randint(0, 6, size=L).tolist()
        if L > 4:
            h[int(rng.randint(0, L))] = V + 2
        n = int(rng.choice([1, 2, 3, 5]))
        ws = [rng.randint(0, 6, size=int(k)).tolist() for k in rng.choice([1, 2, 2, 4], size=5)] + [[31]]
        c.append((f"random {t}", h, P, [31, 2], dict(ngram=n, words=ws, always=[38, 39], begin=[20, 21], min_new=int(rng.randint(0, 4)))))
    return c


def test_resolve_options_accepts_the_seven_options_keywords_win():
    from merlin_amd.generation import _ban_plan, _resolve_options

    o = _resolve_options(None, {})
    assert (o["no_repeat_ngram_size"], o["bad_words_ids"], o["min_new_tokens"], o["suppress_tokens"], o["begin_suppress_tokens"], o["min_p"],
            o["epsilon_cutoff"]) == (0, None, 0, None, None, None, 0.0)
    assert _ban_plan(o, [2]) is None
    kw = dict(no_repeat_ngram_size=3, bad_words_ids=[[5], [6, 7]], min_new_tokens=4, suppress_tokens=[1, 2], begin_suppress_tokens=torch.tensor([9]),
              min_p=0.1, epsilon_cutoff=3e-4)
    o = _resolve_options(None, dict(kw))
    assert o["no_repeat_ngram_size"] == 3 and o["bad_words_ids"] == [[5], [6, 7]] and o["min_new_tokens"] == 4 and o["suppress_tokens"] == [1, 2]
    assert o["begin_suppress_tokens"] == [9] and o["min_p"] == 0.1 and o["epsilon_cutoff"] == 3e-4
    assert _ban_plan(o, [2]) == dict(ngram=3, words=[[5], [6, 7]], always=[1, 2], begin=[9], min_new=4)
    assert _ban_plan(o, [5])["words"] == [[6, 7]] and _ban_plan(o, [])["min_new"] == 0

    class GC:  # a transformers.GenerationConfig stand-in
        no_repeat_ngram_size, bad_words_ids, min_new_tokens, suppress_tokens, begin_suppress_tokens, min_p, epsilon_cutoff = 2, [[8]], 1, [3], [4], 0.2, 0.01
        typical_p = None
    o = _resolve_options(GC(), {})
    assert (o["no_repeat_ngram_size"], o["bad_words_ids"], o["min_new_tokens"], o["suppress_tokens"], o["begin_suppress_tokens"], o["min_p"],
            o["epsilon_cutoff"]) == (2, [[8]], 1, [3], [4], 0.2, 0.01)
    o = _resolve_options(GC(), dict(no_repeat_ngram_size=5, min_p=0.5, suppress_tokens=[7]))
    assert o["no_repeat_ngram_size"] == 5 and o["min_p"] == 0.5 and o["suppress_tokens"] == [7] and o["bad_words_ids"] == [[8]]
    from transformers import GenerationConfig

    o = _resolve_options(GenerationConfig(no_repeat_ngram_size=3, bad_words_ids=[[5, 6]], min_p=0.05), dict(min_new_tokens=2))
    assert o["no_repeat_ngram_size"] == 3 and o["bad_words_ids"] == [[5, 6]] and o["min_p"] == 0.05 and o["min_new_tokens"] == 2
    # an explicit None is the default, [] is off
    o = _resolve_options(None, dict(no_repeat_ngram_size=None, min_new_tokens=None, epsilon_cutoff=None, bad_words_ids=[], suppress_tokens=[]))
    assert o["no_repeat_ngram_size"] == 0 and o["min_new_tokens"] == 0 and o["epsilon_cutoff"] == 0.0 and _ban_plan(o, [1]) is None


@pytest.mark.parametrize("bad,msg", [
    (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"), (dict(no_repeat_ngram_size=2.0), "no_repeat_ngram_size"),
    (dict(no_repeat_ngram_size=True), "no_repeat_ngram_size"),
    (dict(bad_words_ids=[[]]), "bad_words_ids"), (dict(bad_words_ids=[3, 4]), "has to be a list of lists"), (dict(bad_words_ids=[[3, -1]]), "list of positive integers"),
    (dict(bad_words_ids=[[3.5]]), "list of positive integers"), (dict(bad_words_ids="ab"), "has to be a non-empty list"),
    (dict(suppress_tokens=[-2]), "suppress_tokens"), (dict(begin_suppress_tokens=[1.5]), "begin_suppress_tokens"),
    (dict(min_p=-0.1), "`min_p` has to be a float in the \\[0, 1\\] interval"), (dict(min_p=1.5), "min_p"), (dict(min_p="x"), "min_p"),
    (dict(epsilon_cutoff=1.0), "`epsilon_cutoff` has to be a float > 0 and < 1"), (dict(epsilon_cutoff=-1e-3), "epsilon_cutoff"),
    (dict(min_new_tokens=-1), "`min_new_tokens` has to be a positive integer"), (dict(min_new_tokens=1.5), "min_new_tokens"),
])
def test_invalid_values_are_refused_before_device_work(bad, msg):
    from merlin_amd import generation as G

    with pytest.raises(ValueError, match=msg):
        G._resolve_options(None, dict(bad))

    class NoDevice:  # generate() resolves its options before it touches the model or the ids
        def __getattr__(self, name):
            raise AssertionError(f"device work before validation: {name}")

    with pytest.raises(ValueError, match=msg):
        G.generate(NoDevice(), NoDevice(), **bad)


def test_options_that_stay_refused():
    from merlin_amd.generation import _NEUTRAL, _resolve_options

    for bad in (dict(repetition_penalty=1.2), dict(min_length=5), dict(logits_processor=[object()]), dict(num_return_sequences=3), dict(output_scores=True),
                dict(return_dict_in_generate=True), dict(forced_bos_token_id=1), dict(forced_eos_token_id=2), dict(typical_p=0.9), dict(eta_cutoff=1e-3),
                dict(prefix_allowed_tokens_fn=lambda b, i: [1]), dict(sequence_bias={(5,): -1.0})):
        (k,) = bad
        assert k in _NEUTRAL
        with pytest.raises(NotImplementedError, match=k):
            _resolve_options(None, bad)
    for k in ("no_repeat_ngram_size", "bad_words_ids", "min_new_tokens", "suppress_tokens", "begin_suppress_tokens", "min_p", "epsilon_cutoff"):
        assert k not in _NEUTRAL


@pytest.mark.parametrize("case", ban_cases(), ids=lambda c: c[0])
def test_banned_equals_transformers_processors(case):
    from merlin_amd.generation import _banned

    tag, h, P, eos, opts = case
    plan = _opts_to_plan(eos, **opts)
    want = hf_banned(h, V_SMALL, P, eos, **opts)
    got = _banned(h, P, plan, eos)
    assert {t for t in got if t < V_SMALL} == want, (tag, sorted(got), sorted(want))


def test_banned_edge_cases_by_value():
    from merlin_amd.generation import _banned

    plan = lambda **kw: _opts_to_plan(kw.pop("eos", []), **kw)  # noqa: E731
    assert _banned([5, 6, 7, 5, 6, 9, 5, 6], 2, plan(ngram=3), []) == {7, 9}
    assert _banned([4, 4, 4, 4], 1, plan(ngram=3), []) == {4}
    assert _banned([3, 9, 3, 11], 1, plan(ngram=1), []) == {3, 9, 11}
    assert _banned([4], 0, plan(ngram=3), []) == set() and _banned([4, 4], 0, plan(ngram=3), []) == set()
    assert _banned([9, 4], 1, plan(words=[[11], [3, 12], [12]], eos=[12]), [12]) == {11}  # the word [eos] is dropped ...
    assert _banned([9, 3], 1, plan(words=[[11], [3, 12], [12]], eos=[12]), [12]) == {11, 12}  # ... a longer word that ends in eos is not
    assert _banned([2, 3], 1, plan(words=[[2, 3, 14], [3, 15]]), []) == {15}  # a word of L + 1 tokens is longer than the context
    assert _banned([9, 3], 1, plan(words=[[11], [3, 12]]), []) == {11, 12}
    assert _banned([3], 1, plan(words=[[1, 2, 3, 13]]), []) == set()
    p = plan(min_new=2, begin=[4], always=[0], eos=[7, 31])
    assert _banned([1] * 5, 5, p, [7, 31]) == {0, 4, 7, 31} and _banned([1] * 6, 5, p, [7, 31]) == {0, 7, 31} and _banned([1] * 7, 5, p, [7, 31]) == {0}
    assert _banned([1, 2, 1], 1, None, [3]) == set()


def test_word_table_round_trips():
    from merlin_amd.generation import _pack_words, _unpack_words

    rng = np.random.RandomState(1)
    for words in ([[7]], [[1, 2], [3]], [[5, 5, 5, 5], [9], [2, 1]], [rng.randint(0, 50000, size=int(k)).tolist() for k in rng.randint(1, 9, size=64)]):
        flat, off = _pack_words(words)
        assert off[0] == 0 and off[-1] == len(flat) == sum(len(w) for w in words) and len(off) == len(words) + 1
        assert all(b > a for a, b in zip(off, off[1:]))
        assert _unpack_words(flat, off) == words
    assert _pack_words([]) == ([], [0])
