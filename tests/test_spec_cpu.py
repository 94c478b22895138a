"""Prompt-lookup speculative decoding, host side: generate()'s new options and refusals (raised before any device work), the drafter's
restatement `generation._prompt_lookup` against transformers' own PromptLookupCandidateGenerator.get_candidates, and the accept rule as
a pure function.  The sequences of `lookup_cases()` are the ones tests/test_spec_gpu.py runs mh_ngram_draft on."""
import pytest
import torch

from merlin_amd import generation as G


def lookup_cases():
    """(ids, k, max_ngram, max_length): a few hundred random sequences over a vocabulary of 5 (lengths 2..40, k in {1, 3, 15}, n in
    {1, 2, 3}; max_length mostly out of the way, sometimes len + 1 - one token left - or below the sequence length, where it cuts the
    continuation), and hand-made ones: no match at all, a match whose continuation is cut by the sequence end, the max_length cap."""
    g = torch.Generator().manual_seed(20)
    cases = []
    for i in range(360):
        n = int(torch.randint(2, 41, (1,), generator=g))
        ids = torch.randint(0, 5, (n,), generator=g).tolist()
        k, ng = (1, 3, 15)[i % 3], (1, 2, 3)[(i // 3) % 3]
        max_length = (n + 50, n + 50, n + 2, n + 1, max(2, n - 3), max(2, n // 2))[(i // 9) % 6]
        cases.append((ids, k, ng, max_length))
    cases.append(([0, 1, 2, 3, 4], 3, 2, 60))                      # no token repeats: no match for any n
    cases.append(([7, 8, 9, 1, 7, 8], 15, 2, 60))                  # bigram (7, 8) at 0: continuation [9, 1, 7, 8], cut by the sequence end
    cases.append(([7, 8, 9, 1, 2, 3, 7, 8], 15, 2, 5))             # the same match under max_length = 5: [9, 1, 2]
    cases.append(([4, 4], 3, 2, 60))                               # n = 1 only (len - 1): window 0, continuation [4]
    cases.append(([1, 2, 1, 2, 1, 2], 3, 3, 60))                   # overlapping windows: the earliest trigram wins
    cases.append(([3, 1, 2, 5, 5, 1, 2, 9, 9, 1, 2], 1, 2, 60))    # two earlier occurrences: the EARLIEST one's continuation
    return cases


def test_prompt_lookup_equals_transformers_candidate_generator():
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator

    none = cut_by_end = capped = 0
    for ids, k, ng, max_length in lookup_cases():
        gen = PromptLookupCandidateGenerator(eos_token_id=None, num_output_tokens=k, max_matching_ngram_size=ng, max_length=max_length)
        x = torch.tensor([ids])
        want = gen.get_candidates(x)[0][0, len(ids):].tolist()
        got = G._prompt_lookup(ids, k, ng, max_length)
        assert got == want, (ids, k, ng, max_length, got, want)
        assert len(got) <= k
        none += not got
        cut_by_end += 0 < len(got) < k and max_length > len(ids) + 1
        capped += bool(got) and max_length < len(ids)
    assert none >= 10 and cut_by_end >= 10 and capped >= 10, (none, cut_by_end, capped)
    assert G._prompt_lookup([7, 8, 9, 1, 7, 8], 15, 2, 60) == [9, 1, 7, 8]
    assert G._prompt_lookup([7, 8, 9, 1, 2, 3, 7, 8], 15, 2, 5) == [9, 1, 2]
    assert G._prompt_lookup([0, 1, 2, 3, 4], 3, 2, 60) == []
    assert G._prompt_lookup([3, 1, 2, 5, 5, 1, 2, 9, 9, 1, 2], 1, 2, 60) == [5]


def test_accept_rule_corner_cases():
    never = lambda i: False  # noqa: E731
    # no draft token agrees: the step still emits the one token the plain step would have
    assert G._accept([5, 6, 7], [9, 1, 2, 3], 10, never) == ([9], 0, False)
    # all agree: the bonus token after the last draft is emitted too
    assert G._accept([5, 6, 7], [5, 6, 7, 8], 10, never) == ([5, 6, 7, 8], 3, False)
    # the first disagreement in the middle: the model's own token replaces the draft there, nothing behind it counts
    assert G._accept([5, 6, 7], [5, 9, 7, 8], 10, never) == ([5, 9], 1, False)
    # a short draft (padded rows behind it are never looked at)
    assert G._accept([5], [5, 4, 0, 0], 10, never) == ([5, 4], 1, False)
    # a stop inside the accepted run: emitted up to and including it, the criteria are not asked again
    asked = []

    def stop_at_1(i):
        asked.append(i)
        return i == 1

    assert G._accept([5, 6, 7], [5, 6, 7, 8], 10, stop_at_1) == ([5, 6], 3, True)
    assert asked == [0, 1]
    # the max_length cut: only `room` tokens fit, every emitted prefix is still shown to the criteria in order
    asked.clear()
    assert G._accept([5, 6, 7], [5, 6, 7, 8], 2, lambda i: asked.append(i) or False) == ([5, 6], 3, False)
    assert asked == [0, 1]
    assert G._accept([], [4], 1, never) == ([4], 0, False)


class _NoDevice:
    """A model whose every attribute is an error: the refusals must be raised before generate() looks at it."""

    def __getattr__(self, name):
        raise AssertionError(f"generate() touched model.{name} before refusing")


def test_options_and_refusals():
    ids = torch.ones(1, 4, dtype=torch.int64)
    o = G._resolve_options(None, dict(prompt_lookup_num_tokens=3))
    assert o["prompt_lookup_num_tokens"] == 3 and o["max_matching_ngram_size"] == 2
    assert G._resolve_options(None, {})["prompt_lookup_num_tokens"] is None
    assert G._resolve_options(None, dict(prompt_lookup_num_tokens=None))["prompt_lookup_num_tokens"] is None
    assert G._resolve_options(None, dict(prompt_lookup_num_tokens=4, max_matching_ngram_size=3))["max_matching_ngram_size"] == 3
    with pytest.raises(ValueError, match="num_beams"):
        G.generate(_NoDevice(), ids, prompt_lookup_num_tokens=3, num_beams=2, max_new_tokens=4)
    with pytest.raises(ValueError, match="use_cache"):
        G.generate(_NoDevice(), ids, prompt_lookup_num_tokens=3, use_cache=False, max_new_tokens=4)
    with pytest.raises(ValueError, match="assisted generate is only supported for batch_size = 1"):
        G.generate(_NoDevice(), torch.ones(2, 4, dtype=torch.int64), prompt_lookup_num_tokens=3, max_new_tokens=4)
    for bad in (0, 16, -1, 2.5, True):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
            G.generate(_NoDevice(), ids, prompt_lookup_num_tokens=bad, max_new_tokens=4)
    with pytest.raises(TypeError):
        G.generate(_NoDevice(), ids, prompt_lookup_tokens=3)
    with pytest.raises(TypeError):
        G._resolve_options(None, dict(prompt_lookup_num_token=3))


def test_none_takes_the_plain_path(monkeypatch):
    """prompt_lookup_num_tokens=None (the default) goes to _sample_cached with the lookup fields of the resolved call unset - and no
    session, bans or guide, as in every call that does not ask for them; a number goes to the lookup loop; every call fills
    engine.last_generate_stats."""
    calls = []

    class Cfg:
        eos_token_id, pad_token_id, vocab_size = 2, 0, 11

    class Eng:
        pass

    class M:
        config, engine = Cfg(), Eng()

    def plain(call, input_ids):
        assert call.model.config is M.config and call.max_len == 7 and call.stats is M.engine.last_generate_stats
        calls.append(("plain", call.lookup, call.max_ngram, call.session, call.bans, call.guide))
        return torch.cat([input_ids, torch.zeros(1, 3, dtype=torch.int64)], dim=1)

    def lookup(call, input_ids):
        calls.append(("lookup", call.lookup, call.max_ngram, call.session, call.bans, call.guide))
        return input_ids

    monkeypatch.setattr(G, "_sample_cached", plain)
    monkeypatch.setattr(G, "_sample_lookup", lookup)
    ids = torch.ones(1, 4, dtype=torch.int64)
    G.generate(M(), ids, max_new_tokens=3)
    G.generate(M(), ids, max_new_tokens=3, prompt_lookup_num_tokens=None)
    assert calls == [("plain", None, None, None, None, None)] * 2  # the plain loop, nothing of the other modes set
    assert M.engine.last_generate_stats == dict(plain_steps=2, verify_steps=0, drafted=0, accepted=0)
    G.generate(M(), ids, max_new_tokens=3, prompt_lookup_num_tokens=4, max_matching_ngram_size=3)
    assert calls[-1] == ("lookup", 4, 3, None, None, None)
    assert M.engine.last_generate_stats == dict(plain_steps=0, verify_steps=0, drafted=0, accepted=0)
