"""Assisted decoding with a draft model (generate(assistant_model=..., num_assistant_tokens=k)), the host side: option resolution, the
refusals by name before any device work, the cache bookkeeping as a pure function, and the factored speculative loop
(generation._draft_loop) driven by toy drafters and a toy target - pure functions from history to token on a CPU ids buffer."""
import pytest
import torch

from merlin_amd import generation as G


class _NoDevice:  # generate() resolves its options before it touches the model or the ids
    def __getattr__(self, name):
        raise AssertionError(f"device work before validation: {name}")


class _Cfg:
    eos_token_id, pad_token_id, vocab_size = 2, 0, 11


class _Model:
    """Enough of a merlin_amd model for the refusals: .config and .engine, and nothing that works."""
    config, engine = _Cfg(), _NoDevice()


def _draft(vocab=11):
    class Cfg(_Cfg):
        vocab_size = vocab

    class D:
        config, engine = Cfg(), _NoDevice()

    return D()


# ---- options ---------------------------------------------------------------------------------------------------------------------------
def test_the_options_are_accepted():
    """Both names are implemented options now (they raised NotImplementedError, or were ignored, as neutral ones)."""
    d = _draft()
    o = G._resolve_options(None, dict(assistant_model=d, num_assistant_tokens=4))
    assert o["assistant_model"] is d and o["num_assistant_tokens"] == 4
    assert "assistant_model" not in G._NEUTRAL and "num_assistant_tokens" not in G._NEUTRAL
    assert G._DEFAULTS["assistant_model"] is None and G._DEFAULTS["num_assistant_tokens"] is None
    ids = torch.ones(1, 4, dtype=torch.int64)
    assert G._resolve_assistant(o, d, _Model(), None, ids, None) == 4
    assert G._resolve_assistant(G._resolve_options(None, dict(assistant_model=d)), d, _Model(), None, ids, torch.ones(1, 4)) == 5  # None means 5
    for k in (1, 15):
        assert G._resolve_assistant(G._resolve_options(None, dict(assistant_model=d, num_assistant_tokens=k)), d, _Model(), None, ids, None) == k
    # without an assistant the count is not looked at (a transformers GenerationConfig carries its own default)
    assert G._resolve_options(None, dict(num_assistant_tokens=20))["assistant_model"] is None


def test_none_takes_the_plain_path_and_a_model_the_assisted_loop(monkeypatch):
    calls = []

    def plain(call, input_ids):
        calls.append(("plain", call.assistant, call.n_assist))
        return torch.cat([input_ids, torch.zeros(1, 3, dtype=torch.int64)], dim=1)

    def assisted(call, input_ids):
        calls.append(("assisted", call.assistant, call.n_assist, call.lookup, dict(call.stats)))
        return input_ids

    monkeypatch.setattr(G, "_sample_cached", plain)
    monkeypatch.setattr(G, "_sample_assisted", assisted)
    ids = torch.ones(1, 4, dtype=torch.int64)
    M, d = _Model(), _draft()
    M.engine = type("Eng", (), {})()
    G.generate(M, ids, max_new_tokens=3, assistant_model=None, num_assistant_tokens=None)
    assert calls == [("plain", None, None)]
    assert M.engine.last_generate_stats == dict(plain_steps=2, verify_steps=0, drafted=0, accepted=0)  # no new key without the option
    G.generate(M, ids, max_new_tokens=3, assistant_model=d, num_assistant_tokens=3)
    assert calls[-1] == ("assisted", d, 3, None, dict(plain_steps=0, verify_steps=0, drafted=0, accepted=0, draft_steps=0))


REFUSALS = [
    (dict(num_beams=2), "num_beams"),
    (dict(use_cache=False), "assisted generate requires `use_cache=True`"),
    (dict(guidance_scale=1.5), "guidance_scale"),
    (dict(session=type("S", (), dict(fp8_kv=False))()), "session="),
    (dict(prompt_lookup_num_tokens=3), "prompt_lookup_num_tokens"),
    (dict(num_assistant_tokens=0), "num_assistant_tokens"), (dict(num_assistant_tokens=16), "num_assistant_tokens"),
    (dict(num_assistant_tokens=-1), "num_assistant_tokens"), (dict(num_assistant_tokens=2.5), "num_assistant_tokens"),
    (dict(num_assistant_tokens=True), "num_assistant_tokens"),
    (dict(assistant_model=object()), "has to be a merlin_amd model"),
]


@pytest.mark.parametrize("extra,msg", REFUSALS, ids=[m[:24] for _, m in REFUSALS])
def test_refusals_by_name_before_device_work(extra, msg):
    """The model is an object whose every attribute raises: nothing of it is touched before the refusal."""
    ids = torch.ones(1, 4, dtype=torch.int64)
    kw = dict(assistant_model=_draft(), max_new_tokens=4)
    kw.update(extra)
    with pytest.raises(ValueError, match=msg):
        G.generate(_NoDevice(), ids, **kw)


def test_refusals_that_look_at_the_prompt_and_the_vocabulary():
    ids = torch.ones(1, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="assisted generate is only supported for batch_size = 1"):
        G.generate(_NoDevice(), torch.ones(2, 4, dtype=torch.int64), assistant_model=_draft(), max_new_tokens=4)
    am = torch.tensor([[0, 1, 1, 1]])
    with pytest.raises(ValueError, match="un-padded prompt"):
        G.generate(_NoDevice(), ids, attention_mask=am, assistant_model=_draft(), max_new_tokens=4)
    with pytest.raises(ValueError, match="vocab_size = 12, the model 11"):
        G.generate(_Model(), ids, assistant_model=_draft(12), max_new_tokens=4)  # (_Model's engine raises on any use)
    with pytest.raises(TypeError):
        G.generate(_NoDevice(), ids, assistant_models=_draft())
    # the chain graph is an option of assisted calls that use graphs: nothing is silently dropped
    with pytest.raises(ValueError, match="assistant_chain_graph=True"):
        G.generate(_NoDevice(), ids, assistant_chain_graph=True, max_new_tokens=4)
    with pytest.raises(ValueError, match="assistant_chain_graph=True"):
        G.generate(_NoDevice(), ids, assistant_model=_draft(), assistant_chain_graph=True, use_graph=False, max_new_tokens=4)


# ---- cache bookkeeping -----------------------------------------------------------------------------------------------------------------
def test_cache_bookkeeping_is_exhaustive_for_small_rounds():
    """Simulated with explicit key lists: before a round both caches hold seq[:n - 1]; the draft is fed c tokens, the target verifies and
    accepts a.  Afterwards the target holds all but the last token of the new sequence, the draft the same or - a == c - one key less."""
    for n in range(1, 7):
        for k in range(1, 5):
            for c in range(1, k + 1):
                for a in range(0, c + 1):
                    seq = list(range(100, 100 + n))
                    drafts = [200 + i for i in range(c)]
                    accepted = drafts[:a]
                    target_keys = seq[:n - 1] + [seq[n - 1]] + accepted          # verify writes last + drafts, advance(a + 1) keeps these
                    draft_fed = seq[:n - 1] + [seq[n - 1]] + drafts[:c - 1]      # the chain fed last, d_1 .. d_{c-1}
                    new_seq = seq + accepted + [999]                             # the a accepted drafts and the target's own token
                    t, d, owed = G._assisted_caches(n, c, a)
                    assert t == len(target_keys) == len(new_seq) - 1 and target_keys == new_seq[:-1]
                    assert d == min(len(draft_fed), t) and owed == t - d == (1 if a == c else 0)
                    assert draft_fed[:d] == new_seq[:d]  # what the truncated draft cache holds is a prefix of the new sequence
                    if owed:
                        assert new_seq[d] == drafts[-1]  # the key it is short of is the last draft: fed first in the next round
    for bad in ((0, 1, 0), (3, 0, 0), (3, 2, 3), (3, 2, -1)):
        with pytest.raises(ValueError):
            G._assisted_caches(*bad)


def test_rounds_near_max_length_use_the_drafts_that_fit():
    for k in range(1, 5):
        for max_len in range(2, 12):
            for n in range(1, max_len):
                c = G._drafts_that_fit(n, k, max_len)
                assert 0 <= c <= k and n + c + 1 <= max_len or c == 0
                assert c == k or n + c + 1 == max_len or (c == 0 and n + 1 == max_len)  # never fewer than fit
                if c:
                    t, d, owed = G._assisted_caches(n, c, c)
                    assert t + 1 <= max_len  # a fully accepted round ends at or below max_length


# ---- the loop, on toys -------------------------------------------------------------------------------------------------------------------
V = 13


def _target_fn(h):
    """The toy target: next token from the history, a pure function (never 0 = pad; 1 is the EOS of the tests that use one)."""
    return 2 + (3 * h[-1] + 5 * len(h) + (h[-2] if len(h) > 1 else 0)) % (V - 2)


class _ToyTarget:
    def __init__(self, seq, P, fn=_target_fn):
        self.seq, self.P, self.fn, self.keys, self.calls = seq, P, fn, P, []

    def plain(self, n):
        assert self.keys == n - 1  # the cache holds all but the last token
        self.keys += 1
        self.calls.append(("plain", n))
        return [self.fn(self.seq[0, :n].tolist())]

    def verify(self, n, draft, d):
        assert self.keys == n - 1 and len(draft) >= d >= 1
        h = self.seq[0, :n].tolist()
        self.calls.append(("verify", n, d))
        return [self.fn(h + list(draft[:t])) for t in range(d + 1)], list(draft[:d])

    def advance(self, m):
        self.keys += m


class _ToyDrafter:
    """k draft steps per round from `fn(history) -> token`, with _ModelDrafter's bookkeeping: `fed` keys, catch-up steps, commit."""

    def __init__(self, seq, P, k, max_len, fn):
        self.seq, self.k, self.max_len, self.fn, self.fed, self.steps, self.rounds = seq, k, max_len, fn, P, 0, []

    def propose(self, n):
        d = G._drafts_that_fit(n, self.k, self.max_len)
        if d == 0:
            return 0, None
        while self.fed < n - 1:
            self.fed += 1
            self.steps += 1
        assert self.fed == n - 1
        h = self.seq[0, :n].tolist()
        draft = []
        for _ in range(d):
            draft.append(self.fn(h + draft))
            self.fed += 1
            self.steps += 1
        return d, draft

    def commit(self, n, d, a):
        t, keep, owed = G._assisted_caches(n, d, a)
        assert self.fed == n - 1 + d and keep == min(self.fed, t)
        self.fed = keep
        self.rounds.append((n, d, a))


def _agree(h):
    return _target_fn(h)


def _never(h):
    return 2 + (_target_fn(h) - 2 + 1) % (V - 2)


def _every_other(h):
    return _target_fn(h) if len(h) % 2 == 0 else _never(h)


def _plain(prompt, max_len, eos, fn=_target_fn):
    h = list(prompt)
    while len(h) < max_len:
        h.append(fn(h))
        if h[-1] in eos:
            break
    return h


def _replay(seq, P, k, max_len, fn):
    """The assisted loop replayed over a finished sequence -> (verify steps, plain steps, drafted, accepted, draft steps)."""
    n, fed = P + 1, P
    ver = pl = drafted = accepted = steps = 0
    while n < len(seq):
        d = G._drafts_that_fit(n, k, max_len)
        if d == 0:
            pl, n = pl + 1, n + 1
            continue
        steps += (n - 1 - fed) + d
        draft, h = [], seq[:n]
        for _ in range(d):
            draft.append(fn(h + draft))
        a = 0
        while a < d and n + a < len(seq) and draft[a] == seq[n + a]:
            a += 1
        full = a  # the agreeing prefix against the target's own selections, which may run past the emitted sequence's end
        while full < d and draft[full] == _target_fn(h + draft[:full]):
            full += 1
        ver, drafted, accepted = ver + 1, drafted + d, accepted + min(a, len(seq) - n)
        fed = min(n - 1 + d, n + full)
        n += a + 1
    return ver, pl, drafted, accepted, steps


def _run(prompt, k, max_len, fn, eos=(), streamer=None):
    P = len(prompt)
    seq = torch.zeros(1, max_len + k, dtype=torch.int64)
    seq[0, :P] = torch.tensor(prompt)
    stats = dict(plain_steps=0, verify_steps=0, drafted=0, accepted=0, draft_steps=0)
    target, drafter = _ToyTarget(seq, P), _ToyDrafter(seq, P, k, max_len, fn)
    n = G._draft_loop(seq, P, max_len, G._Stopper(max_len, list(eos), None), streamer, stats, [_target_fn(prompt)], drafter, target)
    return seq[0, :n].tolist(), stats, target, drafter


@pytest.mark.parametrize("name,fn", [("agrees", _agree), ("never", _never), ("every_other", _every_other)])
@pytest.mark.parametrize("k", [1, 3, 4])
def test_loop_emits_the_targets_own_sequence(name, fn, k):
    prompt = [3, 7, 4]
    for max_len in (4, 5, 5 + k, 19, 20):
        want = _plain(prompt, max_len, ())
        got, stats, target, drafter = _run(prompt, k, max_len, fn)
        assert got == want and len(got) == max_len, (name, k, max_len)
        ver, pl, drafted, accepted, steps = _replay(want, len(prompt), k, max_len, fn)
        assert stats == dict(plain_steps=pl, verify_steps=ver, drafted=drafted, accepted=accepted, draft_steps=steps), (name, k, max_len, stats)
        assert stats["draft_steps"] == drafter.steps and stats["accepted"] <= stats["drafted"] <= k * stats["verify_steps"]
        assert len(got) - len(prompt) == 1 + stats["plain_steps"] + stats["verify_steps"] + stats["accepted"]
        if max_len >= 19:
            if name == "agrees":
                assert stats["accepted"] >= stats["drafted"] - k and stats["accepted"] > 0  # all but a last round cut by max_length
                assert any(a == d for _, d, a in drafter.rounds) and stats["draft_steps"] > stats["drafted"]  # owed keys were caught up
            if name == "never":
                assert stats["accepted"] == 0 and stats["verify_steps"] == max_len - len(prompt) - 1 - stats["plain_steps"]
            if name == "every_other" and k > 1:
                assert 0 < stats["accepted"] < stats["drafted"]


@pytest.mark.parametrize("name,fn", [("agrees", _agree), ("never", _never), ("every_other", _every_other)])
def test_loop_stops_at_eos_inside_an_accepted_run_and_streams(name, fn):
    prompt, k, max_len = [3, 7, 4], 4, 24
    free = _plain(prompt, max_len, ())
    for pos in (3, 5, 8, 12):  # the token at this position becomes the EOS: the output ends at its first occurrence
        eos = [free[pos]]
        want = _plain(prompt, max_len, eos)
        assert want[-1] == eos[0] and len(want) <= pos + 1

        class Streamer:
            puts = []

            def put(self, t):
                self.puts.append(t.reshape(-1).tolist())

        s = Streamer()
        s.puts = []
        got, stats, target, drafter = _run(prompt, k, max_len, fn, eos=eos, streamer=s)
        assert got == want, (name, pos)
        assert [t for p in s.puts for t in p] == want[len(prompt):]
        assert stats == dict(zip(("verify_steps", "plain_steps", "drafted", "accepted", "draft_steps"), _replay(want, len(prompt), k, max_len, fn)))


def test_lookup_loop_is_the_same_loop():
    """_sample_lookup and _sample_assisted differ in the drafter alone: both go through _draft_loop with the same target class."""
    import inspect

    for fn in (G._sample_lookup, G._sample_assisted):
        src = inspect.getsource(fn)
        assert "_draft_loop(" in src and "_StepTarget(" in src and "while " not in src
    assert "_NgramDrafter(" in inspect.getsource(G._sample_lookup) and "_ModelDrafter(" in inspect.getsource(G._sample_assisted)
