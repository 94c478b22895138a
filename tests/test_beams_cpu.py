"""Beam search on a shared prompt KV cache, host side: generate()'s share_prompt_kv keyword and its refusals (raised before any device
work), and the ancestry rule of mh_beam_ancestry restated in a few lines of Python against physical row gathering (what
engine.reorder_cache does to the cache rows).  `ancestry_step` is the restatement tests/test_beams_gpu.py holds the kernel to."""
import os
import sys

import pytest
import torch

from merlin_amd import generation as G

sys.path.insert(0, os.path.dirname(__file__))
from test_spec_cpu import _NoDevice  # noqa: E402


def ancestry_step(anc, beam_idx, gen):
    """anc: list of rows (lists of length G); -> the table after one reorder at `gen` suffix rows written: row m continues beam_idx[m]'s
    history and will write its next key / value into its own row."""
    out = [list(row) for row in anc]
    for m, src in enumerate(beam_idx):
        out[m][:gen] = anc[src][:gen]
        out[m][gen] = m
    return out


def test_share_prompt_kv_keyword_and_refusals():
    ids = torch.ones(1, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="num_beams"):
        G.generate(_NoDevice(), ids, share_prompt_kv=True, num_beams=1, max_new_tokens=4)
    with pytest.raises(ValueError, match="num_beams"):
        G.generate(_NoDevice(), ids, share_prompt_kv=True, max_new_tokens=4)  # num_beams defaults to 1
    with pytest.raises(ValueError, match="num_beams"):
        G.generate(_NoDevice(), ids, share_prompt_kv=True, num_beams=17, max_new_tokens=4)  # more beams than one query tile
    with pytest.raises(TypeError):
        G.generate(_NoDevice(), ids, share_prompt_kvs=True, num_beams=2, max_new_tokens=4)
    # an explicit keyword of generate(), like fp8_kv: not one of the HF options _resolve_options reads, which stay as they were
    with pytest.raises(TypeError, match="share_prompt_kv"):
        G._resolve_options(None, dict(share_prompt_kv=True))
    assert G._resolve_options(None, dict(num_beams=5))["num_beams"] == 5
    assert "share_prompt_kv" not in G._resolve_options(None, {})


def test_default_and_flag_reach_beam_search(monkeypatch):
    """share_prompt_kv=False (the default) and True reach _beam_search in the resolved call, fp8_kv beside them, and nothing of the modes
    the calls do not ask for: no session, bans or guide."""
    seen = []

    class Cfg:
        eos_token_id, pad_token_id, vocab_size = 2, 0, 11

    class M:
        config = Cfg()

    def beam(call, input_ids):
        assert call.model.config is M.config and (call.num_beams, call.max_len) == (3, 7)
        seen.append((call.share_prompt_kv, call.fp8_kv, call.session, call.bans, call.guide))
        return input_ids

    monkeypatch.setattr(G, "_beam_search", beam)
    ids = torch.ones(1, 4, dtype=torch.int64)
    G.generate(M(), ids, num_beams=3, max_new_tokens=3)
    G.generate(M(), ids, num_beams=3, max_new_tokens=3, share_prompt_kv=True, fp8_kv=True)
    assert seen == [(False, False, None, None, None), (True, True, None, None, None)]


@pytest.mark.parametrize("seed", range(6))
def test_ancestry_rule_reproduces_row_gathering(seed):
    """12 steps of random in-group beam_idx (duplicates and dropped beams, now and then one parent for all or the identity), Bp = 2
    groups of nb = 5: the history of every beam read through the table - key g of beam m from suffix row anc[m][g], slot g - equals the
    explicit per-beam histories under `row i <- row beam_idx[i]`, where every step appends one new entry per beam."""
    g = torch.Generator().manual_seed(seed)
    Bp, nb, steps = 2, 5, 12
    n, G_ = Bp * nb, steps + 1
    anc = [[m] * G_ for m in range(n)]
    store = [[None] * G_ for _ in range(n)]  # the suffix: store[row][slot], written once, never moved
    hist = [[] for _ in range(n)]            # the expanded form: whole histories, gathered every step
    dup = dropped = 0
    for t in range(steps):
        kind = (seed + t) % 6
        if kind == 0:
            local = torch.arange(nb).repeat(Bp, 1)
        elif kind == 1:
            local = torch.randint(0, nb, (Bp, 1), generator=g).repeat(1, nb)
        else:
            local = torch.randint(0, nb, (Bp, nb), generator=g)
        beam_idx = (local + nb * torch.arange(Bp)[:, None]).reshape(-1).tolist()
        dup += len(set(beam_idx)) < n
        dropped += len(set(range(n)) - set(beam_idx)) > 0
        hist = [list(hist[src]) for src in beam_idx]
        anc = ancestry_step(anc, beam_idx, t)
        for m in range(n):  # the append of step t: every beam writes its new entry into its own row, slot t
            new = (t, m, int(torch.randint(0, 1 << 30, (1,), generator=g)))
            store[m][t] = new
            hist[m].append(new)
        for m in range(n):
            assert [store[anc[m][s]][s] for s in range(t + 1)] == hist[m], (t, m)
            assert all(a // nb == m // nb for a in anc[m][:t + 1])  # ancestry stays inside the prompt's group
    assert dup >= 6 and dropped >= 6
