"""model.score() on the host: the packed-row plan (scoring._branch_plan, a pure function of the candidates' token ids), the refusals
score() raises before it touches the engine, and score's arguments staying out of generate()'s option tables."""
import inspect

import pytest
import torch

from merlin_amd import generation as G
from merlin_amd import scoring as S

START, PATCH, END = 101, 100, 102


def _lists(plan):
    return dict(fed=list(plan.fed), seg_start=plan.seg_start.tolist(), rel_pos=plan.rel_pos.tolist(), targets=plan.targets.tolist(),
                first_targets=plan.first_targets.tolist(), offsets=list(plan.offsets))


PLANS = [
    # a single one-token candidate: no row at all
    ([[7]], dict(fed=[], seg_start=[], rel_pos=[], targets=[], first_targets=[7], offsets=[0, 0])),
    # mixed lengths [1, 4, 1, 2]: the one-token candidates own empty row ranges between the others
    ([[11], [21, 22, 23, 24], [31], [41, 42]],
     dict(fed=[21, 22, 23, 41], seg_start=[0, 0, 0, 3], rel_pos=[0, 1, 2, 0], targets=[22, 23, 24, 42], first_targets=[11, 21, 31, 41],
          offsets=[0, 0, 3, 3, 4])),
    # one long candidate: one segment from row 0, the last token never fed
    ([[5, 6, 7, 8, 9, 10, 11]],
     dict(fed=[5, 6, 7, 8, 9, 10], seg_start=[0] * 6, rel_pos=[0, 1, 2, 3, 4, 5], targets=[6, 7, 8, 9, 10, 11], first_targets=[5], offsets=[0, 6])),
]


@pytest.mark.parametrize("conts,want", PLANS, ids=["one_token", "mixed_1_4_1_2", "one_long"])
def test_branch_plan_against_a_literal_expectation(conts, want):
    plan = S._branch_plan(conts)
    assert _lists(plan) == want
    assert plan.seg_start.dtype == plan.rel_pos.dtype == torch.int32 and plan.targets.dtype == plan.first_targets.dtype == torch.int64
    R = len(plan.fed)
    assert R == sum(len(c) - 1 for c in conts) == plan.offsets[-1] and len(plan.offsets) == len(conts) + 1
    seg = plan.seg_start.tolist()
    assert all(seg[r] <= r for r in range(R)) and seg == sorted(seg)
    for c, cand in enumerate(conts):  # the rows map back to their candidate: fed = all but its last token, targets = all but its first
        a, b = plan.offsets[c], plan.offsets[c + 1]
        assert plan.fed[a:b] == cand[:-1] and plan.targets.tolist()[a:b] == cand[1:]
        assert seg[a:b] == [a] * (b - a) and plan.rel_pos.tolist()[a:b] == list(range(b - a))


def test_token_lists_accept_lists_tuples_and_tensors():
    assert S._token_lists([[1, 2], (3,), torch.tensor([4, 5, 6])]) == [[1, 2], [3], [4, 5, 6]]


class _NoDevice:
    """A model whose every attribute is an error: the refusals must be raised before score() looks at it."""

    def __getattr__(self, name):
        raise AssertionError(f"score() touched model.{name} before refusing")


class _TokensOnly(_NoDevice):
    """The three image token ids and nothing else: what the text-only check of the continuations may read."""
    im_start_token, im_patch_token, im_end_token = START, PATCH, END


def test_score_refusals_come_before_device_work():
    ids = torch.ones(1, 4, dtype=torch.int64)
    m = _NoDevice()
    with pytest.raises(ValueError, match="non-empty list"):
        S.score(m, ids, [])
    with pytest.raises(ValueError, match="continuation 1 is empty"):
        S.score(m, ids, [[5], []])
    with pytest.raises(ValueError, match="continuation 0 is empty"):
        S.score(m, ids, [torch.zeros(0, dtype=torch.int64)])
    with pytest.raises(ValueError, match="batch_size = 2"):
        S.score(m, torch.ones(2, 4, dtype=torch.int64), [[5, 6]])
    with pytest.raises(ValueError, match="attention_mask"):
        S.score(m, ids, [[5, 6]], attention_mask=torch.tensor([[0, 1, 1, 1]]))
    s = G.Session(m, capacity=64)
    s8 = G.Session(m, capacity=64, fp8_kv=True)
    with pytest.raises(ValueError, match="session: fp8_kv=True but the session's cache was made with fp8_kv=False"):
        S.score(m, ids, [[5, 6]], fp8_kv=True, session=s)
    with pytest.raises(ValueError, match="session: fp8_kv=False but the session's cache was made with fp8_kv=True"):
        S.score(m, ids, [[5, 6]], session=s8)
    assert s.cache is None and s.tokens == [] and s8.cache is None
    t = _TokensOnly()
    for tok, name in ((START, "im_start_token"), (PATCH, "im_patch_token"), (END, "im_end_token")):
        with pytest.raises(ValueError, match=f"continuation 1 contains the image token id {tok} .{name}.: continuations are text only"):
            S.score(t, ids, [[5, 6], [7, tok, 8]])
    with pytest.raises(ValueError, match="image token id"):
        S.score(t, ids, [torch.tensor([PATCH])], session=G.Session(t, capacity=64))


def test_score_is_an_entry_point_not_a_generate_option():
    prm = inspect.signature(S.score).parameters
    assert list(prm)[:6] == ["model", "input_ids", "continuations", "images", "fp8_kv", "session"]
    assert prm["images"].default is None and prm["fp8_kv"].default is False and prm["session"].default is None
    for name in ("continuations", "score", "candidates"):
        assert name not in G._DEFAULTS and name not in G._NEUTRAL
        with pytest.raises(TypeError):
            G._resolve_options(None, {name: None})
    from merlin_amd.model.llama_mmgpt import MMGPTLlamaForCausalLM

    mp = inspect.signature(MMGPTLlamaForCausalLM.score).parameters
    assert list(mp)[:6] == ["self", "input_ids", "continuations", "images", "fp8_kv", "session"]
    assert {f.name for f in S.ScoreOutput.__dataclass_fields__.values()} == {"token_logprobs", "logprobs", "is_greedy", "stats"}


def test_model_score_names_its_arguments():
    """A misspelt keyword fails at the model's method: it takes no **kwargs."""
    from merlin_amd.model.llama_mmgpt import MMGPTLlamaForCausalLM

    prm = inspect.signature(MMGPTLlamaForCausalLM.score).parameters
    assert list(prm) == ["self", "input_ids", "continuations", "images", "fp8_kv", "session", "attention_mask"]
    assert all(p.kind is not inspect.Parameter.VAR_KEYWORD for p in prm.values()) and prm["attention_mask"].default is None
