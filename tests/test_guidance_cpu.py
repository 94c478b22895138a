"""Classifier-free guidance of generate(), host side: option resolution and the refusals (before any device work), generation._guided_ref
against transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor driven by a stub model with canned logits, and the
unconditional-context helper.  `canned` / `hf_guided` are shared with tests/test_guidance_gpu.py."""
import pytest
import torch

V_SMALL = 40


def canned(context, V=V_SMALL):
    """Logits fp32 [V] that depend on the whole context (a list of ints) and on nothing else."""
    seed = 17
    for t in context:
        seed = (seed * 1000003 + int(t) + 1) % (2 ** 31 - 1)
    return torch.randn(V, generator=torch.Generator().manual_seed(seed)) * 3


class StubModel:
    """What the processor needs of a model: called with the tokens it has not seen yet and the `past_key_values` it returned last time
    (here: the list of tokens seen so far), it answers with canned logits for the whole context at the last position."""

    def __init__(self):
        self.calls = []

    def __call__(self, input_ids, attention_mask=None, use_cache=True, past_key_values=None):
        ctx = list(past_key_values or []) + [int(t) for t in input_ids[0].tolist()]
        assert attention_mask.shape == (1, len(ctx)) and bool(attention_mask.all())
        self.calls.append(ctx)
        logits = torch.zeros(1, input_ids.shape[1], V_SMALL)
        logits[0, -1] = canned(ctx)
        return _Out(logits, ctx)


class _Out:
    def __init__(self, logits, past):
        self.logits, self._past = logits, past

    def get(self, key, default=None):
        return self._past if key == "past_key_values" else default


def hf_guided(g, cond_rows, prompt, new, negative):
    """transformers' processor over len(cond_rows) steps: step t sees input_ids = prompt + new[:t] and the conditional logits cond_rows[t];
    -> (its scores per step, the contexts the stub model was asked for)."""
    from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor as CFG

    stub = StubModel()
    proc = CFG(g, stub, unconditional_ids=None if negative is None else torch.tensor([negative]), use_cache=True)
    out = []
    for t, row in enumerate(cond_rows):
        ids = torch.tensor([list(prompt) + list(new[:t])], dtype=torch.int64)
        out.append(proc(ids, row[None].clone())[0])
    return out, stub.calls


class NoDevice:  # generate() refuses before it touches the model
    def __getattr__(self, name):
        raise AssertionError(f"device work before validation: {name}")


def test_guidance_scale_resolution_none_and_one_are_off_keywords_win():
    from transformers import GenerationConfig

    from merlin_amd.generation import _NEUTRAL, _resolve_guidance, _resolve_options

    ids = torch.zeros(1, 5, dtype=torch.int64)
    for kw in (dict(), dict(guidance_scale=None), dict(guidance_scale=1), dict(guidance_scale=1.0)):
        o = _resolve_options(None, dict(kw))
        assert o["guidance_scale"] is None and _resolve_guidance(o, None, None, ids, None) is None
    for g in (0.0, 0.5, 1.5, 3, -1.0):  # transformers does not restrict it to > 1
        o = _resolve_options(None, dict(guidance_scale=g))
        assert o["guidance_scale"] == float(g) and isinstance(o["guidance_scale"], float)
        assert _resolve_guidance(o, None, None, ids, None) == dict(scale=float(g), ids=None, images=None)
    assert _resolve_options(GenerationConfig(guidance_scale=2.0), {})["guidance_scale"] == 2.0
    assert _resolve_options(GenerationConfig(guidance_scale=2.0), dict(guidance_scale=1.5))["guidance_scale"] == 1.5
    assert _resolve_options(GenerationConfig(guidance_scale=2.0), dict(guidance_scale=1))["guidance_scale"] is None
    for k in ("guidance_scale", "negative_prompt_ids", "negative_prompt_attention_mask"):
        assert k not in _NEUTRAL
    neg = torch.tensor([[4, 5, 6]])
    images = [torch.zeros(1, 3, 4, 4)]
    o = _resolve_options(None, dict(guidance_scale=2.0, negative_prompt_ids=neg, negative_prompt_attention_mask=torch.ones(1, 3, dtype=torch.int64)))
    got = _resolve_guidance(o, images, None, ids, torch.ones(1, 5, dtype=torch.int64))
    assert got["scale"] == 2.0 and got["ids"] is neg and got["images"] is images


IDS = torch.zeros(1, 5, dtype=torch.int64)
NEG = torch.tensor([[4, 5, 6]])
REFUSED = [
    # (keywords of generate(), input_ids, the name the message carries)
    (dict(guidance_scale=True), None, "guidance_scale"),
    (dict(guidance_scale="2"), None, "guidance_scale"),
    (dict(guidance_scale=float("nan")), None, "guidance_scale"),
    (dict(guidance_scale=[2.0]), None, "guidance_scale"),
    (dict(negative_prompt_ids=NEG), None, "negative_prompt_ids"),                           # guidance off: nothing is silently dropped
    (dict(negative_prompt_ids=NEG, guidance_scale=1.0), None, "negative_prompt_ids"),
    (dict(negative_images=[torch.zeros(1, 3, 4, 4)]), None, "negative_images"),
    (dict(negative_prompt_attention_mask=torch.ones(1, 3)), None, "negative_prompt_attention_mask"),
    (dict(guidance_scale=2.0, num_beams=3), None, "num_beams"),
    (dict(guidance_scale=2.0, session=object()), None, "session"),
    (dict(guidance_scale=2.0, prompt_lookup_num_tokens=8), IDS, "prompt_lookup_num_tokens"),
    (dict(guidance_scale=2.0), torch.zeros(2, 5, dtype=torch.int64), "batch_size"),
    (dict(guidance_scale=2.0, attention_mask=torch.tensor([[0, 1, 1, 1, 1]])), IDS, "attention_mask"),
    (dict(guidance_scale=2.0, negative_prompt_ids=NEG, negative_prompt_attention_mask=torch.tensor([[0, 1, 1]])), IDS, "negative_prompt_attention_mask"),
    (dict(guidance_scale=2.0, negative_prompt_ids=NEG, negative_prompt_attention_mask=torch.ones(1, 4)), IDS, "negative_prompt_attention_mask"),
    (dict(guidance_scale=2.0, negative_prompt_ids=torch.tensor([4, 5, 6])), IDS, "negative_prompt_ids"),
    (dict(guidance_scale=2.0, negative_prompt_ids=torch.zeros(2, 3, dtype=torch.int64)), IDS, "negative_prompt_ids"),
    (dict(guidance_scale=2.0, negative_prompt_ids=[[4, 5, 6]]), IDS, "negative_prompt_ids"),
    (dict(guidance_scale=2.0, negative_images=[torch.zeros(1, 3, 4, 4)]), IDS, "negative_images"),  # images without a negative prompt
    (dict(guidance_scale=2.0, negative_prompt_attention_mask=torch.ones(1, 1)), IDS, "negative_prompt_attention_mask"),
]


@pytest.mark.parametrize("i", range(len(REFUSED)))
def test_refusals_carry_the_options_name_and_come_before_device_work(i):
    from merlin_amd import generation as G

    kw, ids, name = REFUSED[i]
    with pytest.raises(ValueError, match=name):
        G.generate(NoDevice(), NoDevice() if ids is None else ids, **kw)


def test_guidance_combines_with_the_options_it_is_documented_with():
    """Nothing here is refused: lookup up to 7, sampling with the warpers, the bans, use_cache=False."""
    from merlin_amd.generation import _resolve_guidance, _resolve_options

    for kw in (dict(prompt_lookup_num_tokens=7), dict(prompt_lookup_num_tokens=1), dict(do_sample=True, min_p=0.1, epsilon_cutoff=1e-3),
               dict(no_repeat_ngram_size=3, bad_words_ids=[[5]]), dict(use_cache=False)):
        o = _resolve_options(None, dict(guidance_scale=1.5, negative_prompt_ids=NEG, **kw))
        assert _resolve_guidance(o, None, None, IDS, None)["scale"] == 1.5


@pytest.mark.parametrize("g", [0.5, 1.5, 3.0])
@pytest.mark.parametrize("negative", [[7, 8, 9, 3], None], ids=["given", "default_last_token"])
def test_guided_ref_equals_transformers_processor_over_three_steps(g, negative):
    """The processor caches the unconditional context (its past_key_values) and feeds only the last token from the second step on: the
    contexts the stub saw are the helper's, and the scores are _guided_ref's on the same canned rows."""
    from merlin_amd.generation import _guided_ref, _uncond_context

    prompt, new = [1, 30, 31, 12], [21, 5, 17]
    cond_rows = [canned(prompt + new[:t]) + 0.5 for t in range(3)]
    want, asked = hf_guided(g, cond_rows, prompt, new, negative)
    for t in range(3):
        ctx = _uncond_context(negative, prompt, new[:t])
        assert asked[t] == ctx
        got = _guided_ref(cond_rows[t], canned(ctx), g)
        assert got.dtype == torch.float32 and torch.equal(got, want[t]), (g, t, float((got - want[t]).abs().max()))
        # and in float64: the form the GPU tests evaluate
        got64 = _guided_ref(cond_rows[t].double(), canned(ctx).double(), g)
        assert float((got64 - want[t].double()).abs().max()) < 1e-4


def test_uncond_context_is_the_negative_prompt_plus_every_generated_token():
    from merlin_amd.generation import _uncond_context

    prompt = [1, 30, 31, 12]
    assert _uncond_context([7, 8], prompt, []) == [7, 8]
    assert _uncond_context([7, 8], prompt, [21]) == [7, 8, 21]
    assert _uncond_context(torch.tensor([7, 8]), torch.tensor(prompt), torch.tensor([21, 5, 17])) == [7, 8, 21, 5, 17]
    assert _uncond_context(None, prompt, []) == [12]                 # transformers' default: the prompt's last token alone
    assert _uncond_context(None, prompt, [21, 5]) == [12, 21, 5]
    assert all(isinstance(t, int) for t in _uncond_context(torch.tensor([7]), prompt, torch.tensor([3])))


def test_guided_ref_identities():
    from merlin_amd.generation import _guided_ref

    x, y = canned([1]).double(), canned([2]).double()
    for g in (0.5, 1.5, 3.0):
        assert float((_guided_ref(x, x, g) - torch.log_softmax(x, -1)).abs().max()) < 1e-12
    assert float((_guided_ref(x, y, 1.0) - torch.log_softmax(x, -1)).abs().max()) < 1e-12
    assert float((_guided_ref(x, y, 0.0) - torch.log_softmax(y, -1)).abs().max()) < 1e-12
