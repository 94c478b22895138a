"""Sessions for generate() on the host: the prefix decision (generation._reusable_prefix, a pure function of token ids, image spans and
image tensors), the refusals generate(session=...) raises before it touches the model, and `session` as a named parameter."""
import pytest
import torch

from merlin_amd import generation as G

START, PATCH, END = 101, 100, 102


def _img(seed):
    return torch.randn(3, 8, 8, generator=torch.Generator().manual_seed(seed))


def _prompt(*parts):
    """Token ids from parts: an int list is text, "img" a 6-token image span."""
    ids = []
    for p in parts:
        ids += [START] + [PATCH] * 4 + [END] if p == "img" else list(p)
    return ids


def _keep(cached, cached_images, new, new_images):
    sp = lambda ids: G._image_spans(ids, START, END)  # noqa: E731
    return G._reusable_prefix(cached, sp(cached), cached_images, new, sp(new), new_images)


def test_image_spans():
    ids = _prompt([1, 5], "img", [7], "img", [9])
    assert G._image_spans(ids, START, END) == [(2, 8), (9, 15)]
    assert G._image_spans([1, START, PATCH], START, END) == []  # an open span is none
    assert G._image_spans(ids, None, None) == []


def test_reusable_prefix_cases():
    a, b = _img(1), _img(2)
    text = [1, 5, 6, 7, 8, 9, 10, 11]
    # identical prompt: all but the last position (its logits select the first new token)
    assert _keep(text, [], text, []) == len(text) - 1
    p = _prompt([1, 5], "img", [7, 8, 9])
    assert _keep(p, [a], p, [a.clone()]) == len(p) - 1
    # divergence in text, before and behind an image
    assert _keep(text, [], text[:5] + [50, 51, 52], []) == 5
    assert _keep(p, [a], p[:9] + [60, 61], [a]) == 9
    assert _keep(p, [a], [1, 6] + p[2:], [a]) == 1
    # a longer prompt on a shorter cache: the whole cache
    assert _keep(text, [], text + [3, 4], []) == len(text)
    # divergence inside an image span: back to the span's start
    cut = list(p)
    cut[5] = 77
    assert _keep(p, [a], cut, [a]) == 2
    # a prefix that ends inside a span (the cache was cut there, or the cap len - 1 falls on <im_end>): the span's start
    assert _keep(p[:6], [a], p, [a]) == 2
    q = _prompt([1, 5], "img")
    assert _keep(q, [a], q, [a]) == 2
    # same ids, one pixel changed in the second of two images: the start of that span; in the first: the start of the first
    two = _prompt([1], "img", [7, 8], "img", [9, 3])
    b2 = b.clone()
    b2[1, 2, 3] += 1.0
    assert G._image_spans(two, START, END) == [(1, 7), (9, 15)]
    assert _keep(two, [a, b], two, [a, b2]) == 9
    a2 = a.clone()
    a2[0, 0, 0] -= 0.5
    assert _keep(two, [a, b], two, [a2, b]) == 1
    assert _keep(two, [a, b], two, [a, b.clone()]) == len(two) - 1
    # equal values in another shape are another image; a missing image is one too
    assert _keep(two, [a, b], two, [a, b.reshape(3, 4, 16)]) == 9
    assert _keep(two, [a, b], two, [a]) == 9
    # new prompt shorter than the cache
    assert _keep(text, [], text[:4], []) == 3
    assert _keep(two, [a, b], two[:9], [a]) == 8
    # empty session; a one-token prompt
    assert _keep([], [], text, []) == 0
    assert _keep([], [], two, [a, b]) == 0
    assert _keep(text, [], text[:1], []) == 0


class _NoDevice:
    """A model whose every attribute is an error: the refusals must be raised before generate() looks at it."""

    def __getattr__(self, name):
        raise AssertionError(f"generate() touched model.{name} before refusing")


def test_session_refusals_come_before_device_work():
    ids = torch.ones(1, 4, dtype=torch.int64)
    s = G.Session(_NoDevice(), capacity=64)
    s8 = G.Session(_NoDevice(), capacity=64, fp8_kv=True)
    assert s.tokens == [] and s.cache is None and s.capacity == 64 and not s.fp8_kv and s8.fp8_kv
    assert s.last == dict(reused_tokens=0, run_tokens=0, images_encoded=0)
    with pytest.raises(ValueError, match="batch_size = 2"):
        G.generate(_NoDevice(), torch.ones(2, 4, dtype=torch.int64), session=s, max_new_tokens=4)
    with pytest.raises(ValueError, match="attention_mask"):
        G.generate(_NoDevice(), ids, attention_mask=torch.tensor([[0, 1, 1, 1]]), session=s, max_new_tokens=4)
    with pytest.raises(ValueError, match="use_cache"):
        G.generate(_NoDevice(), ids, use_cache=False, session=s, max_new_tokens=4)
    with pytest.raises(ValueError, match="fp8_kv"):
        G.generate(_NoDevice(), ids, fp8_kv=True, session=s, max_new_tokens=4)
    with pytest.raises(ValueError, match="fp8_kv"):
        G.generate(_NoDevice(), ids, session=s8, max_new_tokens=4)
    for mode in (dict(num_beams=3), dict(num_beams=3, share_prompt_kv=True), dict(prompt_lookup_num_tokens=4), dict(do_sample=True)):
        with pytest.raises(ValueError, match="session"):
            G.generate(_NoDevice(), torch.ones(2, 4, dtype=torch.int64), session=s, max_new_tokens=4, **mode)
    with pytest.raises(ValueError, match="capacity"):
        G.Session(_NoDevice(), capacity=0)
    s.reset()  # an empty session resets without a cache
    assert s.tokens == [] and s.spans == [] and s.images == []


def test_session_is_a_named_parameter_not_an_option():
    import inspect

    assert inspect.signature(G.generate).parameters["session"].default is None
    assert "session" not in G._DEFAULTS and "session" not in G._NEUTRAL
    with pytest.raises(TypeError):
        G._resolve_options(None, dict(session=None))
    with pytest.raises(TypeError):
        G._resolve_options(None, dict(sessions=1))
    with pytest.raises(TypeError):
        G.generate(_NoDevice(), torch.ones(1, 4, dtype=torch.int64), sesion=None)
