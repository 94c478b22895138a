"""MXFP4 weights for the prompt, the host side (no GPU): the ABI of mh_gemm_fp4w, generate(fp4_prefill=True)'s refusal before any device work,
and the session's bookkeeping of the weight format that wrote its rows, on a fake engine."""
import inspect
import os

import pytest
import torch


def test_header_declares_and_library_exports_the_gemm():
    from merlin_amd import _lib as L
    from merlin_amd.csrc import build

    assert "mh_gemm_fp4w" in L.declared_symbols() and "gemm_fp4w.hip" in build.SOURCES
    restype, argtypes = L.PROTOTYPES["mh_gemm_fp4w"]
    assert restype is L.C.c_int and len(argtypes) == 15 and argtypes[-1] is L.DevPtr
    assert [a is L.DevPtr for a in argtypes[:8]] == [True, False, True, True, True, False, True, False]
    if not os.path.exists(L.LIB_PATH):
        build.build(verbose=False)
    assert hasattr(L.lib(), "mh_gemm_fp4w")


def test_generate_refuses_fp4_prefill_without_fp4_weights_before_touching_the_model():
    from merlin_amd import generation as G

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"model.{name} read before the arguments were checked")

    ids = torch.zeros(1, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="fp4_prefill.*fp4_weights"):
        G.generate(Untouchable(), ids, fp4_prefill=True, max_new_tokens=2)
    with pytest.raises(ValueError, match="fp4_prefill.*fp4_weights"):
        G.generate(Untouchable(), ids, fp4_prefill=True, fp8_weights=True, max_new_tokens=2)
    # a named parameter next to fp4_weights, not an entry of the option tables
    sig = inspect.signature(G.generate).parameters
    assert sig["fp4_prefill"].default is False and sig["fp4_weights"].default is False
    assert "fp4_prefill" not in G._DEFAULTS and "fp4_prefill" not in G._NEUTRAL


class _Cache:
    def __init__(self, Smax):
        self.Smax, self.n = Smax, 0

    def truncate(self, n):
        self.n = n


class _Engine:
    """Records which entry point ran, on how many tokens and with which weight format."""

    def __init__(self):
        self.calls = []

    def new_cache(self, B, Smax, fp8=False):
        return _Cache(Smax)

    def prefill(self, input_ids, attention_mask, images, max_new_tokens, kv_fp8=False, cache=None, w_fp4=False):
        self.calls.append(("prefill", int(input_ids.shape[1]), bool(w_fp4)))
        cache.n = int(input_ids.shape[1])
        return torch.zeros(1, 8), cache

    def extend(self, cache, input_ids, images=None, pos=None, w_fp4=False):
        assert pos == cache.n
        self.calls.append(("extend", int(input_ids.shape[1]), bool(w_fp4)))
        cache.n += int(input_ids.shape[1])
        return torch.zeros(1, 8)


class _Model:
    class config:
        max_position_embeddings = 64

    def __init__(self):
        self.engine = _Engine()


def test_session_remembers_the_weight_format_of_its_rows():
    from merlin_amd.generation import Session

    assert list(inspect.signature(Session.__init__).parameters) == ["self", "model", "capacity", "fp8_kv"]
    assert inspect.signature(Session._prefill).parameters["w_fp4"].default is False
    m = _Model()
    s = Session(m)
    assert s.w_fp4 is False
    a = torch.arange(1, 11)[None]
    b = torch.cat([a, torch.tensor([[20, 21, 22]])], dim=1)
    s._prefill(a, None, 4)                      # 16-bit rows
    assert m.engine.calls[-1] == ("prefill", 10, False) and s.last["reused_tokens"] == 0 and s.w_fp4 is False
    s._prefill(b, None, 4)                      # same format: the prefix is reused
    assert m.engine.calls[-1] == ("extend", 3, False) and s.last == dict(reused_tokens=10, run_tokens=3, images_encoded=0)
    s._prefill(b, None, 4, w_fp4=True)          # the other format: nothing is reused, a full prefill on the fp4 copies
    assert m.engine.calls[-1] == ("prefill", 13, True) and s.last == dict(reused_tokens=0, run_tokens=13, images_encoded=0) and s.w_fp4 is True
    c = torch.cat([b, torch.tensor([[30, 31]])], dim=1)
    s._prefill(c, None, 4, w_fp4=True)          # fp4 again: reuse, and the extension runs on the fp4 copies too
    assert m.engine.calls[-1] == ("extend", 2, True) and s.last["reused_tokens"] == 13
    s._prefill(c, None, 4)                      # back to 16-bit (e.g. model.score on this session): a full prefill again
    assert m.engine.calls[-1] == ("prefill", 15, False) and s.last["reused_tokens"] == 0 and s.w_fp4 is False
    s._prefill(c, None, 4, w_fp4=True)
    s.reset()
    assert s.w_fp4 is False and s.tokens == []
