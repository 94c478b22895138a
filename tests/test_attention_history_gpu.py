"""Attention results must not depend on what an EARLIER call left in scratch memory.

The attention backward keeps its delta / lse rows (ops._delta_ws) and the dS spill of its five-product form (ops._spill_ws) in cached
buffers, the split-K GEMMs their fp32 partials (ops._splitk_workspace), and the split-KV decode kernels merge per-split partials from a
workspace that ops allocates uninitialised.  Every other test starts from fresh or benign scratch.  Here a call runs after

  1. a backward of another length with the same padded length (S = 128, then S = 100: the same [2, B, H, 128] rows), dO scaled by 64;
  2. the same with dO = +inf on rows 100..127 only - the rows the S = 100 call pads with, left non-finite by the earlier call
     (an overflowed fp16 step the caller skipped); NaN arithmetic only;
  3. the cached buffer itself filled with 0xFF bytes (NaN as fp32 and as both 16-bit types) between two identical calls - for the
     delta / lse rows only rows < S: the pad rows are the contract's (include/merlin_hip.h, mh_attn_bwd2);
  4. a caller-owned decode workspace filled with zeros and then with NaN, on lengths [1, chunk, chunk + 1, Smax] that leave whole splits
     without keys;

and every "same result" is torch.equal.  No tolerance is stated in this file: the one bound used (decode outputs) is
N.limit(c_model) through hold()."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import numerics as N  # noqa: E402
from test_attention_structured_gpu import _grow  # noqa: E402
from test_componentwise_gpu import rnd  # noqa: E402
from test_kv8_cpu import kv8_dequantize, kv8_quantize  # noqa: E402
from test_kv8_gpu import hold, rnd_rows  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
B, H, S_SHORT, S_FULL = 1, 2, 100, 128
# (D, causal, fused-kv mode; None = the library's default): the two combinations the model runs, and the two-kernel dK / dV form at D = 128
BWD_FORMS = [(128, True, None), (128, True, 0), (64, False, None)]


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from merlin_amd import ops as O

    assert O.arch_ok(0), "not a gfx950 device"
    return O


class fused_kv:
    """with fused_kv(ops, mode): the dK|dV form of the block (None: leave the default), the default restored after it."""

    def __init__(self, ops, mode):
        from merlin_amd import _lib as L

        self.ops, self.mode, self.mode0 = ops, mode, int(L.lib().mh_attn_bwd_fused_kv_mode())

    def __enter__(self):
        if self.mode is not None:
            self.ops.attn_bwd_fused_kv(self.mode)

    def __exit__(self, *exc):
        self.ops.attn_bwd_fused_kv(self.mode0)


def _qkvdo(S, D, dtype, seed):
    qkv = rnd(B * S, 3 * H * D, dtype=dtype, seed=seed)
    return [qkv[:, i * H * D:(i + 1) * H * D] for i in range(3)] + [rnd(B * S, H * D, dtype=dtype, seed=seed + 9)]


def _backward(ops, q, k, v, do, S, D, causal, fwd=None):
    o, lse = fwd if fwd is not None else ops.attn_fwd2(q, k, v, B, S, H, D, causal)
    return ops.attn_bwd2(q, k, v, o, do, lse, B, S, H, D, causal)


def _same(got, want, what):
    for nm, g, w in zip(("dq", "dk", "dv"), got, want):
        assert bool(torch.isfinite(g.float()).all()), f"{what}: {nm} is not finite"
        assert torch.equal(g, w), f"{what}: {nm} differs from the run on fresh scratch"


def _after_history(ops, dtype, D, causal, mode, poison):
    """G0 = the S = 100 backward on fresh scratch; then, again from fresh scratch, a backward at S = 128 (the same S_pad) whose dO is
    scaled by 64 and set to `poison` on rows 100..127 where that is not None; then the S = 100 backward again."""
    with fused_kv(ops, mode):
        ops.release_attn_scratch()
        q, k, v, do = _qkvdo(S_SHORT, D, dtype, 1)
        fwd = ops.attn_fwd2(q, k, v, B, S_SHORT, H, D, causal)
        G0 = _backward(ops, q, k, v, do, S_SHORT, D, causal, fwd)
        assert all(bool(torch.isfinite(g.float()).all()) for g in G0)
        ops.release_attn_scratch()
        q1, k1, v1, do1 = _qkvdo(S_FULL, D, dtype, 2)
        do1 = (do1.float() * 64).to(dtype)
        if poison is not None:
            do1[S_SHORT:] = poison
        _backward(ops, q1, k1, v1, do1, S_FULL, D, causal)
        G1 = _backward(ops, q, k, v, do, S_SHORT, D, causal, fwd)
    return G0, G1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,causal,mode", BWD_FORMS)
def test_backward_after_a_longer_backward_of_the_same_padded_length(ops, dtype, D, causal, mode):
    G0, G1 = _after_history(ops, dtype, D, causal, mode, None)
    _same(G1, G0, f"S = {S_SHORT} after S = {S_FULL} with 64 x dO")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,causal,mode", BWD_FORMS)
def test_backward_after_a_backward_that_left_non_finite_rows(ops, dtype, D, causal, mode):
    """The S = 128 call has dO = +inf on rows 100..127, so its -delta there is inf or NaN; the S = 100 call pads its last tile with exactly
    those rows.  A masked row's dS = P x (dP - delta) is 0 x (non-finite) = NaN unless the rows read as zeros."""
    G0, G1 = _after_history(ops, dtype, D, causal, mode, float("inf"))
    _same(G1, G0, f"S = {S_SHORT} after S = {S_FULL} with dO = +inf on rows {S_SHORT}..{S_FULL - 1}")


def _fill_ff(t):
    t.view(torch.uint8).fill_(0xFF)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,causal,mode", BWD_FORMS)
def test_backward_with_poisoned_delta_rows(ops, dtype, D, causal, mode):
    """Rows < S of every cached delta / lse buffer hold 0xFF bytes before the second of two identical calls: the backward writes each of
    them before it reads it."""
    with fused_kv(ops, mode):
        ops.release_attn_scratch()  # (so that the one cached buffer is this call's: the pad rows of another shape's are not this test's to touch)
        q, k, v, do = _qkvdo(S_SHORT, D, dtype, 3)
        fwd = ops.attn_fwd2(q, k, v, B, S_SHORT, H, D, causal)
        G0 = _backward(ops, q, k, v, do, S_SHORT, D, causal, fwd)
        (ws,) = ops._delta_cache.values()
        assert ws.shape == (2, B, H, S_FULL)
        ws.view(torch.int32)[..., :S_SHORT].fill_(-1)  # 0xFF bytes
        assert bool(torch.isnan(ws[..., :S_SHORT]).all()) and bool((ws[..., S_SHORT:] == 0).all())
        G1 = _backward(ops, q, k, v, do, S_SHORT, D, causal, fwd)
    _same(G1, G0, "delta / lse rows < S poisoned")


@pytest.mark.parametrize("dtype", DTYPES)
def test_five_product_backward_with_poisoned_spill(ops, dtype):
    """The dS scratch of the five-product backward (S = 256: two 128-key blocks) holds 0xFF bytes before the second of two identical
    calls: the dQ pass reads only what the dK|dV kernel of the same call wrote."""
    S, D = 256, 128
    q, k, v, do = _qkvdo(S, D, dtype, 4)
    o, lse = ops.attn_fwd2(q, k, v, B, S, H, D, True)
    G0 = ops.attn_bwd2(q, k, v, o, do, lse, B, S, H, D, True, spill=True)
    assert ops.LAST_ATTN_BWD_FORM == "five-product" and ops._spill_cache
    for ws in ops._spill_cache.values():
        _fill_ff(ws)
    G1 = ops.attn_bwd2(q, k, v, o, do, lse, B, S, H, D, True, spill=True)
    assert ops.LAST_ATTN_BWD_FORM == "five-product"
    _same(G1, G0, "dS spill poisoned")


@pytest.mark.parametrize("dtype", DTYPES)
def test_split_k_gemms_with_poisoned_partials(ops, dtype, monkeypatch):
    """The fp32 partials of the split-K GEMMs (one cached buffer per stream) hold 0xFF bytes before the second of two identical calls:
    the weight gradient at (130, 512, 264) and (1731, 1024, 256) and the skinny product at (577, 1024, 4096), shapes of their own tests.
    mh_gemm_splitk_max gives (130, 512, 264) ONE split - no partials, the call must simply not care - and (1731, 1024, 256), the smallest
    shape of test_wgrad_split_k_per_element that splits, three."""
    from merlin_amd import _lib as L

    wgrads = []
    for T, No, Ki in [(130, 512, 264), (1731, 1024, 256)]:
        wgrads.append((No, Ki, rnd(T, No, dtype=dtype, scale=0.5), rnd(T, Ki, dtype=dtype, seed=1, scale=0.5)))
    assert int(L.lib().mh_gemm_splitk_max(1024, 256, 1731)) > 1
    M, Nn, K = 577, 1024, 4096
    assert int(L.lib().mh_gemm_splitk_max(M, Nn, K)) > 1
    monkeypatch.setattr(ops, "SKINNY_SPLITK", True)
    monkeypatch.setattr(ops, "SKINNY_SPLITK_ALL", True)  # (the default keeps fp16 on the one-pass order: ops._skinny_splitk_ok)
    a, b = rnd(M, K, dtype=dtype), rnd(Nn, K, dtype=dtype, seed=1, scale=0.5)
    bias, resid = rnd(Nn, dtype=dtype, seed=2), rnd(M, Nn, dtype=dtype, seed=3)

    def run():
        out = []
        for No, Ki, dy, x in wgrads:
            out.append(ops.wgrad_tn(dy, x, torch.empty(No, Ki, dtype=dtype, device=dev()), accum=False))
            out.append(ops.wgrad_tn(dy, x, torch.ones(No, Ki, device=dev()), accum=True))
        return out + [ops.gemm_nt(a, b), ops.gemm_nt(a, b, bias=bias, resid=resid)]

    first = run()
    assert ops._splitk_ws
    for ws in ops._splitk_ws.values():
        _fill_ff(ws)
    names = ("wgrad 130", "wgrad 130 fp32 accumulate", "wgrad 1731", "wgrad 1731 fp32 accumulate", "skinny gemm", "skinny gemm bias + resid")
    for nm, g, w in zip(names, run(), first):
        assert bool(torch.isfinite(g.float()).all()), nm
        assert torch.equal(g, w), f"{nm}: differs after the partials were poisoned"


# ---- the split-KV decode workspace ---------------------------------------------------------------------------------------------------------
def _with_both_workspaces(name, dtype, numel, launch, ref, Bc, mod):
    """launch(ws) -> out [rows, H, D] with a caller-owned workspace: zero-filled, then NaN-filled."""
    outs = []
    for fill in (0.0, float("nan")):
        ws = torch.full((numel,), fill, dtype=torch.float32, device=dev())
        outs.append(launch(ws))
        assert fill == 0.0 or not bool(torch.isnan(ws).all()), f"{name}: the launch did not use the workspace"
    assert bool(torch.isfinite(outs[1].float()).all()), f"{name}: not finite on a NaN-filled workspace"
    assert torch.equal(outs[0], outs[1]), f"{name}: the result depends on what the workspace held"
    hold(name, dtype, outs[0], ref, Bc, mod)


def _decode_refs(rows, dtype):
    """rows: (q [H, D], k64 [n, H, D], v64 [n, H, D]) -> (ref, B, model) stacked."""
    out = [N.attention_decode(q, k, v, k.shape[0]) + (N.attention_decode(q, k, v, k.shape[0], model=dtype),) for q, k, v in rows]
    return tuple(torch.stack([r[i] for r in out]) for i in range(3))


def _kv8_cache(Bn, Smax, Hn, D, dtype, seeds):
    """-> [k8, ks, k64, v8, vs, v64] on the device (the layouts of test_attn_decode_kv8_per_element)."""
    cache = []
    for seed in seeds:
        c8, cs = kv8_quantize(rnd_rows(Bn * Smax * Hn, D, dtype, seed=seed).view(Bn, Smax, Hn, D))
        cache += [c8.view(Bn, Smax, Hn * D).to(dev()), cs.permute(0, 2, 1).contiguous().to(dev()), kv8_dequantize(c8, cs).to(dev())]
    return cache


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_split_workspace_contents_do_not_matter(ops, dtype):
    """mh_attn_decode and mh_attn_decode_kv8 at the shape of their structured test (H = 2, D = 128, Smax raised to three splits), four
    sequences of 1, chunk, chunk + 1 and Smax keys: the first two leave the splits behind the first without a key."""
    from merlin_amd import _lib as L

    Bn, Hn, D = 4, 2, 128
    splits_of = lambda Smax: int(L.lib().mh_attn_decode_splits(Bn, Hn, Smax))  # noqa: E731
    Smax = _grow(splits_of, 40)
    splits = splits_of(Smax)
    chunk = (Smax + splits - 1) // splits
    lens = [1, chunk, chunk + 1, Smax]
    d = Hn * D
    q = rnd_rows(Bn * Hn, D, dtype, seed=5, lo=0.5, hi=2.0).view(Bn, d).to(dev())
    k8, ks, k64, v8, vs, v64 = _kv8_cache(Bn, Smax, Hn, D, dtype, (3, 4))
    k16, v16 = k64.to(dtype).view(Bn, Smax, d), v64.to(dtype).view(Bn, Smax, d)
    assert torch.equal(k16.double().view_as(k64), k64) and torch.equal(v16.double().view_as(v64), v64)
    ref, Bc, mod = _decode_refs([(q[b].view(Hn, D), k64[b, :lens[b]], v64[b, :lens[b]]) for b in range(Bn)], dtype)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev())
    numel = Bn * Hn * splits * (D + 2)
    tag = f"Smax={Smax} splits={splits} lens={lens}"

    def run16(ws):
        out = torch.empty(Bn, d, dtype=dtype, device=dev())
        L.call("mh_attn_decode", q, q.stride(0), k16, v16, out, lens_t, Bn, Hn, D, Smax, ws, ops.dt_of(q), ops._stream())
        return out.view(Bn, Hn, D)

    def run8(ws):
        out = torch.empty(Bn, d, dtype=dtype, device=dev())
        L.call("mh_attn_decode_kv8", q, q.stride(0), k8, v8, ks, vs, out, lens_t, Bn, Hn, D, Smax, ws, ops.dt_of(q), ops._stream())
        return out.view(Bn, Hn, D)

    _with_both_workspaces(f"attention decode 16-bit caller-owned workspace {tag}", dtype, numel, run16, ref, Bc, mod)
    _with_both_workspaces(f"attention decode kv8 caller-owned workspace {tag}", dtype, numel, run8, ref, Bc, mod)


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_multi_split_workspace_contents_do_not_matter(ops, dtype):
    """mh_attn_decode_multi (T = 5, H = 2, D = 128, Smax raised to three splits): query (b, t) sees lens[b] + t keys."""
    from merlin_amd import _lib as L

    Bn, T, Hn, D = 4, 5, 2, 128
    Smax = _grow(lambda s: ops.attn_decode_multi_splits(Bn, T, Hn, s), 40)
    splits = ops.attn_decode_multi_splits(Bn, T, Hn, Smax)
    chunk = (Smax + splits - 1) // splits
    lens = [1, chunk, chunk + 1, Smax - T + 1]
    d = Hn * D
    q = rnd(Bn * T, d, dtype=dtype, seed=5)
    kc, vc = rnd(Bn, Smax, d, dtype=dtype, seed=3), rnd(Bn, Smax, d, dtype=dtype, seed=4)
    k64, v64 = kc.double().view(Bn, Smax, Hn, D), vc.double().view(Bn, Smax, Hn, D)
    ref, Bc, mod = _decode_refs([(q[b * T + t].view(Hn, D), k64[b, :lens[b] + t], v64[b, :lens[b] + t]) for b in range(Bn) for t in range(T)], dtype)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev())

    def run(ws):
        out = torch.empty(Bn * T, d, dtype=dtype, device=dev())
        L.call("mh_attn_decode_multi", q, q.stride(0), kc, vc, out, lens_t, Bn, T, Hn, D, Smax, ws, ops.dt_of(q), ops._stream())
        return out.view(Bn * T, Hn, D)

    _with_both_workspaces(f"attention decode multi caller-owned workspace T={T} Smax={Smax} splits={splits} lens={lens}", dtype,
                          Bn * T * Hn * splits * (D + 2), run, ref, Bc, mod)


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_beams_split_workspace_contents_do_not_matter(ops, dtype):
    """mh_attn_decode_beams at the shape of its structured test (5 beams, H = 4, D = 64, G = 16, Pmax raised to three prefix splits), four
    prompts of 1, chunk, chunk + 1 and Pmax keys; suffix key g of beam m lies in row anc[m, g] of its prompt's beams."""
    from merlin_amd import _lib as L

    Bp, nb, Hn, D, G, gen = 4, 5, 4, 64, 16, 15
    Pmax = _grow(lambda s: ops.attn_decode_beams_splits(Bp, nb, Hn, s, G)[0], 40)
    psplits, ssplits = ops.attn_decode_beams_splits(Bp, nb, Hn, Pmax, G)
    chunk = (Pmax + psplits - 1) // psplits
    pre_lens, sl, n, d = [1, chunk, chunk + 1, Pmax], gen + 1, Bp * nb, Hn * D
    g = torch.Generator().manual_seed(17)
    anc = (torch.randint(0, nb, (Bp, nb, G), generator=g) + nb * torch.arange(Bp)[:, None, None]).view(n, G).to(torch.int32)
    anc[:, gen] = torch.arange(n, dtype=torch.int32)  # the new key is the beam's own
    q = rnd(n, d, dtype=dtype, seed=5)
    pk, pv = rnd(Bp, Pmax, d, dtype=dtype, seed=3), rnd(Bp, Pmax, d, dtype=dtype, seed=4)
    sk, sv = rnd(n, G, d, dtype=dtype, seed=8), rnd(n, G, d, dtype=dtype, seed=9)
    rows, ar = [], torch.arange(sl, device=dev())
    for m in range(n):
        p, pick = m // nb, anc[m, :sl].long().to(dev())
        kk = torch.cat([pk[p, :pre_lens[p]], sk[pick, ar]]).double().view(-1, Hn, D)
        vv = torch.cat([pv[p, :pre_lens[p]], sv[pick, ar]]).double().view(-1, Hn, D)
        rows.append((q[m].view(Hn, D), kk, vv))
    ref, Bc, mod = _decode_refs(rows, dtype)
    pl_t = torch.tensor(pre_lens, dtype=torch.int32, device=dev())
    slens = torch.full((n,), sl, dtype=torch.int32, device=dev())
    anc_d = anc.to(dev())

    def run(ws):
        out = torch.empty(n, d, dtype=dtype, device=dev())
        L.call("mh_attn_decode_beams", q, q.stride(0), pk, pv, pl_t, sk, sv, anc_d, slens, out, Bp, nb, Hn, D, Pmax, G, ws, ops.dt_of(q), ops._stream())
        return out.view(n, Hn, D)

    _with_both_workspaces(f"attention decode beams caller-owned workspace Pmax={Pmax} pre_lens={pre_lens} splits={psplits}+{ssplits}", dtype,
                          n * Hn * (max(psplits, 1) + ssplits) * (D + 2), run, ref, Bc, mod)
