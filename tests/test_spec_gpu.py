"""Prompt-lookup speculative decoding on the GPU: the multi-token append kernels against T calls of the single-token ones (bit for bit),
the multi-query decode attention per element against the fp64 reference and its rounding model (tests/numerics.py, the rule of
tests/test_kv8_gpu.py), the drafter kernel against generation._prompt_lookup, engine.verify_step against sequential decode steps with a
bound measured in the same run, and generate(prompt_lookup_num_tokens=k) against the goldens and the plain path."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import numerics as N  # noqa: E402
from test_kv8_cpu import kv8_dequantize, kv8_quantize  # noqa: E402
from test_kv8_gpu import _dev, _tiny, hold, rnd_rows, same_fp8  # noqa: E402
from test_spec_cpu import lookup_cases  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def O():
    from merlin_amd import ops

    assert ops.arch_ok(0), "not a gfx950 device"
    return ops


# ---- append, multi-token ---------------------------------------------------------------------------------------------------------------
# (B, T, H, D, Smax, pos, rope shift): one block; rope_pos != pos; the last rows of the cache
APPEND_CASES = [(2, 3, 2, 128, 40, [5, 20], 0), (3, 5, 4, 64, 700, [0, 333, 695], 3), (1, 16, 4, 64, 64, [48], 0)]
FILL16, FILL8, FILLS = 0.3125, 0x2B, 7.0


def _caches(B, Smax, H, D, dtype, guard=1):
    """Patterned 16-bit and fp8 caches of B sequences, carved out of buffers with `guard` more sequences behind them."""
    d = H * D
    k16, v16 = (torch.full((B + guard, Smax, d), FILL16, dtype=dtype, device=dev()) for _ in range(2))
    k8, v8 = (torch.full((B + guard, Smax, d), FILL8, dtype=torch.uint8, device=dev()) for _ in range(2))
    ks, vs = (torch.full((B + guard, H, Smax), FILLS, device=dev()) for _ in range(2))
    return [k16, v16], [k8, v8, ks, vs]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,H,D,Smax,pos,shift", APPEND_CASES)
def test_append_multi_equals_T_single_token_calls(O, dtype, B, T, H, D, Smax, pos, shift):
    """Rotated qkv, caches and scales are torch.equal to T calls of mh_decode_rope_append / _kv8 at pos + t (rope_pos + t), and every cache
    row outside [pos, pos + T) keeps its patterned fill - both cache formats."""
    d = H * D
    qkv0 = rnd_rows(B * T * 3 * H, D, dtype, seed=7).view(B * T, 3 * d).to(dev())
    pos_t = torch.tensor(pos, dtype=torch.int32, device=dev())
    rpos = (pos_t + shift) if shift else None
    tab = O.rope_table(Smax + 8, D, 10000.0, dev())
    ref16, ref8 = _caches(B, Smax, H, D, dtype)
    got16, got8 = _caches(B, Smax, H, D, dtype)
    want = [torch.empty_like(qkv0).view(B, T, 3 * d) for _ in range(2)]
    for t in range(T):
        rp = None if rpos is None else rpos + t
        for fmt, (ref, fn) in enumerate(((ref16, O.decode_rope_append), (ref8, O.decode_rope_append_kv8))):
            rows = qkv0.view(B, T, 3 * d)[:, t].clone()  # (a copy: at B = 1 the slice is contiguous as it lies)
            fn(rows, tab, pos_t + t, *[c[:B] for c in ref], H, D, rope_pos=rp)
            want[fmt][:, t] = rows
    q16, q8 = qkv0.clone(), qkv0.clone()
    O.decode_rope_append_multi(q16, tab, pos_t, *[c[:B] for c in got16], T, H, D, rope_pos=rpos)
    O.decode_rope_append_multi_kv8(q8, tab, pos_t, *[c[:B] for c in got8], T, H, D, rope_pos=rpos)
    assert torch.equal(q16.view(B, T, 3 * d), want[0]) and torch.equal(q8.view(B, T, 3 * d), want[1]) and torch.equal(q16, q8)
    assert not torch.equal(q16[:, :2 * d], qkv0[:, :2 * d]) and torch.equal(q16[:, 2 * d:], qkv0[:, 2 * d:])
    for g, r in zip(got16, ref16):
        assert torch.equal(g, r)
    for g, r in zip(got8[:2], ref8[:2]):
        assert same_fp8(g.cpu(), r.cpu())
    for g, r in zip(got8[2:], ref8[2:]):
        assert torch.equal(g, r)
    keep = torch.ones(B + 1, Smax, dtype=torch.bool, device=dev())
    for b in range(B):
        keep[b, pos[b]:pos[b] + T] = False
    for c in got16:
        assert bool((c[keep] == FILL16).all()) and not bool((c[:B][~keep[:B]] == FILL16).all())
    for c in got8[:2]:
        assert bool((c[keep] == FILL8).all())
    for c in got8[2:]:
        assert bool((c.permute(0, 2, 1)[keep] == FILLS).all()) and not bool((c[:B].permute(0, 2, 1)[~keep[:B]] == FILLS).any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_append_multi_stops_at_the_end_of_the_cache(O, dtype):
    """pos + t >= Smax: the row is neither written nor rotated; the rows before it are what two single-token calls write, and the sequence
    that lies behind this one in memory keeps its pattern."""
    B, T, H, D, Smax = 1, 4, 2, 64, 10
    d = H * D
    qkv0 = rnd_rows(B * T * 3 * H, D, dtype, seed=9).view(B * T, 3 * d).to(dev())
    pos_t = torch.tensor([Smax - 2], dtype=torch.int32, device=dev())
    tab = O.rope_table(Smax + 8, D, 10000.0, dev())
    ref16, ref8 = _caches(B, Smax, H, D, dtype)
    got16, got8 = _caches(B, Smax, H, D, dtype)
    want = qkv0.clone()
    for t in range(2):
        rows = qkv0[t:t + 1].clone()
        O.decode_rope_append(rows, tab, pos_t + t, *[c[:B] for c in ref16], H, D)
        O.decode_rope_append_kv8(qkv0[t:t + 1].clone(), tab, pos_t + t, *[c[:B] for c in ref8], H, D)
        want[t] = rows[0]
    q16, q8 = qkv0.clone(), qkv0.clone()
    O.decode_rope_append_multi(q16, tab, pos_t, *[c[:B] for c in got16], T, H, D)
    O.decode_rope_append_multi_kv8(q8, tab, pos_t, *[c[:B] for c in got8], T, H, D)
    assert torch.equal(q16, want) and torch.equal(q8, want) and torch.equal(want[2:], qkv0[2:])
    for g, r in zip(got16 + got8[2:], ref16 + ref8[2:]):
        assert torch.equal(g, r)
    for g, r in zip(got8[:2], ref8[:2]):
        assert same_fp8(g.cpu(), r.cpu())
    assert bool((got16[0][1] == FILL16).all()) and bool((got8[0][1] == FILL8).all()) and bool((got8[2][1] == FILLS).all())


# ---- attention, multi-query ------------------------------------------------------------------------------------------------------------
# (B, T, H, D, Smax, lens): the first query of sequence 0 sees one key; 6 splits of 117 keys at D = 64; 32 splits and all 16 queries; the
# queries of one block straddle a split boundary ("straddle": lens = [2c - 1, 3c - 2], c the chunk of mh_attn_decode_multi_splits);
# T = 1, held beside mh_attn_decode; all 16 queries with a cache small enough for one block per (b, h) (16 x 600 scores = 37.5 KiB), the last
# queries clamped at Smax; 9 queries in the 16-wide form at D = 64
ATTN_CASES = [(2, 3, 2, 128, 40, [1, 30]), (3, 5, 4, 64, 700, [1, 333, 690]), (1, 16, 32, 128, 4200, [4100]), (2, 4, 4, 64, 700, "straddle"),
              (3, 1, 4, 64, 700, [1, 333, 700]), (2, 16, 2, 128, 600, [3, 590]), (1, 9, 2, 64, 300, [290])]
LDS_MAX = 150 * 1024  # what a block of the decode attention kernels may request (include/merlin_hip.h)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,H,D,Smax,lens", ATTN_CASES)
def test_attn_decode_multi_per_element(O, dtype, B, T, H, D, Smax, lens):
    """Query (b, t) is held to N.attention_decode(q[b, t], k, v, lens[b] + t) on the dequantised cache with the limit of the rounding model
    on the same inputs (hold() of tests/test_kv8_gpu.py): the fp8 cache and the 16-bit kernel on the exactly cast dequantised cache,
    split-KV and one block per (b, h).  One block per (b, h) keeps T' x Smax fp32 scores in LDS (T' = T rounded up to 4, 8 or 16): where
    they exceed the 150 KiB a block may request - (1, 16, 32, 128, 4200): 262.5 KiB - the launch is refused with an error code, as
    include/merlin_hip.h states, and that refusal is what is asserted."""
    from merlin_amd._lib import MerlinHipError

    if lens == "straddle":
        splits = O.attn_decode_multi_splits(B, T, H, Smax)
        c = (Smax + splits - 1) // splits
        assert splits > 3 and 3 * c - 2 + T <= Smax
        lens = [2 * c - 1, 3 * c - 2]
    d = H * D
    q = rnd_rows(B * T * H, D, dtype, seed=5, lo=0.5, hi=2.0).view(B * T, d).to(dev())
    cache = []
    for seed in (3, 4):
        c8, cs = kv8_quantize(rnd_rows(B * Smax * H, D, dtype, seed=seed).view(B, Smax, H, D))
        cache += [c8.view(B, Smax, d).to(dev()), cs.permute(0, 2, 1).contiguous().to(dev()), kv8_dequantize(c8, cs).to(dev())]
    k8, ks, k64, v8, vs, v64 = cache
    k16, v16 = k64.to(dtype).view(B, Smax, d), v64.to(dtype).view(B, Smax, d)
    assert torch.equal(k16.double().view_as(k64), k64) and torch.equal(v16.double().view_as(v64), v64)  # the cast to the 16-bit type is exact
    rows = [(b, t) for b in range(B) for t in range(T)]
    pairs = [N.attention_decode(q[b * T + t].view(H, D), k64[b], v64[b], min(lens[b] + t, Smax)) for b, t in rows]
    ref, Bc = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    mod = torch.stack([N.attention_decode(q[b * T + t].view(H, D), k64[b], v64[b], min(lens[b] + t, Smax), model=dtype) for b, t in rows])
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev())
    tq = 4 if T <= 4 else (8 if T <= 8 else 16)
    one_block_fits = 4 * tq * max(Smax, 4 * D) <= LDS_MAX
    tag = f"T={T} Smax={Smax} lens={lens}"
    for split in (True, False):
        how = "split-KV" if split else "one block"
        if not split and not one_block_fits:
            for fn in (lambda: O.attn_decode_multi(q, k16, v16, lens_t, T, H, D, split_kv=False),
                       lambda: O.attn_decode_multi_kv8(q, k8, v8, ks, vs, lens_t, T, H, D, split_kv=False)):
                with pytest.raises(MerlinHipError, match="shape"):
                    fn()
            continue
        o = O.attn_decode_multi_kv8(q, k8, v8, ks, vs, lens_t, T, H, D, split_kv=split)
        hold(f"attention decode multi kv8 {how} {tag}", dtype, o.view(B * T, H, D), ref, Bc, mod)
        o = O.attn_decode_multi(q, k16, v16, lens_t, T, H, D, split_kv=split)
        hold(f"attention decode multi 16-bit {how} {tag}", dtype, o.view(B * T, H, D), ref, Bc, mod)
    if T == 1:
        o = O.attn_decode(q, k16, v16, lens_t, H, D)
        hold(f"attention decode (one query) 16-bit {tag}", dtype, o.view(B, H, D), ref, Bc, mod)


# ---- drafter -----------------------------------------------------------------------------------------------------------------------------
def test_ngram_draft_equals_prompt_lookup(O):
    from merlin_amd.generation import _prompt_lookup

    cases = lookup_cases()
    g = torch.Generator().manual_seed(4)
    long = torch.randint(0, 40, (4096,), generator=g).tolist()
    long[-2:] = long[3000:3002]  # a bigram that certainly occurs before
    cases += [(long, 15, 3, 5000), (long, 4, 2, 4097), (long[:4000] + long[:96], 15, 3, 5000)]
    hits = 0
    for ids, k, ng, max_length in cases:
        x = torch.tensor([ids + [0] * 3], dtype=torch.int64, device=dev())  # (row stride > length)
        out, cnt = O.ngram_draft(x, len(ids), ng, k, max_length)
        want = _prompt_lookup(ids, k, ng, max_length)
        n = int(cnt[0])
        assert out[0, :n].tolist() == want and n == len(want), (len(ids), k, ng, max_length, out[0, :n].tolist(), want)
        hits += bool(want)
    assert hits > 100
    # several rows in one launch: every row is drafted on its own
    rows = [c[0] for c in cases[:8]]
    n = min(len(r) for r in rows)
    x = torch.tensor([r[:n] for r in rows], dtype=torch.int64, device=dev())
    out, cnt = O.ngram_draft(x, n, 2, 3, 100)
    for r in range(len(rows)):
        assert out[r, :int(cnt[r])].tolist() == _prompt_lookup(rows[r][:n], 3, 2, 100)


# ---- engine --------------------------------------------------------------------------------------------------------------------------------
ENGINE_CONFIGS = [("16-bit weights", False, dict()), ("fp8 weights", False, dict(fp8=True)), ("fp4 weights", False, dict(fp4=True)),
                  ("fp8 cache", True, dict())]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("name,kv8,w", ENGINE_CONFIGS)
def test_verify_step_reproduces_sequential_decode_steps(dtype, name, kv8, w):
    """Six teacher-forced tokens.  (a) six decode_steps; (b) one verify_step on a fresh prefill; (c) after (b): advance(3) and one
    decode_step of the fourth token - it must reproduce (a)'s logits there, i.e. the stale rows 3..5 are ignored and overwritten; (d) the
    prompt twice in the batch (B = 2, T = 6), lens unchanged by verify_step.  dev(b, a), dev(c, a), dev(d, a) <= 2 max(d_pre, d_rows), both
    measured in this run: d_pre = dev(full-sequence forward() logits at those positions, a), the use_cache=False cross-check, and d_rows =
    dev(row 0 of decode_step on the prompt replicated to six rows, a), the many-row kernel forms against the one-row forms.  The factor 2
    covers two independent rounding paths; a wrong position, mask or cache row moves the logits by orders of magnitude more.
    With fp8 / fp4 weights d_pre also holds the weight format's error (forward() runs 16-bit weights) and that bound is loose, so a second
    one is asserted as well: (a) .. (d) share their weights whatever the format and differ only in how activations are rounded (row-count
    forms of the projections, the attention kernel, the order of cache writes), which is what the SAME cross-check measures with 16-bit
    weights - d_pre16 = dev(forward() logits, six decode_steps with 16-bit weights on the same cache format).  All three deviations
    must also stay within tight = 2 max(d_pre16, d_rows)."""
    cfg, m, ids, images = _tiny(dtype)
    eng = m.engine
    V, P, S = cfg.vocab_size, ids.shape[1], 6
    assert ids.shape[0] == 1
    g = torch.Generator().manual_seed(11)
    toks = torch.randint(3, V, (S,), generator=g).cuda()
    _, ca = eng.prefill(ids, None, images, S + 2, kv_fp8=kv8)
    a = [eng.decode_step(toks[t:t + 1], ca, **w).clone() for t in range(S)]
    _, cb = eng.prefill(ids, None, images, S + 2, kv_fp8=kv8)
    n0 = cb.lens.clone()
    lb = eng.verify_step(toks[None, :], cb, **w).clone()
    assert lb.shape[:2] == (1, S) and torch.equal(cb.lens, n0)
    cb.advance(3)
    assert torch.equal(cb.lens, n0 + 3)
    lc = eng.decode_step(toks[3:4], cb, **w).clone()
    assert torch.equal(cb.lens, n0 + 4)
    _, cd = eng.prefill(ids.repeat(2, 1), None, images * 2, S + 2, kv_fp8=kv8)
    n2 = cd.lens.clone()
    ld = eng.verify_step(toks[None, :].repeat(2, 1), cd, **w).clone()
    assert torch.equal(cd.lens, n2) and ld.shape[:2] == (2, S)
    with torch.no_grad():
        full = m(input_ids=torch.cat([ids, toks[None, :]], dim=1), images=images).logits[0, P:P + S].float()
    _, c6 = eng.prefill(ids.repeat(6, 1), None, images * 6, S + 2, kv_fp8=kv8)
    rows = [eng.decode_step(toks[t:t + 1].repeat(6), c6, **w)[:1].clone() for t in range(S)]
    d_pre = _dev([full[t:t + 1] for t in range(S)], a, V)
    if w:  # the same cross-check with the 16-bit weights forward() itself uses
        _, c16 = eng.prefill(ids, None, images, S + 2, kv_fp8=kv8)
        d_pre16 = _dev([full[t:t + 1] for t in range(S)], [eng.decode_step(toks[t:t + 1], c16).clone() for t in range(S)], V)
    else:
        d_pre16 = d_pre
    d_rows = _dev(rows, a, V)
    d_b = _dev([lb[:, t] for t in range(S)], a, V)
    d_c = _dev([lc], a[3:4], V)
    d_d = max(_dev([ld[r:r + 1, t] for t in range(S)], a, V) for r in range(2))
    bound = 2 * max(d_pre, d_rows)
    tight = 2 * max(d_pre16, d_rows)
    print(f"SPEC | {name} | {str(dtype)[6:]} | d_pre16 = {d_pre16:.3e} | tight = {tight:.3e} | d_pre = {d_pre:.3e} | d_rows = {d_rows:.3e} | dev(b, a) = {d_b:.3e} | dev(c, a) = {d_c:.3e} | "
          f"dev(d, a) = {d_d:.3e} | bound = {bound:.3e}")
    assert d_b <= bound and d_c <= bound and d_d <= bound, (d_b, d_c, d_d, bound)
    assert max(d_b, d_c, d_d) <= tight, (d_b, d_c, d_d, tight)


# ---- generate() ------------------------------------------------------------------------------------------------------------------------------
def _gold_model(i, dtype=torch.float16):
    from test_generation_gpu import GOLD, _model

    rec = GOLD["cases"][i]
    cfg, batch, m = _model(rec["case"], rec["logit_gain"], dtype)
    ids = batch["input_ids"][:, :rec["prompt_len"]].cuda()
    return rec, cfg, m, ids, [im.cuda() for im in batch["images"]]


def _step_logits(m, ids, am, images, new, kv8=False, **w):
    """The plain path's logits that choose new token number len(new): prefill + teacher-forced decode_steps under the given flags."""
    eng = m.engine
    lg, cache = eng.prefill(ids, am, images, len(new) + 2, kv_fp8=kv8)
    for t in new:
        lg = eng.decode_step(torch.tensor([t], device=ids.device), cache, **w)
    return lg[0, :m.config.vocab_size].float()


def _same_or_greedy_tie(m, ids, am, images, got, want, kv8=False, **w):
    """Equal, or first different at a step where the token the speculative path picked (`got`) lies within rounding of the maximum of the
    plain path's own logits (`want` is that path's output, so its token IS their argmax: the rule of test_generation_gpu._same_or_tie,
    2e-3 of the largest magnitude, is applied to the OTHER token), on the decode path with the same flags."""
    got, want = got.cpu(), want.cpu()
    if got.tolist() == want.tolist():
        return
    P = ids.shape[1]
    n = min(got.shape[1], want.shape[1])
    diff = (got[0, :n] != want[0, :n]).nonzero()
    assert diff.numel(), ("one is a prefix of the other", got.tolist(), want.tolist())
    t = int(diff[0])
    assert t >= P
    lg = _step_logits(m, ids, am, images, want[0, P:t].tolist(), kv8, **w)
    tol = 2e-3 * float(lg.abs().max())
    gap_got, gap_want = float(lg.max() - lg[int(got[0, t])]), float(lg.max() - lg[int(want[0, t])])
    assert gap_got < tol and gap_want < tol, ("diverged at", t, "without a tie", gap_got, gap_want, tol, got.tolist(), want.tolist())


def _replay(seq, P, k, ng, max_len):
    """The lookup loop replayed on the CPU over a finished sequence: -> (verify steps, drafted, accepted, positions of accepted drafts)."""
    from merlin_amd.generation import _prompt_lookup

    n, steps, drafted, accepted, where = P + 1, 0, 0, 0, []
    while n < len(seq):
        d = _prompt_lookup(seq[:n], k, ng, max_len)
        if not d:
            n += 1
            continue
        a = 0
        while a < len(d) and n + a < len(seq) and d[a] == seq[n + a]:
            a += 1
        steps, drafted, accepted = steps + 1, drafted + len(d), accepted + a
        where += list(range(n, n + a))
        n += a + 1
    return steps, drafted, accepted, where


@pytest.mark.parametrize("i", range(5))
def test_greedy_lookup_matches_reference(i):
    from test_generation_gpu import GOLD, _same_or_tie

    assert len(GOLD["cases"]) == 5
    rec, cfg, m, ids, images = _gold_model(i)
    kw = dict(max_new_tokens=rec["max_new_tokens"], do_sample=False, eos_token_id=rec["eos_token_id"], pad_token_id=0)
    want = torch.tensor(rec["greedy"])
    for k in (1, 4, 15):
        for use_graph in (True, False):
            got = m.generate(ids, images=images, prompt_lookup_num_tokens=k, use_graph=use_graph, **kw).cpu()
            _same_or_tie(m, images, got, want, rec["prompt_len"], (k, use_graph))
            st = m.engine.last_generate_stats
            assert st["accepted"] <= st["drafted"] <= k * st["verify_steps"]


def test_left_padded_prompt_lookup_equals_plain():
    rec, cfg, m, ids, images = _gold_model(4)
    pad = torch.zeros(1, 3, dtype=torch.int64, device=ids.device)
    ids_p = torch.cat([pad, ids], dim=1)
    am = torch.cat([torch.zeros_like(pad), torch.ones_like(ids)], dim=1).bool()
    kw = dict(images=images, attention_mask=am, max_new_tokens=24, eos_token_id=-1, pad_token_id=0)
    plain = m.generate(ids_p, **kw)
    assert m.engine.last_generate_stats == dict(plain_steps=23, verify_steps=0, drafted=0, accepted=0)
    for use_graph in (True, False):
        got = m.generate(ids_p, prompt_lookup_num_tokens=4, use_graph=use_graph, **kw)
        assert got.shape == plain.shape and torch.equal(got[:, :ids_p.shape[1]], ids_p)
        _same_or_greedy_tie(m, ids_p, am, images, got, plain)
        assert m.engine.last_generate_stats["verify_steps"] >= 1


def test_seeded_sampling_lookup_equals_plain_or_a_cdf_tie():
    """temperature 0.8, seed 4242: the speculative path replayed from graphs equals the eager one exactly; it equals the plain path, except
    from a step on where mh_select_tokens' own uniform lies within 2e-3 of the inverse-CDF boundary between the two tokens (on the plain
    path's logits for the common prefix): the sampling analogue of _same_or_tie."""
    import numpy as np

    from merlin_amd import ops
    from oracle import gen_ref as R

    rec, cfg, m, ids, images = _gold_model(4)
    P, V = ids.shape[1], cfg.vocab_size
    kw = dict(images=images, max_new_tokens=32, eos_token_id=-1, pad_token_id=0, do_sample=True, temperature=0.8, seed=4242)
    plain = m.generate(ids, **kw).cpu()
    eager = m.generate(ids, prompt_lookup_num_tokens=4, use_graph=False, **kw).cpu()
    graph = m.generate(ids, prompt_lookup_num_tokens=4, use_graph=True, **kw).cpu()
    assert eager.shape == plain.shape and torch.equal(eager, graph), (eager.tolist(), graph.tolist())
    if eager.tolist() != plain.tolist():
        t = int((eager[0] != plain[0]).nonzero()[0])
        assert t >= P
        lg = _step_logits(m, ids, None, images, plain[0, P:t].tolist())
        _, u = ops.select_tokens(lg[None].contiguous(), V, do_sample=True, temperature=0.8, top_k=50, top_p=1.0, seed=4242, step=t - P, return_u=True)
        u = float(u[0])
        cdf = np.cumsum(R.warp_probs(lg.cpu().numpy(), 0.8, 50, 1.0))
        for tok in (int(eager[0, t]), int(plain[0, t])):
            lo, hi = (cdf[tok - 1] if tok else 0.0), cdf[tok]
            assert lo - 2e-3 <= u <= hi + 2e-3, ("diverged at", t, "away from a CDF boundary", tok, u, lo, hi, eager.tolist(), plain.tolist())


@pytest.mark.parametrize("flags", [dict(fp8_kv=True), dict(fp8_weights=True), dict(fp4_weights=True)], ids=lambda f: next(iter(f)))
def test_lookup_with_cache_and_weight_formats(flags):
    rec, cfg, m, ids, images = _gold_model(4)
    kw = dict(images=images, max_new_tokens=24, eos_token_id=-1, pad_token_id=0, **flags)
    plain = m.generate(ids, **kw)
    runs = [m.generate(ids, prompt_lookup_num_tokens=4, **kw) for _ in range(2)]
    assert torch.equal(runs[0], runs[1]) and runs[0].shape == (1, ids.shape[1] + 24)
    w = dict(fp8=bool(flags.get("fp8_weights")), fp4=bool(flags.get("fp4_weights")))
    _same_or_greedy_tie(m, ids, None, images, runs[0], plain, bool(flags.get("fp8_kv")), **w)


def _covering_case():
    """A (prompt, max_new_tokens) whose PLAIN greedy output, replayed through _prompt_lookup on the CPU (k = 4, n = 2), predicts at least one
    accepted and at least one rejected draft token, one of the accepted ones being the first occurrence of its token among the new tokens
    (so that an EOS set to it fires inside an accepted run): the coverage condition of the test below, established on the plain path
    alone.  Candidates: the golden prompts, and the same prompts extended by the first 8 tokens of their own greedy continuation (text
    the output then copies from the PROMPT), with 16, 32 and 64 new tokens."""
    for i in (4, 0, 3):
        rec, cfg, m, ids0, images = _gold_model(i)
        base = dict(images=images, eos_token_id=-1, pad_token_id=0)
        for extend in (8, 0):
            ids = m.generate(ids0, max_new_tokens=extend, **base) if extend else ids0
            P = ids.shape[1]
            for max_new in (16, 32, 64):
                kw = dict(base, max_new_tokens=max_new)
                plain = m.generate(ids, **kw).cpu()
                steps, drafted, accepted, where = _replay(plain[0].tolist(), P, 4, 2, plain.shape[1])
                new = plain[0, P:].tolist()
                inside = [p for p in where if new.index(int(plain[0, p])) == p - P]
                if accepted >= 1 and drafted > accepted and inside:
                    return m, ids, images, kw, plain, inside
    raise AssertionError("no candidate whose plain output has an accepted and a rejected draft token and a first occurrence inside an accepted run")


def test_lookup_accepts_rejects_stops_and_streams():
    """On a case that satisfies the coverage condition (see _covering_case): drafts are accepted and rejected; an EOS token and a
    stopping criterion (a callable returning a bool) that fire INSIDE an accepted run end the output there, as on the plain path; the
    streamer gets every step's tokens in one put and their concatenation is the new tokens."""
    m, ids, images, kw, plain, inside = _covering_case()
    P = ids.shape[1]
    got = m.generate(ids, prompt_lookup_num_tokens=4, **kw).cpu()
    st = dict(m.engine.last_generate_stats)
    _same_or_greedy_tie(m, ids, None, images, got, plain)
    if got.tolist() == plain.tolist():
        assert (st["verify_steps"], st["drafted"], st["accepted"]) == _replay(plain[0].tolist(), P, 4, 2, plain.shape[1])[:3]
    assert st["accepted"] >= 1 and st["drafted"] > st["accepted"] and st["verify_steps"] >= 1, st
    # a stop inside an accepted run: a token whose first occurrence among the new tokens is an accepted draft
    p = inside[-1]
    tok = int(plain[0, p])
    kw_eos = dict(kw, eos_token_id=tok)
    want = m.generate(ids, **kw_eos).cpu()
    got = m.generate(ids, prompt_lookup_num_tokens=4, **kw_eos).cpu()
    assert want.shape[1] == p + 1 and int(want[0, -1]) == tok
    assert got.tolist() == want.tolist()
    seen = []

    def criterion(output_ids, scores, **_):
        seen.append(output_ids.shape[1])
        return bool(output_ids[0, -1] == tok)

    got = m.generate(ids, prompt_lookup_num_tokens=4, stopping_criteria=[criterion], **kw).cpu()
    assert got.tolist() == want.tolist()
    assert seen == list(range(P + 1, p + 2))  # every emitted prefix, in order, none after the stop

    class Streamer:
        def __init__(self):
            self.puts, self.ended = [], False

        def put(self, t):
            self.puts.append(t.clone())

        def end(self):
            self.ended = True

    s = Streamer()
    got = m.generate(ids, prompt_lookup_num_tokens=4, streamer=s, **kw).cpu()
    st = m.engine.last_generate_stats
    assert s.ended and torch.equal(s.puts[0], ids.cpu())
    assert torch.cat([t.reshape(-1) for t in s.puts[1:]]).tolist() == got[0, P:].tolist()
    assert len(s.puts) - 1 == 1 + st["plain_steps"] + st["verify_steps"] and max(t.numel() for t in s.puts[1:]) > 1
