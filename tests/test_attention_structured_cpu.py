"""The structured attention inputs of tests/attn_inputs.py, and the arithmetic the prefill forwards document, on the CPU.

1. Every generator's properties hold at every shape tests/test_attention_structured_gpu.py uses; the suite's randn inputs give no move of the
   running reference after a row's first - the gap those families close.
2. A torch fp32 EMULATOR of the forward's tile loop (csrc/attn_fwd2.hip: 64-key tiles, the lazy rule `m_new > m_run + 8`, alpha per row but
   the rescale of o applied on a ballot over the 32 rows of a wave, P rounded to the 16-bit type before P V, lse = (m_run + log2 l) ln 2)
   stays within numerics.limit(c_model) of the fp64 reference on every family and both types: the documented arithmetic alone meets the
   bound the GPU tests apply.  Likewise a split-KV merge emulator for the decode kernels.
3. MUTANTS of the emulators - o rescaled but l not; alpha applied but m_run not moved; the rescale skipped unless every row of the ballot
   needs it; lse taken from the true maximum; a split merge that drops one split's exp2(m_i - M) - are rejected on at least one family.  On
   the randn inputs the first three are INSIDE the limit for o and for lse: nothing in a randn run reaches the code they break.  The other
   two are not silent on randn, and the test says so instead of asserting it: "lse from the true maximum" leaves o alone - o is all the
   per-element suite held before lse had a bound - but its lse is off by (m_true - m_run) ln 2 on randn as well (c = 2.8e6 against a limit of
   2; the loose lse check of tests/test_ops_gpu.py sees it too); the merge without one split's weight scores c = 30 (bf16) and 239 (fp16) on
   randn, where split maxima differ by about a bit, against 200 to 36 000 on the placements.  Every line printed is
   `mutant | inputs | dtype | c of o (limit) | c of lse (limit)`."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import attn_inputs as AI  # noqa: E402
import numerics as N  # noqa: E402

DTYPES = [torch.bfloat16, torch.float16]
LN2 = 0.6931471805599453


# ---- 1. properties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,S,H,D,causal,lens", AI.PREFILL_SHAPES)
def test_every_family_has_its_properties_at_the_gpu_shapes(dtype, B, S, H, D, causal, lens):
    """The generators assert their own properties; this runs them for every head of every GPU shape and prints the figures."""
    for name in AI.families(causal):
        heads, q, k = AI.prefill_heads(name, B, S, H, D, dtype, causal, lens)
        assert q.shape == k.shape == (B * S, H * D) and q.dtype == dtype
        for i, r in enumerate(heads):
            fig = {key: (r[key] if not torch.is_tensor(r[key]) else (int(r[key].max()), float(r[key].double().median())))
                   for key in ("events", "pmax", "pmin", "lead", "shift", "A_max") if key in r}
            print(f"family {name:6s} {str(dtype)[6:]:9s} S={S} head {i}: {fig}")
            assert r["A_max"] <= AI.A_CAP


def test_issue_figures_of_the_staircase_at_384_causal():
    for dtype in DTYPES:
        r = AI.prefill_family("F1", 384, 128, dtype, True, seed=1)
        assert float(r["events"].double().median()) >= 2 and int(r["events"].max()) >= 4 and r["pmax"] >= 128
        r = AI.prefill_family("F2", 384, 128, dtype, True, seed=1)
        assert int(r["events"].max()) == 0 and r["pmin"] <= 2.0 ** -30


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", [384, 4096])
def test_randn_inputs_never_move_the_reference_after_the_first_tile(dtype, S):
    """The suite's own inputs (randn, D = 128, causal): no event after a row's first tile, P far below the 256 the rule allows."""
    q, k = AI.randn16(S, 128, dtype, 1), AI.randn16(S, 128, dtype, 2)
    ev, pmax = AI.lazy_events(AI.scores64(q, k) * AI.LOG2E, True)
    print(f"randn S={S} {str(dtype)[6:]}: events after the first {int(ev.sum())}, largest P against the reference in force {pmax:.1f}")
    assert int(ev.sum()) == 0 and pmax < 64.0


def test_lazy_events_counts_by_hand():
    """Three tiles of two keys: levels 0, 9, 12 bits -> one move (at 9: > 8 above 0), then 12 is only 3 above 9: P = 8 against the stale
    reference.  Levels 0, 7, 14: 7 does not move it, 14 does; largest P = 2^7."""
    lv = torch.tensor([[0.0, 0.0, 9.0, 9.0, 12.0, 12.0], [0.0, 0.0, 7.0, 7.0, 14.0, 14.0]])
    s = torch.zeros(6, 6)
    s[0], s[1] = lv[0], lv[1]
    ev, pmax = AI.lazy_events(s, False, tile=2)
    assert ev.tolist()[:2] == [1, 1] and pmax == 128.0
    ev, _ = AI.lazy_events(s, True, tile=2)  # causal: row 0 sees key 0 only, row 1 keys 0 and 1
    assert ev.tolist()[:2] == [0, 0]


# ---- 2. the emulators ------------------------------------------------------------------------------------------------------------------------
def emulate_forward(q, k, v, dtype, *, causal, n_valid=None, mutant=None, tile=64, wave=32, thr=8.0):
    """csrc/attn_fwd2.hip in torch fp32, one head: -> (o [S, D] in dtype, lse fp32 [S]).  mutant: None, "l", "m_run", "ballot", "lse"."""
    S, D = q.shape
    n = S if n_valid is None else int(n_valid)
    f32 = torch.float32
    sc = torch.tensor((1.0 / math.sqrt(D)) * 1.4426950408889634, dtype=f32)
    ok = AI.allowed(S, causal, n)
    st = (q.float() @ k.float().t()).masked_fill(~ok, float("-inf"))
    V = v.float()
    m_run = torch.full((S,), float("-inf"), dtype=f32)
    m_true = m_run.clone()
    l_run = torch.zeros(S, dtype=f32)
    o = torch.zeros(S, D, dtype=f32)
    for k0 in range(0, S, tile):
        s_t = st[:, k0:k0 + tile]
        mx = s_t.amax(1) * sc
        m_true = torch.maximum(m_true, mx)
        m_new = torch.maximum(m_run, mx)
        need = m_new > m_run + thr
        first = torch.isinf(m_run)
        alpha = torch.where(need & ~first, torch.exp2(m_run - m_new), torch.where(need, torch.zeros_like(mx), torch.ones_like(mx)))
        move = need if mutant != "m_run" else (need & first)
        m_run = torch.where(move, m_new, m_run)
        m_use = torch.where(torch.isinf(m_run), torch.zeros_like(m_run), m_run)
        p = torch.exp2(s_t * sc - m_use[:, None])
        l_run = (l_run if mutant == "l" else l_run * alpha) + p.sum(1)
        w = need.view(-1, wave) if S % wave == 0 else None
        if w is None:  # (a partial last wave: pad the ballot with lanes that need nothing)
            pad = (-S) % wave
            w = torch.cat([need, torch.zeros(pad, dtype=torch.bool) if mutant != "ballot" else torch.ones(pad, dtype=torch.bool)]).view(-1, wave)
        vote = (w.all(1) if mutant == "ballot" else w.any(1)).repeat_interleave(wave)[:S]
        o = torch.where(vote[:, None], o * alpha[:, None], o)
        o = o + N.r16(p, dtype) @ V[k0:k0 + tile]
    valid = (torch.arange(S) < n) & (l_run > 0)
    inv = torch.where(valid, 1.0 / l_run, torch.zeros_like(l_run))
    lse = torch.where(valid, ((m_true if mutant == "lse" else m_run) + torch.log2(l_run)) * LN2, torch.zeros_like(l_run))
    return (o * inv[:, None]).to(dtype), lse


def emulate_split_decode(q, k64, v64, n, splits, dtype, *, drop=None):
    """The split-KV decode kernels in torch fp32, one sequence: q [H, D], keys and values [n, H, D]; every split keeps (m_i, l_i, o_i) against
    its own maximum with P in fp32, the merge weighs them by exp2(m_i - M).  drop = i: split i's weight is taken as 1."""
    H, D = q.shape
    sc = torch.tensor((1.0 / math.sqrt(D)) * 1.4426950408889634, dtype=torch.float32)
    s = torch.einsum("hd,nhd->hn", q.float(), k64.float()) * sc
    V = v64.float()
    chunk = (n + splits - 1) // splits
    parts = []
    for i in range(splits):
        lo, hi = i * chunk, min(n, (i + 1) * chunk)
        if lo >= hi:
            continue
        m = s[:, lo:hi].amax(1)
        p = torch.exp2(s[:, lo:hi] - m[:, None])
        parts.append((i, m, p.sum(1), torch.einsum("hn,nhd->hd", p, V[lo:hi])))
    M = torch.stack([m for _, m, _, _ in parts]).amax(0)
    num, den = torch.zeros(H, D), torch.zeros(H)
    for i, m, l, o in parts:
        w = torch.ones_like(m) if i == drop else torch.exp2(m - M)
        num, den = num + w[:, None] * o, den + w * l
    return (num / den[:, None]).to(dtype)


def head_inputs(name, S, D, dtype, causal, n, seed=1):
    """-> (q, k, v, A-free dict of the family or None for randn)."""
    if name == "randn":
        q, k, r = AI.randn16(S, D, dtype, 11 * seed), AI.randn16(S, D, dtype, 11 * seed + 1), None
    else:
        r = AI.prefill_family(name, S, D, dtype, causal, n_valid=n, seed=seed)
        q, k = r["q"], r["k"]
    return q, k, AI.randn16(S, D, dtype, 11 * seed + 2)


def forward_scores(q, k, v, dtype, causal, n, mutant=None):
    """-> dict: c of o and of lse for the emulator (or a mutant of it), and the limits from the rounding models."""
    ref = N.attention(q, k, v, causal=causal, n_valid=n)
    mod = N.attention(q, k, v, causal=causal, n_valid=n, model=dtype)
    A_row = N.attention_magnitude(q, k, causal=causal, n_valid=n)
    o, lse = emulate_forward(q, k, v, dtype, causal=causal, n_valid=n, mutant=mutant)
    eps, tiny = N.EPS16[dtype], N.TINY[dtype]
    try:
        c_o = N.componentwise(o, ref["o"], ref["B_o"], eps, tiny)[0]
    except AssertionError:
        c_o = float("inf")
    return {"o": c_o, "lim_o": N.limit(N.componentwise(mod["o"], ref["o"], ref["B_o"], eps, tiny)[0]),
            "lse": N.lse_c(lse, ref["lse"], A_row)[0],
            "lim_lse": N.limit(N.lse_c(N.attention_lse_model(q, k, causal=causal, n_valid=n), ref["lse"], A_row)[0])}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,S,H,D,causal,lens", AI.PREFILL_SHAPES)
def test_the_documented_arithmetic_meets_the_bound_on_every_family(dtype, B, S, H, D, causal, lens):
    for name in ["randn"] + AI.families(causal):
        for n in sorted(set(lens or [S])):
            q, k, v = head_inputs(name, S, D, dtype, causal, n)
            c = forward_scores(q, k, v, dtype, causal, n)
            print(f"emulator | {name:7s} S={S} n={n} | {str(dtype)[6:]:8s} | o {c['o']:.3f} (limit {c['lim_o']:.3f}) | lse {c['lse']:.3f} (limit {c['lim_lse']:.3f})")
            assert c["o"] <= c["lim_o"] and c["lse"] <= c["lim_lse"], (name, S, n, c)


# ---- 3. mutants ------------------------------------------------------------------------------------------------------------------------------
# mutant -> the output it corrupts.  "lse" leaves o alone, so on randn it is o - all the per-element suite holds today - that stays inside.
FORWARD_MUTANTS = {"l": "o", "m_run": "o", "ballot": "o", "lse": "lse"}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mutant", list(FORWARD_MUTANTS))
def test_forward_mutants_pass_on_randn_and_fail_on_a_family(dtype, mutant):
    S, D, causal = 384, 128, True
    what = FORWARD_MUTANTS[mutant]
    q, k, v = head_inputs("randn", S, D, dtype, causal, S)
    c = forward_scores(q, k, v, dtype, causal, S, mutant=mutant)
    print(f"mutant {mutant:7s} | randn   | {str(dtype)[6:]:8s} | o {c['o']:.3f} (limit {c['lim_o']:.3f}) | lse {c['lse']:.3f} (limit {c['lim_lse']:.3f})")
    assert c["o"] <= c["lim_o"], (mutant, "randn", c)
    if what == "o":
        assert c["lse"] <= c["lim_lse"], (mutant, "randn", c)
    caught = []
    for name in AI.families(causal):
        q, k, v = head_inputs(name, S, D, dtype, causal, S)
        c = forward_scores(q, k, v, dtype, causal, S, mutant=mutant)
        print(f"mutant {mutant:7s} | {name:7s} | {str(dtype)[6:]:8s} | o {c['o']:.1f} (limit {c['lim_o']:.3f}) | lse {c['lse']:.1f} (limit {c['lim_lse']:.3f})")
        if c[what] > c["lim_" + what]:
            caught.append(name)
    assert "F1" in caught, (mutant, caught)


def _decode_case(kind, n, H, D, dtype, heavy, shift=0):
    r = AI.cache_family(kind, n, H, D, dtype, heavy, seed=1, shift=shift)
    g = torch.Generator().manual_seed(5)
    from test_kv8_cpu import kv8_dequantize, kv8_quantize

    v8, vs = kv8_quantize(torch.randn(n, H, D, generator=g).to(dtype))
    return r["q"], r["k64"], kv8_dequantize(v8, vs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_split_merge_emulator_and_its_mutant(dtype):
    """The merge emulator meets the decode bound on randn and on every placement; the merge that takes one split's weight as 1 is rejected
    on the placements that put the mass into another split.  Its c on randn is printed as well."""
    n, H, D, splits = 700, 4, 64, 6
    chunk = (n + splits - 1) // splits
    g = torch.Generator().manual_seed(3)
    cases = {"randn": (torch.randn(H, D, generator=g).to(dtype), torch.randn(n, H, D, generator=g).to(dtype).double(), torch.randn(n, H, D, generator=g).to(dtype).double())}
    for tag, heavy in AI.placements(n, chunk, splits).items():
        cases["onehot " + tag] = _decode_case("onehot", n, H, D, dtype, heavy[:1])
        cases["sink " + tag] = _decode_case("sink", n, H, D, dtype, heavy, shift=1)
    drop = 2  # a middle split
    rejected = []
    for tag, (q, k64, v64) in cases.items():
        ref, Bc = N.attention_decode(q, k64, v64, n)
        lim = N.limit(N.componentwise(N.attention_decode(q, k64, v64, n, model=dtype), ref, Bc, N.EPS16[dtype], N.TINY[dtype])[0])
        c = N.componentwise(emulate_split_decode(q, k64, v64, n, splits, dtype), ref, Bc, N.EPS16[dtype], N.TINY[dtype])[0]
        cm = N.componentwise(emulate_split_decode(q, k64, v64, n, splits, dtype, drop=drop), ref, Bc, N.EPS16[dtype], N.TINY[dtype])[0]
        print(f"merge | {tag:22s} | {str(dtype)[6:]:8s} | emulator {c:.3f} | weight of split {drop} dropped {cm:.1f} | limit {lim:.3f}")
        assert c <= lim, (tag, c, lim)
        if cm > lim:
            rejected.append(tag)
    assert any(t.startswith("onehot") for t in rejected) and any(t.startswith("sink") for t in rejected), rejected
    assert "onehot first split" in rejected and "onehot last split" in rejected
