"""Beam search on a shared prompt KV cache (generate(num_beams=n, share_prompt_kv=True)) on the GPU: the ancestry table and the appends to the
per-beam suffix bit for bit against the copying path (engine.expand_cache + reorder_cache), mh_attn_decode_beams / _kv8 per element against
the fp64 reference on the materialised per-beam keys with its rounding model (hold() of tests/test_kv8_gpu.py), decode_step on a
BeamKVCache against decode_step on the expanded cache under the criterion of test_spec_gpu's verify-step test, and generate() against the
goldens, the oracle and the copying path."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import numerics as N  # noqa: E402
from test_beams_cpu import ancestry_step  # noqa: E402
from test_kv8_cpu import kv8_dequantize, kv8_quantize  # noqa: E402
from test_kv8_gpu import _dev, _tiny, hold, rnd_rows, same_fp8  # noqa: E402
from test_spec_gpu import ENGINE_CONFIGS  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
FILL16, FILL8, FILLS = 0.3125, 0x2B, 7.0


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def O():
    from merlin_amd import ops

    assert ops.arch_ok(0), "not a gfx950 device"
    return ops


_MODELS = {}


def tiny(dtype):
    """The tiny multimodal fixture of tests/test_kv8_gpu.py, built once per dtype for this module."""
    if dtype not in _MODELS:
        _MODELS[dtype] = _tiny(dtype)
        _MODELS[dtype][1].engine.ensure_arena()
    return _MODELS[dtype]


def in_group(local, nb):
    """[Bp, nb] beam numbers inside their group -> beam_idx int64 [Bp*nb] on the device."""
    local = torch.as_tensor(local)
    return (local + nb * torch.arange(local.shape[0])[:, None]).reshape(-1).to(dev())


# ---- ancestry and append -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kv8"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_shared_cache_equals_expand_and_reorder(O, dtype, fp8):
    """Bp = 2 prompts (7 and 40 valid rows of Pmax = 40), nb = 5, G = 9, 8 steps: the same random qkv rows appended to the expanded cache
    (expand_cache, then reorder_cache every step: the reference) and to the shared one (pos = gen, rope_pos = apos; then cache.reorder) with
    the same in-group beam_idx - step 2 one parent for all beams of a prompt, step 4 the identity.  After every step materialize() equals
    the expanded cache's valid rows (K, V, scales) and the rotated qkv are equal; the prefix is never written (guard rows at and beyond
    pre_lens included, same storage), and suffix slot 8, which no step writes, keeps its guard values."""
    from merlin_amd.model.engine import HipEngine

    eng = tiny(dtype)[1].engine
    Bp, nb, H, D, Pmax, G, steps = 2, 5, 4, 64, 40, 9, 8
    pre_lens, d, n = [7, 40], 4 * 64, 10
    c0 = HipEngine.KVCache(1, Bp, Pmax, d, dtype, dev(), fp8=fp8, H=H)
    big = HipEngine.KVCache(1, Bp, Pmax + G, d, dtype, dev(), fp8=fp8, H=H)  # the same prompts with room to append: what expand_cache copies
    for i, (t, tb) in enumerate(zip(c0.k + c0.v, big.k + big.v)):
        if fp8:
            t.copy_(kv8_quantize(rnd_rows(Bp * Pmax * H, D, dtype, seed=3 + i).view(Bp, Pmax, H, D))[0].view(Bp, Pmax, d))
        else:
            t.copy_(rnd_rows(Bp * Pmax, d, dtype, seed=3 + i).view(Bp, Pmax, d))
        t[0, pre_lens[0]:] = FILL8 if fp8 else FILL16
        tb[:, :Pmax] = t
    if fp8:
        for i, (t, tb) in enumerate(zip(c0.ks + c0.vs, big.ks + big.vs)):
            t.copy_(torch.exp2(torch.randint(-6, 3, (Bp, H, Pmax), generator=torch.Generator().manual_seed(i)).float()))
            t[0, :, pre_lens[0]:] = FILLS
            tb[:, :, :Pmax] = t
    for c in (c0, big):
        c.lens.copy_(torch.tensor(pre_lens, dtype=torch.int32))
    exp = eng.expand_cache(big, torch.arange(Bp, device=dev()).repeat_interleave(nb))
    sh = eng.share_cache(c0, nb, G)
    ptrs = [t.data_ptr() for lst in c0.sets() for t in lst]
    before = [t.clone() for lst in c0.sets() for t in lst]
    assert sh.prefix is c0 and sh.pre_lens is c0.lens and [t.data_ptr() for lst in sh.prefix.sets() for t in lst] == ptrs
    assert sh.k[0].shape == (n, G, d) and sh.k[0].dtype == c0.k[0].dtype and sh.anc.shape == (n, G) and sh.anc.dtype == torch.int32
    assert sh.gen.tolist() == [0] * n and sh.apos.tolist() == [7] * 5 + [40] * 5
    for t in sh.k + sh.v:
        t.fill_(FILL8 if fp8 else FILL16)
    if fp8:
        assert sh.ks[0].shape == (n, H, G)
        for t in sh.ks + sh.vs:
            t.fill_(FILLS)
    tab = O.rope_table(Pmax + G + 8, D, 10000.0, dev())
    append = O.decode_rope_append_kv8 if fp8 else O.decode_rope_append
    g = torch.Generator().manual_seed(5)
    for t in range(steps):
        qkv0 = rnd_rows(n * 3 * H, D, dtype, seed=100 + t).view(n, 3 * d).to(dev())
        q_ref, q_sh = qkv0.clone(), qkv0.clone()
        append(q_ref, tab, exp.lens, *exp.layer(0), H, D)
        exp.lens.add_(1)
        append(q_sh, tab, sh.gen, *sh.layer(0), H, D, rope_pos=sh.apos)
        sh.gen.add_(1)
        sh.apos.add_(1)
        assert torch.equal(q_ref, q_sh) and not torch.equal(q_ref[:, :2 * d], qkv0[:, :2 * d])
        if t == 2:
            local = torch.randint(0, nb, (Bp, 1), generator=g).repeat(1, nb)
        elif t == 4:
            local = torch.arange(nb).repeat(Bp, 1)
        else:
            local = torch.randint(0, nb, (Bp, nb), generator=g)
        beam_idx = in_group(local, nb)
        eng.reorder_cache(exp, beam_idx, Pmax + t + 1)
        sh.reorder(beam_idx)
        mat = sh.materialize()
        assert mat.B == n and mat.Smax == Pmax + G and mat.lens.tolist() == exp.lens.tolist()
        for m in range(n):
            v = pre_lens[m // nb] + t + 1
            for a, b in zip(mat.sets()[:2], exp.sets()[:2]):
                assert (same_fp8(a[0][m, :v].cpu(), b[0][m, :v].cpu()) if fp8 else torch.equal(a[0][m, :v], b[0][m, :v])), (t, m)
            for a, b in zip(mat.sets()[2:], exp.sets()[2:]):
                assert torch.equal(a[0][m, :, :v], b[0][m, :, :v]), (t, m)
    assert [t.data_ptr() for lst in sh.prefix.sets() for t in lst] == ptrs
    for t, t0 in zip([t for lst in c0.sets() for t in lst], before):
        assert torch.equal(t, t0)
    assert bool((c0.k[0][0, pre_lens[0]:] == (FILL8 if fp8 else FILL16)).all())
    for t in sh.k + sh.v:
        assert bool((t[:, steps:] == (FILL8 if fp8 else FILL16)).all()) and not bool((t[:, :steps] == (FILL8 if fp8 else FILL16)).all())
    if fp8:
        for t in sh.ks + sh.vs:
            assert bool((t[:, :, steps:] == FILLS).all()) and not bool((t[:, :, :steps] == FILLS).any())


def test_beam_ancestry_kernel_alone(O):
    """anc_out[m, :gen[m]] = anc_in[beam_idx[m], :gen[m]] and anc_out[m, gen[m]] = m, with a different gen per row (0, G - 1 and G among
    them: a full row gets no own-row entry, nothing is written behind it); entries beyond gen are not compared.  Then the restatement of
    tests/test_beams_cpu.py over a sequence of steps on two swapped buffers."""
    rows, G = 12, 9
    g = torch.Generator().manual_seed(2)
    anc_in = torch.randint(0, rows, (rows, G), generator=g, dtype=torch.int32).to(dev())
    buf = torch.full((rows + 1, G), -7, dtype=torch.int32, device=dev())
    gen = torch.tensor([0, G - 1, G, 3, 1, 8, 5, 2, 7, 4, 6, 3], dtype=torch.int32, device=dev())
    beam_idx = torch.randint(0, rows, (rows,), generator=g).to(dev())
    O.beam_ancestry(anc_in, buf[:rows], beam_idx, gen)
    want = anc_in[beam_idx]
    for m in range(rows):
        n = int(gen[m])
        assert torch.equal(buf[m, :n], want[m, :n]), m
        assert n == G or int(buf[m, n]) == m
        assert bool((buf[m, n + 1:] == -7).all())
    assert bool((buf[rows] == -7).all())
    Bp, nb = 2, 5
    n = Bp * nb
    a = torch.arange(n, dtype=torch.int32, device=dev())[:, None].repeat(1, G).contiguous()
    b = a.clone()
    ref = a.tolist()
    for t in range(G - 1):
        idx = in_group(torch.randint(0, nb, (Bp, nb), generator=g), nb)
        O.beam_ancestry(a, b, idx, torch.full((n,), t, dtype=torch.int32, device=dev()))
        a, b = b, a
        ref = ancestry_step(ref, idx.tolist(), t)
        assert [r[:t + 1] for r in a.tolist()] == [r[:t + 1] for r in ref]


# ---- attention ---------------------------------------------------------------------------------------------------------------------------
# (Bp, nb, H, D, Pmax, pre_lens, G, gen): one beam, one prompt key, only its own suffix key; TQ = 8 with several prefix splits, a full suffix
# and two prompts of different length; TQ = 4; the full MFMA tile; 9 queries in the 16-wide form at the first step; "straddle": pre_lens =
# [c, c + 1], c the prefix chunk of mh_attn_decode_beams_splits - a split exactly full, and one with a single key
# G = 600: the suffix part's key splits (3 of 200 keys) - all of them full (gen = 599); one full, one with a single key and one empty
# (gen = 200); the same at D = 128 with two prompts, so that the rows of the second prompt's beams lie behind the first's
# gen as a list, one per beam: 63 / 64 / 65 suffix keys at D = 128 and 127 / 128 / 129 at D = 64 - one unrolled iteration of the suffix
# kernel (256 * 8 / D key slices x 4 rows in flight) less one key, exactly, and plus one - in one suffix split and in the first of two
BEAM_ATTN_CASES = [(1, 1, 2, 128, 40, [1], 4, 0), (2, 5, 4, 64, 700, [1, 690], 16, 15), (1, 3, 2, 128, 300, [299], 8, 3),
                   (1, 16, 2, 128, 600, [590], 8, 7), (1, 9, 2, 64, 300, [290], 8, 0), (2, 5, 4, 64, 700, "straddle", 16, 5),
                   (1, 5, 2, 64, 300, [290], 600, 599), (1, 5, 2, 64, 300, [290], 600, 200), (2, 3, 2, 128, 40, [3, 40], 600, 200),
                   (1, 3, 2, 128, 40, [40], 130, [62, 63, 64]), (1, 3, 2, 128, 40, [40], 260, [62, 63, 64]),
                   (1, 3, 2, 64, 40, [40], 130, [126, 127, 128]), (1, 3, 2, 64, 40, [40], 258, [126, 127, 128])]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Bp,nb,H,D,Pmax,pre_lens,G,gen", BEAM_ATTN_CASES)
def test_attn_decode_beams_per_element(O, dtype, Bp, nb, H, D, Pmax, pre_lens, G, gen):
    """Query m is held to N.attention_decode(q[m], k64[m], v64[m], n_m) on the MATERIALISED per-beam keys and values (its prompt's valid
    prefix rows, then suffix rows anc[m, g] for g <= gen) with the limit of the rounding model (hold()): the fp8 kernel on the fp8 cache,
    the 16-bit kernel on the exactly cast dequantised cache.  Every suffix slot no beam references and every prefix row at or beyond
    pre_lens holds NaN (fp8: 0x7F bytes and NaN scales): one row too many, or the wrong beam's row, fails loudly."""
    psplits, ssplits = O.attn_decode_beams_splits(Bp, nb, H, Pmax, G)
    assert psplits >= 1 and ssplits == min((G + 255) // 256, 4) and psplits + ssplits <= 32  # (ceil(G / 256) suffix splits, 4 at the most)
    if pre_lens == "straddle":
        c = (Pmax + psplits - 1) // psplits
        assert psplits > 2 and c + 1 <= Pmax
        pre_lens = [c, c + 1]
    d, n = H * D, Bp * nb
    gens = gen if isinstance(gen, list) else [gen] * n  # the suffix keys of beam m are g <= gens[m]
    assert len(gens) == n
    q = rnd_rows(n * H, D, dtype, seed=5, lo=0.5, hi=2.0).view(n, d).to(dev())
    g = torch.Generator().manual_seed(17)
    anc = torch.randint(0, nb, (Bp, nb, G), generator=g) + nb * torch.arange(Bp)[:, None, None]
    anc = anc.view(n, G).to(torch.int32)
    anc[torch.arange(n), torch.tensor(gens)] = torch.arange(n, dtype=torch.int32)  # the new key is the beam's own
    if nb > 1 and min(gens) > 0:
        anc[1::nb, 0] = anc[0::nb, 0]                 # two beams of every prompt share an ancestor row
        assert int(anc[1, 0]) == int(anc[0, 0])
    used = torch.zeros(n, G, dtype=torch.bool)
    for m in range(n):
        used[anc[m, :gens[m] + 1].long(), torch.arange(gens[m] + 1)] = True
    valid = torch.arange(Pmax)[None, :] < torch.tensor(pre_lens)[:, None]
    fmt = {}
    for name, rows, S, keep, seeds in (("pre", Bp, Pmax, valid, (3, 4)), ("suf", n, G, used, (8, 9))):
        for kv, seed in zip("kv", seeds):
            c8, cs = kv8_quantize(rnd_rows(rows * S * H, D, dtype, seed=seed).view(rows, S, H, D))
            x64 = kv8_dequantize(c8, cs)
            x16 = x64.to(dtype)
            assert torch.equal(x16.double(), x64)  # the cast to the 16-bit type is exact
            c8, cs, x16 = c8.view(rows, S, d).clone(), cs.permute(0, 2, 1).contiguous(), x16.view(rows, S, d).clone()
            x16[~keep] = float("nan")
            c8[~keep] = 0x7F
            cs.permute(0, 2, 1)[~keep] = float("nan")
            fmt[name + kv] = (c8.to(dev()), cs.to(dev()), x16.to(dev()), x64.to(dev()))
    rows = []
    for m in range(n):
        p, sl = m // nb, gens[m] + 1
        pick = anc[m, :sl].long().to(dev())
        k64 = torch.cat([fmt["prek"][3][p, :pre_lens[p]], fmt["sufk"][3][pick, torch.arange(sl, device=dev())]])
        v64 = torch.cat([fmt["prev"][3][p, :pre_lens[p]], fmt["sufv"][3][pick, torch.arange(sl, device=dev())]])
        assert not bool(torch.isnan(k64).any() | torch.isnan(v64).any())
        qm = q[m].view(H, D)
        rows.append(N.attention_decode(qm, k64, v64, k64.shape[0]) + (N.attention_decode(qm, k64, v64, k64.shape[0], model=dtype),))
    ref, Bc, mod = (torch.stack([r[i] for r in rows]) for i in range(3))
    pl = torch.tensor(pre_lens, dtype=torch.int32, device=dev())
    slens = torch.tensor([g_ + 1 for g_ in gens], dtype=torch.int32, device=dev())
    anc_d = anc.to(dev())
    tag = f"Bp={Bp} nb={nb} D={D} Pmax={Pmax} pre_lens={pre_lens} G={G} gen={gen} splits={psplits}+{ssplits}"
    o = O.attn_decode_beams_kv8(q, fmt["prek"][0], fmt["prev"][0], fmt["prek"][1], fmt["prev"][1], pl, fmt["sufk"][0], fmt["sufv"][0],
                                fmt["sufk"][1], fmt["sufv"][1], anc_d, slens, nb, H, D)
    hold(f"attention decode beams kv8 {tag}", dtype, o.view(n, H, D), ref, Bc, mod)
    o = O.attn_decode_beams(q, fmt["prek"][2], fmt["prev"][2], pl, fmt["sufk"][2], fmt["sufv"][2], anc_d, slens, nb, H, D)
    hold(f"attention decode beams 16-bit {tag}", dtype, o.view(n, H, D), ref, Bc, mod)


def test_attn_decode_beams_refuses_a_prompt_beyond_its_split_plan(O):
    """include/merlin_hip.h: 16 beams (the 16-query form: 2400 keys of scores per block at 150 KiB) and G = 8 (one suffix split, so 31 prefix
    splits) take Pmax up to 31 * 2400 = 74 400; one key more has no plan and the launch is refused with an error code."""
    from merlin_amd._lib import MerlinHipError

    nb, H, D, G, lim = 16, 1, 64, 8, 31 * 2400
    assert O.attn_decode_beams_splits(1, nb, H, lim, G) == (31, 1) and O.attn_decode_beams_splits(1, nb, H, lim + 1, G) == (0, 1)
    Pmax = lim + 1
    q = torch.zeros(nb, H * D, dtype=torch.float16, device=dev())
    pre = torch.zeros(1, Pmax, H * D, dtype=torch.float16, device=dev())
    suf = torch.zeros(nb, G, H * D, dtype=torch.float16, device=dev())
    anc = torch.arange(nb, dtype=torch.int32, device=dev())[:, None].repeat(1, G).contiguous()
    one = torch.ones(nb, dtype=torch.int32, device=dev())
    with pytest.raises(MerlinHipError, match="shape"):
        O.attn_decode_beams(q, pre, pre, one[:1], suf, suf, anc, one, nb, H, D)
    pre8, suf8 = pre.view(torch.uint8)[..., :H * D].contiguous(), suf.view(torch.uint8)[..., :H * D].contiguous()
    ps, ss = torch.ones(1, H, Pmax, device=dev()), torch.ones(nb, H, G, device=dev())
    with pytest.raises(MerlinHipError, match="shape"):
        O.attn_decode_beams_kv8(q, pre8, pre8, ps, ps, one[:1], suf8, suf8, ss, ss, anc, one, nb, H, D)


# ---- engine ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("name,kv8,w", ENGINE_CONFIGS)
def test_beam_steps_on_the_shared_cache_reproduce_the_expanded_cache(dtype, name, kv8, w):
    """One multimodal golden prompt, nb = 3, four beam steps (re-order, then decode_step, as _beam_search does) with a fixed beam_idx
    schedule and fixed tokens: (a) on the expanded cache (expand_cache + reorder_cache, the existing path), (b) on the shared cache.  Same
    math, another summation order in the attention: the situation and the criterion of test_spec_gpu.py's
    test_verify_step_reproduces_sequential_decode_steps - dev(b, a) <= 2 max(d_pre, d_rows) and <= tight = 2 max(d_pre16, d_rows), all
    measured in this run on path (a) alone: d_pre = dev(full-sequence forward() logits of every beam's token history, a), d_rows =
    dev(one-row decode_steps along the lineage of the last step's beam 0, a's rows of that lineage), d_pre16 = d_pre of the same run with
    16-bit weights."""
    cfg, m, ids, images = tiny(dtype)
    eng = m.engine
    V, P, nb, S = cfg.vocab_size, ids.shape[1], 3, 4
    g = torch.Generator().manual_seed(11)
    toks = torch.randint(3, V, (S, nb), generator=g).cuda()
    schedule = [[0, 1, 2], [1, 1, 0], [2, 0, 0], [0, 2, 1]]
    rows3 = torch.zeros(nb, dtype=torch.int64, device=ids.device)

    def expanded(**ww):
        _, c0 = eng.prefill(ids, None, images, S + 2, kv_fp8=kv8)
        c = eng.expand_cache(c0, rows3)
        out = []
        for t in range(S):
            eng.reorder_cache(c, torch.tensor(schedule[t], device=ids.device), P + t)
            out.append(eng.decode_step(toks[t], c, **ww).clone())
        return out

    a = expanded(**w)
    _, c0 = eng.prefill(ids, None, images, S + 2, kv_fp8=kv8)
    sh = eng.share_cache(c0, nb, S + 2)
    b = []
    for t in range(S):
        sh.reorder(torch.tensor(schedule[t], device=ids.device))
        b.append(eng.decode_step(toks[t], sh, **w).clone())
    assert sh.gen.tolist() == [S] * nb and sh.apos.tolist() == [P + S] * nb and int(c0.lens[0]) == P
    # every beam's token history and the rows it lived in, replayed on the host
    hist, lineage, per_step = [[] for _ in range(nb)], [[] for _ in range(nb)], []
    for t in range(S):
        hist = [hist[s] + [int(toks[t, i])] for i, s in enumerate(schedule[t])]
        lineage = [lineage[s] + [i] for i, s in enumerate(schedule[t])]
        per_step.append([list(h) for h in hist])
    with torch.no_grad():
        full = [torch.cat([m(input_ids=torch.cat([ids, torch.tensor([h], device=ids.device)], dim=1), images=images).logits[:, -1].float()
                           for h in per_step[t]]) for t in range(S)]
    d_pre = _dev(full, a, V)
    d_pre16 = _dev(full, expanded(), V) if w else d_pre
    _, c1 = eng.prefill(ids, None, images, S + 2, kv_fp8=kv8)
    one = [eng.decode_step(torch.tensor([tk], device=ids.device), c1, **w).clone() for tk in hist[0]]
    d_rows = _dev(one, [a[t][r:r + 1] for t, r in enumerate(lineage[0])], V)
    d_ba = _dev(b, a, V)
    bound, tight = 2 * max(d_pre, d_rows), 2 * max(d_pre16, d_rows)
    print(f"BEAMS | {name} | {str(dtype)[6:]} | d_pre16 = {d_pre16:.3e} | tight = {tight:.3e} | d_pre = {d_pre:.3e} | d_rows = {d_rows:.3e} | "
          f"dev(b, a) = {d_ba:.3e} | bound = {bound:.3e}")
    assert d_ba <= bound, (d_ba, bound)
    assert d_ba <= tight, (d_ba, tight)


# ---- generate() --------------------------------------------------------------------------------------------------------------------------
def _gold():
    from test_generation_gpu import GOLD

    return GOLD


@pytest.mark.parametrize("i", range(len(_gold()["beam_cases"])))
def test_shared_beam_search_matches_transformers(i):
    from test_generation_gpu import _model

    rec = _gold()["beam_cases"][i]
    cfg, batch, m = _model("tiny_1img", rec["logit_gain"])
    ids = torch.tensor(rec["prompt"], dtype=torch.int64).cuda()
    got = m.generate(ids, max_new_tokens=rec["max_new_tokens"], num_beams=rec["num_beams"], length_penalty=rec["length_penalty"],
                     eos_token_id=rec["eos_token_id"], pad_token_id=0, temperature=0.2, share_prompt_kv=True).cpu()
    assert got.tolist() == rec["beam"], (got.tolist(), rec["beam"])


def test_shared_eval_style_multimodal_beam_call_vs_oracle():
    """eval_mmvet.py's `num_beams=5, temperature=0.2, stopping_criteria=[...]` call on a multimodal prompt with share_prompt_kv=True,
    against the oracle's beam search over the fp32 oracle forward; the criteria see the (1 + n_eos) * num_beams candidates."""
    from oracle import gen_ref as G
    from test_generation_gpu import _model, _oracle_fn

    gain, eos = 25.0, 96
    cfg, batch, m = _model("tiny_1img", gain)
    fn = _oracle_fn(cfg, gain, batch["images"])
    ids_cpu = batch["input_ids"][:, :22]
    images = [im.cuda() for im in batch["images"]]
    calls = []

    class Keyword:
        def __call__(self, output_ids, scores, **kw):
            calls.append(tuple(output_ids.shape))
            return bool((output_ids[0, 22:] == -5).any())

    got = m.generate(ids_cpu.cuda(), images=images, num_beams=5, temperature=0.2, max_new_tokens=16, eos_token_id=eos, pad_token_id=0,
                     stopping_criteria=[Keyword()], share_prompt_kv=True).cpu()
    want = G.beam_search(fn, ids_cpu, 5, 16, eos_ids=[eos], pad=0)
    assert got.tolist() == want.tolist(), (got.tolist(), want.tolist())
    assert calls and calls[0] == (10, 23)


def test_two_prompts_in_one_batch_equal_each_prompt_alone():
    from test_generation_gpu import _model

    rec = _gold()["beam_cases"][0]
    cfg, batch, m = _model("tiny_1img", rec["logit_gain"])
    one = torch.tensor(rec["prompt"], dtype=torch.int64)
    ids = torch.cat([one, one.flip(1)]).cuda()  # two text-only prompts of equal length
    kw = dict(max_new_tokens=8, num_beams=3, eos_token_id=-1, pad_token_id=0, share_prompt_kv=True)
    both = m.generate(ids, **kw).cpu()
    assert both.shape == (2, ids.shape[1] + 8) and not torch.equal(both[0], both[1])
    for b in range(2):
        alone = m.generate(ids[b:b + 1], **kw).cpu()
        assert both[b:b + 1].tolist() == alone.tolist(), (b, both[b].tolist(), alone.tolist())


@pytest.mark.parametrize("flags", [dict(fp8_kv=True), dict(fp8_weights=True), dict(fp4_weights=True)], ids=lambda f: next(iter(f)))
def test_sharing_composes_with_cache_and_weight_formats(flags):
    cfg, m, ids, images = tiny(torch.float16)
    kw = dict(images=images, max_new_tokens=8, num_beams=5, eos_token_id=-1, pad_token_id=0, **flags)
    runs = [m.generate(ids, share_prompt_kv=True, **kw) for _ in range(2)]
    assert torch.equal(runs[0], runs[1]) and runs[0].shape[1] > ids.shape[1]
    if flags.get("fp8_kv"):
        plain = m.generate(ids, **kw)
        assert runs[0].tolist() == plain.tolist(), (runs[0].tolist(), plain.tolist())


@pytest.mark.parametrize("fp8_kv", [False, True], ids=["kv16", "kv8"])
def test_shared_run_copies_no_prompt_kv(monkeypatch, fp8_kv):
    """During generate(share_prompt_kv=True) expand_cache and reorder_cache are never called, the prefix tensors are the prefill's own
    (same data_ptr() at the last step), and cache.nbytes is the prefix plus nb x G suffix rows exactly - less than the expanded cache
    with its second buffer set."""
    cfg, m, ids, images = tiny(torch.float16)
    eng = m.engine
    nb, G = 5, 8
    seen = {}
    prefill, share = eng.prefill, eng.share_cache

    def spy_prefill(*a, **kw):
        logits, c = prefill(*a, **kw)
        seen["c0"], seen["ptrs"] = c, [t.data_ptr() for lst in c.sets() for t in lst]
        return logits, c

    def spy_share(c, *a):
        seen["sh"] = share(c, *a)
        return seen["sh"]

    def never(*a, **kw):
        raise AssertionError("the shared path copied or gathered K/V")

    expand = eng.expand_cache
    monkeypatch.setattr(eng, "prefill", spy_prefill)
    monkeypatch.setattr(eng, "share_cache", spy_share)
    monkeypatch.setattr(eng, "expand_cache", never)
    monkeypatch.setattr(eng, "reorder_cache", never)
    out = m.generate(ids, images=images, max_new_tokens=G, num_beams=nb, eos_token_id=-1, pad_token_id=0, share_prompt_kv=True, fp8_kv=fp8_kv)
    assert out.shape[1] > ids.shape[1]
    c0, sh = seen["c0"], seen["sh"]
    assert sh.prefix is c0 and [t.data_ptr() for lst in sh.prefix.sets() for t in lst] == seen["ptrs"]
    assert int(sh.gen[0]) >= 1 and sh.G == G and sh.fp8 == fp8_kv
    assert c0.Smax == ids.shape[1]  # the prefix was prefilled without spare rows: it holds the prompt and nothing else
    H, d, layers = cfg.num_attention_heads, cfg.hidden_size, len(c0.k)
    row = 2 * d * (1 if fp8_kv else 2) + (2 * H * 4 if fp8_kv else 0)  # K and V of one token, and their scales
    assert sh.nbytes == c0.nbytes + layers * ids.shape[0] * nb * G * row
    ex = expand(c0, torch.arange(ids.shape[0], device=ids.device).repeat_interleave(nb))
    assert ex.nbytes == nb * c0.nbytes and sh.nbytes < 2 * ex.nbytes  # (reorder_cache keeps a second set of the same size: *_alt)
