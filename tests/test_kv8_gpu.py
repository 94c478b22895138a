"""fp8 KV cache of generate(): the quantising kernels against the torch restatement of the format (tests/test_kv8_cpu.py) bit for bit, the
decode attention on the fp8 cache against the fp64 reference evaluated on the DEQUANTISED cache (tests/numerics.py: the rule the 16-bit
kernel is held to, so quantisation error is not part of it), and the engine / generate() paths on the tiny fixture of
tests/test_generation_gpu.py."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import numerics as N  # noqa: E402
from test_kv8_cpu import kv8_dequantize, kv8_quantize  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
# (B, H, D, Smax, lens) of test_decode_rope_append_and_attention: no split; 6 splits of 117 keys with a length-1 sequence and D = 64; 32 splits
SHAPES = [(2, 2, 128, 40, [17, 40]), (3, 4, 64, 700, [1, 333, 700]), (1, 32, 128, 4200, [4100])]
F8 = torch.float8_e4m3fn


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from merlin_amd import ops as O

    assert O.arch_ok(0), "not a gfx950 device"
    return O


def rnd_rows(rows, cols, dtype, seed, lo=1e-2, hi=10.0):
    """[rows, cols] normal values whose rows are scaled log-uniformly between lo and hi (row maxima ~1e-2 .. 30), on the CPU."""
    g = torch.Generator().manual_seed(seed + rows + cols)
    mag = torch.exp(torch.rand(rows, 1, generator=g) * (math.log(hi) - math.log(lo)) + math.log(lo))
    return (torch.randn(rows, cols, generator=g) * mag).to(dtype)


def same_fp8(a, b):
    """Two uint8 tensors compared as e4m3 values."""
    return torch.equal(a.view(F8).float(), b.view(F8).float())


def patterned(B, Smax, H, D):
    """A cache that is nowhere zero: bytes 0x2B, scales 7."""
    d = H * D
    mk = lambda: (torch.full((B, Smax, d), 0x2B, dtype=torch.uint8, device=dev()), torch.full((B, H, Smax), 7.0, device=dev()))  # noqa: E731
    return mk() + mk()


# ---- quantisers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,S,H,D,Smax", [(2, 17, 2, 128, 40), (3, 333, 4, 64, 700), (2, 40, 2, 128, 40), (1, 130, 32, 128, 131)])
def test_kv8_fill_matches_the_format(ops, dtype, B, S, H, D, Smax):
    """Prefill quantiser on the k and the v section of a fused q|k|v buffer (ldx = 3 H D): bytes and scales of rows [:, :S] equal the
    restatement's, every other byte and scale keeps its pattern."""
    d = H * D
    qkv_c = rnd_rows(B * S * 3 * H, D, dtype, seed=1).view(B * S, 3 * d)
    qkv_c[1, d:d + D] = 0  # an all-zero group
    qkv = qkv_c.to(dev())
    k8, ks, v8, vs = patterned(B, Smax, H, D)
    for sec, c8, cs in ((1, k8, ks), (2, v8, vs)):
        x = qkv[:, sec * d:(sec + 1) * d]
        assert x.stride(0) == 3 * d
        ops.kv8_fill(x, c8, cs, B, S, H, D)
        q_ref, s_ref = kv8_quantize(qkv_c[:, sec * d:(sec + 1) * d].reshape(B, S, H, D))
        assert same_fp8(c8[:, :S].cpu(), q_ref.view(B, S, d))
        assert torch.equal(cs[:, :, :S].cpu(), s_ref.permute(0, 2, 1))
        assert bool((c8[:, S:] == 0x2B).all()) and bool((cs[:, :, S:] == 7.0).all())
    assert float(ks[0, 0, 1]) == 1.0  # the all-zero group (row 1, head 0 of k): e = 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("B,H,D,Smax,lens", SHAPES)
def test_decode_rope_append_kv8(ops, dtype, B, H, D, Smax, lens, shift):
    """qkv is left exactly as mh_decode_rope_append leaves it; row pos[b] of the fp8 cache is the restatement applied to the 16-bit k row
    that kernel appends and to the v row as it lies in qkv; nothing else is written.  shift = 3: rope_pos != pos."""
    d = H * D
    qkv0 = rnd_rows(B * 3 * H, D, dtype, seed=5).view(B, 3 * d).to(dev())
    pos = torch.tensor([n - 1 for n in lens], dtype=torch.int32, device=dev())
    rpos = (pos + shift) if shift else None
    tab = ops.rope_table(Smax + 8, D, 10000.0, dev())
    kc, vc = torch.zeros(B, Smax, d, dtype=dtype, device=dev()), torch.zeros(B, Smax, d, dtype=dtype, device=dev())
    qkv16 = qkv0.clone()
    ops.decode_rope_append(qkv16, tab, pos, kc, vc, H, D, rope_pos=rpos)
    if shift:  # the position really moved the rotation
        q_at_pos = qkv0.clone()
        ops.decode_rope_append(q_at_pos, tab, pos, kc.clone(), vc.clone(), H, D)
        assert not torch.equal(q_at_pos, qkv16)
    k8, ks, v8, vs = patterned(B, Smax, H, D)
    qkv = qkv0.clone()
    ops.decode_rope_append_kv8(qkv, tab, pos, k8, v8, ks, vs, H, D, rope_pos=rpos)
    assert torch.equal(qkv, qkv16)
    assert torch.equal(qkv[:, 2 * d:], qkv0[:, 2 * d:])
    for b in range(B):
        p = lens[b] - 1
        for c8, cs, row in ((k8, ks, kc[b, p]), (v8, vs, qkv0[b, 2 * d:])):
            q_ref, s_ref = kv8_quantize(row.cpu().view(H, D))
            assert same_fp8(c8[b, p].cpu(), q_ref.view(d)) and torch.equal(cs[b, :, p].cpu(), s_ref)
            keep = torch.ones(Smax, dtype=torch.bool, device=dev())
            keep[p] = False
            assert bool((c8[b][keep] == 0x2B).all()) and bool((cs[b][:, keep] == 7.0).all())


# ---- attention ---------------------------------------------------------------------------------------------------------------------------
def hold(name, dtype, got, ref, B, model):
    """The model's c and the kernel's c against the same reference and B; kernel <= limit(model) (tests/test_componentwise_gpu.py)."""
    cm, _ = N.componentwise(model, ref, B, N.EPS16[dtype], N.TINY[dtype])
    ck, at = N.componentwise(got, ref, B, N.EPS16[dtype], N.TINY[dtype])
    lim = N.limit(cm)
    print(f"CW | {name} | {str(dtype)[6:]} | {cm:.3f} | {ck:.3f} | {lim:.3f} | worst at {at}")
    assert ck <= lim, f"{name} {dtype}: kernel c = {ck:.3f} at {at} exceeds {lim:.3f} (model c = {cm:.3f})"


def _chunk(B, H, Smax):
    from merlin_amd import _lib as L

    splits = int(L.lib().mh_attn_decode_splits(B, H, Smax))
    return (Smax + splits - 1) // splits


# SHAPES, and (6 splits of 117 keys) lengths that are whole chunks of the split plan / whole chunks plus one key
# lengths around one unrolled iteration of the one-query kernel (256 * 8 / D key slices x 4 rows in flight with the 16-bit cache, x 8 with
# the fp8 cache: 64 and 128 keys at D = 128, 128 and 256 at D = 64), and fewer keys than key slices (16 at D = 128, 32 at D = 64)
ATTN_CASES = SHAPES + [(2, 4, 64, 700, "chunk"), (2, 4, 64, 700, "chunk+1"),
                       (3, 2, 128, 130, [63, 64, 65]), (3, 2, 128, 130, [127, 128, 129]), (3, 2, 64, 260, [127, 128, 129]),
                       (3, 2, 64, 260, [255, 256, 257]), (3, 2, 128, 40, [1, 5, 15]), (3, 2, 64, 40, [1, 5, 31])]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,D,Smax,lens", ATTN_CASES)
def test_attn_decode_kv8_per_element(ops, dtype, B, H, D, Smax, lens):
    """Held to the fp64 reference on the dequantised cache, with the limit of the rounding model on the same inputs - split-KV and one
    block per (b, h) - and so is the 16-bit kernel run on the dequantised cache cast to the 16-bit type (an exact cast)."""
    if isinstance(lens, str):
        ch = _chunk(B, H, Smax)
        assert 3 * ch + 1 <= Smax
        lens = [2 * ch, 3 * ch] if lens == "chunk" else [2 * ch + 1, 3 * ch + 1]
    d = H * D
    q = rnd_rows(B * H, D, dtype, seed=5, lo=0.5, hi=2.0).view(B, d).to(dev())
    cache = []
    for seed in (3, 4):
        c8, cs = kv8_quantize(rnd_rows(B * Smax * H, D, dtype, seed=seed).view(B, Smax, H, D))
        cache += [c8.view(B, Smax, d).to(dev()), cs.permute(0, 2, 1).contiguous().to(dev()), kv8_dequantize(c8, cs).to(dev())]
    k8, ks, k64, v8, vs, v64 = cache
    k16, v16 = k64.to(dtype), v64.to(dtype)
    assert torch.equal(k16.double(), k64) and torch.equal(v16.double(), v64)  # the cast to the 16-bit type is exact
    pairs = [N.attention_decode(q[b].view(H, D), k64[b], v64[b], lens[b]) for b in range(B)]
    ref, Bc = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    mod = torch.stack([N.attention_decode(q[b].view(H, D), k64[b], v64[b], lens[b], model=dtype) for b in range(B)])
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev())
    tag = f"Smax={Smax} lens={lens}"
    for split in (True, False):
        o = ops.attn_decode_kv8(q, k8, v8, ks, vs, lens_t, H, D, split_kv=split)
        hold(f"attention decode kv8 {'split-KV' if split else 'one block'} {tag}", dtype, o.view(B, H, D), ref, Bc, mod)
    for split in (True, False):
        o16 = ops.attn_decode(q, k16.view(B, Smax, d), v16.view(B, Smax, d), lens_t, H, D, split_kv=split)
        hold(f"attention decode 16-bit on the dequantised cache {'split-KV' if split else 'one block'} {tag}", dtype, o16.view(B, H, D), ref, Bc, mod)


# ---- engine and generate() -----------------------------------------------------------------------------------------------------------------
GAIN = 25.0


def _tiny(dtype):
    from test_generation_gpu import _model

    cfg, batch, m = _model("tiny_1img", GAIN, dtype)
    ids = batch["input_ids"][:, :22].cuda()
    images = [im.cuda() for im in batch["images"]]
    return cfg, m, ids, images


def _emulate_rows(cache, H, D, lo, hi):
    """Rows [lo, hi) of every layer of a 16-bit cache <- their quantise -> dequantise values (the restatement, on the CPU)."""
    for t in cache.k + cache.v:
        rows = t[:, lo:hi]
        q, s = kv8_quantize(rows.cpu().view(rows.shape[0], hi - lo, H, D))
        rows.copy_(kv8_dequantize(q, s).view(rows.shape).to(t.dtype))


def _dev(x, y, V):
    """Relative L2 distance of the V valid logits, worst over steps and rows."""
    return max(float(((a[:, :V] - b[:, :V]).double().norm(dim=1) / b[:, :V].double().norm(dim=1)).max()) for a, b in zip(x, y))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_engine_fp8_cache_prefill_size_and_teacher_forced_deviation(dtype):
    """Prefill logits do not change; the fp8 cache is (1 + 4/D) / 2 of the 16-bit one; fed the same 8 tokens, the fp8 path (b) deviates from
    the 16-bit path (a) by no more than twice what the format costs - measured in the same run by the emulation (c): the 16-bit path whose
    cache rows are overwritten with their quantise -> dequantise values as they are written - and lies closer to (c) than (c) lies to (a)."""
    cfg, m, ids, images = _tiny(dtype)
    eng = m.engine
    H, V = cfg.num_attention_heads, cfg.vocab_size
    D = cfg.hidden_size // H
    steps = 8
    la, ca = eng.prefill(ids, None, images, steps + 1)
    la = la.clone()
    lb, cb = eng.prefill(ids, None, images, steps + 1, kv_fp8=True)
    lb = lb.clone()
    lc, cc = eng.prefill(ids, None, images, steps + 1)
    assert torch.equal(la, lb)
    assert cb.fp8 and cb.k[0].dtype == torch.uint8 and cb.ks[0].shape == (ids.shape[0], H, cb.Smax)
    assert cb.nbytes * 2 * D == ca.nbytes * (D + 4), (cb.nbytes, ca.nbytes)
    n0 = int(ca.lens[0])
    assert bool((ca.lens == n0).all()) and torch.equal(ca.lens, cb.lens)
    _emulate_rows(cc, H, D, 0, n0)
    g = torch.Generator().manual_seed(11)
    toks = torch.randint(3, V, (steps, ids.shape[0]), generator=g).cuda()
    outs = {"a": [], "b": [], "c": []}
    for t in range(steps):
        outs["a"].append(eng.decode_step(toks[t], ca).clone())
        outs["b"].append(eng.decode_step(toks[t], cb).clone())
        outs["c"].append(eng.decode_step(toks[t], cc).clone())
        _emulate_rows(cc, H, D, n0 + t, n0 + t + 1)
    d_ba, d_ca, d_bc = _dev(outs["b"], outs["a"], V), _dev(outs["c"], outs["a"], V), _dev(outs["b"], outs["c"], V)
    print(f"KV8 | {str(dtype)[6:]} | dev(fp8, 16-bit) = {d_ba:.3e} | dev(emulation, 16-bit) = {d_ca:.3e} | dev(fp8, emulation) = {d_bc:.3e}")
    assert d_ba > 0
    assert d_ba <= 2 * d_ca, (d_ba, d_ca)
    assert d_bc <= d_ca, (d_bc, d_ca)


@pytest.mark.parametrize("dtype", DTYPES)
def test_generate_fp8_kv_graph_sampling_beams_and_fp8_weights(dtype):
    """generate(fp8_kv=True): graph replay equals eager decoding for greedy and seeded sampling, beam search and the fp8-weights
    combination are reproducible, and use_cache=False is refused."""
    cfg, m, ids, images = _tiny(dtype)
    kw = dict(images=images, max_new_tokens=8, eos_token_id=-1, pad_token_id=0, fp8_kv=True)
    for mode in (dict(), dict(do_sample=True, temperature=0.8, seed=4242)):
        eager = m.generate(ids, use_graph=False, **kw, **mode)
        graph = m.generate(ids, use_graph=True, **kw, **mode)
        assert eager.shape[1] == ids.shape[1] + 8 and torch.equal(eager, graph), (mode, eager.tolist(), graph.tolist())
    beams = [m.generate(ids, num_beams=3, **kw) for _ in range(2)]
    assert torch.equal(beams[0], beams[1]) and beams[0].shape[1] > ids.shape[1]
    both = [m.generate(ids, fp8_weights=True, **kw) for _ in range(2)]
    assert torch.equal(both[0], both[1]) and both[0].shape[1] == ids.shape[1] + 8
    with pytest.raises(ValueError):
        m.generate(ids, use_cache=False, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_left_padded_prompts_fill_and_append_the_fp8_cache(dtype):
    """A left-padded batch goes through the prefill's unpad path: the cache keeps the valid keys only and the next token is rotated at
    the padded length (cache.rpos != cache.lens).  The fp8 cache then holds exactly the restatement of the 16-bit cache's valid rows in
    every layer, one decode step appends the restatement of the 16-bit layer-0 row (the only layer whose new row does not depend on
    the cache), and generate(fp8_kv=True) on the padded batch replays from a graph what it decodes eagerly."""
    from test_generation_gpu import _model

    cfg, batch, m = _model("tiny_2img", GAIN, dtype)
    eng = m.engine
    H = cfg.num_attention_heads
    D = cfg.hidden_size // H
    full = batch["input_ids"]
    prompts = [full[0], full[0, :full.shape[1] - 5]]  # two prompts of different lengths over the same image
    P = full.shape[1]
    ids = torch.zeros(2, P, dtype=torch.int64)
    am = torch.zeros(2, P, dtype=torch.bool)
    for i, p in enumerate(prompts):
        ids[i, P - p.numel():], am[i, P - p.numel():] = p, True
    ids, am = ids.cuda(), am.cuda()
    images = [batch["images"][0].cuda()] * 2
    la, ca = eng.prefill(ids, am, images, 4)
    la = la.clone()
    lb, cb = eng.prefill(ids, am, images, 4, kv_fp8=True)
    assert torch.equal(la, lb)
    assert ca.rpos is not None and torch.equal(ca.rpos, cb.rpos) and torch.equal(ca.lens, cb.lens)
    lens = [int(n) for n in ca.lens]
    assert lens == [P, P - 5] and int(cb.rpos[1]) == P

    def same_rows(li, b, lo, hi):
        for c16, c8, cs in ((ca.k[li], cb.k[li], cb.ks[li]), (ca.v[li], cb.v[li], cb.vs[li])):
            q_ref, s_ref = kv8_quantize(c16[b, lo:hi].cpu().view(hi - lo, H, D))
            assert same_fp8(c8[b, lo:hi].cpu(), q_ref.view(hi - lo, H * D)) and torch.equal(cs[b, :, lo:hi].cpu(), s_ref.t()), (li, b)

    for li in range(len(ca.k)):
        for b in range(2):
            same_rows(li, b, 0, lens[b])
    tok = torch.tensor([7, 9], device=ids.device)
    eng.decode_step(tok, ca)
    eng.decode_step(tok, cb)
    assert [int(n) for n in cb.lens] == [n + 1 for n in lens]
    for b in range(2):
        same_rows(0, b, lens[b], lens[b] + 1)
    kw = dict(images=images, attention_mask=am, max_new_tokens=6, eos_token_id=-1, pad_token_id=0, fp8_kv=True)
    eager = m.generate(ids, use_graph=False, **kw)
    graph = m.generate(ids, use_graph=True, **kw)
    assert eager.shape == (2, P + 6) and torch.equal(eager[:, :P], ids) and torch.equal(eager, graph)


@pytest.mark.parametrize("dtype", DTYPES)
def test_expand_and_reorder_move_bytes_and_scales(dtype):
    cfg, m, ids, images = _tiny(dtype)
    eng = m.engine
    B = ids.shape[0]
    _, c0 = eng.prefill(ids, None, images, 4, kv_fp8=True)
    rows = torch.arange(B, device=ids.device).repeat_interleave(3)
    c = eng.expand_cache(c0, rows)
    n0 = int(c0.lens[0])
    assert c.fp8 and c.B == 3 * B
    for lst, lst0 in ((c.k, c0.k), (c.v, c0.v), (c.ks, c0.ks), (c.vs, c0.vs)):
        for t, t0 in zip(lst, lst0):
            assert t.dtype == t0.dtype and torch.equal(t, t0[rows])
    eng.decode_step(torch.arange(3 * B, device=ids.device) + 5, c)  # every beam row appends a different token: rows now differ at n0
    n_valid = n0 + 1
    before = [[t.clone() for t in lst] for lst in (c.k, c.v, c.ks, c.vs)]
    assert not torch.equal(before[0][0][0, n0], before[0][0][1, n0])
    perm = (torch.tensor([2, 0, 0], device=ids.device)[None, :] + 3 * torch.arange(B, device=ids.device)[:, None]).reshape(-1)
    eng.reorder_cache(c, perm, n_valid)
    for lst, old in zip((c.k, c.v), before[:2]):
        for t, t0 in zip(lst, old):
            assert torch.equal(t[:, :n_valid], t0[perm][:, :n_valid])
    for lst, old in zip((c.ks, c.vs), before[2:]):
        for t, t0 in zip(lst, old):
            assert torch.equal(t[:, :, :n_valid], t0[perm][:, :, :n_valid])
    eng.reorder_cache(c, perm, n_valid)  # the second buffer set exists now: once more through the swap
    assert torch.equal(c.k[0][:, :n_valid], before[0][0][perm][perm][:, :n_valid])
    assert torch.equal(c.ks[-1][:, :, :n_valid], before[2][-1][perm][perm][:, :, :n_valid])
