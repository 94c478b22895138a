"""The attention kernels on STRUCTURED softmax rows (tests/attn_inputs.py), per element (tests/numerics.py).

Prefill: every family, bf16 and fp16, at the smallest shapes at which each form's structure is present - the three forward forms (o through
_hold_heads, bit equality of the forms, lse per element), the seven-product backward in the three fused-kv modes and the five-product
backward where it applies.  Cache kernels: one-hot and sink keys placed by key index - inside the first split, the last split, one key of a
middle split, prefix only, suffix only - for mh_attn_decode (merge launch, one block), _multi, extend, extend_branches, _beams
and their fp8-cache forms, against N.attention_decode on the dequantised cache.

Outputs and gradients keep the project's rule: limit = N.limit(c_model), c_model from the rounding model on the same inputs.  lse is held to
|lse - lse64| <= c 2^-24 (|lse64| + A_row + 1) (N.lse_c), c_model from fp32 scores and an fp32 logsumexp (N.attention_lse_model).
Every check prints `CW | operation | dtype | c_model | c_kernel | limit` before it asserts."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import attn_inputs as AI  # noqa: E402
import numerics as N  # noqa: E402
from test_componentwise_gpu import _attention_refs, _heads, _hold_heads, _mask_tag  # noqa: E402
from test_kv8_cpu import kv8_dequantize, kv8_quantize  # noqa: E402
from test_kv8_gpu import hold  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from merlin_amd import ops as O

    assert O.arch_ok(0), "not a gfx950 device"
    return O


# ---- prefill ---------------------------------------------------------------------------------------------------------------------------------
def hold_lse(name, dtype, lse, q, k, refs, B, S, H, D, causal, lens):
    """lse [B, H, S_pad] of a forward against the fp64 lse of the references, per row; the limit from the fp32 model on the same inputs."""
    lens = lens if lens else [S] * B
    heads = list(zip(_heads(q, B, S, H, D), _heads(k, B, S, H, D)))
    A = torch.stack([N.attention_magnitude(qq, kk, causal=causal, n_valid=lens[i // H]) for i, (qq, kk) in enumerate(heads)])
    mod = torch.stack([N.attention_lse_model(qq, kk, causal=causal, n_valid=lens[i // H]) for i, (qq, kk) in enumerate(heads)])
    ref = torch.stack([r["lse"] for r in refs])
    cm, _ = N.lse_c(mod, ref, A)
    ck, at = N.lse_c(lse[:, :, :S].reshape(B * H, S), ref, A)
    lim = N.limit(cm)
    print(f"CW | {name} | {str(dtype)[6:]} | {cm:.3f} | {ck:.3f} | {lim:.3f} | worst at {at}")
    assert ck <= lim, f"{name} {dtype}: kernel c = {ck:.3f} at {at} exceeds {lim:.3f} (model c = {cm:.3f})"
    return ref


def run_prefill(ops, name, dtype, B, S, H, D, causal, lens):
    """One family at one shape through every forward form and backward form.  -> (lse of form 0 [B * H, S], fp64 lse)."""
    heads, q, k = AI.prefill_heads(name, B, S, H, D, dtype, causal, lens)
    q, k = q.to(dev()), k.to(dev())
    v, do = AI.randn16(B * S, H * D, dtype, 21).to(dev()), AI.randn16(B * S, H * D, dtype, 22).to(dev())
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev()) if lens else None
    refs, mods = _attention_refs(q, k, v, do, B, S, H, D, causal, lens, dtype)
    tag = f"{name} S={S} D={D}{_mask_tag(D, causal)}{' ragged' if lens else ''}"
    fwd = {}
    try:
        for form in ((0, 1, 2) if D == 128 else (0,)):
            ops.attn_fwd_pingpong(form)
            fwd[form] = ops.attn_fwd2(q, k, v, B, S, H, D, causal, seqlens=lens_t)
    finally:
        ops.attn_fwd_pingpong(0)
    lse64 = None
    for form, (o, lse) in fwd.items():
        _hold_heads(f"attention o form {form} {tag}", dtype, o, refs, mods, "o", B, S, H, D)
        lse64 = hold_lse(f"attention lse form {form} {tag}", dtype, lse, q, k, refs, B, S, H, D, causal, lens)
    o, lse = fwd[0]
    for form in (1, 2):
        if form in fwd:
            assert torch.equal(fwd[form][0], o), f"{tag}: o of forward form {form} is not bit-identical to form 0"
    if 2 in fwd:
        assert torch.equal(fwd[2][1][:, :, :S], lse[:, :, :S]), f"{tag}: lse of forward form 2 is not bit-identical to form 0"

    from merlin_amd import _lib as L

    mode0 = int(L.lib().mh_attn_bwd_fused_kv_mode())
    seven = {}
    try:
        for mode in ((0, 1, 2) if D == 128 else (mode0,)):
            ops.attn_bwd_fused_kv(mode)
            seven[mode] = ops.attn_bwd2(q, k, v, o, do, lse, B, S, H, D, causal, seqlens=lens_t, spill=False)
            if D == 128 and causal:
                assert ops.LAST_ATTN_BWD_FORM == "seven-product"
    finally:
        ops.attn_bwd_fused_kv(mode0)
    for mode, grads in seven.items():
        for nm, g in zip(("dq", "dk", "dv"), grads):
            _hold_heads(f"attention {nm} 7-product kv mode {mode} {tag}", dtype, g, refs, mods, nm, B, S, H, D)
    first = seven[min(seven)]
    for mode, grads in seven.items():
        assert torch.equal(grads[1], first[1]) and torch.equal(grads[2], first[2]), f"{tag}: dK / dV of fused-kv mode {mode} differ from mode {min(seven)}"
    if causal and D == 128 and S % 128 == 0 and not lens:
        assert mode0 == 2
        dq, dk, dv = ops.attn_bwd2(q, k, v, o, do, lse, B, S, H, D, causal, seqlens=lens_t, spill=True)
        assert ops.LAST_ATTN_BWD_FORM == "five-product"
        for nm, g in (("dq", dq), ("dk", dk), ("dv", dv)):
            _hold_heads(f"attention {nm} 5-product {tag}", dtype, g, refs, mods, nm, B, S, H, D)
        assert torch.equal(dk, first[1]) and torch.equal(dv, first[2]), f"{tag}: dK / dV of the five-product form differ from the seven-product form's"
    return lse[:, :, :S].reshape(B * H, S).double(), lse64, heads


# every (shape, family) that exists: F3-last is F3-own under a causal mask; F4 and its copies have a test of their own
PREFILL_CASES = [shape + (name,) for shape in AI.PREFILL_SHAPES for name in AI.families(shape[4]) if not name.startswith("F4")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,S,H,D,causal,lens,name", PREFILL_CASES)
def test_prefill_on_structured_rows_per_element(ops, dtype, B, S, H, D, causal, lens, name):
    run_prefill(ops, name, dtype, B, S, H, D, causal, lens)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,S,H,D,causal,lens", AI.PREFILL_SHAPES)
def test_prefill_sink_and_shift_per_element(ops, dtype, B, S, H, D, causal, lens):
    """F4 and its two shifted copies: each is held like every family, and lse(shifted) - lse(base) is the shift the generator measured
    (+-40 nats) within the sum of the two rows' lse bounds."""
    base, base64, _ = run_prefill(ops, "F4", dtype, B, S, H, D, causal, lens)
    for name in ("F4+40", "F4-40"):
        lse, lse64, heads = run_prefill(ops, name, dtype, B, S, H, D, causal, lens)
        n_of = [(lens[i // H] if lens else S) for i in range(B * H)]
        for i, r in enumerate(heads):
            n = n_of[i]
            assert abs(abs(r["shift"]) - 40.0) < 0.1
            A = r["A_row"][:n].to(dev())
            lim = N.limit(N.lse_c(N.attention_lse_model(r["q"].to(dev()), r["k"].to(dev()), causal=causal, n_valid=n)[:n], lse64[i, :n], A)[0])
            tol = lim * N.EPS16[torch.float32] * ((lse64[i, :n].abs() + A + 1.0) + (base64[i, :n].abs() + (A - abs(r["shift"])).clamp_min(0) + 1.0))
            d = (lse[i, :n] - base[i, :n] - r["shift"]).abs()
            print(f"SHIFT | {name} S={S} head {i} | {str(dtype)[6:]} | shift {r['shift']:.4f} | worst |lse' - lse - shift| / tol = {float((d / tol).max()):.3f}")
            assert bool((d <= tol).all()), (name, i, float((d / tol).max()))


# ---- cache kernels ---------------------------------------------------------------------------------------------------------------------------
KINDS = [("onehot", 0), ("sink", 1)]  # (family, shift): F3, and F4 with every key moved by +-c e_0 (sign by head)


def _values(n_rows, H, D, dtype, seed):
    """randn values as an fp8 cache holds them: (bytes [n, H*D], scales [H, n], dequantised fp64 [n, H, D])."""
    g = torch.Generator().manual_seed(900 + seed)
    v8, vs = kv8_quantize(torch.randn(n_rows, H, D, generator=g).to(dtype))
    return v8.view(n_rows, H * D), vs.t().contiguous(), kv8_dequantize(v8, vs)


def _cache(seqs, Smax, H, D, dtype, seed):
    """seqs: list of cache_family dicts (k of n_b <= Smax rows each) -> device tensors k8, ks, k16, v8, vs, v16 [B, Smax, ...] and the
    fp64 dequantised k64, v64 lists.  Rows behind a sequence's keys hold finite randn noise (they are not attended)."""
    d, Bn = H * D, len(seqs)
    k8 = torch.zeros(Bn, Smax, d, dtype=torch.uint8)
    ks = torch.ones(Bn, H, Smax)
    k64 = torch.zeros(Bn, Smax, H, D, dtype=torch.float64)
    v8, vs, v64 = torch.zeros_like(k8), torch.ones_like(ks), torch.zeros_like(k64)
    for b, r in enumerate(seqs):
        n = r["k64"].shape[0]
        k8[b, :n], ks[b, :, :n], k64[b, :n] = r["k8"].view(n, d), r["ks"].t(), r["k64"]
        v8[b], vs[b], v64[b] = _values(Smax, H, D, dtype, seed + b)
    k16, v16 = k64.to(dtype).view(Bn, Smax, d), v64.to(dtype).view(Bn, Smax, d)
    assert torch.equal(k16.double().view_as(k64), k64) and torch.equal(v16.double().view_as(v64), v64)  # the cast to the 16-bit type is exact
    return [t.to(dev()) for t in (k8, ks, k16, v8, vs, v16)], k64.to(dev()), v64.to(dev())


def _refs(rows, dtype):
    """rows: list of (q [H, D], k64 [n, H, D], v64 [n, H, D]) on the device -> (ref, B, model) stacked."""
    out = [N.attention_decode(q, k, v, k.shape[0]) + (N.attention_decode(q, k, v, k.shape[0], model=dtype),) for q, k, v in rows]
    return tuple(torch.stack([r[i] for r in out]) for i in range(3))


def _grow(splits_of, Smax, want=3, cap=1 << 16):
    """Raise Smax (x 1.5 a step) only until the host split query reports at least `want` splits."""
    while splits_of(Smax) < want:
        Smax = Smax * 3 // 2
        assert Smax <= cap, "no split plan with three splits"
    return Smax


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,shift", KINDS)
def test_decode_with_placed_heavy_keys_per_element(ops, dtype, kind, shift):
    """mh_attn_decode / _kv8 (split-KV by a merge launch, one block) on the smallest shape of its own test, Smax raised to
    three splits.  Sequence 0 fills the cache; sequence 1 ends one key into the last split, so "last split" is a split of ONE key."""
    from merlin_amd import _lib as L

    B, H, D = 2, 2, 128
    splits_of = lambda Smax: int(L.lib().mh_attn_decode_splits(B, H, Smax))  # noqa: E731
    Smax = _grow(splits_of, 40)
    splits = splits_of(Smax)
    assert splits >= 3
    chunk = (Smax + splits - 1) // splits
    lens = [Smax, (splits - 1) * chunk + 1]
    d = H * D
    for tag, _ in AI.placements(Smax, chunk, splits).items():
        seqs = [AI.cache_family(kind, n, H, D, dtype, AI.placements(n, chunk, splits)[tag], seed=b, shift=shift) for b, n in enumerate(lens)]
        (k8, ks, k16, v8, vs, v16), k64, v64 = _cache(seqs, Smax, H, D, dtype, 1)
        q = torch.stack([r["q"] for r in seqs]).view(B, d).to(dev())
        ref, Bc, mod = _refs([(q[b].view(H, D), k64[b, :lens[b]], v64[b, :lens[b]]) for b in range(B)], dtype)
        lens_t = torch.tensor(lens, dtype=torch.int32, device=dev())
        name = f"{kind} {tag} Smax={Smax} splits={splits}"
        hold(f"attention decode 16-bit merge launch {name}", dtype, ops.attn_decode(q, k16, v16, lens_t, H, D).view(B, H, D), ref, Bc, mod)
        hold(f"attention decode kv8 merge launch {name}", dtype, ops.attn_decode_kv8(q, k8, v8, ks, vs, lens_t, H, D).view(B, H, D), ref, Bc, mod)
        hold(f"attention decode 16-bit one block {name}", dtype, ops.attn_decode(q, k16, v16, lens_t, H, D, split_kv=False).view(B, H, D), ref, Bc, mod)
        hold(f"attention decode kv8 one block {name}", dtype, ops.attn_decode_kv8(q, k8, v8, ks, vs, lens_t, H, D, split_kv=False).view(B, H, D), ref, Bc, mod)


def _multi_rows(seqs, lens, T, k64, v64, H, D):
    return [(seqs[b]["q"][t].to(dev()), k64[b, :lens[b] + t], v64[b, :lens[b] + t]) for b in range(len(lens)) for t in range(T)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,shift", KINDS)
@pytest.mark.parametrize("T", [5, 16])
def test_decode_multi_with_placed_heavy_keys_per_element(ops, dtype, kind, shift, T):
    """mh_attn_decode_multi / _kv8, split-KV and one block: query (b, t) sees lens[b] + t keys; the heavy keys lie among the first lens[b]."""
    B, H, D = 2, 2, 128
    Smax = _grow(lambda s: ops.attn_decode_multi_splits(B, T, H, s), 40)
    splits = ops.attn_decode_multi_splits(B, T, H, Smax)
    assert splits >= 3
    chunk = (Smax + splits - 1) // splits
    lens = [Smax - T + 1, (splits - 1) * chunk + 1]
    assert all((splits - 1) * chunk < n for n in lens)
    d = H * D
    for tag in AI.placements(Smax, chunk, splits):
        seqs = [AI.cache_family(kind, n + T - 1, H, D, dtype, AI.placements(n, chunk, splits)[tag], seed=b, shift=shift, nq=T) for b, n in enumerate(lens)]
        (k8, ks, k16, v8, vs, v16), k64, v64 = _cache(seqs, Smax, H, D, dtype, 2)
        q = torch.cat([r["q"].reshape(T, d) for r in seqs]).to(dev())
        ref, Bc, mod = _refs(_multi_rows(seqs, lens, T, k64, v64, H, D), dtype)
        lens_t = torch.tensor(lens, dtype=torch.int32, device=dev())
        name = f"{kind} {tag} T={T} Smax={Smax} splits={splits}"
        for split in (True, False):
            how = "split-KV" if split else "one block"
            o = ops.attn_decode_multi(q, k16, v16, lens_t, T, H, D, split_kv=split)
            hold(f"attention decode multi 16-bit {how} {name}", dtype, o.view(B * T, H, D), ref, Bc, mod)
            o = ops.attn_decode_multi_kv8(q, k8, v8, ks, vs, lens_t, T, H, D, split_kv=split)
            hold(f"attention decode multi kv8 {how} {name}", dtype, o.view(B * T, H, D), ref, Bc, mod)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,shift", KINDS)
def test_extend_with_placed_heavy_keys_per_element(ops, dtype, kind, shift):
    """mh_attn_extend / _kv8 (flash-style, 64-key tiles: the placements are by key tile): 17 queries, one past a 16-row MFMA tile, against
    caches that end in a partial key tile."""
    B, n_new, H, D, Smax, lens = 2, 17, 2, 128, 300, [200, 131]
    d = H * D
    for tag in AI.placements(200, 64, 4):
        seqs = [AI.cache_family(kind, n + n_new - 1, H, D, dtype, AI.placements(n, 64, (n + 63) // 64)[tag], seed=b, shift=shift, nq=n_new) for b, n in enumerate(lens)]
        (k8, ks, k16, v8, vs, v16), k64, v64 = _cache(seqs, Smax, H, D, dtype, 3)
        q = torch.cat([r["q"].reshape(n_new, d) for r in seqs]).to(dev())
        ref, Bc, mod = _refs(_multi_rows(seqs, lens, n_new, k64, v64, H, D), dtype)
        lens_t = torch.tensor(lens, dtype=torch.int32, device=dev())
        name = f"{kind} {tag} n={n_new} lens={lens}"
        hold(f"attention extend 16-bit {name}", dtype, ops.attn_extend(q, k16, v16, lens_t, n_new, H, D).view(B * n_new, H, D), ref, Bc, mod)
        hold(f"attention extend kv8 {name}", dtype, ops.attn_extend_kv8(q, k8, v8, ks, vs, lens_t, n_new, H, D).view(B * n_new, H, D), ref, Bc, mod)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,shift", KINDS)
def test_extend_branches_with_placed_heavy_keys_per_element(ops, dtype, kind, shift):
    """mh_attn_extend_branches / _kv8: the heavy keys lie in the shared prefix (first, last - partial - and a middle key tile); every query
    sees them next to the rows of its own continuation only."""
    P, segs, H, D, Smax = 200, [5, 3, 9], 2, 64, 256
    R, d = sum(segs), H * D
    seg = [s0 for s0, n in zip([0, 5, 8], segs) for _ in range(n)]
    vis = [list(range(P)) + list(range(P + seg[r], P + r + 1)) for r in range(R)]
    for tag, heavy in AI.placements(P, 64, 4).items():
        r0 = AI.cache_family(kind, P + R, H, D, dtype, heavy, seed=4, shift=shift, nq=R)
        (k8, ks, k16, v8, vs, v16), k64, v64 = _cache([r0], Smax, H, D, dtype, 4)
        q = r0["q"].reshape(R, d).to(dev())
        ref, Bc, mod = _refs([(q[r].view(H, D), k64[0][vis[r]], v64[0][vis[r]]) for r in range(R)], dtype)
        seg_t = torch.tensor(seg, dtype=torch.int32, device=dev())
        name = f"{kind} {tag} P={P} segs={segs}"
        hold(f"attention extend branches 16-bit {name}", dtype, ops.attn_extend_branches(q, k16, v16, seg_t, P, H, D).view(R, H, D), ref, Bc, mod)
        hold(f"attention extend branches kv8 {name}", dtype, ops.attn_extend_branches_kv8(q, k8, v8, ks, vs, seg_t, P, H, D).view(R, H, D), ref, Bc, mod)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,shift", KINDS)
def test_decode_beams_with_placed_heavy_keys_per_element(ops, dtype, kind, shift):
    """mh_attn_decode_beams / _kv8: the whole mass in the prefix only (its first, last and a middle split) and in the suffix only.  Prompt 0
    has ONE prefix key, prompt 1 fills three or more prefix splits.  Suffix key g of beam m lies in row anc[m, g]; the keys of a prompt's
    beams are the family's, their values differ from slot to slot, and suffix slots no beam references hold NaN."""
    Bp, nb, H, D, G, gen = 2, 5, 4, 64, 16, 15
    Pmax = _grow(lambda s: ops.attn_decode_beams_splits(Bp, nb, H, s, G)[0], 40)
    psplits, ssplits = ops.attn_decode_beams_splits(Bp, nb, H, Pmax, G)
    assert psplits >= 3 and ssplits == 1
    chunk = (Pmax + psplits - 1) // psplits
    pre_lens, sl, n, d = [1, Pmax], gen + 1, Bp * nb, H * D
    g = torch.Generator().manual_seed(17)
    anc = (torch.randint(0, nb, (Bp, nb, G), generator=g) + nb * torch.arange(Bp)[:, None, None]).view(n, G).to(torch.int32)
    anc[:, gen] = torch.arange(n, dtype=torch.int32)
    used = torch.zeros(n, G, dtype=torch.bool)
    used[anc[:, :sl].long(), torch.arange(sl)[None, :]] = True
    where = dict(AI.placements(Pmax, chunk, psplits))
    where["suffix only"] = None
    for tag, heavy in where.items():
        seqs = []
        for p in range(Bp):
            hv = [pre_lens[p] + 7, pre_lens[p] + gen] if heavy is None else ([0] if pre_lens[p] == 1 else heavy)
            seqs.append(AI.cache_family(kind, pre_lens[p] + sl, H, D, dtype, hv, seed=10 + p, shift=shift, nq=nb))
        pre = _cache([{key: (r[key][:pre_lens[p]] if key != "q" else r[key]) for key in r if key in ("q", "k8", "ks", "k64")} for p, r in enumerate(seqs)], Pmax, H, D, dtype, 5)
        (pk8, pks, pk16, pv8, pvs, pv16), pk64, pv64 = pre
        sk8, sks = torch.full((n, G, d), 0x7F, dtype=torch.uint8), torch.full((n, H, G), float("nan"))
        sk64 = torch.full((n, G, H, D), float("nan"), dtype=torch.float64)
        sv8, svs, sv64 = sk8.clone(), sks.clone(), sk64.clone()
        for m in range(n):
            r, pl = seqs[m // nb], pre_lens[m // nb]
            vb, vsc, vd = _values(G, H, D, dtype, 50 + m)
            for gi in range(G):
                if used[m, gi]:
                    sk8[m, gi], sks[m, :, gi], sk64[m, gi] = r["k8"][pl + gi].view(d), r["ks"][pl + gi], r["k64"][pl + gi]
                    sv8[m, gi], svs[m, :, gi], sv64[m, gi] = vb[gi], vsc[:, gi], vd[gi]
        sk16, sv16 = sk64.to(dtype).view(n, G, d), sv64.to(dtype).view(n, G, d)
        sk64d, sv64d = sk64.to(dev()), sv64.to(dev())
        rows = []
        for m in range(n):
            p = m // nb
            pick = anc[m, :sl].long().to(dev())
            kk = torch.cat([pk64[p, :pre_lens[p]], sk64d[pick, torch.arange(sl, device=dev())]])
            vv = torch.cat([pv64[p, :pre_lens[p]], sv64d[pick, torch.arange(sl, device=dev())]])
            assert not bool(torch.isnan(kk).any() | torch.isnan(vv).any())
            rows.append((seqs[p]["q"][m % nb].to(dev()), kk, vv))
        ref, Bc, mod = _refs(rows, dtype)
        q = torch.cat([r["q"].reshape(nb, d) for r in seqs]).to(dev())
        pl_t = torch.tensor(pre_lens, dtype=torch.int32, device=dev())
        slens = torch.full((n,), sl, dtype=torch.int32, device=dev())
        anc_d = anc.to(dev())
        name = f"{kind} {tag} Pmax={Pmax} pre_lens={pre_lens} splits={psplits}+{ssplits}"
        o = ops.attn_decode_beams(q, pk16, pv16, pl_t, sk16.to(dev()), sv16.to(dev()), anc_d, slens, nb, H, D)
        hold(f"attention decode beams 16-bit {name}", dtype, o.view(n, H, D), ref, Bc, mod)
        o = ops.attn_decode_beams_kv8(q, pk8, pv8, pks, pvs, pl_t, sk8.to(dev()), sv8.to(dev()), sks.to(dev()), svs.to(dev()), anc_d, slens, nb, H, D)
        hold(f"attention decode beams kv8 {name}", dtype, o.view(n, H, D), ref, Bc, mod)
