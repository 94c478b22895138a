"""Attention inputs whose softmax rows have STRUCTURE, for the per-element tests (tests/numerics.py).  With i.i.d. N(0, 1) q and k the scores
are about N(0, 1) nats and every softmax row is nearly flat: the running reference of the prefill forwards (csrc/attn_fwd2.hip "Lazy
rescaling") never moves after a row's first tile, P never leaves (0, 64], lse stays near log S and no split of a split-KV decode outweighs
the others.  The families here put all of that on the table, one head at a time, on the CPU, seeded, in the 16-bit type:

    F1    staircase up: the score level rises by 6 nats per 64-key tile (x 0.85 on every fourth query row, so that the rows of one wave move
          their reference at different tiles and P against a stale reference reaches past 128)
    F2    staircase down: the level falls by 6 nats per tile - no move after the first, P down to fp16 subnormals and zero
    F3    one-hot: one key leads every other attended key by >= 30 nats - key 0, the row's own key (causal) / a seeded random key
          (non-causal), the last valid key n - 1 (non-causal; under a causal mask the last key a row sees IS its own)
    F4    sink and shift: key 0 leads a scaled-randn rest by 12 nats; two more copies move every key by +-c e_0 so that every score of a row
          shifts by the same +-40 nats (to the rounding of c: `shift` in the result is the exact figure) and P does not change

and `cache_family` places F3 / F4 keys by index in a KV cache (first split, last split, one key of a middle split, prefix or suffix only).

Every generator ASSERTS its properties on the fp64 score matrix of the ROUNDED inputs before it returns, and for every attended pair the cap
A_ij = scale sum_d |q_id k_jd| <= 64 nats: a kernel's fp32 score moves by about sqrt(D) 2^-24 A, which at A = 64 and D = 128 is 0.09 eps(fp16) in
P - inside the factor 2 of numerics.limit.  Larger scores would test the reference's missing score-condition term, not the kernels.
v and do stay randn (`randn16`)."""
import math

import torch

A_CAP = 64.0
LOG2E = 1.4426950408889634
PREFILL_FAMILIES = ["F1", "F2", "F3-key0", "F3-own", "F3-last", "F4", "F4+40", "F4-40"]


def randn16(rows, cols, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, cols, generator=g).to(dtype)


def allowed(S, causal, n_valid=None):
    """bool [S, S]: query i attends key j (the semantics of mh_attn_fwd2: keys >= n_valid excluded, query rows >= n_valid attend nothing)."""
    n = S if n_valid is None else int(n_valid)
    ar = torch.arange(S)
    ok = (ar[None, :] < n) & (ar[:, None] < n)
    return ok & (ar[None, :] <= ar[:, None]) if causal else ok


def scores64(q, k):
    """fp64 scores in nats of the rounded inputs, q [Sq, D] and k [Sk, D]."""
    return (q.double() @ k.double().t()) / math.sqrt(q.shape[-1])


def magnitude(q, k):
    """A_ij = scale sum_d |q_id k_jd|."""
    return (q.double().abs() @ k.double().abs().t()) / math.sqrt(q.shape[-1])


def lazy_events(scores_log2, causal, tile=64, thr=8.0, n_valid=None):
    """The lazy-rescale rule of csrc/attn_fwd2.hip emulated on scores in log2 units [S, S]: the running reference of a row moves to the
    running maximum only when that exceeds it by more than thr.  -> (int64 [S]: moves of the reference AFTER the row's first, the largest
    P = exp2(score - reference in force) over attended pairs)."""
    S = scores_log2.shape[0]
    s = scores_log2.double().masked_fill(~allowed(S, causal, n_valid), float("-inf"))
    m_run = torch.full((S,), float("-inf"), dtype=torch.float64)
    events = torch.zeros(S, dtype=torch.int64)
    pmax = 0.0
    for k0 in range(0, S, tile):
        mx = s[:, k0:k0 + tile].amax(1)
        m_new = torch.maximum(m_run, mx)
        need = m_new > m_run + thr
        events += (need & torch.isfinite(m_run)).long()
        m_run = torch.where(need, m_new, m_run)
        seen = torch.isfinite(mx)
        if bool(seen.any()):
            pmax = max(pmax, float(torch.exp2(mx[seen] - m_run[seen]).max()))
    return events, pmax


def _unit(D, g):
    """A dense unit vector, every entry +-1 / sqrt(D)."""
    return (torch.randint(0, 2, (D,), generator=g).double() * 2 - 1) / math.sqrt(D)


def _softmax64(s, ok):
    s = s.masked_fill(~ok, float("-inf"))
    m = s.amax(1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(1, keepdim=True)
    return e / l.clamp_min(1e-300)


def _finish(name, q, k, dtype, causal, n_valid, extra=None):
    """Round, assert the magnitude cap, -> dict q, k (16-bit), s (fp64 nats), ok, P (fp64), A_row (the row's largest attended A)."""
    q, k = q.to(dtype), k.to(dtype)
    S = q.shape[0]
    ok = allowed(S, causal, n_valid)
    A = magnitude(q, k).masked_fill(~ok, 0.0)
    assert float(A.max()) <= A_CAP, f"{name}: A = {float(A.max()):.1f} nats exceeds the cap {A_CAP}"
    s = scores64(q, k)
    out = {"name": name, "q": q, "k": k, "s": s, "ok": ok, "P": _softmax64(s, ok), "A_row": A.amax(1), "A_max": float(A.max())}
    out.update(extra or {})
    return out


def _staircase(S, D, dtype, causal, n, g, step):
    """q_i = a f_i u + noise, k_j = b_j u + noise: s_ij ~ f_i step (j // 64) nats."""
    u = _unit(D, g)
    a0 = math.sqrt(32.0 * math.sqrt(D))
    f = torch.where(torch.arange(S) % 4 == 3, 0.85, 1.0).double()
    level = step * (torch.arange(S) // 64).double()
    b = level * math.sqrt(D) / a0
    q = (a0 * f)[:, None] * u[None, :] + 0.05 * torch.randn(S, D, generator=g).double()
    k = b[:, None] * u[None, :] + 0.1 * torch.randn(S, D, generator=g).double()
    return q, k


MAX_OVERLAP = 0.4


def _onehot(S, D, dtype, heavy, g):
    """Every distinct heavy key j gets a random unit direction g_j: k_j = a g_j, every other key small noise, q_i = a g_heavy(i) + noise with
    scale a^2 = 54 nats (one shared key) or 57 (many: their directions overlap by up to MAX_OVERLAP, which leaves 57 x 0.6 = 34 nats of
    lead before the noise).  In 64 dimensions random directions of a few hundred keys overlap by up to ~0.5: a heavy direction whose
    |cosine| with an EARLIER heavy key's exceeds MAX_OVERLAP is drawn again.  The redraws come after every other draw, so a set of
    directions that needs none gives the inputs it always gave."""
    keys = torch.unique(heavy)
    s_heavy = 54.0 if keys.numel() == 1 else 57.0
    a = math.sqrt(s_heavy * math.sqrt(D))
    dirs = torch.randn(S, D, generator=g).double()
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    k = 0.3 * torch.randn(S, D, generator=g).double()
    q_noise = 0.05 * torch.randn(S, D, generator=g).double()
    kl = keys.tolist()
    for i, j in enumerate(kl[1:], 1):
        while float((dirs[kl[:i]] @ dirs[j]).abs().max()) > MAX_OVERLAP:
            d = torch.randn(D, generator=g).double()
            dirs[j] = d / d.norm()
    k[keys] = a * dirs[keys]
    q = a * dirs[heavy] + q_noise
    return q, k


def _sink(S, D, dtype, g, c):
    """Channel 0 carries the shift (q = SHIFT_Q[D], k = c), channel 1 the sink (key 0 only, SINK nats), the other channels 0.7 x randn."""
    q = 0.7 * torch.randn(S, D, generator=g).double()
    k = 0.7 * torch.randn(S, D, generator=g).double()
    q[:, 0], k[:, 0] = SHIFT_Q[D], c
    q[:, 1], k[:, 1] = 16.0, 0.0
    k[0, 1] = SINK * math.sqrt(D) / 16.0
    return q, k


SINK = 17.0
# channel 0 of q, and the value c of channel 0 of k, with q c / sqrt(D) ~ 40 nats: both exact in bf16 and fp16, c exact in e4m3 at any power-of-two scale
SHIFT_Q = {128: 15.0625, 64: 16.0}


def shift_channel(D):
    return {128: 30.0, 64: 20.0}[D]


def prefill_family(name, S, D, dtype, causal, n_valid=None, seed=0):
    """One head of family `name` (PREFILL_FAMILIES) -> dict q, k [S, D] in dtype, s, ok, P, A_row, A_max and the family's own figures.
    Rows and keys >= n_valid are padding (finite values of the same construction)."""
    n = S if n_valid is None else int(n_valid)
    g = torch.Generator().manual_seed(1000 * seed + S + D)
    tiles = (n + 63) // 64
    ar = torch.arange(S)
    if name in ("F1", "F2"):
        q, k = _staircase(S, D, dtype, causal, n, g, 6.0 if name == "F1" else -6.0)
        r = _finish(name, q, k, dtype, causal, n)
        ev, pmax = lazy_events(r["s"] * LOG2E, causal, n_valid=n)
        ev = ev[:n]
        r.update(events=ev, pmax=pmax)
        if name == "F1":
            # S = 384 causal: median >= 2, max >= 4, P >= 128.  Fewer tiles: a row that sees t tiles can move at most t - 1 times, and under a
            # causal mask half the rows see at most half the tiles
            want_max, want_med = min(4, tiles - 2), min(2, ((tiles - 2) if causal else (tiles - 1)) // 2)
            assert int(ev.max()) >= want_max and float(ev.double().median()) >= want_med and pmax >= 128.0, (name, S, n, int(ev.max()), float(ev.double().median()), pmax)
            assert pmax <= 256.0
        else:
            pmin = float(r["P"][r["ok"]].min())
            r["pmin"] = pmin
            # 6 nats = 8.66 bits per tile: 2^-30 needs five tiles; below that what the tiles that exist allow (fp16 subnormal from 3 tiles on)
            assert int(ev.max()) == 0 and pmin <= (2.0 ** -30 if tiles >= 5 else 2.0 ** (-8 * (tiles - 1))), (name, S, n, int(ev.max()), pmin)
        return r
    if name.startswith("F3"):
        place = name[3:]
        if place == "key0":
            heavy = torch.zeros(S, dtype=torch.int64)
        elif place == "last":
            assert not causal, "under a causal mask the last key a row sees is its own: F3-own"
            heavy = torch.full((S,), n - 1, dtype=torch.int64)
        else:
            assert place == "own"
            heavy = ar.clone() if causal else torch.full((S,), int(torch.randint(1, n - 1, (1,), generator=g)), dtype=torch.int64)
        heavy = heavy.clamp_max(n - 1)
        q, k = _onehot(S, D, dtype, heavy, g)
        r = _finish(name, q, k, dtype, causal, n)
        s = r["s"].masked_fill(~r["ok"], float("-inf"))[:n]
        top = s.gather(1, heavy[:n, None])[:, 0]
        rest = s.scatter(1, heavy[:n, None], float("-inf")).amax(1)
        lead = float((top - rest)[torch.isfinite(rest)].min()) if bool(torch.isfinite(rest).any()) else float("inf")
        pm = float(r["P"][:n].amax(1).min())
        assert lead >= 30.0 and pm >= 1 - 1e-9, (name, S, n, lead, pm)
        r.update(heavy=heavy, lead=lead)
        return r
    assert name in ("F4", "F4+40", "F4-40"), name
    c = shift_channel(D)
    q, k = _sink(S, D, dtype, g, 0.0)
    base = _finish("F4", q, k, dtype, causal, n)
    s = base["s"].masked_fill(~base["ok"], float("-inf"))[:n]
    vis = base["ok"][:n, 1:].any(1)  # (causal row 0 sees the sink alone)
    lead = float((s[:, 0] - s[:, 1:].amax(1))[vis].min())
    assert lead >= 12.0, (name, S, n, lead)
    base.update(lead=lead, shift=0.0)
    if name == "F4":
        return base
    k = k.clone()
    k[:, 0] = c if name == "F4+40" else -c
    r = _finish(name, q, k, dtype, causal, n)
    d = (r["s"] - base["s"])[base["ok"]]
    shift = float(d.mean())
    assert abs(abs(shift) - 40.0) < 0.1 and float((d - shift).abs().max()) < 1e-9, (name, shift)
    assert float((r["P"] - base["P"]).abs().max()) <= 1e-9, name
    r.update(lead=lead, shift=shift)
    return r


def prefill_heads(name, B, S, H, D, dtype, causal, lens=None):
    """The B x H heads of a test shape -> (list of per-head dicts in (b, h) order, q and k as [B * S, H * D] on the CPU)."""
    heads = [prefill_family(name, S, D, dtype, causal, n_valid=(lens[b] if lens else None), seed=b * H + h + 1) for b in range(B) for h in range(H)]
    pack = lambda key: torch.cat([torch.cat([heads[b * H + h][key] for h in range(H)], 1) for b in range(B)], 0)  # noqa: E731
    return heads, pack("q"), pack("k")


# ---- cache kernels: heavy keys placed by index ----------------------------------------------------------------------------------------------
def cache_family(kind, n, H, D, dtype, heavy, seed, shift=0, kv8=True, nq=None):
    """One sequence of a KV cache with n valid keys: q [H, D] (nq queries: [nq, H, D]) and k [n, H, D].  kind "onehot": key heavy[0] leads every other by >= 30 nats
    in every head (F3); kind "sink": the keys of `heavy` lead a scaled-randn rest by >= 12 nats (F4), and with shift = +-1 every key is moved
    by +-c e_0 as well, which shifts every score by +-40 nats.  kv8: the keys are quantised and dequantised (tests/test_kv8_cpu.py) and the
    properties hold on the DEQUANTISED cache, which is what is returned besides the bytes and scales.
    -> dict q (16-bit), k64 [n, H, D] fp64 (exactly representable in dtype), k8 / ks (kv8) and lead."""
    from test_kv8_cpu import kv8_dequantize, kv8_quantize

    g = torch.Generator().manual_seed(7000 + 13 * seed + n + D)
    heavy = list(heavy)[:1] if kind == "onehot" else list(heavy)
    assert heavy and all(0 <= j < n for j in heavy)
    qs, ks_ = [], []
    for h in range(H):
        if kind == "onehot":
            hv = torch.full((n,), heavy[0], dtype=torch.int64)
            qh, kh = _onehot(n, D, dtype, hv, g)
            qh = qh[:nq or 1]
        else:
            assert kind == "sink"
            c = shift_channel(D) * shift * (1 if h % 2 == 0 else -1)
            qh, kh = _sink(n, D, dtype, g, float(c))
            kh[0, 1] = 0.0
            kh[heavy, 1] = SINK * math.sqrt(D) / 16.0
            qh = qh[:nq or 1]
        qs.append(qh)
        ks_.append(kh)
    assert n >= (nq or 1)
    q = torch.stack(qs, 1).to(dtype)  # [nq, H, D]
    k = torch.stack(ks_, 1).to(dtype)
    out = {"q": q if nq else q[0]}
    if kv8:
        k8, sc = kv8_quantize(k)
        k64 = kv8_dequantize(k8, sc)
        assert torch.equal(k64.to(dtype).double(), k64)
        out.update(k8=k8, ks=sc)
    else:
        k64 = k.double()
    out["k64"] = k64
    s = (torch.einsum("qhd,nhd->qhn", q.double(), k64) / math.sqrt(D)).reshape(-1, n)
    A = torch.einsum("qhd,nhd->qhn", q.double().abs(), k64.abs()) / math.sqrt(D)
    assert float(A.max()) <= A_CAP, f"cache {kind}: A = {float(A.max()):.1f} exceeds the cap"
    hv = torch.zeros(n, dtype=torch.bool)
    hv[heavy] = True
    lead = float((s[:, hv].amin(1) - s[:, ~hv].amax(1)).min()) if n > len(heavy) else float("inf")
    assert lead >= (30.0 if kind == "onehot" else 12.0), (kind, heavy, lead)
    if kind == "onehot":
        assert float(torch.softmax(s, 1).amax(1).min()) >= 1 - 1e-9
    if shift:
        assert float(s.abs().amin(1).min()) >= 20.0  # every score of the row carries the +-40 nats
    out.update(lead=lead, A_max=float(A.max()))
    return out


# (B, S, H, D, causal, lens) of the prefill tests: the five-product backward applies and attn_fwd3 gets a full 256-query block plus a partial
# one; causal with ragged lengths and partial tiles; the non-causal D = 64 form with ragged lengths
# ... and the other two (head dim, mask) combinations the library compiles: non-causal D = 128 (a full 256-query block plus a partial one for
# attn_fwd3 / attn_fwd4; ragged with partial tiles) and causal D = 64 (ragged; whole tiles with two key blocks)
PREFILL_SHAPES = [(1, 384, 1, 128, True, None), (2, 300, 2, 128, True, [300, 177]), (2, 200, 2, 64, False, [200, 130]),
                  (1, 384, 1, 128, False, None), (2, 300, 2, 128, False, [300, 177]), (2, 200, 2, 64, True, [200, 130]), (1, 256, 1, 64, True, None)]


def families(causal):
    """The prefill families that exist under this mask (F3-last is F3-own under a causal mask)."""
    return [f for f in PREFILL_FAMILIES if not (causal and f == "F3-last")]


def placements(n, chunk, splits):
    """Heavy keys by index for a cache of n keys cut into `splits` chunks of `chunk` keys: inside the first split, inside the last split
    (its last key n - 1 first), one key of a middle split.  "onehot" takes the first index of a list, "sink" all of them."""
    assert splits >= 3 and (splits - 1) * chunk < n <= splits * chunk
    mid = splits // 2
    return {"first split": [3, 0, chunk - 1], "last split": [n - 1, (splits - 1) * chunk], "middle split": [mid * chunk + chunk // 2]}
