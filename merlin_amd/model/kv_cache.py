"""The KV caches of the decode path: KVCache, one row per cached token and sequence, and BeamKVCache, beam search on a
shared prompt cache.  The classes own their storage format - 16-bit rows, or OCP e4m3 bytes plus power-of-two scales (include/merlin_hip.h
"fp8 KV cache") - and what a decode step does with it: which ops.X / ops.X_kv8 appends and attends, what "advance" and "re-order" mean.
The engine (engine.HipEngine, which keeps both classes as attributes) never asks a cache for its format, with one exception that concerns
the projection and not the cache: the fused q|k|v launch of a 16-bit single-token step."""
from __future__ import annotations

import torch

from .. import ops as O


class _LayerSets:
    """What both cache types share: per-layer tensor lists k, v [B, rows, H*D] and, fp8 only, ks, vs [B, H, rows]."""

    def layer(self, li):
        """The tensors of layer li: (k, v), or (k8, v8, ks, vs) of the fp8 cache."""
        return (self.k[li], self.v[li], self.ks[li], self.vs[li]) if self.fp8 else (self.k[li], self.v[li])

    def sets(self):
        """The per-layer tensor lists that make up the cache: k, v, and the scales ks, vs of the fp8 cache."""
        return [self.k, self.v, self.ks, self.vs] if self.fp8 else [self.k, self.v]

    def _row_major(self):
        """Every tensor of the cache, set by set and layer by layer, as a view [B, rows, ...]: the one place that knows that the scales
        lie head-major, [B, H, rows], while k and v lie [B, rows, H*D]."""
        return [t if i < 2 else t.transpose(1, 2) for i, lst in enumerate(self.sets()) for t in lst]

    def _op(self, fn):
        """ops.X for the 16-bit cache, ops.X_kv8 for the fp8 one: the pairs take a layer's tensors (self.layer) at the same place."""
        return getattr(O, fn.__name__ + "_kv8") if self.fp8 else fn


class KVCache(_LayerSets):
    """Per-layer rotated keys and values, [B, Smax, H*D] each, plus the valid length of every sequence.
    fp8=True (H heads): k, v hold OCP e4m3 bytes (uint8) and ks, vs [B, H, Smax] one power-of-two fp32 scale per (sequence, head,
    token) - include/merlin_hip.h "fp8 KV cache"; (1 + 4/D) / 2 of the 16-bit cache's bytes."""

    def __init__(self, n_layers, B, Smax, d, dtype, device, fp8=False, H=None):
        self.fp8, self.H = bool(fp8), H
        if fp8:
            dtype = torch.uint8
            self.ks = [torch.zeros(B, H, Smax, dtype=torch.float32, device=device) for _ in range(n_layers)]
            self.vs = [torch.zeros(B, H, Smax, dtype=torch.float32, device=device) for _ in range(n_layers)]
        self.k = [torch.zeros(B, Smax, d, dtype=dtype, device=device) for _ in range(n_layers)]
        self.v = [torch.zeros(B, Smax, d, dtype=dtype, device=device) for _ in range(n_layers)]
        self.lens = torch.zeros(B, dtype=torch.int32, device=device)
        # rotary position of the next token when it differs from its cache row (prompts with padding in front of / inside
        # them keep only their valid keys, positions stay absolute as HF numbers them); None: == lens
        self.rpos = None
        self.B, self.Smax = B, Smax
        self._alt = None  # the second buffer set of reorder

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for lst in self.sets() for t in lst)

    def advance(self, n):
        """lens += n (an int, or int32 [B] on the device), and rpos with it: the token of a decode_step, the tokens of a verify_step that
        are kept.  In place, after every kernel that read them as `pos`: a captured graph sees the same buffers.  Rows beyond the new
        length are stale; the next step overwrites them - that is the whole roll-back of a rejected draft."""
        self.lens.add_(n)
        if self.rpos is not None:
            self.rpos.add_(n)

    def truncate(self, n):
        """lens = n for every sequence: roll the cache back to its first n rows (a session that keeps a prefix of what it holds).  The
        rows behind them are stale and the next prefill / extend / decode step overwrites them, as after a rejected draft."""
        if not 0 <= int(n) <= self.Smax:
            raise ValueError(f"truncate({n}): the cache has rows [0, {self.Smax})")
        if self.rpos is not None:
            raise ValueError("truncate takes a cache whose rotary positions are its rows (no left padding or holes in the prompt)")
        self.lens.fill_(int(n))

    # ---- copies between caches (off the hot path: plain copies, once per call) ----
    def empty_like(self, B, Smax):
        """An empty cache of B sequences and Smax rows in this cache's geometry and format."""
        return KVCache(len(self.k), int(B), int(Smax), self.k[0].shape[-1], self.k[0].dtype, self.lens.device, fp8=self.fp8, H=self.H)

    def copy_rows(self, src, n, dst_seq=slice(None), src_seq=slice(None)):
        """The first n rows of the sequences src_seq of `src` -> the first n rows of the sequences dst_seq of this cache (slices; one
        source sequence goes to every destination), in every tensor of the format.  lens and rpos are the caller's; `src` is not written."""
        for dst, s in zip(self._row_major(), src._row_major()):
            dst[dst_seq, :n].copy_(s[src_seq, :n])

    def grown(self, Smax):
        """engine.grow_cache: a new cache of Smax >= self.Smax rows per sequence holding this one's rows, lengths and positions."""
        if Smax < self.Smax:
            raise ValueError(f"grow_cache({Smax}): the cache already has {self.Smax} rows")
        out = self.empty_like(self.B, Smax)
        out.copy_rows(self, self.Smax)
        out.lens.copy_(self.lens)
        out.rpos = self.rpos.clone() if self.rpos is not None else None
        return out

    def expanded_prefix(self, nb, P, Smax):
        """engine.expand_prefix: a new cache of nb sequences and Smax rows, each holding the first P rows of this one-sequence cache."""
        if self.B != 1 or P > min(Smax, self.Smax):
            raise ValueError(f"expand_prefix takes a one-sequence cache holding {P} <= {min(Smax, self.Smax)} rows")
        out = self.empty_like(nb, Smax)
        out.copy_rows(self, P)
        out.lens.copy_(self.lens.expand(nb))
        return out

    @staticmethod
    def paired(cond_cache, uncond_cache, max_new):
        """engine.pair_cache: a new cache of B = 2 whose row 0 holds the rows of cond_cache and row 1 those of uncond_cache."""
        pair = (cond_cache, uncond_cache)
        if any(not isinstance(c, KVCache) or c.B != 1 or c.rpos is not None for c in pair):
            raise ValueError("pair_cache takes two plain KVCaches of one un-padded sequence each (B = 1, no left padding or holes)")
        if cond_cache.fp8 != uncond_cache.fp8 or max_new < 0:
            raise ValueError(f"pair_cache takes two caches of one format and max_new >= 0, got fp8 = {cond_cache.fp8} / {uncond_cache.fp8}, max_new = {max_new}")
        n = [int(c.lens[0]) for c in pair]
        out = cond_cache.empty_like(2, max(n) + int(max_new))
        for b, (c, P) in enumerate(zip(pair, n)):
            out.copy_rows(c, P, dst_seq=slice(b, b + 1))
        out.lens.copy_(torch.cat([cond_cache.lens, uncond_cache.lens]))
        return out

    def reorder(self, beam_idx, n_valid):
        """Row i <- row beam_idx[i] for the first n_valid positions (HF `_reorder_cache` under beam search): one gather kernel per layer
        and tensor into a second buffer set, then the sets swap."""
        cur = self.sets()
        if self._alt is None:
            self._alt = [[torch.empty_like(t) for t in lst] for lst in cur]
        alt, n, d = self._alt, self.B, self.k[0].shape[-1]
        # k and v move their valid prefix; the scales' head-major rows [H, Smax] have none and move whole
        for first, cols in ((0, n_valid * d), (2, None))[:len(cur) // 2]:
            for li in range(len(self.k)):
                for j in (first, first + 1):
                    O.gather_rows2d(cur[j][li].view(n, -1), beam_idx, alt[j][li].view(n, -1), cols=cols)
        self.k, self.v = alt[:2]
        if self.fp8:
            self.ks, self.vs = alt[2:]
        self._alt = cur

    # ---- the steps that write and read the cache ----
    def append_rows(self, li, k, v, n, row0, H, D):
        """n computed rows per sequence (k, v [B*n, H*D]: rotated keys and values, views of a q|k|v buffer) -> rows [row0, row0 + n) of
        layer li: 16-bit copies, or quantised by mh_kv8_fill - only what is STORED is quantised."""
        if self.fp8:
            O.kv8_fill(k, self.k[li], self.ks[li], self.B, n, H, D, row0=row0)
            O.kv8_fill(v, self.v[li], self.vs[li], self.B, n, H, D, row0=row0)
        else:
            self.k[li][:, row0:row0 + n].copy_(k.view(self.B, n, H * D))
            self.v[li][:, row0:row0 + n].copy_(v.view(self.B, n, H * D))

    def attend(self, fn, li, q, *args):
        """fn(q, <layer li>, *args) in the cache's format: the attention of extend and extend_branches over the rows append_rows wrote."""
        return self._op(fn)(q, *self.layer(li), *args)

    pos = property(lambda self: self.lens, doc="The row the next token of every sequence is appended at, int32 [B] on the device.")
    rope_pos = property(lambda self: self.rpos, doc="Its rotary position when that is not its row, else None.")

    def append_step(self, li, qkv, rope, T, H, D):
        """RoPE in place on the step's qkv rows and K/V append to layer li: one row per sequence at row lens (T = 0, decode_step), or T rows
        per sequence at rows lens .. lens + T - 1 (verify_step)."""
        if T:
            self._op(O.decode_rope_append_multi)(qkv, rope, self.lens, *self.layer(li), T, H, D, rope_pos=self.rpos)
        else:
            self._op(O.decode_rope_append)(qkv, rope, self.lens, *self.layer(li), H, D, rope_pos=self.rpos)

    def attend_step(self, li, q, lens1, T, H, D):
        """The step's attention over layer li after append_step; lens1 = lens + 1, computed once per step: what the first query sees."""
        if T:
            return self._op(O.attn_decode_multi)(q, *self.layer(li), lens1, T, H, D)
        return self._op(O.attn_decode)(q, *self.layer(li), lens1, H, D)


class BeamKVCache(_LayerSets):
    """Beam search on a shared prompt cache (generate(num_beams=n, share_prompt_kv=True); include/merlin_hip.h "beam search on a shared
    prompt cache").  prefix: the prefilled KVCache of the Bp prompts itself - its tensors are used where they lie, never copied;
    pre_lens = prefix.lens.  Suffix: per-layer k, v [Bp*nb, G, H*D] (fp8: + ks, vs [Bp*nb, H, G]) in the prefix's dtype and layout, one
    row per generated token and beam.  gen int32 [Bp*nb]: suffix rows written (the append kernels' pos); apos = rotary position of
    the next token (their rope_pos); anc int32 [Bp*nb, G]: anc[m, g] is the suffix row that holds key / value g of beam m's history.
    Everything a step reads lives on the device."""

    def __init__(self, prefix, nb, G):
        Bp, dev = prefix.B, prefix.lens.device
        self.prefix, self.nb, self.Bp, self.G = prefix, int(nb), Bp, int(G)
        self.fp8, self.H = prefix.fp8, prefix.H
        self.B = n = Bp * self.nb
        self.pre_lens = prefix.lens
        d = prefix.k[0].shape[-1]
        self.k = [torch.zeros(n, G, d, dtype=t.dtype, device=dev) for t in prefix.k]
        self.v = [torch.zeros(n, G, d, dtype=t.dtype, device=dev) for t in prefix.v]
        if self.fp8:
            self.ks = [torch.zeros(n, self.H, G, dtype=torch.float32, device=dev) for _ in prefix.ks]
            self.vs = [torch.zeros(n, self.H, G, dtype=torch.float32, device=dev) for _ in prefix.vs]
        self.gen = torch.zeros(n, dtype=torch.int32, device=dev)
        base = prefix.rpos if prefix.rpos is not None else prefix.lens
        self.apos = base.repeat_interleave(self.nb).contiguous()
        # every column of a row starts as the row itself: a beam that is never re-ordered reads its own rows
        self.anc = torch.arange(n, dtype=torch.int32, device=dev)[:, None].repeat(1, G).contiguous()
        self._anc_alt = self.anc.clone()

    @property
    def nbytes(self):
        """Resident K/V bytes: the prefix once plus the suffix rows (the two ancestry tables, 8 G bytes per beam, are not K/V)."""
        return self.prefix.nbytes + sum(t.numel() * t.element_size() for lst in self.sets() for t in lst)

    def advance(self, n):
        """One more suffix row per beam (a decode_step: n = 1), in place; the prefix does not grow."""
        self.gen.add_(n)
        self.apos.add_(n)

    def reorder(self, beam_idx, n_valid=None):
        """HF `_reorder_cache`: beam m continues beam beam_idx[m] (int64 [Bp*nb] on the device, in-group).  One table kernel
        (mh_beam_ancestry); no key or value moves, so n_valid (KVCache.reorder's valid prefix) is not looked at."""
        O.beam_ancestry(self.anc, self._anc_alt, beam_idx, self.gen)
        self.anc, self._anc_alt = self._anc_alt, self.anc

    pos = property(lambda self: self.gen, doc="The suffix row every beam's next token is appended at.")
    rope_pos = property(lambda self: self.apos, doc="Its rotary position.")

    def append_step(self, li, qkv, rope, T, H, D):
        """RoPE in place and K/V append of one token per beam to its own suffix row gen, rotary position apos (T = 0 only: decode_step)."""
        assert not T, "a BeamKVCache decodes one token per beam"
        self._op(O.decode_rope_append)(qkv, rope, self.gen, *self.layer(li), H, D, rope_pos=self.apos)

    def attend_step(self, li, q, lens1, T, H, D):
        """The step's attention after append_step: every prompt key once for the nb beams of a prompt, then the suffix keys through the
        ancestry table; lens1 = gen + 1."""
        pre = self.prefix
        return self._op(O.attn_decode_beams)(q, *pre.layer(li), pre.lens, *self.layer(li), self.anc, lens1, self.nb, H, D)

    def materialize(self):
        """An ordinary KVCache of Bp*nb rows and Smax = Pmax + G: row m holds its prompt's prefix followed by its ancestry's suffix
        rows.  For tests and debugging only (host loops, copies everything); not on the decode path."""
        pre, n = self.prefix, self.B
        out = pre.empty_like(n, pre.Smax + self.G)
        gen, pl, anc = self.gen.tolist(), pre.lens.tolist(), self.anc.long()
        for m in range(n):
            p, g, at = m // self.nb, gen[m], pl[m // self.nb]
            col = torch.arange(g, device=anc.device)
            out.copy_rows(pre, at, dst_seq=slice(m, m + 1), src_seq=slice(p, p + 1))
            for dst, suf in zip(out._row_major(), self._row_major()):
                dst[m, at:at + g] = suf[anc[m, :g], col]
        out.lens = (pre.lens.repeat_interleave(self.nb) + self.gen).contiguous()
        out.rpos = (self.apos.clone() if pre.rpos is not None else None)
        return out
