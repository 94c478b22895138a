"""merlin_amd/model/kv_cache.py on CPU tensors (no kernels): KVCache.copy_rows in both formats against explicit per-tensor indexing for
its three uses - grow, expand a prefix, pair two caches -, the refusals' messages, that the sources are not written, and the length /
position bookkeeping of advance and truncate."""
import pytest
import torch

from merlin_amd.model.kv_cache import BeamKVCache, KVCache

L, H, D = 2, 2, 4
d = H * D


def _filled(B, Smax, fp8, seed, lens):
    """A cache whose every cell holds a distinct non-zero value (so a copy into the wrong place cannot go unseen), with the given lens."""
    g = torch.Generator().manual_seed(seed)
    c = KVCache(L, B, Smax, d, torch.bfloat16, "cpu", fp8=fp8, H=H)
    for lst in c.sets():
        for t in lst:
            if t.dtype == torch.uint8:
                t.copy_(torch.randint(1, 256, t.shape, generator=g).to(torch.uint8))
            else:
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
    c.lens.copy_(torch.tensor(lens, dtype=torch.int32))
    return c


def _snapshot(c):
    return [t.clone() for lst in c.sets() for t in lst] + [c.lens.clone()]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _check_format(out, src, B, Smax):
    assert out.fp8 == src.fp8 and out.H == src.H and (out.B, out.Smax) == (B, Smax) and len(out.sets()) == (4 if src.fp8 else 2)
    for lst in out.sets()[:2]:
        assert len(lst) == L and all(t.shape == (B, Smax, d) and t.dtype == (torch.uint8 if src.fp8 else torch.bfloat16) for t in lst)
    for lst in out.sets()[2:]:
        assert len(lst) == L and all(t.shape == (B, H, Smax) and t.dtype == torch.float32 for t in lst)
    assert out.lens.dtype == torch.int32 and out.lens.shape == (B,)


@pytest.mark.parametrize("fp8", [False, True])
def test_grow(fp8):
    src = _filled(2, 5, fp8, 1, [3, 5])
    src.rpos = torch.tensor([7, 9], dtype=torch.int32)
    before = _snapshot(src)
    out = src.grown(8)
    _check_format(out, src, 2, 8)
    for li in range(L):
        for name in ("k", "v"):
            a, b = getattr(out, name)[li], getattr(src, name)[li]
            assert torch.equal(a[:, :5], b) and not a[:, 5:].any()
        for name in ("ks", "vs") if fp8 else ():
            a, b = getattr(out, name)[li], getattr(src, name)[li]
            assert torch.equal(a[:, :, :5], b) and not a[:, :, 5:].any()
    assert out.lens.tolist() == [3, 5] and out.rpos.tolist() == [7, 9] and out.rpos is not src.rpos
    assert _same(before, _snapshot(src)) and src.rpos.tolist() == [7, 9]
    assert src.grown(5).Smax == 5 and src.grown(5).rpos is not None
    src.rpos = None
    assert src.grown(6).rpos is None
    with pytest.raises(ValueError, match=r"grow_cache\(4\): the cache already has 5 rows"):
        src.grown(4)


@pytest.mark.parametrize("fp8", [False, True])
def test_expand_prefix(fp8):
    P, nb, Smax = 3, 3, 6
    src = _filled(1, 7, fp8, 2, [P])
    before = _snapshot(src)
    out = src.expanded_prefix(nb, P, Smax)
    _check_format(out, src, nb, Smax)
    for li in range(L):
        for m in range(nb):
            for name in ("k", "v"):
                a, b = getattr(out, name)[li], getattr(src, name)[li]
                assert torch.equal(a[m, :P], b[0, :P]) and not a[m, P:].any()
            for name in ("ks", "vs") if fp8 else ():
                a, b = getattr(out, name)[li], getattr(src, name)[li]
                assert torch.equal(a[m, :, :P], b[0, :, :P]) and not a[m, :, P:].any()
    assert out.lens.tolist() == [P] * nb and out.rpos is None
    assert _same(before, _snapshot(src))
    two = _filled(2, 7, fp8, 3, [3, 3])
    with pytest.raises(ValueError, match="expand_prefix takes a one-sequence cache holding 3 <= 6 rows"):
        two.expanded_prefix(nb, P, Smax)
    with pytest.raises(ValueError, match="expand_prefix takes a one-sequence cache holding 8 <= 7 rows"):
        src.expanded_prefix(nb, 8, 9)


@pytest.mark.parametrize("fp8", [False, True])
def test_pair(fp8):
    cond, uncond = _filled(1, 4, fp8, 4, [3]), _filled(1, 6, fp8, 5, [5])
    before = _snapshot(cond), _snapshot(uncond)
    out = KVCache.paired(cond, uncond, 2)
    _check_format(out, cond, 2, 7)
    for li in range(L):
        for b, (src, P) in enumerate(((cond, 3), (uncond, 5))):
            for name in ("k", "v"):
                a, s = getattr(out, name)[li], getattr(src, name)[li]
                assert torch.equal(a[b, :P], s[0, :P]) and not a[b, P:].any()
            for name in ("ks", "vs") if fp8 else ():
                a, s = getattr(out, name)[li], getattr(src, name)[li]
                assert torch.equal(a[b, :, :P], s[0, :, :P]) and not a[b, :, P:].any()
    assert out.lens.tolist() == [3, 5] and out.rpos is None
    assert _same(before[0], _snapshot(cond)) and _same(before[1], _snapshot(uncond))
    other = _filled(1, 4, not fp8, 6, [3])
    with pytest.raises(ValueError, match=rf"pair_cache takes two caches of one format and max_new >= 0, got fp8 = {fp8} / {not fp8}, max_new = 2"):
        KVCache.paired(cond, other, 2)
    with pytest.raises(ValueError, match="pair_cache takes two caches of one format and max_new >= 0"):
        KVCache.paired(cond, uncond, -1)
    padded = _filled(1, 4, fp8, 7, [3])
    padded.rpos = torch.tensor([4], dtype=torch.int32)
    for bad in ((out, uncond), (cond, out), (padded, uncond), (cond, BeamKVCache(uncond, 2, 2))):
        with pytest.raises(ValueError, match="pair_cache takes two plain KVCaches of one un-padded sequence each"):
            KVCache.paired(*bad, 2)


@pytest.mark.parametrize("fp8", [False, True])
def test_copy_rows_sequence_slices(fp8):
    """dst_seq / src_seq: two rows of a three-sequence cache from rows 1.. of another; everything else stays zero."""
    src = _filled(3, 4, fp8, 8, [4, 4, 4])
    out = src.empty_like(3, 6)
    out.copy_rows(src, 2, dst_seq=slice(0, 2), src_seq=slice(1, 3))
    for li in range(L):
        for name in ("k", "v"):
            a, s = getattr(out, name)[li], getattr(src, name)[li]
            assert torch.equal(a[:2, :2], s[1:, :2]) and not a[:2, 2:].any() and not a[2].any()
        for name in ("ks", "vs") if fp8 else ():
            a, s = getattr(out, name)[li], getattr(src, name)[li]
            assert torch.equal(a[:2, :, :2], s[1:, :, :2]) and not a[:2, :, 2:].any() and not a[2].any()
    assert out.lens.tolist() == [0, 0, 0]  # the lengths are the caller's


def test_advance_and_truncate():
    c = _filled(2, 8, False, 9, [3, 5])
    c.advance(1)
    assert c.lens.tolist() == [4, 6] and c.rpos is None
    c.advance(torch.tensor([2, 0], dtype=torch.int32))
    assert c.lens.tolist() == [6, 6]
    c.truncate(2)
    assert c.lens.tolist() == [2, 2]
    c.truncate(8)
    c.truncate(0)
    assert c.lens.tolist() == [0, 0]
    for bad in (-1, 9):
        with pytest.raises(ValueError, match=r"the cache has rows \[0, 8\)"):
            c.truncate(bad)
    lens, c.rpos = c.lens, torch.tensor([10, 12], dtype=torch.int32)
    rpos = c.rpos
    c.advance(3)
    assert c.lens.tolist() == [3, 3] and c.rpos.tolist() == [13, 15]
    assert c.lens is lens and c.rpos is rpos  # in place: a captured graph reads the same buffers
    with pytest.raises(ValueError, match="truncate takes a cache whose rotary positions are its rows"):
        c.truncate(1)
    assert c.lens.tolist() == [3, 3]


@pytest.mark.parametrize("fp8", [False, True])
def test_beam_cache_advance(fp8):
    pre = _filled(2, 5, fp8, 10, [3, 5])
    before = _snapshot(pre)
    b = BeamKVCache(pre, 3, 4)
    assert b.B == 6 and b.fp8 == fp8 and b.pre_lens is pre.lens
    assert b.gen.tolist() == [0] * 6 and b.apos.tolist() == [3, 3, 3, 5, 5, 5]
    gen, apos = b.gen, b.apos
    b.advance(1)
    b.advance(1)
    assert b.gen.tolist() == [2] * 6 and b.apos.tolist() == [5, 5, 5, 7, 7, 7]
    assert b.gen is gen and b.apos is apos and b.pos is gen and b.rope_pos is apos
    assert _same(before, _snapshot(pre)) and pre.lens.tolist() == [3, 5]  # the prefix does not grow
    pre.rpos = torch.tensor([6, 6], dtype=torch.int32)
    assert BeamKVCache(pre, 2, 4).apos.tolist() == [6, 6, 6, 6]  # rotary positions follow the prefix's, not its rows
