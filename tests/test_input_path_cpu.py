"""tests/input_path_ref.py against independent formulations, without a GPU: a wrong reference must not be able to pass a wrong kernel.
The splice table against a literal torch.cat splice, the float64 gradients against autograd, the conversion sweep's expected bits against
hand-computed ties, the summation bound against a dropped / doubled term and against an fp32 index_add_, and the test batches against the
list of situations they are meant to contain."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import input_path_ref as R  # noqa: E402

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
SPLICE_S = [16, 255, 256, 257, 700, 4096]


# ---- splice table -----------------------------------------------------------------------------------------------------------------------------
def _cat_splice(ids, n_img, P, embed, feats):
    """The reference model's loop, literally: per sample, per (start, image) pair, cut the row open and torch.cat the image's rows in.
    feats [n_images, P, d].  Raises ValueError where the model does."""
    out, g = [], 0
    for b in range(ids.shape[0]):
        cur, row = embed[ids[b]], ids[b]
        imgs = feats[g:g + n_img[b]]
        g += n_img[b]
        if int((row == R.PATCH).sum()) == 0:
            out.append(cur)
            continue
        if int((row == R.START).sum()) != int((row == R.END).sum()):
            raise ValueError("count")
        for s, f in zip(torch.where(row == R.START)[0], imgs):
            if row[s + P + 1] != R.END:
                raise ValueError("end")
            cur = torch.cat((cur[:s + 1], f, cur[s + P + 1:]), 0)
        out.append(cur)
    return torch.stack(out)


@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("S", [16, 255, 257])
def test_splice_table_plus_gather_is_the_literal_cat_splice(S, P):
    good, bad = R.splice_batches(S, P)
    d = 4
    embed = torch.randn(R.END + 1, d, generator=torch.Generator().manual_seed(S))
    for name, ids, n_img in good:
        feats = torch.randn(sum(n_img), P, d, generator=torch.Generator().manual_seed(P))
        want = _cat_splice(ids, n_img, P, embed, feats)
        src, err = R.splice_table(ids, R.offsets(n_img), P)
        assert err == [0, 0, 0, 0], name
        got = R.embed_splice(ids, src, embed, feats.reshape(-1, d)).reshape(ids.shape[0], S, d)
        assert torch.equal(got, want), name
        # with CLS rows in place: rows_per_img = P + 1, row0 = 1 reads the same values from a feature matrix that carries a leading row per image
        wide = torch.cat([torch.full((sum(n_img), 1, d), float("nan")), feats], 1)
        src1, _ = R.splice_table(ids, R.offsets(n_img), P, rows_per_img=P + 1, row0=1)
        assert torch.equal(R.embed_splice(ids, src1, embed, wide.reshape(-1, d)).reshape(ids.shape[0], S, d), want), name
    for name, ids, n_img, b, err in bad:
        feats = torch.randn(sum(n_img), P, d)
        with pytest.raises((ValueError, IndexError)):  # (an END that would sit at S is an IndexError in the model)
            _cat_splice(ids, n_img, P, embed, feats)
        src, got = R.splice_table(ids, R.offsets(n_img), P)
        assert got == err, name
        assert bool((src[b] == -1).all()), name
        keep = [i for i in range(ids.shape[0]) if i != b]
        # the other samples: what they give in a batch of their own (image numbering included)
        want, _ = R.splice_table(ids[keep], R.offsets([n_img[i] for i in keep]), P)
        shift = torch.tensor([sum(n_img[b:b + 1]) * P if i > b else 0 for i in keep], dtype=torch.int32)[:, None]
        assert torch.equal(torch.where(src[keep] >= 0, src[keep] - shift, src[keep]), want), name


@pytest.mark.parametrize("S", SPLICE_S)
def test_splice_batches_contain_every_named_situation(S):
    c = R.chunk_of(S)
    assert c == {16: 1, 255: 1, 256: 1, 257: 2, 700: 3, 4096: 16}[S]
    for P in (1, 4):
        good, bad = R.splice_batches(S, P)
        (_, ids, n_img), (_, ids2, n_img2) = good
        starts = [torch.where(r == R.START)[0].tolist() for r in ids]
        assert int(ids[0, S - 1]) == R.END and S - 1 - P - 1 in starts[0]                       # an END at S - 1
        assert any((s + 1) % c == 0 for s in starts[1])                                          # a START that ends a chunk
        if P == 4:
            assert any(s // c != (s + P) // c for s in starts[1])                                # an image across a chunk border
        if P == 1 and S == 4096:
            assert max(np.bincount(np.array(starts[0]) // c)) >= 2                               # several starts in one thread's chunk
        assert int((ids[2] == R.PATCH).sum()) == 0 and int((ids[2] == R.START).sum()) != int((ids[2] == R.END).sum())
        assert n_img[3] > len(starts[3]) > 0 and 0 < n_img[4] < len(starts[4])
        assert n_img2[0] == 0 and int((ids2[0] == R.PATCH).sum()) > 0
        assert {e[0] for _, _, _, _, e in bad} == {0, 1} and any(e[3] == S - P - 1 for _, _, _, _, e in bad)
        for _, bids, bn, b, e in bad:
            errs = [R.splice_table(bids[i:i + 1], R.offsets(bn[i:i + 1]), P)[1][:2] for i in range(bids.shape[0])]
            assert [i for i, x in enumerate(errs) if x != [0, 0]] == [b] and e[2] == b         # exactly one bad sample


def test_splice_table_image_limit():
    S, P = 4096, 1
    rows = torch.stack([R.place(S, P, [3 * k for k in range(n)], seed=n) for n in (1024, 1025, 1025)])
    n_img = [1024, 1024, 1025]
    src, err = R.splice_table(rows, R.offsets(n_img), P, max_images=1024)
    assert err == [0, 1, 2, 3 * 1024] and bool((src[2] == -1).all())
    assert int((src[0] >= 0).sum()) == 1024 and int((src[1] >= 0).sum()) == 1024 and int(src[1, 3 * 1023 + 1]) == 1024 + 1023
    assert R.splice_table(rows, R.offsets(n_img), P)[1] == [0, 0, 0, 0]  # the model itself has no limit


# ---- embedding gather / scatter -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,d", [(48, 64), (5, 8), (700, 8)])
def test_embedding_gradients_are_autograd_of_the_gather(T, d):
    c = R.embed_case(T, d)
    g = torch.Generator().manual_seed(T)
    embed = torch.randn(R.N_EMBED, d, generator=g, dtype=torch.float64, requires_grad=True)
    feats = torch.randn(c["n_feat"], d, generator=g, dtype=torch.float64, requires_grad=True)
    dout = R.signed_magnitudes((T, d), BF16, 1)
    out = R.embed_splice(c["ids"], c["src"], embed, feats)
    out.backward(dout.double())
    dfeats, dembed, mag, count = R.embed_splice_grads(c["ids"], c["src"], dout, c["n_feat"], R.N_EMBED)
    assert torch.equal(dfeats, feats.grad) and torch.allclose(dembed, embed.grad, rtol=1e-13, atol=0)
    sel = c["src"] >= 0
    assert torch.equal(count, torch.bincount(c["ids"][~sel], minlength=R.N_EMBED))
    assert int((dfeats.abs().sum(1) == 0).sum()) == c["n_feat"] // (c["P"] + 1)  # exactly the CLS rows receive nothing
    # src = None: everything goes to the table
    _, de, _, cnt = R.embed_splice_grads(c["ids"], None, dout, 0, R.N_EMBED)
    assert int(cnt.sum()) == T and torch.allclose(de.sum(0), dout.double().sum(0), rtol=1e-12, atol=1e-12)


def test_embed_cases_hold_what_the_scatter_test_needs():
    for T, d in R.EMBED_SHAPES:
        c = R.embed_case(T, d)
        cnt = torch.bincount(c["ids"][c["src"] < 0], minlength=R.N_EMBED)
        assert c["ids"].numel() == T and int(c["ids"].max()) < R.N_EMBED
        if T >= 700:
            assert int(cnt[c["pad"]]) >= 600 and int(cnt[0]) == 1 and int(cnt[R.N_EMBED - 1]) == 1
        assert int((cnt == 1).sum()) >= 1 and int((cnt == 0).sum()) >= 1
        assert int(c["src"].max()) == c["n_feat"] - 1 and int((c["src"] >= 0).sum()) == c["n_feat"] // (c["P"] + 1) * c["P"]
    assert (1040 * 4096 // 8 + 255) // 256 > 2048 >= (700 * 1536 // 8 + 255) // 256  # which shape wraps the grid


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_summation_bound_holds_for_fp32_and_catches_a_dropped_or_doubled_term(dtype):
    T, d = 700, 64
    c = R.embed_case(T, d)
    dout = R.signed_magnitudes((T, d), dtype, 2)
    assert float(dout.float().abs().min()) >= 0.5 and float(dout.float().abs().max()) < 2.0
    _, ref, mag, count = R.embed_splice_grads(c["ids"], c["src"], dout, c["n_feat"], R.N_EMBED)
    init = torch.randn(R.N_EMBED, d, generator=torch.Generator().manual_seed(3))
    n = count + 1
    bound = R.sum_bound(n)[:, None] * (mag + init.double().abs())
    keep = c["src"] < 0
    got = init.clone().index_add_(0, c["ids"][keep], dout[keep].float())
    assert bool(((got.double() - (ref + init.double())).abs() <= bound).all())
    assert float(bound[count == 0].max()) == 0.0 and bool(torch.equal(got[count == 0], init[count == 0]))
    # one contribution to the pad row dropped, one doubled: off by >= 0.5 in every column, the bound is < 0.1 there
    t = int((c["ids"] == c["pad"]).nonzero()[5])
    for factor in (0.0, 2.0):
        g2 = dout[keep].float()
        g2[int(keep[:t].sum())] *= factor
        wrong = init.clone().index_add_(0, c["ids"][keep], g2)
        off = (wrong.double() - (ref + init.double())).abs()[c["pad"]]
        assert bool((off > 5 * bound[c["pad"]]).all()) and float(bound[c["pad"]].max()) < 0.1


# ---- CLIP input pieces --------------------------------------------------------------------------------------------------------------------------
def test_im2col_against_explicit_loops():
    N, img, ps, kpad = 2, 28, 14, 592
    pix = torch.randn(N, 3, img, img, generator=torch.Generator().manual_seed(0))
    for rpi, row0 in ((None, 0), (5, 1), (7, 2)):
        cols = R.im2col(pix, ps, kpad, BF16, rpi, row0)
        G = img // ps
        r = G * G + row0 if rpi is None else rpi
        want = torch.zeros(N * r, kpad, dtype=BF16)
        for n in range(N):
            for gy in range(G):
                for gx in range(G):
                    blk = pix[n, :, gy * ps:(gy + 1) * ps, gx * ps:(gx + 1) * ps].to(BF16)
                    want[n * r + row0 + gy * G + gx, :588] = blk.reshape(-1)
        assert torch.equal(cols.view(torch.int16), want.view(torch.int16))


def test_assemble_copy_transpose_gather_against_explicit_loops():
    N, G2, d = 2, 3, 8
    g = torch.Generator().manual_seed(1)
    patch, cls, pos = torch.randn(N * (G2 + 1), d, generator=g).to(F16), torch.randn(d, generator=g).to(F16), torch.randn(G2 + 1, d, generator=g).to(F16)
    patch[::G2 + 1] = float("nan")
    x = R.vit_assemble(patch, cls, pos, N, G2, F16)
    for n in range(N):
        for t in range(G2 + 1):
            a = cls if t == 0 else patch[n * (G2 + 1) + t]
            assert torch.equal(x[n * (G2 + 1) + t], (a.float() + pos[t].float()).to(F16))
    src, dst = torch.randn(3, 5, generator=g).to(BF16), torch.randn(4, 9, generator=g).to(BF16)
    out = R.copy2d(src, dst, True)
    assert torch.equal(out[3:], dst[3:]) and torch.equal(out[:, 5:], dst[:, 5:])
    assert all(float(out[r, c]) == float((dst[r, c].float() + src[r, c].float()).to(BF16)) for r in range(3) for c in range(5))
    assert torch.equal(R.copy2d(src, dst, False)[:3, :5], src)
    xt = R.transpose_pad(src, 7)
    assert xt.shape == (5, 7) and all(float(xt[c, r]) == (float(src[r, c]) if r < 3 else 0.0) for r in range(7) for c in range(5))
    idx = torch.tensor([2, -1, 0, 2, -5])
    got = R.gather_rows(dst, idx, cols=4)
    assert all(torch.equal(got[i], dst[j, :4] if j >= 0 else torch.zeros(4, dtype=BF16)) for i, j in enumerate(idx.tolist()))


# ---- conversion ---------------------------------------------------------------------------------------------------------------------------------
BF16_TIES = [  # fp32 bits -> bf16 bits, worked by hand: the dropped half is 0x8000 at a tie, which goes to the even neighbour
    (0x3F808000, 0x3F80), (0x3F818000, 0x3F82), (0x3F808001, 0x3F81), (0x3F807FFF, 0x3F80), (0x7F7F8000, 0x7F80), (0x7F7F7FFF, 0x7F7F),
    (0x00008000, 0x0000), (0x00008001, 0x0001), (0x80018000, 0x8002), (0xFF800000, 0xFF80)]
F16_TIES = [  # fp32 bits -> fp16 bits
    (0x477FF000, 0x7C00),  # 65520 = the midpoint of 65504 and 2^16: ties to the even side, which is inf
    (0x477FEFFF, 0x7BFF),  # just below it: 65504
    (0xC77FF000, 0xFC00),
    (0x33000000, 0x0000),  # 2^-25, half the smallest subnormal: ties to even = 0
    (0x33000001, 0x0001), (0x32FFFFFF, 0x0000), (0xB3000000, 0x8000),
    (0x33C00000, 0x0002),  # 3 * 2^-25, between subnormals 1 and 2: even = 2
    (0x387FE000, 0x0400),  # 2047 * 2^-25, between the largest subnormal and the smallest normal: even = 0x0400
    (0x3F801000, 0x3C00),  # 1 + 2^-11 -> 1
    (0x3F803000, 0x3C02),  # 1 + 3 * 2^-11 -> 1 + 2 * 2^-10
    (0x7F800000, 0x7C00)]


@pytest.mark.parametrize("dtype,ties", [(BF16, BF16_TIES), (F16, F16_TIES)])
def test_conversion_sweep_and_torch_rounding_on_hand_computed_ties(dtype, ties):
    x = R.convert_cases(dtype)
    xb = set(x.view(torch.int32).numpy().view(np.uint32).tolist())
    assert all(b in xb for b, _ in ties)  # the sweep holds every hand-computed case
    got = R.bits16(R.f32_from_bits([b for b, _ in ties]).to(dtype)).tolist()
    assert got == [w for _, w in ties], [hex(v) for v in got]
    y = x.to(dtype)
    assert torch.equal(torch.isnan(y), torch.isnan(x)) and int(torch.isnan(x).sum()) > 0
    if dtype == BF16:
        finite_or_inf = set(range(0x7F81)) | set(range(0x8000, 0xFF81))
        assert x.numel() == 6 * 65536 and set(R.bits16(y[~torch.isnan(y)]).tolist()) == finite_or_inf  # every non-NaN bf16
    else:
        assert 0x477FF000 in xb and 0xC77FF000 in xb and 0x33000000 in xb and 0xB3000000 in xb
        assert set(R.bits16(y[~torch.isnan(y)]).tolist()) == set(range(0x7C01)) | set(range(0x8000, 0xFC01))  # every non-NaN fp16
    # widening every 16-bit pattern and rounding it back is the identity (NaNs stay NaNs)
    a = R.all16(dtype)
    back = a.float().to(dtype)
    keep = ~torch.isnan(a.float())
    assert torch.equal(R.bits16(back)[keep], R.bits16(a)[keep]) and bool(torch.isnan(back.float()[~keep]).all())
