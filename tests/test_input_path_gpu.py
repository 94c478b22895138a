"""The kernels that carry a batch into and out of the model, held per element to tests/input_path_ref.py: the image-feature splice table, the
embedding gather and scatter, the patch im2col and the ViT assemble, the 2-D copy, the padded transpose, the row gathers and the dtype
conversion.  All but the scatter's fp32 sums are exact operations and are compared bit for bit; the sums are held to the bound of fp32
summation in any order.  Every output lives inside a larger buffer filled with a canary, and everything outside the declared result must
come back unchanged.  Shapes: the smallest that reach each branch - a thread's chunk of 1, 2, 3 and 16 positions in the splice kernel, the
wrap of each grid-stride loop, whole tiles beyond the transposed rows, each single broken alignment of the row gather."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import input_path_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF16, F16]
PAD = 64  # guard elements on either side of an output (a multiple of 16 bytes for every dtype)


def dev():
    return torch.device("cuda:0")


def rnd(*shape, dtype=torch.bfloat16, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev())


@pytest.fixture(scope="module")
def ops():
    from merlin_amd import ops as O

    assert O.arch_ok(0), "not a gfx950 device"
    return O


@pytest.fixture(scope="module")
def L():
    from merlin_amd import _lib

    return _lib


class Guard:
    """An output of `shape` in the middle of a canary-filled buffer: .t is the output, intact() says the cells around it are unchanged."""

    def __init__(self, shape, dtype, canary=7, shift=0):
        self.n, self.canary, self.shift = math.prod(shape), canary, shift
        self.buf = torch.full((self.n + 2 * PAD,), canary, dtype=dtype, device=dev())
        self.t = self.buf[PAD + shift:PAD + shift + self.n].view(shape)

    def intact(self):
        lo, hi = self.buf[:PAD + self.shift], self.buf[PAD + self.shift + self.n:]
        return bool((lo == self.canary).all()) and bool((hi == self.canary).all())

    def untouched(self):
        return bool((self.buf == self.canary).all())


def bits(t):
    """A tensor's patterns (16- or 32-bit) on the CPU, as integers."""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(got, want):
    return torch.equal(bits(got), bits(want))


# ---- a. the splice table ------------------------------------------------------------------------------------------------------------------------
def _splice(ops, L, ids, n_img, P, rpi, row0):
    B, S = ids.shape
    src = Guard((B, S), torch.int32, canary=-7)
    err = torch.tensor([0, 0, 0, 0] + [-7] * 8, dtype=torch.int32, device=dev())
    L.call("mh_splice_index", ids.to(dev()), R.offsets(n_img).to(dev()), src.t, err, B, S, P, R.PATCH, R.START, R.END, P if rpi is None else rpi, row0,
           ops._stream())
    assert src.intact() and err[4:].tolist() == [-7] * 8
    return src.t.cpu(), err[:4].tolist()


@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("S", [16, 255, 256, 257, 700, 4096])
def test_splice_index_bit_exact(ops, L, S, P):
    good, bad = R.splice_batches(S, P)
    variants = [(None, 0), (P + 1, 1)] + ([(577, 1)] if P == 4 else [])
    for name, ids, n_img in good:
        for rpi, row0 in variants:
            want, _ = R.splice_table(ids, R.offsets(n_img), P, rows_per_img=rpi, row0=row0)
            got, err = _splice(ops, L, ids, n_img, P, rpi, row0)
            assert err == [0, 0, 0, 0], (name, rpi, err)
            assert torch.equal(got, want), (name, rpi, (got != want).nonzero()[:4].tolist())
    for name, ids, n_img, b, err_want in bad:
        for rpi, row0 in variants[:2]:
            want, e = R.splice_table(ids, R.offsets(n_img), P, rows_per_img=rpi, row0=row0)
            assert e == err_want and bool((want[b] == -1).all())
            got, err = _splice(ops, L, ids, n_img, P, rpi, row0)
            assert err == err_want, (name, err)
            assert torch.equal(got, want), (name, (got != want).nonzero()[:4].tolist())
    # rows_per_img too small for row0 + P: refused, nothing written
    name, ids, n_img = good[0]
    src = Guard(tuple(ids.shape), torch.int32, canary=-7)
    err = torch.zeros(12, dtype=torch.int32, device=dev())
    for rpi, row0 in ((P - 1, 0), (P, 1), (P + 1, 2)):
        rc = L.launch("mh_splice_index", ids.to(dev()), R.offsets(n_img).to(dev()), src.t, err, ids.shape[0], S, P, R.PATCH, R.START, R.END, rpi, row0,
                      ops._stream())
        assert rc == L.DEFINES["MH_ERR_ARG"]
    assert src.untouched() and err.tolist() == [0] * 12


def test_splice_index_at_and_beyond_the_image_limit(ops, L):
    """1024 images in a sample are placed; 1025 starts with 1024 images too (zip); 1025 of both are refused: err[1], the sample, the position of
    the 1025th start, and no feature row for that sample (before the fix: the 1025th image silently kept its token embeddings)."""
    S, P = 4096, 1
    rows = torch.stack([R.place(S, P, [3 * k for k in range(n)], seed=n) for n in (1024, 1025, 1025)])
    for order in ([0, 1, 2], [2, 0, 1]):
        n_img = [[1024, 1024, 1025][i] for i in order]
        ids = rows[order]
        want, err_want = R.splice_table(ids, R.offsets(n_img), P, rows_per_img=2, row0=1, max_images=1024)
        b = order.index(2)
        assert err_want == [0, 1, b, 3 * 1024] and bool((want[b] == -1).all()) and int((want >= 0).sum()) == 2048
        got, err = _splice(ops, L, ids, n_img, P, 2, 1)
        assert err == err_want, err
        assert torch.equal(got, want), (got != want).nonzero()[:4].tolist()
    # without the third sample: no error at all
    got, err = _splice(ops, L, rows[:2], [1024, 1024], P, None, 0)
    assert err == [0, 0, 0, 0] and torch.equal(got, R.splice_table(rows[:2], R.offsets([1024, 1024]), P)[0])


# ---- b. embedding gather ------------------------------------------------------------------------------------------------------------------------
def _patterns16(rows, d, dtype, seed):
    """Arbitrary 16-bit patterns (NaNs, infinities, subnormals included): a gather is a copy of bits."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-32768, 32768, (rows, d), generator=g, dtype=torch.int32).to(torch.int16).view(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,d", R.EMBED_SHAPES)
def test_embed_splice_fwd_and_gather_rows_bit_exact(ops, L, T, d, dtype):
    c = R.embed_case(T, d)
    ids, src = c["ids"].to(dev()), c["src"].to(dev())
    emb, feats = _patterns16(R.N_EMBED, d, dtype, 1), _patterns16(c["n_feat"], d, dtype, 2)
    for s_cpu, f_cpu in ((c["src"], feats), (None, feats), (None, None)):
        out = Guard((T, d), dtype)
        L.call("mh_embed_splice_fwd", ids, None if s_cpu is None else src, emb.to(dev()), None if f_cpu is None else feats.to(dev()), out.t, T, d,
               ops.dt_of(dtype), ops._stream())
        want = R.embed_splice(c["ids"], s_cpu, emb.view(torch.int16), None if s_cpu is None else feats.view(torch.int16))
        assert torch.equal(bits(out.t), want) and out.intact()
    out = Guard((T, d), dtype)
    assert ops.gather_rows(emb.to(dev()), ids, out=out.t) is out.t
    assert torch.equal(bits(out.t), emb.view(torch.int16)[c["ids"]]) and out.intact()
    # src without feats is refused
    assert L.launch("mh_embed_splice_fwd", ids, src, emb.to(dev()), None, out.t, T, d, ops.dt_of(dtype), ops._stream()) == L.DEFINES["MH_ERR_ARG"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,d", R.EMBED_SHAPES)
def test_embed_splice_fwd_f32_bit_exact(ops, L, T, d, dtype):
    c = R.embed_case(T, d)
    ids, src = c["ids"].to(dev()), c["src"].to(dev())
    emb = rnd(R.N_EMBED, d, dtype=dtype, seed=3)
    feats = rnd(c["n_feat"], d, dtype=F32, seed=4)
    for s_cpu, with_feats in ((c["src"], True), (None, True), (None, False)):
        out = Guard((T, d), F32)
        L.call("mh_embed_splice_fwd_f32", ids, None if s_cpu is None else src, emb, feats if with_feats else None, out.t, T, d, ops.dt_of(dtype),
               ops._stream())
        want = R.embed_splice(c["ids"], s_cpu, emb.cpu().float(), feats.cpu())
        assert same_bits(out.t, want) and out.intact()


# ---- c. embedding scatter -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,d", R.EMBED_SHAPES)
def test_embed_splice_bwd_copy_exact_and_sums_within_the_fp32_bound(ops, L, T, d, dtype):
    """dfeats: the mapped rows are copies of dout's, the others (the CLS rows) keep the canary.  dembed32: per element within
    gamma_{n-1} * sum |terms| of the float64 sum, n = contributions to the row (+ 1 for a non-zero start): the bound of fp32 addition in any
    order, so a row with one contribution, or none, is exact.  dout has magnitudes in [0.5, 2): a lost or repeated atomic is off by >= 0.5."""
    c = R.embed_case(T, d)
    ids, src = c["ids"].to(dev()), c["src"].to(dev())
    dout = R.signed_magnitudes((T, d), dtype, 5)
    dout_d = dout.to(dev())
    sel = c["src"] >= 0
    want_feats = torch.full((c["n_feat"], d), 7.0, dtype=dtype)
    want_feats[c["src"][sel].long()] = dout[sel]
    assert int((want_feats == 7).all(1).sum()) == c["n_feat"] // (c["P"] + 1)  # the CLS rows

    def run(use_src, use_feats, init):
        dfe = Guard((c["n_feat"], d), dtype)
        dem = None
        if init is not None:
            dem = Guard((R.N_EMBED, d), F32)
            dem.t.copy_(init)
        L.call("mh_embed_splice_bwd", ids, src if use_src else None, dout_d, dfe.t if use_feats else None, None if dem is None else dem.t, T, d,
               ops.dt_of(dtype), ops._stream())
        assert dfe.intact() and (dem is None or dem.intact())
        return dfe, dem

    def hold_sums(dem, init, s_cpu, what):
        _, ref, mag, count = R.embed_splice_grads(c["ids"], s_cpu, dout, c["n_feat"], R.N_EMBED)
        i64 = init.cpu().double()
        n = count[:, None] + (i64 != 0)
        bound = R.sum_bound(n) * (mag + i64.abs())
        err = (dem.t.cpu().double() - (ref + i64)).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"IP | embed_splice_bwd {what} T={T} d={d} {str(dtype)[6:]} | max n = {int(n.max())} | worst err / bound = {worst:.3f}")
        assert bool((err <= bound).all()), (what, (err > bound).nonzero()[:4].tolist())
        assert same_bits(dem.t.cpu()[count == 0], init.cpu()[count == 0])  # rows that receive nothing: exactly what was there

    zero = torch.zeros(R.N_EMBED, d, device=dev())
    start = rnd(R.N_EMBED, d, dtype=F32, seed=6)
    for init, what in ((zero, "from zero"), (start, "accumulating")):
        dfe, dem = run(True, True, init)
        assert same_bits(dfe.t, want_feats)
        hold_sums(dem, init, c["src"], what)
    dfe, dem = run(True, False, start)                       # dfeats = NULL: the table's gradient alone
    assert dfe.untouched()
    hold_sums(dem, start, c["src"], "dfeats NULL")
    dfe, dem = run(True, True, None)                         # dembed32 = NULL: the features' gradient alone
    assert same_bits(dfe.t, want_feats)
    dfe, dem = run(False, True, start)                       # src = NULL: every position is a token
    assert dfe.untouched()
    hold_sums(dem, start, None, "src NULL")


# ---- d. CLIP input pieces -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pix_dtype", [F32, BF16, F16])
@pytest.mark.parametrize("N,img,ps,kpad", [(3, 56, 14, 640), (1, 28, 14, 592), (13, 112, 14, 640)])
def test_im2col_patches_bit_exact(ops, N, img, ps, kpad, pix_dtype, dtype):
    G2 = (img // ps) ** 2
    pix = rnd(N, 3, img, img, dtype=pix_dtype, seed=7)
    for rpi, row0 in ((None, 0), (G2 + 1, 1), (G2 + 3, 2)):
        rows = N * (G2 + row0 if rpi is None else rpi)
        out = Guard((rows, kpad), dtype)
        ops.im2col_patches(pix, ps, kpad, dtype, rows_per_img=rpi, row0=row0, out=out.t)
        want = R.im2col(pix.cpu(), ps, kpad, dtype, rpi, row0)
        assert same_bits(out.t, want) and out.intact(), (rpi, row0)
        w3 = bits(out.t).view(N, -1, kpad)
        assert int(w3[:, :row0].abs().max() if row0 else 0) == 0 and int(w3[:, row0 + G2:].abs().sum()) == 0 and int(w3[:, :, 3 * ps * ps:].abs().sum()) == 0
    assert (13 * 64 * 640 + 255) // 256 > 2048  # the third geometry wraps the grid in every row layout


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,G2,d", [(3, 16, 128), (1, 1, 8), (17, 256, 1024)])
def test_vit_assemble_both_forms_bit_exact(ops, L, N, G2, d, dtype):
    rows = N * (G2 + 1)
    cls, pos = rnd(d, dtype=dtype, seed=8), rnd(G2 + 1, d, dtype=dtype, seed=9)
    for pdt in (dtype, F32):
        patch = rnd(rows, d, dtype=pdt, seed=10)
        patch.view(N, G2 + 1, d)[:, 0] = float("nan")  # the CLS slot of the patch rows is not read
        out = Guard((rows, d), pdt)
        if pdt == F32:
            L.call("mh_vit_assemble_f32", patch, cls, pos, out.t, N, G2, d, ops.dt_of(dtype), ops._stream())
        else:
            L.call("mh_vit_assemble", patch, cls, pos, out.t, N, G2, d, ops.dt_of(dtype), ops._stream())
        want = R.vit_assemble(patch.cpu(), cls.cpu(), pos.cpu(), N, G2, pdt)
        assert not bool(torch.isnan(want.float()).any())
        assert same_bits(out.t, want) and out.intact(), pdt


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols,lds,ldd", [(128, 588, 600, 640), (128, 588, 640, 588), (33, 1, 3, 5), (900, 588, 588, 640)])
def test_copy2d_and_accumulate_bit_exact(ops, rows, cols, lds, ldd, dtype):
    src = rnd(rows, lds, dtype=dtype, seed=11)
    for accumulate in (False, True):
        dst = Guard((rows, ldd), dtype)
        if accumulate:
            dst.t.copy_(rnd(rows, ldd, dtype=dtype, seed=12))
        before = dst.t.cpu().clone()
        ops.copy2d(src[:, :cols], dst.t, accumulate=accumulate)
        want = R.copy2d(src.cpu()[:, :cols], before, accumulate)
        assert same_bits(dst.t, want) and dst.intact(), accumulate
        assert same_bits(dst.t[:, cols:], before[:, cols:])
    assert (900 * 588 + 255) // 256 > 2048


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Rr,Cc,r_pad", [(613, 200, 640), (64, 64, 64), (65, 1, 256), (1, 130, 64)])
def test_transpose16_strided_input_padded_output(ops, Rr, Cc, r_pad, dtype):
    wide = rnd(Rr, Cc + 5, dtype=dtype, seed=13)
    x = wide[:, 3:3 + Cc]                      # a column slice: ldi = Cc + 5
    out = Guard((Cc, r_pad + 8), dtype)        # a row-strided destination: ldo = r_pad + 8
    ops.transpose16(x, r_pad=r_pad, out=out.t[:, :r_pad])
    want = torch.full((Cc, r_pad + 8), 7.0, dtype=dtype)
    want[:, :r_pad] = R.transpose_pad(x.cpu(), r_pad)
    assert same_bits(out.t, want) and out.intact()
    assert int(bits(out.t[:, Rr:r_pad]).abs().sum()) == 0


def _gather2d(ops, L, src, idx, dst, width_bytes):
    return L.launch("mh_gather_rows2d", src, src.stride(0) * src.element_size(), idx, dst, dst.stride(0) * dst.element_size(), idx.numel(), width_bytes,
                    ops._stream())


@pytest.mark.parametrize("broken", ["nothing", "source stride", "destination stride", "width", "source pointer", "destination pointer"])
def test_gather_rows2d_each_alignment_alone(ops, L, broken):
    """32-bit cells, so one cell is the 4 bytes that break a 16-byte alignment.  From a case in which both strides, the width and both pointers
    allow 16-byte accesses, each of the five is moved by 4 bytes alone: the result is src[idx] (zeros for idx < 0) either way."""
    n_src, width, lds, ldd = 23, 16, 32, 48
    lds += broken == "source stride"
    ldd += broken == "destination stride"
    width += broken == "width"
    g = torch.Generator().manual_seed(14)
    store = torch.randint(-2 ** 31, 2 ** 31 - 1, (n_src * lds + 4,), generator=g, dtype=torch.int64).to(torch.int32).to(dev())
    s0 = 1 if broken == "source pointer" else 0
    src = store[s0:s0 + n_src * lds].view(n_src, lds)
    idx = torch.tensor([5, 5, -1, 0, 22, 5, -3, 11, 0, 22, 1] * 3 + [7], dtype=torch.int64)
    dst = Guard((idx.numel(), ldd), torch.int32, shift=1 if broken == "destination pointer" else 0)
    aligned = [src.data_ptr() % 16 == 0, dst.t.data_ptr() % 16 == 0, lds % 4 == 0, ldd % 4 == 0, width % 4 == 0]
    assert aligned.count(False) == (0 if broken == "nothing" else 1)
    assert _gather2d(ops, L, src, idx.to(dev()), dst.t, 4 * width) == 0
    want = torch.full((idx.numel(), ldd), 7, dtype=torch.int32)
    want[:, :width] = R.gather_rows(src.cpu(), idx, cols=width)
    assert torch.equal(dst.t.cpu(), want) and dst.intact()
    assert bool((want[idx < 0, :width] == 0).all())


def test_gather_rows2d_wrap_of_the_4_byte_arm_and_refusals(ops, L):
    rows, width = 1030, 1025  # 4100 bytes a row: 1030 * 1025 cells in 4-byte accesses are more than 4096 blocks of 256
    assert (rows * width + 255) // 256 > 4096 and (4 * width) % 16 != 0
    g = torch.Generator().manual_seed(15)
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (41, width), generator=g, dtype=torch.int64).to(torch.int32)
    idx = torch.randint(-3, 41, (rows,), generator=g)
    idx[:4] = torch.tensor([40, 0, -1, 40])
    dst = Guard((rows, width + 3), torch.int32)
    assert _gather2d(ops, L, src.to(dev()), idx.to(dev()), dst.t, 4 * width) == 0
    want = torch.full((rows, width + 3), 7, dtype=torch.int32)
    want[:, :width] = R.gather_rows(src, idx)
    assert torch.equal(dst.t.cpu(), want) and dst.intact()
    # a width that is no multiple of 4 bytes: refused, nothing written
    s16 = rnd(8, 8, dtype=BF16, seed=16)
    d16 = Guard((4, 8), BF16)
    rc = _gather2d(ops, L, s16, torch.tensor([1, 2, 3, 0], device=dev()), d16.t, 6)
    assert rc == L.DEFINES["MH_ERR_ARG"] and d16.untouched()


# ---- e. conversion ------------------------------------------------------------------------------------------------------------------------------
def _convert_and_compare(ops, L, x, dst_dtype, what):
    """mh_convert(x) against Tensor.to on the CPU: a NaN wherever the input is one, every other element bit for bit."""
    n = x.numel()
    out = Guard((n,), dst_dtype)
    L.call("mh_convert", x.to(dev()), ops.dt_of(x.dtype), out.t, ops.dt_of(dst_dtype), n, ops._stream())
    assert out.intact(), what
    got = out.t.cpu()
    want = x.float().to(dst_dtype)
    nan = torch.isnan(x.float())
    assert torch.equal(torch.isnan(got.float()), nan), what
    gb, wb = bits(got)[~nan], bits(want)[~nan]
    if not torch.equal(gb, wb):
        at = (gb != wb).nonzero().flatten()
        xb = bits(x)[~nan][at[:6]].tolist()
        raise AssertionError(f"{what}: {at.numel()} of {n} differ; inputs {[hex(v & 0xFFFFFFFF) for v in xb]} gave "
                             f"{[hex(v & 0xFFFF) for v in gb[at[:6]].tolist()]}, expected {[hex(v & 0xFFFF) for v in wb[at[:6]].tolist()]}")


def _tiled(x, n):
    return x.repeat((n + x.numel() - 1) // x.numel())[:n].contiguous()


@pytest.mark.parametrize("dtype", DTYPES)
def test_convert_f32_to_16_rounding_sweep(ops, L, dtype):
    """Every tie, its two neighbours and every exponent (tests/input_path_ref.py: convert_cases): round to nearest even, fp16 overflow to inf
    from 65520, fp32 subnormal inputs NOT flushed (bf16 keeps them as bf16 subnormals)."""
    x = R.convert_cases(dtype)
    _convert_and_compare(ops, L, x, dtype, f"f32 -> {dtype}")
    for n in (1, 7, 524288 + 5):  # one element, a partial vector, five past one pass of the whole grid
        _convert_and_compare(ops, L, _tiled(x[torch.randperm(x.numel(), generator=torch.Generator().manual_seed(n))], n), dtype, f"f32 -> {dtype} n={n}")


@pytest.mark.parametrize("a,b", [(BF16, F16), (F16, BF16), (BF16, F32), (F16, F32)])
def test_convert_from_16_bit_all_patterns(ops, L, a, b):
    x = R.all16(a)
    _convert_and_compare(ops, L, x, b, f"{a} -> {b}")
    for n in (1, 7, 524288 + 5):
        _convert_and_compare(ops, L, _tiled(x.flip(0), n), b, f"{a} -> {b} n={n}")


def test_convert_same_type_and_unknown_codes(ops, L):
    for dt in (BF16, F16):
        _convert_and_compare(ops, L, R.all16(dt), dt, f"{dt} -> itself")
    x = R.convert_cases(BF16)
    out = Guard((x.numel(),), F32)
    L.call("mh_convert", x.to(dev()), L.MH_F32, out.t, L.MH_F32, x.numel(), ops._stream())
    assert same_bits(out.t, x) and out.intact()
    # a dtype code outside {BF16, F16, F32} is refused (it used to be read as fp16) and nothing is written
    src = rnd(64, dtype=F32, seed=17)
    dst = Guard((64,), F32)
    for s, d in ((3, L.MH_F32), (L.MH_F32, 3), (-1, L.MH_BF16), (L.MH_F16, 7), (17, 17)):
        assert L.launch("mh_convert", src, s, dst.t, d, 64, ops._stream()) == L.DEFINES["MH_ERR_DTYPE"], (s, d)
    torch.cuda.synchronize()
    assert dst.untouched()
    assert L.launch("mh_convert", src, L.MH_F32, dst.t, L.MH_F32, 0, ops._stream()) == L.DEFINES["MH_ERR_ARG"]
