"""Plain CPU restatements of the kernels that carry a batch into and out of the model: the image-feature splice table, the embedding gather /
scatter, the CLIP patch im2col and assemble, the 2-D copy, the padded transpose, the row gather and the dtype conversion's rounding sweep.
Written from the semantics (include/merlin_hip.h and the reference model's per-sample loop), with plain torch / numpy; nothing here touches a
GPU.  tests/test_input_path_cpu.py checks them against independent formulations, tests/test_input_path_gpu.py holds the kernels to them.

Also here, because both files need them: the splice batches (`splice_batches`) and the embedding batches (`embed_case`) the tests run."""
import numpy as np
import torch

PATCH, START, END = 1000, 1001, 1002  # special ids of the test rows; text ids are < N_TEXT
N_TEXT = 100
U32 = 2.0 ** -24  # unit roundoff of fp32


# ---- splice table -----------------------------------------------------------------------------------------------------------------------------
def splice_table(ids, img_offset, P, patch=PATCH, start=START, end=END, rows_per_img=None, row0=0, max_images=None):
    """ids int64 [B, S], img_offset [B + 1] (exclusive prefix of images per sample) -> (src int32 [B, S], err [4]).
    src[b, s] = feature row of position s (global image g, patch j: g * rows_per_img + row0 + j) or -1 (keep the token embedding).
    Per sample, in the reference model's order: no patch token -> skipped; #start != #end -> err[0], err[2] = sample, err[3] = the
    difference; the starts are zipped with the sample's images (extras of either ignored) and an image whose end token is not at
    start + P + 1 inside the row -> err[1], err[3] = the start.  A sample that errs gets no row.  With several bad samples err[2..3] are
    the first one's.  max_images: the library's table size - a sample with more usable images errs (err[1]) at its first start beyond it."""
    ids = torch.as_tensor(ids)
    B, S = ids.shape
    rpi = P if rows_per_img is None else rows_per_img
    src = torch.full((B, S), -1, dtype=torch.int32)
    err = [0, 0, 0, 0]

    def flag(slot, b, what):
        if err[0] == 0 and err[1] == 0:
            err[2], err[3] = b, what
        err[slot] = 1

    for b in range(B):
        row = ids[b].tolist()
        if row.count(patch) == 0:
            continue
        starts = [s for s, v in enumerate(row) if v == start]
        n_end = row.count(end)
        if len(starts) != n_end:
            flag(0, b, len(starts) - n_end)
            continue
        n_img = int(img_offset[b + 1]) - int(img_offset[b])
        pairs = list(zip(starts, range(int(img_offset[b]), int(img_offset[b]) + n_img)))
        bad = next((s for s, _ in pairs[:max_images] if s + P + 1 >= S or row[s + P + 1] != end), None)
        if bad is None and max_images is not None and len(pairs) > max_images:
            bad = pairs[max_images][0]
        if bad is not None:
            flag(1, b, bad)
            continue
        for s, g in pairs:
            src[b, s + 1:s + 1 + P] = torch.arange(g * rpi + row0, g * rpi + row0 + P, dtype=torch.int32)
    return src, err


def _text(S, seed):
    return torch.randint(1, N_TEXT, (S,), generator=torch.Generator().manual_seed(seed))


def place(S, P, starts, seed=0, end_shift=0):
    """A row of S text ids with an image (START, P x PATCH, END) at every start; the pieces must not overlap.  Pieces that run past the
    row are cut there.  end_shift moves the END tokens (a misplaced end)."""
    row = _text(S, seed)
    used = torch.zeros(S + P + 3, dtype=torch.bool)
    for s in starts:
        assert 0 <= s < S and not bool(used[s:s + P + 2 + end_shift].any()), (S, P, s)
        used[s:s + P + 2 + end_shift] = True
        row[s] = START
        row[s + 1:min(S, s + 1 + P)] = PATCH
        if s + P + 1 + end_shift < S:
            row[s + P + 1 + end_shift] = END
    return row


def chunk_of(S):
    return (S + 255) // 256  # positions per thread of the 256-thread splice kernel


def packed_starts(S, P, n):
    """n images back to back, the last one's END at S - 1."""
    return [S - (P + 2) * k for k in range(n, 0, -1)]


def border_starts(S, P):
    """Starts that are the LAST position of a thread's chunk (their patches lie in the next chunk) and starts two before a chunk border (the
    patches straddle it), spread over the row."""
    c = chunk_of(S)
    out, nxt = [], 0
    for i, m in enumerate(range(1, S // c + 1, max(1, (S // c) // 7))):
        s = m * c - 1 - (2 if (i & 1) and m * c - 3 >= nxt else 0)
        if s >= nxt and s + P + 1 < S:
            out.append(s)
            nxt = s + P + 2
    return out


def splice_batches(S, P):
    """-> list of (name, ids [B, S], n_img per sample) without errors, then list of (name, ids, n_img, bad sample, err) with exactly one bad
    sample.  Every row shape the issue names occurs: see test_input_path_cpu.py::test_splice_batches_contain_every_named_situation."""
    fit = S // (P + 2)
    n_pack = min(fit, 300)
    packed = place(S, P, packed_starts(S, P, n_pack), seed=1)
    bs = border_starts(S, P)
    border = place(S, P, bs, seed=2)
    text_unbalanced = _text(S, 3)
    text_unbalanced[1], text_unbalanced[S // 2], text_unbalanced[S - 2] = START, START, END
    few = packed_starts(S - 1, P, min(fit, 2))  # (END at S - 2)
    more_images = place(S, P, few, seed=4)
    more_starts = place(S, P, few, seed=5)
    no_images = place(S, P, few[:1], seed=6)
    plain = _text(S, 7)
    good = [("packed|border|text|more images|more starts", torch.stack([packed, border, text_unbalanced, more_images, more_starts]),
             [n_pack, len(bs), 0, len(few) + 2, len(few) - 1]),
            ("no images|plain|border", torch.stack([no_images, plain, border]), [0, 0, len(bs)])]
    bad = []
    # an image whose END would be at S: START at S - P - 1; a stray END in front keeps the counts equal
    over = place(S, P, [S - P - 1], seed=8)
    over[0] = END
    bad.append(("end at S", torch.stack([packed, over, border]), [n_pack, 1, len(bs)], 1, [0, 1, 1, S - P - 1]))
    extra_start = more_images.clone()
    extra_start[0] = START
    bad.append(("one start too many", torch.stack([border, packed, extra_start]), [len(bs), n_pack, 1], 2, [1, 0, 2, 1]))
    extra_end = more_images.clone()
    extra_end[0], extra_end[1] = END, END
    bad.append(("two ends too many", torch.stack([extra_end, packed]), [1, n_pack], 0, [1, 0, 0, -2]))
    if S >= 2 * (P + 3):  # a second image whose END sits one place late (the first one is fine)
        late = place(S, P, [0], seed=9)
        late[P + 2:2 * P + 5] = place(P + 3, P, [0], seed=10, end_shift=1)
        bad.append(("late end", torch.stack([packed, border, plain, late]), [n_pack, len(bs), 0, 2], 3, [0, 1, 3, P + 2]))
    return good, bad


def offsets(n_img):
    return torch.tensor([0] + list(np.cumsum(n_img)), dtype=torch.int32)


# ---- embedding gather / scatter -----------------------------------------------------------------------------------------------------------------
def embed_splice(ids, src, embed, feats):
    """out[t] = feats[src[t]] where src[t] >= 0, else embed[ids[t]].  src None: a plain gather.  feats in any dtype: the result has it."""
    ids = ids.reshape(-1).long()
    out = embed[ids].to(embed.dtype if feats is None else feats.dtype)
    if src is not None:
        sel = src.reshape(-1) >= 0
        out[sel] = feats[src.reshape(-1)[sel].long()]
    return out


def embed_splice_grads(ids, src, dout, n_feat, n_embed):
    """float64 (dfeats [n_feat, d], dembed [n_embed, d], abs-sum of dembed's terms, contributions per embedding row) of embed_splice."""
    ids = ids.reshape(-1).long()
    d = dout.shape[1]
    sel = (src.reshape(-1) >= 0) if src is not None else torch.zeros(ids.numel(), dtype=torch.bool)
    g = dout.double()
    dfeats = torch.zeros(n_feat, d, dtype=torch.float64)
    if src is not None:
        dfeats.index_add_(0, src.reshape(-1)[sel].long(), g[sel])
    dembed = torch.zeros(n_embed, d, dtype=torch.float64).index_add_(0, ids[~sel], g[~sel])
    mag = torch.zeros(n_embed, d, dtype=torch.float64).index_add_(0, ids[~sel], g[~sel].abs())
    count = torch.bincount(ids[~sel], minlength=n_embed)
    return dfeats, dembed, mag, count


def sum_bound(n):
    """gamma_{n-1} = (n - 1) u / (1 - (n - 1) u): |fl(sum of n terms) - sum| <= gamma_{n-1} * sum |terms| for fp32 addition in ANY order."""
    k = (n.double() - 1).clamp_min(0) * U32
    return k / (1 - k)


EMBED_SHAPES = [(48, 64), (5, 8), (1040, 4096), (700, 1536)]  # (T, d); 1040 * 4096 / 8 work items wrap the 2048-block grid
N_EMBED = 203


def embed_case(T, d, seed=0):
    """-> dict ids [T] (token ids and image pieces), src int32 [T] from a rows_per_img = P + 1, row0 = 1 table, n_feat, P, pad id.  The pad id
    fills the tail (hundreds of repeats where T allows), the first and the last table row occur, some ids occur exactly once, some never."""
    B, S, P, n_per = {48: (3, 16, 4, 2), 5: (1, 5, 1, 1), 1040: (2, 520, 4, 9), 700: (1, 700, 4, 5)}[T]
    g = torch.Generator().manual_seed(seed + T)
    rows = []
    pad = 7
    for b in range(B):
        starts = [1 + (P + 3) * k for k in range(n_per)] if S > 5 else [0]
        row = place(S, P, starts, seed=seed + b)
        text = (row < N_TEXT).nonzero().flatten()
        row[text] = torch.randint(20, 60, (text.numel(),), generator=g)  # repeats among 40 ids
        tail = text[text > starts[-1] + P + 1]
        row[tail[len(tail) // 16:]] = pad
        rows.append(row)
    ids = torch.stack(rows)
    if S > 5:
        free = (ids[0] < N_TEXT).nonzero().flatten()
        ids[0, free[0]], ids[0, free[1]], ids[0, free[2]] = 0, N_EMBED - 1, 150  # first / last table row, an id that occurs once
    n_img = [n_per] * B
    src, err = splice_table(ids, offsets(n_img), P, rows_per_img=P + 1, row0=1)
    assert err[:2] == [0, 0]
    # the special ids index rows of the table too (the START / END embeddings are real rows): map them into it
    tok = ids.clone()
    tok[ids == PATCH], tok[ids == START], tok[ids == END] = N_EMBED - 4, N_EMBED - 3, N_EMBED - 2
    return dict(ids=tok.reshape(-1), src=src.reshape(-1), n_feat=sum(n_img) * (P + 1), P=P, pad=pad)


def signed_magnitudes(shape, dtype, seed):
    """Random signs x magnitudes in [0.5, 2), rounded to dtype: a dropped or doubled term of a sum of n of them moves it by >= 0.5."""
    g = torch.Generator().manual_seed(seed)
    mag = 0.5 + 1.5 * torch.rand(shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return (sign * mag).to(dtype).clamp(-1.9921875, 1.9921875)


# ---- CLIP input pieces --------------------------------------------------------------------------------------------------------------------------
def im2col(pixels, ps, kpad, dtype, rows_per_img=None, row0=0):
    """pixels [N, 3, H, H] -> cols [N * rows_per_img, kpad] in dtype: patch p of image n (row-major over the G x G grid) at row
    n * rows_per_img + row0 + p as (channel, y, x), everything else zero.  Pixels are rounded to dtype first."""
    N, _, H, _ = pixels.shape
    G = H // ps
    rpi = G * G + row0 if rows_per_img is None else rows_per_img
    K = 3 * ps * ps
    patches = torch.nn.functional.unfold(pixels.to(dtype).float(), ps, stride=ps).transpose(1, 2)  # [N, G*G, K]
    cols = torch.zeros(N, rpi, kpad)
    cols[:, row0:row0 + G * G, :K] = patches
    return cols.reshape(N * rpi, kpad).to(dtype)


def vit_assemble(patch, cls, pos, N, G2, out_dtype):
    """patch [N * (G2 + 1), d] (16-bit or fp32; its CLS slots are ignored), cls [d], pos [G2 + 1, d] -> x [N * (G2 + 1), d] = fp32 sum
    rounded once to out_dtype."""
    d = patch.shape[1]
    x = patch.float().reshape(N, G2 + 1, d).clone()
    x[:, 0] = cls.float()
    return (x + pos.float()[None]).reshape(N * (G2 + 1), d).to(out_dtype)


def copy2d(src, dst, accumulate):
    """-> the new dst: its [rows, cols] corner (=|+=) src, the sum in fp32 rounded once."""
    out = dst.clone()
    r, c = src.shape
    out[:r, :c] = (dst[:r, :c].float() + src.float()).to(dst.dtype) if accumulate else src
    return out


def transpose_pad(x, r_pad):
    R, Cc = x.shape
    out = torch.zeros(Cc, r_pad, dtype=x.dtype)
    out[:, :R] = x.t()
    return out


def gather_rows(src, idx, cols=None):
    """out[i] = src[idx[i], :cols]; a zero row where idx[i] < 0."""
    cols = src.shape[1] if cols is None else cols
    out = src[idx.clamp_min(0), :cols].clone()
    out[idx < 0] = 0
    return out


# ---- dtype conversion ---------------------------------------------------------------------------------------------------------------------------
def f32_from_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(bits, dtype=np.uint32)).view(np.float32).copy())


def bits16(t):
    """16-bit tensor -> its patterns as int32 in [0, 65536)."""
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def all16(dtype):
    """All 65536 patterns of a 16-bit dtype, in order."""
    return torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16).copy()).view(dtype)


def convert_cases(dst_dtype):
    """fp32 inputs of the rounding sweep.  bf16: all 65536 upper halves x lower halves {0, 1, 0x7fff, 0x8000, 0x8001, 0xffff} (below, at and
    above every tie, every exponent, subnormals, inf, NaN).  fp16: for every finite fp16 magnitude and its successor (inf = 65536 past the
    largest) the value, the exact midpoint and the midpoint -+ one fp32 ulp, both signs (this holds +-65520, the overflow threshold, and
    +-2^-25, half the smallest subnormal), then +-inf, fp32 subnormals and NaNs."""
    if dst_dtype == torch.bfloat16:
        hi = np.arange(65536, dtype=np.uint32)[:, None] << 16
        lo = np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=np.uint32)[None]
        return f32_from_bits((hi | lo).reshape(-1))
    assert dst_dtype == torch.float16
    m = np.arange(0x7C00, dtype=np.uint16)
    a = m.view(np.float16).astype(np.float64)
    b = np.append(a[1:], 65536.0)
    mid = ((a + b) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (a + b) / 2)  # every midpoint is an fp32 number
    mb = mid.view(np.uint32)
    mag = np.concatenate([a.astype(np.float32).view(np.uint32), mb, mb - 1, mb + 1,
                          np.array([0x7F800000, 0x7FC00000, 0x7F800001, 0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF], dtype=np.uint32)])
    return f32_from_bits(np.concatenate([mag, mag | np.uint32(0x80000000)]))
