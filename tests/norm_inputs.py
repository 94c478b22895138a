"""Inputs of the norm-kernel tests (tests/test_norm_arms_gpu.py on the GPU, the mutants of tests/test_numerics_cpu.py on the CPU): seeded, made
on the CPU, in the 16-bit type (or fp32 for the fp32 stream's reader).  Every input with at least 6 rows carries the EDGE ROWS

    row 1   all zero                       rstd = rsqrt(eps); an RMSNorm y of exactly zero, a LayerNorm y of exactly b
    row 2   randn x 1e-3                   eps decides the scale
    row 3   randn x 1e4 (bf16) / x 200 (fp16: 1e4 randn overflows it)
    row 4   30 + randn (LayerNorm only)    a mean 30 times the spread: a variance taken as E[x^2] - mu^2 in fp32 loses it

and `block_ranges` restates the row partition of the backward and column-sum launchers (csrc/norm.hip partials_for)."""
import torch

EPS = float(torch.tensor(1e-5, dtype=torch.float32))  # the C ABI takes eps as `float`: the references use that value
BIG = {torch.bfloat16: 1e4, torch.float16: 200.0}
ROWS_PER_WAVE_BLOCK, MAX_PARTIALS = 4, 1024


def _edges(x, dtype, ln, zero_row):
    rows = x.shape[0]
    if rows >= 6:
        x[1] = 0
        x[2] *= 1e-3
        x[3] *= BIG[dtype]
        if ln:
            x[4] += 30
    elif zero_row and rows >= 2:
        x[1] = 0
    return x


def norm_inputs(rows, d, dtype, ln, *, zero_row=False, seed=0):
    """-> dict x, dy, old [rows, d], w, b, dw_old, db_old [d] in `dtype` on the CPU (b, db_old: LayerNorm's, None otherwise).  zero_row: an
    all-zero row 1 even below 6 rows (the fused quantiser's inputs)."""
    g = torch.Generator().manual_seed(1000003 * seed + 31 * rows + d + (7 if ln else 0))
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x = _edges(rn(rows, d), dtype, ln, zero_row).to(dtype)
    out = {"x": x, "dy": rn(rows, d).to(dtype), "old": rn(rows, d).to(dtype), "w": (1 + 0.1 * rn(d)).to(dtype), "dw_old": rn(d).to(dtype),
           "b": None, "db_old": None}
    if ln:
        out["b"], out["db_old"] = (0.1 * rn(d)).to(dtype), rn(d).to(dtype)
    return out


def f32_inputs(rows, d, dtype, ln, *, seed=0):
    """-> dict x32 fp32 [rows, d] (not representable in 16 bits: its 16-bit copy is a real rounding), w, b in `dtype`."""
    g = torch.Generator().manual_seed(2000003 * seed + 31 * rows + d + (7 if ln else 0))
    x = _edges(torch.randn(rows, d, generator=g), dtype, ln, False)
    return {"x32": x, "w": (1 + 0.1 * torch.randn(d, generator=g)).to(dtype), "b": (0.1 * torch.randn(d, generator=g)).to(dtype) if ln else None}


def colsum_view(buf, rows, d, ld, offset=0):
    """x [rows, d] with row stride ld, `offset` elements into the flat buffer (offset 1: rows that are not 16-byte aligned)."""
    return buf[offset:offset + rows * ld].view(rows, ld)[:, :d]


def colsum_inputs(rows, d, ld, dtype, *, offset=0, seed=0):
    """-> (flat buffer of rows * ld + offset elements - x is colsum_view of it, on whichever device it is moved to -, old [d]) in `dtype`."""
    g = torch.Generator().manual_seed(3000003 * seed + 31 * rows + d + ld + offset)
    x32 = torch.randn(rows * ld + offset, generator=g)
    x = colsum_view(x32, rows, d, ld, offset)
    if rows >= 6:
        x[1] = 0
        x[2] *= 1e-3
        x[3] *= BIG[dtype]
    return x32.to(dtype), torch.randn(d, generator=g).to(dtype)


def partials_for(rows):
    return min(MAX_PARTIALS, (rows + ROWS_PER_WAVE_BLOCK - 1) // ROWS_PER_WAVE_BLOCK)


def block_ranges(rows):
    """-> (nblk, rows_per_block, [(r0, r1) per block]); r0 >= r1 for a block that owns no row (it still writes a zero partial row)."""
    nblk = partials_for(rows)
    rpb = (rows + nblk - 1) // nblk
    return nblk, rpb, [(b * rpb, min(rows, b * rpb + rpb)) for b in range(nblk)]
