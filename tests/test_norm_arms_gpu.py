"""csrc/norm.hip, every dispatch arm and row partition, PER ELEMENT (tests/numerics.py): the launchers choose a kernel form from d, rows and
pointer alignment, and each test id names the arm its shape selects.

    norm_bwd_k<DT, LN, NCH>     NCH in {1, 2, 4, 8} from ceil(d / 512), with full, partly filled (one live lane) and wholly dead register chunks;
                                the row partition nblk = min(1024, ceil(rows / 4)), rows_per_block = ceil(rows / nblk): one block, an idle wave,
                                rows_per_block 5 and 9 (a wave's row loop runs more than once), blocks that own no row
    rmsnorm_fwd_row_k / _fwd_k  both sides of rows 64 / 65 and d 8192 / 8200, with the rstd output no caller requests
    layernorm_fwd_k, rmsnorm_fwd_q8_k<NCH = 8 | 0>, norm_fwd_f32in_k<LN, Y32, NCH = 8 | 2 | 0>
    colsum_partial_v8_k         with its 4-rows-in-flight main loop (rows_per_block >= 32), colsum_partial_k by d % 8 and by alignment alone

Inputs come from tests/norm_inputs.py (CPU, seeded, with the edge rows described there); every bound is numerics.limit(c_model) with the model
evaluated here on the same inputs, and each check prints its `CW | ...` line first (test_componentwise_gpu.hold).  Every output is the leading
part of a buffer whose trailing row holds a sentinel (the kernels write nothing past their output) and is pre-filled with NaN, partial
workspaces included: an element or a partial row that a block leaves unwritten stays NaN and the checker refuses it."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import norm_inputs as NI  # noqa: E402
import numerics as N  # noqa: E402
from test_componentwise_gpu import dev, hold  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="fp16")]
F32 = torch.float32
EPS = NI.EPS
SENTINEL = {torch.float32: 12345.5, torch.bfloat16: -7.0, torch.float16: -7.0, torch.uint8: 0xA5}


@pytest.fixture(scope="module")
def ops():
    from merlin_amd import ops as O

    assert O.arch_ok(0), "not a gfx950 device"
    return O


def L():
    from merlin_amd import _lib

    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def on_dev(inputs):
    return {k: (v.to(dev()) if isinstance(v, torch.Tensor) else v) for k, v in inputs.items()}


def guarded(shape, dtype, init=None):
    """-> (out, buf): `out` of `shape` is the leading part of `buf`, whose trailing row (one more row of a matrix, max(n, 16) more elements of a
    vector) holds the sentinel.  out starts as NaN (0xFF bytes) or as a copy of `init` (the accumulating forms)."""
    shape = tuple(shape)
    n = 1
    for s in shape:
        n *= s
    tail = max(shape[-1], 16)
    buf = torch.full((n + tail,), 0xFF if dtype == torch.uint8 else float("nan"), dtype=dtype, device=dev())
    buf[n:] = SENTINEL[dtype]
    out = buf[:n].view(shape)
    if init is not None:
        out.copy_(init)
    return out, buf


def untouched(*bufs_and_outs):
    """The trailing row of every (out, buf) still holds the sentinel."""
    for out, buf in bufs_and_outs:
        tail = buf[out.numel():]
        assert bool((tail == SENTINEL[buf.dtype]).all()), f"{int((tail != SENTINEL[buf.dtype]).sum())} elements behind the output were written"


def all_nan(*outs):
    return all(bool(torch.isnan(o).all()) for o in outs)


# ---- backward: every NCH, partly filled and dead chunks, the row partition ------------------------------------------------------------------------
BWD = [pytest.param(5, 8, id="NCH1-5x8-one-live-lane"), pytest.param(9, 520, id="NCH2-9x520-chunk1-one-live-lane"),
       pytest.param(9, 1032, id="NCH4-9x1032-chunk2-one-live-lane-chunk3-dead"), pytest.param(9, 2048, id="NCH4-9x2048-full"),
       pytest.param(9, 2056, id="NCH8-9x2056-three-dead-chunks"), pytest.param(6, 4096, id="NCH8-6x4096-full"),
       pytest.param(3, 128, id="NCH1-3x128-one-block-idle-wave"), pytest.param(4097, 128, id="NCH1-4097x128-rows_per_block5-empty-blocks"),
       pytest.param(8200, 128, id="NCH1-8200x128-rows_per_block9-empty-blocks"), pytest.param(4100, 1032, id="NCH4-4100x1032-rows_per_block5-empty-blocks")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ln", [pytest.param(False, id="rmsnorm_bwd"), pytest.param(True, id="layernorm_bwd")])
@pytest.mark.parametrize("rows,d", BWD)
def test_norm_bwd_k_arms_and_row_partition(ops, dtype, ln, rows, d):
    """dx, dw (db) per element, fresh and accumulating; every partial row written (the workspaces start as NaN), those of blocks without a row
    exactly zero, and from 4097 rows the summed fp32 partials under the fp32 bound - one row is below a 16-bit rounding of a column there."""
    I = on_dev(NI.norm_inputs(rows, d, dtype, ln))
    nblk, rpb, ranges = NI.block_ranges(rows)
    assert nblk == ops.norm_partials(rows)
    empty = [b for b, (r0, r1) in enumerate(ranges) if r0 >= r1]
    assert bool(empty) == (rows > 4096) and all(b >= empty[0] for b in empty)
    op = "layernorm_bwd" if ln else "rmsnorm_bwd"
    tag = f"{rows}x{d} nblk={nblk} rows_per_block={rpb}"
    for acc in (False, True):
        how = " accumulate" if acc else ""
        old = I["old"] if acc else None
        if ln:
            ref, mod = N.layernorm(I["x"], I["w"], I["b"], EPS, I["dy"], dx_old=old), N.layernorm(I["x"], I["w"], I["b"], EPS, I["dy"], dx_old=old, model=dtype)
        else:
            ref, mod = N.rmsnorm(I["x"], I["w"], EPS, I["dy"], dx_old=old), N.rmsnorm(I["x"], I["w"], EPS, I["dy"], dx_old=old, model=dtype)
        dx = guarded((rows, d), dtype, init=old)
        parts = {"dw": guarded((nblk, d), F32)}
        if ln:
            parts["db"] = guarded((nblk, d), F32)
            L().call("mh_layernorm_bwd", I["x"], I["w"], I["dy"], dx[0], parts["dw"][0], parts["db"][0], rows, d, EPS, ops.dt_of(dtype), int(acc), stream())
        else:
            L().call("mh_rmsnorm_bwd", I["x"], I["w"], I["dy"], dx[0], parts["dw"][0], rows, d, EPS, ops.dt_of(dtype), int(acc), stream())
        untouched(dx, *parts.values())
        hold(f"{op} dx{how} [{tag}]", dtype, dx[0], ref["dx"], ref["B_dx"], mod["dx"])
        for nm, (part, _) in parts.items():
            unwritten = torch.isnan(part).any(1).nonzero().flatten().tolist()
            assert not unwritten, f"{op} {nm}: partial rows {unwritten[:8]} of {nblk} were not written"
            prev = I[nm + "_old"] if acc else None
            out = guarded((d,), dtype, init=prev)
            ops.reduce_partials(part, nblk, d, out[0], acc)
            untouched(out)
            r, Bc, m = ref[nm], ref["B_" + nm], mod[nm]
            if acc:
                r, Bc, m = r + prev.double(), Bc + prev.double().abs(), m + prev.float()
            hold(f"{op} {nm}{how} [{tag}]", dtype, out[0], r, Bc, N.r16(m, dtype))
            if rows >= 4097 and not acc:
                hold(f"{op} {nm} partials summed, fp32 bound [{tag}]", dtype, part.double().sum(0), ref[nm], ref["B_" + nm], mod[nm], out_dtype=F32)
                assert float(part[empty[0]:].abs().max()) == 0.0, f"{op} {nm}: partial rows of blocks {empty[0]}..{nblk - 1} own no row and must be zero"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ln", [pytest.param(False, id="rmsnorm_bwd"), pytest.param(True, id="layernorm_bwd")])
@pytest.mark.parametrize("rows,d,code", [pytest.param(4, 4104, "MH_ERR_SHAPE", id="d4104-past-NCH8"), pytest.param(4, 12, "MH_ERR_ARG", id="d12-not-a-multiple-of-8"),
                                         pytest.param(0, 128, "MH_ERR_ARG", id="rows0"), pytest.param(4, 0, "MH_ERR_ARG", id="d0"),
                                         pytest.param(4, -8, "MH_ERR_ARG", id="d-negative")])
def test_norm_bwd_refusals_write_nothing(ops, dtype, ln, rows, d, code):
    R, D = max(rows, 4), max(d, 128)  # the buffers are real, so what is refused is the shape and nothing else
    I = on_dev(NI.norm_inputs(R, D, dtype, ln))
    dx, pw, pb = guarded((R, D), dtype), guarded((ops.norm_partials(R), D), F32), guarded((ops.norm_partials(R), D), F32)
    if ln:
        rc = L().launch("mh_layernorm_bwd", I["x"], I["w"], I["dy"], dx[0], pw[0], pb[0], rows, d, EPS, ops.dt_of(dtype), 0, stream())
    else:
        rc = L().launch("mh_rmsnorm_bwd", I["x"], I["w"], I["dy"], dx[0], pw[0], rows, d, EPS, ops.dt_of(dtype), 0, stream())
    torch.cuda.synchronize()
    assert rc == L().DEFINES[code], f"rows = {rows}, d = {d}: status {rc}, expected {code}"
    assert all_nan(dx[0], pw[0], pb[0]), "a refused call wrote to its outputs"
    untouched(dx, pw, pb)


# ---- forward ----------------------------------------------------------------------------------------------------------------------------------
RMS_FWD = [pytest.param(1, 8, id="row_k-1x8"), pytest.param(64, 264, id="row_k-64x264-rows64-boundary"), pytest.param(64, 8192, id="row_k-64x8192-d8192-boundary"),
           pytest.param(65, 4096, id="fwd_k-65x4096-rows65-boundary"), pytest.param(64, 8200, id="fwd_k-64x8200-d8200-boundary"), pytest.param(5, 520, id="row_k-5x520")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,d", RMS_FWD)
def test_rmsnorm_fwd_both_kernels_with_rstd(ops, dtype, rows, d):
    """y per element and the rstd output, which no caller requests: rsqrt(mean x^2 + eps) in fp64 to 4 fp32 ulps (one rounding of the sum, one of
    rsqrtf, each with room to spare).  The fp32 model's own distance from fp64 is printed beside the kernel's."""
    I = on_dev(NI.norm_inputs(rows, d, dtype, False))
    ref, mod = N.rmsnorm(I["x"], I["w"], EPS), N.rmsnorm(I["x"], I["w"], EPS, model=dtype)
    y, rstd = guarded((rows, d), dtype), guarded((rows,), F32)
    L().call("mh_rmsnorm_fwd", I["x"], I["w"], y[0], rstd[0], rows, d, EPS, ops.dt_of(dtype), stream())
    untouched(y, rstd)
    hold(f"rmsnorm_fwd y [{rows}x{d}]", dtype, y[0], ref["y"], ref["B_y"], mod["y"])
    r64 = torch.rsqrt((I["x"].double() ** 2).mean(1) + EPS)
    r32 = torch.rsqrt((I["x"].float() ** 2).mean(1) + EPS)
    assert bool(torch.isfinite(rstd[0]).all()), f"rstd rows {(~torch.isfinite(rstd[0])).nonzero().flatten().tolist()[:8]} were not written"
    um, uk = ((t.double() - r64).abs() / N.ulp(r64, F32) for t in (r32, rstd[0]))
    print(f"CW | rmsnorm_fwd rstd (fp32 ulps) [{rows}x{d}] | {str(dtype)[6:]} | {float(um.max()):.3f} | {float(uk.max()):.3f} | 4.000 | worst at ({int(uk.argmax())},)")
    assert float(uk.max()) <= 4.0, f"rstd row {int(uk.argmax())}: {float(uk.max()):.2f} fp32 ulps from fp64 (the fp32 model: {float(um.max()):.2f})"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,d", [pytest.param(5, 8, id="layernorm_fwd_k-5x8"), pytest.param(9, 520, id="layernorm_fwd_k-9x520"), pytest.param(9, 1032, id="layernorm_fwd_k-9x1032"),
                                    pytest.param(65, 4096, id="layernorm_fwd_k-65x4096"), pytest.param(4, 8200, id="layernorm_fwd_k-4x8200")])
def test_layernorm_fwd(ops, dtype, rows, d):
    I = on_dev(NI.norm_inputs(rows, d, dtype, True))
    ref, mod = N.layernorm(I["x"], I["w"], I["b"], EPS), N.layernorm(I["x"], I["w"], I["b"], EPS, model=dtype)
    y = guarded((rows, d), dtype)
    L().call("mh_layernorm_fwd", I["x"], I["w"], I["b"], y[0], rows, d, EPS, ops.dt_of(dtype), stream())
    untouched(y)
    hold(f"layernorm_fwd y [{rows}x{d}]", dtype, y[0], ref["y"], ref["B_y"], mod["y"])


def first_difference(a, b):
    i = int((a.reshape(-1) != b.reshape(-1)).nonzero()[0])
    return f"first at {N._unravel(i, a.shape)}: {a.reshape(-1)[i].item()!r} against {b.reshape(-1)[i].item()!r}, {int((a != b).sum())} in all"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,d", [pytest.param(5, 4096, id="q8-few-rows-5x4096-zero-row"), pytest.param(5, 520, id="q8-few-rows-5x520-zero-row"),
                                    pytest.param(3, 8, id="q8-few-rows-3x8-zero-row"), pytest.param(65, 4096, id="q8_k-NCH8-65x4096-zero-row"),
                                    pytest.param(65, 520, id="q8_k-generic-65x520-zero-row"), pytest.param(65, 8, id="q8_k-generic-65x8-zero-row")])
def test_rmsnorm_fwd_q8_bit_identical_with_a_zero_row(ops, dtype, rows, d):
    """y, q and scales are the bits of mh_rmsnorm_fwd followed by mh_quant_fp8_rows; the all-zero row 1 has scale exactly 1 and bytes 0.
    Up to 64 rows mh_rmsnorm_fwd runs rmsnorm_fwd_row_k, whose sum of squares is formed in another order than the fused kernel's: at 5 x 4096
    in bf16 rmsnorm_fwd_q8_k<NCH = 8> gave y[4, 1528] one bf16 ulp away, so the launcher runs the two-kernel sequence itself there and the fused
    arms are reached from 65 rows."""
    I = on_dev(NI.norm_inputs(rows, d, dtype, False, zero_row=True))
    assert float(I["x"][1].abs().max()) == 0.0
    y, q, sc = guarded((rows, d), dtype), guarded((rows, d), torch.uint8), guarded((rows,), F32)
    L().call("mh_rmsnorm_fwd_q8", I["x"], I["w"], y[0], q[0], sc[0], rows, d, EPS, ops.dt_of(dtype), stream())
    untouched(y, q, sc)
    ref, mod = N.rmsnorm(I["x"], I["w"], EPS), N.rmsnorm(I["x"], I["w"], EPS, model=dtype)
    hold(f"rmsnorm_fwd_q8 y [{rows}x{d}]", dtype, y[0], ref["y"], ref["B_y"], mod["y"])
    y0 = ops.rmsnorm_fwd(I["x"], I["w"], EPS)
    q0, s0 = ops.quant_fp8_rows(y0)
    assert float(sc[0][1]) == 1.0 and float(q[0][1].max()) == 0 and float(y[0][1].abs().max()) == 0.0
    assert torch.equal(y[0].view(torch.int16), y0.view(torch.int16)), "y: " + first_difference(y[0].view(torch.int16), y0.view(torch.int16))
    assert torch.equal(sc[0], s0), "scales: " + first_difference(sc[0], s0)
    assert torch.equal(q[0], q0), "q: " + first_difference(q[0], q0)


# ---- the fp32 stream's reader ---------------------------------------------------------------------------------------------------------------------
F32IN_D = [pytest.param(4096, id="NCH8-d4096"), pytest.param(1024, id="NCH2-d1024"), pytest.param(520, id="generic-d520"), pytest.param(8, id="generic-d8")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("want_x16", [pytest.param(True, id="x16"), pytest.param(False, id="no-x16")])
@pytest.mark.parametrize("ln", [pytest.param(False, id="f32in_k-rms"), pytest.param(True, id="f32in_k-ln")])
@pytest.mark.parametrize("d", F32IN_D)
def test_norm_fwd_f32in_arms(ops, dtype, ln, want_x16, d):
    rows = 6
    I = on_dev(NI.f32_inputs(rows, d, dtype, ln))
    ref, mod = N.norm_f32in(I["x32"], I["w"], I["b"], EPS, y_dtype=dtype), N.norm_f32in(I["x32"], I["w"], I["b"], EPS, y_dtype=dtype, model=dtype)
    y = guarded((rows, d), dtype)
    x16 = guarded((rows, d), dtype) if want_x16 else None
    L().call("mh_norm_fwd_f32in", I["x32"], I["w"], I["b"], y[0], x16[0] if want_x16 else None, rows, d, EPS, ops.dt_of(dtype), stream())
    untouched(*((y, x16) if want_x16 else (y,)))
    hold(f"norm_fwd_f32in {'ln' if ln else 'rms'} y [{rows}x{d}]", dtype, y[0], ref["y"], ref["B_y"], mod["y"])
    if want_x16:
        assert torch.equal(x16[0].view(torch.int16), ref["x16"].view(torch.int16)), "x16: " + first_difference(x16[0].view(torch.int16), ref["x16"].view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("want_x16", [pytest.param(True, id="x16"), pytest.param(False, id="no-x16")])
@pytest.mark.parametrize("d", [pytest.param(4096, id="f32in_k-Y32-generic-d4096"), pytest.param(1024, id="f32in_k-Y32-generic-d1024"), pytest.param(520, id="f32in_k-Y32-generic-d520")])
def test_layernorm_f32_to_f32(ops, dtype, want_x16, d):
    """The fp32 y is held to eps = 2^-24 per element: the shifted row's mean (30) and the variance around it are what an fp32 kernel can lose."""
    rows = 6
    I = on_dev(NI.f32_inputs(rows, d, dtype, True))
    ref, mod = N.norm_f32in(I["x32"], I["w"], I["b"], EPS, y_dtype=F32), N.norm_f32in(I["x32"], I["w"], I["b"], EPS, y_dtype=F32, model=dtype)
    y = guarded((rows, d), F32)
    x16 = guarded((rows, d), dtype) if want_x16 else None
    L().call("mh_layernorm_f32_to_f32", I["x32"], I["w"], I["b"], y[0], x16[0] if want_x16 else None, rows, d, EPS, ops.dt_of(dtype), stream())
    untouched(*((y, x16) if want_x16 else (y,)))
    hold(f"layernorm_f32_to_f32 y [{rows}x{d}]", dtype, y[0], ref["y"], ref["B_y"], mod["y"], out_dtype=F32)
    if want_x16:
        assert torch.equal(x16[0].view(torch.int16), ref["x16"].view(torch.int16)), "x16: " + first_difference(x16[0].view(torch.int16), ref["x16"].view(torch.int16))


# ---- column sums ------------------------------------------------------------------------------------------------------------------------------
COLSUM = [pytest.param(3, 8, 8, 0, id="v8_k-3x8-one-block"), pytest.param(4097, 264, 272, 0, id="v8_k-4097x264-ld272-rows_per_block5-empty-blocks"),
          pytest.param(4097, 260, 260, 0, id="scalar_k-4097x260-d-not-multiple-of-8"), pytest.param(32768, 8, 8, 0, id="v8_k-32768x8-main-loop-all-thread-rows"),
          pytest.param(32800, 16, 24, 0, id="v8_k-32800x16-ld24-rows_per_block33-main-loop-and-tail"),
          pytest.param(4097, 264, 272, 1, id="scalar_k-4097x264-ld272-base-off-by-one-element")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,d,ld,offset", COLSUM)
def test_colsum_partial_arms(ops, dtype, rows, d, ld, offset):
    buf, old = NI.colsum_inputs(rows, d, ld, dtype, offset=offset)
    buf, old = buf.to(dev()), old.to(dev())
    x = NI.colsum_view(buf, rows, d, ld, offset)
    assert x.stride(0) == ld and (x.data_ptr() % 16 == 0) == (offset == 0)
    nblk, rpb, ranges = NI.block_ranges(rows)
    tag = f"{rows}x{d} ld={ld}{' base+1' if offset else ''} rows_per_block={rpb}"
    part = guarded((nblk, d), F32)
    L().call("mh_colsum_partial", x, ld, part[0], rows, d, ops.dt_of(dtype), stream())
    untouched(part)
    unwritten = torch.isnan(part[0]).any(1).nonzero().flatten().tolist()
    assert not unwritten, f"colsum: partial rows {unwritten[:8]} of {nblk} were not written"
    empty = [b for b, (r0, r1) in enumerate(ranges) if r0 >= r1]
    if empty:
        assert float(part[0][empty[0]:].abs().max()) == 0.0, f"colsum: partial rows of blocks {empty[0]}..{nblk - 1} own no row and must be zero"
    for prev in (None, old):
        how = " accumulate" if prev is not None else ""
        ref, Bc = N.colsum(x, prev)
        out = guarded((d,), dtype, init=prev)
        ops.reduce_partials(part[0], nblk, d, out[0], prev is not None)
        untouched(out)
        hold(f"colsum{how} [{tag}]", dtype, out[0], ref, Bc, N.colsum(x, prev, model=dtype))
    if rows >= 4097:
        ref, Bc = N.colsum(x)
        hold(f"colsum partials summed, fp32 bound [{tag}]", dtype, part[0].double().sum(0), ref, Bc, N.colsum(x, model=F32), out_dtype=F32)
