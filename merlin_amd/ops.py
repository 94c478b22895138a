"""Tensor-level wrappers over the C ABI (include/merlin_hip.h).

PyTorch is used for device memory and streams only: every function checks layouts, allocates
outputs with torch, and enqueues ONE library call on torch's current HIP stream.  No torch
arithmetic happens here, and there is no fallback: without libmerlin_hip.so these raise.
"""
from __future__ import annotations

import os

import torch

from . import _lib as L
from ._lib import C, f32, i32, i64, p, u64  # noqa: F401  (the wrappers: not used here any more, tools/ and tests/ reach them as ops.p, ops.i32, ...)

EPI_BIAS, EPI_QUICK_GELU, EPI_RESIDUAL, EPI_ACCUM, EPI_OUT_F32 = L.EPI_BIAS, L.EPI_QUICK_GELU, L.EPI_RESIDUAL, L.EPI_ACCUM, L.EPI_OUT_F32


def dt_of(t_or_dtype) -> int:
    d = t_or_dtype.dtype if isinstance(t_or_dtype, torch.Tensor) else t_or_dtype
    if d == torch.bfloat16:
        return L.MH_BF16
    if d == torch.float16:
        return L.MH_F16
    if d == torch.float32:
        return L.MH_F32
    raise TypeError(f"unsupported dtype {d}")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- optional per-launch timing (HIP events on the launch stream); used by bench.py's roofline leg ----
_PROF = None


def profile_start():
    global _PROF
    _PROF = []


LAST_PROFILE_BYTES = {}  # {kernel: algorithmic bytes (every operand and the result moved once)} of the last profile_stop()


def profile_stop():
    """-> {kernel: (launches, total_work, total_ms)}; work = FLOPs (gemm/attn) or bytes."""
    global _PROF, LAST_PROFILE_BYTES
    rec, _PROF = _PROF, None
    torch.cuda.synchronize()
    out, nb = {}, {}
    for name, work, s, e, b in rec or []:
        n, w, ms = out.get(name, (0, 0.0, 0.0))
        out[name] = (n + 1, w + work, ms + s.elapsed_time(e))
        nb[name] = nb.get(name, 0.0) + b
    LAST_PROFILE_BYTES = nb
    return out


class _timed:
    __slots__ = ("name", "work", "s", "nbytes")

    def __init__(self, name, work, nbytes=0.0):
        self.name, self.work, self.nbytes = name, work, nbytes

    def __enter__(self):
        if _PROF is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.s.record()

    def __exit__(self, *a):
        if _PROF is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            _PROF.append((self.name, self.work, self.s, e, self.nbytes))


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def _rowmajor(t: torch.Tensor):
    assert t.dim() == 2 and t.stride(1) == 1, f"need row-major 2-D, got {tuple(t.shape)} strides {t.stride()}"
    return t.stride(0)


def arch_ok(dev: int = 0) -> bool:
    return bool(L.lib().mh_arch_ok(dev))


# ---------------------------------------------------------------------------------------------
SKINNY_SPLITK = os.environ.get("MH_SKINNY_SPLITK", "1") != "0"  # A/B switch
SKINNY_SPLITK_ALL = os.environ.get("MH_SKINNY_SPLITK", "1") == "2"  # fp16 too (default: bf16 only, see _skinny_splitk_ok)
SKINNY_MAX_ROWS = 4096


def _epilogue(bias, act, resid, accum, out):
    """-> (MH_EPI_* flag word of a GEMM launch, row stride of resid)."""
    epi = 0
    if bias is not None:
        epi |= EPI_BIAS
    if act == "quick_gelu":
        epi |= EPI_QUICK_GELU
    ldr = 0
    if resid is not None:
        epi |= EPI_RESIDUAL
        ldr = _rowmajor(resid)
    if accum:
        epi |= EPI_ACCUM
    if out.dtype == torch.float32:
        epi |= EPI_OUT_F32
    return epi, ldr


def gemm_nt(a, b, *, out=None, bias=None, resid=None, act=None, accum=False, out_f32=False, n=None, a_t=False, b_t=False):
    """out[M,N] = A @ B^T (+bias)(quick_gelu)(+resid)(+out), 16-bit row-major operands.
    A = a[M,K] (or a[K,M] when a_t: K-strided), B = b[N,K] (or b[K,N] when b_t)."""
    if a_t:
        K, M = a.shape
    else:
        M, K = a.shape
    if b_t:
        assert b.shape[0] == K
        N = b.shape[1] if n is None else n
    else:
        assert b.shape[1] == K
        N = b.shape[0] if n is None else n
    assert a.dtype == b.dtype
    lda, ldb = _rowmajor(a), _rowmajor(b)
    if out is None:
        assert not accum
        out = torch.empty(M, N, dtype=torch.float32 if out_f32 else a.dtype, device=a.device)
    ldc = _rowmajor(out)
    if act not in (None, "quick_gelu"):
        raise ValueError(act)
    epi, ldr = _epilogue(bias, act, resid, accum, out)
    assert out.dtype in (torch.float32, a.dtype)
    # short sequences (a single 613-token example, a prompt's prefill): few output tiles and a long contraction -> split K over
    # several blocks per tile, the epilogue applied by the reduce pass (profiles/r03_skinny_gemm.txt)
    splits = 1
    if _skinny_splitk_ok(a.dtype) and M <= SKINNY_MAX_ROWS and N % 4 == 0 and ldc % 4 == 0:
        splits = int(L.lib().mh_gemm_splitk_max(M, N, K))
    with _timed("gemm_nt", 2.0 * M * N * K, 2.0 * (M * K + N * K) + float(out.element_size()) * M * N):
        if splits > 1:
            ws = _splitk_workspace(a.device, splits * M * N)
            L.call("mh_gemm_splitk_epi", a, lda, int(a_t), b, ldb, int(b_t), out, ldc, bias, resid, ldr, M, N, K, dt_of(a), epi, splits, ws, _stream())
        else:
            L.call("mh_gemm", a, lda, int(a_t), b, ldb, int(b_t), out, ldc, bias, resid, ldr, M, N, K, dt_of(a), epi, _stream())
    return out


def gemv(x, w, out=None, resid=None, out_f32=False, n=None):
    """out[M, N] = x[M, K] @ w[N, K]^T (+ resid), <= 16 rows per launch (decode step): weights streamed once per launch."""
    M, K = x.shape
    N = w.shape[0] if n is None else n
    assert w.shape[1] == K and x.dtype == w.dtype
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32 if out_f32 else x.dtype, device=x.device)
    step = _gemv_rows_per_launch(K)
    for m0 in range(0, M, step):
        mm = min(step, M - m0)
        xs, os_ = x[m0:m0 + mm], out[m0:m0 + mm]
        rs = resid[m0:m0 + mm] if resid is not None else None
        L.call("mh_gemv", xs, _rowmajor(xs), w, _rowmajor(w), os_, _rowmajor(os_), rs, _rowmajor(rs) if rs is not None else 0, mm, N, K, dt_of(x),
               int(out.dtype == torch.float32), _stream())
    return out


def gemv_swiglu(x, wgu, out=None):
    """act[M, ff] = silu(x @ Wg^T) * (x @ Wu^T), wgu = [Wg; Wu] [2 ff, K]: the decode step's gate|up projection + SwiGLU in one launch
    (gate / up rounded to 16 bits first, as gemv + swiglu_fwd).  More than 8 rows: the two launches."""
    M, K = x.shape
    ff = wgu.shape[0] // 2
    assert wgu.shape[1] == K and x.dtype == wgu.dtype
    if not _gemv_fused_rows_ok(M, K):
        return swiglu_fwd(gemv(x, wgu), out=out)
    out = torch.empty(M, ff, dtype=x.dtype, device=x.device) if out is None else out
    L.call("mh_gemv_swiglu", x, _rowmajor(x), wgu, _rowmajor(wgu), out, _rowmajor(out), M, ff, K, dt_of(x), _stream())
    return out


FUSED_NORM_MAX_ROWS = 2


def gemv_norm(x, norm_w, eps, w, swiglu=False, out=None):
    """rmsnorm(x; norm_w, eps) @ w^T with the norm done inside the projection's launch (decode step); swiglu=True: w = [Wg; Wu] and the
    result is silu(gate) * up [M, ff].  The fused form pays for 1-2 rows (every block re-normalises the rows: measured slower than the
    separate norm from 4 rows on); otherwise, or with K > 8192: the separate launches."""
    M, K = x.shape
    if M > FUSED_NORM_MAX_ROWS or K > 8192:
        h = rmsnorm_fwd(x, norm_w, eps)
        return gemv_swiglu(h, w, out=out) if swiglu else gemv(h, w, out=out)  # (gemv_swiglu: fused up to 16 rows)
    N = w.shape[0]
    ff = N // 2 if swiglu else 0
    assert w.shape[1] == K and x.dtype == w.dtype == norm_w.dtype and x.is_contiguous()
    out = torch.empty(M, ff if swiglu else N, dtype=x.dtype, device=x.device) if out is None else out
    L.call("mh_gemv_norm", x, _rowmajor(x), norm_w, eps, w, _rowmajor(w), out, _rowmajor(out), M, N, K, ff, dt_of(x), _stream())
    return out


def quant_fp8_b128(w):
    """w [N, K] (16-bit) -> (q uint8 [N, K] OCP e4m3, scales fp32 [N, ceil(K/128)])."""
    N, K = w.shape
    q = torch.empty(N, K, dtype=torch.uint8, device=w.device)
    sc = torch.empty(N, (K + 127) // 128, dtype=torch.float32, device=w.device)
    L.call("mh_quant_fp8_b128", w, _rowmajor(w), q, sc, N, K, dt_of(w), _stream())
    return q, sc


def gemv_fp8w(x, qw, out=None, resid=None, out_f32=False, n=None):
    """out[M, N] = x[M, K] @ dequant(q, scales)^T (+ resid); qw = (q, scales) from quant_fp8_b128."""
    q, sc = qw
    M, K = x.shape
    N = q.shape[0] if n is None else n
    assert q.shape[1] == K
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32 if out_f32 else x.dtype, device=x.device)
    step = _gemv_rows_per_launch(K)
    for m0 in range(0, M, step):
        mm = min(step, M - m0)
        xs, os_ = x[m0:m0 + mm], out[m0:m0 + mm]
        rs = resid[m0:m0 + mm] if resid is not None else None
        L.call("mh_gemv_fp8w", xs, _rowmajor(xs), q, sc, os_, _rowmajor(os_), rs, _rowmajor(rs) if rs is not None else 0, mm, N, K, dt_of(x),
               int(out.dtype == torch.float32), _stream())
    return out


def gemv_fp8w_norm(x, norm_w, eps, qw, swiglu=False, out=None):
    """gemv_norm with fp8 weights (qw = (q, scales) from quant_fp8_b128).  1-2 rows: norm, projection (and SwiGLU) in one launch;
    3-16 rows: separate norm, SwiGLU still fused; more rows: separate launches."""
    q, sc = qw
    M, K = x.shape
    N = q.shape[0]
    ff = N // 2 if swiglu else 0
    if not _gemv_fused_rows_ok(M, K) or K > 8192:
        y = gemv_fp8w(rmsnorm_fwd(x, norm_w, eps), qw)
        return swiglu_fwd(y, out=out) if swiglu else y
    fuse_norm = M <= FUSED_NORM_MAX_ROWS
    if not fuse_norm:
        x = rmsnorm_fwd(x, norm_w, eps)
        if not swiglu:
            return gemv_fp8w(x, qw, out=out)
    assert q.shape[1] == K and x.is_contiguous()
    out = torch.empty(M, ff if swiglu else N, dtype=x.dtype, device=x.device) if out is None else out
    L.call("mh_gemv_fp8w_norm", x, _rowmajor(x), norm_w if fuse_norm else None, eps, q, sc, out, _rowmajor(out), M, N, K, ff, dt_of(x), _stream())
    return out


def is_fp4_pair(w):
    """True for the (q, scales) pair of quant_fp4_b32 (E8M0 scale bytes); the pair of quant_fp8_b128 carries fp32 scales."""
    return isinstance(w, (tuple, list)) and w[1].dtype == torch.uint8


def quant_fp4_b32(w):
    """w [N, K] (16-bit, K % 32 == 0) -> (q uint8 [N, K/2]: OCP MX e2m1 codes, element 2j in the low nibble of byte j; scales uint8
    [N, K/32]: E8M0 exponents e + 127, one per 32 consecutive k)."""
    N, K = w.shape
    if K % 32:
        raise ValueError(f"quant_fp4_b32: K = {K} is not a multiple of the 32-element scale block")
    q = torch.empty(N, K // 2, dtype=torch.uint8, device=w.device)
    sc = torch.empty(N, K // 32, dtype=torch.uint8, device=w.device)
    L.call("mh_quant_fp4_b32", w, _rowmajor(w), q, sc, N, K, dt_of(w), _stream())
    return q, sc


def _gemv_fp4_rows_per_launch(K):
    """Activation rows one mh_gemv_fp4w launch takes: 16 through the MFMA form (K % 64 == 0), 8 through the wave-per-row form."""
    return 16 if (K % 64 == 0 and _gemv_mfma_min <= 9) else 8


def gemv_fp4w(x, qw, out=None, resid=None, out_f32=False, n=None):
    """out[M, N] = x[M, K] @ dequant(q, scales)^T (+ resid); qw = (q, scales) from quant_fp4_b32."""
    q, sc = qw
    M, K = x.shape
    N = q.shape[0] if n is None else n
    assert q.shape[1] * 2 == K and sc.dtype == torch.uint8
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32 if out_f32 else x.dtype, device=x.device)
    step = _gemv_fp4_rows_per_launch(K)
    for m0 in range(0, M, step):
        mm = min(step, M - m0)
        xs, os_ = x[m0:m0 + mm], out[m0:m0 + mm]
        rs = resid[m0:m0 + mm] if resid is not None else None
        L.call("mh_gemv_fp4w", xs, _rowmajor(xs), q, sc, os_, _rowmajor(os_), rs, _rowmajor(rs) if rs is not None else 0, mm, N, K, dt_of(x),
               int(out.dtype == torch.float32), _stream())
    return out


def gemm_fp4w(x, qw, out=None, resid=None, out_f32=False, accum=False, n=None):
    """out[M, N] = x[M, K] @ dequant(q, scales)^T for any number of rows in ONE launch (prefill, full-sequence forward); qw = (q, scales)
    from quant_fp4_b32, read as stored.  Store forms: 16-bit (+ 16-bit resid), fp32 (out_f32, or an fp32 `out`), fp32 read-modify-write
    (accum: out += product, out given and fp32).  Anything the launcher would refuse is a ValueError and nothing is launched."""
    q, sc = qw
    if x.dim() != 2 or q.dim() != 2 or sc.dim() != 2 or q.dtype != torch.uint8 or sc.dtype != torch.uint8:
        raise ValueError("gemm_fp4w takes x [M, K] and the (q, scales) uint8 pair of quant_fp4_b32")
    M, K = x.shape
    N = q.shape[0] if n is None else n
    if K % 32 or q.shape[1] * 2 != K or sc.shape[1] * 32 != K:
        raise ValueError(f"gemm_fp4w: K = {K} must be a multiple of the 32-element scale block and match the weight's {q.shape[1] * 2}")
    if M < 1 or not 1 <= N <= q.shape[0] or x.dtype not in (torch.bfloat16, torch.float16) or not (q.is_contiguous() and sc.is_contiguous()):
        raise ValueError(f"gemm_fp4w: M = {M}, N = {N} of {q.shape[0]} weight rows, x {x.dtype}")
    out_f32 = bool(out_f32) or (out is not None and out.dtype == torch.float32)
    if accum and not out_f32:
        raise ValueError("gemm_fp4w: accum is the fp32 read-modify-write (out_f32); a 16-bit sum takes resid")
    if accum and out is None:
        raise ValueError("gemm_fp4w: accum adds to `out`, which must be given")
    if resid is not None and (accum or out_f32):
        raise ValueError("gemm_fp4w: resid goes with the 16-bit store only (not with accum or out_f32)")
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32 if out_f32 else x.dtype, device=x.device)
    if out.dtype != (torch.float32 if out_f32 else x.dtype) or out.shape[0] < M or out.shape[1] < N:
        raise ValueError(f"gemm_fp4w: out {tuple(out.shape)} {out.dtype} does not hold [{M}, {N}] {'fp32' if out_f32 else x.dtype}")
    if resid is not None and (resid.dtype != x.dtype or resid.shape[0] < M or resid.shape[1] < N):
        raise ValueError(f"gemm_fp4w: resid {tuple(resid.shape)} {resid.dtype} does not hold [{M}, {N}] {x.dtype}")
    if _rowmajor(x) % 8 or x.data_ptr() % 16:
        raise ValueError("gemm_fp4w: x rows must be 16-byte aligned")
    with _timed("gemm_fp4w", 2.0 * M * N * K, 2.0 * M * K + 0.53125 * N * K + float(out.element_size()) * M * N):
        L.call("mh_gemm_fp4w", x, _rowmajor(x), q, sc, out, _rowmajor(out), resid, _rowmajor(resid) if resid is not None else 0, M, N, K,
               dt_of(x), int(out_f32), int(bool(accum)), _stream())
    return out


def gemv_fp4w_norm(x, norm_w, eps, qw, swiglu=False, out=None):
    """gemv_norm with MXFP4 weights (qw = (q, scales) from quant_fp4_b32).  1-2 rows: norm, projection (and SwiGLU) in one launch;
    3-16 rows: separate norm, SwiGLU still fused; more rows: separate launches."""
    q, sc = qw
    M, K = x.shape
    N = q.shape[0]
    ff = N // 2 if swiglu else 0
    if not _gemv_fused_rows_ok(M, K) or K > 8192:
        y = gemv_fp4w(rmsnorm_fwd(x, norm_w, eps), qw)
        return swiglu_fwd(y, out=out) if swiglu else y
    fuse_norm = M <= FUSED_NORM_MAX_ROWS
    if not fuse_norm:
        x = rmsnorm_fwd(x, norm_w, eps)
        if not swiglu:
            return gemv_fp4w(x, qw, out=out)
    assert q.shape[1] * 2 == K and x.is_contiguous()
    out = torch.empty(M, ff if swiglu else N, dtype=x.dtype, device=x.device) if out is None else out
    L.call("mh_gemv_fp4w_norm", x, _rowmajor(x), norm_w if fuse_norm else None, eps, q, sc, out, _rowmajor(out), M, N, K, ff, dt_of(x), _stream())
    return out


def gemv_qkv_rope(x, norm_w, eps, w, table, pos, kcache, vcache, H, D, rope_pos=None):
    """Decode-step q|k|v: (input_layernorm +) projection + RoPE at pos + K/V append in one launch; w = 16-bit weight [3HD, K], the
    (q, scales) pair of quant_fp8_b128 or that of quant_fp4_b32 (one launch up to 8 rows).  Returns qkv [M, 3HD] (q, k rotated).
    More than 16 rows: the separate launches."""
    M, K = x.shape
    fp8 = isinstance(w, (tuple, list))
    if is_fp4_pair(w):
        if M > 8 or K > 8192:
            qkv = gemv_fp4w(rmsnorm_fwd(x, norm_w, eps), w)
            decode_rope_append(qkv, table, pos, kcache, vcache, H, D, rope_pos=rope_pos)
            return qkv
        if M > FUSED_NORM_MAX_ROWS:
            x, norm_w = rmsnorm_fwd(x, norm_w, eps), None
        assert x.is_contiguous() and pos.dtype == torch.int32 and kcache.is_contiguous() and vcache.is_contiguous()
        qkv = torch.empty(M, 3 * H * D, dtype=x.dtype, device=x.device)
        L.call("mh_gemv_fp4w_qkv_rope", x, _rowmajor(x), norm_w, eps, w[0], w[1], qkv, _rowmajor(qkv), M, K, dt_of(x), table, pos, rope_pos,
               kcache, vcache, H, D, kcache.shape[1], _stream())
        return qkv
    if not _gemv_fused_rows_ok(M, K) or K > 8192 or (M > 8 and (D // 2) % 16):
        h = rmsnorm_fwd(x, norm_w, eps)
        qkv = gemv_fp8w(h, w) if fp8 else gemv(h, w)
        decode_rope_append(qkv, table, pos, kcache, vcache, H, D, rope_pos=rope_pos)
        return qkv
    if M > FUSED_NORM_MAX_ROWS:
        x, norm_w = rmsnorm_fwd(x, norm_w, eps), None
    assert x.is_contiguous() and pos.dtype == torch.int32 and kcache.is_contiguous() and vcache.is_contiguous()
    qkv = torch.empty(M, 3 * H * D, dtype=x.dtype, device=x.device)
    wq, sc = (w if fp8 else (None, None))
    L.call("mh_gemv_qkv_rope", x, _rowmajor(x), norm_w, eps, None if fp8 else w, 0 if fp8 else _rowmajor(w), wq, sc, qkv, _rowmajor(qkv), M, K, dt_of(x), table,
           pos, rope_pos, kcache, vcache, H, D, kcache.shape[1], _stream())
    return qkv


def decode_rope_append(qkv, table, pos, kcache, vcache, H, D, rope_pos=None):
    """qkv [B, 3*H*D] of the new tokens (rotated in place at rope_pos[b], default pos[b]); k, v appended to kcache/vcache [B, Smax, H*D]
    at row pos[b]."""
    B = qkv.shape[0]
    assert qkv.is_contiguous() and pos.dtype == torch.int32 and kcache.is_contiguous() and vcache.is_contiguous()
    assert rope_pos is None or rope_pos.dtype == torch.int32
    L.call("mh_decode_rope_append", qkv, table, pos, rope_pos, kcache, vcache, B, H, D, kcache.shape[1], dt_of(qkv), _stream())


def attn_decode(q, kcache, vcache, lens, H, D, out=None, split_kv=True):
    """q [B, H*D] view (row stride ldq) against the cache [B, Smax, H*D]; keys [0, lens[b])."""
    B = q.shape[0]
    out = torch.empty(B, H * D, dtype=q.dtype, device=q.device) if out is None else out
    Smax = kcache.shape[1]
    splits = int(L.lib().mh_attn_decode_splits(B, H, Smax))
    ws = torch.empty(B * H * splits * (D + 2), dtype=torch.float32, device=q.device) if (splits > 1 and split_kv) else None
    L.call("mh_attn_decode", q, q.stride(0), kcache, vcache, out, lens, B, H, D, Smax, ws, dt_of(q), _stream())
    return out


def kv8_fill(x, c8, scales, B, S, H, D, row0=0):
    """Prefill of the fp8 KV cache: x [B*S, H*D] (a view with row stride x.stride(0), e.g. the k section of the fused q|k|v buffer) ->
    e4m3 rows [b, s < S] of c8 (uint8 [B, Smax, H*D]) and their power-of-two scales [b, h, s] (fp32 [B, H, Smax]).
    row0: the rows go to [b, row0 + s] instead (extending a kept cache: the same launch on views of c8 and scales offset by row0 rows,
    with the cache's own Smax as the stride)."""
    assert x.stride(1) == 1 and x.shape == (B * S, H * D) and c8.dtype == torch.uint8 and c8.is_contiguous() and scales.is_contiguous()
    assert scales.shape == (c8.shape[0], H, c8.shape[1]) and scales.dtype == torch.float32
    assert 0 <= row0 and row0 + S <= c8.shape[1]
    if row0:
        L.call("mh_kv8_fill", x, x.stride(0), c8[:, row0:], scales[:, :, row0:], B, S, H, D, c8.shape[1], dt_of(x), _stream())
        return
    L.call("mh_kv8_fill", x, x.stride(0), c8, scales, B, S, H, D, c8.shape[1], dt_of(x), _stream())


def decode_rope_append_kv8(qkv, table, pos, k8, v8, kscale, vscale, H, D, rope_pos=None):
    """decode_rope_append on the fp8 KV cache: qkv rotated in place (bit-identical), the rotated k row and the v row quantised into
    k8 / v8 (uint8 [B, Smax, H*D]) at row pos[b], their scales into kscale / vscale (fp32 [B, H, Smax])."""
    B = qkv.shape[0]
    assert qkv.is_contiguous() and pos.dtype == torch.int32 and k8.is_contiguous() and v8.is_contiguous() and k8.dtype == v8.dtype == torch.uint8
    assert kscale.is_contiguous() and vscale.is_contiguous() and kscale.shape == vscale.shape == (B, H, k8.shape[1])
    assert rope_pos is None or rope_pos.dtype == torch.int32
    L.call("mh_decode_rope_append_kv8", qkv, table, pos, rope_pos, k8, v8, kscale, vscale, B, H, D, k8.shape[1], dt_of(qkv), _stream())


def attn_decode_kv8(q, k8, v8, kscale, vscale, lens, H, D, out=None, split_kv=True):
    """attn_decode against the fp8 KV cache (k8, v8 uint8 [B, Smax, H*D]; kscale, vscale fp32 [B, H, Smax]); keys [0, lens[b])."""
    B = q.shape[0]
    out = torch.empty(B, H * D, dtype=q.dtype, device=q.device) if out is None else out
    Smax = k8.shape[1]
    assert k8.dtype == v8.dtype == torch.uint8 and k8.shape == v8.shape == (B, Smax, H * D) and k8.is_contiguous() and v8.is_contiguous()
    assert kscale.dtype == vscale.dtype == torch.float32 and kscale.shape == vscale.shape == (B, H, Smax)
    assert kscale.is_contiguous() and vscale.is_contiguous() and lens.dtype == torch.int32 and q.stride(1) == 1
    splits = int(L.lib().mh_attn_decode_splits(B, H, Smax))
    ws = torch.empty(B * H * splits * (D + 2), dtype=torch.float32, device=q.device) if (splits > 1 and split_kv) else None
    L.call("mh_attn_decode_kv8", q, q.stride(0), k8, v8, kscale, vscale, out, lens, B, H, D, Smax, ws, dt_of(q), _stream())
    return out


def decode_rope_append_multi(qkv, table, pos, kcache, vcache, T, H, D, rope_pos=None):
    """decode_rope_append for T new tokens per sequence: qkv [B*T, 3*H*D], row b*T + t rotated in place at rope_pos[b] + t (default pos[b] + t)
    and appended at cache row pos[b] + t; bit-identical to T single-token calls.  Rows that would land at or beyond Smax are left untouched."""
    B = pos.shape[0]
    assert qkv.shape == (B * T, 3 * H * D) and qkv.is_contiguous() and pos.dtype == torch.int32 and kcache.is_contiguous() and vcache.is_contiguous()
    assert rope_pos is None or rope_pos.dtype == torch.int32
    L.call("mh_decode_rope_append_multi", qkv, table, pos, rope_pos, kcache, vcache, B, T, H, D, kcache.shape[1], dt_of(qkv), _stream())


def decode_rope_append_multi_kv8(qkv, table, pos, k8, v8, kscale, vscale, T, H, D, rope_pos=None):
    """decode_rope_append_multi on the fp8 KV cache (k8, v8 uint8 [B, Smax, H*D]; kscale, vscale fp32 [B, H, Smax])."""
    B = pos.shape[0]
    assert qkv.shape == (B * T, 3 * H * D) and qkv.is_contiguous() and pos.dtype == torch.int32
    assert k8.is_contiguous() and v8.is_contiguous() and k8.dtype == v8.dtype == torch.uint8
    assert kscale.is_contiguous() and vscale.is_contiguous() and kscale.shape == vscale.shape == (B, H, k8.shape[1])
    assert rope_pos is None or rope_pos.dtype == torch.int32
    L.call("mh_decode_rope_append_multi_kv8", qkv, table, pos, rope_pos, k8, v8, kscale, vscale, B, T, H, D, k8.shape[1], dt_of(qkv), _stream())


def attn_decode_multi_splits(B, T, H, Smax):
    """Key splits of attn_decode_multi / attn_decode_multi_kv8 with split_kv=True (mh_attn_decode_multi_splits)."""
    return int(L.lib().mh_attn_decode_multi_splits(B, T, H, Smax))


def attn_decode_multi(q, kcache, vcache, lens, T, H, D, out=None, split_kv=True):
    """T queries per sequence: q [B*T, H*D] view (row stride ldq, row b*T + t) against the cache [B, Smax, H*D]; query (b, t) sees keys
    [0, lens[b] + t).  split_kv=False: one block per (b, h) (refused where T x Smax scores do not fit the kernel's LDS)."""
    B = lens.shape[0]
    assert q.shape == (B * T, H * D) and q.stride(1) == 1 and lens.dtype == torch.int32 and kcache.is_contiguous() and vcache.is_contiguous()
    out = torch.empty(B * T, H * D, dtype=q.dtype, device=q.device) if out is None else out
    Smax = kcache.shape[1]
    splits = attn_decode_multi_splits(B, T, H, Smax)
    ws = torch.empty(B * T * H * splits * (D + 2), dtype=torch.float32, device=q.device) if (splits > 1 and split_kv) else None
    L.call("mh_attn_decode_multi", q, q.stride(0), kcache, vcache, out, lens, B, T, H, D, Smax, ws, dt_of(q), _stream())
    return out


def attn_decode_multi_kv8(q, k8, v8, kscale, vscale, lens, T, H, D, out=None, split_kv=True):
    """attn_decode_multi against the fp8 KV cache (k8, v8 uint8 [B, Smax, H*D]; kscale, vscale fp32 [B, H, Smax])."""
    B = lens.shape[0]
    out = torch.empty(B * T, H * D, dtype=q.dtype, device=q.device) if out is None else out
    Smax = k8.shape[1]
    assert q.shape == (B * T, H * D) and q.stride(1) == 1 and lens.dtype == torch.int32
    assert k8.dtype == v8.dtype == torch.uint8 and k8.shape == v8.shape == (B, Smax, H * D) and k8.is_contiguous() and v8.is_contiguous()
    assert kscale.dtype == vscale.dtype == torch.float32 and kscale.shape == vscale.shape == (B, H, Smax)
    assert kscale.is_contiguous() and vscale.is_contiguous()
    splits = attn_decode_multi_splits(B, T, H, Smax)
    ws = torch.empty(B * T * H * splits * (D + 2), dtype=torch.float32, device=q.device) if (splits > 1 and split_kv) else None
    L.call("mh_attn_decode_multi_kv8", q, q.stride(0), k8, v8, kscale, vscale, out, lens, B, T, H, D, Smax, ws, dt_of(q), _stream())
    return out


def attn_extend(q, kcache, vcache, lens, n, H, D, out=None):
    """n new queries per sequence, any n >= 1: q [B*n, H*D] view (row stride ldq, row b*n + t) against the cache [B, Smax, H*D] that
    already holds their keys; query (b, t) sees keys [0, lens[b] + t).  Flash-style (mh_attn_extend): no workspace, no limit on Smax."""
    B = lens.shape[0]
    assert q.shape == (B * n, H * D) and q.stride(1) == 1 and lens.dtype == torch.int32 and kcache.is_contiguous() and vcache.is_contiguous()
    assert kcache.shape == vcache.shape and kcache.shape[0] == B and kcache.shape[2] == H * D
    out = torch.empty(B * n, H * D, dtype=q.dtype, device=q.device) if out is None else out
    assert out.shape == (B * n, H * D) and out.is_contiguous()
    L.call("mh_attn_extend", q, q.stride(0), kcache, vcache, out, lens, B, n, H, D, kcache.shape[1], dt_of(q), _stream())
    return out


def attn_extend_kv8(q, k8, v8, kscale, vscale, lens, n, H, D, out=None):
    """attn_extend against the fp8 KV cache (k8, v8 uint8 [B, Smax, H*D]; kscale, vscale fp32 [B, H, Smax])."""
    B = lens.shape[0]
    Smax = k8.shape[1]
    assert q.shape == (B * n, H * D) and q.stride(1) == 1 and lens.dtype == torch.int32
    assert k8.dtype == v8.dtype == torch.uint8 and k8.shape == v8.shape == (B, Smax, H * D) and k8.is_contiguous() and v8.is_contiguous()
    assert kscale.dtype == vscale.dtype == torch.float32 and kscale.shape == vscale.shape == (B, H, Smax)
    assert kscale.is_contiguous() and vscale.is_contiguous()
    out = torch.empty(B * n, H * D, dtype=q.dtype, device=q.device) if out is None else out
    assert out.shape == (B * n, H * D) and out.is_contiguous()
    L.call("mh_attn_extend_kv8", q, q.stride(0), k8, v8, kscale, vscale, out, lens, B, n, H, D, Smax, dt_of(q), _stream())
    return out


def attn_extend_branches(q, kcache, vcache, seg_start, P, H, D, out=None):
    """The packed rows of several continuations of one prompt: q [R, H*D] view (row stride ldq) against the one-sequence cache
    [1, Smax, H*D] whose rows [0, P) hold the prompt and rows [P, P + R) the rows' own keys; seg_start int32 [R] is the packed index of the
    first row of the row's continuation.  Query r sees keys [0, P) and [P + seg_start[r], P + r] (mh_attn_extend_branches)."""
    R = seg_start.shape[0]
    assert q.shape == (R, H * D) and q.stride(1) == 1 and seg_start.dtype == torch.int32 and seg_start.is_contiguous()
    assert kcache.is_contiguous() and vcache.is_contiguous() and kcache.shape == vcache.shape and kcache.shape[0] == 1 and kcache.shape[2] == H * D
    out = torch.empty(R, H * D, dtype=q.dtype, device=q.device) if out is None else out
    assert out.shape == (R, H * D) and out.is_contiguous()
    L.call("mh_attn_extend_branches", q, q.stride(0), kcache, vcache, out, seg_start, int(P), R, H, D, kcache.shape[1], dt_of(q), _stream())
    return out


def attn_extend_branches_kv8(q, k8, v8, kscale, vscale, seg_start, P, H, D, out=None):
    """attn_extend_branches against the fp8 KV cache (k8, v8 uint8 [1, Smax, H*D]; kscale, vscale fp32 [1, H, Smax])."""
    R = seg_start.shape[0]
    Smax = k8.shape[1]
    assert q.shape == (R, H * D) and q.stride(1) == 1 and seg_start.dtype == torch.int32 and seg_start.is_contiguous()
    assert k8.dtype == v8.dtype == torch.uint8 and k8.shape == v8.shape == (1, Smax, H * D) and k8.is_contiguous() and v8.is_contiguous()
    assert kscale.dtype == vscale.dtype == torch.float32 and kscale.shape == vscale.shape == (1, H, Smax)
    assert kscale.is_contiguous() and vscale.is_contiguous()
    out = torch.empty(R, H * D, dtype=q.dtype, device=q.device) if out is None else out
    assert out.shape == (R, H * D) and out.is_contiguous()
    L.call("mh_attn_extend_branches_kv8", q, q.stride(0), k8, v8, kscale, vscale, out, seg_start, int(P), R, H, D, Smax, dt_of(q), _stream())
    return out


def beam_ancestry(anc_in, anc_out, beam_idx, gen):
    """The table step of HF `_reorder_cache` on a shared prompt cache (mh_beam_ancestry): anc_out[m, :gen[m]] = anc_in[beam_idx[m], :gen[m]],
    anc_out[m, gen[m]] = m; anc int32 [rows, G] (two buffers), beam_idx int64 [rows], gen int32 [rows], all on the device."""
    rows, G = anc_in.shape
    assert anc_in.dtype == anc_out.dtype == gen.dtype == torch.int32 and beam_idx.dtype == torch.int64
    assert anc_out.shape == (rows, G) and beam_idx.shape == gen.shape == (rows,)
    assert anc_in.is_contiguous() and anc_out.is_contiguous() and beam_idx.is_contiguous() and gen.is_contiguous()
    L.call("mh_beam_ancestry", anc_in, anc_out, beam_idx, gen, rows, G, _stream())


def attn_decode_beams_splits(Bp, nb, H, Pmax, G):
    """(prefix key splits, suffix key splits) of attn_decode_beams / _kv8 (mh_attn_decode_beams_splits, mh_attn_decode_beams_suffix_splits);
    0 prefix splits: no plan within the merge kernel's 32 slots and a block's LDS (the call is refused)."""
    return int(L.lib().mh_attn_decode_beams_splits(Bp, nb, H, Pmax, G)), int(L.lib().mh_attn_decode_beams_suffix_splits(G))


def _beams_ws(q, Bp, nb, H, D, Pmax, G):
    ps, ss = attn_decode_beams_splits(Bp, nb, H, Pmax, G)
    return torch.empty(Bp * nb * H * (max(ps, 1) + ss) * (D + 2), dtype=torch.float32, device=q.device)


def attn_decode_beams(q, pre_k, pre_v, pre_lens, suf_k, suf_v, anc, slens, nb, H, D, out=None):
    """Beam-search decode attention on a shared prompt cache: q [Bp*nb, H*D] view (row p*nb + i) against the prompt's keys pre_k / pre_v
    [Bp, Pmax, H*D] (rows < pre_lens[p], loaded once for all nb beams) and the beams' own suf_k / suf_v [Bp*nb, G, H*D], where key g < slens[m]
    of row m lies in row anc[m, g] (int32 [Bp*nb, G])."""
    Bp, Pmax = pre_k.shape[:2]
    rows, G = anc.shape
    assert rows == Bp * nb and q.shape == (rows, H * D) and q.stride(1) == 1 and pre_k.shape == pre_v.shape == (Bp, Pmax, H * D)
    assert suf_k.shape == suf_v.shape == (rows, G, H * D) and pre_k.dtype == suf_k.dtype == q.dtype
    assert all(t.is_contiguous() for t in (pre_k, pre_v, suf_k, suf_v, anc, pre_lens, slens))
    assert anc.dtype == pre_lens.dtype == slens.dtype == torch.int32 and pre_lens.shape == (Bp,) and slens.shape == (rows,)
    out = torch.empty(rows, H * D, dtype=q.dtype, device=q.device) if out is None else out
    L.call("mh_attn_decode_beams", q, q.stride(0), pre_k, pre_v, pre_lens, suf_k, suf_v, anc, slens, out, Bp, nb, H, D, Pmax, G,
           _beams_ws(q, Bp, nb, H, D, Pmax, G), dt_of(q), _stream())
    return out


def attn_decode_beams_kv8(q, pre_k8, pre_v8, pre_ks, pre_vs, pre_lens, suf_k8, suf_v8, suf_ks, suf_vs, anc, slens, nb, H, D, out=None):
    """attn_decode_beams on the fp8 KV cache: uint8 rows as above with fp32 scales pre_ks / pre_vs [Bp, H, Pmax], suf_ks / suf_vs [Bp*nb, H, G]
    (the scale of key g of row m is read at [anc[m, g], h, g])."""
    Bp, Pmax = pre_k8.shape[:2]
    rows, G = anc.shape
    assert rows == Bp * nb and q.shape == (rows, H * D) and q.stride(1) == 1 and pre_k8.shape == pre_v8.shape == (Bp, Pmax, H * D)
    assert suf_k8.shape == suf_v8.shape == (rows, G, H * D) and pre_k8.dtype == pre_v8.dtype == suf_k8.dtype == suf_v8.dtype == torch.uint8
    assert pre_ks.shape == pre_vs.shape == (Bp, H, Pmax) and suf_ks.shape == suf_vs.shape == (rows, H, G)
    assert pre_ks.dtype == pre_vs.dtype == suf_ks.dtype == suf_vs.dtype == torch.float32
    assert all(t.is_contiguous() for t in (pre_k8, pre_v8, pre_ks, pre_vs, suf_k8, suf_v8, suf_ks, suf_vs, anc, pre_lens, slens))
    assert anc.dtype == pre_lens.dtype == slens.dtype == torch.int32 and pre_lens.shape == (Bp,) and slens.shape == (rows,)
    out = torch.empty(rows, H * D, dtype=q.dtype, device=q.device) if out is None else out
    L.call("mh_attn_decode_beams_kv8", q, q.stride(0), pre_k8, pre_v8, pre_ks, pre_vs, pre_lens, suf_k8, suf_v8, suf_ks, suf_vs, anc, slens, out,
           Bp, nb, H, D, Pmax, G, _beams_ws(q, Bp, nb, H, D, Pmax, G), dt_of(q), _stream())
    return out


def ngram_draft(ids, length, max_ngram, k, max_length):
    """Prompt-lookup draft on the device (mh_ngram_draft; generation._prompt_lookup is its restatement): ids int64 [rows, >= length] ->
    (draft int64 [rows, k], count int32 [rows]); only the first count[r] entries of a draft row are written."""
    assert ids.dtype == torch.int64 and ids.dim() == 2 and ids.stride(1) == 1 and ids.shape[1] >= length
    rows = ids.shape[0]
    out = torch.empty(rows, k, dtype=torch.int64, device=ids.device)
    cnt = torch.empty(rows, dtype=torch.int32, device=ids.device)
    L.call("mh_ngram_draft", ids, ids.stride(0), rows, length, max_ngram, k, max_length, out, cnt, _stream())
    return out, cnt


def select_tokens_multi(logits, V=None, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=0, step0=0, min_p=None, epsilon_cutoff=0.0):
    """logits fp32 [B, T, >=V] -> int64 [T, B]: position t of sequence b is drawn as the plain path draws its token number step0 + t, i.e. with
    mh_select_tokens' key (seed, step0 + t, row b) - one launch per t on the strided view logits[:, t].  min_p / epsilon_cutoff: as select_tokens."""
    B, T = logits.shape[:2]
    V = logits.shape[2] if V is None else V
    assert logits.dtype == torch.float32 and logits.stride(2) == 1
    out = torch.empty(T, B, dtype=torch.int64, device=logits.device)
    warp = min_p is not None or epsilon_cutoff
    for t in range(T):
        if warp:
            L.call("mh_select_tokens_warp", logits[:, t], logits.stride(0), B, V, int(do_sample), temperature, top_k, top_p, float(min_p or 0.0),
                   float(epsilon_cutoff or 0.0), seed & 0xFFFFFFFFFFFFFFFF, step0 + t, out[t], None, _stream())
        else:
            L.call("mh_select_tokens", logits[:, t], logits.stride(0), B, V, int(do_sample), temperature, top_k, top_p, seed & 0xFFFFFFFFFFFFFFFF, step0 + t,
                   out[t], None, _stream())
    return out


def ban_tokens(logits, V=None, ids=None, len0=0, len_step=0, ld_ids=None, ngram=0, words=None, word_off=None, always=None, begin=None, begin_index=-1,
               eos=None, min_total=0):
    """-inf into the banned columns of logits fp32 [R, >=V], in place (mh_ban_tokens; generation._banned is its restatement).  ids int64
    [rows, >= len] is the history, row r's first len0 + r * len_step entries valid; ld_ids=0: every row reads ids[0] (the rows of a verify
    step).  ngram: no_repeat_ngram_size; words / word_off: flat int64 tokens + int32 offsets [n_words + 1] (generation._pack_words);
    always / begin / eos: int64 id lists, begin banned when the length is begin_index, eos while it is below min_total.  -> logits."""
    R = logits.shape[0]
    V = logits.shape[1] if V is None else V
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    ld = 0
    if ids is not None:
        assert ids.dtype == torch.int64 and ids.dim() == 2 and ids.stride(1) == 1 and ids.device == logits.device
        ld = ids.stride(0) if ld_ids is None else int(ld_ids)
        assert ld == 0 or (ld == ids.stride(0) and ids.shape[0] >= R)
        assert 0 <= len0 and 0 <= len_step and len0 + (R - 1) * len_step <= ids.shape[1], (len0, len_step, R, tuple(ids.shape))
    n_words = 0
    if words is not None:
        assert words.dtype == torch.int64 and word_off.dtype == torch.int32 and words.is_contiguous() and word_off.is_contiguous()
        n_words = word_off.numel() - 1
    for t in (always, begin, eos):
        assert t is None or (t.dtype == torch.int64 and t.is_contiguous() and t.device == logits.device)
    cnt = lambda t: 0 if t is None else t.numel()  # noqa: E731
    L.call("mh_ban_tokens", logits, logits.stride(0), R, V, ids, ld, int(len0), int(len_step), int(ngram), words, word_off, n_words, always, cnt(always),
           begin, cnt(begin), int(begin_index), eos, cnt(eos), int(min_total), _stream())
    return logits


def _dev_counter(t, dtype, device):
    """A device-resident counter of the *_dev launches: one element of `dtype` on `device` (a view into a larger buffer is fine)."""
    assert isinstance(t, torch.Tensor) and t.dtype == dtype and t.numel() >= 1 and t.device == device, "a device counter: one element of the given type"
    return t


def ban_tokens_dev(logits, V, ids, len_base, len0=0, len_step=0, ld_ids=None, ngram=0, words=None, word_off=None, always=None, begin=None,
                   begin_index=-1, eos=None, min_total=0):
    """ban_tokens with the history length on the device (mh_ban_tokens_dev): row r conditions on the first len_base[0] + len0 + r * len_step
    entries of its ids row, len_base int32 [>= 1] on the logits' device, read at kernel entry - a captured launch follows the counter.
    Same kernel as ban_tokens: bit-identical at equal length.  A row whose length falls outside [0, ids.shape[1]] is left alone."""
    R = logits.shape[0]
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    _dev_counter(len_base, torch.int32, logits.device)
    ld = cols = 0
    if ids is not None:
        assert ids.dtype == torch.int64 and ids.dim() == 2 and ids.stride(1) == 1 and ids.device == logits.device
        ld, cols = (ids.stride(0) if ld_ids is None else int(ld_ids)), ids.shape[1]
        assert ld == 0 or (ld == ids.stride(0) and ids.shape[0] >= R)
    n_words = 0
    if words is not None:
        assert words.dtype == torch.int64 and word_off.dtype == torch.int32 and words.is_contiguous() and word_off.is_contiguous()
        n_words = word_off.numel() - 1
    for t in (always, begin, eos):
        assert t is None or (t.dtype == torch.int64 and t.is_contiguous() and t.device == logits.device)
    cnt = lambda t: 0 if t is None else t.numel()  # noqa: E731
    L.call("mh_ban_tokens_dev", logits, logits.stride(0), R, V, ids, ld, cols, len_base, int(len0), int(len_step), int(ngram), words, word_off, n_words,
           always, cnt(always), begin, cnt(begin), int(begin_index), eos, cnt(eos), int(min_total), _stream())
    return logits


def select_tokens_dev(logits, V, step_base, step_off=0, out=None, ids=None, len_base=None, len_off=0, do_sample=False, temperature=1.0, top_k=0,
                      top_p=1.0, seed=0, return_u=False, min_p=None, epsilon_cutoff=0.0):
    """select_tokens with the step number on the device (mh_select_tokens_dev): row r is drawn with the key (seed, step_base[0] + step_off, r),
    step_base int64 [>= 1] on the logits' device, read at kernel entry.  out int64 [R] (default: a new tensor) gets the tokens; ids int64
    [>= R, cols] (optional, with len_base int32 [>= 1]) gets them too, at column len_base[0] + len_off of every row - nowhere when that
    column is outside the row.  Same kernel as select_tokens: the same tokens and uniforms at equal step."""
    R = logits.shape[0]
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    _dev_counter(step_base, torch.int64, logits.device)
    if out is None:
        out = torch.empty(R, dtype=torch.int64, device=logits.device)
    assert out.dtype == torch.int64 and out.numel() >= R and out.is_contiguous() and out.device == logits.device
    ld = cols = 0
    if ids is not None:
        assert ids.dtype == torch.int64 and ids.dim() == 2 and ids.stride(1) == 1 and ids.device == logits.device and ids.shape[0] >= R
        _dev_counter(len_base, torch.int32, logits.device)
        ld, cols = ids.stride(0), ids.shape[1]
    u = torch.empty(R, dtype=torch.float32, device=logits.device) if return_u else None
    L.call("mh_select_tokens_dev", logits, logits.stride(0), R, V, int(do_sample), temperature, top_k, top_p, float(min_p or 0.0), float(epsilon_cutoff or 0.0),
           seed & 0xFFFFFFFFFFFFFFFF, step_base, int(step_off), out, u, ids, ld, cols, len_base, int(len_off), _stream())
    return (out, u) if return_u else out


_splitk_ws = {}
SPLITK_WS_MIN = 256 * 65536  # floats: one round of 256 tiles of fp32 partials (the most mh_gemm_splitk_max ever asks for)


def _splitk_workspace(device, numel):
    """fp32 partials of the split-K GEMMs: ONE grow-only buffer per (device, stream).  Launches on one stream are ordered, so
    consecutive GEMMs may share it; two streams never do (a size-keyed, process-global cache let concurrent streams race on the
    partials and thrashed on variable-length batches).  While the stream is being captured into a HIP graph the buffer comes from
    the graph's own memory pool and is NOT cached (it must not outlive the graph; the pool re-uses the block for the next GEMM of
    the capture): a captured prefill / wide decode step keeps the split path and with it the eager path's summation order -
    graph and eager logits stay bit-identical."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(numel, dtype=torch.float32, device=device)
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _splitk_ws.get(key)
    if ws is None or ws.numel() < numel:
        if len(_splitk_ws) > 16:  # streams come and go (side streams of captures, tests): drop the buffers of the others
            _splitk_ws.clear()
        ws = _splitk_ws[key] = torch.empty(max(numel, SPLITK_WS_MIN), dtype=torch.float32, device=device)
    return ws


def _skinny_splitk_ok(dtype):
    """Split-K for skinny products (profiles/r03_skinny_gemm.txt).  Kept to bf16, the performance dtype: fp16 is the dtype BASELINE's
    logits tolerance is stated in, and its full-depth bound (tests/test_model_gpu.py) is held with the one-pass summation order it was
    measured with - the single-element maximum moves by +-25 % under ANY change of summation order.  MH_SKINNY_SPLITK=0 / =2 force it
    off / on for every dtype (A/B).  The same decision inside and outside a HIP-graph capture (_splitk_workspace)."""
    if not SKINNY_SPLITK:
        return False
    return dtype == torch.bfloat16 or SKINNY_SPLITK_ALL


_tail_plans = {}


def _tail_plan(M, N, T):
    """256 x 256 output tiles on 256 CUs run in rounds; a weight gradient whose tile count is not a multiple of 256 leaves the
    last round partly empty (gate|up: 86 x 16 = 1376 tiles = 5.375 rounds -> 6; down: 16 x 43 = 688 = 2.69 -> 3: 10-12 % of
    GEMMs that contract over all 32 768 tokens).  Plan: cut the output into a part that fills whole rounds and a remainder that
    is split along K (tokens) so that ITS blocks fill whole, proportionally shorter rounds.  Returns None or
    (axis 'm' | 'n', cut in elements, splits of the remainder)."""
    key = (M, N, T)
    if key in _tail_plans:
        return _tail_plans[key]
    if os.environ.get("MH_NO_TAIL_PLAN"):  # A/B switch for kernel development
        return None
    tm, tn = (M + 255) // 256, (N + 255) // 256
    tiles, nk = tm * tn, (T + 63) // 64
    plan = None
    if tiles >= 256 and nk >= 128 and M % 256 == 0 and N % 256 == 0:
        best = -(-tiles // 256) * 0.96  # must beat the plain launch by > 4 % (the reduce pass and a second launch are not free)
        for axis, ta, tb in (("m", tm, tn), ("n", tn, tm)):
            for a in range(ta - 1, 0, -1):
                ca = -(-(a * tb) // 256)
                if ca * 256 - a * tb > 0.03 * a * tb:
                    continue
                rem = (ta - a) * tb
                for sp in range(2, 17):
                    if nk // sp < 16:
                        break
                    # remainder rounds are 1/sp long; its fp32 partials (sp x rem tiles) are written and read once at ~5 TB/s,
                    # expressed in rounds (one full-K round of 256 tiles takes ~T x 25.7 ns at the kernel's rate)
                    cost = ca + -(-(rem * sp) // 256) / sp + 0.02 + sp * rem * 524288 / 5e12 / (T * 25.7e-9)
                    if cost < best:
                        best, plan = cost, (axis, a * 256, sp)
    _tail_plans[key] = plan
    return plan


def _wgrad_call(dy, x, out, accum, splits):
    T, M = dy.shape
    N = x.shape[1]
    ws = _splitk_workspace(dy.device, splits * M * N) if splits > 1 else None
    L.call("mh_gemm_splitk", dy, _rowmajor(dy), 1, x, _rowmajor(x), 1, out, _rowmajor(out), M, N, T, dt_of(dy), int(accum), int(out.dtype == torch.float32),
           splits, ws, _stream())


def wgrad_tn(dy, x, out, accum):
    """out[N_out, K_in] (+)= dy[T, N_out]^T @ x[T, K_in]: both operands K-strided as they lie in memory, any T (the
    kernel reads rows >= T of the last K-tile as zeros), split-K when the output has too few tiles to fill the chip, and a
    two-part launch (full rounds + a K-split remainder, see _tail_plan) when its tile count leaves a partly empty last round."""
    T, M = dy.shape
    T2, N = x.shape
    assert T == T2 and dy.dtype == x.dtype and M % 8 == 0 and N % 8 == 0
    with _timed("gemm_nt", 2.0 * M * N * T, 2.0 * (M * T + N * T + M * N)):
        plan = _tail_plan(M, N, T)
        if plan is None:
            _wgrad_call(dy, x, out, accum, int(L.lib().mh_gemm_splitk_max(M, N, T)))
        else:
            axis, cut, sp = plan
            if axis == "m":
                _wgrad_call(dy[:, :cut], x, out[:cut], accum, 1)
                _wgrad_call(dy[:, cut:], x, out[cut:], accum, sp)
            else:
                _wgrad_call(dy, x[:, :cut], out[:, :cut], accum, 1)
                _wgrad_call(dy, x[:, cut:], out[:, cut:], accum, sp)
    return out


class _WgradProblem(C.Structure):
    _fields_ = [("dy", C.c_void_p), ("lddy", C.c_int64), ("x", C.c_void_p), ("ldx", C.c_int64), ("out", C.c_void_p), ("ldo", C.c_int64),
                ("M", C.c_int), ("N", C.c_int), ("accumulate", C.c_int), ("reserved", C.c_int)]


WGRAD_GROUPED = os.environ.get("MH_WGRAD_GROUPED", "1") != "0"  # A/B switch
WGRAD_GROUPED_MIN_TILES = 32  # below that (the tiny test models) the per-problem launches are used unless forced


def wgrad_group_pays(T, shapes):
    """Launch-plan predicate of wgrad_tn_grouped for problems of shapes [(M_p, N_p)] over T tokens (host arithmetic only)."""
    tiles = sum(((m + 255) // 256) * ((n + 255) // 256) for m, n in shapes)
    return WGRAD_GROUPED and len(shapes) <= 8 and T >= 1024 and tiles >= WGRAD_GROUPED_MIN_TILES and all(m % 8 == 0 and n % 8 == 0 for m, n in shapes)


def wgrad_tn_grouped(problems, accum, force=False):
    """[(dy [T, M_p], x [T, N_p], out [M_p, N_p])] -> out_p (+)= dy_p^T x_p for all p in ONE launch (mh_wgrad_grouped: one block per
    256 x 256 tile of any problem, whole contraction, no fp32 partials); falls back to wgrad_tn per problem when the group is too small
    to matter or a problem does not meet the kernel's layout conditions."""
    T = problems[0][0].shape[0]
    ok = len(problems) <= 8 and all(dy.shape[0] == T and x.shape[0] == T and dy.dtype == x.dtype == out.dtype and
                                    out.dtype in (torch.bfloat16, torch.float16) for dy, x, out in problems)
    if ok and (force or wgrad_group_pays(T, [(dy.shape[1], x.shape[1]) for dy, x, _ in problems])):
        arr = (_WgradProblem * len(problems))()
        flops = nbytes = 0.0
        for i, (dy, x, out) in enumerate(problems):
            arr[i] = _WgradProblem(dy.data_ptr(), _rowmajor(dy), x.data_ptr(), _rowmajor(x), out.data_ptr(), _rowmajor(out), dy.shape[1], x.shape[1],
                                   int(accum), 0)
            flops += 2.0 * dy.shape[1] * x.shape[1] * T
            nbytes += 2.0 * (dy.shape[1] * T + x.shape[1] * T + dy.shape[1] * x.shape[1])
        with _timed("gemm_nt", flops, nbytes):
            rc = L.launch("mh_wgrad_grouped", arr, len(problems), T, dt_of(problems[0][0]), _stream())
        if rc == 0:
            return
        if rc != -4:  # MH_ERR_SHAPE = "not for this kernel": per-problem launches below; anything else is an error
            L.check(rc, "mh_wgrad_grouped")
    for dy, x, out in problems:
        wgrad_tn(dy, x, out, accum)


def gemm_nt_rope(a, b, table, S, H, D, out=None):
    """qkv = a @ b^T with RoPE applied to the q and k heads in the GEMM epilogue (b = fused [q; k; v] weight, 3*H*D rows)."""
    M, K = a.shape
    N = b.shape[0]
    assert N == 3 * H * D and b.shape[1] == K and a.dtype == b.dtype
    out = torch.empty(M, N, dtype=a.dtype, device=a.device) if out is None else out
    with _timed("gemm_nt", 2.0 * M * N * K, 2.0 * (M * K + N * K + M * N)):
        L.call("mh_gemm_nt_rope", a, _rowmajor(a), b, _rowmajor(b), out, _rowmajor(out), M, N, K, dt_of(a), table, S, D, 2 * H * D, _stream())
    return out


def gemm_swiglu_fwd(x, wgu):
    """gu = x @ wgu^T ([gate; up] rows) and act = silu(gate) * up from ONE GEMM launch.  Returns (gu, act)."""
    M, K = x.shape
    ff = wgu.shape[0] // 2
    gu = torch.empty(M, 2 * ff, dtype=x.dtype, device=x.device)
    act = torch.empty(M, ff, dtype=x.dtype, device=x.device)
    with _timed("gemm_nt", 2.0 * M * 2 * ff * K, 2.0 * (M * K + 2 * ff * K + 3 * M * ff)):
        L.call("mh_gemm_swiglu_fwd", x, _rowmajor(x), wgu, _rowmajor(wgu), gu, 2 * ff, act, ff, M, ff, K, dt_of(x), _stream())
    return gu, act


def gemm_swiglu_bwd(dy, wd, gu):
    """dgu = swiglu_bwd(gu, dy @ wd) with the SwiGLU backward in the dgrad GEMM's epilogue (dact never stored).
    wd = down_proj.weight [d_model, ff]."""
    M, K = dy.shape
    ff = wd.shape[1]
    assert wd.shape[0] == K and gu.shape == (M, 2 * ff)
    dgu = torch.empty_like(gu)
    with _timed("gemm_nt", 2.0 * M * ff * K, 2.0 * (M * K + ff * K + 4 * M * ff)):
        L.call("mh_gemm_swiglu_bwd", dy, _rowmajor(dy), wd, _rowmajor(wd), gu, _rowmajor(gu), dgu, _rowmajor(dgu), M, ff, K, dt_of(dy), _stream())
    return dgu


def gemm_gelu_fwd(x, w1, bias):
    """(f1, a) = (x @ w1^T + bias, quick_gelu(f1)) from ONE GEMM launch (CLIP MLP fc1; the backward needs f1, fc2 needs a)."""
    M, K = x.shape
    N = w1.shape[0]
    f1 = torch.empty(M, N, dtype=x.dtype, device=x.device)
    a = torch.empty(M, N, dtype=x.dtype, device=x.device)
    with _timed("gemm_nt", 2.0 * M * N * K, 2.0 * (M * K + N * K + 2 * M * N)):
        L.call("mh_gemm_gelu_fwd", x, _rowmajor(x), w1, _rowmajor(w1), bias, f1, N, a, N, M, N, K, dt_of(x), _stream())
    return f1, a


def gemm_gelu_bwd(dy, w2, f1):
    """df1 = quick_gelu'(f1) * (dy @ w2) with the GELU backward in the dgrad GEMM's store phase (dy @ w2 never stored); w2 = fc2.weight [d, ff]."""
    M, K = dy.shape
    N = w2.shape[1]
    assert w2.shape[0] == K and f1.shape == (M, N)
    df1 = torch.empty_like(f1)
    with _timed("gemm_nt", 2.0 * M * N * K, 2.0 * (M * K + N * K + 2 * M * N)):
        L.call("mh_gemm_gelu_bwd", dy, _rowmajor(dy), w2, _rowmajor(w2), f1, _rowmajor(f1), df1, _rowmajor(df1), M, N, K, dt_of(dy), _stream())
    return df1


def quant_fp8_rows(x, k_pad=None):
    """x [R, K] (16-bit) -> (q uint8 [R, K] OCP e4m3, scales fp32 [R]): one scale per row.  k_pad > K: q is [R, k_pad], zero behind K."""
    R, K = x.shape
    q = torch.zeros(R, k_pad, dtype=torch.uint8, device=x.device) if (k_pad is not None and k_pad > K) else torch.empty(R, K, dtype=torch.uint8, device=x.device)
    sc = torch.empty(R, dtype=torch.float32, device=x.device)
    L.call("mh_quant_fp8_rows", x, _rowmajor(x), q, q.stride(0), sc, R, K, dt_of(x), _stream())
    return q, sc


_amax_ws = {}


def _b3(b8):
    """(q, row scales[, block exponents]) -> always a triple."""
    return (b8[0], b8[1], b8[2] if len(b8) > 2 else None)


def _exp_image(n_rows, k, device):
    G = round_up((k // 128) * 64, 4096)
    return torch.zeros(16 + ((n_rows + 255) // 256) * 2 * G, dtype=torch.uint8, device=device)  # 16-byte flag header + image


def quant_fp8_rows_e4(w):
    """Weights for the fp8 GEMMs: w [N, K] -> (q uint8 [N, K] e4m3, s fp32 [N], exps): per-row scale s[n] and a 4-bit exponent per
    (row, 128-k block), block scale = s[n] * 2^-e - BASELINE cfg 5's per-128-block scales in the form the MFMA applies itself."""
    N, K = w.shape
    assert K % 128 == 0 and w.stride(1) == 1
    q = torch.empty(N, K, dtype=torch.uint8, device=w.device)
    sc = torch.empty(N, dtype=torch.float32, device=w.device)
    ex = _exp_image(N, K, w.device)
    L.call("mh_quant_fp8_rows_e4", w, _rowmajor(w), q, sc, ex, N, K, dt_of(w), _stream())
    return q, sc, ex


def quant_fp8_rows_t_e4(w):
    """w [R, C] -> (qt [C, round_up(R, 128)], s [C], exps): the same format for w^T (rows = input channels, blocks of 128 output channels)."""
    R, C_ = w.shape
    Rp = round_up(R, 128)
    qt = torch.empty(C_, Rp, dtype=torch.uint8, device=w.device)
    sc = torch.empty(C_, dtype=torch.float32, device=w.device)
    ex = _exp_image(C_, Rp, w.device)
    ws = _amax_ws.get((w.device, C_))
    if ws is None:
        ws = _amax_ws[(w.device, C_)] = torch.empty(C_, dtype=torch.int32, device=w.device)
    L.call("mh_quant_fp8_rows_t_e4", w, _rowmajor(w), qt, Rp, sc, ex, ws, R, C_, dt_of(w), _stream())
    return qt, sc, ex


def quant_fp8_rows_t(x):
    """x [R, C] (16-bit) -> (qt uint8 [C, round_up(R, 128)] = e4m3(x^T / s), s fp32 [C]): the column-scaled TRANSPOSED operand
    (zero-filled pad columns) the wgrad / dgrad GEMMs of the fp8 training step contract over."""
    R, C_ = x.shape
    Rp = round_up(R, 128)
    qt = torch.empty(C_, Rp, dtype=torch.uint8, device=x.device)
    sc = torch.empty(C_, dtype=torch.float32, device=x.device)
    ws = _amax_ws.get((x.device, C_))
    if ws is None:
        ws = _amax_ws[(x.device, C_)] = torch.empty(C_, dtype=torch.int32, device=x.device)
    L.call("mh_quant_fp8_rows_t", x, _rowmajor(x), qt, Rp, sc, ws, R, C_, dt_of(x), _stream())
    return qt, sc


_both_ws = {}


def quant_fp8_both(x, c_pad=None, amax=None):
    """x [R, C] (16-bit) -> ((q [R, C], s_row [R]), (qt [C, round_up(R, 128)], s_col [C])): the row-quantised operand (dgrad) and the
    transposed, per-feature-scaled operand (wgrad) of a gradient tensor from two reads of it.  c_pad > C: q is [R, c_pad] with zero
    columns behind C (a contraction length that is not a whole number of 128-blocks: the vocabulary).
    amax: int32 [R + C] = the tensor's row then column maxima as its producer left them (gemm_fp8_swiglu_bwd(..., want_amax=True)):
    ONE read of x, identical bytes."""
    R, C_ = x.shape
    Rp = round_up(R, 128)
    if c_pad is not None and c_pad > C_:
        q = torch.zeros(R, c_pad, dtype=torch.uint8, device=x.device)
    else:
        q = torch.empty(R, C_, dtype=torch.uint8, device=x.device)
    sr = torch.empty(R, dtype=torch.float32, device=x.device)
    qt = torch.empty(C_, Rp, dtype=torch.uint8, device=x.device)
    sc = torch.empty(C_, dtype=torch.float32, device=x.device)
    if amax is not None:
        assert amax.dtype == torch.int32 and amax.numel() == R + C_ and amax.is_contiguous()
        L.call("mh_quant_fp8_rows_and_t_pre", x, _rowmajor(x), q, q.stride(0), sr, qt, Rp, sc, amax, R, C_, dt_of(x), _stream())
        return (q, sr), (qt, sc)
    ws = _both_ws.get((x.device, R + C_))
    if ws is None:
        if len(_both_ws) > 16:
            _both_ws.clear()
        ws = _both_ws[(x.device, R + C_)] = torch.empty(R + C_, dtype=torch.int32, device=x.device)
    L.call("mh_quant_fp8_rows_and_t", x, _rowmajor(x), q, q.stride(0), sr, qt, Rp, sc, ws, R, C_, dt_of(x), _stream())
    return (q, sr), (qt, sc)


def quant_fp8_t_from_rows(x, row_scales):
    """x [R, C] (16-bit) -> (qt uint8 [C, round_up(R, 128)], s fp32 [C] = one tensor-wide scale, the largest of x's row scales
    as produced by quant_fp8_rows): the transposed operand of the wgrad GEMMs in ONE pass over x."""
    R, C_ = x.shape
    Rp = round_up(R, 128)
    qt = torch.empty(C_, Rp, dtype=torch.uint8, device=x.device)
    sc = torch.empty(C_, dtype=torch.float32, device=x.device)
    L.call("mh_max_to_vec", row_scales, row_scales.numel(), sc, C_, _stream())
    L.call("mh_quant_fp8_t_scaled", x, _rowmajor(x), qt, Rp, sc, R, C_, dt_of(x), _stream())
    return qt, sc


def gemm_fp8_swiglu_bwd(dy8, wdt8, gu, want_amax=False):
    """dgu = swiglu_bwd(gu, dy Wd) on the scaled-fp8 MFMA; dy8 = rowquant(dy) [T, d], wdt8 = rowquant(Wd^T) [ff, d].
    want_amax: returns (dgu, amax int32 [T + 2 ff]) - the row / column maxima of |dgu| taken in the GEMM's store phase (quant_fp8_both(dgu, amax=...))."""
    (qa, sa), (qb, sb, eb) = dy8[:2], _b3(wdt8)
    M, K = qa.shape
    ff = qb.shape[0]
    assert qb.shape[1] == K and gu.shape == (M, 2 * ff)
    dgu = torch.empty_like(gu)
    if want_amax:
        amax = torch.empty(M + 2 * ff, dtype=torch.int32, device=gu.device)
        with _timed("gemm_fp8", 2.0 * M * ff * K):
            L.call("mh_gemm_fp8_swiglu_bwd_amax", qa, qa.stride(0), sa, qb, qb.stride(0), sb, eb, gu, _rowmajor(gu), dgu, _rowmajor(dgu), amax, M, ff, K,
                   dt_of(gu), _stream())
        return dgu, amax
    with _timed("gemm_fp8", 2.0 * M * ff * K):
        L.call("mh_gemm_fp8_swiglu_bwd", qa, qa.stride(0), sa, qb, qb.stride(0), sb, eb, gu, _rowmajor(gu), dgu, _rowmajor(dgu), M, ff, K, dt_of(gu), _stream())
    return dgu


def gemm_fp8(a8, b8, out_dtype=torch.bfloat16, out=None, bias=None, resid=None, act=None, accum=False, dt16=torch.bfloat16):
    """out[M, N] = (sa qa) @ (sb qb)^T on the scaled-fp8 MFMA; a8 = (qa [M, K] uint8, sa [M]), b8 = (qb [N, K], sb [N]).
    A float32 `out` / out_dtype selects the fp32 store phase (the lm_head logits); dt16 is then the type of bias / resid."""
    (qa, sa), (qb, sb, eb) = a8[:2], _b3(b8)
    M, K = qa.shape
    N = qb.shape[0]
    assert qb.shape[1] == K
    out = torch.empty(M, N, dtype=out_dtype, device=qa.device) if out is None else out
    epi, ldr = _epilogue(bias, act, resid, accum, out)
    dt = dt_of(dt16 if out.dtype == torch.float32 else out)
    with _timed("gemm_fp8", 2.0 * M * N * K):
        L.call("mh_gemm_fp8", qa, qa.stride(0), sa, qb, qb.stride(0), sb, eb, out, _rowmajor(out), bias, resid, ldr, M, N, K, dt, epi, _stream())
    return out


def gemm_fp8_rope(a8, b8, table, S, H, D, out_dtype=torch.bfloat16):
    """fp8 q|k|v projection with RoPE in the epilogue (see gemm_nt_rope)."""
    (qa, sa), (qb, sb, eb) = a8[:2], _b3(b8)
    M, K = qa.shape
    N = qb.shape[0]
    out = torch.empty(M, N, dtype=out_dtype, device=qa.device)
    with _timed("gemm_fp8", 2.0 * M * N * K):
        L.call("mh_gemm_fp8_rope", qa, qa.stride(0), sa, qb, qb.stride(0), sb, eb, out, N, M, N, K, dt_of(out), table, S, D, 2 * H * D, _stream())
    return out


def gemm_fp8_swiglu_fwd(a8, b8, out_dtype=torch.bfloat16):
    """fp8 gate|up projection with SwiGLU in the epilogue (see gemm_swiglu_fwd).  Returns (gu, act)."""
    (qa, sa), (qb, sb, eb) = a8[:2], _b3(b8)
    M, K = qa.shape
    ff = qb.shape[0] // 2
    gu = torch.empty(M, 2 * ff, dtype=out_dtype, device=qa.device)
    act = torch.empty(M, ff, dtype=out_dtype, device=qa.device)
    with _timed("gemm_fp8", 2.0 * M * 2 * ff * K):
        L.call("mh_gemm_fp8_swiglu_fwd", qa, qa.stride(0), sa, qb, qb.stride(0), sb, eb, gu, 2 * ff, act, ff, M, ff, K, dt_of(gu), _stream())
    return gu, act


def transpose16(x, r_pad=None, out=None):
    """x[R, C] (16-bit) -> out[C, R_pad] with zero-filled tail columns."""
    R, Cc = x.shape
    ldi = _rowmajor(x)
    r_pad = R if r_pad is None else r_pad
    if out is None:
        out = torch.empty(Cc, r_pad, dtype=x.dtype, device=x.device)
    L.call("mh_transpose16", x, ldi, out, _rowmajor(out), R, Cc, r_pad, _stream())
    return out


def rmsnorm_fwd(x, w, eps, out=None):
    rows, d = x.shape
    assert x.is_contiguous() and w.is_contiguous()
    out = torch.empty_like(x) if out is None else out
    L.call("mh_rmsnorm_fwd", x, w, out, None, rows, d, eps, dt_of(x), _stream())
    return out


def rmsnorm_fwd_q8(x, w, eps):
    """-> (y, (q uint8 [rows, d], scales fp32 [rows])): RMSNorm + row-quantised e4m3 copy of its output in one launch."""
    rows, d = x.shape
    assert x.is_contiguous() and w.is_contiguous()
    y = torch.empty_like(x)
    q = torch.empty(rows, d, dtype=torch.uint8, device=x.device)
    sc = torch.empty(rows, dtype=torch.float32, device=x.device)
    L.call("mh_rmsnorm_fwd_q8", x, w, y, q, sc, rows, d, eps, dt_of(x), _stream())
    return y, (q, sc)


def norm_partials(rows: int) -> int:
    return int(L.lib().mh_norm_bwd_partials(rows))


def reduce_partials(partial, nblk, d, out, accumulate):
    L.call("mh_reduce_partials", partial, nblk, d, out, dt_of(out), int(accumulate), _stream())


def rmsnorm_bwd(x, w, dy, eps, dx=None, accumulate_dx=False, dw_out=None, dw_accumulate=False, ws=None):
    """Returns dx; writes (or accumulates) dw into dw_out (16-bit or fp32 [d])."""
    rows, d = x.shape
    nblk = norm_partials(rows)
    part = torch.empty(nblk, d, dtype=torch.float32, device=x.device) if ws is None else ws
    dx = torch.empty_like(x) if dx is None else dx
    L.call("mh_rmsnorm_bwd", x, w, dy, dx, part, rows, d, eps, dt_of(x), int(accumulate_dx), _stream())
    if dw_out is not None:
        reduce_partials(part, nblk, d, dw_out, dw_accumulate)
    return dx


def layernorm_fwd(x, w, b, eps, out=None):
    rows, d = x.shape
    assert x.is_contiguous()
    out = torch.empty_like(x) if out is None else out
    L.call("mh_layernorm_fwd", x, w, b, out, rows, d, eps, dt_of(x), _stream())
    return out


def layernorm_bwd(x, w, dy, eps, dx=None, accumulate_dx=False, dw_out=None, db_out=None, accumulate=False):
    rows, d = x.shape
    nblk = norm_partials(rows)
    pw = torch.empty(nblk, d, dtype=torch.float32, device=x.device)
    pb = torch.empty(nblk, d, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x) if dx is None else dx
    L.call("mh_layernorm_bwd", x, w, dy, dx, pw, pb, rows, d, eps, dt_of(x), int(accumulate_dx), _stream())
    if dw_out is not None:
        reduce_partials(pw, nblk, d, dw_out, accumulate)
    if db_out is not None:
        reduce_partials(pb, nblk, d, db_out, accumulate)
    return dx


def colsum(x, out, accumulate=False):
    """out[d] (+)= sum over rows of x[rows, d] (bias gradient)."""
    rows, d = x.shape
    nblk = norm_partials(rows)
    part = torch.empty(nblk, d, dtype=torch.float32, device=x.device)
    L.call("mh_colsum_partial", x, _rowmajor(x), part, rows, d, dt_of(x), _stream())
    reduce_partials(part, nblk, d, out, accumulate)
    return out


def swiglu_fwd(gu, out=None):
    rows, ff2 = gu.shape
    ff = ff2 // 2
    assert gu.is_contiguous()
    out = torch.empty(rows, ff, dtype=gu.dtype, device=gu.device) if out is None else out
    L.call("mh_swiglu_fwd", gu, out, rows, ff, dt_of(gu), _stream())
    return out


def swiglu_bwd(gu, dout, dgu=None):
    rows, ff2 = gu.shape
    dgu = torch.empty_like(gu) if dgu is None else dgu
    L.call("mh_swiglu_bwd", gu, dout, dgu, rows, ff2 // 2, dt_of(gu), _stream())
    return dgu


def quick_gelu_fwd(x, out=None):
    out = torch.empty_like(x) if out is None else out
    L.call("mh_quick_gelu_fwd", x, out, x.numel(), dt_of(x), _stream())
    return out


def quick_gelu_bwd(x, dy, dx=None):
    dx = torch.empty_like(x) if dx is None else dx
    L.call("mh_quick_gelu_bwd", x, dy, dx, x.numel(), dt_of(x), _stream())
    return dx


def add(a, b, out=None):
    out = torch.empty_like(a) if out is None else out
    L.call("mh_add", a, b, out, a.numel(), dt_of(a), _stream())
    return out


def convert(src, dst):
    assert src.numel() == dst.numel() and src.is_contiguous() and dst.is_contiguous()
    L.call("mh_convert", src, dt_of(src), dst, dt_of(dst), src.numel(), _stream())
    return dst


def fill_normal_(t, key: int, start: int = 0, sigma: float = 0.02, offset: float = 0.0):
    assert t.is_contiguous()
    L.call("mh_fill_normal", t, t.numel(), key, start, sigma, offset, dt_of(t), _stream())
    return t


def rope_table(S, D, theta, device):
    tab = torch.empty(S, D // 2, 2, dtype=torch.float32, device=device)
    L.call("mh_rope_table", tab, S, D, theta, _stream())
    return tab


def rope_qk_(qkv, table, S, H, D, inverse=False):
    """qkv [T, 3*H*D] (fused q|k|v rows) rotated in place on q and k."""
    T = qkv.shape[0]
    assert qkv.is_contiguous() and qkv.shape[1] == 3 * H * D
    L.call("mh_rope_qk", qkv, table, T, S, H, D, int(inverse), dt_of(qkv), _stream())
    return qkv


def attn_fwd2(q, k, v, B, S, H, D, causal, seqlens=None, out=None, lse=None):
    """q, k, v: [B*S, H*D] views (own row strides).  Returns (o [B*S, H*D], lse [B,H,S_pad]).  No V re-layout pass."""
    out = torch.empty(B * S, H * D, dtype=q.dtype, device=q.device) if out is None else out
    if lse is None:  # the kernel writes rows < S; the pad rows of a ragged S_pad must read as zeros in the backward
        lse = (torch.empty if S % 64 == 0 else torch.zeros)(B, H, round_up(S, 64), dtype=torch.float32, device=q.device)
    L.call("mh_attn_fwd2", q, q.stride(0), k, k.stride(0), v, v.stride(0), out, out.stride(0), lse, seqlens, B, S, H, D, int(causal), dt_of(q), _stream())
    return out, lse


_delta_cache = {}


def _delta_ws(B, H, S, device):
    """[2, B, H, S_pad] fp32 scratch of the attention backward (S_pad = S rounded up to 64), reused across calls (same stream => ordered).
    The kernels write rows < S and READ the pad rows [S, S_pad) of a partial last tile, which must be zero at every call
    (include/merlin_hip.h, mh_attn_bwd2): a masked row's dS is P x (dP - delta) = 0 x delta, NaN where a stale delta is not finite.
    So the buffer is zeroed once and the cache is keyed on S, not on S_pad: two lengths with the same S_pad never share one, and
    under any key the pad rows are never written."""
    key = (device, B, H, S)
    ws = _delta_cache.get(key)
    if ws is None:
        if len(_delta_cache) > 8:
            _delta_cache.clear()
        ws = _delta_cache[key] = torch.zeros(2, B, H, round_up(S, 64), dtype=torch.float32, device=device)
    return ws


_spill_cache = {}
LAST_ATTN_BWD_FORM = None
ATTN_BWD_SPILL = os.environ.get("MH_ATTN_BWD_SPILL", "1") != "0"  # five-product backward (dS spilled by the dK|dV kernel) where it applies


def attn_bwd_spill(on: bool):
    """A/B switch: the causal D = 128 backward runs in its five-product form (dS written by the dK|dV kernel, dQ = dS K as a one-product pass)."""
    global ATTN_BWD_SPILL
    ATTN_BWD_SPILL = bool(on)


ATTN_SPILL_MAX_BYTES = int(float(os.environ.get("MH_ATTN_SPILL_MAX_GB", "12")) * 2 ** 30)  # cap of the dS scratch (cfg 5 needs 8.7 GB)


def release_attn_scratch():
    """Frees the persistent scratch of the attention backward (dS spill of the five-product form, delta / lse rows): call it when a
    process goes from training to inference and wants the HBM back.  The next backward re-allocates what it needs."""
    _spill_cache.clear()
    _delta_cache.clear()


def _spill_ws(B, S, H, device):
    """dS scratch of the five-product attention backward (4.4 GB at cfg 3, 8.7 GB at cfg 5; O(B H S^2)): ONE grow-only buffer per
    (device, stream), shared by every layer (launches on one stream are ordered).  Returns None - the caller then runs the
    seven-product form, which needs no scratch - when the size exceeds ATTN_SPILL_MAX_BYTES (env MH_ATTN_SPILL_MAX_GB, default 12), exceeds a
    quarter of the HBM that is free right now, cannot be allocated (OOM), or a graph capture is in progress.  `release_attn_scratch()` frees it."""
    need = int(L.lib().mh_attn_bwd_spill_bytes(B, S, H))
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _spill_cache.get(key)
    if ws is None or ws.numel() < need:
        if torch.cuda.is_current_stream_capturing() or need > ATTN_SPILL_MAX_BYTES:
            return None
        have = 0 if ws is None else ws.numel()
        free_b = torch.cuda.mem_get_info(device)[0] + torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
        if need - have > free_b // 4:
            return None
        if len(_spill_cache) > 4:
            _spill_cache.clear()
        _spill_cache.pop(key, None)
        del ws
        try:
            ws = _spill_cache[key] = torch.empty(need, dtype=torch.uint8, device=device)
        except torch.cuda.OutOfMemoryError:
            return None
    return ws


def attn_bwd2(q, k, v, o, do, lse, B, S, H, D, causal, seqlens=None, dq=None, dk=None, dv=None, rope=None, spill=None):
    """Backward without re-layout passes (transpose-read kernels).  rope = (cos, sin) table: dq and dk leave the kernels already rotated
    back (inverse RoPE fused into the epilogues: gradients w.r.t. the UN-rotated q, k).  spill (None = ATTN_BWD_SPILL): the causal D = 128
    case with S % 128 == 0 and no ragged lengths runs as FIVE products - the dK|dV kernel spills dS into a scratch buffer, dQ = dS K."""
    dq = torch.empty(B * S, H * D, dtype=q.dtype, device=q.device) if dq is None else dq
    dk = torch.empty(B * S, H * D, dtype=q.dtype, device=q.device) if dk is None else dk
    dv = torch.empty(B * S, H * D, dtype=q.dtype, device=q.device) if dv is None else dv
    delta = _delta_ws(B, H, S, q.device)  # [delta | lse*log2e]
    use_spill = ATTN_BWD_SPILL if spill is None else spill
    # (the dS spill lives in attn_bwd3_kv_k = fused-kv mode 2; in modes 0 / 1 the library would run the seven-product kernels and ignore ds_ws)
    use_spill = use_spill and causal and D == 128 and S % 128 == 0 and seqlens is None and int(L.lib().mh_attn_bwd_fused_kv_mode()) == 2
    ws = _spill_ws(B, S, H, q.device) if use_spill else None
    global LAST_ATTN_BWD_FORM
    if causal and D == 128:
        LAST_ATTN_BWD_FORM = "five-product" if ws is not None else "seven-product"  # (tests: which form the last causal D = 128 call took)
    if ws is not None:
        L.call("mh_attn_bwd2_spill", q, q.stride(0), k, k.stride(0), v, v.stride(0), o, o.stride(0), do, do.stride(0), lse, delta, dq, dq.stride(0), dk,
               dk.stride(0), dv, dv.stride(0), seqlens, B, S, H, D, int(causal), rope, dt_of(q), ws, _stream())
        return dq, dk, dv
    L.call("mh_attn_bwd2", q, q.stride(0), k, k.stride(0), v, v.stride(0), o, o.stride(0), do, do.stride(0), lse, delta, dq, dq.stride(0), dk, dk.stride(0), dv,
           dv.stride(0), seqlens, B, S, H, D, int(causal), rope, dt_of(q), _stream())
    return dq, dk, dv


def im2col_patches(pixels, ps, kpad, dtype, rows_per_img=None, row0=0, out=None):
    """pixels [N,3,H,H] -> cols [N*rows_per_img, kpad]; patch p of image n at row n*rows_per_img + row0 + p, rows below
    row0 (the CLS slot) zero.  `out`: write into a caller-provided row range (one launch per image tensor of a batch)."""
    N, Cc, Himg, Wimg = pixels.shape
    assert Cc == 3 and Himg == Wimg and pixels.is_contiguous()
    G = Himg // ps
    rpi = G * G + row0 if rows_per_img is None else rows_per_img
    cols = torch.empty(N * rpi, kpad, dtype=dtype, device=pixels.device) if out is None else out
    assert cols.shape == (N * rpi, kpad) and cols.is_contiguous()
    L.call("mh_im2col_patches", pixels, dt_of(pixels), cols, N, Himg, ps, kpad, rpi, row0, dt_of(dtype), _stream())
    return cols


def copy2d(src, dst, accumulate=False):
    """dst[r, c] (=|+=) src[r, c] over src's [rows, cols] block; both row-major 16-bit with their own row strides."""
    rows, cols = src.shape
    assert dst.shape[0] >= rows and dst.shape[1] >= cols and src.dtype == dst.dtype
    L.call("mh_copy2d", src, _rowmajor(src), dst, _rowmajor(dst), rows, cols, int(accumulate), dt_of(src), _stream())
    return dst


def select_tokens(logits, V=None, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=0, step=0, return_u=False, min_p=None, epsilon_cutoff=0.0):
    """logits fp32 [R, >=V] -> next token ids int64 [R]: greedy argmax, or temperature / top-k / top-p multinomial with a
    counter-based uniform per (seed, step, row) (include/merlin_hip.h: mh_select_tokens).  min_p (not None) / epsilon_cutoff (not 0): the two
    warpers behind top-p (mh_select_tokens_warp); at their defaults the launch is mh_select_tokens."""
    R = logits.shape[0]
    V = logits.shape[1] if V is None else V
    assert logits.dtype == torch.float32 and logits.stride(1) == 1
    out = torch.empty(R, dtype=torch.int64, device=logits.device)
    u = torch.empty(R, dtype=torch.float32, device=logits.device) if return_u else None
    if min_p is not None or epsilon_cutoff:
        L.call("mh_select_tokens_warp", logits, logits.stride(0), R, V, int(do_sample), temperature, top_k, top_p, float(min_p or 0.0),
               float(epsilon_cutoff or 0.0), seed & 0xFFFFFFFFFFFFFFFF, step, out, u, _stream())
    else:
        L.call("mh_select_tokens", logits, logits.stride(0), R, V, int(do_sample), temperature, top_k, top_p, seed & 0xFFFFFFFFFFFFFFFF, step, out, u, _stream())
    return (out, u) if return_u else out


def log_softmax_rows(logits, V=None, row_bias=None):
    """log_softmax over the first V columns of every row (+ row_bias[r]): fp32 [R, V]."""
    R = logits.shape[0]
    V = logits.shape[1] if V is None else V
    assert logits.dtype == torch.float32 and logits.stride(1) == 1
    out = torch.empty(R, V, dtype=torch.float32, device=logits.device)
    L.call("mh_log_softmax_rows", logits, logits.stride(0), R, V, out, V, row_bias, _stream())
    return out


def guidance_mix(cond, uncond, scale, V=None, out=None):
    """Classifier-free guidance (mh_guidance_mix; generation._guided_ref is its restatement): cond, uncond fp32 [R, >=V] (finite raw logits;
    any row strides - two tensors, or strided views of one buffer) -> out[r, :V] = lu + scale * (lc - lu), lc / lu = log_softmax of the two
    rows.  out: None (a new [R, V] tensor), `cond` itself (in place) or a third fp32 [R, >=V] buffer; columns >= V and uncond are not
    written."""
    R = cond.shape[0]
    V = cond.shape[1] if V is None else V
    assert cond.dtype == uncond.dtype == torch.float32 and cond.dim() == uncond.dim() == 2 and cond.stride(1) == uncond.stride(1) == 1
    assert uncond.shape[0] == R and cond.shape[1] >= V and uncond.shape[1] >= V and cond.device == uncond.device
    out = torch.empty(R, V, dtype=torch.float32, device=cond.device) if out is None else out
    assert out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] == R and out.shape[1] >= V and out.device == cond.device
    L.call("mh_guidance_mix", cond, cond.stride(0), uncond, uncond.stride(0), R, V, float(scale), out, out.stride(0), _stream())
    return out


def token_logprobs(logits, targets, V=None, logprob=None, greedy=None):
    """logits fp32 [R, >=V], targets int64 [R] on the device -> (log_softmax(logits[r, :V])[targets[r]] fp32 [R], targets[r] is the lowest
    index of row r's maximum, int32 [R]) without a [R, V] log-softmax (mh_token_logprobs).  A target outside [0, V): NaN and 0.
    logits may be one row expanded to R (row stride 0): R targets on the same distribution."""
    R = logits.shape[0]
    V = logits.shape[1] if V is None else V
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and targets.dtype == torch.int64 and targets.shape == (R,) and targets.is_contiguous()
    logprob = torch.empty(R, dtype=torch.float32, device=logits.device) if logprob is None else logprob
    greedy = torch.empty(R, dtype=torch.int32, device=logits.device) if greedy is None else greedy
    assert logprob.shape == greedy.shape == (R,) and logprob.dtype == torch.float32 and greedy.dtype == torch.int32
    assert logprob.is_contiguous() and greedy.is_contiguous()
    L.call("mh_token_logprobs", logits, logits.stride(0), R, V, targets, logprob, greedy, _stream())
    return logprob, greedy


def gather_rows2d(src, idx, dst, cols=None):
    """dst[i, :cols] = src[idx[i], :cols] for row-major 2-D views (own row strides); idx int64 on the device."""
    assert src.dim() == 2 and dst.dim() == 2 and src.stride(1) == 1 and dst.stride(1) == 1 and idx.dtype == torch.int64
    cols = src.shape[1] if cols is None else cols
    es = src.element_size()
    L.call("mh_gather_rows2d", src, src.stride(0) * es, idx, dst, dst.stride(0) * es, idx.numel(), cols * es, _stream())
    return dst


def gather_rows(table, idx, out=None):
    """out[i, :] = table[idx[i], :] (idx int64 on the device): the embedding-gather kernel without a splice table."""
    assert idx.dtype == torch.int64 and table.is_contiguous()
    return embed_splice_fwd(idx.contiguous().view(-1), None, table, None, out=out)


def vit_assemble(patch, cls, pos, N, G2):
    d = patch.shape[1]
    x = torch.empty(N * (G2 + 1), d, dtype=patch.dtype, device=patch.device)
    L.call("mh_vit_assemble", patch, cls, pos, x, N, G2, d, dt_of(patch), _stream())
    return x


def conv3x3_cols(x, N, G, C, stride, rows_per_img, row0):
    Go = (G + 2 - 3) // stride + 1
    cols = torch.empty(N * Go * Go, C * 9, dtype=x.dtype, device=x.device)
    L.call("mh_conv3x3_cols", x, cols, N, G, C, stride, rows_per_img, row0, _stream())
    return cols


def conv3x3_col2im(dcols, N, G, C, stride, rows_per_img, row0):
    dx = torch.empty(N * rows_per_img, C, dtype=dcols.dtype, device=dcols.device)
    L.call("mh_conv3x3_col2im", dcols, dx, N, G, C, stride, rows_per_img, row0, dt_of(dcols), _stream())
    return dx


def splice_index(ids, img_offset, P, im_patch, im_start, im_end, err, rows_per_img=None, row0=0):
    B, S = ids.shape
    assert ids.dtype == torch.int64 and ids.is_contiguous()
    src = torch.empty(B, S, dtype=torch.int32, device=ids.device)
    L.call("mh_splice_index", ids, img_offset, src, err, B, S, P, im_patch, im_start, im_end, P if rows_per_img is None else rows_per_img, row0, _stream())
    return src


def mask_lens(mask):
    B, S = mask.shape
    assert mask.is_contiguous() and mask.element_size() == 1
    lens = torch.empty(B, dtype=torch.int32, device=mask.device)
    L.call("mh_mask_lens", mask, lens, B, S, _stream())
    return lens


def norm_fwd_f32in(x32, w, eps, b=None, want_x16=False):
    """Reader of the fp32 residual stream: (y, x16 | None) = (norm(x32) in w's 16-bit dtype, 16-bit copy of x32).  b = None: RMSNorm,
    else LayerNorm.  include/merlin_hip.h: mh_norm_fwd_f32in."""
    rows, d = x32.shape
    assert x32.dtype == torch.float32 and x32.is_contiguous() and w.numel() == d
    y = torch.empty(rows, d, dtype=w.dtype, device=x32.device)
    x16 = torch.empty(rows, d, dtype=w.dtype, device=x32.device) if want_x16 else None
    L.call("mh_norm_fwd_f32in", x32, w, b, y, x16, rows, d, eps, dt_of(w), _stream())
    return y, x16


def vit_assemble_f32(patch32, cls, pos, N, G2):
    """fp32 form of vit_assemble: patch32 = the patch projection's fp32 output [N * (G2 + 1), d]; returns fp32 x."""
    d = patch32.shape[1]
    assert patch32.dtype == torch.float32 and patch32.is_contiguous()
    x = torch.empty(N * (G2 + 1), d, dtype=torch.float32, device=patch32.device)
    L.call("mh_vit_assemble_f32", patch32, cls, pos, x, N, G2, d, dt_of(cls), _stream())
    return x


def layernorm_f32_to_f32(x32, w, b, eps, want_x16=False):
    """(y32, x16 | None) = (LayerNorm(x32) in fp32, 16-bit copy of x32): the CLIP tower's pre_layrnorm at the start of the fp32 stream."""
    rows, d = x32.shape
    assert x32.dtype == torch.float32 and x32.is_contiguous()
    y = torch.empty(rows, d, dtype=torch.float32, device=x32.device)
    x16 = torch.empty(rows, d, dtype=w.dtype, device=x32.device) if want_x16 else None
    L.call("mh_layernorm_f32_to_f32", x32, w, b, y, x16, rows, d, eps, dt_of(w), _stream())
    return y, x16


def embed_splice_fwd_f32(ids, src, embed, feats32):
    """fp32 form of embed_splice_fwd: embedding rows widened, image rows taken from the projector's fp32 output."""
    T = ids.numel()
    d = embed.shape[1]
    assert feats32 is None or (feats32.dtype == torch.float32 and feats32.is_contiguous())
    out = torch.empty(T, d, dtype=torch.float32, device=embed.device)
    L.call("mh_embed_splice_fwd_f32", ids, src, embed, feats32, out, T, d, dt_of(embed), _stream())
    return out


def mask_unpad_index(mask):
    """bool/uint8 mask [B, S] -> (fwd int64 [B*S], inv int64 [B*S], count int32 [B]): the unpad / pad row tables of the key-padding
    attention branch (include/merlin_hip.h: mh_mask_unpad_index), consumed by gather_rows2d."""
    B, S = mask.shape
    assert mask.is_contiguous() and mask.element_size() == 1
    fwd = torch.empty(B * S, dtype=torch.int64, device=mask.device)
    inv = torch.empty(B * S, dtype=torch.int64, device=mask.device)
    cnt = torch.empty(B, dtype=torch.int32, device=mask.device)
    L.call("mh_mask_unpad_index", mask, fwd, inv, cnt, B, S, _stream())
    return fwd, inv, cnt


def check_inputs(ids, labels, mask, lens, err, V):
    """Device-side validation (ids / labels in range, right-padded mask, padding present at all); flags land in err[4:11] (int32[12])."""
    ref = ids if ids is not None else (labels if labels is not None else mask)
    B, S = ref.shape
    assert err.numel() >= 12 and err.dtype == torch.int32
    L.call("mh_check_inputs", ids, labels, mask, lens, err, B, S, V, _stream())


def embed_splice_fwd(ids, src, embed, feats, out=None):
    T = ids.numel()
    d = embed.shape[1]
    out = torch.empty(T, d, dtype=embed.dtype, device=embed.device) if out is None else out
    L.call("mh_embed_splice_fwd", ids, src, embed, feats, out, T, d, dt_of(embed), _stream())
    return out


def embed_splice_bwd(ids, src, dout, dfeats, dembed32):
    T, d = dout.shape
    L.call("mh_embed_splice_bwd", ids, src, dout, dfeats, dembed32, T, d, dt_of(dout), _stream())


def ce_fwd(logits, labels, V):
    """logits fp32 [B*S, ldl]; labels int64 [B, S].  Returns (row_loss[T], lse[T], out2[2])."""
    B, S = labels.shape
    T = B * S
    row_loss = torch.empty(T, dtype=torch.float32, device=logits.device)
    lse = torch.empty(T, dtype=torch.float32, device=logits.device)
    out2 = torch.empty(4, dtype=torch.float32, device=logits.device)
    L.call("mh_ce_fwd", logits, logits.stride(0), labels, row_loss, lse, out2, B, S, V, _stream())
    return row_loss, lse, out2


def ce_bwd(logits, labels, lse, out2, V, Vpad, gscale, dtype, out=None):
    B, S = labels.shape
    T = B * S
    out = torch.empty(T, Vpad, dtype=dtype, device=logits.device) if out is None else out
    L.call("mh_ce_bwd", logits, logits.stride(0), labels, lse, out2, out, out.stride(0), B, S, V, Vpad, gscale, dt_of(dtype), _stream())
    return out


def ce_bwd_rows(logits, labels, lse, out2, rows, V, Vpad, gscale, dtype):
    """Compact form of ce_bwd: row r of the result is the gradient of logits row rows[r] (int64 flat positions, < 0: a zero row)."""
    S = labels.shape[1]
    n = rows.numel()
    out = torch.empty(n, Vpad, dtype=dtype, device=logits.device)
    L.call("mh_ce_bwd_rows", logits, logits.stride(0), labels, lse, out2, out, out.stride(0), rows, n, S, V, Vpad, gscale, dt_of(dtype), _stream())
    return out


def adamw_(param, grad, m, v, lr, beta1, beta2, eps, wd, step, gscale=1.0):
    L.call("mh_adamw", param, grad, m, v, param.numel(), lr, beta1, beta2, eps, wd, step, gscale, dt_of(param), _stream())


def adamw_clip_(param, grad, m, v, lr, beta1, beta2, eps, wd, step, gscale, gscale_dev):
    L.call("mh_adamw_clip", param, grad, m, v, param.numel(), lr, beta1, beta2, eps, wd, step, gscale, gscale_dev, dt_of(param), _stream())


def adamw_split_(param, lo, grad, m, v, lr, beta1, beta2, eps, wd, step, gscale=1.0, gscale_dev=None):
    """AdamW on the fp32 master (param << 16) + lo (lo: int16, same length); param and lo are both rewritten (include/merlin_hip.h)."""
    L.call("mh_adamw_split", param, lo, grad, m, v, param.numel(), lr, beta1, beta2, eps, wd, step, gscale, gscale_dev, dt_of(param), _stream())


def adamw_sr_(param, grad, m, v, lr, beta1, beta2, eps, wd, step, gscale=1.0, gscale_dev=None, key=0, index0=0):
    """AdamW with a stochastically rounded store of param: element i draws from splitmix64(key + ((index0 + i) >> 2))."""
    L.call("mh_adamw_sr", param, grad, m, v, param.numel(), lr, beta1, beta2, eps, wd, step, gscale, gscale_dev, key, index0, dt_of(param), _stream())


P_MODES = {"nearest": 0, "split": 1, "stochastic": 2}  # mh_adamw_compact's p_mode


def adamw_compact_(param, lo, grad, m8, mscale, v16, lr, beta1, beta2, eps, wd, step, gscale=1.0, gscale_dev=None, p_mode=0, p_key=0, state_key=0,
                   index0=0):
    """AdamW on compact moments (include/merlin_hip.h): m8 e4m3 bytes [n] with one scale byte per 128 elements in mscale, v16 bf16 [n], all
    rewritten with stochastic rounding drawn from (state_key, index0 + i); param (and lo, p_mode 1) as adamw_ / adamw_split_ / adamw_sr_ store
    it.  index0 is a multiple of 128 and the slices start on that block."""
    L.call("mh_adamw_compact", param, lo, grad, m8, mscale, v16, param.numel(), lr, beta1, beta2, eps, wd, step, gscale, gscale_dev, p_mode, p_key,
           state_key, index0, dt_of(param), _stream())


def adamw_states_pack(m32, v32, m8, mscale, v16, state_key=0, index0=0):
    """fp32 moments -> the compact form, by the store rule of adamw_compact_."""
    L.call("mh_adamw_states_pack", m32, v32, m8, mscale, v16, m32.numel(), state_key, index0, _stream())


def adamw_states_unpack(m8, mscale, v16, m32=None, v32=None):
    """Compact moments -> fp32 (m, v), exact."""
    n = m8.numel()
    m32 = torch.empty(n, dtype=torch.float32, device=m8.device) if m32 is None else m32
    v32 = torch.empty(n, dtype=torch.float32, device=m8.device) if v32 is None else v32
    L.call("mh_adamw_states_unpack", m8, mscale, v16, m32, v32, n, _stream())
    return m32, v32


def clip_scale(sumsq_t, gscale, max_norm, out2):
    L.call("mh_clip_scale", sumsq_t, gscale, max_norm, out2, _stream())


def sumsq_det(g, partial, out):
    L.call("mh_sumsq_det", g, g.numel(), partial, out, dt_of(g), _stream())


def any_nonzero(g, flag):
    """flag (int32[1], zeroed by the caller) |= 1 when any 16-bit element of g is non-zero (exact, on the bit patterns)."""
    L.call("mh_any_nonzero", g, g.numel(), flag, _stream())


def sumsq(g, out):
    L.call("mh_sumsq", g, g.numel(), out, dt_of(g), _stream())


_gemv_mfma_min = 3


def gemv_mfma_min_rows(rows: int):
    """A/B switch: row count from which gemv / gemv_fp8w / gemv_fp4w use the MFMA kernel (<= 0 restores the measured default, 3; 17 = never)."""
    global _gemv_mfma_min
    _gemv_mfma_min = rows if rows > 0 else 3
    L.lib().mh_gemv_mfma_min_rows(rows)


def gemv_mfma_pair_min_rows(rows16: int, rows_fp8: int):
    """A/B switch: row counts from which the SwiGLU / RoPE-append projections use the MFMA form (<= 0: defaults 6 / 4)."""
    L.lib().mh_gemv_mfma_pair_min_rows(rows16, rows_fp8)


def _gemv_rows_per_launch(K):
    """Activation rows one mh_gemv / mh_gemv_fp8w launch takes: 16 through the MFMA form (needs K % 32 == 0 and the MFMA row
    threshold within reach), 8 through the wave-per-row form otherwise (csrc/decode.hip gemv_impl returns MH_ERR_ARG for 9-16
    rows there: e.g. beam search with 9-16 beam rows on a model whose K is a multiple of 8 but not of 32)."""
    return 16 if (K % 32 == 0 and _gemv_mfma_min <= 9) else 8


def _gemv_fused_rows_ok(M, K):
    """Rows the fused decode projections (SwiGLU / RoPE epilogues) take in one launch: 8 as one wave per row pair, 16 in the MFMA form."""
    return M <= 8 or (M <= 16 and M >= _gemv_mfma_min and K % 64 == 0)


def gemv_ksplit(on: bool):
    """A/B switch: K split over a block's waves in the 1-2 row GEMV at N <= 8192 (default on)."""
    L.lib().mh_gemv_ksplit(1 if on else 0)


def gemv_mfma_wide(on: bool):
    """A/B switch: 16 instead of 8 waves per block in the MFMA GEMV at N <= 8192 (default on)."""
    L.lib().mh_gemv_mfma_wide(1 if on else 0)


def attn_fwd_pingpong(on):
    """A/B switch of the D = 128 attention forward: 0 / False = attn_fwd2 (default), 1 / True = the ping-pong form (8-wave blocks, SIMD partners in
    opposite phases; csrc/attn_fwd3.hip), 2 = one wave per SIMD with 64 query rows per wave (csrc/attn_fwd4.hip)."""
    L.lib().mh_attn_fwd_pingpong(int(on))


def attn_bwd_fused_kv(on):
    """A/B switch for dK and dV of the D = 128 attention backward: True / 2 = attn_bwd3_kv_k (default: one kernel, register-staged copies,
    continuous fragment stream), 1 = attn_bwd2_kv_k<MODE 3> (one kernel, LDS-DMA copies: rounds 2-4), False / 0 = two kernels."""
    L.lib().mh_attn_bwd_fused_kv(2 if on is True else int(on))


def attn_wide_stores(on: bool):
    """A/B switch: the row-per-lane epilogues of the attention kernels write 16 bytes per lane (default) or 8; bit-identical results."""
    L.lib().mh_attn_wide_stores(1 if on else 0)


def gemm_raster_group(gm: int):
    """A/B switch: tile rows per raster group of the MFMA GEMM kernels (1..64; default 0 = automatic: every tile row when there are at most 8, else 4; out of range = automatic)."""
    L.lib().mh_gemm_raster_group(gm)


def gemm_persistent(on: bool):
    """A/B switch: persistent launch of the 256-tile GEMM kernels (default on; env MH_GEMM_PERSISTENT=0 turns it off at import)."""
    L.lib().mh_gemm_persistent(1 if on else 0)


def gemm_w4_policy(mask: int):
    """A/B switch: operand layouts the auto selection sends to the 4-wave 256x256 GEMM (bit 0 TN, bit 1 NN, bit 2 NT, bit 3 fp8 NT; default 11)."""
    L.lib().mh_gemm_w4_policy(mask)


def gemm_w4_half(mode: int):
    """128-row block tiles of the 4-wave GEMM for NT products with few rows (short prefills): 0 = never, 1 = auto (default), 2 = wherever the form exists."""
    L.lib().mh_gemm_w4_half(mode)


def gemm_force_kernel(which: int):
    """0 = auto, 128 / 256 = force that tile size (tests, A/B benchmarks).  Other codes select the development arms and
    exist only in the dev library (tools/dev_arms/)."""
    L.lib().mh_gemm_force_kernel(which)
