"""The fp8 KV-cache format (include/merlin_hip.h "fp8 KV cache") restated in torch, and the properties that make it exact:
K / V rows as OCP e4m3 bytes with one power-of-two fp32 scale per group of D channels.  tests/test_kv8_gpu.py holds the kernels to this
restatement bit for bit."""
import pytest
import torch

DTYPES = [torch.bfloat16, torch.float16]


def kv8_quantize(x):
    """x [..., D] (16-bit or fp32) -> (e4m3 bytes uint8 [..., D], scale fp32 [...]): scale = 2^e, e the smallest integer with
    amax * 2^-e <= 448 (amax = m * 2^ex, m in [0.5, 1): e = ex - 9 if m <= 0.875 else ex - 8), clamped to [-126, 127], 0 for an
    all-zero group; byte = e4m3_rne(x * 2^-e)."""
    xf = x.float()
    amax = xf.abs().amax(-1)
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.875, ex - 9, ex - 8).clamp(-126, 127)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    scale = torch.ldexp(torch.ones_like(amax), e)
    q = torch.ldexp(xf, -e[..., None]).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale


def kv8_dequantize(q, scale, dtype=torch.float64):
    """byte * scale, exact in fp64 (and in fp32)."""
    return q.view(torch.float8_e4m3fn).float().to(dtype) * scale.to(dtype)[..., None]


def rows_with_maxima(n, D, dtype, lo=1e-2, hi=30.0, seed=0):
    """n random rows whose maxima are spread log-uniformly over [lo, hi] (first and last row pinned to the ends), plus an all-zero row."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, D, generator=g)
    x = x / x.abs().amax(-1, keepdim=True)
    mag = torch.exp(torch.linspace(torch.log(torch.tensor(lo)).item(), torch.log(torch.tensor(hi)).item(), n))
    x = (x * mag[:, None]).to(dtype)
    x[n // 2] = 0
    return x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
def test_format_properties(dtype, D):
    x = rows_with_maxima(513, D, dtype, seed=D)
    q, scale = kv8_quantize(x)
    zero = x.float().abs().amax(-1) == 0
    assert int(zero.sum()) == 1 and bool((scale[zero] == 1).all()) and bool((q[zero] == 0).all())  # all-zero group: e = 0, zero bytes
    m, _ = torch.frexp(scale)
    assert bool((m == 0.5).all()), "a scale is not a power of two"
    smax = x.float().abs().amax(-1) / scale  # exact: a power-of-two division
    assert bool(((smax > 224) & (smax <= 448))[~zero].all()), (float(smax[~zero].min()), float(smax[~zero].max()))
    assert not bool(((q & 0x7F) == 0x7F).any()), "NaN byte"
    deq = kv8_dequantize(q, scale)
    assert torch.equal(deq.to(dtype).double(), deq), "dequantised values do not survive the 16-bit type"
    # an element moves by at most half an e4m3 step: 16 where the scaled maximum is in (256, 448], 8 where it is in (224, 256]
    err = (deq - x.double()).abs().amax(-1)
    assert bool((err <= x.double().abs().amax(-1) / 16).all())


def test_exponent_rule_at_the_edges():
    """amax exactly 448 * 2^k keeps e = k; one ulp more moves to k + 1; tiny and huge maxima clamp."""
    for k in (-20, -3, 0, 5):
        a = torch.tensor([[448.0 * 2.0 ** k, 0.0]])
        assert float(kv8_quantize(a)[1]) == 2.0 ** k
        b = torch.nextafter(a, torch.tensor(float("inf")))
        assert float(kv8_quantize(b)[1]) == 2.0 ** (k + 1)
    assert float(kv8_quantize(torch.tensor([[2.0 ** -140, 0.0]]))[1]) == 2.0 ** -126
    q, s = kv8_quantize(torch.tensor([[1.0, -0.4]]))
    assert float(s) == 2.0 ** -8 and torch.equal(kv8_dequantize(q, s), torch.tensor([[1.0, -0.40625]], dtype=torch.float64))


def test_fp8_kv_needs_the_cache():
    """generate(use_cache=False, fp8_kv=True) is refused before the model or the device is touched."""
    from merlin_amd import generation as G

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"model.{name} read before the arguments were checked")

    with pytest.raises(ValueError, match="fp8_kv"):
        G.generate(Untouchable(), torch.zeros(1, 4, dtype=torch.int64), use_cache=False, fp8_kv=True, max_new_tokens=2)
