"""The MXFP4 weight format restated in torch (tests/numerics_fp4.py) and the properties that make the fp4 decode path "the 16-bit path on
weights rounded to a grid": the exponent rule against brute force, idempotence, dequantised values exact in both 16-bit types, the tie table.
tests/test_fp4_gpu.py holds the kernels to this restatement bit for bit."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import numerics_fp4 as F4  # noqa: E402

DTYPES = [torch.bfloat16, torch.float16]
NEW_SYMBOLS = ["mh_quant_fp4_b32", "mh_gemv_fp4w", "mh_gemv_fp4w_norm", "mh_gemv_fp4w_qkv_rope"]


def weights(n, K, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, K, generator=g) * 0.02).to(dtype)


def test_exponent_rule_against_brute_force():
    """Every bf16 magnitude of the binades [2^-4, 2^4), of the lowest normal ones and of the subnormals: e is the smallest integer with
    amax 2^-e <= 6, clamped to >= -126."""
    bits = torch.cat([torch.arange((127 - 4) << 7, (127 + 4) << 7), torch.arange(1, 4 << 7)]).to(torch.int16)
    amax = bits.view(torch.bfloat16).double()
    e = F4.block_exponent(amax.float()).long()
    want = torch.empty_like(e)
    for i, a in enumerate(amax.tolist()):
        k = -160
        while a * 2.0 ** -k > 6.0:
            k += 1
        want[i] = max(k, -126)
    assert torch.equal(e, want)
    assert int(F4.block_exponent(torch.zeros(1))) == 0
    assert int(F4.block_exponent(torch.tensor([2.0 ** -130]))) == -126
    big = torch.tensor([torch.finfo(torch.bfloat16).max])
    assert int(F4.block_exponent(big)) == 126 and float(big) * 2.0 ** -126 <= 6.0 < float(big) * 2.0 ** -125


def test_tie_table():
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], dtype=torch.float64)
    to = torch.tensor([0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0], dtype=torch.float64)
    mags = torch.tensor(F4.MAGNITUDES, dtype=torch.float64)
    assert torch.equal(mags[F4.round_e2m1(ties)], to)
    assert torch.equal(mags[F4.round_e2m1(mags)], mags)
    eps = 2.0 ** -10
    assert torch.equal(mags[F4.round_e2m1(ties + eps)], torch.tensor([0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64))
    assert torch.equal(mags[F4.round_e2m1(ties - eps)], torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0], dtype=torch.float64))
    # through the quantiser, at a block scale of 2^-5 (the block's maximum 6 * 2^-5 keeps e = -5), both signs
    for dtype in DTYPES:
        w = torch.zeros(2, 32, dtype=torch.float64)
        w[0, :7], w[1, :7], w[:, 31] = ties, -ties, 6.0
        q, s = F4.quant((w * 2.0 ** -5).to(dtype))
        assert s.tolist() == [[122], [122]]
        d = F4.dequant(q, s) * 2.0 ** 5
        assert torch.equal(d[0, :7], to) and torch.equal(d[1, :7], -to)


@pytest.mark.parametrize("dtype", DTYPES)
def test_idempotent_and_exact_in_16_bits(dtype):
    w = weights(96, 256, dtype)
    w[3] = 0
    w[5, 32:64] = 0
    q, s = F4.quant(w)
    assert int(s[3].min()) == int(s[3].max()) == int(s[5, 1]) == 127 and int((q[3] & 0x77).max()) == 0
    d = F4.dequant(q, s)
    assert torch.equal(d.to(dtype).double(), d), "dequantised values do not survive the 16-bit type"
    q2, s2 = F4.quant(d.to(dtype))
    assert torch.equal(F4.dequant(q2, s2), d)
    nz = w.double().view(96, 8, 32).abs().amax(-1) > 0
    smax = (w.double().view(96, 8, 32).abs().amax(-1) / F4.scales64(s))[nz]
    assert bool(((smax > 3) & (smax <= 6)).all()), (float(smax.min()), float(smax.max()))
    # an element moves by at most half a grid step: 1 where the scaled value is in [4, 6], i.e. at most amax / 6 ... amax / 3
    err = (d - w.double()).view(96, 8, 32).abs().amax(-1)
    assert bool((err <= F4.scales64(s)).all())
    rel = float((d - w.double()).pow(2).sum().sqrt() / w.double().pow(2).sum().sqrt())
    assert 0.08 < rel < 0.16, rel  # ~12 % relative rms on normal weights


def test_header_declares_and_library_exports_the_fp4_symbols():
    from merlin_amd import _lib as L

    names = L.declared_symbols()
    assert all(n in names and n in L.PROTOTYPES for n in NEW_SYMBOLS)
    if not os.path.exists(L.LIB_PATH):
        from merlin_amd.csrc import build

        build.build(verbose=False)
    lib = L.lib()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)


def test_generate_refuses_fp4_combinations_before_touching_the_model():
    from merlin_amd import generation as G

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"model.{name} read before the arguments were checked")

    ids = torch.zeros(1, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="fp4_weights"):
        G.generate(Untouchable(), ids, fp4_weights=True, fp8_weights=True, max_new_tokens=2)
    with pytest.raises(ValueError, match="use_cache"):
        G.generate(Untouchable(), ids, fp4_weights=True, use_cache=False, max_new_tokens=2)
