"""The compact AdamW moments behind FusedAdamW(states="compact"), without a GPU: the block scale rule at its edges, the exactness of the
decode, the two stochastic stores' probabilities by enumeration of every 16-bit field, the random fields, what the format costs on synthetic
gradient streams (tests/adamw_compact_ref.py's simulator), and the optimizer's host logic on a stub engine."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import adamw_compact_ref as C  # noqa: E402
import adamw_rounding_ref as R  # noqa: E402
from test_adamw_rounding_cpu import HP, _Engine  # noqa: E402

from merlin_amd import optim  # noqa: E402
from merlin_amd.weights import splitmix64_scalar  # noqa: E402

F32 = np.float32


def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(F32)


# ---- 1. the scale rule ------------------------------------------------------------------------------------------------------------------------
def test_scale_rule_at_its_edges():
    for e in (-126, -40, -1, 0, 1, 9, 119):
        top = F32(448.0) * F32(2.0) ** e  # exactly 448 * 2^e: mantissa 0.875 of 2^(e + 9)
        assert math.frexp(float(top))[0] == 0.875
        assert int(C.scale_exp(top)) == e
        assert int(C.scale_exp(np.nextafter(top, F32(np.inf)))) == e + 1  # just above: one more
        if e > -126:
            assert int(C.scale_exp(np.nextafter(top, F32(0)))) == e
            assert int(C.scale_exp(top / 2)) == e - 1 and int(C.scale_exp(np.nextafter(top / 2, F32(np.inf)))) == e
    assert int(C.scale_exp(F32(0))) == 0                                          # an all-zero block
    assert [int(C.scale_exp(x)) for x in _f32([1, 0x7FFFFF, 0x800000])] == [-126] * 3  # the floor: fp32 subnormals, the smallest normal
    assert int(C.scale_exp(F32(448.0) * F32(2.0) ** -127)) == -126
    assert int(C.scale_exp(np.finfo(F32).max)) == 120
    # the definition itself, on random maxima: e is the smallest integer with amax * 2^-e <= 448
    rng = np.random.default_rng(0)
    amax = (rng.uniform(0.5, 1, 4096) * 2.0 ** rng.integers(-140, 128, 4096)).astype(F32)
    amax = amax[amax > 0]
    e = C.scale_exp(amax)
    a = amax.astype(np.float64)
    assert bool((np.ldexp(a, -e) <= 448).all()) and bool(((np.ldexp(a, -(e - 1)) > 448) | (e == -126)).all())
    # in a block only the valid elements count, and the scale byte is e + 127
    m = np.zeros(200, F32)
    m[5], m[130] = 448 * 2.0 ** 3, -3e-5
    codes, scales = C.m_store(m, 1, 0)
    assert scales.tolist() == [3 + 127, int(C.scale_exp(F32(3e-5))) + 127] and codes[5] == 0x7E and (codes[130] & 0x80)
    assert C.m_store(np.zeros(128, F32), 1, 0)[1].tolist() == [127] and not C.m_store(np.zeros(128, F32), 1, 0)[0].any()


def test_never_a_code_above_448_and_the_decode_is_exact():
    assert C.E4M3[0x7E] == 448 and C.E4M3[8] == 2.0 ** -6 and C.E4M3[1] == 2.0 ** -9 and len(C.E4M3) == 127 and bool((np.diff(C.E4M3) > 0).all())
    rng = np.random.default_rng(1)
    n = 128 * 257 + 77
    m = (rng.standard_normal(n) * 10.0 ** rng.uniform(-12, 3, n)).astype(F32)
    m[:128] = _f32([3] * 128)          # a block of fp32 subnormals: e = -126
    m[128] = F32(448.0) * F32(2.0) ** 119  # the largest block maximum whose successors are still fp32 (above it hi * 2^120 can be 2^128)
    m[300:400] = 0
    for key in (0, 12345, 2 ** 64 - 1):
        codes, scales = C.m_store(m, key, 128 * 9)
        assert int((codes & 0x7F).max()) <= 0x7E and int(scales.min()) >= 1 and int(scales.max()) == 246
        back = C.m_decode(codes, scales)  # (asserts that code * 2^e is an fp32)
        again, scales2 = C.m_store(back, key ^ 5, 0)  # a value on the grid is stored as itself whatever the field
        keep = np.repeat(scales2 == scales, 128)[:n]  # (where rounding down emptied the top of a block its scale may drop)
        assert np.array_equal(C.m_decode(again, scales2), back) and keep.mean() > 0.9
        # every value lands on one of its two grid neighbours under the block's scale
        e = np.repeat(scales.astype(np.int64) - 127, 128)[:n]
        y = np.ldexp(np.abs(m.astype(np.float64)), -e)
        idx = np.searchsorted(C.E4M3, y.astype(F32).astype(np.float64), side="right") - 1
        got = (codes & 0x7F).astype(np.int64)
        assert bool(((got == idx) | (got == idx + 1)).all())
        assert np.array_equal(codes & 0x80, ((m.view(np.uint32) >> 24) & 0x80).astype(np.uint8))


# ---- 2. the two stores' probabilities, every field enumerated -----------------------------------------------------------------------------------
def test_m_store_rounds_up_with_probability_ceil_65536_t_over_65536():
    r = np.arange(65536)
    samples = [2.0 ** -9 * f for f in (0.0, 2.0 ** -20, 0.3, 0.999, 1.0, 1.5, 6.25, 7.0, 7.999)]      # the subnormal grid: spacing 2^-9
    for ex in range(-6, 9):                                                                            # every normal binade: spacing 2^(ex - 3)
        samples += [2.0 ** ex * f for f in (1.0, 1.0 + 2.0 ** -23, 1.03, 1.125, 1.2 - 2.0 ** -20, 1.5 + 2.0 ** -4, 1.74, 1.75, 1.99999)]
    checked = 0
    for y in samples:
        y = float(F32(y))
        if y > 448:
            continue
        lo = max(x for x in C.E4M3.tolist() if x <= y)
        hi = min([x for x in C.E4M3.tolist() if x > y], default=None)
        t = Fraction(0) if hi is None else (Fraction(y) - Fraction(lo)) / (Fraction(hi) - Fraction(lo))
        ups = math.ceil(65536 * t)
        assert t <= Fraction(ups, 65536) < t + Fraction(1, 65536)
        code = C.m_code(np.full(65536, y), r)
        lo_code = C.E4M3.tolist().index(lo)
        assert int((code == lo_code + 1).sum()) == ups and int((code == lo_code).sum()) == 65536 - ups, y
        assert bool((code[:ups] == lo_code + 1).all())  # up exactly for r_m < 65536 t
        checked += 1
    assert checked > 130


def test_v_store_rounds_up_with_exactly_the_dropped_fraction():
    r = np.arange(65536)
    for u in (0x3F800000, 0x3F800001, 0x3F808000, 0x3F80FFFF, 0x2F123456, 0x00000001, 0x0001FFFF, 0x7F7F0001, 0x007FFFFF):
        up = int((C.v_bits(np.full(65536, u), r) == (u >> 16) + 1).sum())
        assert up == (u & 0xFFFF) and int((C.v_bits(np.full(65536, u), r) == (u >> 16)).sum()) == 65536 - up
    assert C.v_bits(np.array([0x7F800000, 0x7FC0FFFF]), np.array([0xFFFF, 0xFFFF])).tolist() == [0x7F80, 0x7FC0]  # inf / nan are truncated
    v = np.array([1.0, 1.0 + 2.0 ** -9, 3e-12], F32)
    assert np.array_equal(C.v_decode(C.v_store(C.v_decode(C.v_store(v, 7, 0)), 8, 0)), C.v_decode(C.v_store(v, 7, 0)))  # a bf16 stays


def test_fields_are_a_function_of_key_and_arena_index_only():
    key = C.state_key(3, 17)
    rv, rm = C.state_fields(256, key, 128)
    for j in (128, 129, 200, 383):
        half = (splitmix64_scalar((key + (j >> 1)) & C.MASK64) >> (32 * (j & 1))) & 0xFFFFFFFF
        assert (int(rv[j - 128]), int(rm[j - 128])) == (half & 0xFFFF, half >> 16)
    for cut in (1, 2, 77, 128):  # however the arena is cut into launches
        a, b = C.state_fields(cut, key, 128), C.state_fields(256 - cut, key, 128 + cut)
        assert np.array_equal(np.concatenate([a[0], b[0]]), rv) and np.array_equal(np.concatenate([a[1], b[1]]), rm)
    assert not np.array_equal(C.state_fields(256, key + 1, 128)[0], rv)
    assert abs(float(rv.mean()) / 65536 - 0.5) < 0.1 and abs(float(rm.mean()) / 65536 - 0.5) < 0.1
    # another stream than the parameter store's, for every step
    assert all(C.state_key(s, t) != R.sr_key(s, t) for s in (0, 1, 7) for t in range(1, 200))
    assert len({C.state_key(0, t) for t in range(1, 200)}) == 199


# ---- 3. what the format costs: the simulator ---------------------------------------------------------------------------------------------------
def test_nearest_bf16_v_never_decays_and_the_stochastic_one_follows_fp32():
    g = C.stream(4096, 400, 2, 3, drop_at=100)  # the gradient drops by 1e3 at step 100 of 400
    near = C.simulate(g, m_mode="fp32", v_mode="nearest")
    sr = C.simulate(g, m_mode="fp32", v_mode="sr")
    want = near["v_mean"]
    assert want[-1] < 0.76 * want[98]                                    # fp32 v decays by 0.999^300 = 0.74
    assert near["vq_mean"][-1] == near["vq_mean"][99] > 0.99 * want[98]  # round to nearest: frozen where the drop found it
    # per element and step the stored v is off by less than one bf16 spacing (at most 2^-7 relative) with zero mean and variance <= 1/4 of a
    # spacing squared; the recurrence keeps a 1 / sqrt(1 - 0.999^2) = 22.4 step memory of it: 5 standard deviations of a mean over 4096 elements
    dev = float(np.abs(sr["v_rel"]).max())
    assert dev <= 5 * 2.0 ** -7 * 0.5 * 22.4 / math.sqrt(4096), dev
    assert abs(sr["vq_mean"][-1] / want[-1] - 1) < 0.01 < abs(near["vq_mean"][-1] / want[-1] - 1)


def test_simulated_cost_of_the_format_on_synthetic_streams():
    """The figures the format was chosen on: per step 7.5 - 7.9 % relative RMS against fp32 moments, accumulated over 400 steps 1.4 - 1.6 %
    (noise scales spread over 2 and over 5 decades within a tensor).  1.25 x guards this restatement against drift."""
    for decades in (2, 5):
        r = C.simulate(C.stream(128 * 64, 400, decades, 1))
        print(f"compact moments, {decades} decades: per step {r['step_rms']:.4f}, accumulated {r['acc_l1']:.4f} (L2 {r['acc_l2']:.4f})")
        assert 0.02 < r["step_rms"] <= 1.25 * 0.079, r["step_rms"]
        assert 0.004 < r["acc_l1"] <= 1.25 * 0.016, r["acc_l1"]
    only_m = C.simulate(C.stream(128 * 64, 100, 2, 1), v_mode="fp32")
    only_v = C.simulate(C.stream(128 * 64, 100, 2, 1), m_mode="fp32")
    assert only_v["step_rms"] < 0.3 * only_m["step_rms"]  # nearly all of it is m's 3 mantissa bits; v at 16 bits costs little


# ---- 4. host logic of FusedAdamW ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    log = []

    def adamw_compact_(p, lo, g, m8, mscale, v16, lr, b1, b2, eps, wd, step, gscale=1.0, gdev=None, p_mode=0, p_key=0, state_key=0, index0=0):
        log.append(dict(p=p, lo=lo, g=g, m8=m8, mscale=mscale, v16=v16, step=step, gdev=gdev, p_mode=p_mode, p_key=p_key, state_key=state_key,
                        index0=index0, wd=wd))

    def sumsq_det(g, partial, out):
        out[0] = g.float().pow(2).sum()

    def clip_scale(ss, gscale, max_norm, out2):
        out2[0], out2[1] = 1.0, ss[0].sqrt()

    def refuse(*a, **k):
        raise AssertionError("a compact optimizer launched an fp32-moment kernel")

    for f in (adamw_compact_, sumsq_det, clip_scale):
        monkeypatch.setattr(optim.O, f.__name__, f, raising=True)  # (raising: the wrappers must exist in ops)
    for name in ("adamw_", "adamw_clip_", "adamw_split_", "adamw_sr_"):
        monkeypatch.setattr(optim.O, name, refuse, raising=True)
    return log


def test_option_validation(calls):
    with pytest.raises(ValueError, match="states"):
        optim.FusedAdamW(_Engine(), states="8bit", **HP)
    with pytest.raises(ValueError, match="rounding"):
        optim.FusedAdamW(_Engine(), states="compact", rounding="bankers", **HP)
    opt = optim.FusedAdamW(_Engine(torch.float16), states="compact", **HP)
    with pytest.raises(ValueError, match=r"compact.*float16"):
        opt.step()
    assert calls == [] and opt.state_bytes() == 0  # refused before any buffer or launch
    assert optim.FusedAdamW(_Engine(), **HP).states == "fp32" and optim.STATES == ("fp32", "compact")


@pytest.mark.parametrize("rounding", optim.ROUNDINGS)
def test_compact_dispatches_one_launch_per_run_on_block_aligned_slices(calls, rounding):
    eng = _Engine()
    A = eng.arena
    opt = optim.FusedAdamW(eng, states="compact", rounding=rounding, seed=7, **HP)
    opt.step()
    opt.step(max_grad_norm=1.0)
    assert opt.m is None and opt.v is None
    assert (opt.m8.dtype, opt.mscale.dtype, opt.v16.dtype) == (torch.uint8, torch.uint8, torch.bfloat16)
    assert opt.m8.numel() == opt.v16.numel() == A.total and opt.mscale.numel() == A.total // 128 and bool((opt.mscale == 127).all())
    assert opt.state_bytes() == 3 * A.total + A.total // 128 <= (3 + 1 / 128) * A.total + 128
    assert len(calls) == 2 * len(opt._runs) == 8
    for c, (off, num, _, wd) in zip(calls, opt._runs * 2):
        assert off % 128 == 0 and c["index0"] == off and c["wd"] == wd
        assert c["p"].data_ptr() == A.flat[off:].data_ptr() and c["g"].data_ptr() == A.gflat[off:].data_ptr() and c["p"].numel() == num
        assert c["m8"].data_ptr() == opt.m8[off:].data_ptr() and c["v16"].data_ptr() == opt.v16[off:].data_ptr()
        assert c["mscale"].data_ptr() == opt.mscale[off // 128:].data_ptr() and c["mscale"].numel() >= -(-num // 128)
        assert c["p_mode"] == optim.ROUNDINGS.index(rounding) == optim.O.P_MODES[rounding]
        assert c["state_key"] == opt.state_key(c["step"]) == C.state_key(7, c["step"])
        assert c["p_key"] == (R.sr_key(7, c["step"]) if rounding == "stochastic" else 0)
        assert (c["lo"] is not None) == (rounding == "split") and (c["lo"] is None or c["lo"].data_ptr() == opt.lo[off:].data_ptr())
        assert (c["gdev"] is not None) == (c["step"] == 2)
    assert [c["step"] for c in calls] == [1] * 4 + [2] * 4


def test_state_bytes_and_moments_of_the_default(monkeypatch):
    eng = _Engine()
    opt = optim.FusedAdamW(eng, **HP)
    monkeypatch.setattr(optim.O, "adamw_", lambda p, g, m, v, *a: (m.add_(1.0), v.add_(2.0)), raising=True)
    monkeypatch.setattr(optim.O, "adamw_compact_", lambda *a, **k: pytest.fail("the default launched the compact kernel"), raising=True)
    opt.step()
    assert opt.m8 is None and opt.state_bytes() == 8 * eng.arena.total
    m, v = opt.moments("b.weight")
    assert m.shape == v.shape == (4, 50) and m.dtype == v.dtype == torch.float32 and bool((m == 1).all()) and bool((v == 2).all())
    assert m.data_ptr() == opt.m[eng.arena.offset["b.weight"]:].data_ptr()  # views
