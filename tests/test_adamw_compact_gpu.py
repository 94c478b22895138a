"""mh_adamw_compact / mh_adamw_states_pack / mh_adamw_states_unpack and FusedAdamW(states="compact") on the device.  The arithmetic oracle is
the fp32-moment kernels of the same build run on the decoded moments (p', lo' bit-identical); the stored moments are compared bit for bit
with the integer restatement of tests/adamw_compact_ref.py applied to that oracle's fp32 m', v'.

Sizes: 1, 127, 128, 129 (below, at and just past one block), 1000 (a partial last block whose tail lanes are empty), 128 * 33 + 5 (more than
one 256-thread workgroup, 5 elements in the last block's first lane), each at arena index 0 and 128 * 7."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import adamw_compact_ref as C  # noqa: E402
import adamw_rounding_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
LR, WD = 5e-5, 0.05
B1, B2, EPS = 0.9, 0.999, 1e-8
SIZES = [1, 127, 128, 129, 1000, 128 * 33 + 5]
NEAREST, SPLIT, SR = 0, 1, 2


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from merlin_amd import ops as O

    assert O.arch_ok(0), "not a gfx950 device"
    return O


def _np(t):
    """Device tensor -> numpy, 16-bit types as their bit patterns (uint16)."""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype in (BF16, torch.int16) else t.numpy()


def _bf16(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(BF16).to(dev())


def _compact(m8, ms, v16):
    """numpy (m8, mscale, v16 bits) -> device tensors (uint8, uint8, bf16)."""
    return torch.from_numpy(m8).to(dev()), torch.from_numpy(ms).to(dev()), _bf16(v16)


def _random_moments(n, seed):
    """fp32 (m, v) with magnitudes spread over three decades inside every block, some exact zeros."""
    rng = np.random.default_rng(seed)
    mag = 1e-3 * 10.0 ** rng.uniform(-3, 0, n)
    m = (mag * rng.standard_normal(n)).astype(np.float32)
    v = ((mag * rng.standard_normal(n)) ** 2).astype(np.float32)
    m[rng.random(n) < 0.05] = 0
    return m, v


def _weights_and_grad(n, step, seed=0):
    gen = torch.Generator().manual_seed(1000 * seed + n)
    master = 0.02 * torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 1e-3 * (1 + 0.1 * math.sin(step))
    return master.to(dev()), g.to(BF16).to(dev())


def _same_bits(a, b):
    return np.array_equal(_np(a), _np(b))


def _step_both(ops, p_mode, clip, wd, step, index0, p, lo, g, state, p_key, skey, gscale=0.5, factor=0.8):
    """One step of the fp32-moment kernel on the decoded moments (-> p', lo', m', v' of the oracle) and of mh_adamw_compact on `state` in place."""
    fdev = torch.tensor([factor], dtype=F32, device=dev()) if clip else None
    m32, v32 = ops.adamw_states_unpack(*state)
    po, loo = p.clone(), lo.clone()
    if p_mode == SPLIT:
        ops.adamw_split_(po, loo, g, m32, v32, LR, B1, B2, EPS, wd, step, gscale, fdev)
    elif p_mode == SR:
        ops.adamw_sr_(po, g, m32, v32, LR, B1, B2, EPS, wd, step, gscale, fdev, p_key, index0)
    elif clip:
        ops.adamw_clip_(po, g, m32, v32, LR, B1, B2, EPS, wd, step, gscale, fdev)
    else:
        ops.adamw_(po, g, m32, v32, LR, B1, B2, EPS, wd, step, gscale)
    ops.adamw_compact_(p, lo if p_mode == SPLIT else None, g, *state, LR, B1, B2, EPS, wd, step, gscale, fdev, p_mode, p_key, skey, index0)
    return po, loo, m32, v32


# ---- 1. the fp32-moment kernels as the arithmetic oracle, the restatement as the format's ---------------------------------------------------------
@pytest.mark.parametrize("p_mode", [NEAREST, SPLIT, SR])
@pytest.mark.parametrize("index0", [0, 128 * 7])
@pytest.mark.parametrize("n", SIZES)
def test_three_steps_against_the_fp32_moment_kernels_and_the_restatement(ops, n, index0, p_mode):
    for clip in (False, True):
        for wd in (WD, 0.0):
            m0, v0 = _random_moments(n, n + index0)
            state = _compact(*C.pack(m0, v0, 99, index0))
            got = ops.adamw_states_unpack(*state)
            want = C.unpack(*(_np(t) for t in state))
            assert np.array_equal(_np(got[0]).view(np.uint32), want[0].view(np.uint32)) and np.array_equal(_np(got[1]), want[1])  # exact decode
            master, _ = _weights_and_grad(n, 0)
            hi, low = R.split_bits(master)
            p, lo = hi.clone(), (low.clone() if p_mode == SPLIT else torch.zeros_like(low))
            for step in (1, 2, 3):
                g = _weights_and_grad(n, step)[1]
                p_key, skey = R.sr_key(3, step), C.state_key(3, step)
                po, loo, m32, v32 = _step_both(ops, p_mode, clip, wd, step, index0, p, lo, g, state, p_key, skey)
                what = f"n={n} index0={index0} p_mode={p_mode} clip={clip} wd={wd} step={step}"
                assert _same_bits(p, po), f"{what}: p differs in {int((_np(p) != _np(po)).sum())} elements"
                assert _same_bits(lo, loo), f"{what}: lo"
                assert bool((p != hi).any()) or n < 128, what  # (the step moved something)
                m8, ms, v16 = C.pack(_np(m32), _np(v32), skey, index0)
                assert np.array_equal(_np(state[1]), ms), f"{what}: scale bytes"
                assert np.array_equal(_np(state[0]), m8), f"{what}: {int((_np(state[0]) != m8).sum())} e4m3 bytes differ"
                assert np.array_equal(_np(state[2]), v16), f"{what}: {int((_np(state[2]) != v16).sum())} bf16 v differ"


# ---- 2. footprint ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p_mode", [NEAREST, SPLIT, SR])
def test_nothing_outside_the_slices_and_the_owned_scale_bytes_changes(ops, p_mode):
    off, n, pad = 128 * 3, 128 * 5 + 37, 128 * 2  # a non-zero block offset, a partial last block, two blocks of sentinel behind it
    total = off + n + pad
    nb = -(-n // 128)
    sent = {"p": 0x4A4A, "lo": 0x5B5B, "g": 0x3C3C, "v16": 0x6D6D}
    buf = {k: torch.full((total,), s, dtype=torch.int16, device=dev()) for k, s in sent.items()}
    buf["m8"] = torch.full((total,), 0xE7, dtype=torch.uint8, device=dev())
    buf["ms"] = torch.full((total // 128 + 1,), 0xC3, dtype=torch.uint8, device=dev())
    m32 = torch.full((total,), 7.0, device=dev())
    v32 = torch.full((total,), 9.0, device=dev())
    m0, v0 = _random_moments(n, 5)
    m32[off: off + n], v32[off: off + n] = torch.from_numpy(m0).to(dev()), torch.from_numpy(v0).to(dev())
    sl = slice(off, off + n)
    view = {k: buf[k][sl].view(BF16) if k in ("p", "g", "v16") else buf[k][sl] for k in ("p", "lo", "g", "v16", "m8")}
    ops.adamw_states_pack(m32[sl], v32[sl], view["m8"], buf["ms"][off // 128:], view["v16"], 11, off)
    master, g = _weights_and_grad(n, 1)
    view["p"].copy_(master.to(BF16)), view["g"].copy_(g)
    view["lo"].zero_()
    before = {k: b.clone() for k, b in buf.items()}
    ops.adamw_compact_(view["p"], view["lo"] if p_mode == SPLIT else None, view["g"], view["m8"], buf["ms"][off // 128:], view["v16"], LR, B1, B2, EPS,
                       WD, 1, 1.0, None, p_mode, 77, 78, off)
    m_back, v_back = torch.full((total,), 7.0, device=dev()), torch.full((total,), 9.0, device=dev())
    ops.adamw_states_unpack(view["m8"], buf["ms"][off // 128:], view["v16"], m_back[sl], v_back[sl])
    torch.cuda.synchronize()
    for k in ("p", "lo", "g", "v16", "m8"):
        assert torch.equal(buf[k][:off], before[k][:off]) and torch.equal(buf[k][off + n:], before[k][off + n:]), k
    assert torch.equal(buf["g"], before["g"])
    assert torch.equal(buf["ms"][: off // 128], before["ms"][: off // 128]) and torch.equal(buf["ms"][off // 128 + nb:], before["ms"][off // 128 + nb:])
    assert bool((buf["ms"][off // 128 + nb:] == 0xC3).all()) and bool((buf["m8"][off + n:] == 0xE7).all()) and bool((buf["v16"][:off] == 0x6D6D).all())
    for t, s in ((m32, 7.0), (v32, 9.0), (m_back, 7.0), (v_back, 9.0)):
        assert bool((t[:off] == s).all()) and bool((t[off + n:] == s).all())
    # and everything inside was written
    assert not torch.equal(buf["p"][sl], before["p"][sl]) and not torch.equal(buf["m8"][sl], before["m8"][sl]) and not torch.equal(buf["v16"][sl], before["v16"][sl])
    assert torch.equal(buf["lo"][sl], before["lo"][sl]) == (p_mode != SPLIT)
    assert bool((m_back[sl] != 7.0).all()) and bool((v_back[sl] != 9.0).all())


# ---- 3. cut independence -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p_mode", [NEAREST, SPLIT, SR])
def test_one_launch_equals_two_launches_cut_at_a_block_boundary(ops, p_mode):
    n, index0 = 128 * 40 + 77, 128 * 2
    m0, v0 = _random_moments(n, 1)
    master, g = _weights_and_grad(n, 2)
    out = []
    for cuts in (((0, n),), ((0, 128 * 17), (128 * 17, n)), ((0, 128 * 40), (128 * 40, n))):
        m8, ms, v16 = _compact(*C.pack(m0, v0, 5, index0))
        p, lo = R.split_bits(master)
        for a, b in cuts:
            ops.adamw_compact_(p[a:b], lo[a:b] if p_mode == SPLIT else None, g[a:b], m8[a:b], ms[a // 128:], v16[a:b], LR, B1, B2, EPS, WD, 2, 0.5, None,
                               p_mode, 31, 32, index0 + a)
        out.append([_np(t) for t in (p, lo, m8, ms, v16)])
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)
    shifted = _compact(*C.pack(m0, v0, 5, index0))  # (the fields do depend on the arena index)
    ops.adamw_compact_(R.split_bits(master)[0], None, g, *shifted, LR, B1, B2, EPS, WD, 2, 0.5, None, NEAREST, 31, 32, index0 + 128)
    assert not np.array_equal(_np(shifted[0]), out[0][2])


# ---- 4. unbiasedness -------------------------------------------------------------------------------------------------------------------------
def test_both_stores_are_unbiased(ops):
    n, keys = 2 ** 16, 8
    rng = np.random.default_rng(4)
    e = -12
    y = rng.uniform(0.001, 440.0, n) * 10.0 ** rng.uniform(-3, 0, n)  # every binade of the e4m3 grid, its subnormals included
    y[::128] = 448.0                                                  # pins every block's scale at 2^e
    m = (np.ldexp(y, e) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    v = (rng.uniform(1.0, 2.0, n) * 10.0 ** rng.uniform(-12, -4, n)).astype(np.float32)
    m_d, v_d = torch.from_numpy(m).to(dev()), torch.from_numpy(v).to(dev())
    y32 = np.ldexp(np.abs(m).astype(np.float64), -e)
    idx = np.searchsorted(C.E4M3, y32, side="right") - 1
    m_spacing = np.ldexp(C.E4M3[np.minimum(idx + 1, 126)] - C.E4M3[np.minimum(idx, 125)], e)
    v_spacing = R.bf16_spacing(torch.from_numpy(v)).numpy()
    assert float(((y32 != C.E4M3[idx]).mean())) > 0.98 and float(((v.view(np.uint32) & 0xFFFF) != 0).mean()) > 0.98  # off both grids
    em = ev = 0.0
    m8, ms, v16 = (torch.empty(n, dtype=torch.uint8, device=dev()), torch.empty(n // 128, dtype=torch.uint8, device=dev()),
                   torch.empty(n, dtype=BF16, device=dev()))
    for k in range(keys):
        ops.adamw_states_pack(m_d, v_d, m8, ms, v16, C.state_key(0, k + 1), 0)
        assert bool((ms == e + 127).all())
        mq, vq = ops.adamw_states_unpack(m8, ms, v16)
        em += float(((mq.cpu().numpy().astype(np.float64) - m) / m_spacing).sum())
        ev += float(((vq.cpu().numpy().astype(np.float64) - v) / v_spacing).sum())
    N = n * keys
    em, ev = em / N, ev / N
    bound = 5 * 0.5 / math.sqrt(N)  # per-sample variance t (1 - t) <= 1/4, in spacings; m rounds up with probability < t + 2^-16
    print(f"UNBIASED | m: mean error {em:.3e} spacings (bound {bound + 2.0 ** -16:.3e}) | v: {ev:.3e} (bound {bound:.3e}) | N = {N}")
    assert abs(em) <= bound + 2.0 ** -16, (em, bound)
    assert abs(ev) <= bound, (ev, bound)


# ---- 5. block structure, pack -> unpack --------------------------------------------------------------------------------------------------------
def test_block_structure_and_pack_unpack(ops):
    rng = np.random.default_rng(6)
    n = 128 * 3 + 77
    m = (1e-6 * (1 + rng.random(n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    m[17] *= 2.0 ** 20            # block 0: one element 2^20 times its neighbours (they fall below the grid's smallest step)
    m[128: 256] = 0               # block 1: all zero
    m[256 + 5] = np.float32(-0.0)
    m[128 * 3 + 76] = -0.3        # block 3 is partial and its maximum is its last element (lane 9 of 16; lanes 10 .. 15 hold nothing)
    v = (rng.random(n) * 1e-9).astype(np.float32)
    v[128: 256] = 0
    index0 = 128 * 4
    m8, ms, v16 = (torch.zeros(n, dtype=torch.uint8, device=dev()), torch.zeros(4, dtype=torch.uint8, device=dev()), torch.zeros(n, dtype=BF16, device=dev()))
    for key in (1, 2, 3):
        ops.adamw_states_pack(torch.from_numpy(m).to(dev()), torch.from_numpy(v).to(dev()), m8, ms, v16, key, index0)
        w8, ws, w16 = C.pack(m, v, key, index0)
        assert _np(ms).tolist() == ws.tolist() and ws[1] == 127 and ws[3] == int(C.scale_exp(np.float32(0.3))) + 127
        assert np.array_equal(_np(m8), w8) and np.array_equal(_np(v16), w16)
        assert not _np(m8)[128: 256].any() and _np(m8)[256 + 5] == 0x80 and not _np(v16)[128: 256].any()
        mq, vq = ops.adamw_states_unpack(m8, ms, v16)
        wm, wv = C.unpack(w8, ws, w16)
        assert np.array_equal(_np(mq).view(np.uint32), wm.view(np.uint32)) and np.array_equal(_np(vq), wv)  # unpack is exact
        # every value lands on one of its two grid neighbours
        e = np.repeat(ws.astype(np.int64) - 127, 128)[:n]
        idx = np.searchsorted(C.E4M3, np.ldexp(np.abs(m).astype(np.float64), -e).astype(np.float32).astype(np.float64), side="right") - 1
        code = (_np(m8) & 0x7F).astype(np.int64)
        assert bool(((code == idx) | (code == idx + 1)).all())
        assert bool((np.abs(wv.astype(np.float64) - v) < R.bf16_spacing(torch.from_numpy(v)).numpy() + (v == 0)).all())
    small = (_np(m8)[:128] & 0x7F)
    assert set(small[np.arange(128) != 17].tolist()) <= {0, 1} and small[17] > 0x70


# ---- 6. what v's stochastic store is for ---------------------------------------------------------------------------------------------------------
def test_400_steps_compact_v_follows_the_fp32_v_through_a_gradient_drop(ops):
    n, steps = 4096, 400
    g_all = torch.from_numpy(C.stream(n, steps, 2, 3, drop_at=100)).to(BF16)  # the gradient drops by 1e3 at step 100
    sim = C.simulate(g_all.float().numpy(), seed=0, b1=B1, b2=B2, eps=EPS)     # the same stream, the same keys, fp32 recurrences
    figure = float(np.abs(sim["vq_mean"] / sim["v_mean"] - 1).max())
    g_all = g_all.to(dev())
    p_f, p_c = torch.zeros(n, dtype=BF16, device=dev()), torch.zeros(n, dtype=BF16, device=dev())
    m, v = torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    state = _compact(*C.pack(np.zeros(n, np.float32), np.zeros(n, np.float32), 0, 0))
    ratio = torch.zeros(steps, dtype=torch.float64, device=dev())
    for step in range(1, steps + 1):
        ops.adamw_(p_f, g_all[step - 1], m, v, LR, B1, B2, EPS, 0.0, step)
        ops.adamw_compact_(p_c, None, g_all[step - 1], *state, LR, B1, B2, EPS, 0.0, step, 1.0, None, NEAREST, 0, C.state_key(0, step), 0)
        ratio[step - 1] = state[2].double().mean() / v.double().mean()
        if step == 99:
            v99 = float(state[2].double().mean())
    got = float((ratio - 1).abs().max())
    print(f"V TRACK | 400 steps, drop at 100 | max |mean(v compact) / mean(v fp32) - 1|: kernel {got:.4e}, simulator {figure:.4e}, bound {1.5 * figure:.4e}")
    assert float(state[2].double().mean()) < 0.76 * v99  # it decays: 0.999^300 = 0.74
    assert got <= 1.5 * figure, (got, figure)


# ---- 7. model level ----------------------------------------------------------------------------------------------------------------------------
def test_model_20_steps_compact_moments_follow_fp32_moments(monkeypatch):
    from oracle import cases as OC
    from merlin_amd import _lib as L
    from merlin_amd import optim as OPT
    from test_adamw_rounding_gpu import _build

    cfg, batch = OC.get_case("tiny_2img")
    batch = dict(input_ids=batch["input_ids"].cuda(), attention_mask=batch["attention_mask"].cuda(), labels=batch["labels"].cuda(),
                 images=[im.cuda() for im in batch["images"]])
    lr, wd, clip_at, steps = 5e-5, 0.05, 1.0, 20  # pretrain.sh; HF's default max_grad_norm
    hp = dict(lr=lr, betas=(0.9, 0.95), eps=1e-8, weight_decay=wd, lr_scale_fn=OPT.vit_lr_scale, rounding="split")
    # the expected size: the simulator's accumulated deviation at 20 steps with these betas, the wider of its two spreads (how far the
    # gradient magnitudes of a real tensor spread inside a block is not known); 2 x because the model's gradients are not i.i.d.
    figure = max(C.simulate(C.stream(128 * 64, steps, d, 1), b1=0.9, b2=0.95)["acc_l2"] for d in (2, 5))
    model, control = _build(cfg, BF16), _build(cfg, BF16)
    opt, opt_c = OPT.FusedAdamW(model.engine, states="compact", **hp), OPT.FusedAdamW(control.engine, **hp)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    init = {n: p.detach().float().clone() for n, p in named}
    names, real = [], L.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)

    for _ in range(steps):
        model(**batch).loss.backward()
        control(**batch).loss.backward()
        # as in the fixture this follows, both optimizers are handed the SAME gradients (the compact model's): a gradient that is rounding noise
        # (a key bias: softmax does not see it) would otherwise differ between the two models and be compared with itself
        control.engine.ensure_arena().gflat.copy_(model.engine.ensure_arena().gflat)
        opt.step(max_grad_norm=clip_at)
        opt.zero_grad()
        monkeypatch.setattr(L, "call", recording)
        opt_c.step(max_grad_norm=clip_at)
        monkeypatch.setattr(L, "call", real)
        opt_c.zero_grad()
    new = {"mh_adamw_compact", "mh_adamw_states_pack", "mh_adamw_states_unpack"}
    assert "mh_adamw_split" in names and not (new & set(names))  # states="fp32" launches what it always did
    A = model.engine.ensure_arena()
    assert opt.m is None and opt.state_bytes() <= (3 + 1 / 128) * A.total + 128
    assert opt_c.state_bytes() == 8 * A.total
    worst = (0.0, None)
    rows = []
    for n, p in named:
        d_c, d_f = opt.master(n).double() - init[n].double(), opt_c.master(n).double() - init[n].double()
        ref = float(d_f.norm())
        rel = float((d_c - d_f).norm()) / ref if ref > 0 else float((d_c - d_f).norm())
        rows.append((rel, n))
        worst = max(worst, (rel, n))
        mc, vc = opt.moments(n)
        mf, vf = opt_c.moments(n)
        assert mc.shape == vc.shape == p.shape and mc.dtype == vc.dtype == F32 and mf.data_ptr() == opt_c.m[A.offset[n]:].data_ptr()
        off = A.offset[n]  # moments() is the exact decode of the parameter's slice of the three buffers
        wm, wv = C.unpack(_np(opt.m8[off: off + p.numel()]), _np(opt.mscale[off // 128:]), _np(opt.v16[off: off + p.numel()]))
        assert np.array_equal(_np(mc).reshape(-1).view(np.uint32), wm.view(np.uint32)) and np.array_equal(_np(vc).reshape(-1), wv), n
        assert torch.equal(mf, opt_c.m[off: off + p.numel()].view(p.shape)) and torch.equal(vf, opt_c.v[off: off + p.numel()].view(p.shape))
    rels = sorted(r for r, _ in rows)
    print(f"MODEL | 20 steps, split masters | ||dp_compact - dp_fp32|| / ||dp_fp32|| per tensor: median {rels[len(rels) // 2]:.4f}, worst {worst[0]:.4f} "
          f"({worst[1]}) | simulator {figure:.4f}, bound {2 * figure:.4f} | {len(rels)} tensors")
    for rel, n in sorted(rows, reverse=True)[:5]:
        print(f"MODEL |   {rel:.4f}  {n}")
    assert worst[0] <= 2 * figure, (worst, figure)


# ---- 8. what the ABI refuses -----------------------------------------------------------------------------------------------------------------
def test_abi_refusals(ops):
    from merlin_amd import _lib as L

    n = 256
    p, g, lo, v16 = (torch.zeros(n, dtype=d, device=dev()) for d in (BF16, BF16, torch.int16, BF16))
    m8, ms = torch.zeros(n, dtype=torch.uint8, device=dev()), torch.full((2,), 127, dtype=torch.uint8, device=dev())
    g.fill_(1e-3)
    s = torch.cuda.current_stream().cuda_stream
    ARG, DTYPE = L.DEFINES["MH_ERR_ARG"], L.DEFINES["MH_ERR_DTYPE"]

    def go(p_=p, lo_=lo, g_=g, m8_=m8, ms_=ms, v16_=v16, n_=n, step=1, mode=SPLIT, index0=0, dt=L.MH_BF16):
        return L.launch("mh_adamw_compact", p_, lo_, g_, m8_, ms_, v16_, n_, LR, B1, B2, EPS, WD, step, 1.0, None, mode, 1, 2, index0, dt, s)

    assert go(index0=64) == go(index0=1) == go(index0=-128) == ARG          # a misaligned index0
    assert go(lo_=None) == ARG                                              # a null lo in mode 1
    assert go(dt=L.MH_F16) == go(dt=L.MH_F32) == go(mode=NEAREST, dt=L.MH_F16) == DTYPE
    assert go(n_=0) == go(n_=-5) == go(step=0) == ARG
    assert go(p_=None) == go(g_=None) == go(m8_=None) == go(ms_=None) == go(v16_=None) == ARG
    assert go(mode=3) == go(mode=-1) == ARG
    m32 = torch.ones(n, device=dev())
    assert L.launch("mh_adamw_states_pack", m32, m32, m8, ms, v16, n, 1, 64, s) == ARG
    assert L.launch("mh_adamw_states_pack", None, m32, m8, ms, v16, n, 1, 0, s) == L.launch("mh_adamw_states_pack", m32, m32, m8, ms, v16, 0, 1, 0, s) == ARG
    assert L.launch("mh_adamw_states_unpack", m8, ms, v16, None, m32, n, s) == L.launch("mh_adamw_states_unpack", m8, ms, v16, m32, m32, 0, s) == ARG
    with pytest.raises(L.MerlinHipError, match="dtype"):
        ops.adamw_compact_(p.to(torch.float16), None, g.to(torch.float16), m8, ms, v16, LR, B1, B2, EPS, WD, 1)
    with pytest.raises(L.MerlinHipError, match="bad argument"):
        ops.adamw_compact_(p, None, g, m8, ms, v16, LR, B1, B2, EPS, WD, 1, p_mode=SPLIT)
    with pytest.raises(L.MerlinHipError, match="bad argument"):
        ops.adamw_compact_(p, None, g, m8, ms, v16, LR, B1, B2, EPS, WD, 1, index0=100)
    torch.cuda.synchronize()
    assert not bool(p.any()) and not bool(lo.any()) and not bool(m8.any()) and not bool(v16.any()) and bool((ms == 127).all())  # nothing was launched
    assert bool((m32 == 1).all())
    assert go() == go(mode=NEAREST, lo_=None) == go(mode=SR, lo_=None, index0=128) == 0
    torch.cuda.synchronize()
    assert bool(p.any()) and bool(m8.any()) and bool(v16.any())
