"""The parameter stores behind FusedAdamW(rounding=...), without a GPU: the bit identities of the split master, the defect of the
round-to-nearest store that the two new stores exist for, the unbiasedness of the stochastic store's definition, and the optimizer's host
logic (which launch, which slices, which key, when `lo` is dropped) on a stub engine with torch emulations in place of the kernels."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import adamw_rounding_ref as R  # noqa: E402

from merlin_amd import optim  # noqa: E402

BF16 = torch.bfloat16


def _normals(n=2 ** 20, sigma=0.02, seed=0):
    return sigma * torch.randn(n, generator=torch.Generator().manual_seed(seed))


# ---- 1. bit identities ------------------------------------------------------------------------------------------------------------------
def test_split_and_join_are_inverse_and_split_rounds_to_nearest():
    big = torch.tensor([0x7F7F], dtype=torch.int16).view(BF16).float()  # largest finite bf16
    sub = R.bits_f32(torch.tensor([1, 0x7FFF, 0x8000, 0xFFFF, 0x18000, 0x7FFFFF, 0x80000001, 0x807FFFFF]))  # fp32 / bf16 subnormals
    edge = torch.cat([torch.tensor([0.0, -0.0]), sub, big, -big, torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9, -1.0 - 2.0 ** -9])])
    x = torch.cat([_normals(), edge])
    p, lo = R.split_bits(x)
    assert p.dtype == BF16 and lo.dtype == torch.int16
    assert torch.equal(R.f32_bits(R.join_bits(p, lo)), R.f32_bits(x))  # bitwise, signed zeros included
    assert int(lo.min()) == -32768 and int(lo.max()) == 32767
    assert bool(((p.double() - x.double()).abs() <= R.bf16_spacing(x) / 2).all())
    tie = (R.f32_bits(x) & 0xFFFF) == 0x8000
    differs = R.bf16_bits(p) != R.bf16_bits(x.to(BF16))
    assert bool((tie | ~differs).all()) and 0 < int(differs.sum()) < 1e-4 * x.numel()  # ties away from zero against ties to even
    assert torch.equal(R.f32_bits(R.join_bits(p, torch.zeros_like(lo))), R.f32_bits(p.float()))  # lo = 0: master = p


# ---- 2. the defect: what round-to-nearest does to this project's updates ----------------------------------------------------------------
def test_nearest_store_drops_the_recipes_updates():
    lr = 5e-5  # pretrain.sh's peak lr; a full-lr Adam step moves every element by lr
    p = torch.ones(64, dtype=BF16)
    for _ in range(400):
        p = R.nearest_store(p.float() - lr)
    assert bool((p == 1.0).all())  # norm weights never move: half a spacing below 1.0 is 1.95e-3
    w = _normals().to(BF16)
    for step, share in ((lr, 0.433), (lr * 0.9 ** 22, 0.92)):  # decoder weights; the first ViT layers under LLRD
        frozen = float((R.nearest_store(w.float() - step) == w).double().mean())
        assert abs(frozen - share) <= 0.01, (step, frozen)
    # the split master keeps all of it
    q, lo = R.split_bits(torch.ones(64))
    for _ in range(400):
        q, lo = R.split_bits(R.join_bits(q, lo) - lr)
    assert float((R.join_bits(q, lo).double() - (1 - 400 * lr)).abs().max()) < 400 * 2.0 ** -24


# ---- 3. the stochastic store is unbiased ------------------------------------------------------------------------------------------------
def test_sr_store_is_unbiased():
    n, spacing = 2 ** 20, 2.0 ** -8  # the bf16 spacing just below 1.0
    x = torch.full((n,), 1.0) - torch.tensor(0.1 * spacing)
    got = R.sr_store(x, R.sr_key(0, 1), 0)
    assert bool(((got == 1.0) | (got == 1.0 - spacing)).all())
    err = float(((got.double() - x.double()) / spacing).mean())
    # a sum of n independent errors in (-1, 1) with variance <= 1/4: five standard deviations
    assert abs(err) <= 2.5 / math.sqrt(n), err
    assert abs(float((got == 1.0).double().mean()) - 0.9) <= 2.5 / math.sqrt(n)  # P(up) is the dropped fraction
    near = float(((R.nearest_store(x).double() - x.double()) / spacing).mean())
    assert abs(near - 0.1) < 1e-3  # the nearest store is off by the whole fraction
    # inf / nan are truncated, not carried into
    special = R.bits_f32(torch.tensor([0x7F800000, 0xFF800000, 0x7FC0FFFF]))
    assert R.bf16_bits(R.sr_store(special, 12345, 0)).tolist() == [0x7F80, 0xFF80, 0x7FC0]
    # one hash serves four elements, whatever index the slice starts at
    assert R.sr_fields(16, 99, 0)[5:].tolist() == R.sr_fields(11, 99, 5).tolist()


# ---- 4. host logic of FusedAdamW ---------------------------------------------------------------------------------------------------------
class _Arena:
    def __init__(self, dtype=BF16):
        shapes = {"a.weight": (8, 30), "a.norm.weight": (30,), "b.weight": (4, 50), "frozen.weight": (3, 3), "c.weight": (2, 64)}
        g = torch.Generator().manual_seed(1)
        self.names, self.params, self.offset = list(shapes), {}, {}
        off = 0
        for n, s in shapes.items():
            self.offset[n] = off
            off += -(-math.prod(s) // 128) * 128
        self.total = off
        self.flat = torch.zeros(off, dtype=dtype)
        self.gflat = torch.zeros(off, dtype=dtype)
        for n, s in shapes.items():
            k = math.prod(s)
            self.flat[self.offset[n]: self.offset[n] + k] = (0.02 * torch.randn(k, generator=g)).to(dtype)
            self.gflat[self.offset[n]: self.offset[n] + k] = (0.01 * torch.randn(k, generator=g)).to(dtype)
            self.params[n] = torch.nn.Parameter(self.flat[self.offset[n]: self.offset[n] + k].view(s), requires_grad=n != "frozen.weight")


class _Engine:
    def __init__(self, dtype=BF16):
        self.arena = _Arena(dtype)
        self.weight_version = 0

    def ensure_arena(self):
        return self.arena

    def weights_changed(self):
        self.weight_version += 1


def _adam(master, g, m, v, lr, b1, b2, eps, wd, step, gscale, gdev):
    g = g.float() * gscale * (1.0 if gdev is None else float(gdev[0]))
    m.mul_(b1).add_((1 - b1) * g)
    v.mul_(b2).add_((1 - b2) * g * g)
    return master * (1 - lr * wd) - lr * (m / (1 - b1 ** step)) / ((v / (1 - b2 ** step)).sqrt() + eps)


@pytest.fixture
def calls(monkeypatch):
    """Torch emulations of the launches FusedAdamW.step makes, each recording (name, arguments)."""
    log = []

    def adamw_(p, g, m, v, lr, b1, b2, eps, wd, step, gscale=1.0):
        log.append(("adamw_", p, None))
        p.copy_(R.nearest_store(_adam(p.float(), g, m, v, lr, b1, b2, eps, wd, step, gscale, None)))

    def adamw_clip_(p, g, m, v, lr, b1, b2, eps, wd, step, gscale, gdev):
        log.append(("adamw_clip_", p, None))
        p.copy_(R.nearest_store(_adam(p.float(), g, m, v, lr, b1, b2, eps, wd, step, gscale, gdev)))

    def adamw_split_(p, lo, g, m, v, lr, b1, b2, eps, wd, step, gscale=1.0, gdev=None):
        log.append(("adamw_split_", p, lo))
        hi, low = R.split_bits(_adam(R.join_bits(p, lo), g, m, v, lr, b1, b2, eps, wd, step, gscale, gdev))
        p.copy_(hi)
        lo.copy_(low)

    def adamw_sr_(p, g, m, v, lr, b1, b2, eps, wd, step, gscale=1.0, gdev=None, key=0, index0=0):
        log.append(("adamw_sr_", p, (key, index0)))
        p.copy_(R.sr_store(_adam(p.float(), g, m, v, lr, b1, b2, eps, wd, step, gscale, gdev), key, index0))

    def sumsq_det(g, partial, out):
        out[0] = g.float().pow(2).sum()

    def clip_scale(ss, gscale, max_norm, out2):
        norm = ss[0].sqrt() * abs(gscale)
        out2[0], out2[1] = min(1.0, max_norm / (float(norm) + 1e-6)), norm

    for f in (adamw_, adamw_clip_, adamw_split_, adamw_sr_, sumsq_det, clip_scale):
        monkeypatch.setattr(optim.O, f.__name__, f, raising=True)  # (raising: the wrappers must exist in ops)
    return log


HP = dict(lr=5e-5, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)


def test_refusals_name_the_argument_and_the_dtype(calls):
    with pytest.raises(ValueError, match="rounding"):
        optim.FusedAdamW(_Engine(), rounding="bankers", **HP)
    for mode in ("split", "stochastic"):
        opt = optim.FusedAdamW(_Engine(torch.float16), rounding=mode, **HP)
        with pytest.raises(ValueError, match=r"rounding.*float16"):
            opt.step()
    assert calls == []  # refused before any launch
    optim.FusedAdamW(_Engine(torch.float16), **HP).step()  # the default takes fp16 as it always did
    assert {c[0] for c in calls} == {"adamw_"}


def test_default_mode_launches_what_it_always_did(calls):
    eng = _Engine()
    opt = optim.FusedAdamW(eng, **HP)
    assert opt.rounding == "nearest"
    opt.step()
    opt.step(max_grad_norm=1.0)
    runs = len(opt._runs)
    assert runs == 4  # a.weight | a.norm.weight | b.weight | c.weight: the frozen tensor breaks adjacency, the norm weight the decay
    assert [c[0] for c in calls] == ["adamw_"] * runs + ["adamw_clip_"] * runs
    assert opt.lo is None and opt.reseeds == 0


def test_split_passes_matching_lo_slices_and_reseeds_only_when_the_weights_changed_behind_it(calls):
    eng = _Engine()
    A = eng.arena
    opt = optim.FusedAdamW(eng, rounding="split", **HP)
    before = A.flat.clone()
    opt.step(max_grad_norm=1.0)
    assert opt.lo.dtype == torch.int16 and opt.lo.numel() == A.total
    assert [c[0] for c in calls] == ["adamw_split_"] * 4
    for (_, p, lo), (off, num, _, _) in zip(calls, opt._runs):
        assert p.data_ptr() == A.flat[off:].data_ptr() and lo.data_ptr() == opt.lo[off:].data_ptr() and p.numel() == lo.numel() == num
    for _ in range(3):
        opt.step()
    assert opt.reseeds == 0 and bool((opt.lo != 0).any())
    name = "a.norm.weight"
    off, k = A.offset[name], A.params[name].numel()
    assert torch.equal(opt.master(name), R.join_bits(A.flat[off: off + k], opt.lo[off: off + k]).view(A.params[name].shape))
    assert torch.equal(A.flat[A.offset["frozen.weight"]:][:9], before[A.offset["frozen.weight"]:][:9])
    # the weights change behind the optimizer (a load, a stock torch step): lo no longer belongs to them
    eng.weights_changed()
    assert torch.equal(opt.master(name), A.flat[off: off + k].float().view(-1))  # a stale lo is not used
    calls.clear()
    opt.step()
    assert opt.reseeds == 1
    assert all(c[0] == "adamw_split_" for c in calls)
    opt.step()
    assert opt.reseeds == 1
    # the arena is repacked into a new buffer
    A.flat = A.flat.clone()
    opt.step()
    assert opt.reseeds == 2
    opt.step()
    assert opt.reseeds == 2
    # a reseed zeroes lo before the step: the step then starts from master = p
    eng.weights_changed()
    seen = []
    orig = optim.O.adamw_split_
    optim.O.adamw_split_ = lambda p, lo, *a: (seen.append(int(lo.abs().max())), orig(p, lo, *a))
    try:
        opt.step()
    finally:
        optim.O.adamw_split_ = orig
    assert seen == [0, 0, 0, 0] and opt.reseeds == 3


def test_stochastic_passes_the_arena_offset_and_the_documented_key(calls):
    a, b = optim.FusedAdamW(_Engine(), rounding="stochastic", seed=7, **HP), optim.FusedAdamW(_Engine(), rounding="stochastic", seed=7, **HP)
    other = optim.FusedAdamW(_Engine(), rounding="stochastic", seed=8, **HP)
    keys = []
    for step in (1, 2, 3):
        calls.clear()
        a.step(max_grad_norm=1.0 if step == 2 else None)
        assert [c[0] for c in calls] == ["adamw_sr_"] * 4
        assert [c[2][1] for c in calls] == [r[0] for r in a._runs]  # index0 = the run's arena offset
        assert {c[2][0] for c in calls} == {R.sr_key(7, step)}
        keys.append(calls[0][2][0])
        calls.clear()
        b.step()
        other.step()
        assert calls[0][2][0] == keys[-1] and calls[-1][2][0] == R.sr_key(8, step) != keys[-1]
    assert len(set(keys)) == 3 and all(0 <= k < 2 ** 64 for k in keys)
    assert a.lo is None
    with pytest.raises(ValueError, match="split"):
        a.master("a.weight")
