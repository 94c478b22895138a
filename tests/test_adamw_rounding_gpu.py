"""mh_adamw_split / mh_adamw_sr and FusedAdamW(rounding="split" | "stochastic") on the device, bf16, at the real recipe's lr 5e-5 and
wd 0.05 (pretrain.sh), where the round-to-nearest store of mh_adamw drops most of a step.  References: tests/numerics.py adamw_step in
fp64 (with its fp32 rounding model) fed the fp32 master as `p`, and the integer restatement of the two stores in tests/adamw_rounding_ref.py.

Sizes: 1, 7, 8, 9 (below, at and just past one 16-byte access), 2053 (several blocks and a tail; also as a slice starting at element 1,
where no pointer is 16-byte aligned and the kernel goes element by element), 4 * 2^20 + 2053 (the grid-stride loop wraps once past the
2048-block cap and leaves a tail)."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import adamw_rounding_ref as R  # noqa: E402
import numerics as N  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
LR, WD = 5e-5, 0.05
HP = dict(beta1=0.9, beta2=0.95, eps=1e-8)
BIG = 4 * 2 ** 20 + 2053
SIZES = [(1, 0), (7, 0), (8, 0), (9, 0), (2053, 0), (2053, 1), (BIG, 0)]  # (n, first element of the slice within its 16-byte aligned buffer)
E32, T32 = N.EPS16[F32], 1e-37


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from merlin_amd import ops as O

    assert O.arch_ok(0), "not a gfx950 device"
    return O


def _inputs(n, step, case="weights"):
    """fp32 master (the low half random, not zero) and a bf16 gradient of consistent direction (tests/numerics.py adamw_inputs)."""
    gen = torch.Generator().manual_seed(n)
    master = (1.0 if case == "ones" else 0.0) + 0.02 * torch.randn(n, generator=gen)
    base = torch.randn(n, generator=gen).abs() * 1e-2 * torch.where(master < 0, -1.0, 1.0)
    return master.to(dev()), (base * (1 + 0.1 * math.sin(step))).to(BF16).to(dev())


def _sliced(n, first, dtype):
    """An n-element slice starting `first` elements into a fresh (256-byte aligned) buffer."""
    return torch.zeros(n + first + 8, dtype=dtype, device=dev())[first: first + n]


def _tol(ref, mod):
    """Per-element absolute bound on an fp32 evaluation of p: limit(c of the fp32 rounding model) x 2^-24 (|p| + B_p)."""
    cm = N.componentwise(mod["p"], ref["p"], ref["B_p"], E32, T32)[0]
    return N.limit(cm) * (E32 * (ref["p"].abs() + ref["B_p"]) + T32), cm


# ---- 5. split master, ten steps, each from the state the kernel left ---------------------------------------------------------------------
@pytest.mark.parametrize("decay", [True, False])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("n,first", SIZES)
def test_split_ten_steps_one_at_a_time(ops, n, first, clip, decay):
    wd = WD if decay else 0.0
    gscale, factor = 0.5, 0.8
    fdev = torch.tensor([factor], dtype=F32, device=dev())
    p, lo, m, v, g = _sliced(n, first, BF16), _sliced(n, first, torch.int16), _sliced(n, first, F32), _sliced(n, first, F32), _sliced(n, first, BF16)
    assert (p.data_ptr() % 16 == 0) == (first == 0)
    hi0, lo0 = R.split_bits(_inputs(n, 1)[0])
    p.copy_(hi0), lo.copy_(lo0)
    if n >= 2053:
        assert int(lo.min()) < -30000 and int(lo.max()) > 30000
    worst = {"p": (0.0, 0.0), "m": (0.0, 0.0), "v": (0.0, 0.0)}
    for step in range(1, 11):
        g.copy_(_inputs(n, step)[1])
        master0, m0, v0 = R.join_bits(p, lo), m.clone(), v.clone()
        kw = dict(lr=LR, wd=wd, step=step, gscale=gscale, gscale_dev=factor if clip else None, **HP)
        ref, mod = N.adamw_step(master0, g, m0, v0, **kw), N.adamw_step(master0, g, m0, v0, model=F32, **kw)
        if step == 1:  # what the store is for: at this lr most of the reference's steps are below half a bf16 spacing, and none below fp32's
            assert float(((ref["p"] - master0.double()).abs() < R.bf16_spacing(master0) / 2).double().mean()) > 0.3 or n < 2053
            assert N.resolvable(ref["p"], master0, _tol(ref, mod)[0]) >= 0.9 or n < 2053
        ops.adamw_split_(p, lo, g, m, v, LR, HP["beta1"], HP["beta2"], HP["eps"], wd, step, gscale, fdev if clip else None)
        master = R.join_bits(p, lo)
        hi, low = R.split_bits(master)
        assert torch.equal(R.bf16_bits(hi), R.bf16_bits(p)) and torch.equal(low, lo), f"step {step}: (p, lo) is not the split of its own master"
        for nm, got, Bc in (("p", master, ref["B_p"]), ("m", m, ref["B_m"]), ("v", v, 0.0)):
            cm = N.componentwise(mod[nm], ref[nm], Bc, E32, T32)[0]
            ck, at = N.componentwise(got, ref[nm], Bc, E32, T32)
            assert ck <= N.limit(cm), f"adamw_split {nm} step {step}: kernel c = {ck:.3f} at {at} exceeds {N.limit(cm):.3f} (model {cm:.3f})"
            if ck >= worst[nm][1]:
                worst[nm] = (cm, ck)
    for nm, (cm, ck) in worst.items():
        print(f"CW | adamw_split {nm} n={n}+{first} clip={clip} wd={wd} | fp32 master | {cm:.3f} | {ck:.3f} | {N.limit(cm):.3f} | worst of 10 steps")


def test_split_leaves_the_elements_around_an_unaligned_slice_alone(ops):
    n = 2053
    bufs = {k: torch.full((n + 16,), 3, dtype=d, device=dev()) for k, d in (("p", BF16), ("lo", torch.int16), ("g", BF16), ("m", F32), ("v", F32))}
    s = {k: b[1: 1 + n] for k, b in bufs.items()}
    s["g"].copy_(_inputs(n, 1)[1])
    ops.adamw_split_(s["p"], s["lo"], s["g"], s["m"], s["v"], LR, 0.9, 0.95, 1e-8, WD, 1)
    ops.adamw_sr_(s["p"], s["g"], s["m"], s["v"], LR, 0.9, 0.95, 1e-8, WD, 2, 1.0, None, 5, 3)
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b[:1] == 3).all()) and bool((b[1 + n:] == 3).all()), k


# ---- 6. stochastic store, one step ------------------------------------------------------------------------------------------------------
KEY = R.sr_key(0, 1)


def _sr_case(ops, n, first, clip, decay, key=KEY, index0=12, cut=None, case="weights"):
    """One mh_adamw_sr step (step 3 of a run: non-trivial bias corrections and moments).  -> stored p, and the inputs it started from."""
    wd, gscale, factor, step = (WD if decay else 0.0), 0.5, 0.8, 3
    fdev = torch.tensor([factor], dtype=F32, device=dev())
    p, m, v, g = _sliced(n, first, BF16), _sliced(n, first, F32), _sliced(n, first, F32), _sliced(n, first, BF16)
    master, g0 = _inputs(n, step, case)
    p.copy_(master.to(BF16)), g.copy_(g0), m.copy_(0.19 * g0.float() * gscale), v.copy_(0.0975 * (g0.float() * gscale) ** 2)
    p0, m0, v0 = p.clone(), m.clone(), v.clone()
    for a, b in ((0, n),) if cut is None else ((0, cut), (cut, n)):
        ops.adamw_sr_(p[a:b], g[a:b], m[a:b], v[a:b], LR, HP["beta1"], HP["beta2"], HP["eps"], wd, step, gscale, fdev if clip else None, key, index0 + a)
    kw = dict(lr=LR, wd=wd, step=step, gscale=gscale, gscale_dev=factor if clip else None, **HP)
    return p, (p0, g, m0, v0, kw), (m, v)


@pytest.mark.parametrize("decay", [True, False])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("n,first", SIZES)
def test_stochastic_one_step_contained_predicted_unbiased(ops, n, first, clip, decay):
    index0 = 12 + first
    p, (p0, g, m0, v0, kw), (m, v) = _sr_case(ops, n, first, clip, decay, index0=index0)
    ref, mod = N.adamw_step(p0, g, m0, v0, **kw), N.adamw_step(p0, g, m0, v0, model=F32, **kw)
    ref["B_p"] = ref["B_p"] * (N.EPS16[BF16] / E32)  # (adamw_step scales B_p for a bf16 store of p; here it is the fp32 value that is held)
    tol, cm = _tol(ref, mod)
    for nm, got, Bc in (("m", m, ref["B_m"]), ("v", v, 0.0)):
        c_mod = N.componentwise(mod[nm], ref[nm], Bc, E32, T32)[0]
        ck, at = N.componentwise(got, ref[nm], Bc, E32, T32)
        assert ck <= N.limit(c_mod), f"adamw_sr {nm}: kernel c = {ck:.3f} at {at} exceeds {N.limit(c_mod):.3f}"
    x64 = ref["p"]
    # containment: one of the two bf16 neighbours of the fp64 result, widened by the fp32 bound (and by the fp32 rounding of the bracket itself)
    pad = tol + x64.abs() * 2.0 ** -23
    lo_b, hi_b = R.bf16_floor((x64 - pad).float()), R.bf16_ceil((x64 + pad).float())
    out = (p.float() < lo_b) | (p.float() > hi_b)
    assert not bool(out.any()), f"{int(out.sum())} of {n} stored values are not a bf16 neighbour of the fp64 result"
    # prediction: the documented hash applied to the fp32 model's value
    y = mod["p"].float()
    want = R.sr_store(y, KEY, index0)
    miss = R.bf16_bits(want) != R.bf16_bits(p)
    n_miss = int(miss.sum())
    # an exception needs a multiple of the spacing between |y| + r and the kernel's |y'| + r, and both are within tol of the fp64 result
    r = torch.from_numpy(R.sr_fields(n, KEY, index0)).to(dev())
    d = ((R.f32_bits(y) & 0x7FFFFFFF) + r) & 0xFFFF
    dist = torch.minimum(d, 0x10000 - d).double() / 65536  # distance to the store's threshold, in spacings
    if n_miss:
        far = miss & (dist > 2 * tol / R.bf16_spacing(y))
        assert not bool(far.any()), f"{int(far.sum())} stored values differ from the prediction away from their threshold"
    print(f"SR | n={n}+{first} clip={clip} decay={decay} | model c {cm:.3f} | off the prediction {n_miss} of {n} ({n_miss / n:.2e})")
    assert n_miss <= 0.01 * n, (n_miss, n)
    moved = float((R.bf16_bits(p) != R.bf16_bits(p0)).double().mean())
    assert n < 2053 or moved > 0.2, moved  # (the nearest store leaves 43 % untouched at this lr; this one moves each by its share)
    if n == BIG:
        err = float(((p.double() - x64) / R.bf16_spacing(x64.float())).mean())
        bound = 2.5 / math.sqrt(n) + 2.0 ** -12
        print(f"SR | n={n} | mean error {err:.3e} spacings, bound {bound:.3e}")
        assert abs(err) <= bound, (err, bound)


def test_stochastic_is_a_function_of_key_and_arena_index(ops):
    n = 2053
    a = _sr_case(ops, n, 0, True, True)[0]
    assert torch.equal(R.bf16_bits(a), R.bf16_bits(_sr_case(ops, n, 0, True, True)[0]))
    assert not torch.equal(R.bf16_bits(a), R.bf16_bits(_sr_case(ops, n, 0, True, True, key=KEY + 1)[0]))
    assert not torch.equal(R.bf16_bits(a), R.bf16_bits(_sr_case(ops, n, 0, True, True, index0=16)[0]))
    for cut in (4, 1028, 2052):  # two launches split at a multiple of 4 (the second then starts off the 16-byte grid unless cut % 8 == 0)
        assert torch.equal(R.bf16_bits(a), R.bf16_bits(_sr_case(ops, n, 0, True, True, cut=cut)[0])), cut
    # an arena index off the hash's 4-element grid: 16-byte accesses (three hashes per 8 elements) against the element-by-element path
    assert torch.equal(R.bf16_bits(_sr_case(ops, n, 0, True, True, index0=13)[0]), R.bf16_bits(_sr_case(ops, n, 1, True, True, index0=13)[0]))
    big = _sr_case(ops, BIG, 0, False, True)[0]
    assert torch.equal(R.bf16_bits(big), R.bf16_bits(_sr_case(ops, BIG, 0, False, True, cut=4 * 300001)[0]))


# ---- 7. what the feature is for ----------------------------------------------------------------------------------------------------------
def test_400_steps_on_ones_nearest_freezes_split_and_stochastic_follow(ops):
    n, steps = 2053, 400
    gen = torch.Generator().manual_seed(7)
    base = (torch.rand(n, generator=gen) + 0.5) * 1e-2  # constant sign
    z = lambda dt: torch.zeros(n, dtype=dt, device=dev())  # noqa: E731
    st = {k: dict(p=torch.ones(n, dtype=BF16, device=dev()), m=z(F32), v=z(F32)) for k in ("nearest", "split", "sr")}
    lo = z(torch.int16)
    p64, m64, v64 = torch.ones(n, dtype=torch.float64, device=dev()), z(torch.float64), z(torch.float64)
    acc = torch.zeros(n, dtype=torch.float64, device=dev())
    b1, b2, eps = HP["beta1"], HP["beta2"], HP["eps"]
    for step in range(1, steps + 1):
        g = (base * (1 + 0.1 * math.sin(step))).to(BF16).to(dev())
        ops.adamw_(st["nearest"]["p"], g, st["nearest"]["m"], st["nearest"]["v"], LR, b1, b2, eps, 0.0, step)
        ops.adamw_split_(st["split"]["p"], lo, g, st["split"]["m"], st["split"]["v"], LR, b1, b2, eps, 0.0, step)
        ops.adamw_sr_(st["sr"]["p"], g, st["sr"]["m"], st["sr"]["v"], LR, b1, b2, eps, 0.0, step, 1.0, None, R.sr_key(0, step), 0)
        ref = N.adamw_step(p64, g, m64, v64, lr=LR, wd=0.0, step=step, **HP)  # the fp64 recurrence, from its own state
        p64, m64, v64 = ref["p"], ref["m"], ref["v"]
        acc += N.limit(0) * E32 * (ref["p"].abs() + ref["B_p"])  # one fp32 evaluation per step: two roundings of (|p| + B_p)
    assert bool((st["nearest"]["p"] == 1.0).all())  # control: the round-to-nearest store never leaves 1.0
    assert float((p64 - 1).abs().min()) > 0.9 * steps * LR * 0.5 and float(acc.max()) < 0.05 * steps * LR  # the reference moved, the bound is 5 % of it
    master = R.join_bits(st["split"]["p"], lo)
    err = (master.double() - p64).abs()
    assert bool((err <= acc).all()), (float(err.max()), float(acc.max()))
    assert torch.equal(R.bf16_bits(R.split_bits(master)[0]), R.bf16_bits(st["split"]["p"]))
    spacing = 2.0 ** -8  # of bf16 just below 1.0
    bound = 5 * 0.5 * math.sqrt(steps) * spacing / math.sqrt(n)
    got = float(st["sr"]["p"].double().mean()) - float(p64.mean())
    print(f"400 steps | split: worst |master - fp64| {float(err.max()):.3e} (bound {float(acc.max()):.3e}) | stochastic: mean(p) off by {got:.3e} (bound {bound:.3e}) | moved {1 - float(p64.mean()):.3e}")
    assert abs(got) <= bound, (got, bound)


# ---- 8. model level ----------------------------------------------------------------------------------------------------------------------
def _build(cfg, dtype):
    from merlin_amd.model.llama_mmgpt import build_synthetic_model

    llama = dict(vocab_size=cfg.vocab_size - 3, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                 num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                 rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta, max_position_embeddings=8192)
    vision = dict(hidden_size=cfg.v_hidden_size, intermediate_size=cfg.v_intermediate_size, num_hidden_layers=cfg.v_num_hidden_layers,
                  num_attention_heads=cfg.v_num_attention_heads, image_size=cfg.v_image_size, patch_size=cfg.v_patch_size,
                  layer_norm_eps=cfg.v_layer_norm_eps)
    return build_synthetic_model(llama, vision, projector=cfg.projector, conv_stride=cfg.conv_stride, dtype=dtype, device="cuda", seed=0)


def test_model_20_steps_split_master_follows_torch_adamw_on_fp32_masters():
    from oracle import cases as C
    from oracle import llrd_ref
    from merlin_amd import optim as OPT

    cfg, batch = C.get_case("tiny_2img")
    batch = dict(input_ids=batch["input_ids"].cuda(), attention_mask=batch["attention_mask"].cuda(), labels=batch["labels"].cuda(),
                 images=[im.cuda() for im in batch["images"]])
    lr, wd, clip_at, steps = 5e-5, 0.05, 1.0, 20  # pretrain.sh; HF's default max_grad_norm
    hp = dict(lr=lr, betas=(0.9, 0.95), eps=1e-8, weight_decay=wd, lr_scale_fn=OPT.vit_lr_scale)
    model, control = _build(cfg, BF16), _build(cfg, BF16)
    opt, opt_c = OPT.FusedAdamW(model.engine, rounding="split", **hp), OPT.FusedAdamW(control.engine, **hp)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    init = {n: p.detach().clone() for n, p in named}
    master = {n: p.detach().float().clone().requires_grad_(True) for n, p in named}
    groups = llrd_ref.param_groups(named, lr, wd, OPT.vit_lr_scale)
    ref_opt = torch.optim.AdamW([{"params": [master[n] for n in g["names"]], "lr": g["lr"], "weight_decay": g["weight_decay"]} for g in groups],
                                betas=(0.9, 0.95), eps=1e-8)
    for _ in range(steps):
        model(**batch).loss.backward()
        for n, p in named:
            master[n].grad = p.grad.detach().float().clone()  # the HIP gradients, handed to torch AdamW on the fp32 masters
        torch.nn.utils.clip_grad_norm_([master[n] for n, _ in named], clip_at)
        ref_opt.step()
        opt.step(max_grad_norm=clip_at)
        opt.zero_grad()
        control(**batch).loss.backward()
        opt_c.step(max_grad_norm=clip_at)
        opt_c.zero_grad()
    assert opt.reseeds == 0
    for n, p in named:
        ref, got = master[n].detach(), opt.master(n)
        assert got.dtype == F32 and got.shape == p.shape
        slack = steps * 2.0 ** -14 * (ref.abs() + (ref - init[n].float()).abs()) + 1e-12
        bad = (got - ref).abs() > slack
        assert not bool(bad.any()), (n, int(bad.sum()), float((got - ref).abs().max()))
        assert torch.equal(R.bf16_bits(R.split_bits(got)[0].reshape(-1)), R.bf16_bits(p.detach().reshape(-1))), n
    ctl = dict(control.named_parameters())
    lns = [n for n, _ in named if n.endswith("input_layernorm.weight")]
    assert lns
    for n in lns:
        # Adam's first step moves every element with a gradient by lr = 5e-5: 800 fp32 spacings at 1.0, 1/78 of a bf16 one
        assert float((opt.master(n) != init[n].float()).double().mean()) > 0.5, n
        assert torch.equal(R.bf16_bits(ctl[n].detach()), R.bf16_bits(init[n])), n
    # a load between two steps: lo no longer belongs to the weights
    model.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()})
    model(**batch).loss.backward()
    opt.step(max_grad_norm=clip_at)
    assert opt.reseeds == 1
    opt.zero_grad()
    model(**batch).loss.backward()
    opt.step(max_grad_norm=clip_at)
    assert opt.reseeds == 1


# ---- 9. what the ABI refuses -------------------------------------------------------------------------------------------------------------
def test_abi_refusals(ops):
    from merlin_amd import _lib as L

    n = 64
    p, g, lo = (torch.zeros(n, dtype=d, device=dev()) for d in (BF16, BF16, torch.int16))
    m, v = torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    s = torch.cuda.current_stream().cuda_stream
    split = lambda p_, lo_, n_, dt: L.launch("mh_adamw_split", p_, lo_, g, m, v, n_, LR, 0.9, 0.95, 1e-8, WD, 1, 1.0, None, dt, s)  # noqa: E731
    sr = lambda p_, n_, dt: L.launch("mh_adamw_sr", p_, g, m, v, n_, LR, 0.9, 0.95, 1e-8, WD, 1, 1.0, None, 1, 0, dt, s)  # noqa: E731
    assert split(p, lo, n, L.MH_F16) == sr(p, n, L.MH_F16) == L.DEFINES["MH_ERR_DTYPE"]
    assert split(p, None, n, L.MH_BF16) == split(p, lo, 0, L.MH_BF16) == split(None, lo, n, L.MH_BF16) == L.DEFINES["MH_ERR_ARG"]
    assert sr(None, n, L.MH_BF16) == sr(p, 0, L.MH_BF16) == L.DEFINES["MH_ERR_ARG"]
    half = p.to(torch.float16)
    with pytest.raises(L.MerlinHipError, match="dtype"):
        ops.adamw_split_(half, lo, half, m, v, LR, 0.9, 0.95, 1e-8, WD, 1)
    with pytest.raises(L.MerlinHipError, match="dtype"):
        ops.adamw_sr_(half, half, m, v, LR, 0.9, 0.95, 1e-8, WD, 1)
    with pytest.raises(L.MerlinHipError, match="bad argument"):
        ops.adamw_split_(p, None, g, m, v, LR, 0.9, 0.95, 1e-8, WD, 1)
    torch.cuda.synchronize()
    assert not bool(p.any()) and not bool(lo.any()) and not bool(m.any())  # nothing was launched
    assert split(p, lo, n, L.MH_BF16) == sr(p, n, L.MH_BF16) == 0
