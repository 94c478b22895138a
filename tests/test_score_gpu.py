"""model.score() on the GPU: mh_attn_extend_branches / _kv8 per element against the fp64 reference and its rounding model (the scheme of
tests/test_session_gpu.py::test_attn_extend_per_element) and bit for bit against rows of other candidates, mh_token_logprobs against fp64
log_softmax and first-index argmax, engine.extend_branches against per-candidate prefill + teacher-forced decode steps with a bound measured
in the same run, and model.score against those rows, against transformers, through a session and on degenerate inputs."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import numerics as N  # noqa: E402
from test_kv8_cpu import kv8_dequantize, kv8_quantize  # noqa: E402
from test_kv8_gpu import GAIN, _dev, hold, rnd_rows  # noqa: E402
from test_session_gpu import _measured, _toks  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
FILL = 0.3125


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def O():
    from merlin_amd import ops

    assert ops.arch_ok(0), "not a gfx950 device"
    return ops


def _seg_start(segs):
    out = []
    for n in segs:
        out += [len(out)] * n
    return out


# ---- attention kernel ----------------------------------------------------------------------------------------------------------------------
# (P, segment lengths, H, D, Smax): one row and one prefix key; every query sees the prefix and itself only; P inside a key tile with
# segment boundaries inside a wave's 16 queries; P on a tile boundary with a segment spanning two query tiles, the second tile partial and a
# one-row segment between the others; no prefix; a long prefix ending in a partial tile with unused rows behind the cache's valid rows
BRANCH_CASES = [(1, [1], 2, 128, 40), (5, [1, 1, 1, 1], 2, 64, 32), (37, [17, 3, 30], 4, 64, 128), (64, [70, 1, 25], 2, 128, 200),
                (0, [33, 40], 2, 64, 80), (300, [5, 5, 5], 4, 64, 700)]


def _branch_inputs(dtype, P, segs, H, D, Smax, seeds=(3, 4)):
    d, R = H * D, sum(segs)
    q = rnd_rows(R * H, D, dtype, seed=5, lo=0.5, hi=2.0).view(R, d).to(dev())
    cache = []
    for seed in seeds:
        c8, cs = kv8_quantize(rnd_rows(Smax * H, D, dtype, seed=seed).view(1, Smax, H, D))
        cache += [c8.view(1, Smax, d).to(dev()), cs.permute(0, 2, 1).contiguous().to(dev()), kv8_dequantize(c8, cs).to(dev())]
    k8, ks, k64, v8, vs, v64 = cache
    k16, v16 = k64.to(dtype).view(1, Smax, d), v64.to(dtype).view(1, Smax, d)
    assert torch.equal(k16.double().view_as(k64), k64) and torch.equal(v16.double().view_as(v64), v64)  # the cast to the 16-bit type is exact
    return q, k8, ks, k64, v8, vs, v64, k16, v16


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,segs,H,D,Smax", BRANCH_CASES)
def test_attn_extend_branches_per_element(O, dtype, P, segs, H, D, Smax):
    """Query r is held to N.attention_decode on its gathered visible keys - the P prefix rows, then cache rows P + seg_start[r] .. P + r -
    of the dequantised cache, with the limit of the rounding model on the same inputs (hold() of tests/test_kv8_gpu.py): the fp8 form on
    the fp8 cache and the 16-bit form on the exactly cast dequantised cache.  The output [R, H*D] is carved out of a larger patterned
    buffer whose rows behind it must keep the pattern."""
    d, R = H * D, sum(segs)
    assert P + R <= Smax
    q, k8, ks, k64, v8, vs, v64, k16, v16 = _branch_inputs(dtype, P, segs, H, D, Smax)
    seg = _seg_start(segs)
    vis = [list(range(P)) + list(range(P + seg[r], P + r + 1)) for r in range(R)]
    pairs = [N.attention_decode(q[r].view(H, D), k64[0][vis[r]], v64[0][vis[r]], len(vis[r])) for r in range(R)]
    ref, Bc = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    mod = torch.stack([N.attention_decode(q[r].view(H, D), k64[0][vis[r]], v64[0][vis[r]], len(vis[r]), model=dtype) for r in range(R)])
    seg_t = torch.tensor(seg, dtype=torch.int32, device=dev())
    tag = f"P={P} segs={segs} Smax={Smax}"
    guard = 3
    for name, run in (("kv8", lambda out: O.attn_extend_branches_kv8(q, k8, v8, ks, vs, seg_t, P, H, D, out=out)),
                      ("16-bit", lambda out: O.attn_extend_branches(q, k16, v16, seg_t, P, H, D, out=out))):
        buf = torch.full((R + guard, d), FILL, dtype=dtype, device=dev())
        o = run(buf[:R])
        assert o.data_ptr() == buf.data_ptr()
        hold(f"attention extend branches {name} {tag}", dtype, o.view(R, H, D), ref, Bc, mod)
        assert bool((buf[R:] == FILL).all()), f"{name}: rows behind the output were written"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,segs,H,D,Smax", [BRANCH_CASES[2], BRANCH_CASES[3]])
def test_attn_extend_branches_isolates_the_candidates_bit_for_bit(O, dtype, P, segs, H, D, Smax):
    """A second run with the K and V rows (fp8: bytes and scales) of every segment but one replaced by other finite random values: the
    output rows of the untouched segment are bit-identical to the first run's.  Repeated for each segment, both cache forms."""
    d, R = H * D, sum(segs)
    q, k8, ks, _, v8, vs, _, k16, v16 = _branch_inputs(dtype, P, segs, H, D, Smax)
    _, k8b, ksb, _, v8b, vsb, _, k16b, v16b = _branch_inputs(dtype, P, segs, H, D, Smax, seeds=(13, 14))
    assert not torch.equal(k16, k16b) and not torch.equal(k8, k8b)
    seg_t = torch.tensor(_seg_start(segs), dtype=torch.int32, device=dev())
    first16 = O.attn_extend_branches(q, k16, v16, seg_t, P, H, D)
    first8 = O.attn_extend_branches_kv8(q, k8, v8, ks, vs, seg_t, P, H, D)
    assert bool(torch.isfinite(first16.float()).all()) and bool(torch.isfinite(first8.float()).all())
    start = 0
    for n in segs:
        other = torch.ones(Smax, dtype=torch.bool, device=dev())
        other[:P] = False
        other[P + R:] = False
        other[P + start:P + start + n] = False  # rows of the other segments: True
        assert int(other.sum()) == R - n

        def swap(a, b, scales=False):
            out = a.clone()
            if scales:
                out[:, :, other] = b[:, :, other]
            else:
                out[:, other] = b[:, other]
            return out

        o16 = O.attn_extend_branches(q, swap(k16, k16b), swap(v16, v16b), seg_t, P, H, D)
        o8 = O.attn_extend_branches_kv8(q, swap(k8, k8b), swap(v8, v8b), swap(ks, ksb, True), swap(vs, vsb, True), seg_t, P, H, D)
        rows = slice(start, start + n)
        assert torch.equal(o16[rows].view(torch.int16), first16[rows].view(torch.int16)), ("16-bit", start, n)
        assert torch.equal(o8[rows].view(torch.int16), first8[rows].view(torch.int16)), ("kv8", start, n)
        if R - n > 1:  # the replaced rows did change the other segments' outputs: the second run is not the first
            assert not torch.equal(o16, first16) and not torch.equal(o8, first8)
        start += n


def test_attn_extend_branches_refuses_bad_arguments(O):
    from merlin_amd._lib import MerlinHipError

    H, D, Smax = 2, 64, 32
    q = torch.zeros(4, H * D, dtype=torch.float16, device=dev())
    k = torch.zeros(1, Smax, H * D, dtype=torch.float16, device=dev())
    seg = torch.zeros(3, dtype=torch.int32, device=dev())
    with pytest.raises(MerlinHipError, match="bad argument"):
        O.attn_extend_branches(q.view(-1)[1:1 + 3 * H * D].view(3, H * D), k, k, seg, 5, H, D)  # q rows not 16-byte aligned
    with pytest.raises(MerlinHipError, match="bad argument"):
        O.attn_extend_branches(q[:3], k, k, seg, Smax - 2, H, D)  # P + R > Smax
    k8 = torch.zeros(1, Smax, H * D, dtype=torch.uint8, device=dev())
    sc = torch.ones(1, H, Smax, device=dev())
    with pytest.raises(MerlinHipError, match="bad argument"):
        O.attn_extend_branches_kv8(q[:3], k8, k8, sc, sc, seg, Smax - 2, H, D)
    with pytest.raises(MerlinHipError, match="shape not supported"):
        O.attn_extend_branches(torch.zeros(3, 2 * 32, dtype=torch.float16, device=dev()), torch.zeros(1, Smax, 64, dtype=torch.float16, device=dev()),
                               torch.zeros(1, Smax, 64, dtype=torch.float16, device=dev()), seg, 4, 2, 32)  # D = 32


# ---- mh_token_logprobs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,ldl", [(32003, 32064), (40, 40), (1000, 1008)])
@pytest.mark.parametrize("R", [1, 5, 300])
def test_token_logprobs_against_fp64_log_softmax_and_first_index_argmax(O, R, V, ldl):
    """logits randn * 3 with every third row scaled by 25; row 0's maximum occurs twice.  logprob against fp64 log_softmax of the same fp32
    logits under the bound the repository asserts for mh_log_softmax_rows (1e-4 absolute, tests/test_generation_gpu.py:93: the same
    arithmetic), greedy exactly against argmax with first-index tie-breaking - the target on the second occurrence of the maximum gives 0,
    on the first 1.  Columns [V, ldl) hold the largest value of the buffer; the guard elements around both outputs keep their pattern."""
    g = torch.Generator().manual_seed(R + V)
    x = torch.randn(R, ldl, generator=g) * 3
    x[::3] *= 25
    i1, i2 = 7, V - 2
    x[0, i1] = x[0, i2] = x[0, :V].max() + 1.5
    x[:, V:] = x.abs().max() + 10.0
    tg = torch.randint(0, V, (R,), generator=g)
    tg[1::2] = x[1::2, :V].argmax(-1)  # every second row's target is its argmax: greedy = 1 there
    ref = torch.log_softmax(x[:, :V].double(), -1)
    am = torch.stack([(row == row.max()).nonzero()[0, 0] for row in x[:, :V]])
    assert int(am[0]) == i1
    xd = x.to(dev())
    for t0, g0 in ((i2, 0), (i1, 1)):
        tg[0] = t0
        lp_buf = torch.full((R + 4,), FILL, device=dev())
        gr_buf = torch.full((R + 4,), -7, dtype=torch.int32, device=dev())
        lp, gr = O.token_logprobs(xd, tg.to(dev()), V, logprob=lp_buf[2:2 + R], greedy=gr_buf[2:2 + R])
        want = ref.gather(1, tg[:, None])[:, 0]
        err = float((lp.cpu().double() - want).abs().max())
        print(f"SCORE | token_logprobs | R = {R} V = {V} ldl = {ldl} | max |d logprob| = {err:.3e} | bound = 1e-4")
        assert err < 1e-4
        assert gr.cpu().tolist() == (am == tg).int().tolist() and int(gr[0]) == g0
        assert bool((lp_buf[:2] == FILL).all()) and bool((lp_buf[2 + R:] == FILL).all()), "logprob: guard elements were written"
        assert bool((gr_buf[:2] == -7).all()) and bool((gr_buf[2 + R:] == -7).all()), "greedy: guard elements were written"


def test_token_logprobs_one_row_many_targets_and_a_target_out_of_range(O):
    """Row stride 0 (one row of logits, several targets: the first token of every candidate) equals the same row repeated; a target outside
    [0, V) gives NaN and 0 and leaves the other rows as they are."""
    V = 103
    x = (torch.randn(1, 128, generator=torch.Generator().manual_seed(1)) * 3).to(dev())
    tg = torch.tensor([5, 17, int(x[0, :V].argmax()), 102], device=dev())
    lp, gr = O.token_logprobs(x.expand(4, -1), tg, V)
    lp2, gr2 = O.token_logprobs(x.repeat(4, 1), tg, V)
    assert torch.equal(lp, lp2) and torch.equal(gr, gr2) and gr.tolist() == [0, 0, 1, 0]
    bad = torch.tensor([5, V, -1, 102], device=dev())
    lp3, gr3 = O.token_logprobs(x.repeat(4, 1), bad, V)
    assert bool(torch.isnan(lp3[1:3]).all()) and gr3[1:3].tolist() == [0, 0]
    assert torch.equal(lp3[[0, 3]], lp[[0, 3]]) and torch.equal(gr3[[0, 3]], gr[[0, 3]])


# ---- engine --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture(dtype):
    from test_kv8_gpu import _tiny

    return _tiny(dtype)


def _text(m, toks):
    """Token ids as a list with the three image token ids replaced by a plain text id (continuations are text only)."""
    special = {m.im_start_token, m.im_end_token, m.im_patch_token}
    return [5 if t in special else int(t) for t in (toks.tolist() if isinstance(toks, torch.Tensor) else toks)]


def _cands(m, V):
    """Three candidates of lengths 9, 1 and 14: random tokens from test_session_gpu._toks."""
    return [_text(m, _toks(V, n, seed=seed)) for n, seed in ((9, 21), (1, 22), (14, 23))]


_ARM_A = {}


def _arm_a(dtype, kv8, cand):
    """Arm (a) for one candidate: a fresh prefill, then teacher-forced decode_steps -> fp32 logits [n, V], row j scores token j (row 0 is
    the prompt's last position; the candidate's last token is never fed).  Computed once and shared."""
    key = (dtype, kv8, tuple(cand))
    if key not in _ARM_A:
        cfg, m, ids, images = _fixture(dtype)
        eng, V = m.engine, cfg.vocab_size
        lg, cache = eng.prefill(ids, None, images, len(cand) + 1, kv_fp8=kv8)
        rows = [lg[:, :V].clone()]
        for t in cand[:-1]:
            rows.append(eng.decode_step(torch.tensor([t], device=ids.device), cache)[:, :V].clone())
        _ARM_A[key] = torch.cat(rows)
    return _ARM_A[key]


def _bound(dtype, kv8):
    _, _, d_pre, d_rows = _measured(dtype, kv8)
    return 2 * max(d_pre, d_rows), d_pre, d_rows


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("kv8", [False, True], ids=["kv16", "kv8"])
def test_extend_branches_reproduces_per_candidate_decode_steps(dtype, kv8):
    """Candidates of 9, 1 and 14 tokens.  (a) per candidate a fresh prefill and teacher-forced decode_steps; (b) ONE extend_branches over
    the 8 + 0 + 13 packed rows.  Every row deviates by <= 2 max(d_pre, d_rows), both measured in this run by test_session_gpu._measured
    (the rule and the factor of test_extend_reproduces_sequential_decode_steps); cache.lens stays P, and a following decode_step on the
    cache gives the logits of a decode_step on a fresh prefill under the same bound."""
    from merlin_amd.scoring import _branch_plan

    cfg, m, ids, images = _fixture(dtype)
    eng, V, P = m.engine, cfg.vocab_size, ids.shape[1]
    cands = _cands(m, V)
    plan = _branch_plan(cands)
    R = len(plan.fed)
    assert R == 21 and plan.offsets == [0, 8, 8, 21]
    bound, d_pre, d_rows = _bound(dtype, kv8)
    _, cb = eng.prefill(ids, None, images, R + 2, kv_fp8=kv8)
    hn, lb = eng.extend_branches(cb, plan, return_logits=True)
    assert lb.shape == (R, V) and lb.dtype == torch.float32 and hn.shape == (R, cfg.hidden_size) and int(cb.lens[0]) == P
    worst = 0.0
    for c, cand in enumerate(cands):
        a = _arm_a(dtype, kv8, cand)
        for j in range(len(cand) - 1):
            worst = max(worst, _dev([lb[plan.offsets[c] + j][None]], [a[j + 1][None]], V))
    nxt = _toks(V, 1, seed=12)
    lb_next = eng.decode_step(nxt, cb).clone()
    assert int(cb.lens[0]) == P + 1
    _, cf = eng.prefill(ids, None, images, 2, kv_fp8=kv8)
    d_next = _dev([lb_next], [eng.decode_step(nxt, cf).clone()], V)
    print(f"SESSION | extend_branches | {'fp8' if kv8 else '16-bit'} cache | {str(dtype)[6:]} | d_pre = {d_pre:.3e} | d_rows = {d_rows:.3e} | "
          f"worst dev(b row, a row) = {worst:.3e} | dev(next step) = {d_next:.3e} | bound = {bound:.3e}")
    assert worst <= bound and d_next <= bound, (worst, d_next, bound)
    with pytest.raises(ValueError, match="grow_cache"):
        eng.extend_branches(eng.prefill(ids, None, images, R - 1, kv_fp8=kv8)[1], plan)
    import dataclasses

    broken = plan.seg_start.clone()
    broken[10] = 9  # a segment start that is neither the row itself nor its predecessor's: refused on the host, before the kernel reads it
    with pytest.raises(ValueError, match="seg_start"):
        eng.extend_branches(cb, dataclasses.replace(plan, seg_start=broken), pos=P)
    with pytest.raises(ValueError):
        eng.extend_branches(eng.prefill(ids.repeat(2, 1), None, images * 2, R, kv_fp8=kv8)[1], plan)


# ---- model.score ---------------------------------------------------------------------------------------------------------------------------
def _check_against_arm_a(out, cands, dtype, kv8, tag):
    """Token log-probs against fp64 log_softmax of arm (a)'s rows: <= 2 * bound * ||a_row||_2 per token.  Derived, not chosen: a
    log-probability moves by at most twice the largest logit change, which is at most the L2 change, which _dev bounds relative to the
    row's norm.  logprobs equals the sum of token_logprobs exactly."""
    bound, _, _ = _bound(dtype, kv8)
    worst = 0.0
    for c, cand in enumerate(cands):
        a = _arm_a(dtype, kv8, cand).double().cpu()
        want = torch.log_softmax(a, -1).gather(1, torch.tensor(cand)[:, None])[:, 0]
        lim = 2 * bound * a.norm(dim=1)
        got = out.token_logprobs[c]
        assert got.shape == (len(cand),) and got.dtype == torch.float32
        err = (got.double() - want).abs()
        worst = max(worst, float((err / lim).max()))
        assert bool((err <= lim).all()), (tag, c, err.tolist(), lim.tolist())
        assert float(out.logprobs[c]) == float(got.sum())
    print(f"SCORE | {tag} | {'fp8' if kv8 else '16-bit'} cache | {str(dtype)[6:]} | worst |d logprob| / (2 bound ||a row||) = {worst:.3e} | bound = {bound:.3e}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("kv8", [False, True], ids=["kv16", "kv8"])
def test_score_against_per_candidate_decode_steps(dtype, kv8):
    cfg, m, ids, images = _fixture(dtype)
    V, P = cfg.vocab_size, ids.shape[1]
    cands = _cands(m, V)
    out = m.score(ids, [cands[0], torch.tensor(cands[1]), tuple(cands[2])], images=images, fp8_kv=kv8)
    assert out.stats == dict(prompt_tokens_run=P, prompt_tokens_reused=0, rows=21, images_encoded=sum(im.shape[0] for im in images))
    assert out.logprobs.shape == (3,) and out.logprobs.dtype == torch.float32 and out.is_greedy.shape == (3,) and out.is_greedy.dtype == torch.bool
    _check_against_arm_a(out, cands, dtype, kv8, "score vs arm (a)")
    # C = 1 with n = 40
    long = [_text(m, _toks(V, 40, seed=31))]
    one = m.score(ids, long, images=images, fp8_kv=kv8)
    assert one.stats["rows"] == 39
    _check_against_arm_a(one, long, dtype, kv8, "score C = 1, n = 40")


_HF = {}


def _hf_logits(seq):
    """fp32 transformers logits [len(seq), V] of the text-only form of the tiny model with the fixture's logit gain, on the CPU."""
    from oracle import cases as C
    from oracle.make_gen_golden import hf_llama

    if "m" not in _HF:
        _HF["m"] = hf_llama(C.get_case("tiny_1img")[0], GAIN)
    with torch.no_grad():
        return _HF["m"](torch.tensor([seq], dtype=torch.int64)).logits[0].float()


def _hf_candidates(m, prompt, V):
    """Three candidates chosen on the CPU model: its most likely text continuation of 5 tokens, that continuation with its last two tokens
    replaced, and 7 random tokens - the first is far more likely than the others, so the ranking of the top two is decisive."""
    special = [m.im_start_token, m.im_end_token, m.im_patch_token]
    best = []
    for _ in range(5):
        lg = _hf_logits(prompt + best)[-1, :V].clone()
        lg[special] = -float("inf")
        best.append(int(lg.argmax()))
    return [best, best[:3] + _text(m, _toks(V, 2, seed=41)), _text(m, _toks(V, 7, seed=42))]


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 1e-3), (torch.bfloat16, 1.5e-2)], ids=["float16", "bfloat16"])
def test_score_against_transformers(dtype, tol):
    """Two text-only prompts of tests/test_bans_gpu.py with three candidates each against transformers' fp32 LlamaForCausalLM on the CPU:
    |d token logprob| <= 2 tol max|ref logits of the row| (tol = the bound DESIGN section 4 asserts for tiny-case logits), and the
    ranking of logprobs equals transformers' for every pair whose reference sums differ by more than twice the larger summed per-token
    bound; the top two are such a pair in at least one case."""
    from test_bans_gpu import PROMPTS

    cfg, m, _, _ = _fixture(dtype)
    V = cfg.vocab_size
    decisive = 0
    for prompt in (PROMPTS[1], PROMPTS[3]):
        cands = _hf_candidates(m, prompt, V)
        out = m.score(torch.tensor([prompt], dtype=torch.int64).cuda(), cands)
        assert out.stats == dict(prompt_tokens_run=len(prompt), prompt_tokens_reused=0, rows=sum(len(c) - 1 for c in cands), images_encoded=0)
        sums, lims = [], []
        for c, cand in enumerate(cands):
            ref = _hf_logits(prompt + cand[:-1])[len(prompt) - 1:, :V].double()
            want = torch.log_softmax(ref, -1).gather(1, torch.tensor(cand)[:, None])[:, 0]
            lim = 2 * tol * ref.abs().amax(dim=1)
            err = (out.token_logprobs[c].double() - want).abs()
            print(f"SCORE | vs transformers | {str(dtype)[6:]} | P = {len(prompt)} cand {c} | max |d logprob| = {float(err.max()):.3e} | "
                  f"min bound = {float(lim.min()):.3e} | ref sum = {float(want.sum()):.3f} | got = {float(out.logprobs[c]):.3f}")
            assert bool((err <= lim).all()), (c, err.tolist(), lim.tolist())
            sums.append(float(want.sum()))
            lims.append(float(lim.sum()))
        got = out.logprobs.tolist()
        for i in range(3):
            for j in range(i + 1, 3):
                if abs(sums[i] - sums[j]) > 2 * max(lims[i], lims[j]):
                    assert (got[i] > got[j]) == (sums[i] > sums[j]), (i, j, got, sums)
        order = sorted(range(3), key=lambda c: -sums[c])
        if sums[order[0]] - sums[order[1]] > 2 * max(lims[order[0]], lims[order[1]]):
            decisive += 1
            assert int(out.logprobs.argmax()) == order[0]
    assert decisive >= 1, "no case whose top two reference sums differ by more than twice the summed bound"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_score_is_greedy(dtype):
    """The model's own greedy continuation of 8 tokens is greedy (or the offending step's top two lie within the 2e-3 rule of
    test_generation_gpu._same_or_tie); with one token replaced by a non-argmax token it is not."""
    from test_bans_gpu import PROMPTS

    cfg, m, ids0, images0 = _fixture(dtype)
    V = cfg.vocab_size
    # the fixture's own prompt continues with an image patch token, which a candidate may not hold: the first prompt (the fixture's, then
    # the text-only ones of tests/test_bans_gpu.py) whose greedy continuation of 8 tokens is text
    for ids, images in [(ids0, images0)] + [(torch.tensor([p], dtype=torch.int64).cuda(), None) for p in PROMPTS]:
        P = ids.shape[1]
        seq = m.generate(ids, images=images, max_new_tokens=8, do_sample=False, eos_token_id=-1, pad_token_id=0)
        cand = seq[0, P:].tolist()
        if cand == _text(m, cand):
            break
    else:
        raise AssertionError("no prompt with a text-only greedy continuation")
    assert len(cand) == 8
    with torch.no_grad():
        lg = m(input_ids=seq[:, :-1], images=images).logits[0, P - 1:, :V].float()  # row j chooses token j of the candidate
    low = lg[4].clone()
    low[[m.im_start_token, m.im_end_token, m.im_patch_token]] = float("inf")
    bad = list(cand)
    bad[4] = int(low.argmin())  # the least likely text token at step 4
    assert bad[4] != cand[4] and bad[4] != int(lg[4].argmax())
    out = m.score(ids, [cand, bad], images=images)
    if not bool(out.is_greedy[0]):
        gaps = [(float(lg[j].max() - lg[j, cand[j]]), 2e-3 * float(lg[j].abs().max())) for j in range(8)]
        assert all(g < lim for g, lim in gaps), ("the greedy continuation is not greedy away from a tie", gaps)
    assert not bool(out.is_greedy[1])
    assert float(out.logprobs[0]) > float(out.logprobs[1])


@pytest.mark.parametrize("kv8", [False, True], ids=["kv16", "kv8"])
def test_score_through_a_session(kv8):
    """score twice on one session with different candidates: the second call runs one prompt token (generate's capped reuse rule) and no
    image, the session holds exactly the prompt, and the results are those of a session-less call under the engine bound; then
    generate(session=s) gives the tokens of a fresh generate or differs only at a tie."""
    from test_spec_gpu import _same_or_greedy_tie

    dtype = torch.float16
    cfg, m, ids, images = _fixture(dtype)
    V, P = cfg.vocab_size, ids.shape[1]
    cands = _cands(m, V)
    s = m.new_session(capacity=128, fp8_kv=kv8)
    first = m.score(ids, [[7, 8, 9], [10]], images=images, fp8_kv=kv8, session=s)
    assert first.stats == dict(prompt_tokens_run=P, prompt_tokens_reused=0, rows=2, images_encoded=sum(im.shape[0] for im in images))
    assert int(s.cache.lens[0]) == P and s.tokens == ids[0].tolist()
    out = m.score(ids, cands, images=images, fp8_kv=kv8, session=s)
    assert out.stats == dict(prompt_tokens_run=1, prompt_tokens_reused=P - 1, rows=21, images_encoded=0), out.stats
    assert int(s.cache.lens[0]) == P and s.tokens == ids[0].tolist() and s.cache.fp8 == kv8
    _check_against_arm_a(out, cands, dtype, kv8, "score(session), second call")
    plain = m.score(ids, cands, images=images, fp8_kv=kv8)
    bound, _, _ = _bound(dtype, kv8)
    worst = 0.0
    for c, cand in enumerate(cands):  # the session call against the session-less call, under the engine bound
        lim = 2 * bound * _arm_a(dtype, kv8, cand).double().cpu().norm(dim=1)
        err = (out.token_logprobs[c] - plain.token_logprobs[c]).abs().double()
        worst = max(worst, float((err / lim).max()))
        assert bool((err <= lim).all()), (c, err.tolist(), lim.tolist())
    print(f"SCORE | score(session) vs session-less | {'fp8' if kv8 else '16-bit'} cache | worst |d logprob| / (2 bound ||a row||) = {worst:.3e}")
    kw = dict(images=images, max_new_tokens=8, eos_token_id=-1, pad_token_id=0, fp8_kv=kv8)
    got = m.generate(ids, session=s, **kw)
    assert s.last == dict(reused_tokens=P - 1, run_tokens=1, images_encoded=0), s.last
    _same_or_greedy_tie(m, ids, None, images, got, m.generate(ids, **kw), kv8)
    with pytest.raises(ValueError, match="fp8_kv"):
        m.score(ids, cands, images=images, fp8_kv=not kv8, session=s)


def test_degenerate_inputs_and_untouched_modes_at_the_library_boundary(monkeypatch):
    """The launch symbols recorded at L.call: one candidate of one token (R = 0) scores from the prefill's logits alone - no
    mh_attn_extend_branches launch; a candidate set with rows launches it once per layer; a plain generate reaches neither new symbol."""
    from merlin_amd import _lib as L

    cfg, m, ids, images = _fixture(torch.float16)
    V = cfg.vocab_size
    names = []
    real = L.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(L, "call", recording)
    one = m.score(ids, [[9]], images=images)
    assert one.stats["rows"] == 0 and one.token_logprobs[0].shape == (1,) and float(one.logprobs[0]) == float(one.token_logprobs[0][0])
    assert not any(n.startswith("mh_attn_extend") for n in names) and names.count("mh_token_logprobs") == 1
    a = torch.log_softmax(_arm_a(torch.float16, False, _cands(m, V)[0])[0].double(), -1)
    assert abs(float(one.logprobs[0]) - float(a[9])) < 1e-4  # the same prefill logits, mh_token_logprobs' own bound
    del names[:]
    m.score(ids, [[9, 10, 11], [12, 13]], images=images)
    assert names.count("mh_attn_extend_branches") == cfg.num_hidden_layers and "mh_attn_extend" not in names
    assert names.count("mh_token_logprobs") == 2
    del names[:]
    for extra in (dict(), dict(use_graph=False), dict(num_beams=3), dict(session=m.new_session())):
        m.generate(ids, images=images, max_new_tokens=4, eos_token_id=-1, pad_token_id=0, **extra)
    assert names and not any(n.startswith("mh_attn_extend_branches") or n == "mh_token_logprobs" for n in names)
