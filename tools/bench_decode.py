"""Decode-step timing of the KV-cache path at Llama-7B size (run on the GPU box): prefill a cfg-3 style prompt, then time
decode steps eagerly and (optionally) as a replayed HIP graph.  Reports ms/token and the HBM rate the step sustains
(weights + K/V cache streamed once per step).  The graph replay runs with 16-bit, fp8 (e4m3, one scale per 128 k) and MXFP4 (e2m1, one scale
byte per 32 k) weights in turn; every such line also carries `weights_tb_s`, the weight bytes of its format over the step time.

    python tools/bench_decode.py [B] [context] [--kv fp8] [--verify | --beams | --extend | --bans | --score | --guidance]

--kv fp8: the KV cache as e4m3 bytes + power-of-two scales (prefill(kv_fp8=True)); the HBM figure counts the bytes of the cache format
in use.  Every arm also reports the time of one decode-attention launch (mh_attn_decode / mh_attn_decode_kv8 + the split merge), replayed
from a HIP graph over the 32 layers' caches in turn so that no launch finds its keys in a cache.

--verify: the verify arm instead (prompt-lookup speculative decoding): for 16-bit, fp8 and MXFP4 weights, the plain decode step and the
verify step (engine.verify_step, T rows of one sequence) at T = 2, 4, 8, 16, each replayed from its HIP graph on the same cache, with the
break-even acceptance t_verify / t_plain - 1 (extra tokens a verify step must yield to pay for itself); then one mh_attn_decode_multi
launch at T = 8 against eight one-query launches, both from graphs over the 32 layers' caches.

--beams: the beam-search arm instead (num_beams = 5, one prompt, eager steps as generate() runs them): for 16-bit, fp8 and MXFP4 weights, a
beam step = re-order + decode_step, on the expanded cache (engine.expand_cache + reorder_cache: share_prompt_kv=False, the yardstick) and
on the shared prompt cache (engine.share_cache + BeamKVCache.reorder: share_prompt_kv=True), same box, same process, same beam_idx per
step.  Per arm: median ms of the step and of its re-order and decode parts, one attention launch (from a graph over the 32 layers, as
above), and the resident cache bytes.  --new G (default 24): room for G generated tokens per beam, as max_new_tokens = G gives it; above
24 the timed steps are the LAST 16 of such a run (G - 20 generated keys are taken as written, whatever they hold).

--extend: the session arm instead (generate(session=...): continuing a kept KV cache), B = 1, one process per (context, cache format): a
prompt of one image and text, context + n tokens.  For each n (--n a,b,c; default 32,64,512 at context 613, else 64), in this process:
the prefill of all context + n tokens with the tower for the image (what a call without a session runs; timed as it is, with its cache
allocation, and into an existing cache), engine.extend of the last n tokens on a cache that holds the first `context` (image included), and
one mh_attn_extend launch alone (from a graph over the 32 layers' caches).  Medians of 7 runs after 2 warm-ups, each between two events.

--bans: the token-ban arm instead (generate(no_repeat_ngram_size=3, bad_words_ids=<64 words>, min_new_tokens=...)), B = 1: the graph decode
step + the selection as generate() runs them per token (graph replay, mh_select_tokens greedy, the token copied back), without and with the
one mh_ban_tokens launch in front of the selection, over a history of `context` tokens.  The two arms alternate step by step in the same
process on the same cache (cache.lens put back before each), every step between its own events, after warm-up; medians.  Then the
mh_ban_tokens and mh_select_tokens launches alone, each replayed from a graph of 32 launches.

--score: the scoring arm instead (model.score: the log-likelihoods of C candidate continuations of n tokens each on one prompt), B = 1, one
process per (context, cache format): a prompt of one image and text, `context` tokens.  For (C, n) = (4, 2), (4, 8), (16, 32) (--cn
"C:n,C:n"), three arms that alternate in this process, every run between its own events after a warm-up, medians of 5 (min and max of the two whole-call arms are printed too): (i) model.score - without
a session (the whole prompt runs) and on a session that holds the prompt (one prompt token runs: the candidates' pass alone); (ii) what the
API offered before score: a session prefill, then per candidate engine.extend of its fed tokens, lm_head on its rows and log_softmax_rows
through the existing ops, cache.truncate - after session.reset() and on the held prompt (extend hands out the last row's logits only, so
the lm_head of the other n - 2 rows runs on a stand-in hidden-state buffer: the same launches on the same shapes); (iii) C full forward
calls of prompt + candidate with the log-softmax of the candidate's rows.  Then the attention launches per layer of (i) and (ii), counted
at the library boundary, and one mh_attn_extend_branches launch on the R = C (n - 1) packed rows against the C mh_attn_extend launches it
replaces, each from a graph over the 32 layers' caches.

--guidance: the classifier-free guidance arm instead (generate(guidance_scale=g, negative_prompt_ids=...)), B = 1: the plain decode step on
the prompt's cache against the guided step - the B = 2 step on engine.pair_cache(prompt cache, negative prompt's cache) plus the one
mh_guidance_mix launch on its two rows of logits, in place, as generate() runs it per token.  The negative prompt is the prompt without
its first 576 tokens (an image span: context 613 leaves 37 tokens of text).  Both as replayed HIP graphs (the mix launched behind the
replay) and as eager steps; the four arms alternate step by step in this process (the lengths put back before each), every step between
its own events, after warm-up; medians, and guided / plain of each pair.  Then the mix launch alone, replayed from a graph of 32."""
import sys, os, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from merlin_amd.model.llama_mmgpt import build_synthetic_model
from merlin_amd import synth

from merlin_amd import ops as _O
if os.environ.get("MH_GEMV_MFMA_MIN"):  # A/B: 17 = never use the MFMA GEMV
    _O.gemv_mfma_min_rows(int(os.environ["MH_GEMV_MFMA_MIN"]))
if os.environ.get("MH_GEMV_PAIR_MIN"):  # A/B: "rows16,rows_fp8" from which the SwiGLU / RoPE projections use the MFMA form
    _O.gemv_mfma_pair_min_rows(*[int(a) for a in os.environ["MH_GEMV_PAIR_MIN"].split(",")])
if os.environ.get("MH_GEMV_MFMA_WIDE"):  # A/B: 0 = 8 waves per block in the small-N MFMA GEMV
    _O.gemv_mfma_wide(os.environ["MH_GEMV_MFMA_WIDE"] != "0")
if os.environ.get("MH_GEMV_KSPLIT"):  # A/B: 0 = one wave per row pair in the small-N GEMV
    _O.gemv_ksplit(os.environ["MH_GEMV_KSPLIT"] != "0")
KV8 = False
if "--kv" in sys.argv:
    _i = sys.argv.index("--kv")
    if sys.argv[_i + 1] not in ("fp8", "16"):
        raise SystemExit("--kv takes fp8 or 16")
    KV8 = sys.argv[_i + 1] == "fp8"
    del sys.argv[_i:_i + 2]
KV = "fp8" if KV8 else "16-bit"
VERIFY = "--verify" in sys.argv
if VERIFY:
    sys.argv.remove("--verify")
BEAMS = "--beams" in sys.argv
if BEAMS:
    sys.argv.remove("--beams")
EXTEND = "--extend" in sys.argv
if EXTEND:
    sys.argv.remove("--extend")
BANS = "--bans" in sys.argv
if BANS:
    sys.argv.remove("--bans")
GUIDANCE = "--guidance" in sys.argv
if GUIDANCE:
    sys.argv.remove("--guidance")
SCORE = "--score" in sys.argv
if SCORE:
    sys.argv.remove("--score")
SCORE_CN = [(4, 2), (4, 8), (16, 32)]
if "--cn" in sys.argv:  # --score: the candidate sets, "C:n,C:n"
    _i = sys.argv.index("--cn")
    SCORE_CN = [tuple(int(v) for v in a.split(":")) for a in sys.argv[_i + 1].split(",")]
    del sys.argv[_i:_i + 2]
EXTEND_NS = None
if "--n" in sys.argv:  # --extend: the tail lengths
    _i = sys.argv.index("--n")
    EXTEND_NS = [int(a) for a in sys.argv[_i + 1].split(",")]
    del sys.argv[_i:_i + 2]
BEAMS_NEW = 24
if "--new" in sys.argv:  # --beams: room for this many generated tokens per beam (max_new_tokens); above 24 the steps are timed at its end
    _i = sys.argv.index("--new")
    BEAMS_NEW = int(sys.argv[_i + 1])
    del sys.argv[_i:_i + 2]
B = int(sys.argv[1]) if len(sys.argv) > 1 else 1
S = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
NEW = 160
dev = torch.device("cuda:0")
llama = dict(vocab_size=32000, hidden_size=4096, intermediate_size=11008, num_hidden_layers=32, num_attention_heads=32,
             rms_norm_eps=1e-6, rope_theta=10000.0, max_position_embeddings=8192)
vision = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=336, patch_size=14, layer_norm_eps=1e-5)
model = build_synthetic_model(llama, vision, projector="mlp", conv_stride=1, dtype=torch.bfloat16, device="cuda", seed=0)
g = torch.Generator().manual_seed(0)
ids = torch.randint(3, 32000, (B, S), generator=g).to(dev)


def _replay_ms(graph, n=24, warm=3):
    for _ in range(warm):
        graph.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        graph.replay()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def verify_arm(cache):
    """Plain step vs verify step per weight format, then the multi-query attention launch against T one-query launches.  The plain graph
    advances cache.lens by one per replay and the verify graph leaves it alone: lens is put back before each timing, so every figure is
    taken at `context` keys (+ the 30 replays of a plain timing)."""
    eng = model.engine
    keep = cache.lens.clone()
    for name, kw in (("16-bit", dict()), ("fp8", dict(fp8=True)), ("fp4", dict(fp4=True))):
        g, gtok, _ = eng.capture_decode_graph(cache, **kw)
        t_plain = _replay_ms(g)
        cache.lens.copy_(keep)
        del g
        for T in (2, 4, 8, 16):
            if B * T > 16:
                continue
            gv, vtok, _ = eng.capture_verify_graph(cache, T, **kw)
            t_v = _replay_ms(gv)
            del gv
            print(json.dumps({"verify": name + " weights", "kv": KV, "B": B, "context": S, "T": T, "ms_plain_step": round(t_plain, 3),
                              "ms_verify_step": round(t_v, 3), "break_even_extra_tokens": round(t_v / t_plain - 1, 3)}), flush=True)
    if B == 1:
        T = 8
        q1 = torch.randn(B, 4096, dtype=torch.bfloat16, device=dev)
        qT = torch.randn(B * T, 4096, dtype=torch.bfloat16, device=dev)
        if KV8:
            one = lambda li: _O.attn_decode_kv8(q1, *cache.layer(li), keep, 32, 128)  # noqa: E731
            multi = lambda li: _O.attn_decode_multi_kv8(qT, *cache.layer(li), keep, T, 32, 128)  # noqa: E731
        else:
            one = lambda li: _O.attn_decode(q1, cache.k[li], cache.v[li], keep, 32, 128)  # noqa: E731
            multi = lambda li: _O.attn_decode_multi(qT, cache.k[li], cache.v[li], keep, T, 32, 128)  # noqa: E731
        one(0); multi(0)
        torch.cuda.synchronize()
        g1, gm = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g1):
            for li in range(32):
                for _ in range(T):
                    one(li)
        with torch.cuda.graph(gm):
            for li in range(32):
                multi(li)
        us1, usm = _replay_ms(g1, n=8, warm=2) / 32 * 1e3, _replay_ms(gm, n=8, warm=2) / 32 * 1e3
        print(json.dumps({"attention": "mh_attn_decode_multi" + ("_kv8" if KV8 else ""), "T": T, "keys": int(keep[0]), "us_multi_launch": round(usm, 2),
                          "us_T_single_launches": round(us1, 2), "ratio": round(usm / us1, 3)}), flush=True)


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def beams_arm(cache0, cache_s, nb=5, G=BEAMS_NEW, warm=3, steps=13):
    """Expanded against shared beam steps per weight format (module docstring).  Every step is timed by its own events; medians.
    cache0: the prompt prefilled with G spare rows (what the copying path expands); cache_s: the same prompt prefilled with none (what
    generate(share_prompt_kv=True) shares)."""
    eng = model.engine
    gen = torch.Generator().manual_seed(1)
    idx = [torch.randint(0, nb, (nb,), generator=gen).to(dev) for _ in range(warm + steps)]  # in-group (one prompt), duplicates and drops
    toks = torch.randint(3, 32000, (warm + steps, nb), generator=gen).to(dev)
    P = int(cache0.lens[0])
    gen0 = G - 20 if G > 24 else 0  # generated keys taken as already written
    for name, kw in (("16-bit", dict()), ("fp8", dict(fp8=True)), ("fp4", dict(fp4=True))):
        for shared in (False, True):
            if shared:
                c = eng.share_cache(cache_s, nb, G)
                c.gen.add_(gen0)
                c.apos.add_(gen0)
                reorder = lambda t: c.reorder(idx[t])  # noqa: E731
            else:
                c = eng.expand_cache(cache0, torch.zeros(nb, dtype=torch.int64, device=dev))
                c.lens.add_(gen0)
                reorder = lambda t: eng.reorder_cache(c, idx[t], P + gen0 + t)  # noqa: E731
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(warm + steps)]
            for t in range(warm + steps):
                ev[t][0].record()
                reorder(t)
                ev[t][1].record()
                eng.decode_step(toks[t], c, **kw)
                ev[t][2].record()
            torch.cuda.synchronize()
            ms_r = _median([e[0].elapsed_time(e[1]) for e in ev[warm:]])
            ms_d = _median([e[1].elapsed_time(e[2]) for e in ev[warm:]])
            ms = _median([e[0].elapsed_time(e[2]) for e in ev[warm:]])
            # one attention launch of this arm, from a graph over the 32 layers' caches
            q = torch.randn(nb, 4096, dtype=torch.bfloat16, device=dev)
            if shared:
                sl = c.gen.clone()
                if KV8:
                    attn = lambda li: _O.attn_decode_beams_kv8(q, *cache_s.layer(li), cache_s.lens, *c.layer(li), c.anc, sl, nb, 32, 128)  # noqa: E731
                else:
                    attn = lambda li: _O.attn_decode_beams(q, *cache_s.layer(li), cache_s.lens, *c.layer(li), c.anc, sl, nb, 32, 128)  # noqa: E731
                resident = c.nbytes
            else:
                ln = c.lens.clone()
                if KV8:
                    attn = lambda li: _O.attn_decode_kv8(q, *c.layer(li), ln, 32, 128)  # noqa: E731
                else:
                    attn = lambda li: _O.attn_decode(q, c.k[li], c.v[li], ln, 32, 128)  # noqa: E731
                resident = 2 * c.nbytes  # the second buffer set of reorder_cache (k_alt, v_alt and the scales')
            attn(0)
            torch.cuda.synchronize()
            ga = torch.cuda.CUDAGraph()
            with torch.cuda.graph(ga):
                for li in range(32):
                    attn(li)
            us = _replay_ms(ga, n=8, warm=2) / 32 * 1e3
            del ga
            print(json.dumps({"beams": name + " weights", "kv": KV, "num_beams": nb, "context": P, "max_new": G, "share_prompt_kv": shared, "ms_per_beam_step": round(ms, 3),
                              "ms_reorder": round(ms_r, 3), "ms_decode_step": round(ms_d, 3), "us_attention_launch": round(us, 2),
                              "resident_cache_gb": round(resident / 1e9, 3)}), flush=True)
            del c


def _median_ms(fn, warm=2, reps=7):
    out = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record(); torch.cuda.synchronize()
        if i >= warm:
            out.append(a.elapsed_time(b))
    return _median(out)


def extend_arm():
    """Prefill of context + n tokens against extend of n tokens on a context-token cache, and the attention launch alone (module docstring)."""
    eng = model.engine
    P = S
    span = synth._image_span(576, 32000)
    if B != 1 or P < 1 + len(span):
        raise SystemExit("--extend takes B = 1 and a context that holds BOS and one image span (579 tokens)")
    img = torch.randn(1, 3, 336, 336, generator=g).to(dev)
    for n in EXTEND_NS or ((32, 64, 512) if P == 613 else (64,)):
        row = [1] + span + torch.randint(3, 32000, (P + n - 1 - len(span),), generator=g).tolist()
        ids_t = torch.tensor([row]).to(dev)
        ms_prefill = _median_ms(lambda: eng.prefill(ids_t, None, [img], 8, kv_fp8=KV8))
        pre = eng.new_cache(1, P + n + 8, fp8=KV8)
        ms_prefill_into = _median_ms(lambda: eng.prefill(ids_t, None, [img], 8, kv_fp8=KV8, cache=pre))
        del pre
        _, cache = eng.prefill(ids_t[:, :P], None, [img], n + 8, kv_fp8=KV8)

        def run_extend():
            cache.truncate(P)
            eng.extend(cache, ids_t[:, P:], None, pos=P)

        ms_extend = _median_ms(run_extend)
        q = torch.randn(n, 4096, dtype=torch.bfloat16, device=dev)
        lens1 = torch.full((1,), P + 1, dtype=torch.int32, device=dev)
        if KV8:
            attn = lambda li: _O.attn_extend_kv8(q, *cache.layer(li), lens1, n, 32, 128)  # noqa: E731
        else:
            attn = lambda li: _O.attn_extend(q, cache.k[li], cache.v[li], lens1, n, 32, 128)  # noqa: E731
        attn(0)
        torch.cuda.synchronize()
        ga = torch.cuda.CUDAGraph()
        with torch.cuda.graph(ga):
            for li in range(32):
                attn(li)
        us = _replay_ms(ga, n=8, warm=2) / 32 * 1e3
        del ga, cache
        print(json.dumps({"extend": "16-bit weights", "kv": KV, "context": P, "n": n, "ms_prefill_context_plus_n": round(ms_prefill, 3),
                          "ms_prefill_into_existing_cache": round(ms_prefill_into, 3), "ms_extend_n": round(ms_extend, 3),
                          "prefill_over_extend": round(ms_prefill / ms_extend, 2), "us_attn_extend_launch": round(us, 2)}), flush=True)


def score_arm(warm=1, reps=5):
    """model.score against C extends on a session and against C full forwards (module docstring)."""
    from merlin_amd import _lib as L

    eng = model.engine
    P, V, d = S, model.config.vocab_size, 4096
    span = synth._image_span(576, 32000)
    if B != 1 or P < 1 + len(span):
        raise SystemExit("--score takes B = 1 and a context that holds BOS and one image span (579 tokens)")
    img = torch.randn(1, 3, 336, 336, generator=g).to(dev)
    ids_t = torch.tensor([[1] + span + torch.randint(3, 32000, (P - 1 - len(span),), generator=g).tolist()]).to(dev)
    for C_, n in SCORE_CN:
        conts = [torch.randint(3, 31000, (n,), generator=g).tolist() for _ in range(C_)]
        R = C_ * (n - 1)
        cand_t = [torch.tensor([c], device=dev) for c in conts]
        full_t = [torch.cat([ids_t, c], dim=1) for c in cand_t]
        s1 = model.new_session(capacity=P + R + 8, fp8_kv=KV8)
        s2 = model.new_session(capacity=P + n + 8, fp8_kv=KV8)
        stand_in = torch.randn(max(n - 2, 1), d, dtype=torch.bfloat16, device=dev)

        def arm_ii():
            logits, cache = s2._prefill(ids_t, [img], n)
            first = _O.log_softmax_rows(logits, V)
            got = []
            for c in cand_t:  # the targets are gathered on the device; one read-back at the end, like score()
                got.append(first[0, c[0, :1]])
                if n > 1:
                    cache.truncate(P)
                    got.append(_O.log_softmax_rows(eng.extend(cache, c[:, :-1], None, pos=P), V)[0, c[0, -1:]])
                    if n > 2:
                        x = stand_in[:n - 2]
                        head = _O.gemv(x, eng._lm_head_w(), out_f32=True, n=V) if n - 2 <= 16 else _O.gemm_nt(x, eng._lm_head_w(), out_f32=True)
                        got.append(_O.log_softmax_rows(head, V).gather(1, c[0, 1:-1, None])[:, 0])
            cache.truncate(P)
            return torch.cat(got).cpu()

        def arm_ii_full():
            s2.reset()
            return arm_ii()

        def arm_iii():
            for c, f in zip(conts, full_t):
                lg = model(input_ids=f, images=[img]).logits[0, P - 1:-1, :V].float()
                torch.log_softmax(lg, -1).gather(1, torch.tensor(c, device=dev)[:, None]).sum().item()

        arms = {"i_score": lambda: model.score(ids_t, conts, images=[img], fp8_kv=KV8),
                "i_score_prompt_held": lambda: model.score(ids_t, conts, images=[img], fp8_kv=KV8, session=s1),
                "ii_extends": arm_ii_full, "ii_extends_prompt_held": arm_ii, "iii_forwards": arm_iii}
        names = list(arms)
        ms = {k: [] for k in names}
        for t in range(warm + reps):
            for k in names[t % len(names):] + names[:t % len(names)]:  # the arms alternate, and so does which one goes first
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                arms[k]()
                b.record(); torch.cuda.synchronize()
                if t >= warm:
                    ms[k].append(a.elapsed_time(b))
        spread = {k: (min(v), max(v)) for k, v in ms.items()}
        ms = {k: _median(v) for k, v in ms.items()}
        # attention launches per layer, at the library boundary
        seen, real = [], L.call

        def recording(name, *args):
            seen.append(name)
            return real(name, *args)

        L.call = recording
        try:
            arms["i_score_prompt_held"]()
            n_i = sum(x.startswith("mh_attn_extend_branches") for x in seen) / 32
            del seen[:]
            arm_ii()
            n_ii = sum(x.startswith("mh_attn_extend") for x in seen) / 32 - 1  # (without the one-token extend of the held prompt's last position)
        finally:
            L.call = real
        out = {"score": "16-bit weights", "kv": KV, "context": P, "C": C_, "n": n, "rows": R}
        out.update({"ms_" + k: round(v, 3) for k, v in ms.items()})
        out.update({"min_max_" + k: [round(v, 2) for v in spread[k]] for k in ("i_score", "ii_extends")})
        out.update(ratio_i_over_ii=round(ms["i_score"] / ms["ii_extends"], 3), ratio_i_over_iii=round(ms["i_score"] / ms["iii_forwards"], 3),
                   ratio_prompt_held_i_over_ii=round(ms["i_score_prompt_held"] / ms["ii_extends_prompt_held"], 3),
                   attn_launches_per_layer_i=n_i, attn_launches_per_layer_ii=n_ii)
        if R:  # one packed launch against the C launches it replaces
            cache = s1.cache
            q = torch.randn(R, d, dtype=torch.bfloat16, device=dev)
            seg = torch.arange(C_, dtype=torch.int32, device=dev).repeat_interleave(n - 1) * (n - 1)
            lens1 = torch.full((1,), P + 1, dtype=torch.int32, device=dev)
            if KV8:
                packed = lambda li: _O.attn_extend_branches_kv8(q, *cache.layer(li), seg, P, 32, 128)  # noqa: E731
                single = lambda li: _O.attn_extend_kv8(q[:n - 1], *cache.layer(li), lens1, n - 1, 32, 128)  # noqa: E731
            else:
                packed = lambda li: _O.attn_extend_branches(q, cache.k[li], cache.v[li], seg, P, 32, 128)  # noqa: E731
                single = lambda li: _O.attn_extend(q[:n - 1], cache.k[li], cache.v[li], lens1, n - 1, 32, 128)  # noqa: E731
            packed(0); single(0)
            torch.cuda.synchronize()
            gp, gs = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(gp):
                for li in range(32):
                    packed(li)
            with torch.cuda.graph(gs):
                for li in range(32):
                    for _ in range(C_):
                        single(li)
            out.update(us_attn_extend_branches_launch=round(_replay_ms(gp, n=8, warm=2) / 32 * 1e3, 2),
                       us_C_attn_extend_launches=round(_replay_ms(gs, n=8, warm=2) / 32 * 1e3, 2))
            del gp, gs
        print(json.dumps(out), flush=True)
        del s1, s2


def bans_arm(logits, cache, warm=6, steps=40):
    """Decode step + selection without and with mh_ban_tokens, alternating (module docstring)."""
    from merlin_amd import generation as G

    eng = model.engine
    V, P = 32000, S
    rng = torch.Generator().manual_seed(2)
    words = [torch.randint(3, V, (int(k),), generator=rng).tolist() for k in torch.randint(1, 5, (64,), generator=rng)]
    opt = G._resolve_options(None, dict(no_repeat_ngram_size=3, bad_words_ids=words, min_new_tokens=P + 64))
    plan = G._ban_plan(opt, [2])
    tables = G._ban_tables(plan, [2], P, dev)
    hist = torch.zeros(1, P + NEW + 8, dtype=torch.int64, device=dev)
    hist[:, :P] = ids
    graph, g_tok, g_logits = eng.capture_decode_graph(cache)
    keep = cache.lens.clone()
    g_tok.copy_(logits.argmax(-1))

    def step(ban):
        graph.replay()
        if ban:
            _O.ban_tokens(g_logits, V, hist, len0=P, **tables)
        g_tok.copy_(_O.select_tokens(g_logits, V))

    ev = {ban: [] for ban in (False, True)}
    for t in range(warm + steps):
        for ban in ((False, True) if t % 2 == 0 else (True, False)):  # the arms alternate, and so does which one goes first
            cache.lens.copy_(keep)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(ban)
            b.record()
            if t >= warm:
                ev[ban].append((a, b))
    torch.cuda.synchronize()
    ms = {ban: _median([a.elapsed_time(b) for a, b in ev[ban]]) for ban in ev}
    cache.lens.copy_(keep)
    x = torch.randn(1, g_logits.shape[1], device=dev)
    out = {}
    for name, fn in (("mh_ban_tokens", lambda: _O.ban_tokens(x, V, hist, len0=P, **tables)), ("mh_select_tokens", lambda: _O.select_tokens(x, V))):
        fn()
        torch.cuda.synchronize()
        ga = torch.cuda.CUDAGraph()
        with torch.cuda.graph(ga):
            for _ in range(32):
                fn()
        out[name] = _replay_ms(ga, n=8, warm=2) / 32 * 1e3
        del ga
    print(json.dumps({"bans": "no_repeat_ngram_size=3 + 64 bad words + min_new_tokens", "kv": KV, "context": P, "ms_step_plus_select": round(ms[False], 4),
                      "ms_step_plus_ban_plus_select": round(ms[True], 4), "added_us_per_step": round((ms[True] - ms[False]) * 1e3, 2),
                      "us_mh_ban_tokens_launch": round(out["mh_ban_tokens"], 2), "us_mh_select_tokens_launch": round(out["mh_select_tokens"], 2)}), flush=True)


def guidance_arm(logits, cache, warm=6, steps=40):
    """Plain B = 1 step against the guided step (B = 2 step on the paired cache + mh_guidance_mix), alternating (module docstring)."""
    eng = model.engine
    V, scale = 32000, 1.5
    neg = ids[:, min(576, S - 1):]
    _, cu = eng.prefill(neg, None, None, 0, kv_fp8=KV8)
    pair = eng.pair_cache(cache, cu, NEW + 8)
    del cu
    g1, tok1, log1 = eng.capture_decode_graph(cache)
    g2, tok2, log2 = eng.capture_decode_graph(pair)
    keep1, keep2 = cache.lens.clone(), pair.lens.clone()
    tok1.copy_(logits.argmax(-1))
    tok2.copy_(tok1)  # (broadcast: the one token goes to both rows)

    def step(graph, guided):
        if guided:
            lg = (g2.replay() or log2) if graph else eng.decode_step(tok2, pair)
            _O.guidance_mix(lg[:1], lg[1:], scale, V, out=lg[:1])
        elif graph:
            g1.replay()
        else:
            eng.decode_step(tok1, cache)

    arms = [(True, False), (True, True), (False, False), (False, True)]
    ev = {arm: [] for arm in arms}
    for t in range(warm + steps):
        for arm in (arms if t % 2 == 0 else arms[::-1]):  # the arms alternate, and so does their order
            cache.lens.copy_(keep1)
            pair.lens.copy_(keep2)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(*arm)
            b.record()
            if t >= warm:
                ev[arm].append((a, b))
    torch.cuda.synchronize()
    ms = {arm: _median([a.elapsed_time(b) for a, b in ev[arm]]) for arm in arms}
    cache.lens.copy_(keep1)
    pair.lens.copy_(keep2)
    x = torch.randn(2, log2.shape[1], device=dev)
    _O.guidance_mix(x[:1], x[1:], scale, V, out=x[:1])
    torch.cuda.synchronize()
    ga = torch.cuda.CUDAGraph()
    with torch.cuda.graph(ga):
        for _ in range(32):
            _O.guidance_mix(x[:1], x[1:], scale, V, out=x[:1])
    us_mix = _replay_ms(ga, n=8, warm=2) / 32 * 1e3
    del ga
    print(json.dumps({"guidance": "B = 2 step on the paired cache + mh_guidance_mix vs the plain B = 1 step", "kv": KV, "context": S, "negative_context": int(neg.shape[1]),
                      "ms_plain_step_graph": round(ms[(True, False)], 4), "ms_guided_step_graph": round(ms[(True, True)], 4),
                      "guided_over_plain_graph": round(ms[(True, True)] / ms[(True, False)], 3),
                      "ms_plain_step_eager": round(ms[(False, False)], 4), "ms_guided_step_eager": round(ms[(False, True)], 4),
                      "guided_over_plain_eager": round(ms[(False, True)] / ms[(False, False)], 3), "us_mh_guidance_mix_launch": round(us_mix, 2)}), flush=True)


with torch.no_grad():
    if EXTEND:
        extend_arm()
        sys.exit(0)
    if SCORE:
        score_arm()
        sys.exit(0)
    t0 = time.time()
    logits, cache = model.engine.prefill(ids, None, None, BEAMS_NEW if BEAMS else NEW + 8, kv_fp8=KV8)
    torch.cuda.synchronize()
    print(f"prefill B={B} S={S}: {(time.time()-t0)*1e3:.1f} ms (first call, incl. arena setup)", flush=True)
    if VERIFY:
        verify_arm(cache)
        sys.exit(0)
    if BEAMS:
        beams_arm(cache, model.engine.prefill(ids, None, None, 0, kv_fp8=KV8)[1])
        sys.exit(0)
    if BANS:
        if B != 1:
            raise SystemExit("--bans takes B = 1")
        bans_arm(logits, cache)
        sys.exit(0)
    if GUIDANCE:
        if B != 1:
            raise SystemExit("--guidance takes B = 1")
        guidance_arm(logits, cache)
        sys.exit(0)
    tok = logits.argmax(-1)
    for _ in range(3):
        logits = model.engine.decode_step(tok, cache); tok = logits.argmax(-1)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    n = 32
    for _ in range(n):
        logits = model.engine.decode_step(tok, cache); tok = logits.argmax(-1)
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    wbytes = sum(p.numel() for n_, p in model.named_parameters() if n_.startswith("model.layers") or n_.startswith("lm_head") or n_ == "model.norm.weight") * 2
    cbytes = 2 * 32 * B * (S + 20) * ((4096 + 32 * 4) if KV8 else 4096 * 2)  # fp8: one byte per value + one fp32 scale per head
    print(json.dumps({"decode": "eager", "kv": KV, "B": B, "context": S, "ms_per_step": round(ms, 3), "tokens_per_s": round(B * 1e3 / ms, 1),
                      "hbm_gb_per_step": round((wbytes + cbytes) / 1e9, 2), "hbm_tb_s": round((wbytes + cbytes) / ms / 1e9, 2)}), flush=True)
    # one decode-attention launch, from a graph of 32 (one per layer's cache: 2+ GB between two visits of the same keys)
    qa = torch.randn(B, 4096, dtype=torch.bfloat16, device=dev)
    lens_a = cache.lens.clone()
    if KV8:
        attn = lambda li: _O.attn_decode_kv8(qa, *cache.layer(li), lens_a, 32, 128)  # noqa: E731
    else:
        attn = lambda li: _O.attn_decode(qa, cache.k[li], cache.v[li], lens_a, 32, 128)  # noqa: E731
    attn(0)
    torch.cuda.synchronize()
    ga = torch.cuda.CUDAGraph()
    with torch.cuda.graph(ga):
        for li in range(32):
            attn(li)
    for _ in range(2):
        ga.replay()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(8):
        ga.replay()
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / (8 * 32) * 1e3
    abytes = 2 * B * int(lens_a[0]) * ((4096 + 32 * 4) if KV8 else 4096 * 2)
    print(json.dumps({"attention_launch": "mh_attn_decode_kv8" if KV8 else "mh_attn_decode", "B": B, "keys": int(lens_a[0]), "us_per_launch": round(us, 2),
                      "cache_mb_per_launch": round(abytes / 1e6, 1), "hbm_tb_s": round(abytes / us / 1e6, 2)}), flush=True)
    del ga
    # the same step as one replayed HIP graph
    g, gtok, glog = model.engine.capture_decode_graph(cache)
    gtok.copy_(tok)
    for _ in range(3):
        g.replay(); gtok.copy_(glog.argmax(-1))
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        g.replay(); gtok.copy_(glog.argmax(-1))
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    print(json.dumps({"decode": "hip-graph", "kv": KV, "B": B, "context": S, "ms_per_step": round(ms, 3), "tokens_per_s": round(B * 1e3 / ms, 1),
                      "hbm_gb_per_step": round((wbytes + cbytes) / 1e9, 2), "hbm_tb_s": round((wbytes + cbytes) / ms / 1e9, 2),
                      "weights_tb_s": round(wbytes / ms / 1e9, 2)}), flush=True)
    # fp8 weights (e4m3, per-128-block scales), graph replay
    model.engine.quantize_decode_weights()
    g8, gtok8, glog8 = model.engine.capture_decode_graph(cache, fp8=True)
    gtok8.copy_(tok)
    for _ in range(3):
        g8.replay(); gtok8.copy_(glog8.argmax(-1))
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        g8.replay(); gtok8.copy_(glog8.argmax(-1))
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    w8 = wbytes // 2 + wbytes // 2 // 64  # fp8 bytes + fp32 scales (1 per 128)
    print(json.dumps({"decode": "hip-graph fp8 weights", "kv": KV, "B": B, "context": S, "ms_per_step": round(ms, 3), "tokens_per_s": round(B * 1e3 / ms, 1),
                      "hbm_gb_per_step": round((w8 + cbytes) / 1e9, 2), "hbm_tb_s": round((w8 + cbytes) / ms / 1e9, 2),
                      "weights_tb_s": round(w8 / ms / 1e9, 2)}), flush=True)
    del g8
    # MXFP4 weights (e2m1 values, one power-of-two scale byte per 32 k), graph replay
    model.engine.quantize_decode_weights_fp4()
    g4, gtok4, glog4 = model.engine.capture_decode_graph(cache, fp4=True)
    gtok4.copy_(tok)
    for _ in range(3):
        g4.replay(); gtok4.copy_(glog4.argmax(-1))
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        g4.replay(); gtok4.copy_(glog4.argmax(-1))
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    w4 = wbytes // 4 + wbytes // 2 // 32  # half a byte per weight + one scale byte per 32
    print(json.dumps({"decode": "hip-graph fp4 weights", "kv": KV, "B": B, "context": S, "ms_per_step": round(ms, 3), "tokens_per_s": round(B * 1e3 / ms, 1),
                      "hbm_gb_per_step": round((w4 + cbytes) / 1e9, 2), "hbm_tb_s": round((w4 + cbytes) / ms / 1e9, 2),
                      "weights_tb_s": round(w4 / ms / 1e9, 2)}), flush=True)
