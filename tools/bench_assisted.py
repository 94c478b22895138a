"""Cost of assisted decoding (generate(assistant_model=draft, num_assistant_tokens=k)) at Llama-7B size, B = 1 (run on the GPU box).

    python tools/bench_assisted.py [--contexts 613,4096] [--ks 3,5,7] [--skip-generate]

Random weights accept almost nothing, so this reports what a round COSTS and the yield at which it pays, not a speed-up.  The target is the
synthetic 7B model (V = 32003) with 16-bit, fp8 and MXFP4 decode weights; the drafts are two synthetic text-only decoders at the same
vocabulary, "70M" (hidden 512, 10 layers, 8 heads, MLP 1536: 67 M parameters) and "300M" (hidden 1024, 18 layers, 16 heads, MLP 2816:
297 M).  One process, every figure a median of per-iteration device-event timings after warm-up; arms that are compared alternate.

Per context:
  target lines   the plain decode step and the verify step of k + 1 rows, each replayed from its HIP graph, per weight format.
  draft lines    one round's k draft steps exactly as generate() runs them (generation._ModelDrafter.propose: the token copy, the
                 counters, the replays, the launches) in its two arms - "chain": ONE replay of engine.capture_draft_graph's graph;
                 "steps": per step a token copy, a replay of the single-step graph and the eager scalar selection (with bans: the eager
                 ban launch and the store into the ids buffer as well) - without bans and with no_repeat_ngram_size = 3.  ms per round
                 and per draft step, and chain / steps.
  break-even     (k * t_draft + t_verify) / t_plain - 1: the drafted tokens a round must have accepted on average before it is cheaper
                 than plain steps, for both arms and every weight format.
Then, unless --skip-generate, whole generate() calls at the first context, k = 5, 64 new tokens, greedy: the plain path, both arms with each
draft (ms per round beside the sum the lines above predict: what the host loop adds), and draft = the target itself (its own weights:
every draft accepted) as the full-acceptance bound of the bookkeeping - ms per token against the plain path's, and the stats.  Where an
assisted output leaves the plain path's (random 7B weights give nearly flat logits, and the verify step's many-row kernels round unlike the
one-row step), the line carries the first difference and the gap of the other token below the maximum of the plain path's own logits.
"chain" is generate(assistant_chain_graph=True), "steps" the default."""
import argparse
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from merlin_amd import generation as G  # noqa: E402
from merlin_amd.model.llama_mmgpt import build_synthetic_model  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--contexts", default="613,4096")
ap.add_argument("--ks", default="3,5,7")
ap.add_argument("--skip-generate", action="store_true")
ap.add_argument("--tiny", action="store_true", help="toy geometries: a rehearsal of the script, not a measurement")
args = ap.parse_args()
CONTEXTS = [int(a) for a in args.contexts.split(",")]
KS = [int(a) for a in args.ks.split(",")]
dev = torch.device("cuda:0")
VISION = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, image_size=56, patch_size=14, layer_norm_eps=1e-5)  # (dropped again: text-only)
V0 = 32000


def _decoder(hidden, layers, heads, mlp, seed, vocab=V0):
    llama = dict(vocab_size=vocab, hidden_size=hidden, intermediate_size=mlp, num_hidden_layers=layers, num_attention_heads=heads, rms_norm_eps=1e-6,
                 rope_theta=10000.0, max_position_embeddings=8192)
    m = build_synthetic_model(llama, VISION, projector="mlp", conv_stride=1, dtype=torch.bfloat16, device="cuda", seed=seed)
    m.get_model().vision_tower = None  # text-only
    return m


if args.tiny:
    V0 = 100
    target = _decoder(256, 2, 2, 512, 0, V0)
    DRAFTS = [("70M", _decoder(128, 1, 2, 256, 1, V0)), ("300M", _decoder(256, 1, 2, 512, 2, V0))]
else:
    target = _decoder(4096, 32, 32, 11008, 0)
    DRAFTS = [("70M", _decoder(512, 10, 8, 1536, 1)), ("300M", _decoder(1024, 18, 16, 2816, 2))]
V = target.config.vocab_size
FORMATS = (("16-bit", dict()), ("fp8", dict(fp8=True)), ("fp4", dict(fp4=True)))
SEL = dict(do_sample=False, temperature=1.0, top_k=50, top_p=1.0, seed=0)


def _params(m):
    return sum(p.numel() for n, p in m.named_parameters() if n.startswith(("model.layers", "model.norm", "model.embed_tokens", "lm_head")))


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _alternate(arms, warm=3, reps=15):
    """arms: {name: (reset, run)} -> {name: median ms of run()}, every run between its own events, the arms taking turns."""
    out = {k: [] for k in arms}
    for it in range(warm + reps):
        for name, (reset, run) in arms.items():
            reset()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            torch.cuda.synchronize()
            if it >= warm:
                out[name].append(a.elapsed_time(b))
    return {k: _median(v) for k, v in out.items()}


def target_lines(ids, ctx):
    """-> {(format, k): (ms plain, ms verify)}"""
    eng = target.engine
    _, cache = eng.prefill(ids, None, None, 64)
    keep = cache.lens.clone()
    res = {}
    for name, kw in FORMATS:
        g, _, _ = eng.capture_decode_graph(cache, **kw)
        t_plain = _alternate({"plain": (lambda: cache.lens.copy_(keep), g.replay)})["plain"]
        del g
        for k in KS:
            gv, _, _ = eng.capture_verify_graph(cache, k + 1, **kw)
            t_v = _alternate({"verify": (lambda: None, gv.replay)})["verify"]
            del gv
            res[name, k] = (t_plain, t_v)
            print(json.dumps({"target": name + " weights", "context": ctx, "k": k, "ms_plain_step": round(t_plain, 3), "ms_verify_step_k+1_rows": round(t_v, 3),
                              "break_even_without_draft_cost": round(t_v / t_plain - 1, 3)}), flush=True)
    cache.lens.copy_(keep)
    return res


def draft_lines(name, draft, ids, ctx, tgt):
    """One round's k draft steps through generation._ModelDrafter in both arms, alternating."""
    res = {}
    n = ctx + 1  # the prompt and the prefill's token
    for bans in (False, True):
        for k in KS:
            max_len = ctx + 64
            tables = G._ban_tables(dict(ngram=3, words=[], always=[], begin=[], min_new=0), [], ctx, dev) if bans else None
            arms, drafters = {}, {}
            for arm in ("chain", "steps"):
                seq = torch.zeros(1, max_len + k, dtype=torch.int64, device=dev)
                seq[0, :ctx] = ids[0]
                seq[0, ctx] = 7
                call = types.SimpleNamespace(assistant=draft, model=target, images=None, max_len=max_len, sel=SEL)
                d = G._ModelDrafter(call, seq, k, chain=arm == "chain", graph=True)
                d.prefill(ids, tables)
                drafters[arm] = d

                def reset(d=d):
                    d.cache.truncate(n - 1)
                    d.fed = n - 1

                arms[arm] = (reset, lambda d=d: d.propose(n))
            t = _alternate(arms)
            assert torch.equal(drafters["chain"].tok, drafters["steps"].tok), "the two arms drafted different tokens"
            res[bans, k] = t
            line = {"draft": name, "params_M": round(_params(draft) / 1e6, 1), "context": ctx, "k": k, "bans": "no_repeat_ngram_size=3" if bans else "none",
                    "ms_round_chain": round(t["chain"], 3), "ms_round_steps": round(t["steps"], 3), "ms_draft_step_chain": round(t["chain"] / k, 4),
                    "ms_draft_step_steps": round(t["steps"] / k, 4), "chain_over_steps": round(t["chain"] / t["steps"], 3)}
            if not bans:
                for fmt, _ in FORMATS:
                    t_plain, t_v = tgt[fmt, k]
                    line["break_even_chain_" + fmt] = round((t["chain"] + t_v) / t_plain - 1, 3)
                    line["break_even_steps_" + fmt] = round((t["steps"] + t_v) / t_plain - 1, 3)
            print(json.dumps(line), flush=True)
    return res


def generate_lines(ids, ctx, tgt, drafts):
    """Whole calls: what the host loop adds to a round, and the full-acceptance bound with the target as its own draft."""
    import time

    k, new = 5, 64
    kw = dict(max_new_tokens=new, eos_token_id=-1, pad_token_id=0)

    def run(**extra):
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = target.generate(ids, **kw, **extra)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return _median(ts), dict(target.engine.last_generate_stats), out

    # (the prefill and the captures are in every call: subtract a call of 3 tokens, which has them too, to leave the steps)
    def steps_ms(**extra):
        long, st, out = run(**extra)
        short = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            target.generate(ids, **dict(kw, max_new_tokens=2 + k), **extra)
            torch.cuda.synchronize()
            short.append((time.perf_counter() - t0) * 1e3)
        st_short = dict(target.engine.last_generate_stats)
        return long - _median(short), st, st_short, out

    def tie(out):
        """Equal to the plain output, or: (position of the first difference, the gap between the maximum and the other path's token in
        the plain path's own logits there, as a share of the largest logit magnitude) - the tie rule of the tests is 2e-3."""
        if torch.equal(out, plain):
            return True
        n = min(out.shape[1], plain.shape[1])
        t = int((out[0, :n] != plain[0, :n]).nonzero()[0])
        eng = target.engine
        lg, cache = eng.prefill(ids, None, None, new + 2)
        for tok in plain[0, ctx:t].tolist():
            lg = eng.decode_step(torch.tensor([tok], device=dev), cache)
        lg = lg[0, :V].float()
        return {"first_difference_at_new_token": t - ctx, "gap_over_max_logit": float((lg.max() - lg[int(out[0, t])]) / lg.abs().max())}

    ms, st, st_s, plain = steps_ms()
    per_tok = ms / (new - 2 - k)
    print(json.dumps({"generate": "plain", "context": ctx, "new_tokens": new, "ms_per_token": round(per_tok, 3), "stats": st}), flush=True)
    for name, draft, res in drafts:
        for arm in ("chain", "steps"):
            ms, st, st_s, out = steps_ms(assistant_model=draft, num_assistant_tokens=k, assistant_chain_graph=arm == "chain")
            rounds = st["verify_steps"] - st_s["verify_steps"]
            t_plain, t_v = tgt["16-bit", k]
            print(json.dumps({"generate": f"draft {name}, {arm}", "context": ctx, "k": k, "new_tokens": new, "ms_per_round": round(ms / max(rounds, 1), 3),
                              "ms_round_predicted_draft+verify": round(res[False, k][arm] + t_v, 3), "same_tokens_as_plain": tie(out), "stats": st}), flush=True)
    for arm in ("chain", "steps"):
        ms, st, st_s, out = steps_ms(assistant_model=target, num_assistant_tokens=k, assistant_chain_graph=arm == "chain")
        print(json.dumps({"generate": f"draft = the target itself (full acceptance), {arm}", "context": ctx, "k": k, "new_tokens": new,
                          "ms_per_token": round(ms / (new - 2 - k), 3), "ms_per_token_plain": round(per_tok, 3), "accepted_of_drafted": f"{st['accepted']}/{st['drafted']}",
                          "same_tokens_as_plain": tie(out), "stats": st}), flush=True)


def main():
    g = torch.Generator().manual_seed(0)
    first = None
    for ctx in CONTEXTS:
        ids = torch.randint(3, V0, (1, ctx), generator=g).to(dev)
        tgt = target_lines(ids, ctx)
        drafts = [(name, d, draft_lines(name, d, ids, ctx, tgt)) for name, d in DRAFTS]
        if first is None:
            first = (ids, ctx, tgt, drafts)
    if not args.skip_generate:
        generate_lines(*first)


if __name__ == "__main__":
    with torch.no_grad():
        main()
