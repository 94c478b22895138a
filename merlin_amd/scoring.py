"""score() for MMGPTLlamaForCausalLM on the HIP engine: the log-likelihoods of C candidate continuations of ONE prompt.

Likelihood ranking is the second way such a model is evaluated besides decoding: multiple-choice benchmarks (the `loglikelihood` request
of evaluation harnesses: log p(continuation | context) and "is the continuation the greedy one"), caption / answer re-ranking, grounding
box candidates, reward and filter scores.  One image + question prompt of P tokens, C short text continuations.

The prompt runs once (engine.prefill, or the tail a Session does not hold yet) and its last-position logits score the FIRST token of every
candidate.  Token j >= 1 of a candidate is scored from the row that was fed token j - 1, and the last token is never fed, so the
candidates contribute R = sum(n_c - 1) rows.  They run through the decoder in ONE packed pass over the 16-bit weights
(engine.extend_branches): every row sees the prompt's keys and the earlier rows of its own candidate only (mh_attn_extend_branches).
lm_head and the log-probabilities run in chunks of engine.HEAD_CHUNK rows, and mh_token_logprobs reduces a chunk's fp32 logits to one
log-probability and one greedy flag per row - no [rows, V] log-softmax is written.  _branch_plan is the host part: a pure function.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import ops as O


@dataclass
class BranchPlan:
    """The packed rows of C continuations (see _branch_plan)."""
    fed: list                    # [R] token ids fed to the decoder: every token of a continuation but its last, in packed order
    seg_start: torch.Tensor      # int32 [R]: packed index of the first row of the row's own continuation (non-decreasing, <= r)
    rel_pos: torch.Tensor        # int32 [R]: the row's offset inside its continuation; its rotary position is P + rel_pos
    targets: torch.Tensor        # int64 [R]: the token the row's logits score (the continuation's next token)
    first_targets: torch.Tensor  # int64 [C]: the first token of every continuation, scored by the prompt's last-position logits
    offsets: list                # [C + 1]: continuation c owns the packed rows offsets[c] : offsets[c + 1] (n_c - 1 of them)


@dataclass
class ScoreOutput:
    """token_logprobs: C fp32 tensors [n_c], entry j = log p(c_j | prompt, c_0 .. c_{j-1}) under the softmax over the V valid logits;
    logprobs fp32 [C]: their sums; is_greedy bool [C]: every token of the candidate is the lowest-index argmax of its row; stats:
    prompt_tokens_run, prompt_tokens_reused, rows (= sum(n_c - 1)), images_encoded.  The tensors are on the host."""
    token_logprobs: list
    logprobs: torch.Tensor
    is_greedy: torch.Tensor
    stats: dict


def _token_lists(continuations):
    """continuations (lists, tuples or 1-D tensors of token ids) -> list of lists of ints; refuses what is not a non-empty list of
    non-empty sequences."""
    if isinstance(continuations, torch.Tensor) or not isinstance(continuations, (list, tuple)) or len(continuations) == 0:
        raise ValueError("score: `continuations` has to be a non-empty list of token-id sequences")
    out = []
    for i, c in enumerate(continuations):
        if isinstance(c, torch.Tensor):
            if c.dim() != 1:
                raise ValueError(f"score: continuation {i} has to be a 1-D sequence of token ids, got shape {tuple(c.shape)}")
            c = c.tolist()
        if not isinstance(c, (list, tuple)) or any(isinstance(t, bool) or not isinstance(t, int) for t in c):
            raise ValueError(f"score: continuation {i} has to be a list or a 1-D tensor of integer token ids")
        if len(c) == 0:
            raise ValueError(f"score: continuation {i} is empty (every candidate needs at least one token)")
        out.append([int(t) for t in c])
    return out


def _branch_plan(continuations):
    """The packed pass over C continuations (lists of ints, each non-empty), on the host: continuation c feeds its tokens 0 .. n_c - 2 in
    rows offsets[c] .. offsets[c + 1] - 1; the row fed token j scores token j + 1 and sits at rotary position P + j.  A one-token
    continuation contributes no row; R = 0 is a valid plan (only the prompt's logits are needed).  A pure function."""
    fed, seg, rel, tgt, first, off = [], [], [], [], [], [0]
    for c in continuations:
        if len(c) == 0:
            raise ValueError("_branch_plan: an empty continuation")
        first.append(int(c[0]))
        start = len(fed)
        for j in range(len(c) - 1):
            fed.append(int(c[j]))
            seg.append(start)
            rel.append(j)
            tgt.append(int(c[j + 1]))
        off.append(len(fed))
    return BranchPlan(fed=fed, seg_start=torch.tensor(seg, dtype=torch.int32), rel_pos=torch.tensor(rel, dtype=torch.int32),
                      targets=torch.tensor(tgt, dtype=torch.int64), first_targets=torch.tensor(first, dtype=torch.int64), offsets=off)


@torch.no_grad()
def score(model, input_ids, continuations, images=None, fp8_kv=False, session=None, attention_mask=None):
    """log p(continuation | prompt) for C text continuations of one prompt -> ScoreOutput.
    input_ids [1, P]: one un-padded prompt, image spans as in generate() (`images`).  continuations: a non-empty list of C non-empty
    token-id sequences (lists or 1-D tensors), text only: the image start / end / patch ids are refused.  fp8_kv: the KV cache format
    (the prompt's own attention runs unquantised as in prefill; the candidates' rows read the quantised prompt).  session=s: the longest
    reusable prefix of the prompt comes from the session's cache by generate()'s rules (Session._prefill); afterwards the session holds
    exactly the prompt (cache.lens == P, s.tokens == the prompt; the candidates' rows are stale, as after a rejected draft), so a following
    score() or generate() on the same image and question runs one prompt token.  attention_mask is accepted only without zeros.
    Always the 16-bit weights, like engine.extend.  Refusals are raised before any device work."""
    conts = _token_lists(continuations)
    if input_ids.dim() != 2 or input_ids.shape[1] < 1:
        raise ValueError(f"score: input_ids has to be [1, P >= 1], got {tuple(input_ids.shape)}")
    if input_ids.shape[0] != 1:
        raise ValueError(f"score: the candidates continue one prompt, input_ids has batch_size = {input_ids.shape[0]}")
    if attention_mask is not None and not bool(torch.as_tensor(attention_mask).to(torch.bool).all()):
        raise ValueError("score: takes an un-padded prompt (attention_mask with zeros)")
    if session is not None and bool(fp8_kv) != bool(session.fp8_kv):
        raise ValueError(f"session: fp8_kv={bool(fp8_kv)} but the session's cache was made with fp8_kv={bool(session.fp8_kv)}")
    special = {name: getattr(model, name, None) for name in ("im_start_token", "im_end_token", "im_patch_token")}
    for i, c in enumerate(conts):
        for name, tok in special.items():
            if tok is not None and tok in c:
                raise ValueError(f"score: continuation {i} contains the image token id {tok} ({name}): continuations are text only")
    V = int(model.config.vocab_size)
    for i, c in enumerate(conts):
        if any(not 0 <= t < V for t in c):
            raise ValueError(f"score: continuation {i} has token ids outside [0, {V})")
    plan = _branch_plan(conts)
    R, C, P = len(plan.fed), len(conts), int(input_ids.shape[1])
    eng = model.engine
    if session is not None:
        logits, cache = session._prefill(input_ids, images, R)
        stats = dict(prompt_tokens_run=session.last["run_tokens"], prompt_tokens_reused=session.last["reused_tokens"], rows=R,
                     images_encoded=session.last["images_encoded"])
    else:
        logits, cache = eng.prefill(input_ids, None, images, R, kv_fp8=bool(fp8_kv))
        stats = dict(prompt_tokens_run=P, prompt_tokens_reused=0, rows=R, images_encoded=sum(int(im.shape[0]) for im in (images or [])))
    dev = logits.device
    lp = torch.empty(C + R, dtype=torch.float32, device=dev)
    gr = torch.empty(C + R, dtype=torch.int32, device=dev)
    # the first token of every candidate: C targets on the one row of prompt logits (row stride 0)
    O.token_logprobs(logits[:1].expand(C, -1), plan.first_targets.to(dev), V, logprob=lp[:C], greedy=gr[:C])
    if R:
        hn = eng.extend_branches(cache, plan, pos=P)
        tgt = plan.targets.to(dev)
        for r0 in range(0, R, eng.HEAD_CHUNK):
            r1 = min(R, r0 + eng.HEAD_CHUNK)
            O.token_logprobs(eng.head_logits(hn[r0:r1]), tgt[r0:r1], V, logprob=lp[C + r0:C + r1], greedy=gr[C + r0:C + r1])
    lp, gr = lp.cpu(), gr.cpu()
    off = plan.offsets
    token_logprobs = [torch.cat([lp[c:c + 1], lp[C + off[c]:C + off[c + 1]]]) for c in range(C)]
    greedy = [bool(gr[c]) and bool(gr[C + off[c]:C + off[c + 1]].all()) for c in range(C)]
    return ScoreOutput(token_logprobs=token_logprobs, logprobs=torch.stack([t.sum() for t in token_logprobs]),
                       is_greedy=torch.tensor(greedy, dtype=torch.bool), stats=stats)
