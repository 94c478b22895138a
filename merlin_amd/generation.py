"""generate() for MMGPTLlamaForCausalLM on the HIP engine.

The reference inherits transformers' `GenerationMixin.generate` (LlamaForCausalLM base, llama_mmgpt.py:38) and its eval
scripts drive it as (eval_mmvet.py:101-120, eval_box.py, demo.py, model_worker.py):

    model.generate(input_ids, images=[Tensor[n,3,H,W]], do_sample=True, temperature=0.2, max_new_tokens=1024,
                   stopping_criteria=[KeywordsStoppingCriteria(...)])
    model.generate(input_ids, images=..., num_beams=5, temperature=0.2, max_new_tokens=1024, stopping_criteria=[...])

This module restates the three decoding modes those calls reach - greedy, multinomial sampling with the HF logits warpers
(temperature -> top-k, HF's generation default top_k=50 -> top-p) and beam search (transformers/generation/utils.py `_sample`,
`_beam_search`, the vectorised formulation of the installed transformers) - on top of the engine's prefill + KV-cache decode
step.  Pins (tests/golden/gen_tiny.json, oracle/make_gen_golden.py): greedy = token ids from the REAL reference's generate on
multimodal prompts; beam search = transformers' own generate on a plain LlamaForCausalLM carrying the same decoder weights (the
reference's multimodal beam path needs transformers 4.31's tuple KV cache and cannot run correctly in the build container);
the warper chain = transformers' Temperature/TopK/TopP warpers.  Device work is in kernels (decode step, mh_select_tokens, mh_log_softmax_rows, mh_gather_rows2d);
what stays here is the control flow HF also keeps on the host (beam bookkeeping on [B, 2*num_beams] tensors, the stopping
criteria protocol: user criteria are called with (input_ids, scores) every step exactly like StoppingCriteriaList does).

Token-level constraints (transformers' NoRepeatNGram / NoBadWords / SuppressTokens / SuppressTokensAtBegin / MinNewTokensLength logits
processors: no_repeat_ngram_size, bad_words_ids, suppress_tokens, begin_suppress_tokens, min_new_tokens) all write -inf into chosen logits
given the sequence so far.  They run on the device: the options are resolved once per call into a plan (_ban_plan; its tables are built
once, _ban_tables), the sequence is kept in one preallocated ids buffer, and every step is ONE mh_ban_tokens launch on the step's logits
right before the selection (beam search: on log_probs + running scores before the top-k) - no ids come back to the host.  _banned is the
restatement of the five clauses on a Python list.  Two more warpers, min_p and epsilon_cutoff, are thresholds of the selection kernel
(mh_select_tokens_warp), behind top-p in transformers' order.  A call with none of these options launches what it launched before them.

Classifier-free guidance (transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor, the first processor of its chain: guidance_scale,
negative_prompt_ids, negative_prompt_attention_mask; negative_images is this package's addition for negative prompts with image spans):
a second, unconditional sequence - the negative prompt (default: the prompt's last token) followed by every generated token - is decoded
beside the conditional one, and the step's scores become lu + g (lc - lu) of the two rows' log-softmaxes (mh_guidance_mix) before the bans,
the warpers and the selection.  With a KV cache the two sequences are the two rows of ONE cache (engine.pair_cache), so a step streams the
weights once: a B = 2 decode step (or a [2, T] verify step) plus one mix launch.  _resolve_guidance, _uncond_context and _guided_ref are
the host side as pure functions.

Speculative decoding has ONE loop (_draft_loop: draft, verify in one multi-row step, keep the agreeing prefix plus one) and two drafters:
prompt lookup (_NgramDrafter, prompt_lookup_num_tokens) and a draft model (_ModelDrafter, assistant_model / num_assistant_tokens:
transformers' assisted decoding under this module's contract - the plain path's token stream, not rejection sampling).  The draft model's k
steps with their bans and selections can be one replayable graph (assistant_chain_graph=True: engine.capture_draft_graph on
mh_ban_tokens_dev / mh_select_tokens_dev, whose step number and history length are device counters; the default replays a single-step
graph per draft step - the two measured as a tie).  _resolve_assistant, _assisted_caches and _drafts_that_fit are its host side as pure
functions.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import ops as O

NEG = -1.0e9


def _as_list(x):
    if x is None:
        return []
    if isinstance(x, (list, tuple)):
        return list(x)
    if isinstance(x, torch.Tensor):
        return [int(v) for v in x.reshape(-1).tolist()]
    return [int(x)]


class _Stopper:
    """StoppingCriteriaList semantics: MaxLengthCriteria + EosTokenCriteria + the caller's criteria, OR-ed per sequence.
    User criteria may return a bool (old API, e.g. the reference's KeywordsStoppingCriteria, mm_utils.py:62-85: one verdict
    for the whole batch) or a bool tensor [n]."""

    def __init__(self, max_length, eos_ids, user):
        self.max_length, self.eos_ids, self.user = max_length, eos_ids, list(user or [])

    def __call__(self, ids, scores=None):
        n = ids.shape[0]
        done = torch.full((n,), ids.shape[1] >= self.max_length, dtype=torch.bool, device=ids.device)
        last = ids[:, -1]
        for e in self.eos_ids:
            done = done | (last == e)
        for c in self.user:
            r = c(ids, scores)
            r = torch.as_tensor(r, device=ids.device)
            done = done | (r.to(torch.bool) if r.dim() else r.to(torch.bool).expand(n))
        return done


def _image_spans(ids, im_start, im_end):
    """[(start, end)] of the image spans in a list of token ids: <im_start> at `start`, its <im_end> at `end - 1`; span i is image i of
    the prompt.  An <im_start> without an <im_end> behind it opens no span."""
    spans, open_at = [], None
    if im_start is None or im_end is None:
        return spans
    for i, t in enumerate(ids):
        if t == im_start:
            open_at = i
        elif t == im_end and open_at is not None:
            spans.append((open_at, i + 1))
            open_at = None
    return spans


def _reusable_prefix(cached_ids, cached_spans, cached_images, new_ids, new_spans, new_images):
    """How many leading tokens of the new prompt a session's cache already holds: the longest common token prefix, at most
    len(new_ids) - 1 (one position must run to give the logits that select the first new token), moved back to the start of an image span
    it would cut and to the start of the first image span inside it whose pixels differ (torch.equal on shape and values: equal
    placeholder ids do not mean equal images).  Ids are lists of ints, spans lists of (start, end), images one tensor per span.
    0: nothing to keep, a plain prefill.  A pure function of host data."""
    lim = min(len(cached_ids), len(new_ids) - 1)
    keep = 0
    while keep < lim and int(cached_ids[keep]) == int(new_ids[keep]):
        keep += 1
    for i, (s, e) in enumerate(new_spans):
        if s >= keep:
            break
        if e > keep:  # the prefix ends inside the span
            return s
        same = i < len(cached_spans) and tuple(cached_spans[i]) == (s, e) and i < len(cached_images) and i < len(new_images)
        if same:
            a, b = cached_images[i], new_images[i]
            same = a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.to(b.device), b)
        if not same:
            return s
    return max(keep, 0)


class Session:
    """One sequence's KV cache kept between generate() calls (model.new_session(); generate(..., session=s)), and what it holds, on the
    host: `tokens` (the ids of the cached rows, len(tokens) == cache.lens), `spans` (the image spans among them) and `images` (the tensor
    each span was encoded from).  A call keeps the longest reusable prefix (_reusable_prefix), truncates the cache to it, grows the cache
    when the call needs more rows than it has (to a multiple of 256) and runs only the tail: engine.prefill into this cache when nothing is
    kept, engine.extend otherwise.  `last`: reused_tokens, run_tokens and images_encoded of the last call.  capacity: rows of the cache
    (default config.max_position_embeddings), allocated at the first call.  `w_fp4`: the weight format that wrote the cached rows (True:
    the MXFP4 copies, generate(fp4_prefill=True)); a call with the other format reuses nothing (a full prefill, reused_tokens = 0) -
    rows of two different models are never mixed."""

    def __init__(self, model, capacity=None, fp8_kv=False):
        self.model, self.fp8_kv = model, bool(fp8_kv)
        self.capacity = int(capacity) if capacity is not None else int(model.config.max_position_embeddings)
        if self.capacity < 1:
            raise ValueError(f"new_session(capacity={capacity}): a session needs at least one cache row")
        self.cache = None
        self.last = dict(reused_tokens=0, run_tokens=0, images_encoded=0)
        self.reset()

    def reset(self):
        """Forget everything: the next call prefills its whole prompt.  The cache's memory is kept."""
        self.tokens, self.spans, self.images = [], [], []
        self.w_fp4 = False
        if self.cache is not None:
            self.cache.truncate(0)

    def _prefill(self, input_ids, images, room, w_fp4=False):
        """The session's form of engine.prefill(input_ids, None, images, room): -> (logits fp32 [1, V] at the prompt's last position,
        the session's cache holding the prompt, with `room` free rows behind it).  w_fp4: the prompt runs on the MXFP4 weight copies;
        rows that the other weight format wrote are not reused."""
        m = self.model
        eng = m.engine
        ids = [int(t) for t in input_ids[0].tolist()]
        new_spans = _image_spans(ids, getattr(m, "im_start_token", None), getattr(m, "im_end_token", None)) if images is not None else []
        new_images = [im[j] for im in (images or []) for j in range(im.shape[0])]
        keep = _reusable_prefix(self.tokens, self.spans, self.images, ids, new_spans, new_images)
        if bool(w_fp4) != self.w_fp4:
            keep = 0
        self.w_fp4 = bool(w_fp4)
        need = len(ids) + int(room)
        grown = -(-need // 256) * 256  # a call that needs more rows than the session has gets them in whole 256-row steps
        if self.cache is None or (need > self.cache.Smax and keep == 0):  # (nothing to carry over: no copy)
            self.cache = eng.new_cache(1, self.capacity if need <= self.capacity else grown, fp8=self.fp8_kv)
        elif need > self.cache.Smax:
            self.cache = eng.grow_cache(self.cache, grown)
        self.capacity = self.cache.Smax
        self.cache.truncate(keep)
        kept = sum(1 for _, e in new_spans if e <= keep)  # images whose spans lie in the kept prefix: not encoded again
        if keep == 0:
            logits, _ = eng.prefill(input_ids, None, images, 0, kv_fp8=self.fp8_kv, cache=self.cache, w_fp4=self.w_fp4)
            encoded = len(new_images)
        else:
            tail = new_images[kept:]
            encoded = len(tail)
            logits = eng.extend(self.cache, input_ids[:, keep:], [torch.stack(tail)] if tail else None, pos=keep, w_fp4=self.w_fp4)
        # (copies: a caller that changes its image tensor in place must not change what the session believes it encoded)
        self.tokens, self.spans, self.images = ids, new_spans, self.images[:kept] + [x.clone() for x in new_images[kept:len(new_spans)]]
        self.last = dict(reused_tokens=keep, run_tokens=len(ids) - keep, images_encoded=encoded)
        return logits, self.cache

    def _fed(self, out):
        """After a sampling loop: the cache holds the prompt and every generated token that was fed to the decoder, tokens =
        out[0, :cache.lens] (never more than out holds: a draft accepted beyond a stop is rolled back)."""
        n = min(int(self.cache.lens[0]), int(out.shape[1]))
        self.cache.truncate(n)
        self.tokens = [int(t) for t in out[0, :n].tolist()]


def _resolve_lengths(prompt_len, max_new_tokens, max_length):
    if max_new_tokens is not None:
        return prompt_len + int(max_new_tokens)
    if max_length is not None:
        return int(max_length)
    return max(prompt_len + 1, 20)  # HF GenerationConfig default max_length = 20


# decoding options this module implements, with transformers' GenerationConfig defaults
_DEFAULTS = dict(max_new_tokens=None, max_length=None, eos_token_id=None, pad_token_id=None, do_sample=False, temperature=1.0, top_k=50,
                 top_p=1.0, num_beams=1, length_penalty=1.0, early_stopping=False, use_cache=True, prompt_lookup_num_tokens=None,
                 max_matching_ngram_size=2, no_repeat_ngram_size=0, bad_words_ids=None, min_new_tokens=0, suppress_tokens=None,
                 begin_suppress_tokens=None, min_p=None, epsilon_cutoff=0.0, guidance_scale=None, negative_prompt_ids=None,
                 negative_prompt_attention_mask=None, assistant_model=None, num_assistant_tokens=None)
# options that are accepted only at the value that leaves the implemented modes unchanged (anything else is a decoding mode the
# reference's scripts never reach: refuse it instead of silently returning something different)
_NEUTRAL = dict(repetition_penalty=(1.0, None), num_return_sequences=(1, None), num_beam_groups=(1, None),
                penalty_alpha=(None, 0.0), typical_p=(1.0, None), min_length=(0, None),
                return_dict_in_generate=(False, None), output_scores=(False, None), output_logits=(False, None),
                output_attentions=(False, None), output_hidden_states=(False, None), logits_processor=(None,), prefix_allowed_tokens_fn=(None,),
                encoder_no_repeat_ngram_size=(0, None), diversity_penalty=(0.0, None), eta_cutoff=(0.0, None),
                renormalize_logits=(False, None), forced_bos_token_id=(None,), forced_eos_token_id=(None,), sequence_bias=(None,),
                synced_gpus=(False, None), bos_token_id=None, use_beam_search=None, trust_remote_code=None)


def _resolve_options(generation_config, kw):
    """HF precedence: GenerationConfig fields first, explicit keyword arguments over them; unknown names raise TypeError."""
    opt = dict(_DEFAULTS)
    if generation_config is not None:
        for k in list(_DEFAULTS) + list(_NEUTRAL):
            v = getattr(generation_config, k, None)
            if v is None:
                continue
            if k in _DEFAULTS:
                opt[k] = v
            elif _NEUTRAL[k] is not None and v not in _NEUTRAL[k] and v != []:
                raise NotImplementedError(f"generation_config.{k}={v!r} is not part of the decoding modes the reference's eval scripts use")
    for k, v in kw.items():
        if k in _DEFAULTS:
            opt[k] = _DEFAULTS[k] if v is None and k not in ("max_new_tokens", "max_length", "eos_token_id", "pad_token_id", "prompt_lookup_num_tokens") else v
        elif k in _NEUTRAL:
            ok = _NEUTRAL[k]
            if ok is not None and v not in ok and v != []:
                raise NotImplementedError(f"generate({k}={v!r}) is not part of the decoding modes the reference's eval scripts use")
        else:
            raise TypeError(f"generate() got an unexpected keyword argument '{k}'")
    _validate_constraints(opt)
    return opt


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _id_list(name, v):
    """suppress_tokens / begin_suppress_tokens: None or ids >= 0 (a list, a tuple or a tensor) -> list of ints ([]: off)."""
    v = _as_list(v)
    if any(not _is_int(t) or t < 0 for t in v):
        raise ValueError(f"`{name}` has to be a list of integers >= 0, but is {v}")
    return v


def _validate_constraints(opt):
    """The token-ban and min_p / epsilon options: refused here, before any device work (transformers' messages where its processors have
    one), and brought to one form - ints, lists of ints, floats; 0 / [] / None: off."""
    n = opt["no_repeat_ngram_size"]
    if not _is_int(n) or n < 0:
        raise ValueError(f"`no_repeat_ngram_size` has to be an integer >= 0, but is {n}")
    m = opt["min_new_tokens"]
    if not _is_int(m) or m < 0:
        raise ValueError(f"`min_new_tokens` has to be a positive integer, but is {m}")
    words = opt["bad_words_ids"]
    if words is not None and words != []:
        if not isinstance(words, list):
            raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {words}.")
        if any(not isinstance(w, list) for w in words):
            raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {words}.")
        if any(len(w) == 0 for w in words):
            raise ValueError(f"Each list in `bad_words_ids` has to be a non-empty list of positive integers, but is {words}.")
        if any(not _is_int(t) or t < 0 for w in words for t in w):
            raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {words}.")
    opt["bad_words_ids"] = [list(w) for w in words] if words else None
    opt["suppress_tokens"] = _id_list("suppress_tokens", opt["suppress_tokens"]) or None
    opt["begin_suppress_tokens"] = _id_list("begin_suppress_tokens", opt["begin_suppress_tokens"]) or None
    mp = opt["min_p"]
    if mp is not None:
        if isinstance(mp, bool) or not isinstance(mp, (int, float)) or not 0 <= mp <= 1.0:
            raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {mp}")
        opt["min_p"] = float(mp)
    e = opt["epsilon_cutoff"]
    if isinstance(e, bool) or not isinstance(e, (int, float)) or not 0 <= e < 1:
        raise ValueError(f"`epsilon_cutoff` has to be a float > 0 and < 1, but is {e}")
    opt["epsilon_cutoff"] = float(e)
    g = opt["guidance_scale"]
    if g is not None:
        if isinstance(g, bool) or not isinstance(g, (int, float)) or g != g or g in (float("inf"), float("-inf")):
            raise ValueError(f"`guidance_scale` has to be a real number (1 or None: off), but is {g!r}")
        opt["guidance_scale"] = None if g == 1 else float(g)  # (transformers adds the processor only when the scale is not None and != 1)


def _resolve_guidance(opt, negative_images=None, session=None, input_ids=None, attention_mask=None):
    """Classifier-free guidance of one call, from the resolved options: None when it is off, else dict(scale, ids, images) - ids the negative
    prompt int64 [1, Pn], or None for transformers' default (the prompt's last token alone), images its images.  Everything that cannot be
    served is refused here by name, before any device work: first what needs no tensor (a negative prompt without guidance - nothing is
    silently dropped -, num_beams > 1, session, prompt_lookup_num_tokens > 7), then the shapes (one un-padded prompt, one un-padded negative
    prompt).  A pure function of host data."""
    g, neg, nam = opt["guidance_scale"], opt["negative_prompt_ids"], opt["negative_prompt_attention_mask"]
    if g is None:
        for name, v in (("negative_prompt_ids", neg), ("negative_prompt_attention_mask", nam), ("negative_images", negative_images)):
            if v is not None:
                raise ValueError(f"`{name}` is given but guidance is off (`guidance_scale` is None or 1): it would be dropped")
        return None
    if opt["num_beams"] > 1:
        raise ValueError("`guidance_scale` cannot be combined with num_beams > 1 (beam search applies the processors to log-probabilities that "
                         "must not be renormalised: a different flow)")
    if session is not None:
        raise ValueError("`guidance_scale` cannot be combined with session=: a session holds one sequence, guidance decodes two")
    k = opt["prompt_lookup_num_tokens"]
    if _is_int(k) and k > 7:  # (anything that is no count is refused by the lookup's own check)
        raise ValueError(f"prompt_lookup_num_tokens = {k} with `guidance_scale`: the verify step runs 2 x (k + 1) rows of at most 16, so k <= 7")
    if input_ids.shape[0] != 1:
        raise ValueError(f"`guidance_scale` takes batch_size = 1 (transformers' processor is unbatched too), input_ids has batch_size = {input_ids.shape[0]}")
    if attention_mask is not None and not bool(torch.as_tensor(attention_mask).to(torch.bool).all()):
        raise ValueError("`guidance_scale` takes an un-padded prompt (attention_mask with zeros)")
    if neg is None:
        for name, v in (("negative_prompt_attention_mask", nam), ("negative_images", negative_images)):
            if v is not None:
                raise ValueError(f"`{name}` is given without `negative_prompt_ids` (the default negative prompt is the prompt's last token)")
        return dict(scale=g, ids=None, images=None)
    if not isinstance(neg, torch.Tensor) or neg.dim() != 2 or neg.shape[0] != 1 or neg.shape[1] < 1 or neg.dtype != torch.int64:
        raise ValueError(f"`negative_prompt_ids` has to be an int64 tensor [1, Pn >= 1], but is {tuple(neg.shape) if isinstance(neg, torch.Tensor) else type(neg).__name__}")
    if nam is not None:
        nam = torch.as_tensor(nam)
        if tuple(nam.shape) != tuple(neg.shape) or not bool(nam.to(torch.bool).all()):
            raise ValueError("`negative_prompt_attention_mask` has to be all ones in the shape of `negative_prompt_ids`: a padded negative prompt is refused")
    return dict(scale=g, ids=neg, images=negative_images)


def _resolve_assistant(opt, assistant, model, session=None, input_ids=None, attention_mask=None):
    """Assisted decoding of one call (assistant_model is set), from the resolved options: -> k, the tokens drafted per round
    (num_assistant_tokens; None: 5).  Everything that cannot be served is refused here by name, before any device work: first what needs no
    tensor, then the prompt's shape, last the two models' vocabularies.  A pure function of host data."""
    k = opt["num_assistant_tokens"]
    k = 5 if k is None else k
    if not _is_int(k) or not 1 <= k <= 15:
        raise ValueError(f"num_assistant_tokens = {k!r}: the verify step takes 1..15 drafted tokens (16 rows with the token before them)")
    if opt["prompt_lookup_num_tokens"] is not None:
        raise ValueError("`assistant_model` and `prompt_lookup_num_tokens` are two sources of drafts: pick one")
    if opt["num_beams"] > 1:
        raise ValueError("`assistant_model` drafts for greedy search and sampling: it cannot be combined with num_beams > 1")
    if not opt["use_cache"]:
        raise ValueError("assisted generate requires `use_cache=True`")
    if opt["guidance_scale"] is not None:
        raise ValueError("`assistant_model` cannot be combined with `guidance_scale`: the draft model follows the conditional sequence alone")
    if session is not None:
        raise ValueError("`assistant_model` cannot be combined with session=: the draft model keeps no cache between calls")
    if getattr(assistant, "engine", None) is None or getattr(assistant, "config", None) is None:
        raise ValueError(f"`assistant_model` has to be a merlin_amd model (with .engine and .config), but is {type(assistant).__name__}")
    if input_ids.shape[0] != 1:
        raise ValueError("assisted generate is only supported for batch_size = 1")
    if attention_mask is not None and not bool(torch.as_tensor(attention_mask).to(torch.bool).all()):
        raise ValueError("`assistant_model` takes an un-padded prompt (attention_mask with zeros)")
    va, vt = getattr(assistant.config, "vocab_size", None), model.config.vocab_size
    if va != vt:
        raise ValueError(f"`assistant_model` has vocab_size = {va}, the model {vt}: a draft model has to share the vocabulary")
    return k


def _assisted_caches(n, c, a):
    """The cache bookkeeping of one round of assisted decoding, as a pure function.  Before the round the sequence has n tokens and both
    caches hold the keys of seq[:n - 1].  The draft model was fed c tokens (seq[n - 1], d_1 .. d_{c-1}) and proposed d_1 .. d_c; the
    target verified [seq[n - 1], d_1 .. d_c] and a <= c drafts were accepted, so a + 1 tokens are emitted.  -> (target length, draft
    length, owed): the target keeps the last token and the accepted drafts, n + a rows = all but the last token of the new sequence; the
    draft cache is truncated to the same length, but holds only n - 1 + c rows - when a == c it is `owed` = 1 key short (d_c was never
    fed to it) and the next round feeds it that token first."""
    if not (n >= 1 and 1 <= c and 0 <= a <= c):
        raise ValueError(f"_assisted_caches(n={n}, c={c}, a={a})")
    target = n + a
    draft = min(n - 1 + c, target)
    return target, draft, target - draft


def _drafts_that_fit(n, k, max_len):
    """How many of a round's k drafts are used when the sequence has n tokens: the verify step emits one token more than it accepts, so
    c + 1 <= max_len - n.  0: only one token is left, a plain step."""
    return max(0, min(k, max_len - n - 1))


def _uncond_context(negative_ids, prompt_ids, new_tokens):
    """The unconditional sequence of a guided step, as a list of ints: the negative prompt (None: the prompt's last token, transformers'
    default) followed by every token generated so far."""
    head = [int(prompt_ids[-1])] if negative_ids is None else [int(t) for t in negative_ids]
    return head + [int(t) for t in new_tokens]


def _guided_ref(cond, uncond, g):
    """The guided scores of raw logits cond, uncond [..., V] in their own dtype: lu + g (lc - lu), lc / lu their log-softmaxes (transformers'
    UnbatchedClassifierFreeGuidanceLogitsProcessor; the restatement mh_guidance_mix is tested against)."""
    lc, lu = torch.log_softmax(cond, dim=-1), torch.log_softmax(uncond, dim=-1)
    return g * (lc - lu) + lu


def _pack_words(words):
    """[[ids of word 0], [ids of word 1], ...] -> (flat token list, offsets [n_words + 1]): word w is flat[off[w] : off[w + 1]]."""
    flat, off = [], [0]
    for w in words:
        flat.extend(int(t) for t in w)
        off.append(len(flat))
    return flat, off


def _unpack_words(flat, off):
    return [list(flat[off[w]:off[w + 1]]) for w in range(len(off) - 1)]


def _ban_plan(opt, eos_ids):
    """The token bans of one call, on the host: dict(ngram, words, always, begin, min_new) - words without the ones equal to [eos] (as
    NoBadWordsLogitsProcessor drops them), min_new 0 when there is no eos id to ban - or None when the call bans nothing."""
    words = [list(w) for w in (opt["bad_words_ids"] or []) if not any(list(w) == [e] for e in eos_ids)]
    plan = dict(ngram=int(opt["no_repeat_ngram_size"]), words=words, always=list(opt["suppress_tokens"] or []),
                begin=list(opt["begin_suppress_tokens"] or []), min_new=int(opt["min_new_tokens"]) if eos_ids else 0)
    return plan if any(plan.values()) else None


def _banned(ids_row, P, plan, eos_ids):
    """The token ids whose logits get -inf when the sequence so far is ids_row (a list of ints: the call's whole prompt, pads included,
    then the new tokens) and the prompt had P tokens: the five clauses of mh_ban_tokens, restated (the kernel is tested against this and
    against transformers' processors)."""
    h = [int(t) for t in ids_row]
    L = len(h)
    out = set()
    if plan is None:
        return out
    n = plan["ngram"]
    if n > 0:
        tail = h[L - n + 1:L] if n > 1 else []
        for i in range(0, L - n + 1):
            if h[i:i + n - 1] == tail:
                out.add(h[i + n - 1])
    for w in plan["words"]:
        k = len(w)
        if k == 1 or (k <= L and h[L - (k - 1):] == list(w[:-1])):  # (transformers skips a word longer than the context: k = L + 1 too)
            out.add(int(w[-1]))
    out.update(int(t) for t in plan["always"])
    if L == P:
        out.update(int(t) for t in plan["begin"])
    if L - P < plan["min_new"]:
        out.update(int(e) for e in eos_ids)
    return out


def _ban_tables(plan, eos_ids, P, dev):
    """The plan's device tables, built once per call: the keyword arguments of ops.ban_tokens that do not change from step to step."""
    t64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev) if v else None  # noqa: E731
    kw = dict(ngram=plan["ngram"], always=t64(plan["always"]), begin=t64(plan["begin"]), begin_index=P)
    if plan["words"]:
        flat, off = _pack_words(plan["words"])
        kw.update(words=t64(flat), word_off=torch.tensor(off, dtype=torch.int32, device=dev))
    if plan["min_new"] > 0:
        kw.update(eos=t64(list(eos_ids)), min_total=P + plan["min_new"])
    return kw


@dataclass
class _Call:
    """One generate() call with its arguments resolved once: everything a decoding loop needs, nothing it has to decide again."""
    model: object
    images: object
    attention_mask: object
    max_len: int
    eos_ids: list
    pad: int
    stop: _Stopper
    sel: dict = None             # the selection's arguments (_select); None: beam search
    streamer: object = None
    use_graph: bool = True
    fp8_weights: bool = False    # the decode step's weight format: at most one of the two
    fp4_weights: bool = False
    fp4_prefill: bool = False    # the prompt passes on the MXFP4 copies too (needs fp4_weights)
    fp8_kv: bool = False
    session: Session = None
    bans: dict = None            # _ban_plan; None: the call bans nothing
    guide: dict = None           # _resolve_guidance; None: guidance is off
    stats: dict = None           # engine.last_generate_stats of the call (greedy search and sampling)
    lookup: int = None           # prompt_lookup_num_tokens and, with it, max_matching_ngram_size
    max_ngram: int = None
    assistant: object = None     # assistant_model and, with it, num_assistant_tokens (None: 5)
    n_assist: int = None
    chain_graph: bool = False    # the draft's k steps of a round as one graph replay (assistant_chain_graph)
    num_beams: int = 1
    length_penalty: float = 1.0
    early_stopping: object = False
    share_prompt_kv: bool = False


@torch.no_grad()
def generate(model, input_ids, images=None, attention_mask=None, generation_config=None, stopping_criteria=None, streamer=None,
             use_graph=True, fp8_weights=False, fp8_kv=False, fp4_weights=False, share_prompt_kv=False, seed=None, session=None, negative_images=None,
             fp4_prefill=False, assistant_chain_graph=False, **kw):
    """transformers' `GenerationMixin.generate` for the modes the reference reaches (module docstring).  `streamer` follows HF's
    protocol (`put(prompt ids)`, `put(next tokens)` every step, `end()`): serve/cli.py:93-104 passes a TextStreamer.  Every
    other HF option is either implemented, accepted at its neutral value, or refused by name - nothing is silently dropped.
    fp8_kv=True stores the KV cache as e4m3 bytes with one power-of-two scale per (sequence, head, token) (engine.KVCache fp8=True):
    about half the cache bytes in every mode (greedy, sampling, beam search; with or without use_graph and fp8_weights / fp4_weights).
    fp4_weights=True runs the decode-step projections on MXFP4 copies of the decoder's Linear weights and lm_head (OCP e2m1 values, one
    power-of-two scale per 32 k, engine.quantize_decode_weights_fp4: about 0.53 bytes per weight streamed per token instead of 2; the
    prompt's prefill keeps the 16-bit weights unless fp4_prefill is set), in every mode and with either cache format; the alternative to
    fp8_weights, not an addition to it, and it needs use_cache=True (it applies to the decode step).
    fp4_prefill=True (with fp4_weights=True; alone it is refused) runs every prompt pass of the call on the same MXFP4 copies
    (ops.gemm_fp4w, engine.prefill / extend w_fp4=True): the prefill of greedy search, sampling, prompt lookup and beam search (also with
    share_prompt_kv), both sequences of a guided call and a session's prefill or extension.  The call is then ONE model from the first
    prompt token to the last generated one - the quantised one: the prompt's K/V rows are those the decode step would have written and
    the first token comes from the quantised lm_head - where the default mixes the 16-bit model's prompt rows with the quantised
    model's steps.  A session remembers which format wrote its rows; a call with the other format reuses none of them
    (reused_tokens = 0).  It buys consistency, not time - measured on one MI355X at the 7B geometry (profiles/fp4_prefill_bench.txt): a
    projection through ops.gemm_fp4w takes 1.3-1.5 times the tuned 16-bit GEMM's time at M = 4096 and 1.3-1.9 times at M = 613 (the down
    projection is the 1.9), the whole prefill of a 613-token prompt with one image 19.0 ms against 15.0 (x 1.27).
    share_prompt_kv=True (beam search only: num_beams > 1) keeps the prompt's keys and values once per prompt, where the prefill wrote
    them, instead of one copy per beam (engine.BeamKVCache): a beam owns only the rows of its generated tokens, re-ordering the beams
    rewrites an int32 ancestry table (mh_beam_ancestry) and moves no K/V, and the attention loads every prompt key once for all the beams
    (mh_attn_decode_beams).  The same search in the same arithmetic up to the order of the attention's partial sums; composes with fp8_kv,
    fp8_weights and fp4_weights.  The default (False) is the copying path.
    session=s (a Session, model.new_session()): the call continues from the KV cache the session kept - the longest prefix of the prompt that
    the cache already holds (same tokens, same image pixels) is not run again, only the tail is (engine.extend: no tower for images in
    the prefix) - and leaves what it fed in the session for the next call.  One un-padded prompt per call, use_cache=True, the session's
    cache format; every mode.  s.last = dict(reused_tokens, run_tokens, images_encoded) of the call.  None: every path as without it.
    Token bans - no_repeat_ngram_size, bad_words_ids, suppress_tokens, begin_suppress_tokens, min_new_tokens, with transformers' semantics
    and order (on the raw scores, before the warpers; in beam search on the log-probabilities, a banned candidate's mass is not
    renormalised) - are one mh_ban_tokens launch per step on the device (module docstring).  The history they see is the ids tensor the
    stopping criteria are handed at that step: the call's whole prompt, its pads wherever they sit, then the new tokens - also with a
    session, however much of the prompt came from its cache.  min_p and epsilon_cutoff (do_sample=True only) follow top-p.  All of these
    work on the logits alone, so they compose with every mode and with use_graph, use_cache=False, prompt_lookup_num_tokens, fp8_kv,
    fp8_weights, fp4_weights, share_prompt_kv and sessions without further work.
    Classifier-free guidance - guidance_scale=g (a real number; None or 1: off, and every path runs and launches as without it), with
    transformers' semantics: the scores of a step are lu + g (lc - lu), lc the log-softmax of the logits given the prompt and lu given the
    unconditional context, which is negative_prompt_ids [1, Pn] (negative_prompt_attention_mask: all ones or None; default: the prompt's
    last token) followed by every generated token; the bans, the warpers and the selection act on these scores, greedy takes their argmax.
    negative_images: the images whose spans lie in the negative prompt, in the form of `images` (None: text only) - e.g. the prompt with
    its image against the same text without it.  One un-padded prompt; greedy and sampling (selection key (seed, step, row 0)); with
    use_cache the two sequences share one B = 2 cache (engine.pair_cache: one pass over the weights per token, plus one mh_guidance_mix
    launch), use_cache=False runs two forwards per token; composes with use_graph, fp8_kv, fp8_weights, fp4_weights, the bans, min_p,
    epsilon_cutoff, streamer and stopping criteria (both see the conditional ids only) and prompt_lookup_num_tokens <= 7 (2 (k + 1) <= 16
    verify rows).  Refused by name: num_beams > 1, session=, batch_size > 1, a padded prompt or negative prompt, and a negative prompt or
    negative_images while guidance is off.  engine.last_generate_stats["guided_steps"]: the steps whose scores were mixed.
    Assisted decoding - assistant_model=draft (a second merlin_amd model with the same vocab_size; any depth, width or head count the
    decode kernels take), num_assistant_tokens=k (1..15; None: 5; a generation_config's value counts like the keyword): every round the
    draft model proposes k tokens - its own decode steps on its own 16-bit cache, the call's bans and the call's selection with the plain
    path's key (seed, token number, row 0) after each - and the model verifies them with the last token in ONE step of k + 1 rows
    (engine.verify_step) and keeps the agreeing prefix plus one: the speculative contract of prompt_lookup_num_tokens, not rejection
    sampling.  The output is the plain path's token stream whatever the draft proposes (greedy: exact match; sampling: draft and model share
    the uniform of a position).  The draft gets `images` if it has a vision tower, else it reads the same ids text-only.  With use_graph
    every draft step is a replay of the draft's single-step graph followed by the eager ban and selection launches; without it the steps
    run eagerly.  assistant_chain_graph=True (needs use_graph and assistant_model; refused otherwise): the k draft steps, bans and
    selections of a round are ONE graph replay instead (engine.capture_draft_graph: mh_ban_tokens_dev / mh_select_tokens_dev read the token
    number and the length from two device counters).  It is opt-in because it measured as a tie - within 3 % either way of the per-step arm
    at k = 3, 5, 7 on one MI355X with 67 M and 297 M parameter drafts (profiles/decode_assisted_bench.txt): a draft step's GPU time exceeds
    what the host spends enqueueing it, so there is no host time left to save.  All arms emit the same tokens.  Greedy and sampling;
    composes with use_graph, fp8_kv,
    fp8_weights, fp4_weights (fp4_prefill) on the model - the draft runs 16-bit -, the bans, min_p, epsilon_cutoff, streamer and stopping
    criteria.  Refused by name: num_beams > 1, batch_size > 1, a padded prompt, use_cache=False, guidance_scale, session=,
    prompt_lookup_num_tokens beside it, another vocab_size, k outside 1..15, an assistant without .engine / .config.
    engine.last_generate_stats gains "draft_steps" (assisted calls only): the draft model's decode steps, catch-up steps included (after a
    fully accepted round the draft cache is one key short) and, in the chain graph, the steps of a round near max_length that ran unused.
    None: every path runs and launches as without it."""
    o = _resolve_options(generation_config, kw)
    max_new_tokens, max_length, eos_token_id, pad_token_id = o["max_new_tokens"], o["max_length"], o["eos_token_id"], o["pad_token_id"]
    do_sample, temperature, top_k, top_p = o["do_sample"], o["temperature"], o["top_k"], o["top_p"]
    num_beams, length_penalty, early_stopping, use_cache = o["num_beams"], o["length_penalty"], o["early_stopping"], o["use_cache"]
    if fp8_kv and not use_cache:
        raise ValueError("fp8_kv=True stores the KV cache in fp8: it needs use_cache=True")
    if fp4_weights and fp8_weights:
        raise ValueError("fp4_weights and fp8_weights are alternatives: pick one weight format for the decode step")
    if fp4_weights and not use_cache:
        raise ValueError("fp4_weights=True applies to the KV-cache decode step: it needs use_cache=True")
    if fp4_prefill and not fp4_weights:
        raise ValueError("fp4_prefill=True runs the prompt on the MXFP4 copies that fp4_weights=True decodes with: it needs fp4_weights=True")
    if share_prompt_kv and num_beams <= 1:
        raise ValueError("share_prompt_kv=True shares the prompt's KV cache among the beams of beam search: it needs num_beams > 1")
    if share_prompt_kv and num_beams > 16:
        raise ValueError("share_prompt_kv=True takes num_beams <= 16 (the beams of a prompt are one query tile of the attention kernel)")
    guide = _resolve_guidance(o, negative_images, session, input_ids, attention_mask)  # (refusals by name, before any device work)
    if session is not None:  # a session continues ONE un-padded sequence on its own KV cache: refused before any device work otherwise
        if input_ids.shape[0] != 1:
            raise ValueError(f"session: a session holds one sequence, input_ids has batch_size = {input_ids.shape[0]}")
        if attention_mask is not None and not bool(torch.as_tensor(attention_mask).to(torch.bool).all()):
            raise ValueError("session: a session takes an un-padded prompt (attention_mask with zeros)")
        if not use_cache:
            raise ValueError("session: continuing from a kept KV cache needs use_cache=True")
        if bool(fp8_kv) != bool(session.fp8_kv):
            raise ValueError(f"session: fp8_kv={bool(fp8_kv)} but the session's cache was made with fp8_kv={bool(session.fp8_kv)}")
    lookup, max_ngram = o["prompt_lookup_num_tokens"], o["max_matching_ngram_size"]
    if lookup is not None:  # prompt-lookup speculative decoding: refused before any device work where it does not apply
        if num_beams > 1:
            raise ValueError("prompt_lookup_num_tokens drafts for greedy search and sampling: it cannot be combined with num_beams > 1")
        if not use_cache:
            raise ValueError("assisted generate requires `use_cache=True`")
        if input_ids.shape[0] > 1:
            raise ValueError("assisted generate is only supported for batch_size = 1")
        if not isinstance(lookup, int) or isinstance(lookup, bool) or not 1 <= lookup <= 15:
            raise ValueError(f"prompt_lookup_num_tokens = {lookup!r}: the verify step takes 1..15 drafted tokens (16 rows with the token before them)")
        if not isinstance(max_ngram, int) or max_ngram <= 0:
            raise ValueError("Invalid max_matching_ngram_size or num_output_tokens")
    assistant, n_assist = o["assistant_model"], None
    if assistant_chain_graph and (assistant is None or not use_graph):
        raise ValueError("assistant_chain_graph=True captures the draft model's steps of a round into one graph: it needs `assistant_model` and use_graph=True")
    if assistant is not None:
        n_assist = _resolve_assistant(o, assistant, model, session, input_ids, attention_mask)  # (refusals by name, before any device work)
    cfg = model.config
    eos_ids = _as_list(cfg.eos_token_id if eos_token_id is None else eos_token_id)
    pad = pad_token_id if pad_token_id is not None else (cfg.pad_token_id if cfg.pad_token_id is not None else (eos_ids[0] if eos_ids else 0))
    B, P = input_ids.shape
    max_len = _resolve_lengths(P, max_new_tokens, max_length)
    if max_len <= P:
        return input_ids
    if seed is None:  # torch.manual_seed governs the stream, like HF's torch.multinomial
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if do_sample else 0
    beams = num_beams > 1
    if beams:
        if do_sample:
            raise NotImplementedError("beam-sample is not one of the reference's decoding modes (eval scripts: num_beams=5, do_sample unset)")
        if streamer is not None:  # (transformers raises the same way)
            raise ValueError("`streamer` cannot be used with beam search. Make sure that `num_beams` is set to 1.")
        if attention_mask is not None and not bool(attention_mask.to(torch.bool).all()):
            raise NotImplementedError("beam search takes un-padded prompts (the reference's eval scripts decode one prompt at a time)")
        sel = stats = None
    else:
        sel = dict(do_sample=bool(do_sample), temperature=float(temperature), top_k=int(top_k or 0), top_p=float(top_p), seed=seed)
        if do_sample and (o["min_p"] is not None or o["epsilon_cutoff"] > 0.0):
            sel.update(min_p=o["min_p"], epsilon_cutoff=o["epsilon_cutoff"])
        stats = dict(plain_steps=0, verify_steps=0, drafted=0, accepted=0)
        if assistant is not None:  # (a key of assisted calls only) the draft model's decode steps
            stats["draft_steps"] = 0
    call = _Call(model=model, images=images, attention_mask=None if beams else attention_mask,  # (beam search: all ones, as checked)
                 max_len=max_len, eos_ids=eos_ids, pad=pad, stop=_Stopper(max_len, eos_ids, stopping_criteria), sel=sel, streamer=streamer,
                 use_graph=use_graph, fp8_weights=bool(fp8_weights), fp4_weights=bool(fp4_weights), fp4_prefill=bool(fp4_prefill), fp8_kv=bool(fp8_kv), session=session,
                 bans=_ban_plan(o, eos_ids), guide=guide, stats=stats, lookup=lookup, max_ngram=None if lookup is None else max_ngram,
                 assistant=assistant, n_assist=n_assist, chain_graph=bool(assistant_chain_graph),
                 num_beams=num_beams, length_penalty=length_penalty, early_stopping=early_stopping, share_prompt_kv=bool(share_prompt_kv))
    if beams:
        return _beam_search(call, input_ids)
    if streamer is not None:
        streamer.put(input_ids.cpu())
    if getattr(model, "engine", None) is not None:
        model.engine.last_generate_stats = stats
    if lookup is not None:
        out = _sample_lookup(call, input_ids)
    elif assistant is not None:
        out = _sample_assisted(call, input_ids)
    elif not use_cache:
        out = _sample_recompute(call, input_ids)
    else:
        out = _sample_cached(call, input_ids)
        stats["plain_steps"] = max(0, out.shape[1] - input_ids.shape[1] - 1)  # every new token but the first (the prefill's) is one decode step
    if guide is not None:  # (a key of guided calls only) the prefill pair, then every decode and verify step (use_cache=False: every forward pair)
        stats["guided_steps"] = 1 + stats["plain_steps"] + stats["verify_steps"] if use_cache else out.shape[1] - input_ids.shape[1]
    if session is not None:
        stats.update(session.last)
    if streamer is not None:
        streamer.end()
    return out


def _select(logits, V, sel, step):
    """sel: the selection kernel's keyword arguments as generate() resolved them (do_sample, temperature, top_k, top_p, seed and, only
    where they are set, min_p and epsilon_cutoff)."""
    return O.select_tokens(logits, V, step=step, **sel)


def _guided_prefill(eng, guide, input_ids, images, room, fp8_kv, V, w_fp4=False):
    """The guided form of engine.prefill: the prompt and the unconditional context prefilled one after the other, their caches paired
    (engine.pair_cache: row 0 conditional, row 1 unconditional, `room` free rows behind the longer one) -> (guided scores fp32 [1, >= V],
    the B = 2 cache)."""
    lc, cc = eng.prefill(input_ids, None, images, 0, kv_fp8=fp8_kv, w_fp4=w_fp4)
    lu, cu = eng.prefill(guide["ids"] if guide["ids"] is not None else input_ids[:, -1:], None, guide["images"], 0, kv_fp8=fp8_kv, w_fp4=w_fp4)
    return O.guidance_mix(lc, lu, guide["scale"], V, out=lc), eng.pair_cache(cc, cu, room)


def _sample_recompute(call, ids):
    """use_cache=False: full-sequence forward per token (the cross-check of the cached path).  guide: a second forward on the
    unconditional context per token, then the mix."""
    model, images, attention_mask, max_len, eos_ids, pad = call.model, call.images, call.attention_mask, call.max_len, call.eos_ids, call.pad
    stop, sel, streamer, bans, guide = call.stop, call.sel, call.streamer, call.bans, call.guide
    V = model.config.vocab_size
    unfinished = torch.ones(ids.shape[0], dtype=torch.bool, device=ids.device)
    step = 0
    P = ids.shape[1]
    tables = hist = None
    while True:
        out = model.forward(input_ids=ids, attention_mask=attention_mask, images=images)
        logits = out.logits[:, -1, :].float().contiguous()
        if guide is not None:
            neg = None if guide["ids"] is None else guide["ids"][0].tolist()
            un = torch.tensor([_uncond_context(neg, ids[0, :P].tolist(), ids[0, P:].tolist())], dtype=torch.int64, device=ids.device)
            un = model.forward(input_ids=un, images=guide["images"]).logits[:, -1, :].float().contiguous()
            O.guidance_mix(logits, un, guide["scale"], V, out=logits)
        if bans is not None:
            if tables is None:  # the history lives on the logits' device in one [B, max_len] buffer
                tables = _ban_tables(bans, eos_ids, P, logits.device)
                hist = torch.full((ids.shape[0], max_len), pad, dtype=torch.int64, device=logits.device)
                hist[:, :P] = ids
            O.ban_tokens(logits, V, hist, len0=P + step, **tables)
        nxt = _select(logits, V, sel, step).to(ids.device)
        if eos_ids:
            nxt = torch.where(unfinished, nxt, torch.full_like(nxt, pad))
        if streamer is not None:
            streamer.put(nxt.cpu())
        ids = torch.cat([ids, nxt[:, None]], dim=1)
        if hist is not None and P + step < max_len:
            hist[:, P + step] = nxt
        if attention_mask is not None:
            attention_mask = torch.cat([attention_mask, torch.ones_like(attention_mask[:, :1])], dim=1)
        unfinished = unfinished & ~stop(ids, None)
        step += 1
        if not bool(unfinished.any()):
            return ids


class _Stepper:
    """What the loops on a KV cache share, built from the resolved call: the prefill choice, graph capture, the decode and the verify step
    with the guided mix, the ban launch on tables built once, and the ids buffer of the two sampling loops.  The loops keep their policy."""

    def __init__(self, call):
        self.call, self.eng, self.V = call, call.model.engine, call.model.config.vocab_size
        self.weights = dict(fp8=call.fp8_weights, fp4=call.fp4_weights)
        self.cache = self.graph = self.vgraph = self.tables = self.lens = None

    def prefill(self, input_ids, room):
        """The prompt into a cache with `room` free rows behind it - the guided pair, the session's cache or a new one -> the scores that
        select the first token; the cache is self.cache."""
        c = self.call
        if c.guide is not None:  # one sequence to the caller; rows (conditional, unconditional) to the decode step
            logits, self.cache = _guided_prefill(self.eng, c.guide, input_ids, c.images, room, c.fp8_kv, self.V, w_fp4=c.fp4_prefill)
        elif c.session is not None:
            logits, self.cache = c.session._prefill(input_ids, c.images, room, w_fp4=c.fp4_prefill)
        else:
            logits, self.cache = self.eng.prefill(input_ids, c.attention_mask, c.images, room, kv_fp8=c.fp8_kv, w_fp4=c.fp4_prefill)
        self.input_ids, self.P, self.logits0 = input_ids, input_ids.shape[1], logits
        if c.bans is not None:
            self.tables = _ban_tables(c.bans, c.eos_ids, self.P, logits.device)
        return logits

    def capture(self, T=0):
        """The decode step as one replayable HIP graph on self.cache and, T >= 1 (the lookup loop), the [rows, T] verify step as another."""
        c = self.call
        self.T = T
        if c.use_graph and self.logits0.is_cuda and c.max_len - self.P > 2:
            self.graph, self.g_tok, self.g_logits = self.eng.capture_decode_graph(self.cache, **self.weights)
            if T:
                self.vgraph, self.v_tok, self.v_logits = self.eng.capture_verify_graph(self.cache, T, **self.weights)

    def ids_buffer(self, cells):
        """The sequence as the criteria, the bans and the drafter see it, in one preallocated buffer [B, cells] on the device: the prompt,
        pads behind it.
        Right-padded prompts (ones then zeros; an extension - HF wants left padding): each row continues from its own length, the criteria
        see the pads in the middle and finish() compacts.  Anything else (HF's left padding, holes) follows transformers: new tokens are
        appended after the padded prompt, keys are the valid positions only, rotary positions stay absolute (the engine's unpad / pad
        attention path + compacted KV cache).  ONE decision, the engine's (made on the device from the mask in forward(): a right-padded
        prefix keeps the lens fast path, anything else - or engine.force_unpad - compacts the valid keys and sets cache.rpos): generate()
        follows it instead of classifying again."""
        c, dev = self.call, self.logits0.device
        if c.attention_mask is not None and c.guide is None:  # (guided: all ones, or guidance is refused)
            am = c.attention_mask.to(dev).to(torch.bool)
            if not bool(am.all()) and self.cache.rpos is None:
                self.lens = am.sum(dim=1)
        self.seq = torch.full((self.input_ids.shape[0], cells), c.pad, dtype=torch.int64, device=dev)
        self.seq[:, :self.P] = self.input_ids.to(dev)
        return self.seq

    def step(self, tokens):
        """One decode step on tokens int64 [B] (guided: the one token goes to both rows) -> the scores of the next token."""
        guide = self.call.guide
        if self.graph is not None:
            self.g_tok.copy_(tokens)
            self.graph.replay()
            logits = self.g_logits
        else:
            logits = self.eng.decode_step(tokens if guide is None else tokens.repeat(2), self.cache, **self.weights)
        if guide is not None:  # row 0 becomes the guided scores, in place; the bans and the selection see that row alone
            logits = O.guidance_mix(logits[:1], logits[1:], guide["scale"], self.V, out=logits[:1])
        return logits

    def verify(self, last, draft, c):
        """One verify step of T rows per cache row on `last` [1] followed by the c drafted tokens draft[:, :c] -> scores [1, T, >= V]; does
        not advance the cache.  A short draft is padded to the step's T rows; their scores are not looked at."""
        call, guide = self.call, self.call.guide
        toks = self.v_tok if self.vgraph is not None else torch.empty(self.cache.B, self.T, dtype=torch.int64, device=last.device)
        toks[:, 0] = last
        toks[:, 1:] = call.pad
        toks[:, 1:1 + c] = draft[:, :c]
        if self.vgraph is not None:
            self.vgraph.replay()
            logits = self.v_logits
        else:
            logits = self.eng.verify_step(toks, self.cache, **self.weights)
        if guide is not None:  # rows t and T + t of the step's buffer -> conditional row t, in place
            O.guidance_mix(logits[0], logits[1], guide["scale"], self.V, out=logits[0])
            logits = logits[:1]
        return logits

    def ban(self, logits, len0, ids=None, **kw):
        """-inf into the banned columns of the step's scores given the sequences ids (default: the ids buffer) of length len0: ONE
        mh_ban_tokens launch; nothing when the call bans nothing."""
        if self.tables is not None:
            O.ban_tokens(logits, self.V, self.seq if ids is None else ids, len0=len0, **kw, **self.tables)

    def finish(self, n):
        """The first n cells of the ids buffer as the call's result; a session keeps what was fed."""
        c, P = self.call, self.P
        cur = self.seq[:, :n]
        if self.lens is not None:  # right-padded prompts: each row's continuation starts at its own length
            cur = _compact(self.seq[:, :P], self.lens, self.seq[:, P:n], c.pad)
        if c.session is not None:  # (the last emitted token was never fed to the decoder, a rejected draft's tail is behind cache.lens)
            c.session._fed(cur)
        return cur.to(self.input_ids.device).contiguous()


def _sample_cached(call, input_ids):
    """Greedy search / sampling on the KV cache: one decode step per token."""
    c, st = call, _Stepper(call)
    B, P = input_ids.shape
    max_new = c.max_len - P
    logits = st.prefill(input_ids, max_new)
    st.capture()
    seq = st.ids_buffer(c.max_len)
    unfinished = torch.ones(B, dtype=torch.bool, device=seq.device)
    for step in range(max_new):
        st.ban(logits, P + step)
        nxt = _select(logits, st.V, c.sel, step)
        if c.eos_ids:
            nxt = torch.where(unfinished, nxt, torch.full_like(nxt, c.pad))
        if c.streamer is not None:
            c.streamer.put(nxt.cpu())
        seq[:, P + step] = nxt
        unfinished = unfinished & ~c.stop(seq[:, :P + step + 1], None)
        if not bool(unfinished.any()) or step + 1 == max_new:
            break
        logits = st.step(nxt)
    return st.finish(P + step + 1)


def _prompt_lookup(ids, k, max_ngram, max_length):
    """transformers' PromptLookupCandidateGenerator.get_candidates (no logits processor, no EOS cut) on a list of token ids: for n from
    min(max_ngram, len - 1) down to 1, the EARLIEST window equal to the last n tokens whose continuation
    ids[start : min(start + k, len, max_length)] is not empty; [] when no n has one, or when only one more token fits (max_length ==
    len + 1: the verifying step emits one token more than it accepts).  The restatement mh_ngram_draft is tested against."""
    ids = [int(t) for t in ids]
    n_ids = len(ids)
    if max_length == n_ids + 1:
        return []
    for n in range(min(max_ngram, n_ids - 1), 0, -1):
        tail = ids[n_ids - n:]
        for i in range(n_ids - n + 1):
            if ids[i:i + n] == tail:
                start = i + n
                end = min(start + k, n_ids, max_length)
                if start < end:
                    return ids[start:end]
    return []


def _accept(draft, selected, room, stops):
    """The accept rule of one verify step, as a pure function.  draft: the c drafted tokens; selected: the tokens selected from the verify
    step's c + 1 (or more) logits rows, selected[i] conditioned on draft[:i]; room: how many tokens still fit below max_length;
    stops(i) -> bool: the stopping criteria and EOS test on the sequence with selected[:i + 1] appended (called in order, each prefix once,
    never past a stop).  -> (emitted tokens, a = drafted tokens accepted, stopped).  The longest prefix on which draft and selection agree is
    accepted and the a + 1 selected tokens are emitted - up to and including the first stop, and never more than `room`."""
    a = 0
    while a < len(draft) and int(draft[a]) == int(selected[a]):
        a += 1
    out, stopped = [], False
    for i in range(min(a + 1, room)):
        out.append(int(selected[i]))
        if stops(i):
            stopped = True
            break
    return out, a, stopped


def _draft_loop(seq, P, max_len, stop, streamer, stats, first, drafter, target):
    """The speculative loop, one sequence, with everything that touches a model behind two objects - the lookup drafter and the model
    drafter differ in `drafter` alone; tests drive it with pure functions on a CPU ids buffer.  seq int64 [1, cells]: the ids buffer holding
    the P prompt tokens; first: the token selected from the prefill's scores, as a list.
      drafter.propose(n) -> (d, handle): d >= 0 drafted tokens behind seq[:n] (0: none; never more than fit below max_len with the one
          token a verify step adds) and whatever target.verify needs to find them;  drafter.commit(n, d, a): a of them were accepted;
          drafter.steps: decoder steps it ran (a drafter without a model: 0).
      target.plain(n) -> [token number n - P]: one decode step on seq[0, n - 1], its bans and selection;
      target.verify(n, handle, d) -> (the d + 1 tokens selected from ONE verify step on seq[0, n - 1] and the drafts, selected[t]
          conditioned on draft[:t]; the d drafts), both as lists;  target.advance(m): the step's first m rows are keys now.
    Every round emits the agreeing prefix plus one (_accept) - up to a stop, never beyond max_len.  Selection being keyed by position, the
    token stream is the plain path's whatever the drafter proposes.  -> the sequence's length; stats counts the rounds."""
    n = P  # valid length of seq

    def emit(cand, draft):
        """Append the accepted part of `cand` (selected tokens, on the host) to seq; -> (tokens emitted, accepted, stopped)."""
        nonlocal n
        base = n

        def stops(i):
            seq[0, base + i] = cand[i]
            return bool(stop(seq[:, :base + i + 1], None)[0])

        out, a, stopped = _accept(draft, cand, max_len - n, stops)
        n = base + len(out)
        if streamer is not None:
            streamer.put(torch.tensor([out], dtype=torch.int64))
        return out, a, stopped

    out, _, stopped = emit(first, [])
    while not stopped and n < max_len:
        d, handle = drafter.propose(n)
        if d == 0:
            cand = target.plain(n)
            stats["plain_steps"] += 1
            out, _, stopped = emit(cand, [])
            continue
        before = n
        picked, draft = target.verify(n, handle, d)
        out, a, stopped = emit(picked, draft)
        target.advance(a + 1)  # the last token and the a accepted drafts are keys now; the stale rows behind them get overwritten
        drafter.commit(before, d, a)
        stats["verify_steps"] += 1
        stats["drafted"] += d
        stats["accepted"] += min(a, len(out))  # (a draft token that agreed beyond a stop or max_length was not emitted)
    if "draft_steps" in stats:
        stats["draft_steps"] = drafter.steps
    return n


class _StepTarget:
    """_draft_loop's target on a _Stepper: the decode and the verify step of the call's model with the bans and the selection."""

    def __init__(self, st, seq, k):
        self.st, self.seq, self.k = st, seq, k

    def plain(self, n):
        st, c = self.st, self.st.call
        logits = st.step(self.seq[:, n - 1])
        st.ban(logits, n)
        return _select(logits, st.V, c.sel, n - st.P).tolist()

    def verify(self, n, draft_dev, d):
        st, c, seq, T = self.st, self.st.call, self.seq, self.k + 1
        logits = st.verify(seq[:, n - 1], draft_dev, d)
        if c.bans is not None:  # row t is conditioned on seq[:n] + draft[:t]: the draft goes behind the sequence (emit overwrites those cells)
            seq[0, n:n + d] = draft_dev[0, :d]
            st.ban(logits[0], n, len_step=1, ld_ids=0)
        picked = O.select_tokens_multi(logits, st.V, step0=n - st.P, **c.sel)[:, 0]  # [T]
        both = torch.cat([picked, draft_dev[0]]).tolist()  # one transfer
        return both[:d + 1], both[T:T + d]

    def advance(self, m):
        self.st.cache.advance(m)


class _NgramDrafter:
    """Prompt lookup: up to k tokens from the sequence itself (mh_ngram_draft; _prompt_lookup is its restatement).  No model, no state."""
    steps = 0

    def __init__(self, seq, k, max_ngram, max_len):
        self.seq, self.k, self.max_ngram, self.max_len = seq, k, max_ngram, max_len

    def propose(self, n):
        draft_dev, cnt = O.ngram_draft(self.seq, n, self.max_ngram, self.k, self.max_len)
        return int(cnt[0]), draft_dev

    def commit(self, n, d, a):
        pass


class _ModelDrafter:
    """A draft model (generate(assistant_model=...)): k decode steps of its own engine on its own 16-bit cache, each followed by the call's
    bans (history seq[:n] + draft[:i]) and the target's own selection with key (seed, emitted + i, row 0).  tok int64 [k + 1] holds
    [seq[n - 1], d_1 .. d_k]: step i feeds tok[i] and selects tok[i + 1].
    chain=True: the k steps are ONE graph replay (engine.capture_draft_graph) - per round the host writes tok[0] and the two device
    counters (emitted, n: one 16-byte copy from pinned memory) and replays; the chain always runs its k steps, a round near max_length
    uses the first drafts that fit.  chain=False: the same steps one by one through the scalar entry points (the decode step itself
    replayed from a graph when graph=True).  `fed`: the draft cache's length, kept on the host (_assisted_caches)."""

    def __init__(self, call, seq, k, chain, graph):
        self.call, self.seq, self.k, self.chain, self.steps = call, seq, k, bool(chain), 0
        self.graph_steps = bool(graph) and not self.chain
        self.eng, self.V = call.assistant.engine, call.model.config.vocab_size
        self.sgraph = self.cgraph = None

    def prefill(self, input_ids, tables):
        """The prompt into the draft's cache (with the call's images if the draft has a vision tower, else text-only on the same ids),
        room for the new tokens and k rows of a rejected draft's tail; then the captures."""
        c, k, eng = self.call, self.k, self.eng
        P = input_ids.shape[1]
        tower = getattr(c.assistant.get_model(), "vision_tower", None) if hasattr(c.assistant, "get_model") else None
        _, self.cache = eng.prefill(input_ids, None, c.images if tower is not None else None, c.max_len - P + k)
        dev = self.cache.lens.device
        self.fed, self.P, self.tables = P, P, tables
        if self.chain:
            self.counters = torch.zeros(2, dtype=torch.int64, device=dev)  # [emitted, n]; n is read as int32 (the low word)
            self.host = torch.zeros(2, dtype=torch.int64).pin_memory()
            self._set_counters(P + 1)
            self.cgraph, self.tok = eng.capture_draft_graph(self.cache, k, c.sel, tables, self.seq, (self.counters[:1], self.counters[1:].view(torch.int32)))
        else:
            self.tok = torch.zeros(k + 1, dtype=torch.int64, device=dev)
        if self.chain or self.graph_steps:  # the single step: every step of the per-step arm, the catch-up step of the chain arm
            self.sgraph, self.s_tok, self.s_logits = eng.capture_decode_graph(self.cache)

    def _set_counters(self, n):
        self.host[0], self.host[1] = n - self.P, n
        self.counters.copy_(self.host, non_blocking=True)

    def _step(self, token):
        """One decode step of the draft on token int64 [1] -> its scores."""
        self.steps += 1
        self.fed += 1
        if self.sgraph is not None:
            self.s_tok.copy_(token)
            self.sgraph.replay()
            return self.s_logits
        return self.eng.decode_step(token, self.cache)

    def propose(self, n):
        c, k, seq, tok = self.call, self.k, self.seq, self.tok
        d = _drafts_that_fit(n, k, c.max_len)
        if d == 0:
            return 0, None
        while self.fed < n - 1:  # a key the last round left owed (its last draft was accepted, and never fed)
            self._step(seq[0, self.fed:self.fed + 1])
        tok[:1].copy_(seq[0, n - 1:n])
        if self.chain:
            self._set_counters(n)
            self.cgraph.replay()
            self.steps += k
            self.fed += k
        else:
            for i in range(d):
                logits = self._step(tok[i:i + 1])
                if self.tables is not None:
                    O.ban_tokens(logits, self.V, seq, len0=n + i, **self.tables)
                tok[i + 1:i + 2] = O.select_tokens(logits, self.V, step=n - self.P + i, **c.sel)
                if self.tables is not None:  # the next step's ban reads the draft behind the sequence
                    seq[0, n + i:n + i + 1] = tok[i + 1:i + 2]
        return d, tok[None, 1:]

    def commit(self, n, d, a):
        keep = min(self.fed, _assisted_caches(n, d, a)[0])
        self.cache.truncate(keep)
        self.fed = keep


def _sample_lookup(call, input_ids):
    """Greedy search / sampling with prompt-lookup drafts (one sequence): every step drafts up to k tokens from the sequence itself
    (mh_ngram_draft), runs them with the last token through ONE verify step of k + 1 rows (engine.verify_step: the weights are streamed
    once), selects all k + 1 rows with the plain path's RNG key - row t as token number emitted + t - and keeps the agreeing prefix plus
    one (_accept).  Selection being keyed by position, the token stream is the plain path's.  No draft: the plain decode step.
    guide: the steps run on the paired cache with the same tokens in both rows ([2, T] verify rows, 2 T <= 16), row pair t is mixed into
    conditional row t before the bans and the selection, and both sequences keep the same accepted count."""
    c, st = call, _Stepper(call)
    k, max_len = c.lookup, c.max_len
    P = input_ids.shape[1]
    logits = st.prefill(input_ids, max_len - P + k)  # k rows of room for a rejected draft's tail
    st.capture(k + 1)
    # (with bans: k cells more, a draft is written behind the sequence before it is verified)
    seq = st.ids_buffer(max_len + (k if c.bans is not None else 0))
    st.ban(logits, P)
    first = _select(logits, st.V, c.sel, 0).tolist()
    n = _draft_loop(seq, P, max_len, c.stop, c.streamer, c.stats, first, _NgramDrafter(seq, k, c.max_ngram, max_len), _StepTarget(st, seq, k))
    return st.finish(n)


def _sample_assisted(call, input_ids):
    """Greedy search / sampling with a draft model (one sequence): _sample_lookup's loop with _ModelDrafter in the drafter's place.  Every
    round the draft model proposes k tokens (fewer near max_length), the target verifies them with the last token in one step of k + 1
    rows and keeps the agreeing prefix plus one.  Both caches get k spare rows; the ids buffer k spare cells (the drafts are written
    behind the sequence before they are verified).  call.chain_graph: the draft steps of a round as one graph (where the call uses graphs at all)."""
    c, st = call, _Stepper(call)
    k, max_len = c.n_assist, c.max_len
    P = input_ids.shape[1]
    logits = st.prefill(input_ids, max_len - P + k)
    st.capture(k + 1)
    seq = st.ids_buffer(max_len + k)
    graphs = st.graph is not None  # (the stepper's own decision: use_graph, a device, more than two new tokens)
    drafter = _ModelDrafter(c, seq, k, chain=graphs and c.chain_graph, graph=graphs)
    drafter.prefill(input_ids, st.tables)
    st.ban(logits, P)
    first = _select(logits, st.V, c.sel, 0).tolist()
    n = _draft_loop(seq, P, max_len, c.stop, c.streamer, c.stats, first, drafter, _StepTarget(st, seq, k))
    return st.finish(n)


def _compact(ids, lens, new, pad):
    B, P = ids.shape
    out = torch.full((B, P + new.shape[1]), pad, dtype=ids.dtype, device=ids.device)
    for b in range(B):
        lb = int(lens[b])
        out[b, :lb] = ids[b, :lb]
        out[b, lb:lb + new.shape[1]] = new[b]
    return out


def _gather_beams(t, idx):
    """t [B, n, ...] gathered along dim 1 by idx [B, k] (HF `_gather_beams`)."""
    while idx.dim() < t.dim():
        idx = idx.unsqueeze(-1)
    return torch.gather(t, 1, idx.expand(-1, -1, *t.shape[2:]))


def _beam_search(call, input_ids):
    """Beam search as transformers' `_beam_search` runs it (do_sample=False, num_return_sequences=1).  The prompt is
    prefilled ONCE per prompt and its KV cache expanded to num_beams rows (the reference reaches the same state through
    `inputs_embeds.repeat_interleave(5)`, base_mmgpt.py:162-163, after computing one row); every step the cache rows are
    re-ordered by the surviving beams' parents (HF `_reorder_cache`) with one gather kernel per layer.
    share_prompt_kv: the prefilled cache stays the one copy of the prompt's K/V (engine.share_cache) and the re-ordering is a table step."""
    c, st = call, _Stepper(call)
    eng, V = st.eng, st.V
    nb, max_len, eos_ids, pad, stop, length_penalty, early_stopping = c.num_beams, c.max_len, c.eos_ids, c.pad, c.stop, c.length_penalty, c.early_stopping
    B, P = input_ids.shape
    max_new = max_len - P
    # No spare rows behind the prompt where the beams append to rows of their own: the shared prompt cache's prefix holds the prompt and
    # nothing else, and a session's cache is the prompt cache - read by both paths, written by neither, it keeps the prompt
    logits0 = st.prefill(input_ids, 0 if c.share_prompt_kv or c.session is not None else max_new)
    cache0 = st.cache
    dev = logits0.device
    ids = input_ids.to(dev)
    expand = torch.arange(B, device=dev).repeat_interleave(nb)
    if c.share_prompt_kv:
        st.cache = eng.share_cache(cache0, nb, max_new)  # cache0 lives on inside it: it is the prefix
    elif c.session is not None:
        st.cache = eng.expand_prefix(cache0, nb, P, P + max_new)  # (P + max_new rows per beam, not the session's capacity)
    else:
        st.cache = eng.expand_cache(cache0, expand)
    del cache0
    logits = torch.empty(B * nb, logits0.shape[1], dtype=torch.float32, device=dev)
    O.gather_rows2d(logits0, expand, logits)

    n_eos = len(eos_ids)
    keep = max(2, 1 + n_eos) * nb
    top_mask = torch.cat([torch.ones(nb, dtype=torch.bool), torch.zeros(keep - nb, dtype=torch.bool)]).to(dev)
    fill = (pad or eos_ids[0]) if eos_ids else -1  # HF `_beam_search`: `pad_token_id or eos_token_id[0] if ... else -1` (a pad id of 0 is falsy)
    running = torch.full((B, nb, max_len), fill, dtype=torch.int64, device=dev)
    running[:, :, :P] = ids[:, None, :]
    sequences = running.clone()
    running_scores = torch.zeros(B, nb, dtype=torch.float32, device=dev)
    running_scores[:, 1:] = NEG
    beam_scores = torch.full((B, nb), NEG, dtype=torch.float32, device=dev)
    seq_len = torch.zeros(B, nb, dtype=torch.int64, device=dev)      # generated length of every finished hypothesis
    finished = torch.zeros(B, nb, dtype=torch.bool, device=dev)
    unsat = torch.ones(B, 1, dtype=torch.bool, device=dev)          # "early-stop heuristic unsatisfied"
    batch_off = (torch.arange(B, device=dev) * nb)[:, None]
    cur = P
    while True:
        acc = O.log_softmax_rows(logits, V, row_bias=running_scores.reshape(-1).contiguous())  # log_probs + running_beam_scores
        # HF: the processors run on log_softmax(logits) of flat_running_sequences; a ban only writes -inf, so after the add
        st.ban(acc, cur, ids=running.view(B * nb, max_len))
        top_lp, top_i = torch.topk(acc.view(B, nb * V), k=keep)
        parent = top_i // V
        tok = top_i % V
        cand = _gather_beams(running, parent)
        cand[:, :, cur] = tok
        hits = stop(cand[:, :, :cur + 1].reshape(B * keep, cur + 1), None).view(B, keep)
        # beams that continue: the best non-finished candidates
        run_lp = top_lp + hits.to(torch.float32) * NEG
        nxt_i = torch.topk(run_lp, k=nb)[1]
        running = _gather_beams(cand, nxt_i)
        running_scores = _gather_beams(run_lp, nxt_i)
        beam_idx = (_gather_beams(parent, nxt_i) + batch_off).reshape(-1)
        # finished hypotheses: only the top num_beams candidates may finish; keep the best num_beams overall
        just = hits & top_mask[None, :]
        fin_lp = top_lp / float((cur + 1 - P) ** length_penalty)
        full = finished.all(dim=-1, keepdim=True) & (early_stopping is True)
        fin_lp = fin_lp + full.to(torch.float32) * NEG + (~unsat).to(torch.float32) * NEG + (~just).to(torch.float32) * NEG
        m_seq = torch.cat([sequences, cand], dim=1)
        m_sc = torch.cat([beam_scores, fin_lp], dim=1)
        m_len = torch.cat([seq_len, torch.full((B, keep), cur + 1 - P, dtype=torch.int64, device=dev)], dim=1)
        m_fin = torch.cat([finished, just], dim=1)
        best = torch.topk(m_sc, k=nb)[1]
        sequences, beam_scores = _gather_beams(m_seq, best), _gather_beams(m_sc, best)
        seq_len, finished = _gather_beams(m_len, best), _gather_beams(m_fin, best)
        cur += 1
        # early-stop heuristic (early_stopping=False default: best attainable running score at the current length)
        hyp_len = (max_len - P) if (early_stopping == "never" and length_penalty > 0.0) else (cur - P)
        best_running = running_scores[:, :1] / float(hyp_len ** length_penalty)
        worst_fin = torch.where(finished, beam_scores.min(dim=1, keepdim=True)[0], torch.full_like(beam_scores, NEG))
        unsat = unsat & (best_running > worst_fin).any(dim=-1, keepdim=True)
        go_on = bool(unsat.any()) and not (bool(finished.all()) and early_stopping is True) and not bool(hits.all())
        if not go_on:
            break
        st.cache.reorder(beam_idx, cur - 1)  # (cur - 1 valid rows: what the copying cache moves; the shared one rewrites its table)
        logits = st.step(running[:, :, cur - 1].reshape(-1).contiguous())
    out_len = P + int(seq_len[:, 0].max())
    return sequences[:, 0, :out_len].to(input_ids.device)
