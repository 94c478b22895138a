"""The hot path: MMGPTLlamaForCausalLM forward + backward as a hand-scheduled sequence of HIP
kernels (include/merlin_hip.h) over the flat parameter arena.  No autograd graph, no torch math:
torch supplies device memory and the stream.

Forward (reference call chain -> here):
  llama_mmgpt.py:72   prepare_inputs_labels_for_multimodal -> tower() + projector() + splice()
  clip_encoder.py:74-82 / HF CLIPVisionModel            -> tower()   (im2col+GEMM, LN, 23 layers)
  mlp_projector.py:19-23 / conv_projector.py:23-39      -> projector()
  base_mmgpt.py:99-160                                  -> splice()  (index kernel + one gather)
  llama_mmgpt.py:75   LlamaModel (32 x decoder layer)   -> _llama_layer_fwd() | _llama_layer_fwd_fp8()
  llama_flash_attn_monkey_patch.py:20-103               -> fused QKV GEMM + RoPE + flash attention (_attn_fwd)
  llama_mmgpt.py:87-100 lm_head + shifted CE            -> the tail of forward(); _head_bwd_rows / _fp8 / _dense
There is ONE layer schedule per tower and operand precision: _llama_layer_fwd / _vit_layer_fwd (16-bit operands, on a 16-bit or an
fp32 residual stream: _stream_norm / _stream_add pick by the stream's dtype) and _llama_layer_fwd_fp8 / _vit_layer_fwd_fp8 (inference
and training), each with its _bwd.  All of them return (16-bit layer input, stream after the layer, saved activations | None).
Backward mirrors it layer by layer.  Each decoder / encoder layer keeps only its input; the layer
forward is recomputed inside the backward (the reference trains with --gradient_checkpointing True,
pretrain.sh:31), or, with `save_activations=True`, kept resident (288 GB HBM makes that affordable).
Weight gradients are written straight into the gradient arena (fused accumulate in the GEMM
epilogue); `on_grads_ready(name_list)` fires per layer so the data-parallel all-reduce of that bucket
overlaps the rest of the backward (merlin_amd/dp.py).
"""
from __future__ import annotations

import math
import os
import weakref

import torch

from .. import ops as O
from .arena import Arena
from .config import head_dim_of, rope_theta_of
from .kv_cache import BeamKVCache, KVCache

VT = "model.vision_tower.vision_tower.vision_model."


def _ru(x, m):
    return (x + m - 1) // m * m


class _LlamaLayerW:
    __slots__ = ("wqkv", "wo", "wgu", "wd", "ln1", "ln2", "names", "p")


class _VitLayerW:
    __slots__ = ("wqkv", "bqkv", "wo", "bo", "w1", "b1", "w2", "b2", "ln1w", "ln1b", "ln2w", "ln2b", "names", "p")


class HipEngine:
    def __init__(self, model):
        self._model = weakref.ref(model)
        self.arena = None
        self._arena_sig = None
        self.rope = None
        self.save_activations = False
        self.on_grads_ready = None  # callable(list_of_param_names) | None: a bucket's gradients are final (dp.GradSync)
        self.on_backward_begin = None  # callable(fresh: bool) | None
        self.strict_checks = True
        self.parity_fp32 = False  # opt-in checking mode: fp32-store forward (merlin_amd/parity.py)
        self.keep_full_lengths = False  # tests: pass the per-sample lengths to the attention kernels even when every sequence fills the context
        self.force_unpad = False  # tests: send right-padded masks through the general unpad / pad attention path as well
        # fp8 training step beyond the decoder: lm_head on by default (-0.5 % of a cfg-5 step); the CLIP tower's Linears (K = 1024: their
        # quantisation passes cost more than the fp8 MFMA returns, +0.6 %, profiles/r03_fp8_parts_ab.txt) implemented, tested, off by default
        self.fp8_head = True
        self.fp8_tower = False
        # fp8 step: the SwiGLU-backward dgrad takes the row / column maxima of dgu in its store phase (mh_gemm_fp8_swiglu_bwd_amax) so that the quantiser
        # behind it reads the layer's largest gradient tensor once instead of twice; identical bytes (tests/test_fp8_training_gpu.py); env MH_FP8_FUSED_AMAX=0: A/B
        self.fp8_fused_amax = os.environ.get("MH_FP8_FUSED_AMAX", "1") != "0"
        # Both towers' residual streams are fp32 (updated in place by the accumulating fp32 epilogue of the projections that feed them,
        # read by mh_norm_fwd_f32in); GEMM operands, attention and every saved activation stay 16-bit, the backward runs on the 16-bit
        # copies of the layer inputs the stream's reader emits.  Default ON since round 4: the configuration that is benchmarked is the
        # one whose parity is quoted (full-depth 7B fp16 logits 4.6e-3 -> 2.1e-3 of max|logit| against the reference's fp32 output, within
        # 1.1x of the measured 16-bit-operand floor: tests/test_parity_floor_gpu.py) at +1.4 % step time.  False = 16-bit streams (the
        # reference's own bf16 training numerics).  The fp8 paths keep 16-bit streams.
        self.fp32_residual = True
        # Resident-activation footprint (save_activations = True), a slope instead of the cliff to full layer recompute (bench.py picks the lowest
        # level that leaves --min-free-gb of HBM next to RCCL's buffers): 0 = keep everything (251 GB at cfg 3, the fastest); 1 = do not keep the
        # normed GEMM operands h1 / h2 of the decoder and tower layers - the backward re-derives them from the saved 16-bit layer inputs with the
        # forward's norm kernels right before the weight gradients that read them (-19.8 GB for ~7 ms per step); 2 = additionally recompute
        # act = silu(gate) * up from the saved gate|up tensor in the first `mem_act_layers` decoder layers (-0.72 GB and +0.45 ms per layer).
        self.mem_level = 0
        self.mem_act_layers = 16
        # lm_head backward over the SCORED rows only: the reference's loss ignores every position whose shifted label is -100
        # (llama_mmgpt.py:92-100), so those rows of dlogits are exactly zero and contribute nothing to d(hidden) = dlogits W and
        # dW = dlogits^T hidden.  The scored rows (cfg 3: the 603 trajectory positions of each 4096-position sequence) are compacted on the
        # device (mh_mask_unpad_index over the flat batch; their count is read back without a wait) and both products contract over them alone
        # whenever they are at most half of the batch.  Exact arithmetic, fewer zero terms; False = the dense products.
        self.sparse_head = os.environ.get("MH_DENSE_HEAD", "0") != "1"  # (env: A/B switch for benchmarks)
        self.sparse_last_layer = os.environ.get("MH_DENSE_LAST_LAYER", "0") != "1"  # last decoder layer's MLP / o-proj backward over the scored rows
        self._err = None
        self.weight_version = 0  # bumped whenever parameter VALUES change (optimizer step, loads, repack): derived copies
        self._derived = {}       # (fp8 weights, the K-padded patch-embedding weight) are keyed on it
        self._pver = None        # torch version counters of the parameters at the last forward (ensure_arena)

    # ------------------------------------------------------------------------------------------
    # parameter arena
    # ------------------------------------------------------------------------------------------
    @property
    def model(self):
        return self._model()

    def _ordered_params(self):
        m = self.model
        named = dict(m.named_parameters())
        order = []
        cfg = m.config
        for i in range(cfg.num_hidden_layers):
            p = f"model.layers.{i}."
            order += [p + "self_attn.q_proj.weight", p + "self_attn.k_proj.weight", p + "self_attn.v_proj.weight",
                      p + "self_attn.o_proj.weight", p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight",
                      p + "mlp.down_proj.weight", p + "input_layernorm.weight", p + "post_attention_layernorm.weight"]
        order += ["model.norm.weight", "lm_head.weight", "model.embed_tokens.weight"]  # (norm, lm_head) = one DP bucket
        if any(k.startswith(VT) for k in named):
            vt = m.get_model().vision_tower
            for i in range(vt.config.num_hidden_layers):
                p = VT + f"encoder.layers.{i}."
                order += [p + f"self_attn.{n}_proj.weight" for n in ("q", "k", "v")]
                order += [p + f"self_attn.{n}_proj.bias" for n in ("q", "k", "v")]
                order += [p + "self_attn.out_proj.weight", p + "self_attn.out_proj.bias",
                          p + "layer_norm1.weight", p + "layer_norm1.bias", p + "layer_norm2.weight", p + "layer_norm2.bias",
                          p + "mlp.fc1.weight", p + "mlp.fc1.bias", p + "mlp.fc2.weight", p + "mlp.fc2.bias"]
            order += [VT + "embeddings.class_embedding", VT + "embeddings.patch_embedding.weight",
                      VT + "embeddings.position_embedding.weight", VT + "pre_layrnorm.weight", VT + "pre_layrnorm.bias",
                      VT + "post_layernorm.weight", VT + "post_layernorm.bias"]
        rest = [k for k in named if k not in set(order)]
        order += rest
        missing = [k for k in order if k not in named]
        if missing:
            raise RuntimeError(f"parameters expected by the HIP engine are missing: {missing[:4]}...")
        return [(k, named[k]) for k in order]

    def ensure_arena(self):
        m = self.model
        sig = tuple(id(p) for _, p in m.named_parameters())
        if self.arena is None or self._arena_sig != sig:
            cfg = m.config
            vpad = _ru(cfg.vocab_size, 64)
            self.arena = Arena(self._ordered_params(), alloc_numel={"lm_head.weight": vpad * cfg.hidden_size})
            self._arena_sig = sig
            self._bind = None
        if self.arena.ensure_packed() or self._bind is None:
            self._bind_views()
        # Parameters are views of the arena, so ANY in-place update of one (a stock torch.optim step on param.grad under HF
        # Trainer, p.mul_(), clip-by-value, EMA swaps ...) changes the arena behind the derived copies.  torch counts in-place
        # writes per tensor (`_version`): a changed signature drops the copies exactly like FusedAdamW.step / load_state_dict do.
        # (Writes through `p.data` get a fresh version counter from torch and stay invisible: call weights_changed() after those.)
        pv = self._param_versions()
        if pv != self._pver:
            if self._pver is not None:
                self.weights_changed()
            self._pver = pv
        return self.arena

    def _param_versions(self):
        return tuple(p._version for p in self.arena.params.values())

    def _bind_views(self):
        """Fused weight views (q|k|v, gate|up) over the arena."""
        m, A = self.model, self.arena
        cfg = m.config
        d, ff = cfg.hidden_size, cfg.intermediate_size
        self.llama = []
        for i in range(cfg.num_hidden_layers):
            p = f"model.layers.{i}."
            W = _LlamaLayerW()
            W.p = p
            W.wqkv = A.span(p + "self_attn.q_proj.weight", p + "self_attn.v_proj.weight", (3 * d, d))
            W.wo = A.view(p + "self_attn.o_proj.weight", shape=(d, d))
            W.wgu = A.span(p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight", (2 * ff, d))
            W.wd = A.view(p + "mlp.down_proj.weight", shape=(d, ff))
            W.ln1 = A.view(p + "input_layernorm.weight")
            W.ln2 = A.view(p + "post_attention_layernorm.weight")
            W.names = [n for n in A.names if n.startswith(p)]
            self.llama.append(W)
        self.vit = []
        tower = getattr(m.get_model(), "vision_tower", None)
        if tower is not None:
            vc = tower.config
            vd, vff = vc.hidden_size, vc.intermediate_size
            for i in range(vc.num_hidden_layers):
                p = VT + f"encoder.layers.{i}."
                W = _VitLayerW()
                W.p = p
                W.wqkv = A.span(p + "self_attn.q_proj.weight", p + "self_attn.v_proj.weight", (3 * vd, vd))
                W.bqkv = A.span(p + "self_attn.q_proj.bias", p + "self_attn.v_proj.bias", (3 * vd,))
                W.wo, W.bo = A.view(p + "self_attn.out_proj.weight", shape=(vd, vd)), A.view(p + "self_attn.out_proj.bias")
                W.w1, W.b1 = A.view(p + "mlp.fc1.weight", shape=(vff, vd)), A.view(p + "mlp.fc1.bias")
                W.w2, W.b2 = A.view(p + "mlp.fc2.weight", shape=(vd, vff)), A.view(p + "mlp.fc2.bias")
                W.ln1w, W.ln1b = A.view(p + "layer_norm1.weight"), A.view(p + "layer_norm1.bias")
                W.ln2w, W.ln2b = A.view(p + "layer_norm2.weight"), A.view(p + "layer_norm2.bias")
                W.names = [n for n in A.names if n.startswith(p)]
                self.vit.append(W)
        self._bind = True
        self.rope = None
        self.weights_changed()

    def weights_changed(self):
        """Parameter values changed (optimizer step, checkpoint load, init, repack): drop every derived copy."""
        self.weight_version += 1
        self._derived = {}
        self._fp8 = self._fp8_fwd = self._fp4 = None

    def _derive(self, key, make):
        hit = self._derived.get(key)
        if hit is None or hit[0] != self.weight_version:
            hit = self._derived[key] = (self.weight_version, make())
        return hit[1]

    def _trainable(self, name):
        return self.arena.params[name].requires_grad

    # ------------------------------------------------------------------------------------------
    # helpers
    # ------------------------------------------------------------------------------------------
    def _rope_table(self, S, device):
        cfg = self.model.config
        if self.rope is None or self.rope.shape[0] < S or self.rope.device != device:
            # computed on the host exactly like transformers' LlamaRotaryEmbedding (fp32), then uploaded:
            # init-time plumbing; mh_rope_table is the device-side equivalent (tests compare them)
            D = head_dim_of(cfg)
            n = max(S, 64)
            inv = 1.0 / (rope_theta_of(cfg) ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
            fr = torch.outer(torch.arange(n, dtype=torch.float32), inv)
            self.rope = torch.stack((fr.cos(), fr.sin()), dim=-1).contiguous().to(device)
        return self.rope

    def _wgrad(self, dy, x, gout, fresh, Tpad):
        """gout[N_out, K_in] (+)= dy[T, N_out]^T @ x[T, K_in].  The contraction runs over tokens, so both operands
        are K-strided as they lie in memory: the MFMA kernel reads them with transpose-reads, no copies, any T
        (the CLIP tower's 27 696 tokens are not a multiple of the 64-token K-tile), split-K for the small CLIP
        weights.  Odd feature widths (not a multiple of 8) fall back to zero-padded transposed copies."""
        if dy.shape[1] % 8 == 0 and x.shape[1] % 8 == 0:
            O.wgrad_tn(dy, x, gout, accum=not fresh)
            return
        dyT = O.transpose16(dy, r_pad=Tpad)
        xT = O.transpose16(x, r_pad=Tpad)
        O.gemm_nt(dyT, xT, out=gout, accum=not fresh)

    @staticmethod
    def _qkv(t):
        """The q | k | v thirds of a fused [T, 3 d] buffer (or of its gradient) as column views."""
        d = t.shape[1] // 3
        return t[:, :d], t[:, d:2 * d], t[:, 2 * d:]

    @staticmethod
    def _stream_norm(x, w, eps, b=None, want_x16=True):
        """The norm that reads the residual stream x (b = None: RMSNorm, else LayerNorm) -> (h, x16): x16 = the 16-bit copy of x that
        the backward keeps.  An fp32 stream's reader writes it next to h (only when wanted); a 16-bit stream is its own copy."""
        if x.dtype == torch.float32:
            return O.norm_fwd_f32in(x, w, eps, b=b, want_x16=want_x16)
        return (O.rmsnorm_fwd(x, w, eps) if b is None else O.layernorm_fwd(x, w, b, eps)), x

    @staticmethod
    def _stream_add(x, a, w, bias=None):
        """x + a w^T (+ bias) -> the residual stream after the projection: an fp32 stream is updated IN PLACE (fp32 read-modify-write
        in the GEMM epilogue), a 16-bit one is a new tensor."""
        if x.dtype == torch.float32:
            return O.gemm_nt(a, w, bias=bias, out=x, accum=True)
        return O.gemm_nt(a, w, bias=bias, resid=x)

    def _lm_head_w(self):
        """lm_head.weight with its zero pad rows: [Vpad, d], the vocabulary rounded up to whole 64-row tiles."""
        cfg = self.model.config
        Vpad, d = _ru(cfg.vocab_size, 64), cfg.hidden_size
        return self.arena.view("lm_head.weight", numel=Vpad * d, shape=(Vpad, d))

    def _lm_head_g(self):
        """The gradient block of _lm_head_w(): rows [V, Vpad) receive exact zeros (dlogits' pad columns are zero)."""
        cfg = self.model.config
        Vpad, d = _ru(cfg.vocab_size, 64), cfg.hidden_size
        off = self.arena.offset["lm_head.weight"]
        return self.arena.gflat[off: off + Vpad * d].view(Vpad, d)

    def _tower_embed_names(self):
        """The bucket behind the tower's first layer: patch / class / position embeddings + pre_layrnorm."""
        return [n for n in self.arena.names if n.startswith(VT + "embeddings.") or n.startswith(VT + "pre_layrnorm")]

    def _ready(self, names):
        if self.on_grads_ready is not None:
            self.on_grads_ready(names)

    def _untouched(self, names, fresh):
        """A trainable bucket this backward does not reach: zero it on the first micro-step (the arena may hold the previous
        step's values), leave accumulated values alone otherwise, and report it like any other bucket."""
        if fresh:
            for n in names:
                if self.arena.params[n].requires_grad:
                    self.arena.gview(n).zero_()
        self._ready(names)

    # ------------------------------------------------------------------------------------------
    # vision tower
    # ------------------------------------------------------------------------------------------
    def _vit_layer_fwd(self, W, x, N, S, vc, keep, need_x16=True):
        """One CLIP encoder layer on the residual stream x [T, vd] (16-bit: a new tensor per projection; fp32: updated IN PLACE) ->
        (x16 = the 16-bit copy of the layer input for the backward, the stream after the layer, saved activations | None)."""
        H = vc.num_attention_heads
        D = vc.hidden_size // H
        eps = vc.layer_norm_eps
        h1, x16 = self._stream_norm(x, W.ln1w, eps, b=W.ln1b, want_x16=need_x16)  # (the 16-bit copy is the BACKWARD's: not written without one)
        qkv = O.gemm_nt(h1, W.wqkv, bias=W.bqkv)
        o, lse = O.attn_fwd2(*self._qkv(qkv), N, S, H, D, causal=False)
        x = self._stream_add(x, o, W.wo, bias=W.bo)
        h2, x2 = self._stream_norm(x, W.ln2w, eps, b=W.ln2b, want_x16=keep)
        if keep:
            f1, a = self._fc1_gelu(h2, W)  # f1 (kept for the backward) and quick_gelu(f1) from one launch
        else:
            f1 = None
            a = O.gemm_nt(h2, W.w1, bias=W.b1, act="quick_gelu")
        x = self._stream_add(x, a, W.w2, bias=W.b2)
        return x16, x, (((None if self.mem_level else h1), qkv, o, lse, x2, (None if self.mem_level else h2), f1, a) if keep else None)

    @staticmethod
    def _fc1_gelu(h2, W):
        if W.w1.shape[0] % 8 == 0 and h2.shape[1] % 64 == 0:
            return O.gemm_gelu_fwd(h2, W.w1, W.b1)
        f1 = O.gemm_nt(h2, W.w1, bias=W.b1)
        return f1, O.quick_gelu_fwd(f1)

    def _vit_layer_bwd(self, W, x, dy, N, S, vc, saved, fresh):
        A = self.arena
        H = vc.num_attention_heads
        vd = vc.hidden_size
        D = vd // H
        eps = vc.layer_norm_eps
        if saved is None:
            _, _, saved = self._vit_layer_fwd(W, x, N, S, vc, keep=True)
        h1, qkv, o, lse, x2, h2, f1, a = saved
        if h1 is None:  # mem_level >= 1: re-derived from the saved 16-bit layer inputs
            h1 = O.layernorm_fwd(x, W.ln1w, W.ln1b, eps)
            h2 = O.layernorm_fwd(x2, W.ln2w, W.ln2b, eps)
        T = x.shape[0]
        Tpad = _ru(T, 64)
        p = W.p
        acc = not fresh
        # The four weight gradients of the layer are issued as ONE grouped launch (O.wgrad_tn_grouped: 48 + 16 + 64 + 64 output tiles of
        # 256^2 for ViT-L fill the chip together for the whole 27 696-token contraction; one by one each needed split-K with fp32
        # partials).  Its operands must therefore all be alive at one point: the LayerNorm backward that used to accumulate dx2 IN PLACE
        # into dy gets a copy to accumulate into (57 MB at cfg 3), the grouped launch sits before the last in-place accumulation.
        grouped = O.wgrad_group_pays(T, [(dy.shape[1], a.shape[1]), (f1.shape[1], h2.shape[1]), (dy.shape[1], o.shape[1]), (qkv.shape[1], h1.shape[1])])
        if f1.shape[1] % 8 == 0 and dy.shape[1] % 64 == 0:
            df1 = O.gemm_gelu_bwd(dy, W.w2, f1)  # quick-GELU backward in the fc2 dgrad's store phase (dy W2 never stored)
        else:
            df1 = O.quick_gelu_bwd(f1, O.gemm_nt(dy, W.w2, b_t=True))
        if not grouped:
            self._wgrad(dy, a, A.gview(p + "mlp.fc2.weight"), fresh, Tpad)
        O.colsum(dy, A.gview(p + "mlp.fc2.bias"), accumulate=acc)
        dh2 = O.gemm_nt(df1, W.w1, b_t=True)
        if not grouped:
            self._wgrad(df1, h2, A.gview(p + "mlp.fc1.weight"), fresh, Tpad)
        O.colsum(df1, A.gview(p + "mlp.fc1.bias"), accumulate=acc)
        dx2 = O.layernorm_bwd(x2, W.ln2w, dh2, eps, dx=O.copy2d(dy, torch.empty_like(dy)) if grouped else dy, accumulate_dx=True,
                              dw_out=A.gview(p + "layer_norm2.weight"), db_out=A.gview(p + "layer_norm2.bias"), accumulate=acc)
        do = O.gemm_nt(dx2, W.wo, b_t=True)
        if not grouped:
            self._wgrad(dx2, o, A.gview(p + "self_attn.out_proj.weight"), fresh, Tpad)
        O.colsum(dx2, A.gview(p + "self_attn.out_proj.bias"), accumulate=acc)
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = self._qkv(dqkv)
        O.attn_bwd2(*self._qkv(qkv), o, do, lse, N, S, H, D, False, dq=dq, dk=dk, dv=dv)
        dh1 = O.gemm_nt(dqkv, W.wqkv, b_t=True)
        gqkv = A.gspan(p + "self_attn.q_proj.weight", p + "self_attn.v_proj.weight", (3 * vd, vd))
        if grouped:
            O.wgrad_tn_grouped([(dy, a, A.gview(p + "mlp.fc2.weight")), (df1, h2, A.gview(p + "mlp.fc1.weight")),
                                (dx2, o, A.gview(p + "self_attn.out_proj.weight")), (dqkv, h1, gqkv)], accum=acc)
        else:
            self._wgrad(dqkv, h1, gqkv, fresh, Tpad)
        O.colsum(dqkv, A.gspan(p + "self_attn.q_proj.bias", p + "self_attn.v_proj.bias", (3 * vd,)), accumulate=acc)
        dx = O.layernorm_bwd(x, W.ln1w, dh1, eps, dx=dx2, accumulate_dx=True, dw_out=A.gview(p + "layer_norm1.weight"),
                             db_out=A.gview(p + "layer_norm1.bias"), accumulate=acc)
        self._ready(W.names)
        return dx

    # ---- the same encoder layer with its four Linears on the scaled-fp8 MFMA (fp8 training step, BASELINE cfg 5: "all Llama / ViT
    # Linear weights").  Operand formats as in the decoder (fp8_train_weights): activations / gradients row-quantised per token, the
    # transposed wgrad operands per feature (gradients) or tensor-wide (activations), weights per output channel + 128-block exponents.
    # LayerNorm, attention, quick-GELU, bias gradients and the residual stream stay 16-bit.
    def fp8_tower_weights(self, li):
        def make():
            out = []
            for W in self.vit:
                out.append(dict(wqkv=O.quant_fp8_rows_e4(W.wqkv), wo=O.quant_fp8_rows_e4(W.wo), w1=O.quant_fp8_rows_e4(W.w1), w2=O.quant_fp8_rows_e4(W.w2),
                                wqkvT=O.quant_fp8_rows_t_e4(W.wqkv), woT=O.quant_fp8_rows_t_e4(W.wo), w1T=O.quant_fp8_rows_t_e4(W.w1),
                                w2T=O.quant_fp8_rows_t_e4(W.w2)))
            return self._drop_zero_exponents(out)
        return self._derive("fp8_tower_weights", make)[li]

    def _vit_layer_fwd_fp8(self, W, li, x, N, S, vc, keep):
        H = vc.num_attention_heads
        D = vc.hidden_size // H
        eps = vc.layer_norm_eps
        Q = self.fp8_tower_weights(li)
        dt = x.dtype
        h1 = O.layernorm_fwd(x, W.ln1w, W.ln1b, eps)
        a1 = O.quant_fp8_rows(h1)
        qkv = O.gemm_fp8(a1, Q["wqkv"], out_dtype=dt, bias=W.bqkv)
        o, lse = O.attn_fwd2(*self._qkv(qkv), N, S, H, D, causal=False)
        a2 = O.quant_fp8_rows(o)
        x2 = O.gemm_fp8(a2, Q["wo"], out_dtype=dt, bias=W.bo, resid=x)
        h2 = O.layernorm_fwd(x2, W.ln2w, W.ln2b, eps)
        a3 = O.quant_fp8_rows(h2)
        if keep:
            f1 = O.gemm_fp8(a3, Q["w1"], out_dtype=dt, bias=W.b1)
            a = O.quick_gelu_fwd(f1)
        else:
            f1 = None
            a = O.gemm_fp8(a3, Q["w1"], out_dtype=dt, bias=W.b1, act="quick_gelu")
        a4 = O.quant_fp8_rows(a)
        y = O.gemm_fp8(a4, Q["w2"], out_dtype=dt, bias=W.b2, resid=x2)
        return x, y, ((h1, qkv, o, lse, x2, h2, f1, a, (a1[1], a2[1], a3[1], a4[1])) if keep else None)

    def _vit_layer_bwd_fp8(self, W, li, x, dy, N, S, vc, saved, fresh):
        A = self.arena
        H = vc.num_attention_heads
        vd = vc.hidden_size
        D = vd // H
        eps = vc.layer_norm_eps
        if saved is None:
            _, _, saved = self._vit_layer_fwd_fp8(W, li, x, N, S, vc, keep=True)
        h1, qkv, o, lse, x2, h2, f1, a, (s_h1, s_o, s_h2, s_a) = saved
        Q = self.fp8_tower_weights(li)
        dt = x.dtype
        p = W.p
        acc = not fresh
        # fc2
        dy8, dyT8 = O.quant_fp8_both(dy)
        da = O.gemm_fp8(dy8, Q["w2T"], out_dtype=dt)
        self._wgrad_fp8(dyT8, a, s_a, A.gview(p + "mlp.fc2.weight"), fresh)
        O.colsum(dy, A.gview(p + "mlp.fc2.bias"), accumulate=acc)
        del dy8, dyT8
        df1 = O.quick_gelu_bwd(f1, da)
        df18, df1T8 = O.quant_fp8_both(df1)
        dh2 = O.gemm_fp8(df18, Q["w1T"], out_dtype=dt)
        self._wgrad_fp8(df1T8, h2, s_h2, A.gview(p + "mlp.fc1.weight"), fresh)
        O.colsum(df1, A.gview(p + "mlp.fc1.bias"), accumulate=acc)
        del df18, df1T8
        dx2 = O.layernorm_bwd(x2, W.ln2w, dh2, eps, dx=dy, accumulate_dx=True, dw_out=A.gview(p + "layer_norm2.weight"),
                              db_out=A.gview(p + "layer_norm2.bias"), accumulate=acc)
        dx28, dx2T8 = O.quant_fp8_both(dx2)
        do = O.gemm_fp8(dx28, Q["woT"], out_dtype=dt)
        self._wgrad_fp8(dx2T8, o, s_o, A.gview(p + "self_attn.out_proj.weight"), fresh)
        O.colsum(dx2, A.gview(p + "self_attn.out_proj.bias"), accumulate=acc)
        del dx28, dx2T8
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = self._qkv(dqkv)
        O.attn_bwd2(*self._qkv(qkv), o, do, lse, N, S, H, D, False, dq=dq, dk=dk, dv=dv)
        dqkv8, dqkvT8 = O.quant_fp8_both(dqkv)
        dh1 = O.gemm_fp8(dqkv8, Q["wqkvT"], out_dtype=dt)
        self._wgrad_fp8(dqkvT8, h1, s_h1, A.gspan(p + "self_attn.q_proj.weight", p + "self_attn.v_proj.weight", (3 * vd, vd)), fresh)
        O.colsum(dqkv, A.gspan(p + "self_attn.q_proj.bias", p + "self_attn.v_proj.bias", (3 * vd,)), accumulate=acc)
        dx = O.layernorm_bwd(x, W.ln1w, dh1, eps, dx=dx2, accumulate_dx=True, dw_out=A.gview(p + "layer_norm1.weight"),
                             db_out=A.gview(p + "layer_norm1.bias"), accumulate=acc)
        self._ready(W.names)
        return dx

    def tower(self, images, ctx=None):
        """list of [n_i,3,H,W] -> x [Nimg*(G2+1), vd] = hidden_states[select_layer] (CLS rows kept in place)."""
        m = self.model
        tower = m.get_model().vision_tower
        vc = tower.config
        A = self.arena
        dt = A.flat.dtype
        dev = A.flat.device
        G = vc.image_size // vc.patch_size
        G2 = G * G
        S = G2 + 1
        vd = vc.hidden_size
        K = 3 * vc.patch_size * vc.patch_size
        Kpad = _ru(K, 64)
        N = sum(int(im.shape[0]) for im in images)
        # patch rows are gathered straight into the tower's token-major layout [N, 1 + G2, Kpad] (zero CLS slot per image), one
        # launch per image tensor of the batch: no torch.cat of the pixels, and the weight gradient is one GEMM over all rows
        cols = torch.empty(N * S, Kpad, dtype=dt, device=dev)
        r = 0
        for im in images:
            im = im.to(device=dev)
            if im.dtype not in (torch.float32, dt):
                im = im.float()
            n = int(im.shape[0])
            O.im2col_patches(im.contiguous(), vc.patch_size, Kpad, dt, rows_per_img=S, row0=1, out=cols[r * S:(r + n) * S])
            r += n

        def _pad_patch_weight():  # K = 588 -> 640 (zero tail), once per weight version
            wp = torch.zeros(vd, Kpad, dtype=dt, device=dev)
            return O.copy2d(A.view(VT + "embeddings.patch_embedding.weight", shape=(vd, K)), wp)

        wpad = self._derive("patch_wpad", _pad_patch_weight)
        L = tower.layers_used
        train_tower = ctx is not None and ctx["train_tower"]
        xs, saves = [], []
        r32 = self.fp32_residual and not (ctx is not None and ctx.get("fp8"))
        cls_w, pos_w = A.view(VT + "embeddings.class_embedding"), A.view(VT + "embeddings.position_embedding.weight", shape=(S, vd))
        if r32:
            # the fp32 stream STARTS from fp32 values (round 4): patch projection stored in fp32, class / position embeddings added in fp32,
            # pre_layrnorm fp32 -> fp32; x0 = the 16-bit copy of its input the backward keeps.  (16-bit tensors at the start of the
            # stream were a sixth of the full-depth logits error: profiles/r04_parity_floor.txt)
            x0_32 = O.vit_assemble_f32(O.gemm_nt(cols, wpad, out_f32=True), cls_w, pos_w, N, G2)
            x, x0 = O.layernorm_f32_to_f32(x0_32, A.view(VT + "pre_layrnorm.weight"), A.view(VT + "pre_layrnorm.bias"), vc.layer_norm_eps,
                                           want_x16=train_tower)
            del x0_32
        else:
            x0 = O.vit_assemble(O.gemm_nt(cols, wpad), cls_w, pos_w, N, G2)
            x = O.layernorm_fwd(x0, A.view(VT + "pre_layrnorm.weight"), A.view(VT + "pre_layrnorm.bias"), vc.layer_norm_eps)
        fp8_tower = bool(ctx is not None and ctx.get("fp8_train") and self.fp8_tower and not r32 and vd % 128 == 0 and
                         vc.intermediate_size % 128 == 0)
        keep = train_tower and self.save_activations
        for i in range(L):
            if fp8_tower:
                x16, x, sv = self._vit_layer_fwd_fp8(self.vit[i], i, x, N, S, vc, keep)
            else:
                x16, x, sv = self._vit_layer_fwd(self.vit[i], x, N, S, vc, keep, need_x16=train_tower)
            if train_tower:
                xs.append(x16)
            saves.append(sv)
            x16 = None  # (a 16-bit stream's x16 IS the layer input: without a backward it is not held past its layer)
        if r32:
            x = O.convert(x, torch.empty(x.shape, dtype=dt, device=dev))  # hidden_states[select_layer] as the projector's 16-bit GEMM operand
        if ctx is not None:
            ctx.update(vit_cols=cols if train_tower else None, vit_x0=x0 if train_tower else None, vit_xs=xs, vit_saves=saves,
                       vit_N=N, vit_S=S, vit_Kpad=Kpad, fp8_tower=fp8_tower)
        return x, N, S

    def tower_bwd(self, ctx, dx, fresh):
        m = self.model
        tower = m.get_model().vision_tower
        vc = tower.config
        A = self.arena
        N, S = ctx["vit_N"], ctx["vit_S"]
        L = tower.layers_used
        for i in reversed(range(L)):
            if ctx.get("fp8_tower"):
                dx = self._vit_layer_bwd_fp8(self.vit[i], i, ctx["vit_xs"][i], dx, N, S, vc, ctx["vit_saves"][i], fresh)
            else:
                dx = self._vit_layer_bwd(self.vit[i], ctx["vit_xs"][i], dx, N, S, vc, ctx["vit_saves"][i], fresh)
            ctx["vit_xs"][i] = None
            ctx["vit_saves"][i] = None
        acc = not fresh
        vd = vc.hidden_size
        G2 = S - 1
        dx0 = O.layernorm_bwd(ctx["vit_x0"], A.view(VT + "pre_layrnorm.weight"), dx, vc.layer_norm_eps,
                              dw_out=A.gview(VT + "pre_layrnorm.weight"), db_out=A.gview(VT + "pre_layrnorm.bias"), accumulate=acc)
        d3 = dx0.view(N, S, vd)
        # position embedding / class embedding grads: sums over images (column sums of [N, S*vd] and of the CLS rows)
        O.colsum(dx0.view(N, S * vd), A.gview(VT + "embeddings.position_embedding.weight").view(S * vd), accumulate=acc)
        O.colsum(d3[:, 0, :], A.gview(VT + "embeddings.class_embedding"), accumulate=acc)
        # patch embedding weight grad: dW[vd, Kpad] = dx0^T @ cols over ALL token rows (the CLS rows of cols are zero): one
        # K-strided MFMA GEMM on the operands as they lie in memory, then the K-padding is dropped by a strided copy
        K = 3 * vc.patch_size * vc.patch_size
        Kpad = ctx["vit_Kpad"]
        gw = torch.empty(vd, Kpad, dtype=dx0.dtype, device=dx0.device)
        O.wgrad_tn(dx0, ctx["vit_cols"], gw, accum=False)
        O.copy2d(gw[:, :K], A.gview(VT + "embeddings.patch_embedding.weight").view(vd, K), accumulate=acc)
        self._ready(self._tower_embed_names())

    # ------------------------------------------------------------------------------------------
    # projector
    # ------------------------------------------------------------------------------------------
    def projector(self, x, N, S, ctx=None, out_f32=False):
        """x [N*S, vd] (tower output incl. CLS rows) -> (feats2d, rows_per_img, row0, P).  out_f32: the features stay fp32 (they are spliced
        straight into the decoder's fp32 residual stream)."""
        m = self.model
        proj = m.get_model().projector
        A = self.arena
        kind = "conv" if hasattr(proj, "conv_stride") else "mlp"
        tower = m.get_model().vision_tower
        cls_keep = tower.select_feature == "cls_patch"
        if kind == "mlp":
            feats = O.gemm_nt(x, A.view("model.projector.projector.weight"), bias=A.view("model.projector.projector.bias"), out_f32=out_f32)
            if ctx is not None:
                ctx.update(proj_in=x)
            return feats, S, (0 if cls_keep else 1), (S if cls_keep else S - 1)
        # ConvProjector (conv_projector.py:23-39): Conv2d(vd -> d, k3, stride, pad 1) over the G x G patch grid as an
        # implicit GEMM: gather -> MFMA GEMM with weight.view(d, vd*9) in place (+bias) -> [N*(G/s)^2, d]
        if cls_keep:
            raise NotImplementedError("ConvProjector needs the square patch grid (vision_select_feature='patch')")
        vd = x.shape[1]
        G = int(round(math.sqrt(S - 1)))
        stride = proj.conv_stride
        cols = O.conv3x3_cols(x, N, G, vd, stride, S, 1)
        w = A.view("model.projector.projector.weight", shape=(A.params["model.projector.projector.weight"].shape[0], vd * 9))
        feats = O.gemm_nt(cols, w, bias=A.view("model.projector.projector.bias"), out_f32=out_f32)
        Go = (G + 2 - 3) // stride + 1
        if ctx is not None:
            ctx.update(proj_in=cols, proj_conv=(N, G, vd, stride, S))
        return feats, Go * Go, 0, Go * Go

    def projector_bwd(self, ctx, dfeats, fresh):
        """returns dx for the tower output ([N*S, vd])."""
        A = self.arena
        x = ctx["proj_in"]
        wname, bname = "model.projector.projector.weight", "model.projector.projector.bias"
        conv = ctx.get("proj_conv")  # (N, G, vd, stride, S): the weight is the implicit GEMM's [d, vd*9], x its gathered columns
        wshape = (A.params[wname].shape[0], conv[2] * 9) if conv is not None else None
        dx = None
        if ctx["train_tower"]:
            dx = O.gemm_nt(dfeats, A.view(wname, shape=wshape), b_t=True)
            if conv is not None:  # dx was d(columns) [rows, vd*9]
                dx = O.conv3x3_col2im(dx, *conv, 1)
        if self._trainable(wname):
            self._wgrad(dfeats, x, A.gview(wname, shape=wshape), fresh, _ru(x.shape[0], 64))
            O.colsum(dfeats, A.gview(bname), accumulate=not fresh)
            self._ready([wname, bname])
        return dx

    # ------------------------------------------------------------------------------------------
    # Llama
    # ------------------------------------------------------------------------------------------
    def _llama_layer_fwd(self, W, x, B, S, lens, keep, kv_out=None, unpad=None, need_x16=True):
        """One decoder layer on the residual stream x [T, d] (16-bit: a new tensor per projection; fp32: updated IN PLACE) ->
        (x16 = the 16-bit copy of the layer input for the backward, the stream after the layer, saved activations | None)."""
        cfg = self.model.config
        H, D = cfg.num_attention_heads, head_dim_of(cfg)
        eps = cfg.rms_norm_eps
        h1, x16 = self._stream_norm(x, W.ln1, eps, want_x16=need_x16)  # (the 16-bit copy is the BACKWARD's: not written without one)
        qkv = O.gemm_nt_rope(h1, W.wqkv, self.rope, S, H, D)  # q|k|v projection with RoPE in the GEMM epilogue
        o, lse, packed = self._attn_fwd(qkv, B, S, H, D, lens, unpad, kv_out)
        x = self._stream_add(x, o, W.wo)                      # x += o Wo^T
        h2, x2 = self._stream_norm(x, W.ln2, eps, want_x16=keep)
        gu, act = O.gemm_swiglu_fwd(h2, W.wgu)  # gate|up projection; SwiGLU in the same launch's epilogue
        x = self._stream_add(x, act, W.wd)                    # x += act Wd^T
        return x16, x, (self._slim(W, (h1, qkv, o, lse, x2, h2, gu, act, packed)) if keep else None)

    def _slim(self, W, saved):
        """mem_level: drop what the backward can re-derive (see __init__)."""
        if not self.mem_level:
            return saved
        h1, qkv, o, lse, x2, h2, gu, act, packed = saved
        drop_act = self.mem_level >= 2 and int(W.p.split(".")[2]) < self.mem_act_layers
        return (None, qkv, o, lse, x2, None, gu, None if drop_act else act, packed)

    # ---- attention under a key-padding mask (llama_flash_attn_monkey_patch.py:87-102) ---------------------------------------------
    # Right-padded batches (the collator's, collator.py:29-34) only need per-sample lengths: the kernels skip keys >= lens[b] and
    # zero the padded query rows.  Any other mask takes the reference's own route: unpad_input (gather the valid rows of the ROTATED
    # q|k|v - positions stay absolute, RoPE ran in the projection's epilogue) -> causal varlen attention over the packed tokens ->
    # pad_input (scatter back, zeros elsewhere), with the same two gathers around the backward.
    def _attn_fwd(self, qkv, B, S, H, D, lens, unpad, kv_out=None):
        if unpad is None:
            q, k, v = self._qkv(qkv)
            if kv_out is not None:  # prefill: rotated keys and values go to rows [:, :S] of the decode cache, kv_out = (cache, layer)
                kv_out[0].append_rows(kv_out[1], k, v, S, 0, H, D)
            o, lse = O.attn_fwd2(q, k, v, B, S, H, D, causal=True, seqlens=lens)
            return o, lse, None
        fwd, inv, cnt = unpad
        qkv_c = O.gather_rows2d(qkv, fwd, torch.empty_like(qkv))
        q, k, v = self._qkv(qkv_c)
        if kv_out is not None:  # the cache keeps only the VALID keys (rows 0..count-1); their rotation already carries the position
            kv_out[0].append_rows(kv_out[1], k, v, S, 0, H, D)
        o_c, lse = O.attn_fwd2(q, k, v, B, S, H, D, causal=True, seqlens=cnt)
        o = O.gather_rows2d(o_c, inv, torch.empty_like(o_c))
        return o, lse, (qkv_c, o_c)

    def _attn_bwd(self, qkv, o, do, lse, B, S, H, D, lens, unpad, packed):
        """-> dqkv [T, 3 H D] w.r.t. the UN-rotated q, k (inverse RoPE applied)."""
        dqkv = torch.empty_like(qkv)
        if unpad is None:
            dq, dk, dv = self._qkv(dqkv)
            O.attn_bwd2(*self._qkv(qkv), o, do, lse, B, S, H, D, True, seqlens=lens, dq=dq, dk=dk, dv=dv,
                        rope=self.rope)  # inverse RoPE of dq, dk fused into the kernels' epilogues
            return dqkv
        fwd, inv, cnt = unpad
        if packed is None:  # (layer recompute dropped them)
            qkv_c = O.gather_rows2d(qkv, fwd, torch.empty_like(qkv))
            o_c = O.gather_rows2d(o, fwd, torch.empty_like(o))
        else:
            qkv_c, o_c = packed
        do_c = O.gather_rows2d(do, fwd, torch.empty_like(do))
        dqkv_c = torch.empty_like(qkv)
        dq, dk, dv = self._qkv(dqkv_c)
        O.attn_bwd2(*self._qkv(qkv_c), o_c, do_c, lse, B, S, H, D, True, seqlens=cnt, dq=dq, dk=dk, dv=dv)
        O.gather_rows2d(dqkv_c, inv, dqkv)
        return O.rope_qk_(dqkv, self.rope, S, H, D, inverse=True)  # positions are those of the UNPACKED rows

    def quantize_forward_weights(self):
        """fp8 (e4m3, one scale per output channel) copies of the decoder's Linear weights for the fp8 FORWARD (inference /
        prefill form of BASELINE cfg 5's fp8 MFMA weight path).  Re-run after the weights change."""
        self.ensure_arena()
        self._fp8_fwd = self._drop_zero_exponents([dict(wqkv=O.quant_fp8_rows_e4(W.wqkv), wo=O.quant_fp8_rows_e4(W.wo), wgu=O.quant_fp8_rows_e4(W.wgu),
                                                        wd=O.quant_fp8_rows_e4(W.wd)) for W in self.llama])
        return self._fp8_fwd

    # ---- fp8 TRAINING step (BASELINE cfg 5: "fp8 MFMA weight path"; no reference counterpart) -------------
    # Every decoder Linear - forward, dgrad and wgrad - runs on the scaled-fp8 MFMA as an NT product of two ROW-quantised
    # e4m3 operands (include/merlin_hip.h, "fp8 TRAINING step"): activations / gradients are quantised dynamically per row
    # (per token for forward and dgrad, per feature - on the transposed copy - for wgrad), weights per output channel (W8)
    # and per input channel (WT8 = rowquant(W^T)), re-quantised once per weight version.  Residual stream, norms, RoPE,
    # attention, SwiGLU, CE and all gradient accumulators stay 16-bit / fp32 as in the bf16 step; lm_head (fp8_head_weights) and the
    # CLIP tower's Linears (_vit_layer_fwd_fp8) join the decoder's on the fp8 MFMA.
    def fp8_train_weights(self, li):
        def make():
            out = []
            for W in self.llama:
                # weights: per-row fp32 scale + per-128-block exponents (applied by the MFMA's block-scale operand)
                out.append(dict(wqkv=O.quant_fp8_rows_e4(W.wqkv), wo=O.quant_fp8_rows_e4(W.wo), wgu=O.quant_fp8_rows_e4(W.wgu), wd=O.quant_fp8_rows_e4(W.wd),
                                wqkvT=O.quant_fp8_rows_t_e4(W.wqkv), woT=O.quant_fp8_rows_t_e4(W.wo), wguT=O.quant_fp8_rows_t_e4(W.wgu),
                                wdT=O.quant_fp8_rows_t_e4(W.wd)))
            return self._drop_zero_exponents(out)
        return self._derive("fp8_train_weights", make)[li]

    def fp8_head_weights(self):
        """lm_head.weight [V, d] for the fp8 training step: per-output-channel copy (logits) and the copy of its transpose (dgrad)."""
        def make():
            wlm = self._lm_head_w()  # incl. the zero pad rows
            # (the transposed copy is quantised per input channel only: its rows are the whole vocabulary long, beyond what the
            #  block-exponent image of the 8-wave kernel holds)
            return self._drop_zero_exponents([dict(w=O.quant_fp8_rows_e4(wlm), wT=O.quant_fp8_rows_t(wlm))])[0]
        return self._derive("fp8_head_weights", make)

    @staticmethod
    def _drop_zero_exponents(layers):
        """The quantiser leaves a device flag per weight: "some 128-block exponent is non-zero".  Read all of them back ONCE per weight
        version (one host sync per optimizer step) and drop the exponent image of every weight whose blocks all sit within a factor 2
        of their row maximum (i.i.d.-like weights: all of them) - such operands may take the 4-wave fp8 GEMM (csrc/gemm_w4.hip), which
        applies per-row scales only; the others keep the image and the 8-wave kernel's block-scaled loop."""
        trip = [(d, k) for d in layers for k, v in d.items() if len(v) > 2 and v[2] is not None]
        if not trip:
            return layers
        flags = torch.stack([d[k][2][:4].view(torch.int32) for d, k in trip]).view(-1).cpu()
        for (d, k), f in zip(trip, flags.tolist()):
            if f == 0:
                d[k] = d[k][:2]
        return layers

    def _llama_layer_fwd_fp8(self, W, Q, x, B, S, lens, keep, kv_out=None, unpad=None):
        """Decoder layer with every Linear on the scaled-fp8 MFMA: activations are quantised per token row right before each GEMM
        (dynamic scaling), weights per output channel (Q: this layer's dict from quantize_forward_weights() - inference - or
        fp8_train_weights(li) - training); residual stream, norms, RoPE, attention and SwiGLU stay 16-bit.  Returns like
        _llama_layer_fwd: (the layer input, the layer output, saved activations | None)."""
        cfg = self.model.config
        H, D = cfg.num_attention_heads, head_dim_of(cfg)
        eps = cfg.rms_norm_eps
        h1, a1 = O.rmsnorm_fwd_q8(x, W.ln1, eps)  # norm + row quantisation of its output in one launch
        qkv = O.gemm_fp8_rope(a1, Q["wqkv"], self.rope, S, H, D, out_dtype=x.dtype)
        o, lse, packed = self._attn_fwd(qkv, B, S, H, D, lens, unpad, kv_out)
        a2 = O.quant_fp8_rows(o)
        x2 = O.gemm_fp8(a2, Q["wo"], out_dtype=x.dtype, resid=x)
        h2, a3 = O.rmsnorm_fwd_q8(x2, W.ln2, eps)
        gu, act = O.gemm_fp8_swiglu_fwd(a3, Q["wgu"], out_dtype=x.dtype)
        a4 = O.quant_fp8_rows(act)
        y = O.gemm_fp8(a4, Q["wd"], out_dtype=x.dtype, resid=x2)
        # the row scales (one float per token) are kept: their maximum is the tensor-wide scale of the transposed wgrad operand
        return x, y, ((h1, qkv, o, lse, x2, h2, gu, act, (a1[1], a2[1], a3[1], a4[1]), packed) if keep else None)

    # ---- MXFP4 weights for the prompt (forward only): the prefill's counterpart of the decode step's fp4 GEMVs --------------------------
    @staticmethod
    def _stream_add_fp4(x, a, qw):
        """_stream_add on an MXFP4 weight pair: an fp32 stream is updated IN PLACE (fp32 read-modify-write), a 16-bit one is a new tensor."""
        if x.dtype == torch.float32:
            return O.gemm_fp4w(a, qw, out=x, accum=True)
        return O.gemm_fp4w(a, qw, resid=x)

    def _llama_layer_fwd_fp4(self, W, Q, x, B, S, lens, kv_out=None, unpad=None):
        """Forward-only decoder layer on the MXFP4 copies (Q: this layer's dict of quantize_decode_weights_fp4()): _llama_layer_fwd with
        ops.gemm_fp4w for the four projections - q|k|v then ops.rope_qk_, o with the residual form, gate|up then ops.swiglu_fwd, down with
        the residual form - so the K/V rows it writes are those of the model decode_step(fp4=True) runs.  Norms, RoPE, attention, SwiGLU
        and the residual stream (fp32 or 16-bit) are the 16-bit layer's.  -> the stream after the layer."""
        cfg = self.model.config
        H, D = cfg.num_attention_heads, head_dim_of(cfg)
        eps = cfg.rms_norm_eps
        h1, _ = self._stream_norm(x, W.ln1, eps, want_x16=False)
        qkv = O.rope_qk_(O.gemm_fp4w(h1, Q["wqkv"]), self.rope, S, H, D)
        o, _, _ = self._attn_fwd(qkv, B, S, H, D, lens, unpad, kv_out)
        x = self._stream_add_fp4(x, o, Q["wo"])
        h2, _ = self._stream_norm(x, W.ln2, eps, want_x16=False)
        act = O.swiglu_fwd(O.gemm_fp4w(h2, Q["wgu"]))
        return self._stream_add_fp4(x, act, Q["wd"])

    def _wgrad_fp8(self, dyT8, x, sx, gout, fresh):
        """gout[N_out, K_in] (+)= dy^T x on the scaled-fp8 MFMA: both operands as transposed e4m3 copies (contraction over the
        tokens, zero-padded to a multiple of 128).  The GRADIENT operand is scaled per output feature (column maxima: a pass
        over dy - the q / k / v thirds of dqkv differ by orders of magnitude, a tensor-wide scale flushes the small ones to
        zero, measured - shared with the row quantisation of the same tensor for the dgrad: O.quant_fp8_both reads it twice in
        all); the ACTIVATION operand (norm outputs, attention output, SwiGLU output: homogeneous columns) by its
        tensor-wide scale = the largest of the row scales its forward quantisation already produced (single pass)."""
        O.gemm_fp8(dyT8, O.quant_fp8_t_from_rows(x, sx), out=gout, accum=not fresh)

    def _llama_layer_bwd_fp8(self, W, li, x, dy, B, S, lens, saved, fresh, unpad=None):
        cfg = self.model.config
        A = self.arena
        d, ff, H, D = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, head_dim_of(cfg)
        eps = cfg.rms_norm_eps
        Q = self.fp8_train_weights(li)
        if saved is None:
            _, _, saved = self._llama_layer_fwd_fp8(W, Q, x, B, S, lens, keep=True, unpad=unpad)
        h1, qkv, o, lse, x2, h2, gu, act, (s_h1, s_o, s_h2, s_act), packed = saved
        p = W.p
        acc = not fresh
        train = self._trainable(p + "mlp.down_proj.weight")
        dt = x.dtype
        dy8, dyT8 = O.quant_fp8_both(dy) if train else (O.quant_fp8_rows(dy), None)
        # SwiGLU backward in the dgrad's store phase - which also takes the row / column maxima its quantiser needs (one read of dgu less)
        dgu, dgu_amax = O.gemm_fp8_swiglu_bwd(dy8, Q["wdT"], gu, want_amax=True) if train and self.fp8_fused_amax else (O.gemm_fp8_swiglu_bwd(dy8, Q["wdT"], gu), None)
        if train:
            self._wgrad_fp8(dyT8, act, s_act, A.gview(p + "mlp.down_proj.weight"), fresh)
        del act, gu, dy8, dyT8
        dgu8, dguT8 = O.quant_fp8_both(dgu, amax=dgu_amax) if train else (O.quant_fp8_rows(dgu), None)
        dh2 = O.gemm_fp8(dgu8, Q["wguT"], out_dtype=dt)
        if train:
            self._wgrad_fp8(dguT8, h2, s_h2, A.gspan(p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight", (2 * ff, d)), fresh)
        del dgu, dgu8, dguT8
        dx2 = O.rmsnorm_bwd(x2, W.ln2, dh2, eps, dx=dy, accumulate_dx=True,
                            dw_out=A.gview(p + "post_attention_layernorm.weight") if train else None, dw_accumulate=acc)
        dx28, dx2T8 = O.quant_fp8_both(dx2) if train else (O.quant_fp8_rows(dx2), None)
        do = O.gemm_fp8(dx28, Q["woT"], out_dtype=dt)
        if train:
            self._wgrad_fp8(dx2T8, o, s_o, A.gview(p + "self_attn.o_proj.weight"), fresh)
        del dx28, dx2T8
        dqkv = self._attn_bwd(qkv, o, do, lse, B, S, H, D, lens, unpad, packed)
        dqkv8, dqkvT8 = O.quant_fp8_both(dqkv) if train else (O.quant_fp8_rows(dqkv), None)
        dh1 = O.gemm_fp8(dqkv8, Q["wqkvT"], out_dtype=dt)
        if train:
            self._wgrad_fp8(dqkvT8, h1, s_h1, A.gspan(p + "self_attn.q_proj.weight", p + "self_attn.v_proj.weight", (3 * d, d)), fresh)
        dx = O.rmsnorm_bwd(x, W.ln1, dh1, eps, dx=dx2, accumulate_dx=True,
                           dw_out=A.gview(p + "input_layernorm.weight") if train else None, dw_accumulate=acc)
        if train:
            self._ready(W.names)
        return dx

    def _llama_layer_bwd(self, W, x, dy, B, S, lens, saved, fresh, unpad=None, rows=None):
        cfg = self.model.config
        A = self.arena
        d, ff, H, D = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, head_dim_of(cfg)
        eps = cfg.rms_norm_eps
        if saved is None:
            _, _, saved = self._llama_layer_fwd(W, x, B, S, lens, keep=True, unpad=unpad)
        h1, qkv, o, lse, x2, h2, gu, act, packed = saved
        T = x.shape[0]
        Tpad = _ru(T, 64)
        p = W.p
        acc = not fresh
        train = self._trainable(p + "mlp.down_proj.weight")
        # ---- MLP half, post-attention norm and o projection: ONE schedule, over all T rows (g = identity) or, with `rows`, over the scored ones.
        # LAST decoder layer under a sparse loss (engine.sparse_head): dy - the gradient of this layer's output - is exactly zero on every
        # row the loss does not score (the head's dgrad gathered zero rows there and RMSNorm backward is row-wise), so the MLP half, the
        # post-attention norm and the o projection of this layer contract / map over the scored rows alone: the rows are gathered into
        # compact [npad, .] operands (rows_f: flat positions, -1 = zero pad row), run through the same kernels, and the two results the
        # rest of the backward needs dense - d(attention output) and the residual gradient - are gathered back (rows_i; zero rows elsewhere).
        # Each operand of a weight gradient is gathered right before the launch that reads it.
        if rows is None:
            g, Rpad = (lambda t: t), Tpad
        else:
            rows_f, rows_i = rows
            Rpad = rows_f.numel()
            g = lambda t: O.gather_rows2d(t, rows_f, torch.empty(Rpad, t.shape[1], dtype=t.dtype, device=t.device))  # noqa: E731
        dy_c, gu_c, x2_c = g(dy), g(gu), g(x2)
        dgu = O.gemm_swiglu_bwd(dy_c, W.wd, gu_c)  # dact = dy Wd never leaves the kernel: SwiGLU backward in the epilogue
        if train:
            act_c = g(act) if act is not None else O.swiglu_fwd(gu_c)  # (mem_level 2: not kept)
            self._wgrad(dy_c, act_c, A.gview(p + "mlp.down_proj.weight"), fresh, Rpad)
            del act_c
        del gu_c
        dh2 = O.gemm_nt(dgu, W.wgu, b_t=True)
        if train:
            # mem_level >= 1: the normed operand is re-derived from the saved 16-bit layer-half input
            h2_c = g(h2) if h2 is not None else O.rmsnorm_fwd(x2_c, W.ln2, eps)
            self._wgrad(dgu, h2_c, A.gspan(p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight", (2 * ff, d)), fresh, Rpad)
            del h2_c
        del dgu
        dx2 = O.rmsnorm_bwd(x2_c, W.ln2, dh2, eps, dx=dy_c, accumulate_dx=True,
                            dw_out=A.gview(p + "post_attention_layernorm.weight") if train else None, dw_accumulate=acc)
        do = O.gemm_nt(dx2, W.wo, b_t=True)
        if train:
            self._wgrad(dx2, g(o), A.gview(p + "self_attn.o_proj.weight"), fresh, Rpad)
        if rows is not None:  # back to all T rows
            do = O.gather_rows2d(do, rows_i, torch.empty(T, d, dtype=do.dtype, device=do.device))
            dx2 = O.gather_rows2d(dx2, rows_i, dy)  # (dy's storage: its values live on in the compact dx2 = dy_c)
            del dy_c, x2_c, dh2
        # ---- attention and the q|k|v projection: always dense
        dqkv = self._attn_bwd(qkv, o, do, lse, B, S, H, D, lens, unpad, packed)
        dh1 = O.gemm_nt(dqkv, W.wqkv, b_t=True)
        if train:
            self._wgrad(dqkv, h1 if h1 is not None else O.rmsnorm_fwd(x, W.ln1, eps),  # (mem_level >= 1: re-derived, gone after the launch)
                        A.gspan(p + "self_attn.q_proj.weight", p + "self_attn.v_proj.weight", (3 * d, d)), fresh, Tpad)
        dx = O.rmsnorm_bwd(x, W.ln1, dh1, eps, dx=dx2, accumulate_dx=True,
                           dw_out=A.gview(p + "input_layernorm.weight") if train else None, dw_accumulate=acc)
        if train:
            self._ready(W.names)
        return dx

    # ------------------------------------------------------------------------------------------
    # splice / head
    # ------------------------------------------------------------------------------------------
    def _check_errors(self):
        """Reads the device-side validation flags back (raises like the reference would) and returns True when the attention
        mask is NOT a right-padded prefix (left padding, holes): the caller then takes the unpad / pad attention path."""
        self._mask_all_ones = False
        if self._err is None:
            return False
        err, ev = self._err
        self._err = None
        ev.synchronize()
        e = err.tolist()
        if e[0]:
            raise ValueError(f"The number of image start tokens and image end tokens should be the same (sample {e[2]}, difference {e[3]}).")
        if e[1]:
            raise ValueError(f"The image end token should follow the image start token (sample {e[2]}, <im_start> at {e[3]}).")
        if e[4]:
            raise IndexError(f"index out of range in self: input_ids holds an id outside [0, vocab_size) at flat position {e[5]}")
        if e[6]:
            raise IndexError(f"Target out of bounds: labels holds a value that is neither -100 nor in [0, vocab_size) at flat position {e[7]}")
        self._mask_all_ones = not e[10]
        return bool(e[8])

    def _splice_geometry(self):
        """(rows per image in the projector output, first patch row, P = image tokens per image) from the configs alone, so the
        index / validation kernels can run BEFORE the tower (their flags are read back while the GPU is busy with it)."""
        inner = self.model.get_model()
        tower, proj = inner.vision_tower, inner.projector
        vc = tower.config
        G = vc.image_size // vc.patch_size
        if hasattr(proj, "conv_stride"):
            Go = (G + 2 - 3) // proj.conv_stride + 1
            return Go * Go, 0, Go * Go
        S = G * G + 1
        cls_keep = tower.select_feature == "cls_patch"
        return S, (0 if cls_keep else 1), (S if cls_keep else S - 1)

    def validate_and_index(self, input_ids, labels, mask, lens, images, use_images):
        """One pass of device-side input checks (+ the splice row table when the batch carries images); returns src | None."""
        m = self.model
        dev = self.arena.flat.device
        err_dev = torch.zeros(12, dtype=torch.int32, device=dev)
        src = None
        if use_images:
            rpi, row0, P = self._splice_geometry()
            counts = [int(im.shape[0]) for im in images]
            off = [0]
            for c in counts:
                off.append(off[-1] + c)
            B = input_ids.shape[0]
            off = (off + [off[-1]] * (B + 1))[: B + 1]  # fewer image entries than samples: zip() semantics
            img_off = torch.tensor(off, dtype=torch.int32).to(dev, non_blocking=True)
            src = O.splice_index(input_ids, img_off, P, m.im_patch_token, m.im_start_token, m.im_end_token, err_dev,
                                 rows_per_img=rpi, row0=row0)
        # strict_checks = False drops the id / label range checks, never the mask classification: whether the mask is a right-padded
        # prefix (lens fast path) or not (unpad / pad path) decides what the attention kernels compute, and generate() follows the
        # same decision (prefill -> cache.rpos), so it is always made here, on the device, from the mask itself
        if self.strict_checks or mask is not None:
            if self.strict_checks and (input_ids is not None or labels is not None or mask is not None):
                O.check_inputs(input_ids, labels, mask, lens, err_dev, m.config.vocab_size)
            elif mask is not None:
                O.check_inputs(None, None, mask, lens, err_dev, m.config.vocab_size)
            if getattr(self, "_err_host", None) is None:
                self._err_host = torch.empty(12, dtype=torch.int32, pin_memory=True)  # reused: every forward consumes its own check
            host = self._err_host
            host.copy_(err_dev, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._err = (host, ev)
        return src

    # ------------------------------------------------------------------------------------------
    # public entry points
    # ------------------------------------------------------------------------------------------
    def forward(self, input_ids, attention_mask, labels, images, inputs_embeds=None, want_grad=False, loss_only=False,
                kv_cache=None, last_only=False, fp8=False, fp4=False):
        """Returns (loss fp32 scalar tensor | None, logits fp32 [B,S,V] view | None, ctx).
        fp4=True (forward only): the decoder layers and lm_head run on the MXFP4 copies of quantize_decode_weights_fp4() - the model that
        decode_step(fp4=True) continues; tower, projector, embeddings and norms are unchanged."""
        m = self.model
        cfg = m.config
        A = self.ensure_arena()
        dt, dev = A.flat.dtype, A.flat.device
        inner = m.get_model()
        tower = getattr(inner, "vision_tower", None)
        B, S = (input_ids.shape if input_ids is not None else inputs_embeds.shape[:2])
        T = B * S
        d = cfg.hidden_size
        ctx = {"B": B, "S": S, "want_grad": want_grad, "fp8_train": fp8 == "train", "fp8": bool(fp8)}
        ctx["train_tower"] = bool(want_grad and tower is not None and not tower.freeze_vision_tower and
                                  any(p.requires_grad for p in tower.parameters()))
        self._rope_table(S, dev)
        if input_ids is not None:
            input_ids = input_ids.to(dev).contiguous()
        lens = None
        if attention_mask is not None:
            am = attention_mask.to(dev)
            if am.dtype != torch.bool:
                am = am != 0
            lens = O.mask_lens(am.contiguous())
        ctx["lens"] = lens
        if labels is not None:
            labels = labels.to(dev).contiguous()
        # ---- multimodal splice (base_mmgpt.py:82-165) ----
        feats = None
        use_images = tower is not None and images is not None and input_ids is not None and S != 1
        src = self.validate_and_index(input_ids, labels, am.contiguous() if attention_mask is not None else None, lens, images, use_images)
        r32 = self.fp32_residual and not fp8  # (the fp8 paths run on 16-bit streams)
        if use_images:
            xt, N, Sv = self.tower(images, ctx)
            feats, rpi, row0, P = self.projector(xt, N, Sv, ctx, out_f32=r32 and inputs_embeds is None)
            assert (rpi, row0, P) == self._splice_geometry()
            ctx.update(src=src, n_feat_rows=feats.shape[0])
        general_mask = self._check_errors()  # the flags were produced before the tower was enqueued: no wait for compute
        unpad = None
        if attention_mask is not None and (general_mask or self.force_unpad):
            unpad = O.mask_unpad_index(am.contiguous())
        elif attention_mask is not None and self._mask_all_ones and not self.keep_full_lengths:
            # the collator's mask of a batch without padding (cfg 3 / cfg 5: every sequence fills the context) is all ones: drop the lengths, so the
            # attention kernels take their no-lengths forms (llama_flash_attn_monkey_patch.py:76-85, the `key_padding_mask is None` branch:
            # cu_seqlens = arange) - the flag comes from the same device-side check as the mask classification, read back without a wait
            lens = None
            ctx["lens"] = None
        ctx["unpad"] = unpad
        if inputs_embeds is not None:
            x = inputs_embeds.to(device=dev, dtype=dt).reshape(T, d).contiguous()
            if r32:
                x = O.convert(x, torch.empty(x.shape, dtype=torch.float32, device=dev))
        elif r32:  # the decoder's fp32 stream starts from the projector's fp32 output and the widened embedding rows
            x = O.embed_splice_fwd_f32(input_ids.view(-1), src.view(-1) if src is not None else None,
                                       A.view("model.embed_tokens.weight", shape=(cfg.vocab_size, d)), feats)
        else:
            x = O.embed_splice_fwd(input_ids.view(-1), src.view(-1) if src is not None else None,
                                   A.view("model.embed_tokens.weight", shape=(cfg.vocab_size, d)), feats)
        ctx["ids"] = input_ids
        del feats
        # ---- decoder ----
        xs, saves = [], []
        fp8_train = fp8 == "train"
        keep = want_grad and self.save_activations
        if fp8 and (d % 128 or cfg.intermediate_size % 128):
            raise RuntimeError("the fp8 GEMM path needs hidden and intermediate sizes that are multiples of 128")
        if fp8_train and kv_cache is not None:
            raise RuntimeError("prefill runs the 16-bit or fp8-forward path")
        if fp8 and not fp8_train and want_grad:
            raise RuntimeError("model.fp8_forward is the inference form (forward only); set model.fp8_training = True for the fp8 training step")
        if fp4 and fp8:
            raise RuntimeError("fp4 and fp8 weights are alternatives, not a combination (model.fp4_forward / model.fp8_forward)")
        if fp4 and want_grad:
            raise RuntimeError("model.fp4_forward is the inference form (forward only): the MXFP4 copies have no backward")
        if fp4:
            F4 = getattr(self, "_fp4", None) or self.quantize_decode_weights_fp4()

            def layer(li, x, kv):
                return None, self._llama_layer_fwd_fp4(self.llama[li], F4["layers"][li], x, B, S, lens, kv_out=kv, unpad=unpad), None
        elif fp8:
            if fp8_train:
                Q8 = [self.fp8_train_weights(li) for li in range(len(self.llama))]
            else:
                Q8 = getattr(self, "_fp8_fwd", None) or self.quantize_forward_weights()
            layer = lambda li, x, kv: self._llama_layer_fwd_fp8(self.llama[li], Q8[li], x, B, S, lens, keep, kv_out=kv, unpad=unpad)  # noqa: E731
        else:
            layer = lambda li, x, kv: self._llama_layer_fwd(self.llama[li], x, B, S, lens, keep, kv_out=kv, unpad=unpad, need_x16=want_grad)  # noqa: E731
        for li in range(len(self.llama)):
            x16, x, sv = layer(li, x, (kv_cache, li) if kv_cache is not None else None)
            if want_grad:
                xs.append(x16)
            saves.append(sv)
            x16 = None  # (a 16-bit stream's x16 IS the layer input: without a backward it is not held past its layer)
        hn, x = self._stream_norm(x, A.view("model.norm.weight"), cfg.rms_norm_eps, want_x16=want_grad)
        ctx.update(xs=xs, saves=saves, x_last=x if want_grad else None)
        # ---- lm_head + shifted CE (llama_mmgpt.py:87-100) ----
        V = cfg.vocab_size
        Vpad = _ru(V, 64)
        wlm = self._lm_head_w()
        if last_only:  # prefill of generate(): only each sequence's last valid position feeds the sampler
            last = (lens.to(torch.int64) - 1) if lens is not None else torch.full((B,), S - 1, dtype=torch.int64, device=dev)
            rows = O.gather_rows(hn, torch.arange(B, device=dev) * S + last.clamp_min(0))
            if fp4:  # (the fp4 copy of lm_head has V rows)
                return None, O.gemv_fp4w(rows, F4["lm_head"], out_f32=True, n=V), ctx
            return None, O.gemv(rows, wlm, out_f32=True, n=V), ctx
        # fp8 training step: the head's three GEMMs run on the scaled-fp8 MFMA too (BASELINE cfg 5: every Linear) when the geometry
        # allows it (contractions over d, V and T in whole 128-blocks); the logits stay fp32
        fp8_head = bool(fp8_train and self.fp8_head and not last_only and d % 128 == 0)
        ctx["fp8_head"] = fp8_head
        self.last_fp8 = dict(decoder=bool(fp8_train), tower=bool(ctx.get("fp8_tower")), head=fp8_head)  # which parts of this forward ran on fp8 (tests, bench)
        if fp8_head:
            hn8 = O.quant_fp8_rows(hn)
            logits = O.gemm_fp8(hn8, self.fp8_head_weights()["w"], out=torch.empty(T, Vpad, dtype=torch.float32, device=dev), dt16=dt)
            ctx["hn_scales"] = hn8[1] if want_grad else None
            del hn8
        elif fp4:  # [T, Vpad] fp32; the copy holds the V vocabulary rows, the pad columns read as the zero rows of the 16-bit weight
            logits = torch.zeros(T, Vpad, dtype=torch.float32, device=dev) if Vpad != V else torch.empty(T, V, dtype=torch.float32, device=dev)
            O.gemm_fp4w(hn, F4["lm_head"], out=logits[:, :V])
        else:
            logits = O.gemm_nt(hn, wlm, out_f32=True)  # [T, Vpad] fp32
        loss = None
        if labels is not None:
            row_loss, lse, out = O.ce_fwd(logits, labels, V)
            loss = out[2]
            ctx.update(labels=labels, ce_lse=lse, ce_out=out)
            if want_grad and self.sparse_head and not fp8_head and T % 64 == 0:
                # scored rows: position (b, s) iff s < S - 1 and labels[b, s + 1] != -100; row tables + count now, the count is read in backward
                sup = torch.zeros(B, S, dtype=torch.uint8, device=dev)
                sup[:, :-1] = labels[:, 1:] != -100
                rows_f, rows_i, cnt = O.mask_unpad_index(sup.view(1, T))
                # one pinned word PER forward context (torch's caching host allocator recycles it when the context dies): any number of
                # grad-enabled forwards may be outstanding before their backwards run (losses of many micro-batches summed, one .backward())
                slot = torch.empty(1, dtype=torch.int32, pin_memory=True)
                slot.copy_(cnt, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                ctx["scored_rows"] = (rows_f, rows_i, slot, ev)
        ctx.update(hn=hn if want_grad else None, logits=logits if want_grad else None)
        lg = logits.view(B, S, Vpad)[:, :, :V]
        return loss, lg, ctx

    def _scored_rows(self, ctx):
        """(rows_f [npad], rows_i [T]) when the forward tabled the scored rows and they are at most half of the batch, else None."""
        if ctx.get("scored_rows") is None or ctx.get("fp8_head"):
            return None
        rows_f, rows_i, host, ev = ctx["scored_rows"]
        ev.synchronize()  # (recorded in the forward: long done)
        npad = _ru(max(int(host[0]), 1), 256)
        return (rows_f[:npad], rows_i) if 2 * npad <= ctx["B"] * ctx["S"] else None

    def _head_bwd_rows(self, ctx, rows, gscale, acc):
        """lm_head backward over the scored rows alone (engine.sparse_head) -> dhn [T, d], exact zeros on the un-scored rows."""
        cfg = self.model.config
        T, d, V = ctx["B"] * ctx["S"], cfg.hidden_size, cfg.vocab_size
        dt = self.arena.flat.dtype
        rows_f, rows_i = rows
        npad = rows_f.numel()
        dl_c = O.ce_bwd_rows(ctx["logits"], ctx["labels"], ctx["ce_lse"], ctx["ce_out"], rows_f, V, _ru(V, 64), float(gscale), dt)  # [npad, Vpad], zero rows behind the count
        ctx["logits"] = None
        hn_c = O.gather_rows2d(ctx["hn"], rows_f, torch.empty(npad, d, dtype=dt, device=dl_c.device))
        dhn_c = O.gemm_nt(dl_c, self._lm_head_w(), b_t=True)  # [npad, d]
        if self._trainable("lm_head.weight"):
            O.gemm_nt(dl_c, hn_c, a_t=True, b_t=True, out=self._lm_head_g(), accum=acc)
        return O.gather_rows2d(dhn_c, rows_i, torch.empty(T, d, dtype=dt, device=dl_c.device))

    def _head_bwd_fp8(self, ctx, gscale, fresh):
        """lm_head backward on the scaled-fp8 MFMA (fp8 training step, engine.fp8_head) -> dhn [T, d]."""
        V = self.model.config.vocab_size
        Vpad = _ru(V, 64)
        dt = self.arena.flat.dtype
        dlogits = O.ce_bwd(ctx["logits"], ctx["labels"], ctx["ce_lse"], ctx["ce_out"], V, Vpad, float(gscale), dt)
        ctx["logits"] = None
        train_head = self._trainable("lm_head.weight")
        V128 = _ru(Vpad, 128)  # the dgrad contracts over the (padded) vocabulary in whole 128-blocks: zero columns behind Vpad
        dl8, dlT8 = O.quant_fp8_both(dlogits, c_pad=V128) if train_head else (O.quant_fp8_rows(dlogits, k_pad=V128), None)
        dhn = O.gemm_fp8(dl8, self.fp8_head_weights()["wT"], out_dtype=dt)  # [T, d]
        if train_head:
            self._wgrad_fp8(dlT8, ctx["hn"], ctx["hn_scales"], self._lm_head_g(), fresh)
        return dhn

    def _head_bwd_dense(self, ctx, gscale, acc):
        """lm_head backward over every row: dhn [T, d] = dlogits W, dW (+)= dlogits^T hn."""
        V = self.model.config.vocab_size
        Vpad = _ru(V, 64)
        T = ctx["B"] * ctx["S"]
        dt = self.arena.flat.dtype
        dlogits = O.ce_bwd(ctx["logits"], ctx["labels"], ctx["ce_lse"], ctx["ce_out"], V, Vpad, float(gscale), dt)
        ctx["logits"] = None
        dhn = O.gemm_nt(dlogits, self._lm_head_w(), b_t=True)  # [T, d]; B = W^T [d, Vpad]
        if not self._trainable("lm_head.weight"):
            return dhn
        if T % 64 == 0:
            O.gemm_nt(dlogits, ctx["hn"], a_t=True, b_t=True, out=self._lm_head_g(), accum=acc)
        else:  # T is no whole number of 64-token tiles: zero-padded transposed copies
            Tpad = _ru(T, 64)
            dlT = O.transpose16(dlogits, r_pad=Tpad)  # [Vpad, Tpad]
            hnT = O.transpose16(ctx["hn"], r_pad=Tpad)
            O.gemm_nt(dlT[:V], hnT, out=self.arena.gview("lm_head.weight"), accum=acc)
        return dhn

    def backward(self, ctx, gscale=1.0):
        """d(loss)/d(params) * gscale into the gradient arena (param.grad views)."""
        m = self.model
        cfg = m.config
        A = self.arena
        B, S = ctx["B"], ctx["S"]
        d, V = cfg.hidden_size, cfg.vocab_size
        dt = A.flat.dtype
        fresh = A.ensure_grads()
        if self.on_backward_begin is not None:
            self.on_backward_begin(fresh)
        acc = not fresh
        lens = ctx["lens"]
        # Every trainable bucket is reported through _ready() on EVERY backward, in one fixed order (head, decoder layers
        # L-1..0, embedding, projector, tower layers, tower embeddings), whatever this rank's batch contained: the
        # data-parallel all-reduce sequence is then identical on all ranks (merlin_amd/dp.py).
        # ---- head: d(loss)/d(normed hidden state) [T, d]; each path writes lm_head's gradient itself ----
        sparse = self._scored_rows(ctx)
        if sparse is not None:
            dhn = self._head_bwd_rows(ctx, sparse, gscale, acc)
        elif ctx.get("fp8_head"):
            dhn = self._head_bwd_fp8(ctx, gscale, fresh)
        else:
            dhn = self._head_bwd_dense(ctx, gscale, acc)
        dx = O.rmsnorm_bwd(ctx["x_last"], A.view("model.norm.weight"), dhn, cfg.rms_norm_eps,
                           dw_out=A.gview("model.norm.weight") if self._trainable("model.norm.weight") else None, dw_accumulate=acc)
        self._ready(["lm_head.weight", "model.norm.weight"])
        ctx["hn"] = ctx["x_last"] = None
        # ---- decoder ----
        for i in reversed(range(len(self.llama))):
            if ctx.get("fp8_train"):
                dx = self._llama_layer_bwd_fp8(self.llama[i], i, ctx["xs"][i], dx, B, S, lens, ctx["saves"][i], fresh, unpad=ctx.get("unpad"))
            else:
                dx = self._llama_layer_bwd(self.llama[i], ctx["xs"][i], dx, B, S, lens, ctx["saves"][i], fresh, unpad=ctx.get("unpad"),
                                           rows=sparse if (i == len(self.llama) - 1 and self.sparse_last_layer) else None)
            ctx["xs"][i] = None
            ctx["saves"][i] = None
        # ---- embedding + splice ----
        src = ctx.get("src")
        ids = ctx["ids"]
        inner = m.get_model()
        tower = getattr(inner, "vision_tower", None)
        proj = getattr(inner, "projector", None)
        wname, bname = "model.projector.projector.weight", "model.projector.projector.bias"
        emb_train = self._trainable("model.embed_tokens.weight")
        proj_train = proj is not None and any(p.requires_grad for p in proj.parameters())
        tower_train = tower is not None and not tower.freeze_vision_tower and any(p.requires_grad for p in tower.parameters())
        need_feats = src is not None and (ctx["train_tower"] or proj_train)
        dfeats = torch.zeros(ctx["n_feat_rows"], d, dtype=dt, device=dx.device) if need_feats else None
        dembed32 = torch.zeros(V, d, dtype=torch.float32, device=dx.device) if (emb_train and ids is not None) else None
        if ids is not None and (need_feats or emb_train):
            O.embed_splice_bwd(ids.view(-1), src.view(-1) if src is not None else None, dx, dfeats, dembed32)
        if emb_train:
            g = A.gview("model.embed_tokens.weight")
            if ids is None:  # inputs_embeds path: no token rows were looked up, the embedding gradient of this pass is zero
                if fresh:
                    g.zero_()
            elif acc:
                tmp = torch.empty_like(g)
                O.convert(dembed32, tmp)
                O.add(g, tmp, out=g)
            else:
                O.convert(dembed32, g)
            self._ready(["model.embed_tokens.weight"])
        del dx
        if need_feats:
            dxt = self.projector_bwd(ctx, dfeats, fresh)
            if ctx["train_tower"]:
                self.tower_bwd(ctx, dxt, fresh)
        elif src is None:
            # a batch without image tokens (text-only step, decode-shaped input): image-side gradients of this pass are zero.
            # The reference keeps those parameters in the graph with `0 * projector(dummy_feature)` (base_mmgpt.py:109-113);
            # here their buckets are zero-filled (first micro-step only) and still reported, in the usual order.
            if proj_train:
                self._untouched([wname, bname], fresh)
            if tower_train:
                for i in reversed(range(tower.layers_used)):
                    self._untouched(self.vit[i].names, fresh)
                self._untouched(self._tower_embed_names(), fresh)
        # trainable parameters no backward ever reaches (CLIP layers past select_layer, post_layernorm; a tower whose
        # freeze flag is set while its tensors still require grad): zero, never reported (identically on every rank)
        if fresh and tower is not None:
            L = tower.layers_used
            for n in A.names:
                if not n.startswith(VT) or not A.params[n].requires_grad:
                    continue
                dead = n.startswith(VT + "post_layernorm") or any(n.startswith(VT + f"encoder.layers.{i}.") for i in range(L, tower.config.num_hidden_layers))
                if dead or not tower_train:
                    A.gview(n).zero_()
        self._ready(None)  # end of backward

    # ------------------------------------------------------------------------------------------
    # KV-cache decode (llama_mmgpt.py:114-134, HF LlamaAttention with past_key_values)
    # ------------------------------------------------------------------------------------------
    # the cache types own their storage format and their part of a step (kv_cache.py); kept here under the names they always had
    KVCache, BeamKVCache = KVCache, BeamKVCache

    def share_cache(self, cache, num_beams, max_new):
        """BeamKVCache on the prefilled `cache` of Bp prompts: num_beams beams per prompt, room for max_new generated tokens each.  The
        prompt's K/V are not copied (expand_cache is the copying form)."""
        if not 1 <= num_beams <= 16 or max_new < 1:
            raise ValueError(f"share_cache takes 1 <= num_beams <= 16 (the attention kernel's query tile) and max_new >= 1, got {num_beams}, {max_new}")
        self._rope_table(cache.Smax + max_new, cache.lens.device)  # the prefill may have been given no room to append (its rows stay the prompt's)
        return HipEngine.BeamKVCache(cache, num_beams, max_new)

    def prefill(self, input_ids, attention_mask, images, max_new_tokens, inputs_embeds=None, kv_fp8=False, cache=None, w_fp4=False):
        """Full forward over the prompt that also fills a KV cache; returns (logits fp32 [B, V] at each sequence's last
        valid position, cache).  Right-padded prompts (attention_mask) decode from their own length.
        kv_fp8=True: the cache is stored as e4m3 bytes + power-of-two scales (KVCache fp8=True); the prompt's own attention still runs on
        the unquantised keys and values, so these logits do not change.
        cache: an existing KVCache to fill from row 0 instead of a new one (a session's: generation.Session); it keeps its own format and
        must have B rows and room for the prompt and max_new_tokens.
        w_fp4=True: the decoder and lm_head run on the MXFP4 copies (forward(fp4=True)): keys, values and logits of the model that
        decode_step(fp4=True) continues."""
        self.ensure_arena()
        B, S = (input_ids.shape if input_ids is not None else inputs_embeds.shape[:2])
        A = self.arena
        if cache is None:
            cache = self.new_cache(B, S + max_new_tokens, fp8=kv_fp8)
        elif cache.B != B or S + max_new_tokens > cache.Smax:
            raise ValueError(f"prefill into a cache of {cache.B} x {cache.Smax} rows: the prompt needs {B} x {S + max_new_tokens}")
        else:
            cache.rpos = None
        self._rope_table(max(S + max_new_tokens, cache.Smax), A.flat.device)
        _, logits, ctx = self.forward(input_ids, attention_mask, None, images, inputs_embeds=inputs_embeds, kv_cache=cache,
                                      last_only=True, fp4=w_fp4)
        lens = ctx["lens"]
        if ctx.get("unpad") is not None:
            # general mask (left padding / holes): the cache holds the valid keys only; the next token's rotary position is the
            # padded prompt length, as LlamaModel numbers it when generate() passes no position_ids (llama_mmgpt.py:114-134)
            cache.lens.copy_(ctx["unpad"][2])
            cache.rpos = torch.full((B,), S, dtype=torch.int32, device=A.flat.device)
        else:
            cache.lens.copy_(lens if lens is not None else torch.full((B,), S, dtype=torch.int32, device=A.flat.device))
        return logits, cache

    def extend(self, cache, input_ids, images=None, pos=None, w_fp4=False):
        """n = input_ids.shape[1] new positions of ONE sequence on a plain KVCache that already holds P = cache.lens[0] tokens; returns
        logits fp32 [1, V] at the last new position and advances the cache by n.  The prefill's path on the tail alone: embedding and
        image splice of the tail (tower and projector only for `images`, the images whose spans lie in the tail), per layer the prefill's
        GEMMs with the RoPE epilogue reading the table from row P on (rotary positions P .. P + n - 1), the rotated keys and the values
        appended to cache rows [P, P + n) (fp8 cache: quantised by mh_kv8_fill on views offset by P), then mh_attn_extend over the cache
        AFTER the append - the new keys are read as stored, like decode_step and verify_step read them.  The 16-bit weights, or with
        w_fp4=True the MXFP4 copies of quantize_decode_weights_fp4() (ops.gemm_fp4w per projection, the last row's logits by
        ops.gemv_fp4w): the weight format must be the one that wrote the cached rows.
        pos: P when the caller knows it on the host (a session does); None reads cache.lens back."""
        m = self.model
        cfg = m.config
        if not isinstance(cache, HipEngine.KVCache) or cache.B != 1 or cache.rpos is not None:
            raise ValueError("extend takes a plain KVCache of one sequence whose rotary positions are its rows (B = 1, no left padding or holes)")
        if input_ids.dim() != 2 or input_ids.shape[0] != 1 or input_ids.shape[1] < 1:
            raise ValueError(f"extend takes input_ids [1, n >= 1], got {tuple(input_ids.shape)}")
        n = int(input_ids.shape[1])
        P = int(cache.lens[0]) if pos is None else int(pos)
        if P < 0 or P + n > cache.Smax:
            raise ValueError(f"extend: {P} cached + {n} new tokens exceed the cache's {cache.Smax} rows (grow_cache makes a larger one)")
        A = self.ensure_arena()
        dev = A.flat.device
        d, H, D, V = cfg.hidden_size, cfg.num_attention_heads, head_dim_of(cfg), cfg.vocab_size
        rope = self._rope_table(cache.Smax, dev)[P:]  # row t of the slice is position P + t: the GEMM epilogue's table with S = n
        ids = input_ids.to(dev).contiguous()
        tower = getattr(m.get_model(), "vision_tower", None)
        use_images = tower is not None and images is not None and sum(int(im.shape[0]) for im in images) > 0
        src = self.validate_and_index(ids, None, None, None, images, use_images)
        r32 = self.fp32_residual
        feats = None
        if use_images:
            xt, N, Sv = self.tower(images, None)
            feats, rpi, row0, Pimg = self.projector(xt, N, Sv, None, out_f32=r32)
            assert (rpi, row0, Pimg) == self._splice_geometry()
        self._check_errors()
        emb = A.view("model.embed_tokens.weight", shape=(V, d))
        splice = O.embed_splice_fwd_f32 if r32 else O.embed_splice_fwd
        x = splice(ids.view(-1), src.view(-1) if src is not None else None, emb, feats)
        del feats
        lens1 = cache.lens + 1  # what the first new query sees: the cached rows and its own key
        hn = self._extend_layers(cache, x, rope, n, P, O.attn_extend, lens1, n, H, D, w_fp4=w_fp4)
        if w_fp4:
            logits = O.gemv_fp4w(hn[n - 1:n], self._fp4["lm_head"], out_f32=True, n=V)
        else:
            logits = O.gemv(hn[n - 1:n], self._lm_head_w(), out_f32=True, n=V)
        cache.advance(n)
        return logits

    def _extend_layers(self, cache, x, rope, n, P, attn, *attn_args, w_fp4=False):
        """The layer loop of extend and extend_branches over the n embedded rows x of one sequence: the prefill's GEMMs with `rope` as the
        RoPE epilogue's table (row t: the position of row t), the rotated keys and the values appended to cache rows [P, P + n), then
        attn (ops.attn_extend or ops.attn_extend_branches, with attn_args behind q and the layer's tensors) over the cache AFTER the
        append.  w_fp4=True: the projections of _llama_layer_fwd_fp4 on the MXFP4 copies.  -> the normalised final hidden rows [n, d]."""
        cfg = self.model.config
        H, D, eps = cfg.num_attention_heads, head_dim_of(cfg), cfg.rms_norm_eps
        F4 = (getattr(self, "_fp4", None) or self.quantize_decode_weights_fp4())["layers"] if w_fp4 else None
        for li, W in enumerate(self.llama):
            h1, _ = self._stream_norm(x, W.ln1, eps, want_x16=False)
            qkv = O.rope_qk_(O.gemm_fp4w(h1, F4[li]["wqkv"]), rope, n, H, D) if w_fp4 else O.gemm_nt_rope(h1, W.wqkv, rope, n, H, D)
            q, k, v = self._qkv(qkv)
            cache.append_rows(li, k, v, n, P, H, D)
            o = cache.attend(attn, li, q, *attn_args)
            x = self._stream_add_fp4(x, o, F4[li]["wo"]) if w_fp4 else self._stream_add(x, o, W.wo)
            h2, _ = self._stream_norm(x, W.ln2, eps, want_x16=False)
            act = O.swiglu_fwd(O.gemm_fp4w(h2, F4[li]["wgu"])) if w_fp4 else O.gemm_swiglu_fwd(h2, W.wgu)[1]
            x = self._stream_add_fp4(x, act, F4[li]["wd"]) if w_fp4 else self._stream_add(x, act, W.wd)
        return self._stream_norm(x, self.arena.view("model.norm.weight"), eps, want_x16=False)[0]

    HEAD_CHUNK = 256  # rows of fp32 logits held at a time by the scoring pass (256 x V floats: 33 MB at V = 32003)

    def head_logits(self, hn):
        """fp32 logits [rows, >= V] of normalised hidden rows through lm_head (the first V columns are valid): the decode step's GEMV up
        to its 16 rows, the prefill's GEMM beyond."""
        V = self.model.config.vocab_size
        if hn.shape[0] <= 16:
            return O.gemv(hn, self._lm_head_w(), out_f32=True, n=V)
        return O.gemm_nt(hn, self._lm_head_w(), out_f32=True)

    def extend_branches(self, cache, plan, pos=None, return_logits=False):
        """The R = len(plan.fed) packed rows of several text continuations of ONE prompt (generation scoring: scoring.score) on a plain
        KVCache that holds the P = cache.lens[0] prompt tokens: extend's layer loop with every continuation branching off the prompt.
        plan (scoring._branch_plan): fed [R] token ids, seg_start int32 [R] (the packed index of the first row of the row's continuation)
        and rel_pos int32 [R] (the row's offset inside it).  The embedding is a plain gather, the RoPE epilogue reads a table whose row
        r is position P + rel_pos[r], the rotated keys and the values go to cache rows [P, P + R) in packed order, and
        mh_attn_extend_branches lets row r see the prompt and rows seg_start[r] .. r only.  One pass over the 16-bit weights for all
        continuations.  cache.lens is NOT advanced: the rows behind the prompt are stale afterwards, as after a rejected draft.
        Returns the normalised final hidden rows [R, d] (head_logits turns a chunk of them into logits); return_logits=True: (hidden,
        fp32 logits [R, V]), for tests.  pos: P when the caller knows it on the host."""
        m = self.model
        cfg = m.config
        if not isinstance(cache, HipEngine.KVCache) or cache.B != 1 or cache.rpos is not None:
            raise ValueError("extend_branches takes a plain KVCache of one sequence whose rotary positions are its rows (B = 1, no left padding or holes)")
        fed = [int(t) for t in (plan.fed.tolist() if isinstance(plan.fed, torch.Tensor) else plan.fed)]
        R = len(fed)
        d, H, D, V = cfg.hidden_size, cfg.num_attention_heads, head_dim_of(cfg), cfg.vocab_size
        if R < 1 or tuple(plan.seg_start.shape) != (R,) or tuple(plan.rel_pos.shape) != (R,):
            raise ValueError(f"extend_branches takes a plan of R >= 1 rows with seg_start and rel_pos [R], got {R} fed tokens")
        if any(not 0 <= t < V for t in fed):
            raise ValueError(f"extend_branches: fed token ids must lie in [0, {V})")
        seg_h, rel_h = [int(v) for v in plan.seg_start.tolist()], [int(v) for v in plan.rel_pos.tolist()]
        # the kernel's tile skips rely on it: a segment starts at its own first row, so seg_start is non-decreasing and <= r
        if any(not (s == r or (r > 0 and s == seg_h[r - 1])) or rel_h[r] != r - s for r, s in enumerate(seg_h)):
            raise ValueError("extend_branches: seg_start[r] must be the packed index of the first row of r's own continuation "
                             "(non-decreasing, seg_start[r] <= r, a new value only at r itself) and rel_pos[r] = r - seg_start[r]")
        P = int(cache.lens[0]) if pos is None else int(pos)
        if P < 0 or P + R > cache.Smax:
            raise ValueError(f"extend_branches: {P} cached + {R} rows exceed the cache's {cache.Smax} rows (grow_cache makes a larger one)")
        A = self.ensure_arena()
        dev = A.flat.device
        seg = plan.seg_start.to(device=dev, dtype=torch.int32).contiguous()
        rel = plan.rel_pos.to(device=dev, dtype=torch.int64)
        rope = self._rope_table(cache.Smax, dev).index_select(0, rel + P)  # row r: position P + rel_pos[r] (< P + R <= Smax)
        ids = torch.tensor(fed, dtype=torch.int64, device=dev)
        emb = A.view("model.embed_tokens.weight", shape=(V, d))
        x = (O.embed_splice_fwd_f32 if self.fp32_residual else O.embed_splice_fwd)(ids, None, emb, None)
        hn = self._extend_layers(cache, x, rope, R, P, O.attn_extend_branches, seg, P, H, D)
        if not return_logits:
            return hn
        step = self.HEAD_CHUNK
        return hn, torch.cat([self.head_logits(hn[r0:r0 + step])[:, :V] for r0 in range(0, R, step)])

    def grow_cache(self, cache, Smax):
        """A new KVCache of Smax >= cache.Smax rows per sequence holding the rows of `cache` (the scales [B, H, Smax] of the fp8 form
        included), same format, lengths and positions.  Off the hot path: plain copies, once per growth of a session."""
        out = cache.grown(Smax)
        self._rope_table(int(Smax), out.lens.device)
        return out

    def new_cache(self, B, Smax, fp8=False):
        """An empty KVCache of B sequences and Smax rows in the model's geometry (a session's cache: generation.Session)."""
        cfg = self.model.config
        A = self.ensure_arena()
        self._rope_table(int(Smax), A.flat.device)
        return HipEngine.KVCache(len(self.llama), int(B), int(Smax), cfg.hidden_size, A.flat.dtype, A.flat.device, fp8=bool(fp8),
                                 H=cfg.num_attention_heads)

    def expand_prefix(self, cache, nb, P, Smax):
        """New cache of nb rows and Smax rows per sequence whose every row holds the first P rows of the one-sequence `cache` (beam search
        from a session's cache, which may be far larger than the prompt: expand_cache would copy all of it per beam).  Once per call,
        plain copies; `cache` is not written."""
        out = cache.expanded_prefix(nb, P, Smax)
        self._rope_table(int(Smax), out.lens.device)
        return out

    def pair_cache(self, cond_cache, uncond_cache, max_new):
        """A plain KVCache of B = 2 for guided decoding (generate(guidance_scale=...)): row 0 holds the rows of the conditional prompt's
        cache, row 1 the unconditional's, lens per row, Smax = max(len) + max_new, the format of its inputs (16-bit, or fp8 with ks / vs).
        Both inputs are one-sequence, un-padded caches of one format.  Once per call, plain copies; the inputs are not written.
        decode_step and verify_step run on it like on any right-padded batch."""
        out = KVCache.paired(cond_cache, uncond_cache, max_new)
        self._rope_table(out.Smax, out.lens.device)
        return out

    def expand_cache(self, cache, rows):
        """New cache whose row i is a copy of `cache` row rows[i] (int64 on the device): a prefilled batch expanded to
        num_beams rows per prompt (the reference: inputs_embeds.repeat_interleave(5), base_mmgpt.py:162-163)."""
        A = self.arena
        n = int(rows.numel())
        Smax, d = cache.Smax, cache.k[0].shape[-1]
        out = HipEngine.KVCache(0, n, Smax, d, A.flat.dtype, A.flat.device, fp8=cache.fp8, H=cache.H)
        for li in range(len(cache.k)):
            for src_l, dst_l in zip(cache.sets(), out.sets()):
                src = src_l[li]
                dst = torch.empty(n, *src.shape[1:], dtype=src.dtype, device=src.device)
                O.gather_rows2d(src.view(cache.B, -1), rows, dst.view(n, -1))
                dst_l.append(dst)
        out.lens = cache.lens.index_select(0, rows).contiguous()  # B int32 values, once per generate() call
        out.rpos = cache.rpos.index_select(0, rows).contiguous() if cache.rpos is not None else None
        return out

    def reorder_cache(self, cache, beam_idx, n_valid):
        """cache row i <- cache row beam_idx[i] for the first n_valid positions (HF `_reorder_cache` under beam search):
        one gather kernel per layer and tensor into a second buffer set, then the sets swap."""
        cache.reorder(beam_idx, n_valid)

    def quantize_decode_weights(self):
        """fp8 (OCP e4m3, one scale per 128 k) copies of the decoder's Linear weights for the decode step (BASELINE cfg 5's
        weight format; activations stay 16-bit).  ~half the bytes per token.  Re-run after the weights change."""
        self.ensure_arena()
        q = []
        for W in self.llama:
            q.append(dict(wqkv=O.quant_fp8_b128(W.wqkv), wo=O.quant_fp8_b128(W.wo), wgu=O.quant_fp8_b128(W.wgu), wd=O.quant_fp8_b128(W.wd)))
        self._fp8 = dict(layers=q, lm_head=O.quant_fp8_b128(self._lm_head_w()[:self.model.config.vocab_size]))
        return self._fp8

    def quantize_decode_weights_fp4(self):
        """MXFP4 (OCP e2m1, one power-of-two scale per 32 k: ops.quant_fp4_b32) copies of the decoder's Linear weights and of lm_head's
        vocab_size rows for the decode step (activations stay 16-bit).  ~0.53 bytes per weight.  weights_changed() drops them."""
        cfg = self.model.config
        for name in ("hidden_size", "intermediate_size"):
            if getattr(cfg, name) % 32:
                raise ValueError(f"fp4 decode weights need {name} = {getattr(cfg, name)} to be a multiple of the 32-element scale block")
        self.ensure_arena()
        q = []
        for W in self.llama:
            q.append(dict(wqkv=O.quant_fp4_b32(W.wqkv), wo=O.quant_fp4_b32(W.wo), wgu=O.quant_fp4_b32(W.wgu), wd=O.quant_fp4_b32(W.wd)))
        self._fp4 = dict(layers=q, lm_head=O.quant_fp4_b32(self._lm_head_w()[:cfg.vocab_size]))
        return self._fp4

    def decode_step(self, tokens, cache, fp8=False, fp4=False):
        """One new token per sequence (tokens int64 [B]) at position cache.lens[b]; returns logits fp32 [B, V] and
        advances the cache.  Every op is an HBM-bound kernel: weights and cache are streamed exactly once.
        fp8=True uses the fp8 weight copies of quantize_decode_weights(), fp4=True the MXFP4 copies of quantize_decode_weights_fp4()
        (one of the two).  An fp8 cache (prefill(kv_fp8=True)) appends and attends in its own kernels (mh_decode_rope_append_kv8,
        mh_attn_decode_kv8), with any weight format."""
        logits = self._decode_rows(tokens, cache, fp8, fp4, 0)
        cache.advance(1)  # in place, after every kernel that read the positions: the captured graph sees the same buffers
        return logits

    def verify_step(self, tokens, cache, fp8=False, fp4=False):
        """T new tokens per sequence (tokens int64 [B, T], B*T <= 16) at positions cache.lens[b] .. + T - 1: the decode step's body on
        B*T rows, one pass over the weights; returns logits fp32 [B, T, V], row (b, t) conditioned on the cache and tokens[b, :t + 1].
        Writes cache rows lens .. lens + T - 1 (mh_decode_rope_append_multi*, attention by mh_attn_decode_multi* with causality inside
        the block) and does NOT advance the cache: the caller keeps what it accepts with cache.advance(n); rows beyond the new length
        are stale and the next step overwrites them.  The verify step of prompt-lookup decoding (generation.py)."""
        B, T = tokens.shape
        if B != cache.B or not 1 <= T or B * T > 16:
            raise ValueError(f"verify_step takes tokens [B = {cache.B}, T] with B*T <= 16, got {tuple(tokens.shape)}")
        return self._decode_rows(tokens.reshape(-1), cache, fp8, fp4, T).view(B, T, -1)

    def _decode_rows(self, tokens, cache, fp8, fp4, T):
        """The decode body: T = 0, one row per sequence (decode_step); T >= 1, rows b*T + t (verify_step).  Does not advance the cache."""
        if fp8 and fp4:
            raise ValueError(f"{'verify_step' if T else 'decode_step'}: fp8 and fp4 weights are alternatives, not a combination")
        cfg = self.model.config
        A = self.arena
        d, H, D, V = cfg.hidden_size, cfg.num_attention_heads, head_dim_of(cfg), cfg.vocab_size
        eps = cfg.rms_norm_eps
        if fp4:
            F4 = getattr(self, "_fp4", None) or self.quantize_decode_weights_fp4()
            gemv, gemv_norm, head = O.gemv_fp4w, O.gemv_fp4w_norm, F4["lm_head"]
            layers = [(Q["wqkv"], Q["wo"], Q["wgu"], Q["wd"]) for Q in F4["layers"]]
        elif fp8:
            F8 = getattr(self, "_fp8", None) or self.quantize_decode_weights()
            gemv, gemv_norm, head = O.gemv_fp8w, O.gemv_fp8w_norm, F8["lm_head"]
            layers = [(Q["wqkv"], Q["wo"], Q["wgu"], Q["wd"]) for Q in F8["layers"]]
        else:
            gemv, gemv_norm, head = O.gemv, O.gemv_norm, self._lm_head_w()
            layers = [(W.wqkv, W.wo, W.wgu, W.wd) for W in self.llama]
        emb = A.view("model.embed_tokens.weight", shape=(V, d))
        x = O.gather_rows(emb, tokens.to(A.flat.device).view(-1))
        if T and isinstance(cache, BeamKVCache):
            raise ValueError("verify_step takes a KVCache: a BeamKVCache decodes one token per beam (decode_step)")
        lens1 = cache.pos + 1  # what a step's first query sees: the cached rows and its own key
        for li, (wqkv, wo, wgu, wd) in enumerate(layers):
            W = self.llama[li]
            if not cache.fp8 and T == 0:
                # a 16-bit cache's single-token step: input_layernorm + q|k|v projection + RoPE + K/V append in one launch
                qkv = O.gemv_qkv_rope(x, W.ln1, eps, wqkv, self.rope, cache.pos, *cache.layer(li), H, D, rope_pos=cache.rope_pos)
            else:  # the projection, then RoPE + append as a launch of the cache's own
                qkv = gemv_norm(x, W.ln1, eps, wqkv)
                cache.append_step(li, qkv, self.rope, T, H, D)
            o = cache.attend_step(li, qkv[:, :d], lens1, T, H, D)
            x2 = gemv(o, wo, resid=x)
            act = gemv_norm(x2, W.ln2, eps, wgu, swiglu=True)  # post_attention_layernorm + gate|up + SwiGLU: one launch
            x = gemv(act, wd, resid=x2)
        hn = O.rmsnorm_fwd(x, A.view("model.norm.weight"), eps)
        return gemv(hn, head, out_f32=True, n=V)  # (the 16-bit weight view carries its zero pad rows; the fp8 copy has V rows)

    def capture_decode_graph(self, cache, fp8=False, fp4=False):
        """Capture one decode step (≈300 launches) into a HIP graph bound to `cache`: returns (graph, token buffer int64 [B],
        logits buffer fp32 [B, V]).  Positions live in cache.lens on the device and advance inside the graph, so every
        replay is the next token.  One eager warm-up step runs first (function attributes, symbol look-ups and allocator
        warm-up must not happen during capture); it writes only the cache rows the first real step rewrites."""
        dev = self.arena.flat.device
        tok = torch.zeros(cache.B, dtype=torch.int64, device=dev)
        keep = cache.lens.clone()
        keep_r = cache.rpos.clone() if cache.rpos is not None else None
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self.decode_step(tok, cache, fp8=fp8, fp4=fp4)
        torch.cuda.current_stream(dev).wait_stream(side)
        cache.lens.copy_(keep)
        if keep_r is not None:
            cache.rpos.copy_(keep_r)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            logits = self.decode_step(tok, cache, fp8=fp8, fp4=fp4)
        cache.lens.copy_(keep)  # capture does not execute, but keep the invariant explicit
        if keep_r is not None:
            cache.rpos.copy_(keep_r)
        return g, tok, logits

    def capture_verify_graph(self, cache, T, fp8=False, fp4=False):
        """capture_decode_graph for verify_step: returns (graph, token buffer int64 [B, T], logits buffer fp32 [B, T, V]).  One eager
        warm-up on a side stream, then the capture on a single stream (no parallel branches).  The step reads cache.lens / rpos from
        the device and does not advance them, so the graph can be replayed next to the plain decode graph on the same cache; the
        warm-up writes only rows at and beyond the current length, which the next real step rewrites."""
        dev = self.arena.flat.device
        tok = torch.zeros(cache.B, T, dtype=torch.int64, device=dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self.verify_step(tok, cache, fp8=fp8, fp4=fp4)
        torch.cuda.current_stream(dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            logits = self.verify_step(tok, cache, fp8=fp8, fp4=fp4)
        return g, tok, logits

    def draft_chain(self, cache, tok, k, sel, ban_tables, seq, counters):
        """The body capture_draft_graph captures, on the current stream: k times [decode step on tok[i] (16-bit weights) -> the call's bans
        (mh_ban_tokens_dev, history seq[0, :n + i]) -> selection with key (seed, emitted + i, row 0) (mh_select_tokens_dev)], the token
        written to tok[i + 1] - which step i + 1 feeds - and to seq[0, n + i], which the next step's ban reads (stream order).  emitted
        (int64) and n (int32) are the device counters `counters` = (step_base, len_base).  Advances the cache by k."""
        V = self.model.config.vocab_size
        step_base, len_base = counters
        for i in range(k):
            logits = self.decode_step(tok[i:i + 1], cache)
            if ban_tables is not None:
                O.ban_tokens_dev(logits, V, seq, len_base, len0=i, **ban_tables)
            O.select_tokens_dev(logits, V, step_base, i, out=tok[i + 1:i + 2], ids=seq, len_base=len_base, len_off=i, **sel)

    def capture_draft_graph(self, cache, k, sel, ban_tables, seq, counters):
        """The draft chain of assisted decoding (generate(assistant_model=...)) as ONE replayable HIP graph bound to `cache`, this
        (draft) engine's one-sequence 16-bit cache: draft_chain's k steps.  -> (graph, tok int64 [k + 1]): the caller writes the
        sequence's last token to tok[0] and the two counters, replays, and reads the k drafted tokens from tok[1:] (tok is also the
        verify step's input row).  sel: the selection's keyword arguments; ban_tables: generation._ban_tables of the call or None; seq
        int64 [1, cells]: the call's ids buffer; counters = (emitted int64 [1], n int32 [1]) on the device.  The cache advances by k
        inside the graph; the caller truncates it to what was accepted.  Captured on one stream, no parallel branches
        (capture_verify_graph).  The eager warm-up writes cache rows at and behind the current length, tok[1:] and k cells of seq behind
        the counter's n: all of them scratch until the next replay rewrites them; the cache's length is restored."""
        if cache.B != 1 or cache.fp8 or cache.rpos is not None or not 1 <= k <= 15:
            raise ValueError("capture_draft_graph takes a one-sequence 16-bit cache without padding and 1 <= k <= 15")
        dev = self.arena.flat.device
        tok = torch.zeros(k + 1, dtype=torch.int64, device=dev)
        keep = cache.lens.clone()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self.draft_chain(cache, tok, k, sel, ban_tables, seq, counters)
        torch.cuda.current_stream(dev).wait_stream(side)
        cache.lens.copy_(keep)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.draft_chain(cache, tok, k, sel, ban_tables, seq, counters)
        cache.lens.copy_(keep)  # (capture does not execute)
        return g, tok

    # standalone sub-module calls (reference module surface; not used by the fused forward)
    def tower_forward_public(self, images):
        self.ensure_arena()
        tower = self.model.get_model().vision_tower
        x, N, S = self.tower(images, None)
        vd = x.shape[1]
        x3 = x.view(N, S, vd)
        feats = x3 if tower.select_feature == "cls_patch" else x3[:, 1:]
        feats = feats.to(images[0].dtype)
        return torch.split(feats, [im.shape[0] for im in images], dim=0)

    def projector_forward_public(self, features):
        """mlp_projector.py:19-23 / conv_projector.py:23-39 as a standalone call: list of [n_i, P, C] -> list of [n_i, P', d]."""
        self.ensure_arena()
        A = self.arena
        proj = self.model.get_model().projector
        wname, bname = "model.projector.projector.weight", "model.projector.projector.bias"
        out = []
        for f in features:
            if hasattr(proj, "conv_stride"):
                if f.dim() == 1:  # conv_projector.py:27-28: the 1-D dummy feature is tiled to 256 tokens
                    f = f.view(1, 1, -1).repeat(1, 256, 1)
                n, P, C = f.shape
                G = int(math.sqrt(P))
                x = f.to(A.flat.dtype).reshape(n * P, C).contiguous()
                cols = O.conv3x3_cols(x, n, G, C, proj.conv_stride, P, 0)
                w = A.view(wname, shape=(A.params[wname].shape[0], C * 9))
                y = O.gemm_nt(cols, w, bias=A.view(bname))
                out.append(y.view(n, -1, y.shape[-1]))
                continue
            f2 = f.to(A.flat.dtype).reshape(-1, f.shape[-1]).contiguous()
            y = O.gemm_nt(f2, A.view(wname), bias=A.view(bname))
            out.append(y.view(*f.shape[:-1], -1))
        return out
