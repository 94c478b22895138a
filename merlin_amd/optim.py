"""Fused AdamW over the flat parameter arena (reference: torch AdamW built by MMGPTTrainer.create_optimizer,
mmgpt/engine/train/trainer.py:45-74: decoupled weight decay, no decay on biases / norm weights).

One `mh_adamw` launch per run of adjacent parameters sharing (lr scale, weight decay): a handful of launches
per layer instead of one per tensor.  fp32 moments live in two flat buffers shaped like the arena.

How the new value of a parameter goes back into the bf16 arena is `FusedAdamW(rounding=...)`:

  "nearest"     (default) round to nearest even, as torch AdamW on bf16 parameters does (the reference: builder.py:163).  An update below
                half a bf16 spacing is rounded away.  Emulated on the CPU (tests/test_adamw_rounding_cpu.py): a tensor of ones stepped 400
                times by 5e-5 (pretrain.sh's peak lr, a full-lr Adam step) is still exactly 1.0 (half a spacing below 1.0 is 1.95e-3); of
                weights drawn at sigma 0.02, 43 % are bit-identical after one such step (every |w| >= 2^-6 has a half-spacing of
                6.1e-5 > lr), and 92 % at the first ViT layers' lr under LLRD (0.9^22: 4.9e-6), where the cosine schedule takes every layer
                in the end.
  "split"       an int16 low half per parameter (`self.lo`, +2 bytes per parameter: 14.1 GB for the 7B arena, 26 B moved per parameter
                instead of 22; a full fp32 copy would be +28 GB): (p, lo) together are an fp32 master, the update is exact fp32-master
                AdamW, and p is that master rounded to nearest.  bf16 only.  `lo` is only valid beside the p it was written with: when the
                weights changed behind the optimizer (a load, a stock torch step, a repack) the next step() restarts from master := p and
                counts it in `self.reseeds`.
  "stochastic"  no extra state: the store rounds up with a probability equal to the dropped fraction (unbiased), drawn from a hash of
                (seed, step, arena index), so every data-parallel rank computes the same bits from the same gradients.  bf16 only.

How the moments are kept is `FusedAdamW(states=...)`, independent of `rounding`:

  "fp32"        (default) m and v as two fp32 vectors shaped like the arena: 8 bytes per parameter (56 GB for the 7B arena), 22 bytes moved
                per parameter and step.
  "compact"     m as OCP e4m3 bytes with one power-of-two scale byte per 128-element block, v as bf16, both written with stochastic
                rounding from a hash of (seed, step, arena index): 3 + 1/128 bytes per parameter (21 GB), 12 bytes moved.  The format is
                include/merlin_hip.h's (mh_adamw_compact).  v is not rounded to nearest because one step changes it by at most
                1 - beta2 relative, below half a bf16 spacing: it would never decay.  The update itself runs on the decoded fp32 moments
                and the unrounded new ones, so only the stored moments carry the format's noise; simulated on synthetic gradient streams
                (tests/adamw_compact_ref.py) a step deviates by about 8 % relative RMS from fp32 moments and 400 accumulated steps by about
                1.5 %.  bf16 only.

Not covered: optimizer-state save and restore (FusedAdamW has none for m and v either).  Resuming with lo = 0 restarts from the stored bf16
weights."""
from __future__ import annotations

import math
import re

import torch

from . import ops as O
from .weights import MASK64, splitmix64_scalar

ROUNDINGS = ("nearest", "split", "stochastic")
STATES = ("fp32", "compact")
BLOCK = 128  # elements per scale byte of the compact m; arena offsets are multiples of it (arena.ALIGN)


# ---- layer-wise learning-rate decay (mmgpt/utils/llrd_utils.py:4-23), selected by --llrd / --llm_llrd (trainer.py:56-61) ----
def vit_lr_scale(name: str) -> float:
    """CLIP tower: 0.9 ** (22 - layer) for encoder layers, 0.1 for the rest of the vision model, 1 elsewhere."""
    if "vision_model.encoder.layers" in name:
        layer = int(re.findall(r"layers\.(\d+)\.", name)[0])
        return 0.9 ** (23 - layer - 1)
    if "vision_model" in name:
        return 0.1
    return 1


def llm_lr_scale(name: str) -> float:
    """Decoder: 0.931 ** (31 - layer) for `model.layers.N.`, 1 elsewhere."""
    if "model.layers" in name:
        layer = int(re.findall(r"layers\.(\d+)\.", name)[0])
        return 0.931 ** (32 - layer - 1)
    return 1


def per_param_hparams(named_parameters, lr, weight_decay, lr_scale_fn=None):
    """{name: (lr, weight_decay)} for the trainable parameters: the two rules of the reference's optimizer construction
    (trainer.py:45-74 / llrd_utils.py:26-79) - biases and 1-D tensors are not decayed; lr is scaled per layer by lr_scale_fn.
    (The reference materialises this as torch param groups; the fused optimizer keeps it per arena range instead.)"""
    out = {}
    for name, prm in named_parameters:
        if not prm.requires_grad:
            continue
        wd = 0.0 if (name.endswith(".bias") or prm.dim() == 1) else weight_decay
        out[name] = (lr * (lr_scale_fn(name) if lr_scale_fn is not None else 1), wd)
    return out


def cosine_with_warmup(step: int, total_steps: int, warmup_ratio: float = 0.0, num_cycles: float = 0.5) -> float:
    """lr multiplier of HF's `cosine` scheduler as the reference launches it (pretrain.sh:28-29: --warmup_ratio 0.01
    --lr_scheduler_type cosine): linear warm-up over ceil(total * ratio) steps, then half a cosine to zero."""
    warmup = math.ceil(total_steps * warmup_ratio)
    if step < warmup:
        return float(step) / float(max(1, warmup))
    progress = float(step - warmup) / float(max(1, total_steps - warmup))
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * num_cycles * 2.0 * progress)))


class FusedAdamW:
    def __init__(self, engine, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, lr_scale_fn=None, rounding="nearest", seed=0,
                 states="fp32"):
        """rounding: how p is stored ("nearest", "split", "stochastic"); states: how m and v are kept ("fp32", "compact"): see the module
        docstring for both; seed: of the stochastic stores.  No state is saved or restored: resuming a "split" run starts from the stored
        bf16 weights (lo = 0), and m, v start from zero."""
        if rounding not in ROUNDINGS:
            raise ValueError(f"rounding={rounding!r} is not one of {ROUNDINGS}")
        if states not in STATES:
            raise ValueError(f"states={states!r} is not one of {STATES}")
        self.engine = engine
        self.rounding, self.states, self.seed = rounding, states, int(seed)
        self.lo = None        # "split": int16 low halves of the fp32 masters, shaped like the arena
        self.reseeds = 0      # "split": how often lo was dropped because the weights changed behind the optimizer
        self._lo_for = None   # (engine.weight_version, address of the arena's flat) that lo belongs to
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.lr_scale_fn = lr_scale_fn  # name -> multiplier (layer-wise lr decay, llrd_utils.py:4-79)
        self.step_count = 0
        self.m = self.v = None                        # states="fp32"
        self.m8 = self.mscale = self.v16 = None       # states="compact": e4m3 bytes, one scale byte per BLOCK elements, bf16
        self._runs = None
        self._flat_id = None
        self._clip = None
        self._ss = None

    def _build(self):
        A = self.engine.ensure_arena()
        if self.states == "compact" and A.flat.dtype != torch.bfloat16:
            raise ValueError(f"states='compact' needs bfloat16 parameters, got {A.flat.dtype}: mh_adamw_compact is bf16 only")
        sig = (A.flat.data_ptr(), tuple(p.requires_grad for p in A.params.values()))  # freeze / unfreeze rebuilds the runs
        if self._flat_id == sig and self._runs is not None:
            return A
        if self.states == "compact":
            if self.m8 is None or self.m8.numel() != A.total or self.m8.device != A.flat.device:
                self.m8 = torch.zeros(A.total, dtype=torch.uint8, device=A.flat.device)
                self.mscale = torch.full((A.total // BLOCK,), 127, dtype=torch.uint8, device=A.flat.device)  # an all-zero block: e = 0
                self.v16 = torch.zeros(A.total, dtype=torch.bfloat16, device=A.flat.device)
        elif self.m is None or self.m.numel() != A.total or self.m.device != A.flat.device:
            self.m = torch.zeros(A.total, dtype=torch.float32, device=A.flat.device)
            self.v = torch.zeros(A.total, dtype=torch.float32, device=A.flat.device)
        hp = per_param_hparams(A.params.items(), 1.0, self.weight_decay, self.lr_scale_fn)  # lr as a multiplier of self.lr
        runs = []
        prev = -2  # index (arena order) of the last trainable parameter: runs only merge DIRECTLY adjacent parameters
        for idx, n in enumerate(A.names):
            p = A.params[n]
            if not p.requires_grad:
                continue
            sc, wd = hp[n]
            off, num = A.offset[n], p.numel()
            if runs and prev == idx - 1 and runs[-1][2] == sc and runs[-1][3] == wd:
                runs[-1][1] = off + num - runs[-1][0]  # merge (alignment gaps between neighbours hold zeros and stay zero)
            else:
                runs.append([off, num, sc, wd])
            prev = idx
        self._runs = runs
        self._flat_id = sig
        return A

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0, max_grad_norm: float = None, lr_mult: float = 1.0):
        """One AdamW update.  grad_scale folds 1/world_size (and loss scaling) into the kernel; max_grad_norm clips the
        global gradient norm like HF Trainer (--max_grad_norm, default 1.0) with the coefficient computed and applied
        on the device; lr_mult is the scheduler's multiplier for this step (cosine_with_warmup)."""
        A = self._build()
        if self.rounding != "nearest" and A.flat.dtype != torch.bfloat16:
            raise ValueError(f"rounding={self.rounding!r} needs bfloat16 parameters, got {A.flat.dtype}: the top half of an fp32 is a bf16")
        if A.gflat is None:
            return
        self.step_count += 1
        if self.rounding == "split":
            self._ensure_lo(A)
        key = self.sr_key(self.step_count) if self.rounding == "stochastic" else None
        skey = self.state_key(self.step_count) if self.states == "compact" else None
        b1, b2 = self.betas
        clip = None
        if max_grad_norm is not None and max_grad_norm > 0:
            if self._clip is None or self._clip.device != A.flat.device:
                self._clip = torch.zeros(2, dtype=torch.float32, device=A.flat.device)
            O.clip_scale(self.grad_norm_sq(), grad_scale, max_grad_norm, self._clip)
            clip = self._clip
        for off, num, sc, wd in self._runs:
            if self.states == "compact":
                O.adamw_compact_(A.flat[off: off + num], self.lo[off: off + num] if self.rounding == "split" else None, A.gflat[off: off + num],
                                 self.m8[off: off + num], self.mscale[off // BLOCK:], self.v16[off: off + num], self.lr * sc * lr_mult, b1, b2,
                                 self.eps, wd, self.step_count, grad_scale, clip, O.P_MODES[self.rounding], key or 0, skey, off)
                continue
            args = (A.flat[off: off + num], A.gflat[off: off + num], self.m[off: off + num], self.v[off: off + num],
                    self.lr * sc * lr_mult, b1, b2, self.eps, wd, self.step_count, grad_scale)
            if self.rounding == "split":
                O.adamw_split_(args[0], self.lo[off: off + num], *args[1:], clip)
            elif self.rounding == "stochastic":
                O.adamw_sr_(*args, clip, key, off)
            elif clip is None:
                O.adamw_(*args)
            else:
                O.adamw_clip_(*args, clip)
        self.engine.weights_changed()  # derived copies (fp8 weights, padded patch-embedding weight) are stale now
        if self.rounding == "split":
            self._lo_for = self._weights_id(A)

    def sr_key(self, step: int) -> int:
        """The stochastic store's hash key of one step."""
        return splitmix64_scalar((self.seed & MASK64) ^ ((step * 0xD1342543DE82EF95) & MASK64))

    def state_key(self, step: int) -> int:
        """The compact moments' hash key of one step (another stream than sr_key's)."""
        return splitmix64_scalar((self.seed & MASK64) ^ ((step * 0xA0761D6478BD642F) & MASK64))

    def state_bytes(self) -> int:
        """Bytes held in moment buffers (0 before the first step builds them)."""
        return sum(t.numel() * t.element_size() for t in (self.m, self.v, self.m8, self.mscale, self.v16) if t is not None)

    def moments(self, name):
        """fp32 (m, v) of one parameter, shaped like it: views of the fp32 buffers, or decoded copies of the compact ones (exact).  For tests
        and checkpoint tooling, not the hot path."""
        A = self._build()
        p, off = A.params[name], A.offset[name]
        if self.states == "compact":
            m, v = O.adamw_states_unpack(self.m8[off: off + p.numel()], self.mscale[off // BLOCK:], self.v16[off: off + p.numel()])
        else:
            m, v = self.m[off: off + p.numel()], self.v[off: off + p.numel()]
        return m.view(p.shape), v.view(p.shape)

    def _weights_id(self, A):
        return (self.engine.weight_version, A.flat.data_ptr())

    def _ensure_lo(self, A):
        """lo belongs to the weights this optimizer last wrote: anything else (a load, a stock torch step, a repack) restarts master := p.
        A needless restart costs at most half a bf16 spacing, once."""
        if self.lo is None or self.lo.numel() != A.total or self.lo.device != A.flat.device:
            self.lo = torch.zeros(A.total, dtype=torch.int16, device=A.flat.device)
        elif self._lo_for != self._weights_id(A):
            self.lo.zero_()
            self.reseeds += 1

    def master(self, name):
        """fp32 master of a parameter under rounding="split", rebuilt from (p, lo): for tests and checkpoint tooling, not the hot path."""
        if self.rounding != "split":
            raise ValueError(f"master() needs rounding='split', not {self.rounding!r}")
        A = self.engine.ensure_arena()
        p = A.params[name]
        off = A.offset[name]
        hi = A.flat[off: off + p.numel()].view(torch.int16).to(torch.int32) << 16
        if self.lo is not None and self._lo_for == self._weights_id(A):  # (a stale lo is not used: master = p)
            hi = hi + self.lo[off: off + p.numel()].to(torch.int32)
        return hi.view(torch.float32).view(p.shape)

    def last_grad_norm(self):
        """Total gradient norm seen by the last clipped step (device scalar; what HF logs as grad_norm)."""
        return None if self._clip is None else self._clip[1]

    def zero_grad(self, set_to_none=True):
        A = self.engine.arena
        if A is None:
            return
        for p in A.params.values():
            p.grad = None

    def grad_norm_sq(self):
        """Sum of squares of the gradient arena (device scalar tensor; frozen parameters hold zeros)."""
        A = self.engine.arena
        if self._ss is None or self._ss.device != A.flat.device:
            self._ss = torch.zeros(2049, dtype=torch.float32, device=A.flat.device)
        O.sumsq_det(A.gflat, self._ss[1:], self._ss[:1])  # fixed-order reduction: reproducible clip coefficient
        return self._ss[:1]

    def grad_norm(self):
        """Global L2 norm of the gradient arena (device scalar tensor)."""
        return self.grad_norm_sq().sqrt()
