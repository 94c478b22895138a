"""AdamW on compact moments against the same build's fp32-moment kernels, per parameter store (nearest, split, stochastic), HIP events, on the
GPU box: mh_adamw_compact moves 12 + 1/64 bytes per parameter (p, g read, p written: 6; the e4m3 byte, the bf16 v and 1/128 scale byte read and
written: 6 + 1/64) where mh_adamw_clip / mh_adamw_sr move 22 and mh_adamw_split 26 (split: + 4 for lo in both forms).

    python tools/bench_adamw_compact.py [--out profiles/adamw_compact_bench.txt] [--rounds 5] [--skip-arena]

Two sizes: one launch over 2^30 parameters, and the run list FusedAdamW builds for the 7B arena (ViT-L/14-336 + mlp projector + Llama-7B with
layer-wise lr decay on the tower, bench.py's optimizer), one launch per run as step() makes them.  The arms alternate inside every round, every
arm is warmed at the size it is timed at, and a timing covers `iters` passes between two device events.  No ratio is asserted: the byte counts
predict 12/22 (16/26 for split) of the fp32-moment time, and the report says what was measured."""
import argparse
import gc
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from merlin_amd import ops as O  # noqa: E402

HP = (5e-5, 0.9, 0.95, 1e-8, 0.05)  # lr, beta1, beta2, eps, wd (pretrain.sh)
BYTES = {"nearest": (22, 12 + 1 / 64), "split": (26, 16 + 1 / 64), "stochastic": (22, 12 + 1 / 64)}  # per parameter: fp32 moments, compact


def event_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def arena_runs(dev):
    """(total, [(offset, elements)]) of the optimizer runs of the benchmark's model."""
    from bench import LLAMA_7B, VIT_L_336
    from merlin_amd.model.llama_mmgpt import build_synthetic_model
    from merlin_amd.optim import FusedAdamW, vit_lr_scale

    model = build_synthetic_model(LLAMA_7B, VIT_L_336, projector="mlp", dtype=torch.bfloat16, device=dev, seed=0)
    opt = FusedAdamW(model.engine, lr=HP[0], betas=HP[1:3], weight_decay=HP[4], lr_scale_fn=vit_lr_scale, states="compact")
    total = opt._build().total
    runs = [(off, num) for off, num, _, _ in opt._runs]
    del opt, model
    gc.collect()
    torch.cuda.empty_cache()
    return total, runs


def measure(what, total, runs, dev, rounds, lines):
    p, g = torch.empty(total, dtype=torch.bfloat16, device=dev), torch.empty(total, dtype=torch.bfloat16, device=dev)
    O.fill_normal_(p, 1, 0, 0.02)
    O.fill_normal_(g, 2, 0, 0.01)
    m, v, lo = torch.zeros(total, device=dev), torch.zeros(total, device=dev), torch.zeros(total, dtype=torch.int16, device=dev)
    m8, ms = torch.zeros(total, dtype=torch.uint8, device=dev), torch.full((total // 128,), 127, dtype=torch.uint8, device=dev)
    v16 = torch.zeros(total, dtype=torch.bfloat16, device=dev)
    gdev = torch.ones(1, device=dev)
    n = sum(num for _, num in runs)

    def fp32(mode):
        for off, num in runs:
            s = slice(off, off + num)
            if mode == "split":
                O.adamw_split_(p[s], lo[s], g[s], m[s], v[s], *HP, 10, 1.0, gdev)
            elif mode == "stochastic":
                O.adamw_sr_(p[s], g[s], m[s], v[s], *HP, 10, 1.0, gdev, 0x1234567, off)
            else:
                O.adamw_clip_(p[s], g[s], m[s], v[s], *HP, 10, 1.0, gdev)

    def compact(mode):
        for off, num in runs:
            s = slice(off, off + num)
            O.adamw_compact_(p[s], lo[s] if mode == "split" else None, g[s], m8[s], ms[off // 128:], v16[s], *HP, 10, 1.0, gdev, O.P_MODES[mode],
                             0x1234567, 0x7654321, off)

    arms = {}
    for mode in O.P_MODES:
        arms[f"fp32 moments, {mode}"] = (BYTES[mode][0], lambda mode=mode: fp32(mode))
        arms[f"compact moments, {mode}"] = (BYTES[mode][1], lambda mode=mode: compact(mode))
    iters = max(4, min(50, int(2e10 // n)))  # about 0.1 s of fp32-moment work per timing
    for _, fn in arms.values():  # warm every arm at this size
        fn()
    torch.cuda.synchronize()
    ms_of = {k: [] for k in arms}
    for _ in range(rounds):  # alternate the arms: whatever else the box is doing hits all of them
        for k, (_, fn) in arms.items():
            ms_of[k].append(event_ms(fn, iters))
    lines.append(f"{what}: {n} parameters in {len(runs)} launch(es) per pass, {iters} passes per timing")
    med = {k: statistics.median(t) for k, t in ms_of.items()}
    for k, (bpp, _) in arms.items():
        lines.append(f"  {k:28s} {med[k]:9.3f} ms ({min(ms_of[k]):.3f} .. {max(ms_of[k]):.3f})   {n * bpp / med[k] / 1e9:6.2f} TB/s at {bpp:.3f} B per parameter")
    slower = []
    for mode in O.P_MODES:
        a, b = med[f"fp32 moments, {mode}"], med[f"compact moments, {mode}"]
        lines.append(f"  {mode}: compact / fp32 moments = {b / a:.3f} (bytes moved: {BYTES[mode][1] / BYTES[mode][0]:.3f})")
        if b >= a:
            slower.append(mode)
    lines.append("")
    return slower


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adamw_compact_bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-arena", action="store_true", help="only the single 2^30 launch (the arena needs the 7B model built once for its run list)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this is a GPU measurement: there is no CPU fallback"
    dev = torch.device("cuda:0")
    assert O.arch_ok(0), "not a gfx950 device"
    lines = [f"AdamW on compact moments (e4m3 m with a scale byte per 128, bf16 v, stochastic stores) against fp32 moments; {torch.cuda.get_device_name(0)}",
             f"bf16 parameters, lr {HP[0]} betas {HP[1:3]} wd {HP[4]}, clip factor on the device; same build, same process, arms alternating",
             f"median of {a.rounds} rounds (min .. max); TB/s = the bytes the form has to move over the time", ""]
    slower = measure("one launch", 2 ** 30, [(0, 2 ** 30)], dev, a.rounds, lines)
    if not a.skip_arena:
        total, runs = arena_runs(dev)
        slower += measure("the 7B arena's run list", total, runs, dev, a.rounds, lines)
    if slower:
        lines.append(f"compact is NOT faster than fp32 moments for: {sorted(set(slower))}.  Likely reason: the kernel is bound by its VALU work per element (four "
                     "splitmix64 per 8 elements, the stochastic e4m3 rounding, the 16-lane maximum) and not by HBM.")
    else:
        lines.append("compact is faster than fp32 moments in every arm; where the ratio stays above the byte ratio the kernel's VALU work per element (four "
                     "splitmix64 per 8 elements, the stochastic e4m3 rounding, the 16-lane maximum) shows beside the HBM stream.")
    txt = "\n".join(lines) + "\n"
    print(txt, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
