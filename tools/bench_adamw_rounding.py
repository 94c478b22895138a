"""AdamW store policies at the optimizer's sizes: mh_adamw_clip (round to nearest, 22 B moved per parameter: p and g read, p written, m and v
read and written) against mh_adamw_split (+ lo read and written: 26 B) and mh_adamw_sr (22 B), HIP events, on the GPU box.

    python tools/bench_adamw_rounding.py [--baseline-lib PARENT/libmerlin_hip.so] [--out profiles/adamw_rounding_bench.txt]

--baseline-lib: a kernel library built from the PARENT commit; its mh_adamw_clip is the baseline line, timed in the same process, the arms
alternating.  Without it the baseline is this tree's mh_adamw_clip (the same source) and the report says so.
Criteria (the 5 % is the box-to-box and run-to-run spread of the README, with room): split <= 26/22 x baseline x 1.05, stochastic <= baseline x 1.05."""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from merlin_amd import _lib as L  # noqa: E402
from merlin_amd import ops as O  # noqa: E402

SIZES = (("one decoder layer's run", 202_383_360), ("the 7B arena", 7_050_000_000 // 128 * 128))
HP = (5e-5, 0.9, 0.95, 1e-8, 0.05)  # lr, beta1, beta2, eps, wd (pretrain.sh)


def baseline_clip(path):
    """mh_adamw_clip of another build of the library, typed by this tree's header (the prototype is the parent's too)."""
    so = C.CDLL(path)
    fn = so.mh_adamw_clip
    fn.restype, fn.argtypes = L.PROTOTYPES["mh_adamw_clip"]

    def call(p, g, m, v, gdev):
        L.check(fn(p, g, m, v, p.numel(), *HP, 10, 1.0, gdev, L.MH_BF16, torch.cuda.current_stream().cuda_stream), "baseline mh_adamw_clip")
    return call


def event_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "adamw_rounding_bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    assert O.arch_ok(0), "not a gfx950 device"
    base = baseline_clip(a.baseline_lib) if a.baseline_lib else None
    lines = [f"AdamW store policies, bf16, lr {HP[0]} wd {HP[4]}, clip factor on the device; {torch.cuda.get_device_name(0)}",
             "baseline = mh_adamw_clip of " + ("the parent commit's library (--baseline-lib), same process, arms alternating" if base else
                                               "THIS tree (no --baseline-lib given; adamw_k is the parent's source unchanged)"),
             f"median of {a.rounds} rounds (min .. max); bytes/s at 22 B per parameter (nearest, stochastic) and 26 B (split)", ""]
    verdicts = []
    for what, n in SIZES:
        p, g = torch.empty(n, dtype=torch.bfloat16, device=dev), torch.empty(n, dtype=torch.bfloat16, device=dev)
        O.fill_normal_(p, 1, 0, 0.02)
        O.fill_normal_(g, 2, 0, 0.01)
        m, v, lo = torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.int16, device=dev)
        gdev = torch.ones(1, device=dev)
        arms = {"mh_adamw_clip (this tree)": (22, lambda: O.adamw_clip_(p, g, m, v, *HP, 10, 1.0, gdev)),
                "mh_adamw_split": (26, lambda: O.adamw_split_(p, lo, g, m, v, *HP, 10, 1.0, gdev)),
                "mh_adamw_sr": (22, lambda: O.adamw_sr_(p, g, m, v, *HP, 10, 1.0, gdev, 0x1234567, 0))}
        if base:
            arms = {"mh_adamw_clip (parent commit)": (22, lambda: base(p, g, m, v, gdev)), **arms}
        iters = 20 if n < 1e9 else 4
        for _, fn in arms.values():  # warm every arm at this size
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for _ in range(a.rounds):  # alternate the arms: whatever else the box is doing hits all of them
            for k, (_, fn) in arms.items():
                ms[k].append(event_ms(fn, iters))
        lines.append(f"{what}: {n} parameters, {iters} launches per timing")
        med = {}
        for k, (bpp, _) in arms.items():
            med[k] = statistics.median(ms[k])
            lines.append(f"  {k:32s} {med[k]:9.3f} ms ({min(ms[k]):.3f} .. {max(ms[k]):.3f})   {n * bpp / med[k] / 1e9:6.2f} TB/s at {bpp} B")
        b = med[next(iter(arms))]
        for k, lim, txt in (("mh_adamw_split", b * 26 / 22 * 1.05, "26/22 x baseline x 1.05"), ("mh_adamw_sr", b * 1.05, "baseline x 1.05")):
            ok = med[k] <= lim
            verdicts.append(ok)
            lines.append(f"  criterion {k} <= {txt} = {lim:.3f} ms: {'MET' if ok else 'NOT MET'} ({med[k]:.3f} ms, {med[k] / b:.3f} x baseline)")
        lines.append("")
        del p, g, m, v, lo
        torch.cuda.empty_cache()
    lines.append("all criteria met" if all(verdicts) else "NOT all criteria met")
    txt = "\n".join(lines) + "\n"
    print(txt, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
