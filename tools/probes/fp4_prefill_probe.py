"""What generate(fp4_prefill=True) costs: ops.gemm_fp4w against ops.gemm_nt on the four decoder projections of the 7B geometry, and the whole
prefill of the cfg 2 prompt (one 336-px image + text, S = 613) on the MXFP4 copies against the 16-bit weights.  Run on the GPU box:

    python tools/probes/fp4_prefill_probe.py [--layers 32] [--no-prefill]

Both arms of a comparison alternate in this process (measuring rule: same box, same run); per arm the median of ROUNDS windows of ITERS
launches between two device events, after warm-up.  Operands ~ N(0, 1)-scaled like activations and weights (the clocks depend on the bits).
gemm_nt is timed with the epilogue the 16-bit layer fuses there (RoPE / residual / SwiGLU); the fp4 arm adds the separate rope_qk_ / swiglu_fwd
launch it needs, so a row is one projection as the layer runs it.  Ratios inside the box spread of +- 2 % (profiles/README.md) print as "equal"."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from merlin_amd import ops as O

dev = torch.device("cuda:0")
dt = torch.bfloat16
d, ff, H, D = 4096, 11008, 32, 128
ROUNDS, ITERS = 7, 100
LAYERS = int(sys.argv[sys.argv.index("--layers") + 1]) if "--layers" in sys.argv else 32


def rnd(*s, scale=1.0):
    return (torch.randn(*s, device=dev) * scale).to(dt)


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def ab(fa, fb, iters=ITERS):
    """Median ms of the two arms, alternating A B A B ..."""
    for _ in range(2):
        fa(), fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(window(fa, iters))
        tb.append(window(fb, iters))
    return statistics.median(ta), statistics.median(tb)


def verdict(r):
    return "equal" if abs(r - 1.0) <= 0.02 else f"x {r:.2f}"


def projections():
    wqkv, wo, wgu, wd = rnd(3 * d, d, scale=0.02), rnd(d, d, scale=0.02), rnd(2 * ff, d, scale=0.02), rnd(d, ff, scale=0.02)
    q = {k: O.quant_fp4_b32(w) for k, w in dict(wqkv=wqkv, wo=wo, wgu=wgu, wd=wd).items()}
    for M in (613, 4096):
        x, xf, resid = rnd(M, d), rnd(M, ff), rnd(M, d)
        x32 = resid.float()
        rope = O.rope_table(M, D, 10000.0, dev)
        rows = [
            ("q|k|v + RoPE", 3 * d, d, lambda: O.gemm_nt_rope(x, wqkv, rope, M, H, D), lambda: O.rope_qk_(O.gemm_fp4w(x, q["wqkv"]), rope, M, H, D)),
            ("o + fp32 stream", d, d, lambda: O.gemm_nt(x, wo, out=x32, accum=True), lambda: O.gemm_fp4w(x, q["wo"], out=x32, accum=True)),
            ("gate|up + SwiGLU", 2 * ff, d, lambda: O.gemm_swiglu_fwd(x, wgu), lambda: O.swiglu_fwd(O.gemm_fp4w(x, q["wgu"]))),
            ("down + fp32 stream", d, ff, lambda: O.gemm_nt(xf, wd, out=x32, accum=True), lambda: O.gemm_fp4w(xf, q["wd"], out=x32, accum=True)),
            ("o, 16-bit + resid", d, d, lambda: O.gemm_nt(x, wo, resid=resid), lambda: O.gemm_fp4w(x, q["wo"], resid=resid)),
            ("q|k|v, GEMM alone", 3 * d, d, lambda: O.gemm_nt(x, wqkv), lambda: O.gemm_fp4w(x, q["wqkv"])),
        ]
        for name, N, K, f16, f4 in rows:
            t16, t4 = ab(f16, f4)
            fl = 2.0 * M * N * K
            print(json.dumps({"projection": name, "M": M, "N": N, "K": K, "gemm_nt_ms": round(t16, 4), "gemm_fp4w_ms": round(t4, 4),
                              "gemm_nt_tflops": round(fl / t16 / 1e9, 1), "gemm_fp4w_tflops": round(fl / t4 / 1e9, 1), "fp4_over_16bit": verdict(t4 / t16)}), flush=True)


def prefill():
    from merlin_amd import synth
    from merlin_amd.model.llama_mmgpt import build_synthetic_model

    llama = dict(vocab_size=32000, hidden_size=d, intermediate_size=ff, num_hidden_layers=LAYERS, num_attention_heads=H, rms_norm_eps=1e-6,
                 rope_theta=10000.0, max_position_embeddings=8192)
    vision = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=336, patch_size=14, layer_norm_eps=1e-5)
    model = build_synthetic_model(llama, vision, projector="mlp", conv_stride=1, dtype=dt, device="cuda", seed=0)
    batch = synth.single_image_batch()
    ids, images = batch["input_ids"].to(dev), [im.to(dev) for im in batch["images"]]
    eng = model.engine
    with torch.no_grad():
        eng.quantize_decode_weights_fp4()
        t16, t4 = ab(lambda: eng.prefill(ids, None, images, 8), lambda: eng.prefill(ids, None, images, 8, w_fp4=True), iters=10)
    print(json.dumps({"prefill": "cfg 2 prompt, tower included", "S": int(ids.shape[1]), "layers": LAYERS, "ms_16bit": round(t16, 3), "ms_fp4": round(t4, 3),
                      "fp4_over_16bit": verdict(t4 / t16)}), flush=True)


if __name__ == "__main__":
    assert O.arch_ok(0), "not a gfx950 device"
    projections()
    if "--no-prefill" not in sys.argv:
        prefill()
