"""Launch trace + output hashes of the engine, scenario by scenario: the yardstick for host-side refactors of model/engine.py
("the same launches in the same order with the same arguments, the same bits out").  Uses the public surface only, so the same
file runs on two commits; compare the outputs with diff.

    python tools/engine_trace.py --list                     scenario names, one per line
    python tools/engine_trace.py [--detail FILE] NAME...    the scenarios, a fresh model each -> summary lines on stdout

Per scenario: `launches N sha256(list)` - the list holds each C ABI call's symbol and its scalar (non-pointer) arguments in order,
recorded by wrapping merlin_amd._lib.launch, through which every call goes - and `out NAME sha256` for the loss, the logits and all
param.grad together (generate: the token ids).  FILE receives the list itself and one hash per gradient tensor, for finding a
difference.  Run each call under its own time limit."""
import hashlib
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from merlin_amd import _lib as L  # noqa: E402

DT = torch.bfloat16
S = {}  # name -> (kind, case, engine options, model options)
for case in ("tiny_2img", "tiny_padbatch", "tiny_textonly", "tiny_conv2", "medium_cfg1"):
    for r32 in (True, False):
        for save in ((True, False) if case.startswith("tiny") else (False,)):
            S[f"train/{case}/r32={int(r32)}/save={int(save)}"] = ("train", case, dict(fp32_residual=r32, save_activations=save), {})
for r32 in (True, False):
    for lvl in (1, 2):
        S[f"train/tiny_2img/r32={int(r32)}/mem_level={lvl}"] = ("train", "tiny_2img", dict(fp32_residual=r32, save_activations=True, mem_level=lvl), {})
for save in (True, False):
    S[f"train/tiny_padbatch/force_unpad/save={int(save)}"] = ("train", "tiny_padbatch", dict(force_unpad=True, save_activations=save), {})
    S[f"train/leftpad/save={int(save)}"] = ("train", "leftpad", dict(save_activations=save), {})
    S[f"fp8train/tiny_2img/head=1/save={int(save)}"] = ("train", "tiny_2img", dict(fp8_tower=True, fp8_head=True, save_activations=save), dict(fp8_training=True))
for sparse in (True, False):  # labels on the trajectory tails only: 988 scored rows of 2048
    S[f"train/interpair/sparse={int(sparse)}"] = ("train", "interpair", dict(sparse_head=sparse, sparse_last_layer=sparse), {})
S["fp8train/tiny_2img/head=0/save=0"] = ("train", "tiny_2img", dict(fp8_tower=True, fp8_head=False), dict(fp8_training=True))
S["fp8train/medium_cfg1/head=1/save=0"] = ("train", "medium_cfg1", dict(fp8_tower=True, fp8_head=True), dict(fp8_training=True))
S["fp8forward/tiny_2img"] = ("forward", "tiny_2img", {}, dict(fp8_forward=True))
for fp8w in (False, True):
    S[f"generate/tiny_2img/fp8w={int(fp8w)}"] = ("generate", "tiny_2img", {}, dict(fp8_weights=fp8w))
    S[f"generate/leftpad/fp8w={int(fp8w)}"] = ("generate", "leftpad", {}, dict(fp8_weights=fp8w))


def get_case(name):
    from merlin_amd import synth
    from oracle import cases as C

    if name == "interpair":
        cfg = C.tiny_cfg()
        return cfg, synth.interpair_batch(B=4, S=512, frames=12, base_vocab=cfg.vocab_size - 3, P=cfg.num_patches, image_size=cfg.v_image_size)
    cfg, b = C.get_case("tiny_padbatch" if name == "leftpad" else name)
    if name == "leftpad":  # every row's valid tokens moved to the end; the first valid token is predicted from a pad row: not scored
        b = dict(b, input_ids=b["input_ids"].clone(), labels=b["labels"].clone(), attention_mask=b["attention_mask"].clone().bool())
        for k in range(b["input_ids"].shape[0]):
            n = int(b["attention_mask"][k].sum())
            for key in ("input_ids", "labels", "attention_mask"):
                b[key][k] = torch.cat([b[key][k, n:], b[key][k, :n]])
            b["labels"][k, -n] = -100
    return cfg, b


def sha(t):
    return hashlib.sha256(t.detach().reshape(-1).cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def run(name, detail_file=None):
    kind, case, eopts, mopts = S[name]
    cfg, b = get_case(case)
    from test_model_gpu import _build  # the tests' model: build_synthetic_model(seed=0) at the case's geometry

    model = _build(cfg, DT)
    for k, v in eopts.items():
        assert hasattr(model.engine, k), k
        setattr(model.engine, k, v)
    inputs = dict(input_ids=b["input_ids"].cuda(), attention_mask=b["attention_mask"].cuda(), images=[im.cuda() for im in b["images"]])
    trace, real, outs = [], L.launch, {}

    def traced(sym, *args):
        scal = [a for a, t in zip(args, L.PROTOTYPES[sym][1]) if t is not L.DevPtr]
        trace.append(sym + "".join(f" {a!r}" for a in scal))
        return real(sym, *args)

    L.launch = traced
    try:
        if kind == "generate":
            outs["tokens"] = model.generate(**inputs, max_new_tokens=6, use_graph=False, eos_token_id=-1, pad_token_id=0, **mopts)
        else:
            for k, v in mopts.items():
                setattr(model, k, v)
            with torch.enable_grad() if kind == "train" else torch.no_grad():
                out = model(**inputs, labels=b["labels"].cuda())
                if kind == "train":
                    out.loss.backward()
            outs.update(loss=out.loss, logits=out.logits)
            outs.update({"grad/" + k: p.grad for k, p in model.named_parameters() if p.grad is not None})
            if mopts:
                print(f"[{name}] last_fp8 {getattr(model.engine, 'last_fp8', None)}")
        torch.cuda.synchronize()
    finally:
        L.launch = real
    print(f"[{name}] launches {len(trace)} {hashlib.sha256(chr(10).join(trace).encode()).hexdigest()}")
    grads = [f"{k} {sha(v)}" for k, v in outs.items() if k.startswith("grad/")]
    for k, v in outs.items():
        if not k.startswith("grad/"):
            print(f"[{name}] out {k} {sha(v)}")
    if grads:
        print(f"[{name}] out grads({len(grads)}) {hashlib.sha256(chr(10).join(grads).encode()).hexdigest()}")
    if detail_file:
        with open(detail_file, "a") as f:
            f.writelines(f"[{name}] {t}\n" for t in trace + grads)


if __name__ == "__main__":
    if sys.argv[1:] == ["--list"]:
        print("\n".join(S))
    else:
        names, out_file = (sys.argv[3:], sys.argv[2]) if sys.argv[1] == "--detail" else (sys.argv[1:], None)
        for n in names:
            run(n, out_file)
