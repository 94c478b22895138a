"""The kernels that issue their MFMAs from inline asm: csrc/gemm_w4.hip (every 16-bit decoder GEMM, and the fp8 4-wave kernel), csrc/attn_bwd2.hip
(the default dK|dV kernel attn_bwd3_kv_k, the opt-in attn_bwd2_kv_k<MODE 3>) and csrc/attn_fwd4.hip.  hipcc inserts none of the wait states
an MFMA needs around an asm statement and is free to place register copies directly in front of / behind them (profiles/r04_attn_fwd_wave64.txt,
hazards 1-3: silent wrong results, found on hardware).  What keeps these kernels correct is where the compiler put things in THIS build, so
the listing itself is checked: tools/check_mfma_hazards.py finds no instruction that touches an asm MFMA's registers too early and no asm
MFMA that reads a register written less than two wait states before it, no scratch access sits between a kernel's first and last MFMA (a
spilled register whose load is in flight is garbage), and no kernel spills more VGPRs than its committed budget.  hipcc cross-compiles
gfx950 without a GPU."""
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "merlin_amd", "csrc")
CHECKER = os.path.join(ROOT, "tools", "check_mfma_hazards.py")

# kernels per listing: a renamed or dropped instantiation must not pass silently
KERNELS = {"gemm_w4": 42, "attn_bwd2": 42, "attn_fwd4": 4}

# .vgpr_spill_count budget of every asm-MFMA kernel, at the values of the listing this test was written against; kernels not named here: 0.
# The spills sit in the store phases, outside the K loop (the scratch-span test holds them there); the budget freezes them so that they can
# only shrink.  gemm_w4<DT, AKS, BKS, EK, MI>, gemm_w4_f8<DT, EK>: EK 0 plain / residual, 1 fp32 store, 2 fp32 accumulate, 3 RoPE,
# 4 SwiGLU, 5 SwiGLU backward.
SPILL_BUDGET = {
    "gemm_w4<0,0,0,0,8>": 8, "gemm_w4<0,0,1,0,8>": 10, "gemm_w4<0,1,0,0,8>": 10, "gemm_w4<0,1,1,0,8>": 8,
    "gemm_w4<0,0,0,2,8>": 10, "gemm_w4<0,0,0,3,8>": 6, "gemm_w4<0,0,0,4,8>": 41,
    "gemm_w4<1,0,0,0,8>": 8, "gemm_w4<1,0,1,0,8>": 10, "gemm_w4<1,1,0,0,8>": 10, "gemm_w4<1,1,1,0,8>": 8,
    "gemm_w4<1,0,0,2,8>": 10, "gemm_w4<1,0,0,3,8>": 6, "gemm_w4<1,0,0,4,8>": 41,
    "gemm_w4_f8<0,1>": 2, "gemm_w4_f8<0,3>": 10, "gemm_w4_f8<0,4>": 4, "gemm_w4_f8<0,5>": 2,
    "gemm_w4_f8<1,1>": 2, "gemm_w4_f8<1,3>": 10, "gemm_w4_f8<1,4>": 4, "gemm_w4_f8<1,5>": 2,
}


def _hipcc():
    for c in ("/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


needs_hipcc = pytest.mark.skipif(_hipcc() is None, reason="hipcc not installed")


def _checker():
    spec = importlib.util.spec_from_file_location("check_mfma_hazards", CHECKER)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    """{source stem: hipcc -S listing}, the three sources compiled at once (gemm_w4.hip alone takes minutes)."""
    from merlin_amd.csrc import build

    d = tmp_path_factory.mktemp("listings")
    procs = {}
    for stem in KERNELS:
        cmd = [_hipcc(), *build.FLAGS, "-I", CSRC, "--cuda-device-only", "-S", os.path.join(CSRC, stem + ".hip"), "-o", str(d / (stem + ".s"))]
        procs[stem] = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out = {}
    for stem, p in procs.items():
        _, err = p.communicate()
        assert p.returncode == 0, (stem, err[-2000:])
        out[stem] = (d / (stem + ".s")).read_text()
    return out


def _pretty(sym):
    """_ZN6mhgemm12_GLOBAL__N_17gemm_w4ILi0ELb0ELb0ELi4ELi8EEEvNS_8GemmArgsE -> gemm_w4<0,0,0,4,8>"""
    m = re.search(r"_GLOBAL__N_1(\d+)(\w+)", sym)
    n, rest = int(m.group(1)), m.group(2)
    args = re.match(r"I((?:L[a-z]\d+E)+)E", rest[n:])
    return rest[:n] + ("<" + ",".join(re.findall(r"L[a-z](\d+)E", args.group(1))) + ">" if args else "")


def _spills(text):
    out, cur = {}, None
    for line in text[text.index(".amdgpu_metadata"):].split("\n"):
        m = re.match(r"\s+\.symbol:\s+(\S+)\.kd$", line)
        if m:
            cur = m.group(1)
        m = re.match(r"\s+\.vgpr_spill_count:\s+(\d+)", line)
        if m:
            out[cur] = int(m.group(1))
    return out


def _asm_mfma_kernels(chk, text):
    """{readable name: (symbol, body)} of the kernels that issue at least one MFMA from inline asm."""
    return {_pretty(k): (k, body) for k, body in chk.kernels(text).items() if k and chk.asm_mfmas(body)}


@needs_hipcc
@pytest.mark.parametrize("stem", sorted(KERNELS))
def test_listing_has_the_expected_kernels(listings, stem):
    chk = _checker()
    kernels = [k for k in chk.kernels(listings[stem]) if k]
    assert len(kernels) == len(set(kernels)) == KERNELS[stem], [_pretty(k) for k in kernels]
    if stem == "attn_fwd4":
        assert len([k for k in kernels if "attn_fwd4_k" in k]) == 4, kernels  # bf16 / fp16 x causal / full
    for name in SPILL_BUDGET:
        assert stem != "gemm_w4" or name in _asm_mfma_kernels(chk, listings[stem]), f"spill budget names {name}, which the listing lacks"


@needs_hipcc
@pytest.mark.parametrize("stem", sorted(KERNELS))
def test_asm_mfma_kernels_have_no_hazards(listings, stem):
    chk = _checker()
    ks = _asm_mfma_kernels(chk, listings[stem])
    assert ks
    bad = [f"{name}: {h}" for name, (_, body) in ks.items() for h in chk.check(body)[:4]]
    assert not bad, "\n".join(bad)


@needs_hipcc
@pytest.mark.parametrize("stem", sorted(KERNELS))
def test_asm_mfma_kernels_keep_scratch_out_of_the_mfma_span_and_spills_within_budget(listings, stem):
    chk = _checker()
    text = listings[stem]
    spills = _spills(text)
    ks = _asm_mfma_kernels(chk, text)
    in_span, over = {}, {}
    for name, (sym, body) in ks.items():
        mf = [i for i, (_, raw, _) in enumerate(body) if (chk.parse(raw) or ("",))[0].startswith("v_mfma")]
        scr = [ln for ln, raw, _ in body[mf[0]:mf[-1] + 1] if re.search(r"\bscratch_(load|store)", raw.split(";")[0])]
        if scr:
            in_span[name] = scr[:4]
        if spills[sym] > SPILL_BUDGET.get(name, 0):
            over[name] = (spills[sym], SPILL_BUDGET.get(name, 0))
    assert not in_span, in_span
    assert not over, over  # (spill count, budget)


@needs_hipcc
def test_attn_fwd4_listing_has_no_spills_and_no_mfma_hazards(listings, tmp_path):
    text = listings["attn_fwd4"]
    kernels = re.findall(r"^(_ZN6mhattn\S*attn_fwd4_k\S*):", text, flags=re.M)
    assert len(set(kernels)) == 4, kernels  # bf16 / fp16 x causal / full
    spills = [int(x) for x in re.findall(r"\.vgpr_spill_count:\s*(\d+)", text)]
    assert spills and max(spills) == 0, spills
    assert "scratch_load" not in text and "scratch_store" not in text
    listing = tmp_path / "attn_fwd4.s"  # the command line on the raw listing
    listing.write_text(text)
    for k in sorted(set(kernels)):
        c = subprocess.run([sys.executable, CHECKER, str(listing), k], capture_output=True, text=True)
        assert c.returncode == 0, c.stderr
        assert c.stdout.strip().endswith("hazards: 0"), (k, c.stdout[-1500:])


def _run(tmp_path, listing, sel="_Zk"):
    f = tmp_path / "t.s"
    f.write_text(listing)
    return subprocess.run([sys.executable, CHECKER, str(f), sel], capture_output=True, text=True)


def _asm(*lines):
    return "".join(f"\t;;#ASMSTART\n\t{x}\n\t;;#ASMEND\n" for x in lines)


MFMA = "v_mfma_f32_32x32x16_bf16"


def test_hazard_checker_sees_a_stale_read_and_a_late_write(tmp_path):
    """The checker itself: an accumulator copied directly behind its MFMA, and an AccVGPR written directly in front of the MFMA that reads it."""
    chk = os.path.join(ROOT, "tools", "check_mfma_hazards.py")
    bad = tmp_path / "bad.s"
    bad.write_text("_Zk:\n\tv_mfma_f32_32x32x16_bf16 a[0:15], v[0:3], v[4:7], a[0:15]\n\tv_accvgpr_read_b32 v9, a3\n"
                   "\tv_accvgpr_write_b32 a20, v1\n\tv_mfma_f32_32x32x16_bf16 v[16:31], a[20:23], v[4:7], 0\n\ts_endpgm\n")
    c = subprocess.run([sys.executable, chk, str(bad), "_Zk"], capture_output=True, text=True)
    assert c.stdout.strip().endswith("hazards: 2"), c.stdout
    good = tmp_path / "good.s"
    good.write_text("_Zk:\n\tv_mfma_f32_32x32x16_bf16 a[0:15], v[0:3], v[4:7], a[0:15]\n\ts_nop 15\n\ts_nop 3\n\tv_accvgpr_read_b32 v9, a3\n"
                    "\tv_accvgpr_write_b32 a20, v1\n\ts_nop 1\n\tv_mfma_f32_32x32x16_bf16 v[16:31], a[20:23], v[4:7], 0\n\ts_endpgm\n")
    c = subprocess.run([sys.executable, chk, str(good), "_Zk"], capture_output=True, text=True)
    assert c.stdout.strip().endswith("hazards: 0"), c.stdout
    c = subprocess.run([sys.executable, chk, str(good), "_Znope"], capture_output=True, text=True)
    assert c.returncode == 2


def test_hazard_checker_rules_for_writes_branches_and_compiler_mfmas(tmp_path):
    """One seeded bad and one good listing per rule: write-after-write on an in-flight MFMA's destination, write-after-read of its C
    operand, a hazard across a loop's back edge, one across a forward branch, and the MFMAs hipcc schedules itself (padded by hipcc) ignored."""
    cases = {
        # an accvgpr write one MFMA behind the MFMA that still writes that register
        "waw": (_asm(f"{MFMA} a[0:15], v[0:3], v[4:7], 0", f"{MFMA} a[32:47], v[0:3], v[4:7], 0") + "\tv_accvgpr_write_b32 a3, v1\n",
                _asm(f"{MFMA} a[0:15], v[0:3], v[4:7], 0", f"{MFMA} a[32:47], v[0:3], v[4:7], 0", f"{MFMA} a[48:63], v[0:3], v[4:7], 0")
                + "\tv_accvgpr_write_b32 a3, v1\n"),
        # a VALU write to a register the MFMA in flight reads as C
        "war": (_asm(f"{MFMA} a[0:15], v[0:3], v[4:7], a[16:31]") + "\tv_accvgpr_write_b32 a20, v1\n",
                _asm(f"{MFMA} a[0:15], v[0:3], v[4:7], a[16:31]") + "\ts_nop 15\n\ts_nop 3\n\tv_accvgpr_write_b32 a20, v1\n"),
        # the loop's last MFMA against the copy at the loop head, reached only through the back edge
        "back edge": ("\ts_mov_b32 s0, 0\n.LBB0_1:\n\tv_accvgpr_read_b32 v9, a3\n\ts_nop 15\n\ts_nop 3\n"
                      + _asm(f"{MFMA} a[0:15], v[0:3], v[4:7], a[0:15]") + "\ts_add_u32 s0, s0, 1\n\ts_cmp_lt_u32 s0, 4\n\ts_cbranch_scc1 .LBB0_1\n",
                      "\ts_mov_b32 s0, 0\n.LBB0_1:\n\tv_accvgpr_read_b32 v9, a3\n\ts_nop 15\n\ts_nop 3\n"
                      + _asm(f"{MFMA} a[0:15], v[0:3], v[4:7], a[0:15]", "s_nop 15\n\ts_nop 3")
                      + "\ts_add_u32 s0, s0, 1\n\ts_cmp_lt_u32 s0, 4\n\ts_cbranch_scc1 .LBB0_1\n"),
        # the loop exit through an unconditional forward branch: the copy at its target still sees the MFMA in flight
        "forward branch": (_asm(f"{MFMA} a[0:15], v[0:3], v[4:7], a[0:15]") + "\ts_branch .LBB0_3\n.LBB0_2:\n\ts_nop 15\n\ts_nop 15\n"
                           ".LBB0_3:\n\tv_accvgpr_read_b32 v9, a3\n",
                           _asm(f"{MFMA} a[0:15], v[0:3], v[4:7], a[0:15]", "s_nop 15\n\ts_nop 3") + "\ts_branch .LBB0_3\n.LBB0_2:\n"
                           "\ts_nop 15\n\ts_nop 15\n.LBB0_3:\n\tv_accvgpr_read_b32 v9, a3\n"),
        # the same copy behind an MFMA that hipcc scheduled itself: the bad form is the asm MFMA, the good one the compiler's in a kernel
        # that has asm statements (in one without any, e.g. a listing stripped of its markers, every MFMA is checked: the test above)
        "asm only": (_asm(f"{MFMA} a[0:15], v[0:3], v[4:7], a[0:15]") + "\tv_accvgpr_read_b32 v9, a3\n",
                     _asm("s_waitcnt lgkmcnt(0)") + f"\t{MFMA} a[0:15], v[0:3], v[4:7], a[0:15]\n\ts_nop 7\n\tv_accvgpr_read_b32 v9, a3\n"),
    }
    for rule, (bad, good) in cases.items():
        c = _run(tmp_path, "_Zk:\n" + bad + "\ts_endpgm\n")
        assert c.stdout.strip().endswith("hazards: 1"), (rule, c.stdout)
        c = _run(tmp_path, "_Zk:\n" + good + "\ts_endpgm\n")
        assert c.stdout.strip().endswith("hazards: 0"), (rule, c.stdout)
