"""CPU-side checks of the drop-in boundary: the C-ABI library builds/loads and exports every symbol
that include/merlin_hip.h declares (no compute calls: there is no GPU here)."""
import os

import pytest


def test_library_exports_every_declared_symbol():
    from merlin_amd import _lib as L

    if not os.path.exists(L.LIB_PATH):
        from merlin_amd.csrc import build

        build.build(verbose=False)
    lib = L.lib()
    names = L.declared_symbols()
    assert len(names) >= 30, names
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, f"declared in include/merlin_hip.h but not exported: {missing}"
    assert lib.mh_version() >= 100
    assert b"dtype" in lib.mh_strerror(-2)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from merlin_amd import _lib as L

    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(L.MerlinHipError):
        L.lib()


def test_product_never_imports_oracle():
    """The HIP path must not route through the CPU oracle (or any CPU fallback)."""
    import pathlib
    import re

    root = pathlib.Path(__file__).resolve().parents[1] / "merlin_amd"
    bad = []
    for f in root.rglob("*.py"):
        txt = f.read_text()
        if re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M):
            bad.append(str(f))
    assert not bad, bad


def test_host_side_launch_plans():
    """Host-only entry points (no launch): the split counts mh_gemm_splitk_max hands the skinny-GEMM path of ops.gemm_nt and the
    split-KV count of the decode attention."""
    import ctypes as C

    from merlin_amd import _lib as L

    lib = L.lib()
    sk = lambda M, N, K: int(lib.mh_gemm_splitk_max(C.c_int(M), C.c_int(N), C.c_int(K)))  # noqa: E731
    assert sk(613, 4096, 4096) == 5 and sk(613, 4096, 11008) == 5   # o / down projections of one 613-token sequence: 48 tiles
    assert sk(613, 12288, 4096) == 1 and sk(613, 22016, 4096) == 1   # q|k|v and gate|up fill the chip on their own
    assert sk(32768, 4096, 4096) == 1                                # the headline shapes never split
    assert sk(613, 4096, 512) == 1                                   # short contractions are not worth the reduce pass
    for M, N, K in ((577, 1024, 4096), (40, 4096, 12288), (1000, 1032, 2048)):
        s = sk(M, N, K)
        nk = (K + 63) // 64
        assert 1 < s <= 16 and (s - 1) * ((nk + s - 1) // s) < nk, (M, N, K, s)  # no empty split
    assert int(lib.mh_attn_decode_splits(C.c_int(1), C.c_int(32), C.c_int(4096))) == 32
    assert int(lib.mh_attn_decode_splits(C.c_int(8), C.c_int(32), C.c_int(4096))) == 4


def test_grouped_wgrad_host_plan_and_struct_layout():
    """Host side of mh_wgrad_grouped: the launch-plan predicate (a CLIP-L layer's four weight gradients over 27 696 tokens are grouped, the tiny
    test models' are not, odd widths never) and the ctypes mirror of `MhWgradProblem` (include/merlin_hip.h) - 3 pointers + 3 strides + 4 ints."""
    import ctypes as C

    from merlin_amd import ops as O

    vd, vff = 1024, 4096
    assert O.wgrad_group_pays(48 * 577, [(vd, vff), (vff, vd), (vd, vd), (3 * vd, vd)])
    assert not O.wgrad_group_pays(3 * 17, [(128, 256), (256, 128), (128, 128), (384, 128)])       # tiny fixture: a few tiles, a few tokens
    assert not O.wgrad_group_pays(48 * 577, [(vd, vff), (vff, vd), (vd, vd), (3 * vd, vd + 4)])  # a width the kernel cannot take
    assert not O.wgrad_group_pays(48 * 577, [(vd, vff)] * 9)                                      # more problems than one launch holds
    assert C.sizeof(O._WgradProblem) == 64
    assert [f[0] for f in O._WgradProblem._fields_] == ["dy", "lddy", "x", "ldx", "out", "ldo", "M", "N", "accumulate", "reserved"]


def test_every_declared_symbol_is_typed_from_the_header():
    import ctypes as C

    from merlin_amd import _lib as L

    lib = L.lib()
    assert sorted(L.PROTOTYPES) == L.declared_symbols() and len(L.PROTOTYPES) == len(L.declared_symbols())
    for name, (restype, argtypes) in L.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    n_args = lambda name: len(getattr(lib, name).argtypes)  # noqa: E731
    assert n_args("mh_version") == 0 and n_args("mh_attn_bwd2_spill") == 28 and n_args("mh_gemm") == 17
    assert lib.mh_gemm.argtypes[1] is C.c_int64 and lib.mh_gemm.argtypes[2] is C.c_int and lib.mh_gemm.argtypes[-1] is L.DevPtr
    assert lib.mh_fill_normal.argtypes[2] is C.c_uint64 and lib.mh_fill_normal.argtypes[4] is C.c_float
    assert lib.mh_gemm.restype is C.c_int and lib.mh_strerror.restype is C.c_char_p and lib.mh_gemm_persistent.restype is None
    assert lib.mh_attn_bwd_spill_bytes.restype is C.c_int64


def test_64_bit_return_value_needs_no_patch():
    """cfg 5 (B 4, S 8192, H 32): n = S / 128 = 64, n^2 + n units of 16 384 bytes per (batch, head) (csrc/attn_bwd2.hip ds_units_per_bh);
    read as a C int the value would be 134 217 728."""
    from merlin_amd import _lib as L

    need = L.lib().mh_attn_bwd_spill_bytes(4, 8192, 32)
    assert need == 4 * 32 * (64 * 64 + 64) * 16384 == 8724152320 and need > 2 ** 32


def test_call_checks_count_and_types_before_the_library_is_entered():
    """None of these may reach the kernel library: a launch with a wrong argument list would run with a garbage pointer or size."""
    import ctypes as C

    from merlin_amd import _lib as L

    L.lib()
    assert len(L.PROTOTYPES["mh_p32_rmsnorm"][1]) == 7  # (x, w, y, rows, d, eps, stream)
    with pytest.raises(TypeError, match="takes 7 arguments, got 6"):
        L.call("mh_p32_rmsnorm", None, None, None, 4, 16, 1e-5)
    with pytest.raises(TypeError, match="takes 7 arguments, got 8"):
        L.call("mh_p32_rmsnorm", None, None, None, 4, 16, 1e-5, None, None)
    with pytest.raises(C.ArgumentError):
        L.call("mh_p32_rmsnorm", None, None, None, 4.0, 16, 1e-5, None)   # a float where the prototype says int
    with pytest.raises(C.ArgumentError):
        L.call("mh_p32_rmsnorm", 1.5, None, None, 4, 16, 1e-5, None)      # neither a tensor, None, an address nor a ctypes pointer
    with pytest.raises(KeyError):
        L.call("mh_no_such_function")

    class T:  # what the pointer type takes: tensors by data_ptr(), None, addresses, ctypes pointer values and arrays
        def data_ptr(self):
            return 0x7F0012345678

    assert L.DevPtr.from_param(T()).value == 0x7F0012345678 and L.DevPtr.from_param(None) is None
    assert L.DevPtr.from_param(1 << 40).value == 1 << 40
    v, arr = C.c_void_p(5), (C.c_int64 * 2)()
    assert L.DevPtr.from_param(v) is v and L.DevPtr.from_param(arr) is arr


def test_missing_header_fails_loudly(tmp_path):
    from merlin_amd import _lib as L

    with pytest.raises(L.MerlinHipError):
        L._parse_header(str(tmp_path / "nope.h"))
    bad = tmp_path / "bad.h"
    bad.write_text("int mh_ok(int a, void* stream);\nint mh_odd(size_t n, void* stream);\n")
    with pytest.raises(L.MerlinHipError, match="size_t"):  # an unknown C type is an error, not a skipped entry
        L._parse_header(str(bad))
    bad.write_text("int mh_ok(int a, void* stream);\nunsigned mh_odd(int n);\n")
    with pytest.raises(L.MerlinHipError, match="mh_odd"):  # so is a prototype the pattern cannot read
        L._parse_header(str(bad))


def test_constants_equal_the_headers_defines():
    import re

    from merlin_amd import _lib as L
    from merlin_amd import ops as O

    d = {k: int(v.strip("()")) for k, v in re.findall(r"#define\s+(MH_\w+)\s+(\(?-?\d+\)?)", open(L.HEADER).read())}
    assert (L.MH_BF16, L.MH_F16, L.MH_F32) == (d["MH_BF16"], d["MH_F16"], d["MH_F32"]) == (0, 1, 2)
    got = (O.EPI_BIAS, O.EPI_QUICK_GELU, O.EPI_RESIDUAL, O.EPI_ACCUM, O.EPI_OUT_F32)
    assert got == (L.EPI_BIAS, L.EPI_QUICK_GELU, L.EPI_RESIDUAL, L.EPI_ACCUM, L.EPI_OUT_F32)
    assert got == tuple(d["MH_EPI_" + k] for k in ("BIAS", "QUICK_GELU", "RESIDUAL", "ACCUM", "OUT_F32")) == (1, 2, 4, 8, 16)


def test_every_call_site_in_the_package_matches_its_prototype():
    """Static pass over merlin_amd/**/*.py: every L.call / L.launch names a declared symbol with the prototype's argument count, and no
    launch function (last parameter `void* stream`) is called as an attribute of lib(), past the count check."""
    import ast
    import pathlib
    import re

    from merlin_amd import _lib as L

    hdr = re.sub(r"/\*.*?\*/", "", open(L.HEADER).read(), flags=re.S)
    launches = set(re.findall(r"\b(mh_\w+)\s*\([^()]*\bvoid\s*\*\s*stream\s*\)", hdr))
    assert len(launches) > 80 and launches < set(L.PROTOTYPES) and all(L.PROTOTYPES[n][0] is L.C.c_int for n in launches)
    sites, bad = 0, []
    for f in (pathlib.Path(__file__).resolve().parents[1] / "merlin_amd").rglob("*.py"):
        for node in ast.walk(ast.parse(f.read_text())):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)):
                continue
            where = f"{f.name}:{node.lineno}"
            if node.func.attr in ("call", "launch") and isinstance(node.func.value, ast.Name) and node.func.value.id == "L":
                name = node.args[0].value if node.args and isinstance(node.args[0], ast.Constant) else None
                sites += 1
                if name not in L.PROTOTYPES:
                    bad.append(f"{where}: {name!r} is not declared (the name must be a literal)")
                elif any(isinstance(a, ast.Starred) for a in node.args) or node.keywords:
                    bad.append(f"{where}: {name}: starred / keyword arguments cannot be counted")
                elif len(node.args) - 1 != len(L.PROTOTYPES[name][1]):
                    bad.append(f"{where}: {name} takes {len(L.PROTOTYPES[name][1])} arguments, {len(node.args) - 1} passed")
            elif node.func.attr in launches:
                bad.append(f"{where}: {node.func.attr} launched without L.call")
            elif node.func.attr.startswith("mh_") and len(node.args) != len(L.PROTOTYPES.get(node.func.attr, (None, node.args))[1]):
                bad.append(f"{where}: {node.func.attr}: {len(node.args)} arguments passed")
    assert not bad, "\n".join(bad)
    assert sites >= 80, sites


# Launch symbols no `ops.` function wraps: the fp32-store parity kernels, launched by merlin_amd/parity.py when engine.parity_fp32 is set.
# Per-kernel tests of them are out of scope; each is named with the GPU test that runs it (tiny_conv2 is the fixture with a conv projector).
REACHED_ONLY_THROUGH_THE_ENGINE = {
    "mh_p32_split3": "tests.test_parity_mode_gpu::test_parity_mode_tiny",
    "mh_p32_rmsnorm": "tests.test_parity_mode_gpu::test_parity_mode_tiny",
    "mh_p32_layernorm": "tests.test_parity_mode_gpu::test_parity_mode_tiny",
    "mh_p32_elementwise": "tests.test_parity_mode_gpu::test_parity_mode_tiny",
    "mh_p32_rope": "tests.test_parity_mode_gpu::test_parity_mode_tiny",
    "mh_p32_embed_splice": "tests.test_parity_mode_gpu::test_parity_mode_tiny",
    "mh_p32_im2col": "tests.test_parity_mode_gpu::test_parity_mode_tiny",
    "mh_p32_vit_assemble": "tests.test_parity_mode_gpu::test_parity_mode_tiny",
    "mh_p32_conv3x3_cols": "tests.test_parity_mode_gpu::test_parity_mode_tiny",
    "mh_p32_attention": "tests.test_parity_mode_gpu::test_parity_mode_at_benchmark_sequence_lengths",
}


def test_every_launch_symbol_is_reached_by_a_gpu_test():
    """Static pass: every launch symbol of include/merlin_hip.h (last parameter `void* stream`) is named by an `ops.` function that some GPU
    test file calls (through the functions of ops.py that function calls, e.g. colsum -> reduce_partials), or by a literal L.call in such a
    file; the only exceptions are listed above by name.  A new entry point without a GPU test fails here."""
    import ast
    import pathlib
    import re

    from merlin_amd import _lib as L
    from merlin_amd import ops as O

    root = pathlib.Path(__file__).resolve().parents[1]
    hdr = re.sub(r"/\*.*?\*/", "", open(L.HEADER).read(), flags=re.S)
    launches = set(re.findall(r"\b(mh_\w+)\s*\([^()]*\bvoid\s*\*\s*stream\s*\)", hdr))
    assert len(launches) > 80

    def literals(node):
        return {n.args[0].value for n in ast.walk(node) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr in ("call", "launch")
                and isinstance(n.func.value, ast.Name) and n.func.value.id == "L" and n.args and isinstance(n.args[0], ast.Constant)}

    fns = {}
    for node in ast.parse((root / "merlin_amd" / "ops.py").read_text()).body:
        if isinstance(node, ast.FunctionDef):
            fns[node.name] = (literals(node), {n.func.id for n in ast.walk(node) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name)})

    def reach(name, seen):
        if name in seen or name not in fns:
            return set()
        seen.add(name)
        return set(fns[name][0]).union(*(reach(c, seen) for c in fns[name][1]))

    reached, files = set(), 0
    for f in sorted((root / "tests").glob("test_*.py")):
        txt = f.read_text()
        if not re.search(r"^(pytestmark = |@)pytest\.mark\.gpu", txt, flags=re.M):
            continue
        files += 1
        tree = ast.parse(txt)
        reached |= literals(tree)
        for n in ast.walk(tree):
            if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id in ("ops", "O"):
                reached |= reach(n.attr, set())
    assert files >= 10
    unreached = launches - reached
    assert unreached == set(REACHED_ONLY_THROUGH_THE_ENGINE), (sorted(unreached - set(REACHED_ONLY_THROUGH_THE_ENGINE)), sorted(set(REACHED_ONLY_THROUGH_THE_ENGINE) - unreached))
    parity = (root / "merlin_amd" / "parity.py").read_text()
    for sym, test in REACHED_ONLY_THROUGH_THE_ENGINE.items():
        mod, fn = test.split("::")
        assert f'"{sym}"' in parity, sym
        src = (root / (mod.replace(".", "/") + ".py")).read_text()
        assert f"def {fn}(" in src, test
    # the A/B setters are host-only (each stores one int) and typed from the header like every other symbol; the reachability pass above has
    # already shown that tests/test_entry_points_gpu.py calls the wrappers of the arms documented as bit-identical
    for fn in ("gemm_persistent", "gemm_raster_group", "attn_wide_stores"):
        assert fn in fns and not fns[fn][0], fn  # (a setter launches nothing)
    used = {n.attr for n in ast.walk(ast.parse((root / "tests" / "test_entry_points_gpu.py").read_text()))
            if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == "ops"}
    assert {"gemm_persistent", "gemm_raster_group", "attn_wide_stores"} <= used
    assert O.gemm_persistent(True) is None
    assert O.gemv_ksplit(True) is None and O.gemm_w4_policy(11) is None and O.gemm_raster_group(0) is None
    with pytest.raises(Exception, match="argument 1"):
        O.gemm_raster_group(2.5)
