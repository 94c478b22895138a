"""ctypes binding of libmerlin_hip.so, typed from include/merlin_hip.h: the header is the only table of prototypes and constants.
Fails loudly when the library or the header is missing: there is NO CPU / eager fallback for the product path."""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# MH_LIB_PATH: kernel-development override (tools/dev_arms/libmerlin_hip_dev.so = product kernels + A/B arms)
LIB_PATH = os.environ.get("MH_LIB_PATH") or os.path.join(_HERE, "csrc", "libmerlin_hip.so")
HEADER = os.path.join(_HERE, "..", "include", "merlin_hip.h")

_lib = None


class MerlinHipError(RuntimeError):
    pass


class DevPtr:
    """Parameter type of every pointer in the ABI: a tensor (its data_ptr()), None (null), a Python int (an address) or a ctypes
    pointer value / array (c_void_p, a Structure array)."""

    @classmethod
    def from_param(cls, v):
        if v is None or isinstance(v, (C.c_void_p, C.Array, C._Pointer)):
            return v
        return C.c_void_p(v if isinstance(v, int) else v.data_ptr())  # (anything else: AttributeError, which ctypes reports with the argument's index)


_RESTYPES = {"int": C.c_int, "int64_t": C.c_int64, "const char*": C.c_char_p, "void": None}
_SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float}
_POINTEES = {"void", "float", "int", "int32_t", "int64_t", "unsigned", "MhWgradProblem"}
# hand wrappers: for symbols outside the header (untyped: tools/dev_arms/dev_ops.py) and for callers in tools/ and tests/ that still wrap (through ops)
i32, i64, f32, u64, p = C.c_int, C.c_int64, C.c_float, C.c_uint64, DevPtr.from_param


def _header(path) -> str:
    """The header's text without its comments."""
    if not os.path.exists(path):
        raise MerlinHipError(f"{path} not found: the binding takes its prototypes and constants from the header.")
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _parse_header(path):
    """-> ({macro: int}, {function: (restype, [argtypes])}) of every `#define MH_* <int>` and every prototype in the header."""
    txt = _header(path)
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(MH_\w+)\s+\(?(-?\d+)\)?\s*$", txt, flags=re.M)}
    txt = re.sub(r"^\s*#.*$", "", txt, flags=re.M)
    protos = {}
    for ret, name, params in re.findall(r"(?:^|[;{}])\s*(const char\*|int64_t|int|void)\s+(mh_\w+)\s*\(([^()]*)\)\s*(?=;)", txt, flags=re.M):
        argtypes = []
        for prm in ([] if params.strip() == "void" else params.split(",")):
            ctype = " ".join(re.sub(r"\w+\s*$", "", prm).replace("*", " * ").split())  # drop the parameter's name
            if ctype.endswith("*") and ctype[:-1].replace("const", "").strip() in _POINTEES:
                argtypes.append(DevPtr)
            elif ctype in _SCALARS:
                argtypes.append(_SCALARS[ctype])
            else:
                raise MerlinHipError(f"{path}: {name}: unknown parameter type '{ctype}' in '{prm.strip()}'")
        protos[name] = (_RESTYPES[ret], argtypes)
    if unread := [n for n in declared_symbols(path) if n not in protos]:
        raise MerlinHipError(f"{path}: declared but without a readable prototype: {unread}")
    return defines, protos


def declared_symbols(path=None) -> list:
    """Every function name declared in include/merlin_hip.h."""
    return sorted(set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", _header(path or HEADER))))


DEFINES, PROTOTYPES = _parse_header(HEADER)
MH_BF16, MH_F16, MH_F32 = DEFINES["MH_BF16"], DEFINES["MH_F16"], DEFINES["MH_F32"]
EPI_BIAS, EPI_QUICK_GELU, EPI_RESIDUAL, EPI_ACCUM, EPI_OUT_F32 = (DEFINES["MH_EPI_" + k] for k in ("BIAS", "QUICK_GELU", "RESIDUAL", "ACCUM", "OUT_F32"))


def lib() -> C.CDLL:
    """The loaded library, every symbol of the header typed.  Status-returning launches go through call(); host queries and the void
    setters are plain attribute calls.  Symbols outside the header (the dev library's extra arms) stay untyped."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MerlinHipError(
                f"{LIB_PATH} not found: build it with `python -m merlin_amd.csrc.build` "
                "(hipcc --offload-arch=gfx950).  merlin_amd has no CPU fallback.")
        # torch must load ITS HIP runtime first: if libmerlin_hip.so pulled in a second copy of libamdhip64
        # before torch, the process would hold two runtimes and this one would see no device.
        import torch  # noqa: F401

        so = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():  # (a declared symbol the library lacks: AttributeError naming it)
            fn = getattr(so, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = so
        if os.environ.get("MH_GEMM_PERSISTENT") == "0":  # A/B switches for benchmarks
            _lib.mh_gemm_persistent(0)
        if os.environ.get("MH_ATTN_BWD_FUSED_KV"):  # 0: dK, dV from two kernels; 1: attn_bwd2_kv_k<MODE 3>; 2: attn_bwd3_kv_k (default)
            _lib.mh_attn_bwd_fused_kv(int(os.environ["MH_ATTN_BWD_FUSED_KV"]))
        if os.environ.get("MH_ATTN_WIDE_STORES"):
            _lib.mh_attn_wide_stores(int(os.environ["MH_ATTN_WIDE_STORES"]))
        if os.environ.get("MH_W4_MASK"):  # layouts the auto selection gives to the 4-wave GEMM (bit 0 TN, 1 NN, 2 NT)
            _lib.mh_gemm_w4_policy(int(os.environ["MH_W4_MASK"]))
        if os.environ.get("MH_W4_HALF"):  # 128-row block tiles of the 4-wave GEMM: 0 never, 1 auto (default), 2 wherever the form exists
            _lib.mh_gemm_w4_half(int(os.environ["MH_W4_HALF"]))
        if os.environ.get("MH_GEMM_GM"):
            _lib.mh_gemm_raster_group(int(os.environ["MH_GEMM_GM"]))
    return _lib


def check(code: int, what: str) -> None:
    if code != 0:
        msg = lib().mh_strerror(code).decode()
        raise MerlinHipError(f"{what} failed: {msg} (code {code})")


def launch(name: str, *args) -> int:
    """Calls the declared function `name` and returns its status.  ctypes rejects too few arguments but passes extra ones to a cdecl
    function, so the count is checked here."""
    if len(args) != len(PROTOTYPES[name][1]):
        raise TypeError(f"{name} takes {len(PROTOTYPES[name][1])} arguments, got {len(args)}")
    return getattr(_lib or lib(), name)(*args)


def call(name: str, *args) -> None:
    """launch() that raises MerlinHipError on a non-zero status."""
    check(launch(name, *args), name)
