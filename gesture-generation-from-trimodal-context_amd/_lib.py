"""ctypes binding of libtrimodal_hip.so (the C ABI declared in include/trimodal_hip.h).

The header is the table: it is parsed once at import (text only; the library is not opened before load()) and every prototype's restype /
argtypes, and ABI_VERSION, come from it.  A new entry point needs its declaration there and nothing here; only the struct mirrors below are
written by hand (tests/test_abi_cpu.py pins their layout against the C compiler's).  A declaration outside the header's "plain C types
only" convention fails the import, naming it.

There is no CPU fallback: if the library is missing or a symbol is absent the import fails loudly.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# (TG_LIB_PATH: another build of the same library -- same-box A/B timing against an older build, tools/ab_bench.sh; the lab library of the
# ablation tools.  Unset in every test and in bench.py's default run.)
LIB_PATH = os.environ.get("TG_LIB_PATH") or os.path.join(_HERE, "libtrimodal_hip.so")
HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "trimodal_hip.h")


class Window(C.Structure):
    """struct tg_window (include/trimodal_hip.h)."""
    _fields_ = [("ptr", C.c_void_p), ("batch_stride", C.c_int64), ("row_stride", C.c_int64), ("rows_in", C.c_int32),
                ("rows_out", C.c_int32), ("row_step", C.c_int32), ("shift", C.c_int32), ("dil", C.c_int32),
                ("cw", C.c_int32), ("K", C.c_int32)]


P, I32, I64, F32, U32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_uint32
WP = C.POINTER(Window)


class NtProblem(C.Structure):
    """struct tg_gemm_nt_problem"""
    _fields_ = [("A", Window), ("Bw", P), ("ldb", I64), ("b_seg_k", I32), ("reserved", I32), ("b_seg_stride", I64), ("bias", P), ("C", P),
                ("c_batch_stride", I64), ("c_row_stride", I64), ("c_rows_out", I32), ("M", I32), ("N", I32), ("act_slope", F32),
                ("accumulate", I32), ("out_scale", P), ("b_planes", P), ("b_plane_stride", I64), ("b_rows", I32), ("b_row0", I32),
                ("gate", P), ("res", P), ("C2", P), ("res_slope", F32), ("drop_site", U32), ("drop_state", P), ("drop_index0", I64),
                ("drop_p", F32), ("reserved4", I32), ("b_planes_kind", I32), ("reserved5", I32), ("b_inv_scale", P), ("a_row_scale", P), ("a_rowmax", P), ("c_rowmax", P), ("c2_rowmax", P), ("a_rowmax_rows", I32), ("reserved6", I32)]


class TnProblem(C.Structure):
    """struct tg_gemm_tn_problem"""
    _fields_ = [("dY", P), ("ldy", I64), ("A", Window), ("dW", P), ("ldw", I64), ("M", I32), ("N", I32), ("out_kw", I32), ("reserved", I32),
                ("dbias", P), ("ws", P), ("ws_floats", I64), ("y_colmax", P), ("a_colmax", P)]


class AeStepArgs(C.Structure):
    """struct tg_ae_step_args"""
    _fields_ = [("x", P), ("params", P), ("grads", P), ("off", I32 * 44), ("running_mean", P * 8), ("running_var", P * 8),
                ("num_batches_tracked", P * 8), ("ws", P), ("ws_bytes", I64), ("loss", P), ("recon", P), ("feat", P), ("step", P), ("B", I32),
                ("bn_eps", F32), ("momentum", F32), ("last_phase", I32), ("adam_m", P), ("adam_v", P), ("lr", F32), ("beta1", F32), ("beta2", F32), ("adam_eps", F32)]


MAX_GROUP = 8

STRUCTS = {"tg_window": Window, "tg_gemm_nt_problem": NtProblem, "tg_gemm_tn_problem": TnProblem, "tg_ae_step_args": AeStepArgs}
_BY_VALUE = {"int32_t": I32, "int64_t": I64, "uint32_t": U32, "float": F32}
# C return type -> restype.  c_int32 IS c_int here, so "returns a status" (int) is told from "returns a number" (int32_t) by the spelling
RESTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "const char *": C.c_char_p}
_POINTEES = {"void", "char", "int", "float", "double"} | {f"{u}int{n}_t" for u in ("", "u") for n in (8, 16, 32, 64)}


def strip_comments(text):
    """The header's comments hold parentheses, semicolons and text that looks like a prototype: they go first."""
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)


# one parameter: [const] TYPE [const] {* [const]} [name] [[n]]
_PARAM = re.compile(r"\s*(?:const\s+)?(\w+)(?:\s+const\b)?((?:\s*\*(?:\s*const\b)?)*)\s*(?:(?<=[\s*])(?!const\b)\w+)?\s*(\[[^\]]*\])?\s*")


def _argtype(arg, decl):
    """One parameter of `decl` -> its ctypes type; ValueError for anything but the forms the header's conventions allow."""
    m = _PARAM.fullmatch(arg)
    base, stars, array = m.groups() if m else ("", "", None)
    ptr = "".join(stars.split()) + ("*" if array else "")             # `int32_t out[6]` is `int32_t* out`
    if base not in _POINTEES and base not in STRUCTS:
        raise ValueError(f"{decl}: unknown type in parameter `{arg}`")
    if not ptr and base in _BY_VALUE:
        return _BY_VALUE[base]
    if ptr.count("*") == 1:
        return P if base not in STRUCTS else WP if base == "tg_window" else C.POINTER(STRUCTS[base])
    if ptr in ("*const*", "*const*const") and base not in STRUCTS:
        return C.POINTER(P)
    raise ValueError(f"{decl}: parameter `{arg}` is outside the plain-C convention of the header")


def parse_header(text):
    """Every `RET tg_name(ARGS);` of a header text -> {name: (RET as spelled, [argtypes])}, in declaration order.  Comments, preprocessor lines,
    the extern "C" bracket and typedef struct blocks are skipped; any other statement, return type or parameter raises ValueError."""
    text = re.sub(r"#\s*ifdef\s+__cplusplus.*?#\s*endif", " ", strip_comments(text), flags=re.S)
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    text = re.sub(r"\btypedef\s+struct\b[^{;]*\{[^{}]*\}\s*\w+\s*;", " ", text)
    out = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = re.fullmatch(r"(.*?)\b(tg_\w+) ?\((.*)\)", stmt)
        if not m:
            raise ValueError(f"not a tg_* prototype: `{stmt[:120]}`")
        ret, name, args = " ".join(re.findall(r"\w+|\S", m.group(1))), m.group(2), m.group(3).strip()
        if ret not in RESTYPES:
            raise ValueError(f"{name}: return type `{ret}` is outside the plain-C convention of the header")
        if name in out:
            raise ValueError(f"{name}: declared twice")
        if not args:
            raise ValueError(f"{name}: empty parameter list; write (void)")
        out[name] = (ret, [] if args == "void" else [_argtype(a, name) for a in args.split(",")])
    return out


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            text = f.read()
    except OSError as e:
        raise ImportError(f"{HEADER_PATH} not readable ({e}): the binding is derived from the C header, which ships beside the package "
                          "(<package>/../include/trimodal_hip.h)") from None
    m = re.search(r"^#define\s+TG_ABI_VERSION\s+(\d+)\s*$", text, flags=re.M)
    if not m:
        raise ImportError(f"{HEADER_PATH} has no #define TG_ABI_VERSION")
    return int(m.group(1)), parse_header(text)


# name -> (C return type as spelled, argtypes) of every declared function, and the same with the restype: what load() sets
ABI_VERSION, DECLARED = _read_header()
PROTOTYPES = {n: (RESTYPES[r], a) for n, (r, a) in DECLARED.items()}
# the process-wide getters and setters: they return int as well, but give or take a plain value (a zero argument is valid), so they are
# not among the entries that must refuse null / zero arguments (tests/abi_fuzz.py)
GETTERS_SETTERS = ("tg_version", "tg_set_deterministic", "tg_get_deterministic", "tg_set_tn_workgroup_cap", "tg_get_tn_workgroup_cap",
                   "tg_set_math_mode", "tg_get_math_mode", "tg_set_nt_mover_waves")
# name -> argtypes of the status-returning entry points (0 on success, message in tg_last_error): what call() is for
SIGNATURES = {n: a for n, (r, a) in DECLARED.items() if r == "int" and n not in GETTERS_SETTERS}
_lib = None


def load():
    """Load the shared library once; raise with a build hint if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C gesture-generation-from-trimodal-context_amd/csrc`). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing: intended
        fn.argtypes = argtypes
        fn.restype = restype
    if lib.tg_version() != ABI_VERSION:
        raise RuntimeError(f"libtrimodal_hip.so ABI {lib.tg_version()} != expected {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {lib.tg_last_error().decode()}")
