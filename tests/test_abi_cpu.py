"""CPU-side checks of the drop-in boundary: the binding's header parser maps what it knows and refuses the rest, the ctypes struct mirrors
have the C compiler's layout, the C-ABI library loads and exports every declared symbol, the host mirror has the reference's state_dict key
set, and the product package never touches oracle/ or /root/reference."""
import ctypes
import os
import re
import sys

import pytest

import torch

from conftest import ROOT


def _build_if_needed():
    lib = os.path.join(ROOT, "gesture-generation-from-trimodal-context_amd", "libtrimodal_hip.so")
    if not os.path.exists(lib):
        import __graft_entry__ as g
        g.build()
    return lib


def test_library_exports_every_declared_symbol(pkg):
    L = pkg._lib
    lib = ctypes.CDLL(_build_if_needed())
    missing = [n for n in L.PROTOTYPES if not hasattr(lib, n)]
    assert not missing, missing
    other = {n for n, (ret, _) in L.DECLARED.items() if ret != "int"}             # by C spelling: ctypes.c_int32 is ctypes.c_int
    assert len(L.PROTOTYPES) >= 194 and "tg_last_error" in other and not other & set(L.SIGNATURES)
    assert set(L.SIGNATURES) | set(L.GETTERS_SETTERS) | other == set(L.PROTOTYPES)
    assert all(L.PROTOTYPES[n][1] is L.SIGNATURES[n] for n in L.SIGNATURES) and not set(L.GETTERS_SETTERS) & set(L.SIGNATURES)
    lib.tg_version.restype = ctypes.c_int
    assert lib.tg_version() == L.ABI_VERSION


SYNTHETIC = """
/* int tg_fake(int32_t x); an unbalanced ( and a ; in a block comment
 * int tg_fake2(void);  )) */
#ifndef SYN_H
#define SYN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define TG_ABI_VERSION 3      // int tg_fake3(void); (
typedef struct tg_window {
    const float* ptr;         /* ; ( */
    int64_t batch_stride, row_stride;
} tg_window;
typedef struct { int32_t off[44]; float* p[8]; } tg_ae_step_args;
int tg_version(void);
const char* tg_last_error(void);
int64_t tg_ws_bytes(int32_t B,
                    int32_t H);            // ) ; int tg_fake4(float y);
int32_t tg_plan(const tg_gemm_nt_problem* problems, int32_t n, int32_t out[6], int32_t* tile_m);
int tg_many(const tg_window* A, const float* x, int64_t ldx, uint32_t site, float slope,
            const float* const* v, float* const* w, const void* const* params,
            const uint64_t* s, double* ws, const tg_gemm_tn_problem* q, tg_ae_step_args* args,
            void* stream);
int tg_unnamed(int32_t, const float*, float *const *);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_maps_a_synthetic_header_exactly(pkg):
    L = pkg._lib
    P, I32, I64, F32, U32, PP = L.P, L.I32, L.I64, L.F32, L.U32, ctypes.POINTER(L.P)
    got = L.parse_header(SYNTHETIC)
    assert got == {
        "tg_version": ("int", []),
        "tg_last_error": ("const char *", []),
        "tg_ws_bytes": ("int64_t", [I32, I32]),
        "tg_plan": ("int32_t", [ctypes.POINTER(L.NtProblem), I32, P, P]),
        "tg_many": ("int", [L.WP, P, I64, U32, F32, PP, PP, PP, P, P, ctypes.POINTER(L.TnProblem), ctypes.POINTER(L.AeStepArgs), P]),
        "tg_unnamed": ("int", [I32, P, PP]),
    }
    assert list(got) == ["tg_version", "tg_last_error", "tg_ws_bytes", "tg_plan", "tg_many", "tg_unnamed"]       # declaration order
    assert [L.RESTYPES[got[n][0]] for n in got] == [ctypes.c_int, ctypes.c_char_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_int]
    assert L.I32 is not L.I64 and L.F32 is not L.U32 and L.P is not PP                      # the equality above tells the types apart


@pytest.mark.parametrize("decl", [
    "int tg_bad(tg_window w);",                       # a struct by value
    "int tg_bad(int32_t n, void (*cb)(int32_t));",    # a function pointer
    "int tg_bad(const char* fmt, ...);",
    "int tg_bad(double x);",
    "int tg_bad(int n);",                             # sizes are int32_t / int64_t
    "int tg_bad(size_t n);",                          # an unknown type name
    "int tg_bad(unsigned int n);",
    "int tg_bad(tg_thing* t);",
    "int tg_bad(float** v);",                         # only T* const* is a pointer table
    "int tg_bad(const tg_window* const* w);",
    "int tg_bad(float* v[4]);",
    "int tg_bad();",
    "void tg_bad(int32_t n);",
    "float tg_bad(void);",
    "tg_window tg_bad(void);",
    "float* tg_bad(void);",
    "static int tg_bad(void);",
    "int tg_bad(void); int tg_bad(int32_t n);",       # declared twice
])
def test_parser_refuses_what_it_does_not_know_and_names_the_declaration(pkg, decl):
    with pytest.raises(ValueError, match="tg_bad"):
        pkg._lib.parse_header("int tg_ok(int32_t n);\n" + decl + "\nint tg_after(void);\n")


@pytest.mark.parametrize("text", ["int helper(int32_t n);", "struct tg_s { int32_t a; };", "typedef int32_t tg_i;", "extern int tg_flag;"])
def test_parser_refuses_statements_that_are_no_tg_prototype(pkg, text):
    with pytest.raises(ValueError, match="not a tg_\\* prototype"):
        pkg._lib.parse_header("int tg_ok(int32_t n);\n" + text + "\n")


def test_missing_header_fails_at_import_with_a_plain_message(pkg, monkeypatch):
    monkeypatch.setattr(pkg._lib, "HEADER_PATH", "/nonexistent/include/trimodal_hip.h")
    with pytest.raises(ImportError, match="derived from the C header"):
        pkg._lib._read_header()


def _struct_bodies(L):
    """name -> the declarators of every typedef struct of the header, e.g. `int32_t M, N, out_kw, reserved;` gives four."""
    text = L.strip_comments(open(os.path.join(ROOT, "include", "trimodal_hip.h")).read())
    return {m.group(2): [d for stmt in m.group(1).split(";") if stmt.strip() for d in stmt.split(",")]
            for m in re.finditer(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", text)}


def test_struct_mirrors_have_the_layout_the_c_compiler_gives_the_header(pkg, tmp_path):
    """sizeof, and offsetof / sizeof of every field the ctypes classes name, from a host program compiled against the real header; the field
    counts against the declarators of the struct bodies, so a field added to the header alone fails even where it lands in tail padding."""
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no host C compiler")
    L = pkg._lib
    bodies = _struct_bodies(L)
    assert set(bodies) == set(L.STRUCTS) and len(bodies) == 4
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "trimodal_hip.h"', 'int main(void) {']
    for cname, cls in L.STRUCTS.items():
        lines.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'    printf("{cname}.{f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));' for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    exe = str(tmp_path / "layout")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]                          # a ctypes field the C struct does not have stops here
    c = {k: tuple(int(x) for x in v) for k, *v in (ln.split() for ln in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())}
    for cname, cls in L.STRUCTS.items():
        assert c[cname] == (ctypes.sizeof(cls),), (cname, c[cname], ctypes.sizeof(cls))
        assert len(cls._fields_) == len(bodies[cname]), (cname, len(cls._fields_), len(bodies[cname]))
        for f, _ in cls._fields_:
            d = getattr(cls, f)
            assert c[f"{cname}.{f}"] == (d.offset, d.size), (cname, f, c[f"{cname}.{f}"], (d.offset, d.size))
    assert [c[n][0] for n in L.STRUCTS] == [56, 288, 144, 488]


def test_argument_checks_fail_loudly_without_gpu(pkg):
    """Entry points validate arguments on the host before any launch: callable here, no GPU needed."""
    lib = pkg._lib.load()
    rc = lib.tg_adam_step(None, None, None, None, 0, 0.1, 0.5, 0.999, 1e-8, None, None)
    assert rc != 0 and b"tg_adam_step" in lib.tg_last_error()
    rc = lib.tg_gru_forward(None, 0, None, None, None, None, None, None, 0, 1, 1, 4, None)
    assert rc != 0


def test_state_dict_keys_match_reference(pkg):
    import argparse
    from oracle import ref_model as O
    a = argparse.Namespace(n_pre_poses=4, n_poses=34, input_context="both", hidden_size=300, n_layers=4, dropout_prob=0.3,
                           freeze_wordembed=False)
    g = pkg.PoseGenerator(a, 27, 512, 300, None, pkg.Vocab.speakers(17))
    d = pkg.ConvDiscriminator(27)
    ae = pkg.EmbeddingNet(a, 27, 34)
    gs, ds, as_ = O.make_generator_state(0), O.make_discriminator_state(1), O.make_autoencoder_state(2)
    for mod, st, n in ((g, gs, 117), (d, ds, 52), (ae, as_, 70)):
        sd = mod.state_dict()
        assert len(sd) == n and set(sd) == set(st)
        for k in sd:
            assert tuple(sd[k].shape) == tuple(st[k].shape) and sd[k].dtype == st[k].dtype, k
        mod.load_state_dict(st, strict=True)
    # the TCN's duplicated registration shares storage, like the reference
    sd = g.state_dict()
    assert sd["text_encoder.tcn.network.0.conv1.weight_v"].data_ptr() == sd["text_encoder.tcn.network.0.net.0.weight_v"].data_ptr()
    assert sum(p.numel() for p in g.parameters()) == 13_204_939 - (20000 - 512) * 300 - (1371 - 17) * 16
    assert sum(p.numel() for p in d.parameters()) == 253_950 and sum(p.numel() for p in ae.parameters()) == 190_691


def test_product_never_imports_oracle_or_reference():
    pdir = os.path.join(ROOT, "gesture-generation-from-trimodal-context_amd")
    for dirpath, _, files in os.walk(pdir):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f
                assert "sys.path" not in src or f == "__init__.py", f
                assert "/root/reference" not in src, f


def test_missing_library_fails_loudly(pkg, monkeypatch):
    monkeypatch.setattr(pkg._lib, "_lib", None)
    monkeypatch.setattr(pkg._lib, "LIB_PATH", "/nonexistent/libtrimodal_hip.so")
    try:
        pkg._lib.load()
    except RuntimeError as e:
        assert "no CPU fallback" in str(e)
    else:
        raise AssertionError("load() must raise when the HIP library is missing")


def test_every_entry_point_validates_its_arguments(pkg):
    """tests/abi_fuzz.py: every C-ABI function called with nulls / zero sizes / negative sizes / zeroed tables comes back with a status
    and never crashes -- no GPU needed, validation precedes any launch."""
    from tests.abi_fuzz import fuzz
    assert fuzz() >= 4 * len(pkg._lib.SIGNATURES)


def test_entry_points_under_host_address_sanitizer():
    """The same fuzz against the host-ASan build of the library (make -C csrc asan) in a subprocess with the ASan runtime preloaded:
    an out-of-bounds read of a launcher (problem tables, pointer arrays, split plans) would abort the subprocess with a report."""
    import glob
    import subprocess
    csrc = os.path.join(ROOT, "gesture-generation-from-trimodal-context_amd", "csrc")
    rt = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so"))
    if not rt or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no ROCm toolchain / ASan runtime on this machine")
    subprocess.run(["make", "-C", csrc, "-j4", "asan"], check=True, capture_output=True)
    lib = os.path.join(ROOT, "gesture-generation-from-trimodal-context_amd", "libtrimodal_hip_asan.so")
    # the runtime goes first, anything already preloaded stays; no GPU visible to the subprocess, on a GPU machine too (the fuzz is a host check)
    pre = os.environ.get("LD_PRELOAD")
    env = dict(os.environ, LD_PRELOAD=rt[-1] + (":" + pre if pre else ""), ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=66",
               HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "abi_fuzz.py"), lib], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "abi fuzz ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def test_deferred_weight_gradients_are_grouped_by_kernel_family(pkg, monkeypatch):
    """layers.tn_group_deferred (host logic, no GPU): problems that qualify for the bf16 x 3 weight-gradient kernel and those that do not are
    launched in separate groups of at most MAX_GROUP, every problem exactly once, order kept inside a kind."""
    from types import SimpleNamespace as NS
    L, ops = pkg.layers, pkg.ops
    calls = []
    monkeypatch.setattr(ops, "gemm_tn_group", lambda probs: calls.append(list(probs)))
    def prob(M, N, K, tag):
        return dict(dY=torch.zeros(M, N), A=NS(K=K, s=NS(cw=K)), dW=None, dbias=None, tag=tag)
    big = [prob(7168, 192, 128, f"big{i}") for i in range(14)]           # the discriminator's GRU layers 1..3 (ih + hh) and layer 0 hh
    small = [prob(7168, 192, 8, "ih0f"), prob(7168, 192, 8, "ih0r"), prob(7680, 8, 24, "conv2"), prob(8192, 8, 48, "conv1"), prob(512, 192, 128, "short")]
    mixed = [big[0], small[0], *big[1:8], small[1], *big[8:], *small[2:]]
    L.tn_group_deferred(mixed)
    assert [len(c) for c in calls] == [8, 6, 5]
    assert [p["tag"] for c in calls[:2] for p in c] == [f"big{i}" for i in range(14)]
    assert [p["tag"] for p in calls[2]] == ["ih0f", "ih0r", "conv2", "conv1", "short"]


def test_nt_epilogue_operands_are_checked_on_the_host(pkg, monkeypatch):
    """ops._nt_problem: res and out2 go together and every epilogue operand must be laid out exactly like the output (the wrappers accept
    CUDA tensors only; that check is lifted here to reach the layout checks without a GPU)."""
    ops, Win = pkg.ops, pkg.ops.Win
    monkeypatch.setattr(ops, "_f32", lambda t, name="tensor": None)
    x, w, out = torch.zeros(64, 32), torch.zeros(16, 32), torch.zeros(64, 16)
    q = ops._nt_problem(Win.plain(x), w, None, out, gate=torch.zeros(64, 16), res=torch.zeros(64, 16), out2=torch.zeros(64, 16), res_slope=0.0)
    assert q.gate and q.res and q.C2 and q.res_slope == 0.0
    with pytest.raises(AssertionError):
        ops._nt_problem(Win.plain(x), w, None, out, res=torch.zeros(64, 16))
    with pytest.raises(AssertionError):
        ops._nt_problem(Win.plain(x), w, None, out, gate=torch.zeros(64, 17))
    with pytest.raises(AssertionError):
        ops._nt_problem(Win.plain(x), w, None, out, gate=torch.zeros(16, 64).t())
