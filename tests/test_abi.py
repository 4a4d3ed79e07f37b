"""The C-ABI boundary as a C caller sees it: tests/abi_smoke.c is compiled (by __graft_entry__.build()) against
include/lpd_hip.h and linked with liblpd_hip.so.  On CPU only the symbol/size calls run; on the GPU box it drives
lpd_gemm (row-major and cloud-panel operands), lpd_gemm_bf16x3 and lpd_knn through the header's prototypes.

The ctypes binding (lpdnet_hip/_lib.py) derives its argtypes, restypes and constants from the same header's text: a host C++ program
reports every entry point's types, the layout of LpdCleanParams and the value of every LPD_* integer macro as the compiler reads them,
and they must equal what the binding read; the reader itself is exercised on strings."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "abi_smoke")
HEADER = os.path.join(ROOT, "include", "lpd_hip.h")


def _ensure_built():
    if not os.path.exists(BIN):
        from lpdnet_hip import _build
        _build.build()
        _build.build_abi_smoke()
    return BIN


def test_definitions_are_compiled_against_the_public_header():
    """csrc/lpd_common.h includes include/lpd_hip.h, so a prototype that differs from its extern "C" definition is a compile
    error in build(); this guards the include itself."""
    text = open(os.path.join(ROOT, "lpd-net-pytorch_amd", "csrc", "lpd_common.h")).read()
    assert '#include "../../include/lpd_hip.h"' in text
    for f in os.listdir(os.path.join(ROOT, "lpd-net-pytorch_amd", "csrc")):
        if f.endswith(".hip"):
            assert '#include "lpd_common.h"' in open(os.path.join(ROOT, "lpd-net-pytorch_amd", "csrc", f)).read(), f


def test_c_caller_links_and_resolves_symbols():
    r = subprocess.run([_ensure_built(), "--symbols"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "symbols OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_c_caller_runs_the_kernels_through_the_header(cuda):
    r = subprocess.run([_ensure_built()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "abi_smoke OK" in r.stdout, r.stdout + r.stderr


# ---- the binding's reading of the header (lpdnet_hip/_lib.py parse_header) against a C++ compiler's reading of the same file ----

LETTER = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_longlong: "l", ctypes.c_uint: "u", ctypes.c_ulonglong: "U",
          ctypes.c_float: "f", ctypes.c_double: "d", ctypes.c_char_p: "s"}

PROGRAM_HEAD = r"""
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "lpd_hip.h"
template <class T> constexpr char scalar() {
    return std::is_same_v<T, int> ? 'i' : std::is_same_v<T, long long> ? 'l' : std::is_same_v<T, unsigned> ? 'u'
         : std::is_same_v<T, unsigned long long> ? 'U' : std::is_same_v<T, float> ? 'f' : std::is_same_v<T, double> ? 'd' : '?';
}
template <class T> constexpr char param() { return std::is_pointer_v<T> ? 'p' : scalar<T>(); }
template <class T> constexpr char ret() { return std::is_same_v<T, const char*> ? 's' : param<T>(); }
template <class F> struct Sig;
template <class R, class... A> struct Sig<R (*)(A...)> {
    static void print(const char* name) {
        const char params[] = {param<A>()..., 0};
        std::printf("fn %s %c:%s\n", name, ret<R>(), params);
    }
};
int main() {
"""


def _header_functions():
    """every lpd_* name in front of a parenthesis outside the block comments (as tests/test_host_cpu.py collects them): NOT _lib's reader"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(lpd_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def compiler_view(tmp_path_factory):
    """the lines a C++17 program prints about include/lpd_hip.h: compiled with -I include alone, nothing linked"""
    from lpdnet_hip import _lib, ops
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    body = [f'    Sig<decltype(&{n})>::print("{n}");' for n in _header_functions()]
    body.append('    std::printf("sizeof %zu\\n", sizeof(LpdCleanParams));')
    body += [f'    std::printf("field {f} %zu\\n", offsetof(LpdCleanParams, {f}));' for f, _ in ops.CleanParams._fields_]
    body += [f'    std::printf("define {d} %lld\\n", (long long)({d}));' for d in _lib.DEFINES]
    d = tmp_path_factory.mktemp("abi_types")
    (d / "abi_types.cpp").write_text(PROGRAM_HEAD + "\n".join(body) + "\n    return 0;\n}\n")
    r = subprocess.run([cxx, "-std=c++17", "-I", os.path.dirname(HEADER), str(d / "abi_types.cpp"), "-o", str(d / "abi_types")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(d / "abi_types")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return [line.split(" ") for line in r.stdout.splitlines()]


def test_binding_types_equal_the_compilers(compiler_view):
    """Every entry point: the return type and each parameter type that decltype(&lpd_x) has, as letters, against the ctypes classes the
    binding derived from the header's text.  A c_int where the prototype says long long, or a missing parameter, fails here."""
    from lpdnet_hip import _lib
    lines = [l for l in compiler_view if l[0] == "fn"]
    got = {name: letters for _, name, letters in lines}
    assert len(got) == len(lines) == len(_lib.SIGNATURES)
    assert "?" not in "".join(got.values())
    for name, letters in got.items():
        want = LETTER[_lib._RESTYPES.get(name, ctypes.c_int)] + ":" + "".join(LETTER[t] for t in _lib.SIGNATURES[name])
        assert letters == want, (name, letters, want)
    assert (_lib._c_int, _lib._c_ll, _lib._c_f, _lib._c_p) == (ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_void_p)


def test_clean_params_layout_equals_the_compilers(compiler_view):
    from lpdnet_hip import ops
    assert [int(v) for kind, v, *_ in compiler_view if kind == "sizeof"] == [ctypes.sizeof(ops.CleanParams)] == [64]
    got = [(name, int(off)) for kind, name, off in (l for l in compiler_view if l[0] == "field")]
    assert got == [(f, getattr(ops.CleanParams, f).offset) for f, _ in ops.CleanParams._fields_] and len(got) == 16


def test_defines_equal_the_compilers(compiler_view):
    from lpdnet_hip import _lib, ops
    got = {name: int(v) for kind, name, v in (l for l in compiler_view if l[0] == "define")}
    assert got == _lib.DEFINES
    assert {"LPD_OK", "LPD_ERR_ARG", "LPD_ERR_LAUNCH", "LPD_ERR_UNSUPPORTED", "LPD_ACT_NONE", "LPD_ACT_RELU", "LPD_ACT_LEAKY", "LPD_ACT_SIGMOID",
            "LPD_KNN_PM_PREPARED", "LPD_CLEAN_CHUNK"} <= set(got)
    assert (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LEAKY, ops.ACT_SIGMOID) == tuple(got["LPD_ACT_" + n] for n in ("NONE", "RELU", "LEAKY", "SIGMOID"))
    assert (ops.KNN_PM_PREPARED, ops.CLEAN_CHUNK) == (got["LPD_KNN_PM_PREPARED"], got["LPD_CLEAN_CHUNK"])
    # every integer limit that a wrapper enforces: defined in the public header, and ops holds the compiler's value under its name
    assert set(WRAPPER_LIMITS) <= set(_lib.DEFINES)
    for name in WRAPPER_LIMITS:
        assert getattr(ops, name[len("LPD_"):]) == got[name], name


WRAPPER_LIMITS = [
    "LPD_SUBMAP_MIN_N", "LPD_SUBMAP_MAX_N", "LPD_SUBMAP_MAX_POINTS",
    "LPD_TUPLE_MAX_ITEMS", "LPD_TUPLE_MAX_SAMPLES", "LPD_TUPLE_MAX_LISTS", "LPD_TUPLE_MAX_ROWS",
    "LPD_PLACES_MAX_ITEMS", "LPD_PLACES_MAX_SEGMENTS", "LPD_PLACES_CHUNK",
    "LPD_CLEAN_MAX_H",
    "LPD_DRIVE_MAX_SCANS", "LPD_DRIVE_MAX_WINDOWS", "LPD_DRIVE_MAX_WINDOW_NO", "LPD_DRIVE_MAX_UNITS",
    "LPD_MAP_CHUNK", "LPD_MAP_MAX_PROBES", "LPD_MAP_MIN_CAPACITY", "LPD_MAP_MAX_CAPACITY", "LPD_MAP_QLIM",
    "LPD_ALIGN_GRID", "LPD_ALIGN_MAX_S", "LPD_ALIGN_MAX_LAYERS", "LPD_ALIGN_MAX_H", "LPD_ALIGN_MAX_R", "LPD_ALIGN_MAX_POINTS", "LPD_ALIGN_MAX_PAIRS",
    "LPD_ICP_MAX_POINTS", "LPD_ICP_MAX_PAIRS", "LPD_ICP_MAX_ITERS", "LPD_ICP_MIN_INLIERS", "LPD_ICP_SUMS",
    "LPD_STAT_CMAX", "LPD_RECALL_KMAX"]


# ---- the reader on strings ----

def test_reader_reads_the_headers_grammar():
    from lpdnet_hip._lib import parse_header
    i, l, f, p = ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_void_p
    sigs, res, defs = parse_header("""
        #define LPD_A 7
        #define LPD_B (-3)
        #define LPD_C ( - 2 )
        #define LPD_HEX 0x10
        #define LPD_FLOAT 512.0f
        #define LPD_EXPR (1 << 20)
        #define LPD_CALL(x) lpd_macro(x)
        #define OTHER 1
        typedef struct LpdS { float a, b; int32_t n; } LpdS;
        int lpd_multi(const float* x, int n,
                      long long stride,
                      float slope, void* stream);
        int lpd_none(void);
        long long lpd_unnamed(int, long long, const float*, unsigned);
        int lpd_ptrs(float** xx, const LpdS* prm, uint16_t* idx16, unsigned char* mask, const void *frags);
        const char* lpd_text(void);
        const char *lpd_text2(void);
        int lpd_scalars(int32_t a, int64_t b, unsigned c, unsigned int d, uint32_t e, unsigned long long g, uint64_t h, float x, double y,
                        const int z);
        /* lpd_in_block(NULL, 64, ...) then
           int lpd_in_block2(int n); */
        // int lpd_in_line(int n);
        int lpd_after(int n);   // lpd_in_line2(3);
    """)
    assert sigs == {"lpd_multi": [p, i, l, f, p], "lpd_none": [], "lpd_unnamed": [i, l, p, ctypes.c_uint], "lpd_ptrs": [p] * 5,
                    "lpd_text": [], "lpd_text2": [],
                    "lpd_scalars": [i, l, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_ulonglong, f, ctypes.c_double, i],
                    "lpd_after": [i]}
    assert res == {"lpd_unnamed": l, "lpd_text": ctypes.c_char_p, "lpd_text2": ctypes.c_char_p}
    assert defs == {"LPD_A": 7, "LPD_B": -3, "LPD_C": -2, "LPD_HEX": 16}


@pytest.mark.parametrize("proto", ["int lpd_bad(size_t n);", "int lpd_bad(int a, long n);", "int lpd_bad(struct S v);", "int lpd_bad(int (*cb)(int));",
                                   "int lpd_bad(unsigned long);", "int lpd_bad(LpdS v);", "int lpd_bad();", "int lpd_bad(int a[4]);",
                                   "long lpd_bad(void);", "size_t lpd_bad(void);", "float* lpd_bad(void);", "static int lpd_bad(void);",
                                   "inline int lpd_bad(void);", "__attribute__((visibility(\"default\"))) int lpd_bad(void);",
                                   "int lpd_bad(void) __attribute__((cold));", "int lpd_ok(void); int lpd_bad(int n); long long lpd_bad(int n);"])
def test_reader_refuses_what_it_cannot_map(proto):
    from lpdnet_hip._lib import LpdHipError, parse_header
    with pytest.raises(LpdHipError, match="lpd_bad"):
        parse_header("int lpd_first(int n);\n" + proto + "\nint lpd_last(void);\n")


def test_header_is_read_at_import_only_and_a_missing_header_names_its_path(monkeypatch, tmp_path):
    """load() and the calls work from the dicts made at import; the header is found from the module's own location."""
    from lpdnet_hip import _build, _lib
    assert _lib.HEADER_PATH == _build.PUBLIC_HEADER == HEADER
    parses = []
    monkeypatch.setattr(_lib, "parse_header", lambda text: parses.append(text))
    monkeypatch.setattr(_lib, "_lib", None)      # load() as the first caller meets it
    lib = _lib.load()
    assert lib.lpd_version() >= 100 and _lib.load() is lib and lib.lpd_last_error.restype is ctypes.c_char_p
    _lib.check(0, "nothing")
    assert parses == []
    missing = str(tmp_path / "include" / "lpd_hip.h")
    monkeypatch.setattr(_lib, "HEADER_PATH", missing)
    with pytest.raises(_lib.LpdHipError, match=re.escape(missing)):
        _lib._read_header()
