"""ctypes binding of liblpd_hip.so.  include/lpd_hip.h is the only description of the C-ABI: the argument and return types of
every entry point (SIGNATURES, _RESTYPES) and the integer constants it defines (DEFINES) are read from its text once, when this
module is imported.  A prototype outside the header's closed grammar raises instead of being guessed; tests/test_abi.py holds the
result to what a C++ compiler reads in the same header.

torch is imported first on purpose: liblpd_hip.so needs libamdhip64.so.7, and the dynamic loader
then reuses the HIP runtime torch already loaded (same SONAME), so device pointers and stream
handles are shared between torch and these kernels.

There is NO fallback: if the library is missing this raises, and every op in ops.py raises on
non-CUDA tensors.
"""
import ctypes
import os
import re

import torch  # noqa: F401  (must precede CDLL, see above)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LPD_HIP_LIB") or os.path.join(_HERE, "liblpd_hip.so")   # override: kernel-variant builds (tools/)
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "lpd_hip.h")      # = _build.PUBLIC_HEADER

_c_int = ctypes.c_int
_c_ll = ctypes.c_longlong
_c_f = ctypes.c_float
_c_p = ctypes.c_void_p

# the header's whole type vocabulary; every parameter whose type contains `*` is a c_void_p
_SCALARS = {"int": _c_int, "int32_t": _c_int, "long long": _c_ll, "int64_t": _c_ll,
            "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "uint32_t": ctypes.c_uint,
            "unsigned long long": ctypes.c_ulonglong, "uint64_t": ctypes.c_ulonglong, "float": _c_f, "double": ctypes.c_double}
_RETURNS = {"int": _c_int, "long long": _c_ll, "const char*": ctypes.c_char_p}
_TYPE_WORDS = {w for t in _SCALARS for w in t.split()} | {"long", "short", "char", "signed", "void"}      # never a parameter's name


class LpdHipError(RuntimeError):
    pass


def _param_type(param):
    if "*" in param:
        return _c_p
    words = [w for w in param.split() if w != "const"]
    for n in (3, 2, 1):      # the longest type first; what is left is at most the parameter's name
        ctype, name = _SCALARS.get(" ".join(words[:n])), words[n:]
        if ctype and (not name or (len(name) == 1 and name[0].isidentifier() and name[0] not in _TYPE_WORDS)):
            return ctype
    return None


def parse_header(text):
    """(SIGNATURES, _RESTYPES, DEFINES) of a header's text: name -> argtypes of every prototype `ret lpd_name(params);`, the returns
    that are not int, and every `#define LPD_NAME <integer literal>`."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)      # the comments hold call-like text
    defines = {m[1]: int("".join(m[2].split()), 0) for m in re.finditer(
        r"^[ \t]*#[ \t]*define[ \t]+(LPD_\w+)[ \t]+\(?[ \t]*(-?[ \t]*(?:0[xX][0-9a-fA-F]+|[1-9][0-9]*|0))[ \t]*\)?[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    signatures, restypes = {}, {}
    for m in re.finditer(r"([^;{}]*?)\b(lpd_\w+)\s*\(([^;{}]*)\)\s*;", text):      # everything since the last statement is the return type
        ret, name, params = re.sub(r"\s*\*\s*", "*", " ".join(m[1].split())), m[2], m[3]
        if name in signatures:
            raise LpdHipError(f"lpd_hip.h declares {name} twice")
        if ret not in _RETURNS:
            raise LpdHipError(f"lpd_hip.h: {name}: no ctypes type for the return type {ret!r}")
        params = [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")]
        argtypes = [None if "(" in p or ")" in p or "[" in p else _param_type(p) for p in params]
        if None in argtypes:
            raise LpdHipError(f"lpd_hip.h: {name}: no ctypes type for the parameter {params[argtypes.index(None)]!r}")
        signatures[name] = argtypes
        if _RETURNS[ret] is not _c_int:
            restypes[name] = _RETURNS[ret]
    return signatures, restypes, defines


def _read_header():
    try:
        with open(HEADER_PATH) as fh:
            return parse_header(fh.read())
    except OSError as e:
        raise LpdHipError(f"{HEADER_PATH}: the public header is not readable ({e}); the binding is derived from it") from None


# name -> argtypes (restype is int unless listed in _RESTYPES); LPD_* name -> value
SIGNATURES, _RESTYPES, DEFINES = _read_header()

_lib = None


def load():
    """Load liblpd_hip.so; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LpdHipError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` at the repo root (needs hipcc). There is no CPU/PyTorch fallback for this path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, ctypes.c_int)
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().lpd_last_error()
        raise LpdHipError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")
