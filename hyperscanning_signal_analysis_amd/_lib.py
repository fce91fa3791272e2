"""ctypes binding of libhypermvar.so (the C ABI declared in include/hypermvar.h).

The shared library is built in-tree by `__graft_entry__.build()` / `make -C csrc`.  There is NO CPU
fallback: if the library is missing or a symbol is absent, importing the engine fails loudly.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_int, c_int32, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhypermvar.so")
HEADER = os.path.join(_HERE, os.pardir, "include", "hypermvar.h")


class HypermvarLibraryError(ImportError):
    pass


_SCALARS = {"int": c_int, "int32_t": c_int32, "int64_t": c_int64, "double": c_double}


def _ctype(decl, named, where):
    """ctypes type of a return type (named=False) or of a `type name` parameter (named=True) of the prototype `where`."""
    if "*" in decl:
        return c_char_p if not named and decl.replace("*", " * ").split() == ["const", "char", "*"] else c_void_p
    words = [w for w in decl.split() if w != "const"]
    if len(words) != 1 + named or words[0] not in _SCALARS:
        raise HypermvarLibraryError(f"cannot bind `{' '.join(decl.split())}` of `{where}`: the binding knows int, int32_t, "
                                    "int64_t, double and pointers, and every parameter must be named")
    return _SCALARS[words[0]]


def signatures_from_header(text):
    """{name: (restype, [argtypes])} of every hmv_* prototype in the text of a header.  A pointer is c_void_p (a returned
    `const char*` c_char_p), the four scalar types are themselves, and anything else raises: a guess here would hand a
    kernel launch a truncated or shifted argument."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = "\n".join(line for line in text.split("\n") if not line.lstrip().startswith("#"))
    sigs = {}
    for ret, name, args in re.findall(r"([\w\s*]*?)\b(hmv_\w+)\s*\(([^()]*)\)\s*;", text):
        where = " ".join(f"{ret}{name}({args})".split())
        args = [] if args.strip() in ("", "void") else args.split(",")
        sigs[name] = (_ctype(ret, False, where), [_ctype(a, True, where) for a in args])
    n_seen = len(re.findall(r"\bhmv_\w+\s*\(", text))
    if n_seen != len(sigs):      # a function pointer, a macro-wrapped or a repeated declaration: never skipped silently
        raise HypermvarLibraryError(f"`hmv_name(` occurs {n_seen} times but {len(sigs)} prototypes could be read")
    return sigs


def _header_text():
    try:
        with open(HEADER) as f:
            return f.read()
    except OSError as e:
        raise HypermvarLibraryError(f"{HEADER} not found: the ctypes table is read from it") from e


# name -> (restype, argtypes): include/hypermvar.h is the one statement of the C ABI
SIGNATURES = signatures_from_header(_header_text())

# option bits of the fused entry points (include/hypermvar.h)
FLAG_UNFUSED_NORM = 1
FLAG_YW_TILED = 2
FLAG_YW_ONE_LAUNCH = 4
FLAG_DIRECT_LAGCOV = 8
FLAG_YW_PIVOTED = 16
# measures of hmv_sliding_auto_f64 and the criterion numbering it shares with hmv_fad_f64
MEASURE_FFDTF = 0
MEASURE_DDTF = 1
MEASURE_GPDC = 2
CRITERIA = {"AIC": 0, "HQ": 1, "SC": 2}
# hmv_set_tuning keys
TUNE_NORM_LAG = 1
TUNE_LAG_GROUP = 2
TUNE_K3_FORM = 3
TUNE_YW_FORM = 4
TUNE_K3_LDS_PAD = 5
TUNE_K3_SPLIT = 6
K3_SPLIT_NO_FRONT = 1 << 19         # added to a TUNE_K3_SPLIT value: K1 is never cut at the split
# limits of hmv_decimate_fir_f64
MAX_DECIMATE = 32
MAX_DECIMATE_TAPS = 641
# modes of hmv_phase_sync_c128
PHASE_UNIT = 0
PHASE_RAW = 1


_lib = None


def load():
    """Load libhypermvar.so and bind every symbol of include/hypermvar.h.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    global LIB_PATH
    # A/B measurements of kernel variants on ONE box: HYPERMVAR_LIB names another build of the same library
    LIB_PATH = os.environ.get("HYPERMVAR_LIB", LIB_PATH)
    if not os.path.exists(LIB_PATH):
        raise HypermvarLibraryError(
            f"{LIB_PATH} not found: build the HIP library first "
            f"(python -c 'import __graft_entry__ as g; g.build()' or make -C {_HERE}/csrc). "
            "There is no CPU fallback for the MVAR/ffDTF path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:  # pragma: no cover
            raise HypermvarLibraryError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def call(lib, entry: str, *args):
    """lib.<entry>(*args) for an entry that returns a status, which `check` turns into an exception: a torch tensor is
    passed as its data pointer, None as a null pointer, everything else as it is."""
    fn = getattr(lib, entry)
    check(fn(*(0 if a is None else a.data_ptr() if hasattr(a, "data_ptr") else a for a in args)), entry)


def check(rc: int, what: str):
    if rc == 0:
        return
    lib = load()
    if rc < 0:
        raise ValueError(f"{what}: {lib.hmv_last_error().decode()} (code {rc})")
    raise RuntimeError(f"{what}: HIP error {rc}")
