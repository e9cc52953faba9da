"""ctypes loader for libspeinet_hip.so — the C-ABI declared in include/speinet_hip.h.

The product path has no CPU fallback: if the library is missing or a call fails, a RuntimeError is raised.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libspeinet_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "speinet_hip.h")

_lib = None

# the scalar C types the header uses -> ctypes; a pointer parameter of any kind is c_void_p, a `const char*` return c_char_p
_SCALARS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "float": C.c_float, "spei_stream_t": C.c_void_p}
_DECL = re.compile(r"([^;{}()]*?)\b(spei_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")


def _strip(text: str) -> str:
    """Header text without comments and preprocessor lines."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return re.sub(r"^\s*#.*$", "", text, flags=re.M)


def _ctype(decl: str, param: bool):
    """ctypes type of one parameter (`const float* a0`, `int64_t n`) or of a return type; raises on a type it does not know."""
    toks = [t for t in decl.replace("*", " * ").split() if t != "const"]
    if "*" in toks:
        if param:
            return C.c_void_p
        if toks == ["char", "*"]:
            return C.c_char_p
    else:
        if param and len(toks) > 1:
            toks = toks[:-1]                               # the parameter's name
        if " ".join(toks) in _SCALARS:
            return _SCALARS[" ".join(toks)]
    raise ValueError(f"include/speinet_hip.h: no ctypes mapping for {'parameter' if param else 'return type'} {decl.strip()!r}")


def parse_header(text: str) -> dict:
    """name -> (restype, argtypes) of every `spei_*` function declared in the header text."""
    out = {}
    for ret, name, args in _DECL.findall(_strip(text)):
        args = args.strip()
        out[name] = (_ctype(ret, False), [] if args in ("", "void") else [_ctype(a, True) for a in args.split(",")])
    return out


# name -> (restype, argtypes): include/speinet_hip.h is the one declaration of the C-ABI
SIGNATURES = parse_header(open(HEADER_PATH).read())


def header_symbols() -> list:
    """Entry points declared in include/speinet_hip.h (parsed from the header text)."""
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(spei_[a-z0-9_]+)\s*\(", text)) - {"spei_stream_t"})


def lib():
    """Load (once) and return the shared library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m speinet_amd.build` (hipcc --offload-arch=gfx950). "
                "speinet_amd has no CPU fallback.")
        # torch ships its own libamdhip64.so.7; it must be in the process BEFORE this library is loaded so
        # both resolve to ONE HIP runtime (same SONAME) and share device pointers and streams.
        import torch  # noqa: F401
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        _lib = h
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {lib().spei_last_error().decode()}")
