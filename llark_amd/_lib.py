"""ctypes loader for ``libllark_hip.so`` (the C-ABI declared in ``include/llark_hip.h``).

The product path has NO CPU or PyTorch fallback: if the HIP library cannot be loaded this module
raises, and every op wrapper in :mod:`llark_amd.ops` goes through it.
"""
from __future__ import annotations

import ctypes
import os
import re
import subprocess
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_uint, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LLARK_HIP_LIB") or os.path.join(_HERE, "libllark_hip.so")   # override: profiling builds only
CSRC = os.path.join(_HERE, "csrc")

_lib = None


class LlarkHipError(RuntimeError):
    pass


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 into ``llark_amd/libllark_hip.so`` (hipcc cross-compiles
    without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    srcs.append(os.path.join(_HERE, "..", "include", "llark_hip.h"))
    stale = (not os.path.exists(LIB_PATH)) or any(
        os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs if os.path.exists(s)
    )
    if force or stale:
        cmd = ["make", "-C", CSRC, "-j8"] + (["-B"] if force else [])
        res = subprocess.run(cmd, capture_output=not verbose, text=True)
        if res.returncode != 0:
            raise LlarkHipError(f"building libllark_hip.so failed:\n{res.stdout}\n{res.stderr}")
    return LIB_PATH


# ---- the C ABI, read from include/llark_hip.h: the header is the only place a signature is written down ----------------
HEADER = os.path.join(_HERE, "..", "include", "llark_hip.h")
_CTYPES = {"int": c_int, "int64_t": c_int64, "long long": c_int64, "unsigned": c_uint, "float": c_float, "double": c_double,
           "llark_stream_t": c_void_p, "llark_workspace_t": c_void_p}
_PROTO = re.compile(r"(?:\A|(?<=[;{}]))\s*([\w\s*]+?)\s*\b(llark_\w+)\s*\(([^()]*)\)\s*;")


def _ctype(decl: str, proto: str, param: bool):
    """ctypes type of one parameter declaration (``param``) or of a return type; an unknown type raises."""
    tok = re.findall(r"\w+|\*|\[\s*\]", re.sub(r"\bconst\b", " ", decl))
    if param:                                   # drop the parameter's name; `T x[]` is `T* x`
        tok = tok[:-2] + ["*"] if tok and tok[-1][0] == "[" else tok[:-1]
    if "*" in tok:
        return c_char_p if tok[0] == "char" else c_void_p
    if tok == ["void"] and not param:
        return None
    if " ".join(tok) not in _CTYPES:
        raise LlarkHipError(f"include/llark_hip.h: unknown type in '{decl.strip()}' of `{proto}`")
    return _CTYPES[" ".join(tok)]


def parse_header(text: str) -> dict:
    """name -> (restype, argtypes, index of the llark_stream_t parameter or None) for every ``ret llark_name(params);`` of a C
    header.  Fails loudly: an unknown type, or a ``llark_name(`` the prototype pattern did not take, raises LlarkHipError."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    protos = {}
    for m in _PROTO.finditer(text):
        ret, name, params = m.groups()
        proto = " ".join(m.group(0).split())
        decls = [] if params.strip() in ("", "void") else params.split(",")
        stream = [i for i, d in enumerate(decls) if re.search(r"\bllark_stream_t\b", d)]
        protos[name] = (_ctype(ret, proto, False), [_ctype(d, proto, True) for d in decls], stream[0] if stream else None)
    mentioned = re.findall(r"\b(llark_\w+)\s*\(", text)
    if len(protos) != len(mentioned):
        raise LlarkHipError(f"include/llark_hip.h: {len(mentioned)} `llark_name(` but {len(protos)} prototypes parsed "
                            f"(not taken: {sorted(set(mentioned) - set(protos))})")
    return protos


def _read_header() -> str:
    try:
        with open(HEADER) as f:
            return f.read()
    except OSError as e:                        # no fallback table: without the header there are no signatures
        raise LlarkHipError(f"cannot read {HEADER}: {e}") from e


_PROTOS = parse_header(_read_header())
_SIGS = {name: p[1] for name, p in _PROTOS.items()}            # name -> argtypes
_STREAM_ARG = {name: p[2] for name, p in _PROTOS.items()}      # name -> position of the llark_stream_t parameter, or None


def declared_symbols():
    """Every symbol ``include/llark_hip.h`` declares."""
    return sorted(_PROTOS)


# ---- host-side launch lists -------------------------------------------------------------------------------------------
# A fixed-shape forward is the same sequence of C-ABI calls with the same pointers every time.  While a recorder is
# installed, lib() hands out a proxy that executes each call AND appends (function, name, args, timing label) to the
# recorder; ops.LaunchList.replay() then re-issues the list without re-deriving shapes, views or pointers in Python
# (the per-launch host cost drops from tens of microseconds to the ctypes call itself).  hipGraph replay of the same
# sequences measured slower than eager launches on ROCm 7.2 (profiles/r01_gemm_ablation.txt), hence a host list.
_recorder = None
current_label = None          # (name, work) of the ops._timed region the next call belongs to


class _RecordingProxy:
    def __init__(self, real, rec):
        self._real, self._rec = real, rec

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("llark_") or name == "llark_last_error":
            return fn
        rec = self._rec

        def call(*args):
            rc = fn(*args)
            rec.append((fn, name, args, current_label))
            return rc

        return call


def set_recorder(rec) -> None:
    global _recorder
    _recorder = rec


def lib():
    L = _real_lib()
    return _RecordingProxy(L, _recorder) if _recorder is not None else L


def _real_lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            # same image on the GPU box: hipcc is present, so a missing .so is built, never skipped
            build()
        try:
            L = ctypes.CDLL(LIB_PATH)
        except OSError as e:  # fail loudly: there is no fallback path
            raise LlarkHipError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (restype, argtypes, _) in _PROTOS.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = L
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().llark_last_error().decode("utf-8", "replace")
        raise LlarkHipError(f"{what or 'llark_hip'} failed (code {rc}): {msg}")
