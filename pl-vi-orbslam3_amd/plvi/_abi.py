"""The ABI layer of plvi: library loading, the ctypes signatures derived from include/plvi_frontend.h, device
buffers, and the small marshalling vocabulary every wrapper in plvi/__init__.py is written in.

A host form reads: ``table`` per input (contiguous, typed, rows of a fixed width), ``same_len`` per side (every
per-record array has that side's count), ``out`` per output (at least one cell), then one ``call`` by name.
"""
import ctypes
import os
import pathlib
import re
import sys

import numpy as np

_PKG = pathlib.Path(__file__).resolve().parent.parent
# PLVI_LIB: an alternative build of the same library (A/B experiments, tools/build_variant.sh)
LIB_PATH = pathlib.Path(os.environ["PLVI_LIB"]) if os.environ.get("PLVI_LIB") else _PKG / "lib" / "libplvi_frontend.so"
HEADER_PATH = _PKG.parent / "include" / "plvi_frontend.h"

PLVI_OK = 0
PLVI_E_EMPTY = -1
PLVI_E_BADARG = -2
PLVI_E_CAPACITY = -3
PLVI_E_HIP = -4
PLVI_E_OVERFLOW = -5
PLVI_E_SIZE = -6
PLVI_E_CAPTURE = -7

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
KEYLINE_DTYPE = np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"), ("pt_x", "<f4"),
                          ("pt_y", "<f4"), ("response", "<f4"), ("size", "<f4"), ("startPointX", "<f4"),
                          ("startPointY", "<f4"), ("endPointX", "<f4"), ("endPointY", "<f4"),
                          ("sPointInOctaveX", "<f4"), ("sPointInOctaveY", "<f4"), ("ePointInOctaveX", "<f4"),
                          ("ePointInOctaveY", "<f4"), ("lineLength", "<f4"), ("numOfPixels", "<i4")])


class PlviError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what} failed with status {code}")
        self.code = code


# ------------------------------------------------------------ signatures
_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
            "double": ctypes.c_double}
_DECL = re.compile(r"^[ \t]*([A-Za-z_][\w \t\*]*?)\s*\b(plvi_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", re.M)
_NAME = re.compile(r"\b(plvi_[a-z0-9_]+)\s*\(")


def _ctype(decl, name, named, where):
    """The ctypes type of one C parameter (named) or return type: a pointer is c_void_p (const char* is
    c_char_p), int / unsigned / size_t / float / double are their scalars, anything else is refused."""
    words = decl.replace("*", " * ").split()
    if "*" in words:
        return ctypes.c_char_p if words[:3] == ["const", "char", "*"] and words.count("*") == 1 else ctypes.c_void_p
    words = [w for w in words if w != "const"]
    base = " ".join(words[:-1] if named and len(words) > 1 else words)
    if base not in _SCALARS:
        raise RuntimeError(f"{where}: {name}: no ctypes rule for `{decl.strip()}`")
    return _SCALARS[base]


def signatures(header=None):
    """{name: (argtypes, restype)} of every function declared in include/plvi_frontend.h (or `header`), the only
    statement of the ABI: load() applies it to the library.  Raises RuntimeError naming the symbol when a
    declaration is not understood -- a `plvi_*(` name without a parsed declaration, or a parameter outside
    _ctype's rule (a struct by value, a function pointer) -- instead of guessing a type."""
    path = pathlib.Path(header or HEADER_PATH)
    txt = path.read_text()
    names = sorted(set(_NAME.findall(txt)))
    txt = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", txt, flags=re.S))
    sig = {}
    for ret, name, params in _DECL.findall(txt):
        params = [p for p in params.split(",") if p.strip() not in ("", "void")]
        sig[name] = ([_ctype(p, name, True, path.name) for p in params], _ctype(ret, name, False, path.name))
    if sorted(sig) != names:
        raise RuntimeError(f"{path.name}: {len(sig)} declarations parsed for {len(names)} names; "
                           f"not understood: {sorted(set(names) ^ set(sig))}")
    return sig


def _declare(lib):
    for name, (args, res) in signatures().items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    return lib


_lib = None
_runtime = None

c_int_p = ctypes.POINTER(ctypes.c_int)
c_void_pp = ctypes.POINTER(ctypes.c_void_p)


def load(runtime=None):
    """Load the HIP library (raises if it was not built: there is no fallback).

    Which HIP runtime the library binds to is decided here, once per process:
    PyTorch's bundled libamdhip64 (HIP 7.0 on this image) and /opt/rocm's
    (7.2) share the SONAME libamdhip64.so.7, so whichever loads first serves
    both -- unless ours comes first and torch is imported later, in which case
    torch loads its own copy by file name and that second runtime finds no
    device.  `runtime`:

    * "torch": import torch first (one runtime for both).  On the 7.0 runtime
      `plvi_frame_extract_batch` / `plvi_stereo_frame_extract_batch` refuse
      stream capture with PLVI_E_CAPTURE; everything else
      behaves identically.
    * "system": do not import torch; the library binds to /opt/rocm's runtime
      (capture supported).  Do not import torch later in the same process.
    * None (default): "torch" if torch is already imported, else the
      PLVI_RUNTIME environment variable ("torch" / "system"; PLVI_NO_TORCH=1
      means "system"), else "torch" when torch is installed -- the safe choice
      for a process that may import torch later.
    """
    global _lib, _runtime
    if _lib is None:
        if runtime is None:
            if "torch" in sys.modules:
                runtime = "torch"
            elif os.environ.get("PLVI_NO_TORCH"):
                runtime = "system"
            else:
                runtime = os.environ.get("PLVI_RUNTIME", "torch")
        if runtime not in ("torch", "system"):
            raise ValueError(f"plvi.load: runtime must be 'torch' or 'system', not {runtime!r}")
        if runtime == "torch":
            try:
                import torch  # noqa: F401
            except ImportError:
                runtime = "system"
        if not LIB_PATH.exists():
            raise RuntimeError(f"{LIB_PATH} missing: build it with `make -C pl-vi-orbslam3_amd`")
        if not HEADER_PATH.exists():
            raise RuntimeError(f"{HEADER_PATH} missing: the ctypes signatures are derived from it")
        _lib = _declare(ctypes.CDLL(str(LIB_PATH)))
        _runtime = runtime
    elif runtime is not None and runtime != _runtime:
        raise RuntimeError(f"plvi.load: library already bound to the {_runtime!r} HIP runtime")
    return _lib


def bound_runtime():
    """'torch' or 'system': the HIP runtime the loaded library is bound to (None before load())."""
    return _runtime


def exported_symbols():
    """Function names declared in include/plvi_frontend.h."""
    return sorted(set(_NAME.findall(HEADER_PATH.read_text())))


# ------------------------------------------------------------ marshalling
def _check(rc, what):
    if rc < 0:
        raise PlviError(rc, what)
    return rc


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _arg(a):
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return ctypes.byref(a) if isinstance(a, ctypes.Structure) else a


def status(name, *args):
    """The entry point `name` called with an ndarray as its data pointer and a ctypes.Structure by reference;
    None (NULL), ints (counts, device addresses), floats and ctypes objects go through unchanged.  Returns the
    raw status."""
    return getattr(load(), name)(*[_arg(a) for a in args])


def call(name, *args):
    """status(), with a negative status raised as PlviError(name)."""
    return _check(status(name, *args), name)


def table(a, dtype, width=None):
    """A host table as the C side reads it: C-contiguous, of `dtype`, in rows of `width` (a flat array is
    folded; rows of another width are refused); KEYPOINT_DTYPE / KEYLINE_DTYPE are viewed.  None stays None."""
    if a is None:
        return None
    if dtype is KEYPOINT_DTYPE or dtype is KEYLINE_DTYPE:
        return np.ascontiguousarray(a).view(dtype)
    a = np.ascontiguousarray(a, dtype)
    if width is None:
        return a
    if a.ndim == 2 and a.shape[1] != width:
        raise ValueError(f"table rows are {a.shape[1]} wide, expected {width}")
    return a.reshape(-1, width)


def same_len(n, **arrays):
    """The C entry points read n records from every host array: refuse a shorter (or longer) one
    instead of letting hipMemcpy read past its end.  None (an optional array) passes."""
    for name, a in arrays.items():
        if a is not None and len(a) != n:
            raise ValueError(f"{name} has {len(a)} records, expected {n}")



def out(n, fill, dtype=np.int32, width=None):
    """A host output of n records pre-filled with `fill`, at least one record long (slice it to [:n])."""
    return np.full(max(n, 1) if width is None else (max(n, 1), width), fill, dtype)


class DeviceBuffer:
    """hipMalloc'd buffer owned from Python (no torch needed)."""

    def __init__(self, nbytes):
        p = ctypes.c_void_p()
        call("plvi_device_malloc", ctypes.byref(p), max(1, nbytes))
        self._lib = load()
        self.ptr, self.nbytes = p.value, nbytes

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        call("plvi_memcpy", self.ptr, arr, arr.nbytes, 1)

    def download(self, arr, src_ptr=None):
        call("plvi_memcpy", arr, src_ptr or self.ptr, arr.nbytes, 2)
        return arr

    def __del__(self):
        try:
            if self.ptr:
                self._lib.plvi_device_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


def download(ptr, arr):
    """Copy device memory at `ptr` into numpy array `arr` (synchronous)."""
    call("plvi_memcpy", arr, ptr, arr.nbytes, 2)
    return arr


def to_device(*tables, counts=None):
    """One item through a batch form: each host table uploaded into a DeviceBuffer of capacity max(n, 1) records
    (an empty table is one zero record), and with `counts` a 16-byte int32 buffer [*counts, 0, ...] whose tail
    takes the call's output counts.  Returns (buffers, counts buffer or None)."""
    bufs = []
    for a in tables:
        a = a if len(a) else np.zeros((1,) + a.shape[1:], a.dtype)
        bufs.append(DeviceBuffer(a.nbytes))
        bufs[-1].upload(a)
    cnt = None
    if counts is not None:
        cnt = DeviceBuffer(16)
        cnt.upload(np.array(list(counts) + [0] * (4 - len(counts)), np.int32))
    return bufs, cnt
