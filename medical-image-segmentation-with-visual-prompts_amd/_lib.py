"""ctypes binding of libmivp_hip.so (the C ABI declared in include/mivp.h).

The header is the prototype table: ``lib()`` parses it once and sets ``restype`` and ``argtypes`` on every function it
declares, so call sites pass plain Python numbers and ctypes converts them to the declared widths (or refuses them).
``call`` also refuses an undeclared name and an argument count other than the prototype's -- a cdecl function would take
surplus arguments silently.

The product path has NO fallback: if the library is missing or a call fails,
a RuntimeError is raised.  Tensors are passed as raw device pointers
(``tensor.data_ptr()``) plus the current torch HIP stream.
"""
import ctypes as C
import os
import re

import torch

from .build import HEADER

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmivp_hip.so")
ABI_VERSION = 18

i32, f32, vp, i64 = C.c_int32, C.c_float, C.c_void_p, C.c_int64


class SwinDesc(C.Structure):
    _fields_ = [(n, i32) for n in ("B", "C", "heads", "vol_in", "vol_out", "P", "Nq", "Nqp", "Np", "Npp", "Nkp",
                                   "aug", "augp", "has_mask")] + [("win", i32 * 3), ("q_scale", f32), ("ln_eps", f32),
                                                                  ("attn_drop_thr", C.c_uint32), ("attn_drop_scale", f32),
                                                                  ("attn_seed", C.c_uint32), ("proj_drop_thr", C.c_uint32),
                                                                  ("proj_drop_scale", f32), ("proj_seed", C.c_uint32),
                                                                  ("seed_epoch", C.c_void_p)]


class MergeDesc(C.Structure):
    _fields_ = [("B", i32), ("C", i32), ("dims", i32 * 3), ("odims", i32 * 3), ("merge_last", i32), ("Cout", i32),
                ("ln_eps", f32)]


class ConvDesc(C.Structure):
    _fields_ = [("B", i32), ("dims", i32 * 3), ("Cin", i32), ("Cout", i32), ("Kp", i32), ("pro_affine", i32),
                ("pro_lrelu", i32), ("add_residual", i32), ("out_f32", i32)]


class EmbedDesc(C.Structure):
    _fields_ = [("B", i32), ("Cin", i32), ("dims", i32 * 3), ("C", i32), ("nblk", i32)]


class UpcatDesc(C.Structure):
    _fields_ = [("B", i32), ("idims", i32 * 3), ("odims", i32 * 3), ("scale", i32 * 3), ("Cx", i32), ("Cs", i32),
                ("align_corners", i32)]


class OperandDesc(C.Structure):
    _fields_ = [("mode", i32), ("ld", i32), ("rows", i32), ("hd", i32), ("dims", i32 * 3), ("cin", i32)]


class GemmTnDesc(C.Structure):
    _fields_ = [("T", i64), ("M", i32), ("N", i32), ("a", OperandDesc), ("b", OperandDesc), ("alpha", f32),
                ("accumulate", i32), ("perm_cin", i32)]


class RegionTable(C.Structure):
    _fields_ = [("capacity", i32), ("image_dtype", i32)] + [
        (k, C.c_void_p) for k in ("n", "overflow", "cls", "size", "first", "bbox", "coord_sum", "vmin", "vmax", "vsum",
                                  "vsqsum")]


# ---------------------------------------------------------------------------------------------
# prototypes: the whole type vocabulary of include/mivp.h
# ---------------------------------------------------------------------------------------------
_SCALARS = {"int": C.c_int, "int32_t": i32, "uint32_t": C.c_uint32, "int64_t": i64, "size_t": C.c_size_t, "float": f32,
            "double": C.c_double}
_MIRRORS = {"Mivp" + cls.__name__: cls for cls in (SwinDesc, MergeDesc, ConvDesc, EmbedDesc, UpcatDesc, OperandDesc,
                                                   GemmTnDesc, RegionTable)}
_POINTEES = {"void", "float", "uint8_t", "int32_t", "uint32_t", "int64_t", "uint64_t"}     # of T* and T* const*
_RETURNS = {"int": C.c_int, "size_t": C.c_size_t, "char*": C.c_char_p}
_PROTO = re.compile(r"([\w\s*]+?)\b(mivp_\w+)\s*\(([^()]*)\)\s*;")


def _ctype(decl, fn):
    """ctypes type of one parameter declaration ``type name``; an unknown type is an error, never a silent void*."""
    m = re.fullmatch(r"(.*[\s*])\w+", decl.strip(), flags=re.S)
    t = re.sub(r"\bconst\b|\s", "", m.group(1)) if m else ""
    base, stars = t.rstrip("*"), len(t) - len(t.rstrip("*"))
    if t in _SCALARS:
        return _SCALARS[t]
    if t == "mivp_stream_t" or (base in _POINTEES and stars in (1, 2)):
        return vp
    if base in _MIRRORS and stars == 1:
        return C.POINTER(_MIRRORS[base])
    raise RuntimeError(f"mivp_amd: {fn}: parameter '{decl.strip()}' of mivp.h has a type this binding does not know")


def parse_header(path=HEADER):
    """{name: (restype, [argtypes])} of every function the header declares."""
    if not os.path.exists(path):
        raise RuntimeError(f"mivp_amd: {path} is missing. The binding takes every prototype from that header, so it has "
                           "to sit next to the package (include/mivp.h of the source tree).")
    with open(path) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)                    # comments
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)                                # preprocessor lines
    text = re.sub(r"typedef\s+struct\b[^{;]*\{[^}]*\}[^;]*;", "", text)             # descriptor structs
    protos = {}
    for ret, fn, params in _PROTO.findall(text):
        ret = re.sub(r"\bconst\b|\s", "", ret)
        if ret not in _RETURNS:
            raise RuntimeError(f"mivp_amd: {fn}: return type '{ret}' of mivp.h is unknown to this binding")
        params = [] if params.strip() in ("", "void") else params.split(",")
        protos[fn] = (_RETURNS[ret], [_ctype(p, fn) for p in params])
    return protos


_lib = None
_fns = {}          # name -> (bound function, number of parameters): what `call` looks at


def lib():
    """Load the shared library once and bind every prototype of the header; fail loudly if it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"mivp_amd: {LIB_PATH} is missing. Build it with `python __graft_entry__.py` "
                "(hipcc --offload-arch=gfx950). There is no CPU or PyTorch fallback for the hot path.")
        so = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in parse_header().items():
            fn = getattr(so, name)
            fn.restype, fn.argtypes = restype, argtypes
            _fns[name] = (fn, len(argtypes))
        ver = so.mivp_abi_version()
        if ver != ABI_VERSION:
            raise RuntimeError(f"mivp_amd: ABI version mismatch: library {ver}, binding {ABI_VERSION}")
        _lib = so
    return _lib


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream():
    """The current HIP stream of the current device as a plain int, like ``ptr`` (every kernel is launched on it).  The raw getter is
    ~10x cheaper than building a torch.cuda.Stream object per launch (80+ launches per step)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    """Device address of a tensor as a plain int (None -> None, which a pointer parameter takes as NULL).  Tensors must be
    contiguous.  Not a ``c_void_p``: every function has ``argtypes``, and converting an int is what costs least per launch
    (a ``c_void_p`` object per pointer made a 14-argument call about 1 us dearer)."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise RuntimeError("mivp_amd: non-contiguous tensor passed to the C ABI")
    if not t.is_cuda:
        raise RuntimeError("mivp_amd: the HIP kernels need device tensors (no CPU fallback; the CPU oracle "
                           "lives in oracle/ and is test infrastructure only)")
    return t.data_ptr()


def call(name, *args):
    if _lib is None:
        lib()
    try:
        fn, n = _fns[name]
    except KeyError:
        raise RuntimeError(f"mivp_amd: {name} is not declared in mivp.h") from None
    if len(args) != n:
        raise TypeError(f"mivp_amd: {name} takes {n} arguments (mivp.h), {len(args)} given")
    rc = fn(*args)
    if rc != 0:
        raise RuntimeError(f"mivp_amd: {name} failed with code {rc}: {lib().mivp_last_error().decode()}")


# ---------------------------------------------------------------------------------------------
# optional per-kernel timing (bench.py): HIP events on the stream the kernel is launched on
# ---------------------------------------------------------------------------------------------
_prof = {"on": False, "sel": {}}          # key -> {"names": (...), "pred": callable | None, "events": [], "desc": ..., "entry": ...}


def profile_select(name, pred=None, key="roofline"):
    """Time every call of C-ABI entry ``name`` (a name or a tuple of names) whose ctypes args satisfy ``pred`` while
    profiling is on; several selections can be active under different ``key``s."""
    _prof["sel"][key] = {"names": (name,) if isinstance(name, str) else tuple(name), "pred": pred, "events": [],
                         "desc": None, "entry": None}


def profile_reset(on: bool):
    if on:
        for s in _prof["sel"].values():
            s["events"] = []
    _prof["on"] = on


def profile_result(key="roofline"):
    """(mean launch duration in ms, launches, descriptor of the last timed launch); ``profile_entry(key)`` names it."""
    s = _prof["sel"].get(key)
    if not s or not s["events"]:
        return 0.0, 0, None
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in s["events"]]
    return sum(ms) / len(ms), len(ms), s["desc"]


def profile_entry(key="roofline"):
    s = _prof["sel"].get(key)
    return s["entry"] if s else None


_plain_call = call


def call(name, *args):  # noqa: F811  (wraps the plain call with the optional event pair)
    if _prof["on"]:
        for s in _prof["sel"].values():
            if name in s["names"] and (s["pred"] is None or s["pred"](args)):
                a = torch.cuda.Event(enable_timing=True)
                b = torch.cuda.Event(enable_timing=True)
                a.record()
                _plain_call(name, *args)
                b.record()
                s["events"].append((a, b))
                d = args[0]._obj
                s["desc"] = type(d).from_buffer_copy(d)
                s["entry"] = name
                return
    _plain_call(name, *args)
