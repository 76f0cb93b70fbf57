"""ctypes binding of libnerflidar_hip.so.  include/nerflidar_hip.h is the only statement of the C ABI: the prototypes and the integer
`#define`s are read from it when this module is imported, `lib()` sets every function's argtypes / restype from them, and `call`
checks the arguments of a launch against the same table before anything is loaded or launched.

There is no CPU fallback: if the shared object is missing or a call fails, this raises.  Build it
with `make -C nerf-lidar_amd` (or `python -c "import __graft_entry__ as g; g.build()"`).
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NLR_LIB_PATH") or os.path.join(_HERE, "libnerflidar_hip.so")  # override: diagnostic builds only
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "nerflidar_hip.h")  # as buildinfo.kernel_source_files


def _code(text: str) -> str:
    """The header without its comments (they name kernels and Python helpers too); line breaks stay where they were."""
    return re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: " " + "\n" * m.group(0).count("\n"), text, flags=re.S)


def defines(text: str) -> Dict[str, int]:
    """Every `#define NLR_* <integer>` of a header text."""
    return {k: int(v, 0) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(NLR_\w+)[ \t]+(-?\w+)[ \t]*$", _code(text), flags=re.M)
            if re.fullmatch(r"-?(0[xX][0-9a-fA-F]+|\d+)", v)}


_HEADER = open(HEADER_PATH).read()
DEFINES = defines(_HEADER)
NLR_MAX_LEVELS, NLR_MAX_GRID_LEVELS, NLR_MAX_VIEW_DEPTH = (DEFINES[k] for k in ("NLR_MAX_LEVELS", "NLR_MAX_GRID_LEVELS", "NLR_MAX_VIEW_DEPTH"))
# switches 0..6, then read-backs (nlr_debug_get): LAST_ROUTE = how the last level of the most recent render ran; TRAIN_* = the most
# recent nlr_mlp_train_forward / _backward (or _split) call: route = TRAIN_FULL | TRAIN_TRUNK | TRAIN_BWD, and the first row / row
# count the trunk-and-heads instance ran on
(DBG_FORCE_GENERIC, DBG_MLP_WORKGROUPS, DBG_BINNED_C4, DBG_NO_XPAIR_SCATTER, DBG_SCATTER_LEVELS, DBG_NO_SCATTER_CACHE, DBG_RAY_GROUPS,
 DBG_LAST_ROUTE, DBG_TRAIN_ROUTE, DBG_TRAIN_TRUNK_ROW0, DBG_TRAIN_TRUNK_ROWS) = (DEFINES["NLR_" + k] for k in (
     "DBG_FORCE_GENERIC", "DBG_MLP_WORKGROUPS", "DBG_BINNED_C4", "DBG_NO_XPAIR_SCATTER", "DBG_SCATTER_LEVELS", "DBG_NO_SCATTER_CACHE",
     "DBG_RAY_GROUPS", "DBG_LAST_ROUTE", "DBG_TRAIN_ROUTE", "DBG_TRAIN_TRUNK_ROW0", "DBG_TRAIN_TRUNK_ROWS"))
# not `#define`s of the header (its NLR_PREC_* and NLR_K_COUNT are enumerators, the route values live in its comments): literals
PREC_F32, PREC_MIXED, PREC_FAST = 0, 1, 2
NLR_K_COUNT = 6
ROUTE_FULL, ROUTE_FULL_FUSED, ROUTE_LIDAR, ROUTE_LIDAR_FUSED = 1, 2, 3, 4
TRAIN_FULL, TRAIN_TRUNK, TRAIN_BWD = 1, 2, 4

c_fp = C.c_void_p  # device / host pointers travel as integers


# ---- the structs of the header, by hand (tests/test_abi.py compares every field's offset and size with the C compiler's) ------------
class NlrLinear(C.Structure):
    _fields_ = [("weight", c_fp), ("bias", c_fp), ("out_features", C.c_uint32), ("in_features", C.c_uint32)]


class NlrGridDesc(C.Structure):
    _fields_ = [("table", c_fp), ("table_dtype", C.c_int32), ("num_levels", C.c_uint32), ("level_dim", C.c_uint32),
                ("base_resolution", C.c_uint32), ("log2_per_level_scale", C.c_float), ("offsets", c_fp),
                ("gridtype", C.c_uint32), ("align_corners", C.c_uint32), ("interp", C.c_uint32)]


class NlrMlpDesc(C.Structure):
    _fields_ = [("grid", NlrGridDesc), ("density0", NlrLinear), ("density2", NlrLinear), ("disable_rgb", C.c_uint32),
                ("bottleneck_width", C.c_uint32), ("net_depth_viewdirs", C.c_uint32), ("net_width_viewdirs", C.c_uint32),
                ("skip_layer_dir", C.c_uint32), ("deg_view", C.c_uint32), ("view", NlrLinear * NLR_MAX_VIEW_DEPTH),
                ("rgb_layer", NlrLinear), ("use_semantic", C.c_uint32), ("no_sem_layer", C.c_uint32),
                ("class_num", C.c_uint32), ("sem0", NlrLinear), ("sem2", NlrLinear), ("use_intensity", C.c_uint32),
                ("int0", NlrLinear), ("int2", NlrLinear), ("density_bias", C.c_float), ("rgb_premultiplier", C.c_float),
                ("rgb_bias", C.c_float), ("rgb_padding", C.c_float), ("re_weights", C.c_uint32)]


class NlrObjClassDesc(C.Structure):
    _fields_ = [("mlp", NlrMlpDesc), ("latent_size", C.c_uint32), ("split_latent", C.c_uint32), ("class_type", C.c_int32)]


class NlrObjectsDesc(C.Structure):
    _fields_ = [("n_classes", C.c_uint32), ("classes", C.POINTER(NlrObjClassDesc)), ("n_tracks", C.c_uint32), ("track_class", c_fp),
                ("latents", c_fp)]


class NlrModelDesc(C.Structure):
    _fields_ = [("num_levels", C.c_uint32), ("num_samples", C.c_uint32 * NLR_MAX_LEVELS),
                ("mlps", C.POINTER(NlrMlpDesc) * NLR_MAX_LEVELS), ("dilation_multiplier", C.c_float),
                ("dilation_bias", C.c_float), ("anneal_slope", C.c_float), ("resample_padding", C.c_float),
                ("power_lambda", C.c_float), ("std_scale", C.c_float), ("bg_intensity", C.c_float),
                ("opaque_background", C.c_uint32), ("mlp_precision", C.c_uint32)]


class NlrRays(C.Structure):
    _fields_ = [(k, c_fp) for k in ("origins", "directions", "viewdirs", "radii", "near", "far", "base_x", "base_y")]


RAY_KEYS = tuple(k for k, _ in NlrRays._fields_)  # the batch keys of a ray bundle


class NlrRenderCfg(C.Structure):
    _fields_ = [("train_frac", C.c_float), ("compute_extras", C.c_uint32), ("sample_n", C.c_uint32),
                ("sample_m", C.c_uint32), ("rand_jitter", c_fp * NLR_MAX_LEVELS), ("rand_deg", c_fp * NLR_MAX_LEVELS),
                ("scale_factor", C.c_float), ("shuffled_rays", C.c_uint32)]


class NlrLevelOut(C.Structure):
    _fields_ = [(k, c_fp) for k in ("sdist", "tdist", "weights", "density", "rgb", "semantic", "intensity", "depth", "r_rgb", "r_acc",
                                    "r_distance_mean", "r_distance_median", "r_distance_percentile_5", "r_distance_percentile_95")]


class NlrOut(C.Structure):
    _fields_ = [(k, c_fp) for k in ("rgb", "depth", "semantic", "intensity", "acc", "distance_mean", "distance_median",
                                    "distance_percentile_5", "distance_percentile_95", "labels", "points", "packed")] + \
               [("packed_h", C.c_uint32), ("packed_w", C.c_uint32), ("history", NlrLevelOut * NLR_MAX_LEVELS)]


STRUCTS = {c.__name__: c for c in (NlrLinear, NlrGridDesc, NlrMlpDesc, NlrObjClassDesc, NlrObjectsDesc, NlrModelDesc, NlrRays, NlrRenderCfg,
                                   NlrLevelOut, NlrOut)}


# ---- the prototypes of the header ---------------------------------------------------------------------------------------------------
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_RETURNS = {"void": None, "const char *": C.c_char_p, **_SCALARS}
# what a tensor behind a `T *` must hold (torch, numpy); void takes any
_POINTEE_DTYPE = {"float": (torch.float32, np.float32), "double": (torch.float64, np.float64), "int32_t": (torch.int32, np.int32),
                  "uint32_t": (torch.int32, np.int32), "uint8_t": (torch.uint8, np.uint8), "void": (None, None)}


class Param(NamedTuple):
    name: str                # as the header names it
    decl: str                # "const int32_t *ray_idx"
    pointee: Optional[str]   # base type of a pointer, None for a scalar
    const: bool
    ctype: object            # what argtypes gets
    kind: str                # how `call` treats it: int, float, device, host, struct, handle, handles


class Signature(NamedTuple):
    name: str
    returns: str             # "int", "size_t", "const char *", ...
    restype: object
    params: Tuple[Param, ...]
    prototype: str
    launcher: bool           # returns a status and ends in `void *stream`: what `call` takes


def signatures(text: Optional[str] = None) -> Dict[str, Signature]:
    """name -> Signature of every `nlr_*` prototype, of the header next to the package or of a header `text`.  Anything outside the
    ABI's vocabulary - int, int32_t, uint32_t, uint8_t (behind a pointer), float, double, size_t, void, const char *, pointers to those, to the bound structs, to
    the opaque handles, and `T **` - is an error that quotes the prototype: no type is ever guessed."""
    if text is None:
        return _SIGNATURES
    code = re.sub(r"^[ \t]*#.*$", " ", _code(text), flags=re.M)
    handles = set(re.findall(r"\btypedef\s+struct\s+(\w+)\s+\1\s*;", code))  # declared, never defined: opaque
    out = {}
    for m in re.finditer(r"([^;{}()]*?)\b(nlr_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", code):
        proto = " ".join(m.group(0).split())
        name = m.group(2)

        def refuse(what):
            raise RuntimeError(f"include/nerflidar_hip.h: {what} is outside the ABI's type vocabulary in `{proto}`")

        returns = " ".join(m.group(1).split())
        if returns not in _RETURNS:
            refuse(f"return type `{returns}`")
        params = []
        plist = " ".join(m.group(3).split())
        for decl in ([] if plist == "void" else plist.split(",")):
            pm = re.fullmatch(r"\s*(const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(\w+)\s*", decl)
            if not pm:
                refuse(f"parameter `{decl.strip()}`")
            const, base, depth, pname = bool(pm.group(1)), pm.group(2), pm.group(3).count("*"), pm.group(4)
            if depth == 0 and base in _SCALARS:
                ctype, kind = _SCALARS[base], "float" if base in ("float", "double") else "int"
            elif depth == 1 and base in _POINTEE_DTYPE:
                ctype, kind = c_fp, "host" if pname.endswith("_host") else "device"
            elif depth == 1 and base in STRUCTS:
                ctype, kind = C.POINTER(STRUCTS[base]), "struct"
            elif depth == 1 and base in handles:
                ctype, kind = c_fp, "handle"
            elif depth == 2 and (base in handles or base in _POINTEE_DTYPE):
                ctype, kind = C.POINTER(c_fp), "handles"
            else:
                refuse(f"parameter `{decl.strip()}`")
            norm = f"{'const ' if const else ''}{base} {'*' * depth}{pname}" if depth < 2 else " ".join(decl.split())
            params.append(Param(pname, norm, base if depth else None, const, ctype, kind))
        launcher = returns == "int" and bool(params) and params[-1].decl == "void *stream"
        out[name] = Signature(name, returns, _RETURNS[returns], tuple(params), proto, launcher)
    return out


_SIGNATURES = signatures(_HEADER)
EXPORTS = list(_SIGNATURES)

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: the HIP extension has not been built (make -C nerf-lidar_amd). "
                               "There is no CPU fallback for the render path.")
        L = C.CDLL(LIB_PATH)
        for sig in _SIGNATURES.values():
            fn = getattr(L, sig.name)
            fn.restype, fn.argtypes = sig.restype, [p.ctype for p in sig.params]
        _lib = L
    return _lib


def check(rc: int, what: str = ""):
    """Status -> RuntimeError with the library's message (the reference raises through TORCH_CHECK)."""
    if rc != 0:
        msg = lib().nlr_last_error().decode(errors="replace")
        raise RuntimeError(f"{what or 'libnerflidar_hip'} failed ({rc}): {msg}")


def ptr(t):
    """data_ptr of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def current_stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(name: str, *args, device=None) -> None:
    """Launch `name` - a function of the header that returns a status and ends in `void *stream` - with every argument but the
    stream.  The arguments are checked against the header's prototype before the library is touched; a refusal is a RuntimeError that
    names the function, the parameter as the header names it, what was expected and what was found.  This refuses, it does not
    repair: `.contiguous()`, `.float()`, `.int()` stay with the caller.
      None              NULL for any pointer (the library checks NULLs itself)
      T *               a contiguous CUDA tensor: float32 for float, float64 for double, int32 for int32_t / uint32_t, any dtype for
                        void; all of a call's tensors on one device
      T *name_host      a contiguous CPU tensor or numpy array of that dtype
      Struct *          an instance of the ctypes class, passed by reference
      Handle *          the c_void_p a *_create call filled;  T **: such a c_void_p (by reference) or an array of them
      scalars           through int() / float()
    The call runs inside `torch.cuda.device` of the tensors' device (`device=` when there is no tensor) on that device's current
    stream, and its status goes through `check`."""
    sig = _SIGNATURES.get(name)
    if sig is None or not sig.launcher:
        raise RuntimeError(f"{name}: not a launcher of include/nerflidar_hip.h (a status-returning function whose last parameter is the stream)")
    params = sig.params[:-1]
    if len(args) != len(params):
        raise RuntimeError(f"{name}: takes {len(params)} arguments before the stream ({', '.join(p.name for p in params)}), got {len(args)}")

    def refuse(p, expected, a):
        found = f"{a.dtype} tensor of shape {tuple(a.shape)}, strides {a.stride()} on {a.device}" if isinstance(a, torch.Tensor) else \
            f"{a.dtype} array of shape {a.shape}" if isinstance(a, np.ndarray) else type(a).__name__
        raise RuntimeError(f"{name}: {p.name} (`{p.decl}`) must be {expected}, got a {found}")

    dev, conv = None, []
    for p, a in zip(params, args):
        kind = p.kind
        if kind == "int":
            a = int(a)
        elif kind == "float":
            a = float(a)
        elif a is None:
            pass
        elif kind == "device" or kind == "host":
            dtype, np_dtype = _POINTEE_DTYPE[p.pointee]
            if kind == "host" and isinstance(a, np.ndarray):
                if (dtype is not None and a.dtype != np_dtype) or not a.flags.c_contiguous:
                    refuse(p, f"a contiguous {dtype} CPU tensor or numpy array", a)
                a = a.ctypes.data
            else:
                if not isinstance(a, torch.Tensor):
                    refuse(p, "a tensor or None", a)
                if dtype is not None and a.dtype != dtype:
                    refuse(p, f"a {dtype} tensor", a)
                if not a.is_contiguous():
                    refuse(p, "a contiguous tensor", a)
                if a.is_cuda == (kind == "host"):
                    refuse(p, "a CPU tensor or numpy array (host memory)" if kind == "host" else "a CUDA tensor (no CPU fallback)", a)
                if kind == "device":
                    if dev is None:
                        dev = a.device
                    elif a.device != dev:
                        refuse(p, f"on {dev} like the call's other tensors", a)
                a = a.data_ptr()
        elif kind == "struct":
            if not isinstance(a, p.ctype._type_):
                refuse(p, f"a {p.ctype._type_.__name__} or None", a)
            a = C.byref(a)
        elif kind == "handle":
            if not isinstance(a, (C.c_void_p, int)):
                refuse(p, "the c_void_p handle of a *_create call", a)
        else:  # handles: T **
            if isinstance(a, C.c_void_p):
                a = C.byref(a)
            elif not (isinstance(a, C.Array) and a._type_ is C.c_void_p):
                refuse(p, "a c_void_p (passed by reference) or an array of c_void_p", a)
        conv.append(a)
    if device is not None:
        device = torch.device(device)
        if dev is not None and device.index is not None and device != dev:
            raise RuntimeError(f"{name}: device={device}, but the tensors are on {dev}")
    dev = dev if dev is not None else device
    if dev is None:
        raise RuntimeError(f"{name}: no tensor argument to take the device from: pass device=")
    fn = getattr(lib(), name)
    with torch.cuda.device(dev):
        rc = fn(*conv, torch.cuda.current_stream(dev).cuda_stream)
    check(rc, name)


def rays(batch, n: int, optional=()):
    """(NlrRays, keep) of a batch of n rays: every key of RAY_KEYS as a contiguous float32 [n, -1] CUDA tensor; `keep` maps the keys
    to the tensors whose addresses the struct carries (hold it for as long as the struct is in use).  A key listed in `optional` may
    be absent and stays NULL (`viewdirs` of a LiDAR-only render)."""
    r, keep = NlrRays(), {}
    for k in RAY_KEYS:
        t = batch.get(k)
        if t is None:
            if k in optional:
                continue
            raise RuntimeError(f"batch['{k}'] is missing")
        if not t.is_cuda:
            raise RuntimeError(f"batch['{k}'] must be a CUDA tensor (no CPU fallback)")
        keep[k] = t = t.reshape(n, -1).contiguous().float()
        setattr(r, k, t.data_ptr())
    return r, keep
