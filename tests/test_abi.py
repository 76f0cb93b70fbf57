"""The boundary between Python and libnerflidar_hip.so: include/nerflidar_hip.h is the only statement of the C ABI.  `_lib` reads the
prototypes from it, the C compiler confirms the hand-written ctypes structs field by field (tests/abi_layout_check.c), and `_lib.call`
refuses a wrong argument before the library is loaded.  No GPU and no library except in the last test."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from nerflidar_hip import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = open(os.path.join(ROOT, "include", "nerflidar_hip.h")).read()
CODE = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)


# ---- parse ------------------------------------------------------------------------------------------------------------------------------
def test_parser_finds_every_declared_function():
    declared = set(re.findall(r"\b(nlr_[a-z_0-9]+)\s*\(", CODE))   # the regex of test_library.py
    sigs = _lib.signatures()
    assert declared and set(sigs) == declared and set(_lib.EXPORTS) == declared
    for name, s in sigs.items():
        assert s.name == name and name in s.prototype and s.prototype.endswith(");")
        assert all(p.name and p.ctype is not None for p in s.params)

    s = sigs["nlr_obj_frame_backward"]
    assert len(s.params) == 20 and s.params[10].decl == "const int32_t *ray_idx" and s.params[10].name == "ray_idx"
    assert (s.params[10].pointee, s.params[10].const, s.params[10].kind) == ("int32_t", True, "device")
    assert s.params[-1].decl == "void *stream" and s.launcher and s.restype is C.c_int
    p = sigs["nlr_hash_decay_forward"].params[4]
    assert p.decl == "double *level_sumsq" and p.pointee == "double" and not p.const
    p = sigs["nlr_model_create"].params[1]
    assert p.decl == "NlrModel **out" and p.ctype is C.POINTER(C.c_void_p)
    assert sigs["nlr_model_create"].params[0].ctype is C.POINTER(_lib.NlrModelDesc)
    s = sigs["nlr_grid_backward_workspace_bytes"]
    assert s.returns == "size_t" and s.restype is C.c_size_t and not s.launcher
    assert [(p.name, p.kind) for p in s.params if p.name.endswith("_host")] == [("offsets_host", "host")]
    assert sigs["nlr_last_error"].restype is C.c_char_p and sigs["nlr_last_error"].params == ()
    assert sigs["nlr_model_destroy"].restype is None
    # what `call` takes: a status and the stream last
    assert all((s.returns == "int" and s.params[-1].name == "stream") == s.launcher for s in sigs.values() if s.params)


def test_defines_are_the_headers():
    d = _lib.defines(HEADER)
    assert d == {k: int(v) for k, v in re.findall(r"#define\s+(NLR_\w+)\s+(\d+)", CODE)} and len(d) >= 14
    assert (_lib.NLR_MAX_LEVELS, _lib.NLR_MAX_VIEW_DEPTH) == (d["NLR_MAX_LEVELS"], d["NLR_MAX_VIEW_DEPTH"])
    for k, v in d.items():
        if k.startswith("NLR_DBG_"):
            assert getattr(_lib, k[4:]) == v, k


@pytest.mark.parametrize("bad", ["int nlr_new_thing(const float *x, long n, void *stream);",
                                 "int nlr_new_thing(const NlrUnbound *desc, void *stream);",
                                 "int nlr_new_thing(float ***x);",
                                 "unsigned nlr_new_thing(void);"])
def test_unknown_type_is_refused_with_the_prototype(bad):
    with pytest.raises(RuntimeError) as e:
        _lib.signatures(HEADER.replace("int nlr_version(void);", "int nlr_version(void);\n" + bad))
    assert bad in str(e.value)


# ---- layout -----------------------------------------------------------------------------------------------------------------------------
def _header_fields():
    """Struct -> field names, from the header's text."""
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", CODE, flags=re.S):
        out[name] = [re.search(r"(\w+)\s*(?:\[[^\]]*\])?\s*$", part).group(1) for decl in body.split(";") if decl.strip()
                     for part in decl.split(",")]
    return out


def test_struct_layouts_match_the_c_compiler(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no host C compiler"
    exe = str(tmp_path / "abi_layout_check")
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "abi_layout_check.c"), "-o", exe],
                   check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    c_sizes = {m[1]: int(m[2]) for m in (re.fullmatch(r"(\w+) sizeof (\d+)", l) for l in lines) if m}
    c_fields = {}
    for m in (re.fullmatch(r"(\w+)\.(\w+) (\d+) (\d+)", l) for l in lines):
        if m:
            c_fields.setdefault(m[1], []).append((m[2], int(m[3]), int(m[4])))
    hdr = _header_fields()
    assert set(hdr) == set(c_sizes) == set(c_fields) == set(_lib.STRUCTS) and len(hdr) == 10
    for name, cls in _lib.STRUCTS.items():
        py = [(f[0], getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_]
        assert [f[0] for f in c_fields[name]] == hdr[name], f"{name}: tests/abi_layout_check.c and the header list different fields"
        assert py == c_fields[name], f"{name}: ctypes (name, offset, size) {py} != C {c_fields[name]}"
        assert C.sizeof(cls) == c_sizes[name], name


# ---- refusals: nothing is loaded, nothing is launched --------------------------------------------------------------------------------
class _Loaded(Exception):
    pass


@pytest.fixture
def no_lib(monkeypatch):
    def lib():
        raise _Loaded("lib() entered")
    monkeypatch.setattr(_lib, "lib", lib)


def _box(**over):
    """nlr_track_box_params(tracks, timestamps, N, n_obj, T, box_params) with NULL for every pointer but those given."""
    a = dict(tracks=None, timestamps=None, N=3, n_obj=2, T=2, box_params=None)
    a.update(over)
    return ["nlr_track_box_params"] + list(a.values())


def test_call_refuses_before_the_library_is_touched(no_lib):
    f, dev = torch.zeros(4, 6), "cuda:0"
    cases = [   # (parameter the refusal must name, what it expected, the call)
        ("tracks", "torch.float32", _box(tracks=torch.zeros(2, 2, 9, dtype=torch.float64))),                 # float64 for `const float *`
        ("ray_idx", "torch.int32", ["nlr_obj_frame_backward", None, None, None, None, None, None, 4, 5, 2, 2,
                                    torch.zeros(3, dtype=torch.int64), None, None, 3, None, None, None, None, 0]),  # int64 for `const int32_t *`
        ("box_params", "contiguous", _box(box_params=torch.zeros(3, 2, 16)[:, :, ::2])),                     # a strided view
        ("timestamps", "a CUDA tensor (no CPU fallback)", _box(timestamps=torch.zeros(3))),                  # CPU memory for a device parameter
        ("offsets_host", "torch.int32", ["nlr_hash_decay_forward", None, np.zeros(3, np.int64), 2, 2, None]),   # numpy, wrong dtype
        ("desc", "NlrModelDesc", ["nlr_model_create", _lib.NlrRays(), C.c_void_p(None)]),                    # another struct
    ]
    for param, expected, (name, *args) in cases:
        with pytest.raises(RuntimeError) as e:
            _lib.call(name, *args, device=dev)
        msg = str(e.value)
        assert msg.startswith(f"{name}: {param} (`") and expected in msg and ", got a " in msg, msg
    with pytest.raises(RuntimeError, match=r"nlr_track_box_params: takes 6 arguments before the stream \(tracks, .*box_params\), got 5"):
        _lib.call(*_box()[:-1], device=dev)                                                                  # too few
    with pytest.raises(RuntimeError, match="nlr_track_box_params: no tensor argument to take the device from"):
        _lib.call(*_box())                                                                                   # no tensor, no device=
    with pytest.raises(RuntimeError, match="nlr_workspace_bytes: not a launcher"):
        _lib.call("nlr_workspace_bytes", None, 4, device=dev)
    # the whole message: function, parameter as the header declares it, expected, found
    with pytest.raises(RuntimeError, match=r"nlr_track_box_params: tracks \(`const float \*tracks`\) must be a torch.float32 tensor, got a torch.float64 "
                                           r"tensor of shape \(2, 2, 9\)"):
        _lib.call(*_box(tracks=torch.zeros(2, 2, 9, dtype=torch.float64)), device=dev)
    # a tensor on the host where the header declares host memory passes the checks
    with pytest.raises(_Loaded):
        _lib.call("nlr_hash_decay_forward", None, torch.zeros(3, dtype=torch.int32), 2, 2, None, device=dev)
    with pytest.raises(_Loaded):
        _lib.call("nlr_hash_decay_forward", None, np.zeros(3, np.int32), 2, 2, None, device=dev)


def test_none_is_null_for_every_pointer(no_lib):
    for name, s in _lib.signatures().items():
        if s.launcher:
            args = [None if p.pointee else 1 for p in s.params[:-1]]
            with pytest.raises(_Loaded):   # every check passed: the next step is the library
                _lib.call(name, *args, device="cuda:0")


def test_rays_keys_and_refusals():
    from nerflidar_hip import models
    assert _lib.RAY_KEYS == tuple(f[0] for f in _lib.NlrRays._fields_) == models._RAY_KEYS
    batch = {k: torch.zeros(4, 3) for k in _lib.RAY_KEYS}
    with pytest.raises(RuntimeError, match=r"batch\['origins'\] must be a CUDA tensor \(no CPU fallback\)"):
        _lib.rays(batch, 4)
    del batch["viewdirs"], batch["origins"]
    with pytest.raises(RuntimeError, match=r"batch\['origins'\] is missing"):
        _lib.rays(batch, 4, optional=("viewdirs",))


# ---- one launch through both spellings -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_call_launches_what_the_raw_spelling_launches():
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    tracks = torch.rand(2, 2, 9, generator=g)
    tracks[:, 0, 7], tracks[:, 1, 7] = 0.0, 1.0                      # the two recorded poses' timestamps
    tracks, ts = tracks.to(dev), torch.tensor([0.1, 0.5, 0.9], device=dev)
    raw, via = torch.full((3, 2, 8), -7.0, device=dev), torch.full((3, 2, 8), -7.0, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nlr_track_box_params(_lib.ptr(tracks), _lib.ptr(ts), 3, 2, 2, _lib.ptr(raw), _lib.current_stream()), "raw")
    _lib.call("nlr_track_box_params", tracks, ts, 3, 2, 2, via)
    assert not bool((raw == -7.0).any()) and torch.equal(raw.view(torch.int32), via.view(torch.int32))
    wide = torch.full((3, 2, 16), -7.0, device=dev)
    with pytest.raises(RuntimeError, match="box_params.*contiguous"):
        _lib.call("nlr_track_box_params", tracks, ts, 3, 2, 2, wide[:, :, ::2])
    torch.cuda.synchronize()
    assert bool((wide == -7.0).all())
