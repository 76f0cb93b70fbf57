"""Rays without colour supervision in the fused training step (header section 6b, `_split`): rows ordered colour rays first,
rows [M_color, M) run the density trunk and the heads only - `nlr_mlp_train_forward_split` / `_backward_split` / `_wgrad_split`
through the C ABI against their unsplit twins and against float64 on the saved tensors, and `color_rays` of
`TrainableNerfLevel` / `TrainableModel` / `training_step` end to end.  Shapes and inputs are those of tests/test_mlp_wgrad.py."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import test_mlp_wgrad as tw
from nerflidar_hip import _lib, losses as nlosses, training as ntrain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nlr_mlp_train_forward_split", "nlr_mlp_train_backward_split", "nlr_mlp_train_wgrad_split")
SHAPES = [("C2", 32), ("REF", 32), ("P_W128I", 64), ("P_NOSEM", 32), ("P_D3", 32)]
# colour rays of the 24: none, M_color = 96 / 192 rows (not a multiple of 128), M_color = 256 / 512 rows (a multiple), all
COUNTS = [0, 3, 8, 24]
CASES = [(wl, S, n) for wl, S in SHAPES for n in COUNTS]
IDS = [f"{wl}-{S}-colour{n}" for wl, S, n in CASES]
NAN16 = 0x7FC1  # a quiet NaN of bf16 with a payload: "never written"


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------
def test_split_entry_points_declared_and_listed():
    hdr = open(os.path.join(ROOT, "include", "nerflidar_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    declared = set(re.findall(r"\b(nlr_[a-z_0-9]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW:
        assert name in declared, f"{name} not declared in include/nerflidar_hip.h"
        assert name in _lib.EXPORTS, f"{name} not in _lib.EXPORTS"
        assert hasattr(L, name), f"{name} not exported by the library"
        assert getattr(L, name).argtypes is not None, f"{name}: argtypes not declared in _lib"
    assert len(L.nlr_mlp_train_forward_split.argtypes) == len(L.nlr_mlp_train_forward.argtypes) + 1
    assert len(L.nlr_mlp_train_backward_split.argtypes) == len(L.nlr_mlp_train_backward.argtypes) + 1
    assert len(L.nlr_mlp_train_wgrad_split.argtypes) == len(L.nlr_mlp_train_wgrad.argtypes) + 1
    assert (_lib.DBG_TRAIN_ROUTE, _lib.DBG_TRAIN_TRUNK_ROW0, _lib.DBG_TRAIN_TRUNK_ROWS) == (8, 9, 10)


def test_color_rays_keyword_and_range():
    for fn in (ntrain.TrainableNerfLevel.forward, ntrain.TrainableModel.forward, ntrain.training_step):
        assert inspect.signature(fn).parameters["color_rays"].default is None, fn
    assert inspect.signature(ntrain.training_step).parameters["check_color_rays"].default is False
    assert ntrain._check_color_rays(None, 8) is None
    assert ntrain._check_color_rays(0, 8) == 0 and ntrain._check_color_rays(8, 8) == 8 and ntrain._check_color_rays(np.int64(3), 8) == 3
    for bad in (-1, 9, 2.0, "3", True):
        with pytest.raises(ValueError):
            ntrain._check_color_rays(bad, 8)
    # the modules refuse it before anything touches a device
    from nerflidar_hip import config as nconfig
    mc = nconfig.workload("REF", 12)
    lvl = ntrain.TrainableNerfLevel(mc.nerf_mlp)
    tdist = torch.zeros(8, 33)
    for bad in (-1, 9, 1.5):
        with pytest.raises(ValueError):
            lvl({}, tdist, color_rays=bad)
        with pytest.raises(ValueError):
            ntrain.TrainableModel(mc)({"origins": torch.zeros(8, 3)}, color_rays=bad)


def test_colourless_fraction_options_and_masks():
    import importlib.util
    from nerflidar_hip import scene as nscene, train_scene
    a = train_scene.build_parser().parse_args(["--out", "x"])
    assert a.colourless_fraction == 0.0
    a = train_scene.build_parser().parse_args(["--out", "x", "--colourless-fraction", "0.2", "--rays", "4096"])
    assert a.colourless_fraction == 0.2 and nlosses.colourless_count(a.rays, a.colourless_fraction) == 819
    spec = importlib.util.spec_from_file_location("train_step_bench", os.path.join(ROOT, "scripts", "train_step_bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)   # importing it runs nothing: the benchmark sits behind main()
    b = bench.build_parser().parse_args(["REF", "4096", "--colourless-fraction", "1.0"])
    assert (b.workload, b.rays, b.colourless_fraction) == ("REF", 4096, 1.0)
    assert bench.build_parser().parse_args([]).colourless_fraction == 0.0
    assert nlosses.colourless_count(10, 0.0) == 0 and nlosses.colourless_count(10, 0.25) == 2 and nlosses.colourless_count(10, 1.0) == 10
    with pytest.raises(ValueError):
        nlosses.colourless_count(10, 1.5)
    # masks: the suffix and only the suffix
    rays = nscene.random_lidar_rays(64, 0, 1, "cpu")
    sup = nscene.supervise(rays, colourless=16)
    assert sup["mask_rgb"].tolist() == [True] * 48 + [False] * 16 and torch.equal(sup["mask_rgb"], sup["sem_mask"])
    assert bool(sup["depth_mask"].all()) and bool(sup["lidar_mask"].all())
    assert bool(nscene.supervise(rays)["mask_rgb"].all())
    nlosses.check_colourless(sup, 48)
    for bad in (47, 0):
        with pytest.raises(ValueError):
            nlosses.check_colourless(sup, bad)
    with pytest.raises(ValueError):
        nscene.supervise(rays, colourless=65)
    m = bench.colourless_batch(dict(origins=torch.zeros(10, 3)), 3)
    assert m["mask_rgb"].tolist() == [True] * 7 + [False] * 3 and torch.equal(m["mask_rgb"], m["sem_mask"])


# ---- on the GPU: the C ABI -------------------------------------------------------------------------------------------------------
class Scene:
    pass


@functools.lru_cache(maxsize=None)
def _scene(wl, S):
    """One level per shape, run once through the UNSPLIT entry points (autograd path, fused_wgrad): its saved tensors are the
    reference of every comparison, its plan (tapes packed by that forward) serves the direct calls."""
    cfg, sd, batch, tdist, cot, N = tw._scene(wl, S)
    lvl = tw._run_level(cfg, sd, batch, tdist, cot, True)
    s = Scene()
    s.cfg, s.lvl, s.d, s.S, s.N, s.M = cfg, lvl, lvl._dbg, S, N, N * S
    s.K = cfg.class_num if cfg.use_semantic else 0
    W, WB, D = cfg.net_width_viewdirs, cfg.bottleneck_width, cfg.net_depth_viewdirs
    s.HH = (64 if s.K else 0) + (64 if cfg.use_intensity else 0)
    s.c_q, s.c_x = 64 + WB, 64 + WB + s.HH
    s.aw = s.c_x + D * W
    assert s.aw == lvl._plan.act_w
    cm = lambda t, c: t.reshape(s.M, c).t().contiguous()
    s.g = dict(density=cot["density"].reshape(s.M).contiguous(), rgb=cm(cot["rgb"], 3),
               sem=cm(cot["semantic"], s.K) if s.K else None, inten=cot["intensity"].reshape(s.M).contiguous() if cfg.use_intensity else None)
    # the unsplit backward through the C ABI on the same cotangents = what the autograd path saved
    rc, G, dF = _backward(s, None, s.d["acts"], s.g)
    assert rc == 0 and torch.equal(G.view(torch.int16), s.d["gacts"].view(torch.int16)) and torch.equal(dF, s.d["d_feat"])
    return s


def _nan16(*shape):
    return torch.full(shape, NAN16, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def _is_nan16(t):
    return bool((t.view(torch.int16) == NAN16).all())


def _forward(s, Mc, M=None, S=None, null=(), fill=None):
    """nlr_mlp_train_forward_split (Mc = None: the unsplit entry point) into pre-filled outputs."""
    d, plan = s.d, s.lvl._plan
    M = s.M if M is None else M
    new = lambda *sh: torch.full(sh, float("nan") if fill is None else fill, device="cuda")
    out = dict(density=new(s.M), rgb=new(3, s.M), sem=new(s.K, s.M) if s.K else None, inten=new(s.M) if s.cfg.use_intensity else None,
               acts=_nan16(s.M, s.aw) if fill is None else torch.full((s.M, s.aw), fill, dtype=torch.bfloat16, device="cuda"))
    a = dict(features=d["feats"], enc=d["enc"], **out)
    for k in null:
        a[k] = None
    L = _lib.lib()
    p = _lib.ptr
    if Mc is None:
        rc = L.nlr_mlp_train_forward(plan.handle, p(a["features"]), p(a["enc"]), M, s.S if S is None else S, p(a["density"]), p(a["rgb"]),
                                     p(a["sem"]), p(a["inten"]), p(a["acts"]), _lib.current_stream())
    else:
        rc = L.nlr_mlp_train_forward_split(plan.handle, p(a["features"]), p(a["enc"]), M, Mc, s.S if S is None else S, p(a["density"]),
                                           p(a["rgb"]), p(a["sem"]), p(a["inten"]), p(a["acts"]), _lib.current_stream())
    torch.cuda.synchronize()
    return rc, out


def _backward(s, Mc, acts, g, M=None, S=None, null=(), fill=None):
    d, plan = s.d, s.lvl._plan
    M = s.M if M is None else M
    gacts = _nan16(s.M, s.aw + 64) if fill is None else torch.full((s.M, s.aw + 64), fill, dtype=torch.bfloat16, device="cuda")
    d_feat = torch.full_like(d["d_feat"], float("nan") if fill is None else fill)
    a = dict(density=d["density"], rgb=d["rgb"], sem=d["sem"] if d["sem"].numel() else None, acts=acts, gacts=gacts, d_feat=d_feat)
    for k in null:
        a[k] = None
    L = _lib.lib()
    p = _lib.ptr
    tail = (p(a["density"]), p(a["rgb"]), p(a["sem"]), p(a["acts"]), p(g["density"]), p(g["rgb"]), p(g["sem"]), p(g["inten"]), p(a["gacts"]),
            p(a["d_feat"]), _lib.current_stream())
    if Mc is None:
        rc = L.nlr_mlp_train_backward(plan.handle, M, s.S if S is None else S, *tail)
    else:
        rc = L.nlr_mlp_train_backward_split(plan.handle, M, Mc, s.S if S is None else S, *tail)
    torch.cuda.synchronize()
    return rc, gacts, d_feat


def _wgrad(s, Mc, acts, gacts, M=None, S=None, null=(), fill=float("nan")):
    d, plan = s.d, s.lvl._plan
    M = s.M if M is None else M
    ws = s.lvl._wgrad_workspace(acts.device)
    a = dict(features=d["feats"], enc=d["enc"], acts=acts, gacts=gacts, d_params=torch.full((plan.n_params,), fill, device="cuda"))
    for k in null:
        a[k] = None
    L = _lib.lib()
    p = _lib.ptr
    tail = (p(a["features"]), p(a["enc"]), p(a["acts"]), p(a["gacts"]), p(a["d_params"]), p(ws), ws.numel(), _lib.current_stream())
    if Mc is None:
        rc = L.nlr_mlp_train_wgrad(plan.handle, M, s.S if S is None else S, *tail)
    else:
        rc = L.nlr_mlp_train_wgrad_split(plan.handle, M, Mc, s.S if S is None else S, *tail)
    torch.cuda.synchronize()
    return rc, a["d_params"]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _route():
    L = _lib.lib()
    return L.nlr_debug_get(_lib.DBG_TRAIN_ROUTE), L.nlr_debug_get(_lib.DBG_TRAIN_TRUNK_ROW0), L.nlr_debug_get(_lib.DBG_TRAIN_TRUNK_ROWS)


def _want_route(M, Mc, bwd):
    return ((_lib.TRAIN_FULL if Mc > 0 else 0) | (_lib.TRAIN_TRUNK if Mc < M else 0) | (_lib.TRAIN_BWD if bwd else 0), Mc, M - Mc)


@pytest.mark.gpu
@pytest.mark.parametrize("wl,S,n", CASES, ids=IDS)
def test_forward_split_against_unsplit(wl, S, n):
    """density / semantic / intensity and the trunk and head columns of acts: the unsplit bits on every row; rgb and the view
    columns: the unsplit bits on rows < M_color; rgb == 0 and view columns untouched on the others."""
    s = _scene(wl, S)
    Mc, d = n * S, s.d
    rc, o = _forward(s, Mc)
    assert rc == 0, _lib.lib().nlr_last_error().decode()
    assert _route() == _want_route(s.M, Mc, False)
    assert torch.equal(_bits(o["density"]), _bits(d["density"]))
    if s.K:
        assert torch.equal(_bits(o["sem"]), _bits(d["sem"]))
    if s.cfg.use_intensity:
        assert torch.equal(_bits(o["inten"]), _bits(d["inten"]))
    assert torch.equal(_bits(o["acts"][:, :s.c_x]), _bits(d["acts"][:, :s.c_x]))
    assert torch.equal(_bits(o["rgb"][:, :Mc]), _bits(d["rgb"][:, :Mc]))
    assert torch.equal(_bits(o["acts"][:Mc, s.c_x:]), _bits(d["acts"][:Mc, s.c_x:]))
    assert bool((_bits(o["rgb"][:, Mc:]) == 0).all())          # +0.0, bit for bit
    assert _is_nan16(o["acts"][Mc:, s.c_x:])                    # not written


def _poisoned(s, Mc):
    """The unsplit activations with the view columns of the colourless rows replaced by the NaN pattern."""
    acts = s.d["acts"].clone()
    acts.view(torch.int16)[Mc:, s.c_x:] = NAN16
    return acts


def _chain_rule_f64(s, rows):
    """d_features and the trunk / head columns of gacts of `rows` WITHOUT the view MLP, by the chain rule in float64 on the saved
    activations, with the bf16 rounding of each gradient tile between layers that the kernel applies (tests/test_training.py, (2))."""
    cfg, d, lvl, K, HH = s.cfg, s.d, s.lvl, s.K, s.HH
    WB = cfg.bottleneck_width
    A = d["acts"][rows].double().cpu()
    R = A.shape[0]
    r16 = lambda t: t.float().to(torch.bfloat16).double()
    wt = lambda m: r16(m.weight.detach().cpu())
    gsel = lambda t: None if t is None else (t[..., rows] if t.dim() == 2 else t[rows]).double().cpu()
    want = {}
    dhbe = torch.zeros(R, WB, dtype=torch.float64)
    if HH:
        dlo = torch.zeros(R, 32, dtype=torch.float64)
        if K:
            pr, gs = d["sem"][:, rows].double().cpu().t(), gsel(s.g["sem"]).t()
            dlo[:, :K] = pr * (gs - (pr * gs).sum(-1, keepdim=True))
        if cfg.use_intensity:
            dlo[:, K] = gsel(s.g["inten"])
        want[s.aw] = r16(dlo)
        h1 = torch.cat(([wt(lvl.sem_layer[0])] if K else []) + ([wt(lvl.intensity_layer[0])] if cfg.use_intensity else []), 0)
        h2 = torch.zeros(32, HH, dtype=torch.float64)
        r0 = 0
        if K:
            h2[:K, :64] = wt(lvl.sem_layer[2])
            r0 = 64
        if cfg.use_intensity:
            h2[K, r0:r0 + 64] = wt(lvl.intensity_layer[2])[0]
        dq = (A[:, s.c_q:s.c_q + HH] > 0) * (r16(dlo) @ h2)
        want[s.c_q] = dq
        dhbe = dhbe + r16(dq) @ h1
    dhbe[:, 0] += gsel(s.g["density"]) * (1 - torch.exp(-d["density"][rows].double().cpu()))
    want[64] = dhbe
    dhid = (A[:, :64] > 0) * (r16(dhbe) @ wt(lvl.density_layer[2]))
    want[0] = dhid
    return want, r16(dhid) @ wt(lvl.density_layer[0])


@pytest.mark.gpu
@pytest.mark.parametrize("wl,S,n", CASES, ids=IDS)
def test_backward_split_against_unsplit_and_float64(wl, S, n):
    """Rows < M_color: d_features and every gacts column are the unsplit call's bits (same kernel, same data).  Colourless rows:
    d_features and the trunk / head columns against the float64 chain rule on the saved activations at 4e-3 of each tensor's norm
    (the gate of the backward kernel), everything finite, with the view columns of acts and all of gacts
    pre-filled with a NaN pattern: the view and rgb_layer columns of gacts still hold it afterwards."""
    s = _scene(wl, S)
    Mc, d = n * S, s.d
    g = dict(s.g, rgb=None) if n == 0 else s.g      # M_color == 0: g_rgb may be NULL
    rc, G, dF = _backward(s, Mc, _poisoned(s, Mc), g)
    assert rc == 0, _lib.lib().nlr_last_error().decode()
    assert _route() == _want_route(s.M, Mc, True)
    assert torch.equal(_bits(G[:Mc]), _bits(d["gacts"][:Mc]))
    assert torch.equal(_bits(dF[:Mc]), _bits(d["d_feat"][:Mc]))
    if Mc == s.M:
        return
    rows = slice(Mc, s.M)
    assert _is_nan16(G[rows, s.c_x:s.aw]) and _is_nan16(G[rows, s.aw + 32:])      # view layers, rgb_layer: not written
    written = torch.cat([G[rows, :s.c_x], G[rows, s.aw:s.aw + 32]], 1).float()
    assert bool(torch.isfinite(written).all()) and bool(torch.isfinite(dF[rows]).all())
    want, dfeat = _chain_rule_f64(s, rows)

    def close(name, got, ref):
        err = float(np.linalg.norm(got - ref)) / max(float(np.linalg.norm(ref)), 1e-30)
        print(f"{wl} S={S} colour rays {n}: {name} relative norm error {err:.3e}")
        assert err <= 4e-3, f"{wl} {name}: relative norm error {err:.3e} > 4e-3"

    for c0, w in want.items():
        close(f"gacts[{c0}:{c0 + w.shape[1]}]", G[rows, c0:c0 + w.shape[1]].double().cpu().numpy(), w.numpy())
    close("d_feat", dF[rows].double().cpu().numpy(), dfeat.numpy())
    # reported, not asserted: the same rows from the unsplit call with g_rgb zeroed on them (sums that differ by exact zeros)
    gz = s.g["rgb"].clone()
    gz[:, Mc:] = 0
    rc, Gz, dFz = _backward(s, None, d["acts"], dict(s.g, rgb=gz))
    assert rc == 0
    same = torch.equal(_bits(Gz[rows, :s.c_x]), _bits(G[rows, :s.c_x])) and torch.equal(_bits(dFz[rows]), _bits(dF[rows])) and \
        torch.equal(_bits(Gz[rows, s.aw:s.aw + 32]), _bits(G[rows, s.aw:s.aw + 32]))
    print(f"{wl} S={S} colour rays {n}: colourless rows bit-equal to the unsplit call with g_rgb = 0 there: {same}")


def _want_f64_split(s, acts, gacts, Mc):
    """tests/test_mlp_wgrad.py:_want_f64 with a row count per Linear: view layers and rgb_layer over rows < M_color."""
    cfg, d, S = s.cfg, s.d, s.S
    feat = d["feats"].to(torch.bfloat16).double().cpu()
    enc = d["enc"].to(torch.bfloat16).double().cpu().repeat_interleave(S, dim=0)
    want, bound, colour = [], [], []
    for g0, n_out, blocks in tw._linears(cfg, s.aw):
        is_colour = s.c_x <= g0 < s.aw or g0 == s.aw + 32
        R = Mc if is_colour else s.M
        src = {"acts": acts[:R].double().cpu(), "feat": feat[:R], "enc": enc[:R]}
        g = gacts[:R, g0:g0 + n_out].double().cpu()
        x = torch.cat([src[k][:, c:c + w] for k, c, w in blocks], 1)
        for w_, b_ in ((g.t() @ x, g.abs().t() @ x.abs()), (g.sum(0), g.abs().sum(0))):
            want.append(w_.reshape(-1).numpy())
            bound.append(R * 2.0 ** -23 * b_.reshape(-1).numpy())
            colour.append(np.full(w_.numel(), is_colour))
    want, bound, colour = np.concatenate(want), np.concatenate(bound), np.concatenate(colour)
    assert np.isfinite(want).all()
    return want, bound + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64), colour


@pytest.mark.gpu
@pytest.mark.parametrize("wl,S,n", CASES, ids=IDS)
def test_wgrad_split_against_float64_on_poisoned_tensors(wl, S, n):
    """Every element of d_params against float64 GEMMs over the saved tensors (view / rgb Linears: rows < M_color, the others: all
    rows) at rows 2^-23 sum|terms| + 1 ulp, with the unwritten columns of the colourless rows holding NaN; two calls, same bits;
    the bmm form on the same tensors finite and within 2^-9 in norm (its partial results are bf16: one rounding of 8 mantissa bits
    per element, split-K factor 1 at these sizes; DESIGN records 1.45e-3 .. 1.66e-3 for it)."""
    s = _scene(wl, S)
    Mc = n * S
    rc, G, _ = _backward(s, Mc, _poisoned(s, Mc), dict(s.g, rgb=None) if n == 0 else s.g)
    assert rc == 0
    acts = _poisoned(s, Mc)
    rc, got_t = _wgrad(s, Mc, acts, G)
    assert rc == 0, _lib.lib().nlr_last_error().decode()
    rc, again = _wgrad(s, Mc, acts, G)
    assert rc == 0 and torch.equal(_bits(got_t), _bits(again))
    got = got_t.double().cpu().numpy()
    assert np.isfinite(got).all()
    want, bound, colour = _want_f64_split(s, acts, G, Mc)
    assert got.shape == want.shape == (s.lvl._plan.n_params,)
    err = np.abs(got - want)
    worst = int(np.argmax(err / bound))
    nrm = float(np.linalg.norm(want))
    e_new = float(np.linalg.norm(got - want)) / nrm
    assert (err <= bound).all(), f"element {worst}: |got - want| = {err[worst]:.3e} > bound {bound[worst]:.3e} ({int((err > bound).sum())} elements)"
    if Mc == 0:
        assert (got[colour] == 0).all() and colour.any()
    if Mc == s.M:
        assert torch.equal(_bits(got_t), _bits(s.d["d_params"]))
    # the bmm form of the same reduction (fused_wgrad=False)
    s.lvl._S = S
    assert s.M < 4096   # split-K factor 1
    bmm = torch.cat([t.reshape(-1).float() for t in ntrain._wgrad_bmm(s.lvl, s.M, s.d["feats"], s.d["enc"], acts, G, Mc)]).double().cpu().numpy()
    assert bmm.shape == want.shape and np.isfinite(bmm).all()
    e_bmm = float(np.linalg.norm(bmm - want)) / nrm
    print(f"wgrad split {wl} S={S} colour rays {n}: err_kernel {e_new:.3e}  err_bmm {e_bmm:.3e}  worst element {err[worst]:.3e} of bound {bound[worst]:.3e}")
    assert e_bmm <= 2.0 ** -9, f"bmm form: relative norm error {e_bmm:.3e} > 2^-9"
    if Mc == 0:
        assert (bmm[colour] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("wl,S", SHAPES)
def test_all_colour_is_the_unsplit_call_and_no_colour_takes_null(wl, S):
    s = _scene(wl, S)
    d = s.d
    rc, o = _forward(s, s.M)
    rc0, u = _forward(s, None)
    assert rc == 0 and rc0 == 0
    for k in o:
        if o[k] is not None:
            assert torch.equal(_bits(o[k]), _bits(u[k])), k
    rc, G, dF = _backward(s, s.M, d["acts"], s.g)
    assert rc == 0 and torch.equal(_bits(G), _bits(d["gacts"])) and torch.equal(_bits(dF), _bits(d["d_feat"]))
    rc, P = _wgrad(s, s.M, d["acts"], d["gacts"])
    assert rc == 0 and torch.equal(_bits(P), _bits(d["d_params"]))
    # M_color == 0: no view MLP at all, g_rgb = NULL
    rc, o = _forward(s, 0)
    assert rc == 0 and _route() == (_lib.TRAIN_TRUNK, 0, s.M) and bool((_bits(o["rgb"]) == 0).all()) and _is_nan16(o["acts"][:, s.c_x:])
    rc, G, dF = _backward(s, 0, o["acts"], dict(s.g, rgb=None))
    assert rc == 0 and _route() == (_lib.TRAIN_TRUNK | _lib.TRAIN_BWD, 0, s.M) and bool(torch.isfinite(dF).all())
    rc, P = _wgrad(s, 0, o["acts"], G)
    assert rc == 0 and bool(torch.isfinite(P).all())
    off = 0
    view = {id(p) for p in [q for i in range(s.cfg.net_depth_viewdirs) for q in getattr(s.lvl, f"lin_second_stage_{i}").parameters()]
            + list(s.lvl.rgb_layer.parameters())}
    for p in s.lvl._mlp_params():
        part = P[off:off + p.numel()]
        assert (float(part.abs().max()) == 0.0) == (id(p) in view)
        off += p.numel()


@pytest.mark.gpu
def test_split_refusals_launch_nothing():
    s = _scene("C2", 32)
    d, M, S = s.d, s.M, s.S
    assert M % 5 != 0 and (3 * S) % 5 != 0
    SENT = 7.0

    def untouched(*ts):
        return all(bool((t.float() == SENT).all()) for t in ts if t is not None)

    fwd = [(dict(Mc=M + S), "M_color > M"), (dict(Mc=3 * S + 1), "M_color % S"), (dict(Mc=3 * S, S=5), "M % S"),
           (dict(Mc=3 * S, null=("features",)), "features"), (dict(Mc=3 * S, null=("enc",)), "enc"),
           (dict(Mc=3 * S, null=("density",)), "density"), (dict(Mc=3 * S, null=("rgb",)), "rgb"), (dict(Mc=3 * S, null=("acts",)), "acts"),
           (dict(Mc=3 * S, null=("sem",)), "semantic"), (dict(Mc=3 * S, null=("inten",)), "intensity")]
    for kw, word in fwd:
        rc, o = _forward(s, fill=SENT, **kw)
        msg = _lib.lib().nlr_last_error().decode()
        assert rc != 0 and word in msg and "forward_split" in msg, (kw, rc, msg)
        assert untouched(*o.values()), kw
    bwd = [(dict(Mc=M + S), "M_color > M"), (dict(Mc=3 * S + 1), "M_color % S"), (dict(Mc=3 * S, S=5), "M % S"),
           (dict(Mc=3 * S, null=("density",)), "density"), (dict(Mc=3 * S, null=("rgb",)), "rgb"), (dict(Mc=3 * S, null=("gacts",)), "gacts"),
           (dict(Mc=3 * S, null=("d_feat",)), "d_features")]
    for kw, word in bwd:
        Mc = kw.pop("Mc")
        rc, G, dF = _backward(s, Mc, d["acts"], s.g, fill=SENT, **kw)
        msg = _lib.lib().nlr_last_error().decode()
        assert rc != 0 and word in msg and "backward_split" in msg, (kw, rc, msg)
        assert untouched(G, dF), kw
    rc, G, dF = _backward(s, 3 * S, None, s.g, fill=SENT)
    assert rc != 0 and "acts" in _lib.lib().nlr_last_error().decode() and untouched(G, dF)
    wg = [(dict(Mc=M + S), "M_color > M"), (dict(Mc=3 * S + 1), "M_color % S"), (dict(Mc=3 * S, S=5), "M % S"),
          (dict(Mc=3 * S, null=("features",)), "features"), (dict(Mc=3 * S, null=("enc",)), "enc"),
          (dict(Mc=3 * S, null=("acts",)), "acts"), (dict(Mc=3 * S, null=("gacts",)), "gacts")]
    for kw, word in wg:
        Mc = kw.pop("Mc")
        rc, P = _wgrad(s, Mc, d["acts"], d["gacts"], fill=SENT, **kw)
        msg = _lib.lib().nlr_last_error().decode()
        assert rc != 0 and word in msg and "wgrad_split" in msg, (kw, rc, msg)
        assert untouched(P), kw
    need = int(_lib.lib().nlr_mlp_train_wgrad_workspace_bytes(s.lvl._plan.handle, M))
    assert need == s.lvl._wgrad_workspace(d["acts"].device).numel()   # unchanged by the split


# ---- on the GPU: end to end ------------------------------------------------------------------------------------------------------
def _model_and_batch(wl, n_rays=256):
    from nerflidar_hip import config as nconfig, scene as nscene, weights as nweights
    mc = nconfig.workload(wl, 12)
    sd = nweights.synth_state_dict(mc, seed=0, trained_like=True)
    rays = nscene.random_lidar_rays(n_rays, 0, 1, torch.device("cuda"))
    return mc, sd, rays


def _one_step(mc, sd, batch, fused, wgrad, color_rays):
    tm = ntrain.TrainableModel(mc, fused_mlp=fused, fused_wgrad=wgrad).cuda().load_reference(sd)
    rend, hist = tm(batch, randomized=False, color_rays=color_rays)
    route = _route()
    terms = nlosses.total_loss(rend, hist, batch)
    loss = sum(terms.values())
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().double().cpu().numpy() for k, p in tm.named_parameters() if p.grad is not None}
    return {k: float(v) for k, v in terms.items()}, grads, rend, route


@pytest.mark.gpu
@pytest.mark.parametrize("wl", ["C2", "REF"])
@pytest.mark.parametrize("fused,wgrad", [(False, False), (True, False), (True, True)], ids=["torch", "fused", "fused-wgrad"])
def test_whole_model_step_with_color_rays_matches_the_masked_step(wl, fused, wgrad):
    """One forward + loss + backward of a TrainableModel with color_rays = n and mask_rgb / sem_mask zero on the suffix against the
    same model and batch with color_rays = None.  Torch Linear path: every loss term and every parameter gradient to 6e-5
    (relative; gradients in norm).  Fused path: the gates tests/test_training.py applies to fused against torch, unchanged: terms
    to 3e-2, gradients to 4e-2 of their norm.  With fused_mlp the trunk-and-heads instance must have run on the rows [n S, N S)."""
    from nerflidar_hip import scene as nscene
    mc, sd, rays = _model_and_batch(wl)
    N = rays["origins"].shape[0]
    S = mc.level_samples()[-1]
    for n in (0, 100, N):
        batch = nscene.supervise(rays, colourless=N - n)
        assert int(batch["mask_rgb"].sum()) == n and int(batch["sem_mask"].sum()) == n
        t0, g0, r0, route0 = _one_step(mc, sd, batch, fused, wgrad, None)
        t1, g1, r1, route1 = _one_step(mc, sd, batch, fused, wgrad, n)
        if fused:
            assert route0 == (_lib.TRAIN_FULL, N * S, 0)
            assert route1 == _want_route(N * S, n * S, False)   # the forward of the last level was the last forward call
            assert _lib.lib().nlr_debug_get(_lib.DBG_TRAIN_ROUTE) == _want_route(N * S, n * S, True)[0]
        rt, gt = (3e-2, 4e-2) if fused else (6e-5, 6e-5)
        assert set(t0) == set(t1) and set(g0) == set(g1)
        for k in t0:
            print(f"{wl} {'fused' if fused else 'torch'} n={n}: term {k} {t0[k]:.6e} / {t1[k]:.6e}")
            np.testing.assert_allclose(t1[k], t0[k], rtol=rt, atol=1e-12, err_msg=k)
        worst = 0.0
        for k in g0:
            nrm = float(np.linalg.norm(g0[k]))
            err = float(np.linalg.norm(g1[k] - g0[k])) / max(nrm, 1e-30)
            worst = max(worst, err if nrm > 0 else 0.0)
            if nrm == 0:       # no colour ray at all: the view MLP has an exactly zero gradient both ways
                assert float(np.abs(g1[k]).max()) == 0.0, k
            else:
                assert err <= gt, f"{wl} n={n} grad {k}: relative norm error {err:.3e} > {gt}"
        print(f"{wl} {'fused' if fused else 'torch'} n={n}: worst gradient relative norm error {worst:.3e}")
        assert bool(torch.isfinite(r1[-1]["rgb"]).all())


@pytest.mark.gpu
def test_level_rgb_is_zero_on_colourless_rays_both_paths():
    cfg, sd, batch, tdist, cot, N = tw._scene("REF", 32)
    for fused in (False, True):
        lvl = ntrain.TrainableNerfLevel(cfg, fused_mlp=fused).load_reference(sd).cuda()
        with torch.no_grad():
            full, part = lvl(batch, tdist), lvl(batch, tdist, color_rays=5)
        assert part["rgb"].shape == full["rgb"].shape
        assert float(part["rgb"][5:].abs().max()) == 0.0
        for k in full:
            a, b = (part[k], full[k]) if k != "rgb" else (part[k][:5], full[k][:5])
            if fused:
                assert torch.equal(a, b), k
            else:
                np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-5, atol=1e-6, err_msg=k)
        r, _ = lvl.render(batch, tdist, color_rays=5)
        assert bool(torch.isfinite(r["rgb"]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("wgrad", [False, True])
def test_training_step_with_color_rays_reads_nothing_back(wgrad):
    """tests/test_training.py::test_training_step_reads_nothing_back_until_its_terms_are_asked_for with color_rays in the step."""
    from nerflidar_hip import config as nconfig, scene as nscene, weights as nweights
    mc = nconfig.workload("REF", 12)
    mc.config.use_intensity = True
    mc.__post_init__()
    tm = ntrain.TrainableModel(mc, fused_mlp=True, fused_wgrad=wgrad).cuda().load_reference(nweights.synth_state_dict(mc, seed=0, trained_like=True))
    opt = torch.optim.Adam(tm.parameters(), lr=1e-3, eps=1e-15)
    n = 2048
    colourless = nlosses.colourless_count(n, 0.2)
    batch = nscene.supervise(nscene.random_lidar_rays(n, 0, 1, torch.device("cuda")), colourless=colourless)
    first = ntrain.training_step(tm, opt, batch, color_rays=n - colourless, check_color_rays=True)   # warm-up; the check reads the mask
    assert set(first) >= {"data", "depth", "sem", "int", "loss"} and all(np.isfinite(v) for v in first.values())
    with pytest.raises(ValueError):
        # broken promise (ray n - colourless - 1 is colour-supervised), found by the explicit check only
        ntrain.training_step(tm, opt, batch, color_rays=n - colourless - 1, check_color_rays=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ntrain.training_step(tm, opt, batch, as_tensors=True, color_rays=n - colourless)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(isinstance(v, torch.Tensor) and v.is_cuda and v.dim() == 0 for v in out.values())
    assert np.isfinite(float(out["loss"]))
    assert _lib.lib().nlr_debug_get(_lib.DBG_TRAIN_TRUNK_ROWS) == colourless * mc.level_samples()[-1]
