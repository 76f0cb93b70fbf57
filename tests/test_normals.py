"""Density normals (header section 12, nerflidar_hip/normals.py; ZI/models.py:1070-1094, :525-529, render.py:255-261): a float64
restatement on the CPU, the conditions the GPU cases have to meet, the refusals, and on the GPU `nlr_density_normals` against that
restatement, through `Model` / `render_image` / `render_lidar`, and at the edges of its envelope."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from grid_ref import _grid_lookup, _level_table
from oracle import nlr_oracle as orc
from test_pose_refine import _candidate_rays, _encoder

N_RAYS = 37
# (S, n, L, C): one partial wave of samples, exactly one, more than one; one multisample; one and two features per level
CASES = [(1, 7, 4, 4), (3, 7, 4, 4), (33, 7, 4, 4), (64, 7, 4, 4), (70, 7, 4, 4), (33, 1, 4, 4), (33, 7, 4, 1), (33, 7, 3, 2)]
FINE = (33, 7, 10, 4)
# The operator's envelope is F = L * C a multiple of 4 (header section 12): (33, 7, 3, 2) has F = 6, so on the GPU that case is held to
# the refusal the envelope prescribes, and (33, 7, 4, 2) is run beside it for two features per level.
GPU_CASES = CASES + [(33, 7, 4, 2)]
ACCURACY_LINES = []   # what the GPU tests measured; scripts/normals_accuracy.py runs them and writes this list to profiles/


def _record(line):
    print(line)
    ACCURACY_LINES.append(line)


# ---- the float64 / float32 restatement (CPU, torch autograd) --------------------------------------------------------------------
def _layers(F, seed):
    """density_layer.0 and row 0 of density_layer.2, seeded: w0 uniform +-1.7/sqrt(F), b0 +-0.1, w2_row0 +-1/8."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1
    return (u(64, F) * 1.7 / np.sqrt(F)).float(), (u(64) * 0.1).float(), (u(64) / 8).float()


def _restate(rays, tdist, rand_deg, table, enc, n, re_w, layers, dtype, weights=None):
    """cast_rays -> contract_mean_std -> lookup -> erf weights -> mean -> density layers -> autograd.grad with respect to the means
    -> mean over the multisamples -> normalise, in `dtype`.  Returns a dict of detached tensors."""
    o, d, bx, by, radii = [t.to(dtype) for t in rays]
    means, stds = orc.cast_rays(tdist.to(dtype), o, d, radii, bx, by, n=n, m=3, std_scale=0.35, rand_deg=None if rand_deg is None else rand_deg.to(dtype))
    means = means.detach().requires_grad_(True)                          # models.py:1077
    z, zs = orc.contract_mean_std(means, stds)
    x01 = (z / 2 + 1) / 2
    f = _grid_lookup(x01.reshape(-1, 3), table.to(dtype), enc).reshape(x01.shape[:-1] + (enc.num_levels, -1))   # [N,S,n,L,C]
    if re_w:
        gs = enc.grid_sizes.to(dtype)
        f = f * torch.erf(1 / torch.clamp(torch.sqrt(8 * (zs / 2)[..., None] ** 2 * gs ** 2), min=1e-10))[..., None]
    f = f.mean(dim=2).flatten(-2, -1)                                     # [N,S,F]
    w0, b0, w2 = [t.to(dtype) for t in layers]
    h = f @ w0.T + b0
    raw = torch.relu(h) @ w2                                              # raw_density up to density_layer.2's bias (models.py:996-997)
    (g,) = torch.autograd.grad(raw.sum(), means)                          # models.py:1082-1088 (d_output = ones)
    G = g.mean(-2)                                                        # models.py:1089
    nrm = -G / G.norm(dim=-1, keepdim=True).clamp_min(1e-5)               # models.py:1094, ref_utils.py:23-25
    out = dict(raw_grad=G, normals=nrm, features=f.detach(), h=h.detach(), x01=x01.detach(), means=means.detach())
    if weights is not None:
        out["ray_normals"] = (weights.to(dtype)[..., None] * nrm).sum(-2)
    return out


def _near(ref, enc):
    """[N, S] bool in float64: any coordinate of any multisample within 1e-4 cell of a cell face on any level, any hidden pre-activation
    with |h| < 1e-5, or any multisample with | |m|^2 - 1 | < 1e-5: where a float32 evaluation may take the other branch."""
    x01, h, means = ref["x01"], ref["h"], ref["means"]
    bad = torch.zeros(x01.shape[:2], dtype=torch.bool)
    for scale, *_ in _level_table(enc):
        pos = x01 * scale + (0.0 if enc.align_corners else 0.5)
        bad |= ((pos - torch.round(pos)).abs() < 1e-4).flatten(2).any(-1)
    bad |= (h.abs() < 1e-5).any(-1)
    bad |= (((means ** 2).sum(-1) - 1).abs() < 1e-5).any(-1)
    return bad


@functools.lru_cache(maxsize=None)
def _case(S, n, L, C, half, re_w, rand):
    """Rays, layers, weights and the float64 / float32 CPU restatements of one case, computed once and left unchanged."""
    enc = _encoder(L, C)
    table = enc.embeddings.detach()
    table = table.half().float() if half else table
    rays, tdist, rd = _candidate_rays(N_RAYS, S, n, 4000 + S * 10 + n, rand)
    layers = _layers(L * C, 17 * L + C)
    ref = _restate(rays, tdist, rd, table, enc, n, re_w, layers, torch.float64)
    near = _near(ref, enc)
    weights = torch.softmax(torch.randn(N_RAYS, S, generator=torch.Generator().manual_seed(S + n)) * 2, dim=-1)
    weights = torch.where(near, torch.zeros_like(weights), weights).contiguous()      # the near samples' weights are 0 on both sides
    ref["ray_normals"] = (weights.double()[..., None] * ref["normals"]).sum(-2)
    f32 = _restate(rays, tdist, rd, table, enc, n, re_w, layers, torch.float32, weights=weights)
    m2 = (ref["means"] ** 2).sum(-1)
    return dict(enc=enc, table=table, rays=rays, tdist=tdist, rd=rd, layers=layers, weights=weights, near=near, want=ref,
                f32={k: v.double() for k, v in f32.items()}, inside=bool((m2 <= 1).any()), outside=bool((m2 > 1).any()), half=half)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_restatement_agrees_with_a_finite_difference_of_the_density():
    """The checker itself: the float64 gradient against central differences of the float64 raw density along each axis, on samples
    that are not near a branch (where the density is smooth)."""
    k = _case(3, 7, 4, 4, False, True, True)
    enc, n = k["enc"], 7

    def density(shift):
        o, d, bx, by, radii = [t.double() for t in k["rays"]]
        means, stds = orc.cast_rays(k["tdist"].double(), o, d, radii, bx, by, n=n, m=3, std_scale=0.35, rand_deg=k["rd"].double())
        z, zs = orc.contract_mean_std(means + shift, stds)
        x01 = (z / 2 + 1) / 2
        f = _grid_lookup(x01.reshape(-1, 3), k["table"].double(), enc).reshape(x01.shape[:-1] + (enc.num_levels, -1))
        f = f * torch.erf(1 / torch.clamp(torch.sqrt(8 * (zs / 2)[..., None] ** 2 * enc.grid_sizes.double() ** 2), min=1e-10))[..., None]
        w0, b0, w2 = [t.double() for t in k["layers"]]
        return torch.relu(f.mean(dim=2).flatten(-2, -1) @ w0.T + b0) @ w2

    eps = 1e-6
    keep = ~k["near"]
    for c in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[c] = eps
        fd = (density(e) - density(-e)) / (2 * eps)          # all multisamples move together: sum_j d/dm_j = n * mean_j
        got = k["want"]["raw_grad"][..., c] * n
        assert float((fd - got)[keep].abs().max()) <= 1e-5 * float(got[keep].abs().max()), c


def test_the_cases_hold_what_they_claim():
    """A condition, not a measurement: in every GPU case at most 10 % of the samples are `near`, no kept sample has a zero gradient,
    and both branches of the contraction occur."""
    worst = 0.0
    for S, n, L, C in GPU_CASES + [FINE]:
        for rand in (False, True):
            for half in (False, True):
                k = _case(S, n, L, C, half, True, rand)
                frac = float(k["near"].float().mean())
                worst = max(worst, frac)
                assert frac <= 0.10, (S, n, L, C, rand, half, frac)
                assert float(k["want"]["raw_grad"].norm(dim=-1)[~k["near"]].min()) > 0
                if S * n > 1:
                    assert k["inside"] and k["outside"], (S, n, L, C)
    print(f"largest share of near samples over the cases: {100 * worst:.2f} %")


def test_workspace_formula_and_chunking():
    from nerflidar_hip import normals as nn_
    assert nn_.workspace_bytes(37, 33, 16) == 2 * 37 * 33 * 16 * 4 and nn_.workspace_bytes(0, 5, 8) == 0
    # C2's last level: 128 samples x 40 features = 40 960 bytes per ray; 16 384 rays run as chunks under the 256 MiB budget
    per = nn_.rays_per_chunk(128, 40)
    assert nn_.WORKSPACE_BUDGET_BYTES == 256 << 20 and per == (256 << 20) // 40960 and nn_.workspace_bytes(per, 128, 40) <= 256 << 20
    assert nn_.workspace_bytes(per + 1, 128, 40) > 256 << 20 and nn_.rays_per_chunk(128, 40, budget=1) == 1
    assert nn_.rays_per_chunk(1 << 20, 4) * (1 << 20) * 8 < 1 << 32          # a chunk's samples fit the kernels' 32-bit index
    from nerflidar_hip import _lib
    sig = _lib.signatures()["nlr_density_normals"]
    assert sig.launcher and [p.name for p in sig.params[-7:-1]] == ["weights", "raw_grad", "normals", "ray_normals", "workspace", "workspace_bytes"]
    assert _lib.signatures()["nlr_density_normals_workspace_bytes"].returns == "size_t"
    with pytest.raises(ValueError, match="want"):
        nn_.density_normals(None, {}, torch.zeros(1, 2), None, None, None, want=("normal",))
    with pytest.raises(ValueError, match="weights"):
        nn_.density_normals(None, {}, torch.zeros(1, 2), None, None, None)


def test_gin_binding_and_parser_flag():
    from nerflidar_hip import config as nconfig, render_lidar
    assert nconfig.ModelConfig().nerf_mlp.disable_density_normals is True
    mc = nconfig.parse_gin_bindings("NerfMLP.disable_density_normals = False\nConfig.analytic_gradient = True")
    assert mc.nerf_mlp.disable_density_normals is False and mc.prop_mlp.disable_density_normals is True and mc.config.analytic_gradient is True
    a = render_lidar.parse_args(["--normals", "--workload", "REFI"])
    assert a.normals is True and render_lidar.parse_args([]).normals is False
    assert render_lidar.parse_args(["--normals", "--lidar-only"]).lidar_only
    with pytest.raises(SystemExit):
        render_lidar.parse_args(["--normals", "--synthetic-tracks", "2"])


def _normals_config(name="REFI", lg=12):
    from nerflidar_hip import config as nconfig
    mc = nconfig.workload(name, lg)
    mc.nerf_mlp.disable_density_normals = False
    return mc


def test_refusals_name_the_setting():
    """Finite-difference normals, the dynamic-object branch and the training model refuse before anything touches the GPU."""
    from nerflidar_hip import models as nmodels, objects as nobj, training as ntrain
    mc = _normals_config()
    with pytest.raises(NotImplementedError, match="disable_density_normals"):
        ntrain.TrainableModel(mc)
    mc.config.instance_obj = True
    with pytest.raises(NotImplementedError, match="disable_density_normals"):
        nobj.DynamicModel(mc, {}, np.zeros((1, 2, 9), np.float32), ["vehicle.car"])
    with pytest.raises(NotImplementedError, match="disable_density_normals"):
        ntrain.TrainableModel(mc, tracks=np.zeros((1, 2, 9), np.float32), class_names=["vehicle.car"])

    class Stub:                                               # CapturedRender looks before it captures
        has_density_normals = True
    with pytest.raises(NotImplementedError, match="disable_density_normals"):
        nmodels.CapturedRender(Stub(), {})



# ---- the fixture from the reference (tests/golden/make_golden_normals.py) -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture():
    """The fixture, its batch rebuilt from the recipe, the encoder and layers of the same seeded state dict, and the float64 / float32
    CPU restatements on the fixture's own tdist and weights."""
    from conftest import golden
    from nerflidar_hip import camera as ncamera, config as nconfig, lidar as nlidar, weights as nweights
    from nerflidar_hip.gridencoder import GridEncoder
    g = golden("normals_fwd")
    mc = nconfig.workload("REF", int(g["log2_hashmap"]))
    mc.config.use_intensity = True
    mc.nerf_mlp.disable_density_normals = False
    mc.nerf_mlp.grid_disired_resolution = int(g["grid_disired_resolution"])
    mc.__post_init__()
    sd = nweights.synth_state_dict(mc, seed=int(g["seed"]), trained_like=True)
    cam = ncamera.synthetic_camera_batch(width=int(g["cam_w"]), height=int(g["cam_h"]), focal=6.0, seed=int(g["seed"]))
    lid = nlidar.synthetic_sweep(width=int(g["width"]), seed=int(g["seed"]), beams=list(g["beams"]))
    keys = ("origins", "directions", "viewdirs", "radii", "near", "far", "base_x", "base_y")
    batch = {k: torch.from_numpy(np.concatenate([cam[k].reshape(cam[k].shape[0], -1), lid[k].reshape(lid[k].shape[0], -1)], 0)) for k in keys}
    enc = GridEncoder.from_mlp_config(mc.nerf_mlp)
    with torch.no_grad():
        enc.embeddings.copy_(torch.from_numpy(np.asarray(sd["nerf_mlp.encoder.embeddings"], np.float32)))
    f = lambda name: torch.from_numpy(np.asarray(sd["nerf_mlp.density_layer." + name], np.float32))
    layers = (f("0.weight"), f("0.bias"), f("2.weight")[0].contiguous())
    rays = [batch[k] for k in ("origins", "directions", "base_x", "base_y", "radii")]
    t = {k: torch.from_numpy(g[k]) for k in ("tdist", "weights", "raw_grad_density", "normals", "out_normals", "out_depth", "near")}
    refs = {dt: _restate(rays, t["tdist"], None, enc.embeddings.detach(), enc, 7, True, layers, dt, weights=t["weights"]) for dt in (torch.float64, torch.float32)}
    return dict(g=g, mc=mc, sd=sd, batch=batch, enc=enc, layers=layers, rays=rays, f64=refs[torch.float64],
                f32={k: v.double() for k, v in refs[torch.float32].items()}, **t)


def _fixture_errors(got, fx):
    """(raw_grad max abs, normals max |dn| where |G| >= 1e-3 max|G|, ray_normals max abs over rays whose samples are all kept) against
    the reference's values, outside the stored `near`."""
    keep = ~fx["near"]
    G = fx["raw_grad_density"].double().norm(dim=-1)
    big = keep & (G >= 1e-3 * float(G[keep].max()))
    whole = keep.all(-1)
    assert int(whole.sum()) > 0
    return (float((got["raw_grad"].double() - fx["raw_grad_density"].double())[keep].abs().max()),
            float((got["normals"].double() - fx["normals"].double()).norm(dim=-1)[big].max()),
            float((got["ray_normals"].double() - fx["out_normals"].double())[whole].abs().max()))


def test_fixture_conditions_and_the_float64_restatement_against_it():
    """The fixture is data of the stated size, `near` covers at most 10 % of its samples and is the mask the tests' own definition
    gives, both branches of the contraction occur; and the float64 restatement agrees with the reference (float32) outside `near`:
    raw_grad within 1e-4 of its maximum, the rendered normals likewise.  This checks the checker."""
    fx = _fixture()
    assert os.path.getsize(os.path.join(GOLDEN, "normals_fwd.npz")) <= 200 * 1000
    N, S = fx["weights"].shape
    assert fx["tdist"].shape == (N, S + 1) and fx["raw_grad_density"].shape == (N, S, 3) and fx["normals"].shape == (N, S, 3)
    assert fx["out_normals"].shape == (N, 3) and fx["out_depth"].shape == (N,) and fx["near"].dtype == torch.bool
    assert float(fx["near"].float().mean()) <= 0.10 and torch.equal(_near(fx["f64"], fx["enc"]), fx["near"])
    m2 = (fx["f64"]["means"] ** 2).sum(-1)
    assert bool((m2 <= 1).any()) and bool((m2 > 1).any())
    keep = ~fx["near"]
    gmax = float(fx["raw_grad_density"].abs().max())
    err = float((fx["f64"]["raw_grad"] - fx["raw_grad_density"].double())[keep].abs().max())
    assert err <= 1e-4 * gmax, (err, gmax)
    whole = keep.all(-1)
    rn = float((fx["f64"]["ray_normals"] - fx["out_normals"].double())[whole].abs().max())
    assert rn <= 1e-4 * float(fx["out_normals"].abs().max()), rn
    # the stored normals are the stored gradient normalised, and the rendered ones their weighted sum (render.py:255-261)
    G = fx["raw_grad_density"]
    assert float((fx["normals"] + G / G.norm(dim=-1, keepdim=True).clamp_min(1e-5)).abs().max()) <= 1e-6
    assert float(((fx["weights"][..., None] * fx["normals"]).sum(-2) - fx["out_normals"]).abs().max()) <= 1e-5


# ---- GPU: the operator alone ---------------------------------------------------------------------------------------------------
def _gpu_encoder(k):
    enc, dev = k["enc"], torch.device("cuda")
    e2 = type("Enc", (), {})()                                # the encoder's attributes with this case's table (f32 or f16 values)
    for a in ("num_levels", "output_dim", "base_resolution", "per_level_scale", "_offsets_host", "gridtype_id", "align_corners", "interp_id"):
        setattr(e2, a, getattr(enc, a))
    e2.embeddings = k["table"].to(dev).half() if k["half"] else k["table"].to(dev)
    return e2


def _gpu_batch(k):
    o, d, bx, by, radii = [t.cuda() for t in k["rays"]]
    return dict(origins=o, directions=d, base_x=bx, base_y=by, radii=radii, viewdirs=d, near=radii, far=radii)


def _gpu_normals(k, n, re_w, want=("raw_grad", "normals", "ray_normals"), features=False, **kw):
    from nerflidar_hip.normals import density_normals
    dev = torch.device("cuda")
    return density_normals(_gpu_encoder(k), _gpu_batch(k), k["tdist"].to(dev), *[t.to(dev) for t in k["layers"]], weights=k["weights"].to(dev),
                           sample_n=n, rand_deg=None if k["rd"] is None else k["rd"].to(dev), re_weights=re_w, want=want,
                           return_features=features, **kw)


def _errors(got, k, ref):
    """(max abs of raw_grad, max |dn| over kept samples with |G| >= 1e-3 max|G|, max abs of ray_normals) of `got` against float64."""
    keep, want = ~k["near"], k["want"]
    G = want["raw_grad"].norm(dim=-1)
    big = keep & (G >= 1e-3 * float(G[keep].max()))
    return (float((got["raw_grad"] - want["raw_grad"])[keep].abs().max()), float((got["normals"] - want["normals"]).norm(dim=-1)[big].max()),
            float((got["ray_normals"] - want["ray_normals"]).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("S,n,L,C", GPU_CASES)
def test_operator_matches_float64_autograd(S, n, L, C):
    """`nlr_density_normals` against the float64 restatement, N = 37, f32 and f16 tables, re_weights on and off, rand_deg on and off.
    The gate is the project's own (test_pose_refine.py): the same restatement in float32 on the CPU deviates from float64 by some
    amount, and the kernel may deviate by at most 4 x that over the samples that are not `near`: raw_grad (max abs), normals (max |dn|
    where |G| >= 1e-3 max|G|), ray_normals (max abs, the near samples' weights 0 on both sides).
    (33, 7, 3, 2) is F = 6 features, outside the envelope (F % 4 == 0): the operator must refuse it, with the message."""
    if (L * C) % 4:
        with pytest.raises(RuntimeError, match=r"\(-2\).*F = L \* C = 6"):
            _gpu_normals(_case(S, n, L, C, False, True, False), n, True)
        return
    for half in (False, True):
        for re_w in (True, False):
            for rand in (False, True):
                k = _case(S, n, L, C, half, re_w, rand)
                got = _gpu_normals(k, n, re_w, features=True)
                torch.cuda.synchronize()
                got = {key: v.cpu().double() for key, v in got.items()}
                ferr = float((got["features"] - k["want"]["features"]).abs().max())
                assert ferr <= 9.2e-5, ("features", ferr)              # the bound derived in test_pose_refine.py
                for key in ("raw_grad", "normals", "ray_normals"):
                    assert got[key].shape == k["want"][key].shape and bool(torch.isfinite(got[key]).all()), key
                errs, yard = _errors(got, k, k["want"]), _errors(k["f32"], k, k["want"])
                scale = float(k["want"]["raw_grad"][~k["near"]].abs().max())
                tag = f"operator S={S} n={n} L={L} C={C} {'f16' if half else 'f32'} re_w={int(re_w)} rand={int(rand)}"
                for name, e, y in zip(("raw_grad", "normals", "ray_normals"), errs, yard):
                    _record(f"{tag} {name}: err {e:.3e} f32-reference {y:.3e} (x{e / max(y, 1e-300):.2f})" +
                            (f" max|G| {scale:.3e} err/max {e / scale:.2e}" if name == "raw_grad" else "") +
                            f" left out {int(k['near'].sum())}/{k['near'].numel()}")
                for name, e, y in zip(("raw_grad", "normals", "ray_normals"), errs, yard):
                    assert e <= 4 * y, (name, half, re_w, rand, e, y)


@pytest.mark.gpu
def test_operator_fine_levels_percentiles():
    """L = 10: on the fine levels a float32 position is uncertain by more than the face margin, the float32 CPU path itself shows
    maxima of 1e-2 of max|G|, and a maximum means nothing.  The median and the 90th percentile of |dn| over ALL samples are held to
    4 x the same percentiles of the float32 CPU path."""
    S, n, L, C = FINE
    for half in (False, True):
        k = _case(S, n, L, C, half, True, True)
        got = _gpu_normals(k, n, True)
        torch.cuda.synchronize()
        dn = (got["normals"].cpu().double() - k["want"]["normals"]).norm(dim=-1).flatten()
        d32 = (k["f32"]["normals"] - k["want"]["normals"]).norm(dim=-1).flatten()
        assert bool(torch.isfinite(dn).all())
        for q in (0.5, 0.9):
            e, y = float(torch.quantile(dn, q)), float(torch.quantile(d32, q))
            _record(f"fine levels S={S} n={n} L={L} C={C} {'f16' if half else 'f32'} |dn| quantile {q}: {e:.3e} f32-reference {y:.3e} (x{e / y:.2f}); "
                    f"max {float(dn.max()):.3e} f32-reference max {float(d32.max()):.3e}")
            assert e <= 4 * y, (q, e, y)


@pytest.mark.gpu
def test_operator_on_the_reference_fixture():
    """The operator on the fixture's own tdist and weights against the reference's raw_grad_density, normals and rendered normals
    outside the stored `near` (rendered normals: the rays whose samples are all kept).  The gates are measured: 4 x what the float32
    CPU restatement shows against the same fixture (profiles/density_normals_accuracy.txt holds both columns)."""
    from nerflidar_hip.normals import density_normals
    fx = _fixture()
    dev = torch.device("cuda")
    enc = fx["enc"]
    e2 = type("Enc", (), {})()
    for a in ("num_levels", "output_dim", "base_resolution", "per_level_scale", "_offsets_host", "gridtype_id", "align_corners", "interp_id"):
        setattr(e2, a, getattr(enc, a))
    e2.embeddings = enc.embeddings.detach().to(dev)
    got = density_normals(e2, {k: v.to(dev) for k, v in fx["batch"].items()}, fx["tdist"].to(dev), *[t.to(dev) for t in fx["layers"]],
                          weights=fx["weights"].to(dev))
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in got.items()}
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    errs, yard = _fixture_errors(got, fx), _fixture_errors(fx["f32"], fx)
    for name, e, y in zip(("raw_grad", "normals", "ray_normals"), errs, yard):
        _record(f"fixture normals_fwd {name}: operator against the reference {e:.3e}, f32 CPU restatement against the reference {y:.3e} (x{e / max(y, 1e-300):.2f}); "
                f"max|G| {float(fx['raw_grad_density'].abs().max()):.3e}, left out {int(fx['near'].sum())}/{fx['near'].numel()}")
    for name, e, y in zip(("raw_grad", "normals", "ray_normals"), errs, yard):
        assert e <= 4 * y, (name, e, y)


@pytest.mark.gpu
def test_operator_outputs_are_independent_and_repeatable():
    """Each output requested alone has the bits it has when all are requested, the dict holds exactly what was asked for, two runs
    and two chunkings are bitwise equal, and a buffer passed for no output is not written."""
    k = _case(70, 7, 4, 4, False, True, True)
    a, b = _gpu_normals(k, 7, True), _gpu_normals(k, 7, True)
    assert set(a) == {"raw_grad", "normals", "ray_normals"}
    for key in a:
        assert torch.equal(a[key], b[key]), key
    for key in a:
        only = _gpu_normals(k, 7, True, want=(key,))
        assert set(only) == {key} and torch.equal(only[key], a[key]), key
    from nerflidar_hip import normals as nn_
    small = _gpu_normals(k, 7, True, workspace_budget=nn_.workspace_bytes(5, 70, 16))    # 8 chunks of 5, 5, ..., 2 rays
    for key in a:
        assert torch.equal(small[key], a[key]), key
    # the raw call with two outputs NULL: only the third is written, and the workspace past its stated size is left alone
    from nerflidar_hip import _lib
    dev = torch.device("cuda")
    rays, held = _lib.rays(_gpu_batch(k), N_RAYS)
    tab = k["table"].to(dev)                               # (held: the descriptor carries its address)
    gd = nn_.grid_desc(k["enc"], tab)
    need = nn_.workspace_bytes(N_RAYS, 70, 16)
    assert _lib.lib().nlr_density_normals_workspace_bytes(N_RAYS, 70, 16) == need
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=dev)
    out = torch.full((N_RAYS, 70, 3), 7.0, device=dev)
    w0, b0, w2 = [t.to(dev) for t in k["layers"]]
    _lib.call("nlr_density_normals", rays, k["tdist"].to(dev), N_RAYS, 70, 7, 3, 0.35, k["rd"].to(dev), gd, 1, 64, w0, b0, w2, None, None, out, None,
              ws, need)
    torch.cuda.synchronize()
    assert torch.equal(out, a["normals"]) and bool((ws[need:] == 0x5A).all())


def _raw_call(k, gd, hidden=64, ws_bytes=None, ws=True, n_rays=N_RAYS, S=3):
    from nerflidar_hip import _lib, normals as nn_
    dev = torch.device("cuda")
    rays, held = _lib.rays(_gpu_batch(k), N_RAYS)
    F = gd.num_levels * gd.level_dim
    need = nn_.workspace_bytes(N_RAYS, S, F)
    buf = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    w0, b0, w2 = torch.zeros(hidden, max(F, 1), device=dev), torch.zeros(hidden, device=dev), torch.zeros(hidden, device=dev)
    out = torch.zeros(N_RAYS, S, 3, device=dev)
    td = k["tdist"].to(dev)
    rc = _lib.lib().nlr_density_normals(C.byref(rays), _lib.ptr(td), n_rays, S, 7, 3, 0.35, None, C.byref(gd), 1, hidden, _lib.ptr(w0), _lib.ptr(b0),
                                        _lib.ptr(w2), None, _lib.ptr(out), None, None, _lib.ptr(buf) if ws else None,
                                        need if ws_bytes is None else ws_bytes, _lib.current_stream())
    torch.cuda.synchronize()
    return rc, _lib.lib().nlr_last_error()


@pytest.mark.gpu
def test_envelope_refusals_carry_a_message():
    """F = 68, F = 6, hidden != 64, level_dim = 3: NLR_ERR_UNSUPPORTED; a short or missing workspace: NLR_ERR_WORKSPACE; N = 0: NLR_OK."""
    from nerflidar_hip import normals as nn_
    k = _case(3, 7, 4, 4, False, True, False)
    dev = torch.device("cuda")
    tab = k["table"].to(dev)
    UNSUPPORTED, WORKSPACE = -2, -4

    def desc(L, Cdim):
        gd = nn_.grid_desc(k["enc"], tab)
        gd.num_levels, gd.level_dim = L, Cdim
        return gd

    rc, msg = _raw_call(k, desc(17, 4))
    assert rc == UNSUPPORTED and b"F = L * C = 68" in msg
    rc, msg = _raw_call(k, desc(3, 2))
    assert rc == UNSUPPORTED and b"F = L * C = 6" in msg
    rc, msg = _raw_call(k, desc(4, 3))
    assert rc == UNSUPPORTED and b"level_dim = 3" in msg
    rc, msg = _raw_call(k, desc(4, 4), hidden=32)
    assert rc == UNSUPPORTED and b"hidden width 32" in msg
    need = nn_.workspace_bytes(N_RAYS, 3, 16)
    rc, msg = _raw_call(k, desc(4, 4), ws_bytes=need - 1)
    assert rc == WORKSPACE and b"workspace too small" in msg
    rc, msg = _raw_call(k, desc(4, 4), ws=False)
    assert rc == WORKSPACE and b"workspace is NULL" in msg
    assert _raw_call(k, desc(4, 4), n_rays=0, ws=False)[0] == 0
    assert _raw_call(k, desc(4, 4))[0] == 0


# ---- GPU: through the model ----------------------------------------------------------------------------------------------------
def _mixed_batch(seed=5, width=12):
    """Camera rays, then a 12-column sweep: both sides of the unit sphere (tests/golden/make_golden_pose.pose_batch_np)."""
    from nerflidar_hip import camera as ncamera, lidar as nlidar
    cam = ncamera.synthetic_camera_batch(width=8, height=6, focal=6.0, seed=seed)
    lid = nlidar.synthetic_sweep(width=width, seed=seed, beams=nlidar.LIDAR_ANGLES[::4])
    keys = ("origins", "directions", "viewdirs", "radii", "near", "far", "base_x", "base_y")
    return {k: torch.from_numpy(np.concatenate([cam[k].reshape(cam[k].shape[0], -1), lid[k].reshape(lid[k].shape[0], -1)], 0)).cuda() for k in keys}


@functools.lru_cache(maxsize=None)
def _models(name):
    from nerflidar_hip import config as nconfig, weights as nweights
    from nerflidar_hip.models import Model
    plain, mc = nconfig.workload(name, 12), _normals_config(name, 12)
    sd = nweights.synth_state_dict(plain, seed=3, trained_like=True)
    return Model(plain, sd), Model(mc, sd), sd


def _same(a, b, skip=()):
    assert set(a) - set(skip) == set(b) - set(skip), (sorted(a), sorted(b))
    for key in a:
        if key in skip:
            continue
        if a[key] is None or b[key] is None:
            assert a[key] is None and b[key] is None, key
        else:
            assert a[key].dtype == b[key].dtype and torch.equal(a[key], b[key]), key


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["REFI", "C1"])
def test_model_forward_carries_the_operators_normals_and_changes_nothing_else(name):
    """`forward`'s ray_history[-1]['normals'] / renderings[-1]['normals'] are, bit for bit, `density_normals` on that call's own
    tdist, weights and rand_deg; every other key has the bits it has with normals disabled; for rand falsy, a seeded generator, and
    the LiDAR-only render."""
    from nerflidar_hip.normals import density_normals
    m0, m1, sd = _models(name)
    assert not m0.has_density_normals and m1.has_density_normals
    batch = _mixed_batch()
    n = batch["origins"].shape[0]
    samples = m1.mc.level_samples()
    for seeded in (False, True):
        gens = [torch.Generator(device="cuda").manual_seed(11) if seeded else False for _ in range(3)]
        r0, h0 = m0(gens[0], batch, 1.0, True)
        r1, h1 = m1(gens[1], batch, 1.0, True)
        rd = None
        if seeded:                                            # the draws of Model.forward, in its order
            [torch.rand(n, 1, device="cuda", generator=gens[2]) for _ in samples]
            rd = [torch.rand(n, S, 7, device="cuda", generator=gens[2]) for S in samples][-1]
        assert len(r0) == len(r1) and len(h0) == len(h1)
        for a, b in zip(r0[:-1] + h0[:-1], r1[:-1] + h1[:-1]):
            _same(a, b)
        _same(r0[-1], r1[-1], skip=("normals",))
        _same(h0[-1], h1[-1], skip=("normals", "raw_grad_density"))
        assert "normals" not in r0[-1] and "normals" not in h0[-1]
        ns = m1._normals
        want = density_normals(ns.encoder, batch, h1[-1]["tdist"], ns.w0, ns.b0, ns.w2, weights=h1[-1]["weights"], rand_deg=rd, std_scale=m1.mc.std_scale)
        assert r1[-1]["normals"].shape == (n, 3) and h1[-1]["normals"].shape == (n, samples[-1], 3)
        assert torch.equal(r1[-1]["normals"], want["ray_normals"]) and torch.equal(h1[-1]["normals"], want["normals"])
        assert torch.equal(h1[-1]["raw_grad_density"], want["raw_grad"])
        assert bool(torch.isfinite(want["normals"]).all()) and float(want["raw_grad"].abs().max()) > 0
        if seeded:
            assert not torch.equal(h1[-1]["normals"], keep_det)
        keep_det = h1[-1]["normals"]
    # the sd's own layers are what the model kept
    assert torch.equal(m1._normals.w0.cpu(), torch.from_numpy(np.asarray(sd["nerf_mlp.density_layer.0.weight"], np.float32)))
    assert torch.equal(m1._normals.w2.cpu(), torch.from_numpy(np.asarray(sd["nerf_mlp.density_layer.2.weight"], np.float32)[0]))
    # LiDAR-only, and compute_extras off: per-sample normals without the rendered one
    for kw in (dict(lidar_only=True), dict(lidar_only=True, compute_extras=False), dict(compute_extras=False)):
        ra, ha = m0.render_rays(batch, want_history=True, **kw)
        rb, hb = m1.render_rays(batch, want_history=True, **kw)
        _same(ra, rb, skip=("normals",))
        for a, b in zip(ha, hb):
            _same(a, b, skip=("normals", "raw_grad_density"))
        assert ("normals" in rb) == kw.get("compute_extras", True) and torch.equal(hb[-1]["normals"], keep_first(m1, batch))
    ra, ha = m1.render_rays(batch)                              # without the history nothing is added
    assert "normals" not in ra and all("normals" not in h for h in ha)
    from nerflidar_hip.models import CapturedRender
    with pytest.raises(NotImplementedError, match="disable_density_normals"):
        CapturedRender(m1, batch)


def keep_first(model, batch):
    return model(False, batch, 1.0, True)[1][-1]["normals"]


@pytest.mark.gpu
def test_render_image_and_render_lidar_return_the_normals(tmp_path):
    """`render_image` returns `normals` [H, W, 3], chunked or not, equal to the unsharded call; `render_lidar --normals` writes
    points_normals_%04d.npy with the values of the sweep's render beside the reference's three files."""
    from nerflidar_hip import config as nconfig, lidar as nlidar, render_lidar
    from nerflidar_hip.models import render_image
    m0, m1, _ = _models("REFI")
    from nerflidar_hip import camera as ncamera
    cam = ncamera.synthetic_camera_batch(width=8, height=6, focal=6.0, seed=2)
    img = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda().reshape(6, 8, -1) for k, v in cam.items()
           if k in ("origins", "directions", "viewdirs", "radii", "near", "far", "base_x", "base_y")}
    flat = {k: v.reshape(48, -1) for k, v in img.items()}
    whole = m1(False, flat, 1.0, True)[0][-1]["normals"]
    for chunk in (16384, 20):
        cfg = nconfig.Config(use_intensity=True, render_chunk_size=chunk)
        out = render_image(m1, None, img, False, cfg)
        assert out["normals"].shape == (6, 8, 3) and out["normals"].dtype == torch.float32
        assert torch.equal(out["normals"].reshape(48, 3), whole), chunk
        assert "normals" not in render_image(m0, None, img, False, cfg)
    sweep = render_image(m1, None, flat, False, cfg, image=False)
    assert sweep["normals"].shape == (48, 3) and torch.equal(sweep["normals"], whole)
    # the driver
    args = ["--workload", "REFI", "--log2-hashmap", "12", "--width", "12", "--sweeps", "1", "--render-dir", str(tmp_path), "--normals"]
    assert render_lidar.main(args) == 0
    out_dir = tmp_path / "lidar_replay"
    assert sorted(os.listdir(out_dir)) == ["points_0000.npy", "points_normals_0000.npy", "points_rgb_0000.npy", "points_semantic_0000.npy"]
    got = np.load(out_dir / "points_normals_0000.npy")
    pts = np.load(out_dir / "points_0000.npy")
    assert got.dtype == np.float32 and got.shape == (pts.shape[0], 3) and np.isfinite(got).all() and np.abs(got).max() > 0
    from nerflidar_hip import weights as nweights
    from nerflidar_hip.models import Model
    mc = _normals_config("REFI", 12)
    model = Model(mc, nweights.synth_state_dict(mc, seed=0, trained_like=True))
    b = nlidar.synthetic_sweep(width=12, seed=0, scale_factor=1.0 / 250.0, sweep_idx=0)
    res = render_lidar.render_sweep(model, b, 1.0 / 250.0)
    assert np.array_equal(got, res["normals"].cpu().numpy())
    assert (np.linalg.norm(got, axis=-1) <= 1 + 1e-5).all()      # a weighted sum of unit vectors with weights that sum to at most 1
    lo = render_lidar.render_sweep_device(model, {kk: torch.from_numpy(np.ascontiguousarray(v)).cuda() for kk, v in b.items()}, 1.0 / 250.0, lidar_only=True)
    assert torch.equal(lo["normals"], res["normals"]) and "rgb" not in lo
    render_lidar.main(args[:-1] + ["--render-dir", str(tmp_path / "plain")])
    assert "points_normals_0000.npy" not in os.listdir(tmp_path / "plain" / "lidar_replay")
