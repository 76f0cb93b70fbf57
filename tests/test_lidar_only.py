"""LiDAR-only rendering (`nlr_render_lidar`, `render_rays(lidar_only=True)`): a render for a caller that reads no colour.  The
direction encoding and the view MLP of the last level are not executed; every other output must be the SAME BITS as the full
render's, whichever route the library takes: the LiDAR-only compositing instance of the NerfMLP kernel (NLR_PREC_FAST, no per-sample
history: `_lib.ROUTE_LIDAR_FUSED`) or the kernels of `nlr_mlp_level(rgb = NULL)` + `nlr_composite_level(rgb = NULL)`
(`_lib.ROUTE_LIDAR`).  The route is read back from the library (NLR_DBG_LAST_ROUTE), never inferred from a timing."""
import ctypes as C

import numpy as np
import pytest
import torch

from nerflidar_hip import _lib, config as nconfig, lidar as nlidar, weights as nweights

DEV = "cuda:0"
SF = 1 / 250


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _route():
    return _lib.lib().nlr_debug_get(_lib.DBG_LAST_ROUTE)


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_lidar_entry_points_are_exported():
    L = _lib.lib()
    for name in ("nlr_render_lidar", "nlr_render_lidar_dynamic"):
        assert name in _lib.EXPORTS
        assert getattr(L, name) is not None
    assert L.nlr_render_lidar.argtypes == L.nlr_render_rays.argtypes
    assert L.nlr_render_lidar_dynamic.argtypes == L.nlr_render_rays_dynamic.argtypes


def test_struct_sizes_are_unchanged():
    """The mode travels as an entry point of its own: no struct grew a flag."""
    assert C.sizeof(_lib.NlrRays) == 64
    assert C.sizeof(_lib.NlrLevelOut) == 112
    assert C.sizeof(_lib.NlrOut) == 12 * 8 + 8 + 4 * 112
    assert C.sizeof(_lib.NlrRenderCfg) == 16 + 2 * 32 + 8 == 88


def test_render_lidar_parser_has_the_option_and_refuses_the_unet(capsys):
    from nerflidar_hip import render_lidar
    assert render_lidar.parse_args([]).lidar_only is False
    a = render_lidar.parse_args(["--lidar-only", "--sweeps", "2"])
    assert a.lidar_only is True and a.raydrop_unet is None
    assert render_lidar.parse_args(["--raydrop-unet", "unet.pth"]).raydrop_unet == "unet.pth"
    with pytest.raises(SystemExit) as e:
        render_lidar.parse_args(["--lidar-only", "--raydrop-unet", "unet.pth"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--lidar-only" in err and "--raydrop-unet" in err and "rgb" in err


@pytest.mark.parametrize("wl", ["C2", "REF", "C1"])
def test_lidar_flops_are_the_full_count_minus_view_mlp_and_rgb(wl):
    from nerflidar_hip.flops import flops_per_ray, lidar_flops_per_ray, lidar_macs_per_sample, macs_per_sample
    mc = nconfig.workload(wl)
    cfg = mc.nerf_mlp
    view = sum(o * i for name, (o, i), _ in nweights.mlp_param_shapes(cfg) if name.startswith("lin_second_stage_"))
    rgb = sum(o * i for name, (o, i), _ in nweights.mlp_param_shapes(cfg) if name == "rgb_layer")
    assert view > 0 and rgb == 3 * cfg.net_width_viewdirs
    assert lidar_macs_per_sample(cfg) == macs_per_sample(cfg) - view - rgb
    assert lidar_flops_per_ray(mc) == flops_per_ray(mc) - 2 * mc.level_samples()[-1] * (view + rgb)
    # trunk + heads by hand: density_layer (F -> 64 -> bottleneck) + every built 64-wide head
    heads = sum(o * i for name, (o, i), _ in nweights.mlp_param_shapes(cfg) if name.startswith(("sem_layer", "intensity_layer")))
    F = cfg.grid_num_levels * cfg.grid_level_dim
    assert lidar_macs_per_sample(cfg) == 64 * F + cfg.bottleneck_width * 64 + heads


# ---- GPU: same bits as the full render --------------------------------------------------------------------------------------------
def _model(wl, log2, precision, seed=0):
    from nerflidar_hip.models import Model
    mc = nconfig.workload(wl, log2)
    sd = nweights.synth_state_dict(mc, seed=seed, trained_like=True)
    return mc, Model(mc, sd, device=DEV, precision=precision)


def _same_bits(model, batch, want_history, compute_extras, packed_shape, expect_route):
    n = batch["origins"].shape[0]
    tf = torch.full(packed_shape, -7.0, device=DEV)
    tl = torch.full(packed_shape, -7.0, device=DEV)
    rf, hf = model.render_rays(batch, compute_extras=compute_extras, want_history=want_history, scale_factor=SF, packed=tf)
    torch.cuda.synchronize()
    assert _route() in (_lib.ROUTE_FULL, _lib.ROUTE_FULL_FUSED)
    rl, hl = model.render_rays(batch, compute_extras=compute_extras, want_history=want_history, scale_factor=SF, packed=tl,
                               lidar_only=True)
    torch.cuda.synchronize()
    assert _route() == expect_route, (_route(), expect_route)
    assert "rgb" not in rl and "rgb" in rf
    assert set(rl) == set(rf) - {"rgb"}
    for k in rl:
        if k != "packed":
            assert torch.equal(rl[k], rf[k]), k
    assert len(hl) == len(hf)
    for li, (a, b) in enumerate(zip(hl, hf)):
        last = li == len(hf) - 1
        assert set(a) == set(b) - ({"rgb"} if last else set()), (li, set(a) ^ set(b))
        for k in a:
            assert torch.equal(a[k], b[k]), (li, k)
    pf, pl = tf.reshape(n, 7), tl.reshape(n, 7)
    assert torch.equal(pl[:, [0, 1, 2, 6]], pf[:, [0, 1, 2, 6]])
    assert bool((pl[:, 3:6] == 0).all())
    assert float(pf[:, 3:6].abs().sum()) > 0          # the full render does write a colour there
    return rl, hl


# (workload, log2 hash-map size, seed of the synthetic weights).  The seeds are chosen on the CPU oracle so that the 192-ray sweep
# below shows several classes: C1 with seed 0 renders class 18 on every ray, with seed 2 seven classes.
CASES = [("C2", 14, 0), ("REF", 14, 0), ("C1", 14, 2), ("P_F20", 12, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("wl,log2,seed", CASES)
@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("want_history", [False, True])
@pytest.mark.parametrize("compute_extras", [True, False])
def test_lidar_only_is_the_full_render_without_rgb(wl, log2, seed, precision, want_history, compute_extras):
    mc, model = _model(wl, log2, precision, seed=seed)
    H, wp = 8, 24
    b = nlidar.synthetic_sweep(width=wp, seed=3, beams=nlidar.LIDAR_ANGLES[::4])   # 192 rays, beam-major [H, wp]
    batch = {k: cu(v) for k, v in b.items()}
    # the fused instance serves NLR_PREC_FAST with level_dim 4 and no per-sample history of the last level; everything else falls back
    fused = precision == _lib.PREC_FAST and not want_history and mc.nerf_mlp.grid_level_dim == 4
    route = _lib.ROUTE_LIDAR_FUSED if fused else _lib.ROUTE_LIDAR
    for shape in ((H * wp, 7), (wp, H, 7)):   # ray-order records and the azimuth-major tile
        rl, hl = _same_bits(model, batch, want_history, compute_extras, shape, route)
    # not vacuous: a field with real density and more than one class
    _, hh = model.render_rays(batch, want_history=True, lidar_only=True)
    assert float(hh[-1]["density"].max()) > 1
    assert int(rl["labels"].unique().numel()) >= 2


@pytest.mark.gpu
def test_both_routes_are_taken():
    """C2 at NLR_PREC_FAST without history runs the new kernel instance; with per-sample history it takes the fallback."""
    mc, model = _model("C2", 14, _lib.PREC_FAST)
    batch = {k: cu(v) for k, v in nlidar.synthetic_sweep(width=8, seed=0).items()}
    model.render_rays(batch, lidar_only=True)
    assert _route() == _lib.ROUTE_LIDAR_FUSED
    model.render_rays(batch, lidar_only=True, want_history=True)
    assert _route() == _lib.ROUTE_LIDAR
    model.render_rays(batch)
    assert _route() == _lib.ROUTE_FULL_FUSED
    # the profiling scopes agree: one per-ray pre-kernel, one MLP launch, and the view MLP's time is gone
    L = _lib.lib()
    ms, cnt = (C.c_float * _lib.NLR_K_COUNT)(), (C.c_uint32 * _lib.NLR_K_COUNT)()
    _lib.check(L.nlr_profile_begin(model._handle))
    model.render_rays(batch, lidar_only=True)
    _lib.check(L.nlr_profile_end(model._handle, _lib.current_stream(), ms, cnt))
    assert cnt[4] == 1 and cnt[3] == 1 and cnt[5] == mc.num_levels


@pytest.mark.gpu
@pytest.mark.parametrize("wl", ["C2", "REF"])
def test_lidar_only_ray_count_prefixes(wl):
    """Ray counts whose last 256-sample tile is partial or pulled back inside the buffer, and M < 64: every prefix of the sweep
    renders what the same rays render inside the full sweep."""
    mc, model = _model(wl, 14, _lib.PREC_FAST, seed=11)
    full = {k: cu(v) for k, v in nlidar.synthetic_sweep(width=40, seed=11).items()}   # 1280 rays
    rf, _ = model.render_rays(full, scale_factor=0.004, lidar_only=True)
    assert _route() == _lib.ROUTE_LIDAR_FUSED
    ff, _ = model.render_rays(full, scale_factor=0.004)
    keys = ("depth", "semantic", "labels", "points", "acc", "distance_median") + (("intensity",) if "intensity" in rf else ())
    for k in keys:
        assert torch.equal(rf[k], ff[k]), k
    for n in (1, 3, 127, 129, 1000, 1279):
        rn, _ = model.render_rays({k: v[:n].contiguous() for k, v in full.items()}, scale_factor=0.004, lidar_only=True)
        assert _route() == _lib.ROUTE_LIDAR_FUSED
        for k in keys:
            assert torch.equal(rn[k], rf[k][:n]), (wl, n, k)


# ---- GPU: the trained checkpoints against the reference's own run -----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["REFI", "C2"])
@pytest.mark.parametrize("precision", [0, 1, 2])
def test_trained_scene_lidar_only_max_gates(case, precision):
    """tests/test_trained_scene.py's gates (the project's, not new ones) on the LiDAR-only render of the trained checkpoints."""
    import test_trained_scene as tts
    from nerflidar_hip import checkpoints as nckpt
    g, mc, sd, batch = tts._setup(case)
    model = nckpt.model_from_checkpoint(tts._ckpt(case), base=mc, device=DEV, precision=precision)[0]
    b = {k: cu(v) for k, v in batch.items() if k != "viewdirs"}
    r, _ = model.render_rays(b, scale_factor=SF, lidar_only=True)
    assert _route() == (_lib.ROUTE_LIDAR_FUSED if precision == _lib.PREC_FAST else _lib.ROUTE_LIDAR)
    npy = lambda t: t.detach().cpu().numpy()
    labels = npy(r["labels"])
    d = np.abs(npy(r["depth"]) - g["out_depth"])
    i = np.abs(npy(r["intensity"]) - g["out_intensity"])
    s = np.abs(npy(r["semantic"]) - g["out_semantic"])
    msg = (f"{case} precision {precision}: depth L1 {d.mean():.2e} max {d.max():.2e}; intensity max {i.max():.2e}; "
           f"semantic max {s.max():.2e}; labels differ {(labels != g['out_semantic'].argmax(-1)).sum()}")
    print(msg)
    assert d.max() <= 1e-3, msg
    assert d.mean() <= 1e-4, msg
    assert i.max() <= 1e-3, msg
    assert s.max() <= 5e-3, msg
    np.testing.assert_array_equal(labels, g["out_semantic"].argmax(-1), err_msg=msg)
    assert np.abs(npy(r["acc"]) - g["out_acc"]).max() <= 1e-5
    assert "rgb" not in r


# ---- GPU: HIP graph ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lidar_only_sweep_replays_from_a_hip_graph():
    """The shape of test_static_sweep_replays_from_a_hip_graph: the LiDAR-only sweep captured once, inputs refilled in place, the replay
    bit-identical to an eager LiDAR-only call on the new inputs."""
    from nerflidar_hip.models import CapturedRender
    mc, model = _model("C2", 14, _lib.PREC_FAST)
    H, wp = 8, 24
    sweeps = [nlidar.synthetic_sweep(width=wp, seed=s_, beams=nlidar.LIDAR_ANGLES[::4]) for s_ in (0, 1)]
    batch = {k: cu(v) for k, v in sweeps[0].items() if k != "viewdirs"}
    tile = torch.zeros(wp, H, 7, device=DEV)
    cap = CapturedRender(model, batch, compute_extras=True, scale_factor=SF, packed=tile, lidar_only=True)
    assert "rgb" not in cap.out
    for sw in (sweeps[1], sweeps[0]):
        for k in batch:
            batch[k].copy_(cu(sw[k]))               # refill the captured input buffers in place
        tile.zero_()
        for v in cap.out.values():
            v.zero_()
        out = cap.replay()
        torch.cuda.synchronize()
        eager_tile = torch.zeros(wp, H, 7, device=DEV)
        want, _ = model.render_rays({k: cu(v) for k, v in sw.items()}, compute_extras=True, scale_factor=SF, packed=eager_tile,
                                    lidar_only=True)
        torch.cuda.synchronize()
        assert _route() == _lib.ROUTE_LIDAR_FUSED
        for k in ("depth", "intensity", "semantic", "labels", "acc", "points", "distance_median"):
            assert torch.equal(out[k], want[k]), k
        assert torch.equal(tile, eager_tile)
        assert float(tile[..., [0, 1, 2, 6]].abs().sum()) > 0 and bool((tile[..., 3:6] == 0).all())


# ---- GPU: dynamic objects ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("precision", [0, 2])
def test_dynamic_lidar_only_equals_the_full_dynamic_render(precision):
    import test_objects as tobj
    from conftest import golden
    from nerflidar_hip import objects as nobj
    g = golden("obj_REF_small")
    mc, b, cids, cfgs, sd = tobj._scene(g)
    mc.config.instance_obj = True
    model = nobj.DynamicModel(mc, sd, g["tracks"], tobj.NAMES, precision=precision, obj_log2_hashmap=int(g["log2_hashmap"]))
    batch = {k: cu(v) for k, v in b.items()}
    rf, hf = model.render_rays(batch, want_history=True, scale_factor=SF)
    rl, hl = model.render_rays({k: v for k, v in batch.items() if k != "viewdirs"}, want_history=True, scale_factor=SF, lidar_only=True)
    assert _route() == _lib.ROUTE_LIDAR          # the object merge sits between MLP and compositing: per-sample kernels
    assert "rgb" not in rl and "rgb" not in hl[-1]
    for k in ("depth", "semantic", "labels", "points", "acc"):
        assert torch.equal(rl[k], rf[k]), k
    for li, (a, c) in enumerate(zip(hl, hf)):
        assert torch.equal(a["obj_mask"], c["obj_mask"]), li
        for k in ("density", "weights", "depth", "tdist"):
            assert torch.equal(a[k], c[k]), (li, k)
    assert torch.equal(hl[-1]["semantic"], hf[-1]["semantic"])
    assert bool(hl[-1]["obj_mask"].any()) and 14 in set(rl["labels"].cpu().tolist())   # the object branch decides labels


# ---- GPU: refusals and viewdirs ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_render_lidar_refuses_an_rgb_output_and_needs_no_viewdirs():
    mc, model = _model("C2", 14, _lib.PREC_FAST)
    b = nlidar.synthetic_sweep(width=8, seed=0, beams=nlidar.LIDAR_ANGLES[::4])
    batch = {k: cu(v) for k, v in b.items()}
    n = batch["origins"].shape[0]
    L = _lib.lib()
    rays = _lib.NlrRays()
    keep = []
    for k in ("origins", "directions", "radii", "near", "far", "base_x", "base_y"):   # viewdirs stays NULL
        t = batch[k].reshape(n, -1).contiguous().float()
        keep.append(t)
        setattr(rays, k, t.data_ptr())
    cfg = _lib.NlrRenderCfg()
    cfg.train_frac, cfg.compute_extras, cfg.sample_n, cfg.sample_m = 1.0, 0, 7, 3
    ws = torch.empty(L.nlr_workspace_bytes(model._handle, n), dtype=torch.uint8, device=DEV)
    depth = torch.full((n,), -3.0, device=DEV)
    rgb = torch.full((n, 3), -3.0, device=DEV)
    hrgb = torch.full((3, n, mc.level_samples()[-1]), -3.0, device=DEV)

    def call(out):
        with torch.cuda.device(DEV):
            rc = L.nlr_render_lidar(model._handle, C.byref(rays), n, C.byref(cfg), C.byref(out), _lib.ptr(ws), ws.numel(),
                                    _lib.current_stream())
        torch.cuda.synchronize()
        return rc, L.nlr_last_error().decode()

    out = _lib.NlrOut()
    out.depth, out.rgb = depth.data_ptr(), rgb.data_ptr()
    rc, msg = call(out)
    assert rc == -1 and "out->rgb" in msg, (rc, msg)          # NLR_ERR_INVALID
    assert bool((depth == -3).all()) and bool((rgb == -3).all())   # nothing was written
    out = _lib.NlrOut()
    out.depth = depth.data_ptr()
    out.history[mc.num_levels - 1].rgb = hrgb.data_ptr()
    rc, msg = call(out)
    assert rc == -1 and "history[2].rgb" in msg, (rc, msg)
    assert bool((depth == -3).all()) and bool((hrgb == -3).all())
    out = _lib.NlrOut()
    out.depth = depth.data_ptr()
    rc, msg = call(out)
    assert rc == 0, msg
    want, _ = model.render_rays(batch, compute_extras=False)
    assert torch.equal(depth, want["depth"])
    # Python: a batch without viewdirs renders LiDAR-only, and still raises in the full mode
    nov = {k: v for k, v in batch.items() if k != "viewdirs"}
    r, _ = model.render_rays(nov, compute_extras=False, lidar_only=True)
    assert torch.equal(r["depth"], want["depth"])
    with pytest.raises(RuntimeError, match="viewdirs"):
        model.render_rays(nov, compute_extras=False)
