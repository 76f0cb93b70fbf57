"""Scope row f-1: dynamic-object branch (Config.instance_obj=True).  The fixture `obj_REF_small` is the reference's own
Model.forward with three tracks (tests/golden/make_golden.py:gen_objects); the oracle restatement is held to it on the CPU, the
GPU path (fused static stages + torch ObjMLPs, nerflidar_hip/objects.py) to the fixture and to the oracle."""
import numpy as np
import pytest
import torch

from conftest import golden
from nerflidar_hip import config as nconfig, lidar as nlidar, objects as nobj, weights as nweights
from oracle import nlr_oracle as orc

NAMES = ["vehicle.car", "vehicle.truck", "vehicle.car"]


def _scene(g):
    lg, seed, width = int(g["log2_hashmap"]), int(g["seed"]), int(g["width"])
    mc = nconfig.workload("REF", lg)
    b = nlidar.synthetic_sweep(width=width, seed=seed, beams=list(g["beams"]))
    b["timestamp"] = g["timestamp"]
    cids = [int(c) for c in g["class_ids"]]
    cfgs = {cid: nconfig.obj_mlp_config(cid, latent_size=128, log2_hashmap=lg) for cid in sorted(set(cids))}
    sd = nweights.synth_state_dict(mc, seed=seed, trained_like=True)
    sd.update(nweights.synth_object_state_dict(cfgs, len(cids), seed=seed))
    return mc, b, cids, cfgs, sd


def test_synthetic_scene_is_the_fixtures():
    g = golden("obj_REF_small")
    mc, b, cids, cfgs, sd = _scene(g)
    np.testing.assert_array_equal(nobj.synthetic_tracks(b, 3, 5, int(g["seed"])), g["tracks"])
    np.testing.assert_array_equal(nobj.synthetic_timestamps(b["origins"].shape[0], int(g["seed"])), g["timestamp"])
    assert cids == [nobj.query_class(c) for c in NAMES] == [13, 14, 13]
    assert [nobj.query_class(c) for c in ("human.pedestrian.adult", "vehicle.bus.rigid", "vehicle.trailer", "movable_object.barrier")] == [11, 15, 14, 255]


def test_oracle_pose_and_box_transform_match_reference():
    g = golden("obj_REF_small")
    pose = orc.obj_get_pose(torch.from_numpy(g["timestamp"]), torch.from_numpy(g["tracks"]))
    np.testing.assert_allclose(pose.numpy(), g["pose"], rtol=0, atol=1e-7)
    b = nlidar.synthetic_sweep(width=int(g["width"]), seed=int(g["seed"]), beams=list(g["beams"]))
    pts_o, dirs_o, imap = orc.obj_box_pts(torch.from_numpy(g["pts_w"]), torch.from_numpy(b["viewdirs"]), torch.from_numpy(g["pose"]))
    np.testing.assert_array_equal(imap.numpy(), g["imap"])
    np.testing.assert_allclose(pts_o.numpy(), g["pts_o"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(dirs_o.numpy(), g["dirs_o"], rtol=1e-6, atol=1e-6)
    # the same two functions as the product path writes them (torch, device-agnostic)
    pose2 = nobj.get_pose(torch.from_numpy(g["timestamp"]), torch.from_numpy(g["tracks"]))
    np.testing.assert_allclose(pose2.numpy(), g["pose"], rtol=0, atol=1e-7)
    p2, d2, m2 = nobj.box_pts(torch.from_numpy(g["pts_w"]), torch.from_numpy(b["viewdirs"]), pose2)
    np.testing.assert_array_equal(m2.numpy(), g["imap"])
    np.testing.assert_allclose(p2.numpy(), g["pts_o"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(d2.numpy(), g["dirs_o"], rtol=1e-6, atol=1e-6)


def test_oracle_forward_with_objects_matches_reference():
    g = golden("obj_REF_small")
    mc, b, cids, cfgs, sd = _scene(g)
    objs = orc.make_objects(sd, g["tracks"], cids, cfgs)
    with torch.no_grad():
        rend, hist = orc.model_forward(sd, mc, {k: torch.from_numpy(v) for k, v in b.items()}, objects=objs)
    for lvl in range(3):
        np.testing.assert_array_equal(hist[lvl]["obj_mask"].numpy(), g[f"hist{lvl}_obj_mask"])
        np.testing.assert_allclose(hist[lvl]["sdist"].numpy(), g[f"hist{lvl}_sdist"], atol=2e-6, rtol=0)
        np.testing.assert_allclose(hist[lvl]["density"].numpy(), g[f"hist{lvl}_density"], atol=1e-3, rtol=2e-4)
        np.testing.assert_allclose(rend[lvl]["depth"].numpy(), g[f"lvl{lvl}_depth"], atol=2e-5, rtol=0)
    assert g["hist2_obj_mask"].sum() > 100 and g["hist0_obj_mask"].sum() > 100
    np.testing.assert_allclose(hist[2]["rgb"].numpy(), g["hist2_rgb"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(hist[2]["semantic"].numpy(), g["hist2_semantic"], atol=2e-5, rtol=0)
    for k in ("rgb", "depth", "semantic", "acc"):
        np.testing.assert_allclose(rend[-1][k].numpy(), g["out_" + k], atol=2e-5, rtol=0, err_msg=k)
    np.testing.assert_array_equal(rend[-1]["semantic"].numpy().argmax(-1), g["out_semantic"].argmax(-1))
    # the objects matter: without them the rendering is different on the rays that cross a box
    with torch.no_grad():
        r0, _ = orc.model_forward(sd, mc, {k: torch.from_numpy(v) for k, v in b.items()})
    hit = g["hist2_obj_mask"].any(-1)
    assert np.abs(r0[-1]["depth"].numpy() - g["out_depth"])[hit].max() > 1e-3


def test_object_parameter_shapes_are_the_references():
    cfg = nconfig.obj_mlp_config(13, latent_size=128, log2_hashmap=21)
    assert cfg.grid_num_levels == 7 and cfg.dim_dir_enc == 15
    assert dict((n, s) for n, s, _ in nweights.mlp_param_shapes(cfg)) == {
        "density_layer.0": (64, 14 + 64), "density_layer.2": (64, 64), "lin_second_stage_0": (32, 64 + 15 + 64),
        "lin_second_stage_1": (32, 32 + 143), "rgb_layer": (3, 32)}


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("precision", [0, 1, 2])
def test_dynamic_model_matches_reference(precision):
    g = golden("obj_REF_small")
    mc, b, cids, cfgs, sd = _scene(g)
    mc.config.instance_obj = True
    model = nobj.DynamicModel(mc, sd, g["tracks"], NAMES, precision=precision, obj_log2_hashmap=int(g["log2_hashmap"]))
    batch = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    rend, hist = model(False, batch, train_frac=1.0, compute_extras=True)
    npy = lambda t: t.detach().cpu().numpy()
    for lvl in range(3):
        # a sample exactly on a box face can fall on either side after 1-ulp differences in tdist: allow a handful
        assert (npy(hist[lvl]["obj_mask"]) != g[f"hist{lvl}_obj_mask"]).sum() <= 2
        assert np.abs(npy(rend[lvl]["depth"]) - g[f"lvl{lvl}_depth"]).mean() <= 1e-3
    d = np.abs(npy(rend[-1]["depth"]) - g["out_depth"])
    assert d.mean() <= 1e-3 and np.percentile(d, 95) <= 1e-3          # north_star gate: depth L1 <= 1e-3
    np.testing.assert_array_equal(npy(rend[-1]["semantic"]).argmax(-1), g["out_semantic"].argmax(-1))
    assert np.abs(npy(rend[-1]["semantic"]) - g["out_semantic"]).max() <= 2e-3
    assert np.abs(npy(rend[-1]["rgb"]) - g["out_rgb"]).mean() <= (2e-4 if precision == 0 else 3e-3)
    assert 14 in set(g["out_semantic"].argmax(-1).tolist())  # a truck is visible: the object branch decides labels
    # curr_track (models.py:307-313): moving every box far away must give the static rendering
    far_tracks = g["tracks"].copy()
    far_tracks[:, :, :3] += 50.0
    r_far, h_far = model(False, batch, train_frac=1.0, compute_extras=True, curr_track=far_tracks)
    from nerflidar_hip.models import Model
    static = Model(nconfig.workload("REF", int(g["log2_hashmap"])), sd, precision=precision)
    r_st, _ = static(False, batch, train_frac=1.0, compute_extras=True)
    assert not bool(h_far[-1]["obj_mask"].any())
    assert torch.equal(r_far[-1]["depth"], r_st[-1]["depth"]) and torch.equal(r_far[-1]["semantic"], r_st[-1]["semantic"])


@pytest.mark.gpu
def test_dynamic_model_rejects_what_the_reference_cannot_run():
    g = golden("obj_REF_small")
    mc, b, cids, cfgs, sd = _scene(g)
    mc2 = nconfig.workload("C2", int(g["log2_hashmap"]))
    sd2 = nweights.synth_state_dict(mc2, seed=0)
    sd2.update({k: v for k, v in sd.items() if k.startswith(("obj_mlp", "latent"))})
    with pytest.raises(NotImplementedError, match="intensity"):
        nobj.DynamicModel(mc2, sd2, g["tracks"], NAMES, obj_log2_hashmap=int(g["log2_hashmap"]))
    model = nobj.DynamicModel(mc, sd, g["tracks"], NAMES, obj_log2_hashmap=int(g["log2_hashmap"]))
    batch = {k: torch.from_numpy(v).cuda() for k, v in b.items() if k != "timestamp"}
    with pytest.raises(RuntimeError, match="timestamp"):
        model.render_rays(batch)
    with pytest.raises(ValueError, match="class name"):
        nobj.DynamicModel(mc, sd, g["tracks"], NAMES[:2], obj_log2_hashmap=int(g["log2_hashmap"]))


@pytest.mark.gpu
def test_dynamic_model_from_checkpoint(tmp_path):
    from nerflidar_hip import checkpoints as ck
    g = golden("obj_REF_small")
    mc, b, cids, cfgs, sd = _scene(g)
    extra = dict(sd)
    extra["glo_vecs.weight"] = np.zeros((4, 4), np.float32)
    ck.save_checkpoint(tmp_path, extra, 77)
    base = nconfig.ModelConfig(num_prop_samples=(64, 64), num_nerf_samples=32)
    m2, step, left = ck.dynamic_model_from_checkpoint(tmp_path, g["tracks"], NAMES, base=base, precision=1)
    assert step == 77 and left == ["glo_vecs.weight"] and m2.mc.config.latent_size == 128
    mc.config.instance_obj = True
    m1 = nobj.DynamicModel(mc, sd, g["tracks"], NAMES, precision=1, obj_log2_hashmap=int(g["log2_hashmap"]))
    batch = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    r1, r2 = m1.render_rays(batch)[0], m2.render_rays(batch)[0]
    for k in ("depth", "rgb", "semantic"):
        assert torch.equal(r1[k], r2[k]), k


@pytest.mark.gpu
def test_overlapping_boxes_last_track_wins():
    """Two boxes on the same spot with different classes: the reference's track loop lets the later one overwrite the earlier
    (ZI/models.py:415,475); the product path evaluates only the winner - same result, checked against the oracle's loop."""
    g = golden("obj_REF_small")
    mc, b, cids, cfgs, sd = _scene(g)
    tracks = g["tracks"].copy()
    tracks[1] = tracks[0]          # the truck sits exactly on car 0
    tracks[1, :, -1] = 1
    tracks[2, :, :3] = tracks[0, :, :3] + 0.03   # car 2 overlaps both partly
    objs = orc.make_objects(sd, tracks, cids, cfgs)
    with torch.no_grad():
        rend_o, hist_o = orc.model_forward(sd, mc, {k: torch.from_numpy(v) for k, v in b.items()}, objects=objs)
    mc.config.instance_obj = True
    model = nobj.DynamicModel(mc, sd, tracks, NAMES, precision=0, obj_log2_hashmap=int(g["log2_hashmap"]))
    rend, hist = model(False, {k: torch.from_numpy(v).cuda() for k, v in b.items()}, train_frac=1.0, compute_extras=True)
    npy = lambda t: t.detach().cpu().numpy()
    assert int(hist_o[-1]["obj_mask"].sum()) > 50
    for lvl in range(3):
        assert (npy(hist[lvl]["obj_mask"]) != hist_o[lvl]["obj_mask"].numpy()).sum() <= 2
    same = npy(hist[-1]["obj_mask"]) == hist_o[-1]["obj_mask"].numpy()
    m = hist_o[-1]["obj_mask"].numpy() & same
    # inside the boxes the per-sample semantic is the winner's one-hot: identical class per sample
    np.testing.assert_array_equal(npy(hist[-1]["semantic"])[m].argmax(-1), hist_o[-1]["semantic"].numpy()[m].argmax(-1))
    assert set(hist_o[-1]["semantic"].numpy()[m].argmax(-1).tolist()) == {13, 14} or set(hist_o[-1]["semantic"].numpy()[m].argmax(-1).tolist()) == {13}
    d = np.abs(npy(rend[-1]["depth"]) - rend_o[-1]["depth"].numpy())
    assert d.mean() <= 1e-3
    np.testing.assert_array_equal(npy(rend[-1]["semantic"]).argmax(-1), rend_o[-1]["semantic"].numpy().argmax(-1))


@pytest.mark.gpu
def test_track_box_params_kernel_matches_get_pose():
    """`nlr_track_box_params` against the reference's get_pose (fixture `pose`) pushed through the world2object constants."""
    g = golden("obj_REF_small")
    mc, b, cids, cfgs, sd = _scene(g)
    mc.config.instance_obj = True
    model = nobj.DynamicModel(mc, sd, g["tracks"], NAMES, obj_log2_hashmap=int(g["log2_hashmap"]))
    box = model.box_params(torch.from_numpy(g["timestamp"]).cuda()).cpu()
    pose = torch.from_numpy(g["pose"])
    theta = pose[:, :, 3]
    want = torch.cat([torch.cos(theta)[..., None], torch.sin(theta)[..., None], nobj._rotate_yaw_z(-pose[:, :, :3], theta),
                      1 / (pose[:, :, 4:7] / 2 + 1e-9)], dim=-1)
    np.testing.assert_allclose(box.numpy(), want.numpy(), rtol=2e-6, atol=2e-6)
    # timestamps exactly on a record and outside the recorded span (weights clamp to [0, 1])
    ts = torch.tensor([0.0, 0.25, 1.0, -0.5, 1.5])
    box2 = model.box_params(ts.cuda()).cpu()
    pose2 = nobj.get_pose(ts[:, None], torch.from_numpy(g["tracks"]))
    th2 = pose2[:, :, 3]
    want2 = torch.cat([torch.cos(th2)[..., None], torch.sin(th2)[..., None], nobj._rotate_yaw_z(-pose2[:, :, :3], th2),
                       1 / (pose2[:, :, 4:7] / 2 + 1e-9)], dim=-1)
    np.testing.assert_allclose(box2.numpy(), want2.numpy(), rtol=2e-6, atol=2e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [0, 2])
def test_device_side_object_branch_matches_the_torch_stage_loop(precision):
    """The object networks as one kernel per class on device-compacted lists (`nlr_render_rays_dynamic`) against the same branch
    with torch ops (`render_rays_torch`): same owners, per-sample results inside the boxes to fp32 summation-order accuracy."""
    g = golden("obj_REF_small")
    mc, b, cids, cfgs, sd = _scene(g)
    mc.config.instance_obj = True
    model = nobj.DynamicModel(mc, sd, g["tracks"], NAMES, precision=precision, obj_log2_hashmap=int(g["log2_hashmap"]))
    batch = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    r1, h1 = model.render_rays(batch, want_history=True, scale_factor=1 / 250)
    r2, h2 = model.render_rays_torch(batch, want_history=True, scale_factor=1 / 250)
    for lvl in range(3):
        assert torch.equal(h1[lvl]["obj_mask"], h2[lvl]["obj_mask"]), lvl
        assert torch.equal(h1[lvl]["tdist"], h2[lvl]["tdist"]) or lvl > 0
        m = h1[lvl]["obj_mask"]
        assert int(m.sum()) > 100
        d1, d2 = h1[lvl]["density"][m], h2[lvl]["density"][m]
        # raw density carries the trained-like gain of 1500 (weights.synth_state_dict): 1e-7 of summation-order noise in the
        # trunk is 1.5e-4 of density
        assert bool(((d1 - d2).abs() <= 3e-4 + 5e-5 * d2.abs()).all()), (lvl, float((d1 - d2).abs().max()))
    m = h1[-1]["obj_mask"]
    assert float((h1[-1]["rgb"][m] - h2[-1]["rgb"][m]).abs().max()) <= 2e-5
    assert torch.equal(h1[-1]["semantic"][m], h2[-1]["semantic"][m])        # one-hot of the owner's class
    assert float((r1["depth"] - r2["depth"]).abs().max()) <= 2e-5
    assert torch.equal(r1["labels"], r2["labels"])
    assert float((r1["rgb"] - r2["rgb"]).abs().max()) <= 1e-4


@pytest.mark.gpu
def test_device_side_object_branch_has_no_host_synchronisation():
    """The whole dynamic sweep can be captured into a HIP graph and replayed: nothing in it reads back to the host."""
    g = golden("obj_REF_small")
    mc, b, cids, cfgs, sd = _scene(g)
    mc.config.instance_obj = True
    model = nobj.DynamicModel(mc, sd, g["tracks"], NAMES, obj_log2_hashmap=int(g["log2_hashmap"]))
    batch = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    want, _ = model.render_rays(batch)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        model.render_rays(batch)          # warm-up on the capture stream (workspace sized)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            got, _ = model.render_rays(batch)
    got["depth"].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got["depth"], want["depth"]) and torch.equal(got["semantic"], want["semantic"])


@pytest.mark.gpu
def test_object_abi_error_paths():
    """Error behaviour of the device-side object API (header section 7b): enumerated status + message, nothing launched."""
    import ctypes as C
    from nerflidar_hip import _lib
    g = golden("obj_REF_small")
    mc, b, cids, cfgs, sd = _scene(g)
    mc.config.instance_obj = True
    model = nobj.DynamicModel(mc, sd, g["tracks"], NAMES, obj_log2_hashmap=int(g["log2_hashmap"]))
    L = _lib.lib()
    n, S = 64, 16
    dev = "cuda"
    rays = _lib.NlrRays()
    keep = {k: torch.zeros(n, 3 if k in ("origins", "directions", "viewdirs", "base_x", "base_y") else 1, device=dev) for k in
            ("origins", "directions", "viewdirs", "radii", "near", "far", "base_x", "base_y")}
    for k, t in keep.items():
        setattr(rays, k, t.data_ptr())
    td = torch.linspace(0, 1, S + 1, device=dev).repeat(n, 1).contiguous()
    dens = torch.zeros(n, S, device=dev)
    ws = torch.empty(int(L.nlr_objects_workspace_bytes(model._objects, n, S)), dtype=torch.uint8, device=dev)
    box3 = torch.zeros(n, 3, 8, device=dev)
    box3[..., 0] = 1.0          # cos
    box3[..., 2:5] = 5.0        # box centres far from the (all-zero) rays
    box3[..., 5:8] = 10.0       # boxes of half-size 0.1
    box2 = torch.zeros(n, 2, 8, device=dev)
    call = lambda box, nobjs, wsb: L.nlr_objects_apply(model._objects, C.byref(rays), _lib.ptr(td), _lib.ptr(box), n, S, nobjs, _lib.ptr(dens), None,
                                                       None, 0, None, _lib.ptr(ws), wsb, None)
    assert call(box2, 2, ws.numel()) == -1 and b"3 tracks" in L.nlr_last_error()           # track count of the object set
    assert call(box3, 3, 16) == -4 and b"workspace" in L.nlr_last_error()                 # NLR_ERR_WORKSPACE
    assert call(box3, 3, ws.numel()) == 0                                                  # no sample inside any box: nothing is touched
    torch.cuda.synchronize()
    assert float(dens.abs().max()) == 0.0
    assert L.nlr_track_box_params(_lib.ptr(model.tracks), _lib.ptr(td), n, 3, 1, _lib.ptr(box3), None) == -1 and b"T = 1" in L.nlr_last_error()


# ---- the owner map and the compaction at the edges of their loops -------------------------------------------------------------
# (N, S, n_obj): the smallest shapes that reach the four-boxes-per-trip tail clamp of nlr_box_owner_kernel with 1, 3, 0, 1 and 1
# leftover boxes, sample counts that are no multiple of 64 or 256, and exactly one whole block (64 * 4).
OWNER_CASES = [(3, 2, 1), (37, 5, 3), (37, 5, 4), (64, 4, 5), (130, 7, 9)]
# The test asserts, over the box constants the kernel wrote, that no |coordinate| of any (sample, box) pair lies within 1e-6 of 1.  The
# seed was picked with torch's CPU expressions for those constants, where the closest pair of the five cases is 1.6e-4 away.
OWNER_SEED = 4


def _owner_scene(N, S, n_obj, seed=OWNER_SEED):
    """Seeded rays in a narrow cone, sorted random tdist in [0, 1], and tracks from `synthetic_tracks` on those rays: track 1
    sits on top of track 0 (the later one must win) and the last of three or more tracks is moved out of every ray's reach."""
    gen = torch.Generator().manual_seed(1000 * seed + 100 * n_obj + N)
    o = (torch.rand(N, 3, generator=gen) - 0.5) * 0.04
    d = torch.tensor([1.0, 0.2, 0.1]) + (torch.rand(N, 3, generator=gen) - 0.5) * 0.5
    td = torch.sort(torch.rand(N, S + 1, generator=gen), dim=-1)[0].contiguous()
    ts = torch.rand(N, 1, generator=gen)
    tracks = nobj.synthetic_tracks({"origins": o.numpy(), "directions": d.numpy()}, n_obj, 5, seed, size=(0.3, 0.2, 0.2), depth=(0.2, 0.8))
    if n_obj >= 2:
        tracks[1, :, :8] = tracks[0, :, :8]
    if n_obj >= 3:
        tracks[-1, :, :3] += 50.0
    return o, d, td, ts, tracks


def _owner_reference(o, d, td, box):
    """float32 on the CPU, operation by operation in the order of the device functions (csrc/nlr_objects.hip): interval midpoint,
    quirk rotation, scale-and-shift, strict |x| < 1, the last containing track wins.  -> (winner [N,S], box coordinates
    [N,S,n_obj,3])."""
    tm = 0.5 * (td[:, :-1] + td[:, 1:])
    p = tm[..., None] * d[:, None, :] + o[:, None, :]                       # [N, S, 3]
    b = box[:, None]                                                        # [N, 1, n_obj, 8]
    px, py, pz = (p[..., None, c] for c in range(3))
    rx = b[..., 0] * px - b[..., 1] * py
    ry = b[..., 1] * rx + b[..., 0] * py                                    # (sic) the rotated x
    x = torch.stack([b[..., 5] * (rx + b[..., 2]), b[..., 6] * (ry + b[..., 3]), b[..., 7] * (pz + b[..., 4])], dim=-1)
    inside = (x.abs() < 1.0).all(-1)                                        # [N, S, n_obj]
    idx = torch.arange(box.shape[1], dtype=torch.int32).expand_as(inside)
    winner = torch.where(inside, idx, torch.full_like(idx, -1)).max(-1)[0] if box.shape[1] else torch.full(inside.shape[:2], -1, dtype=torch.int32)
    return winner.int(), x


@pytest.mark.gpu
@pytest.mark.parametrize("N,S,n_obj", OWNER_CASES)
def test_owner_map_and_compaction_at_the_loop_edges(N, S, n_obj):
    """`nlr_box_winner` and `nlr_objects_apply` (both through nlr_box_owner_kernel) against a float32 CPU restatement over the box
    constants the kernel reads; then scan + scatter: exactly the owned samples get a density."""
    import ctypes as C
    from nerflidar_hip import _lib
    g = golden("obj_REF_small")
    mc, _, _, cfgs, sd = _scene(g)
    names = [NAMES[t % 3] for t in range(n_obj)]
    sd.update(nweights.synth_object_state_dict(cfgs, n_obj, seed=int(g["seed"])))
    o, d, td, ts, tracks = _owner_scene(N, S, n_obj)
    mc.config.instance_obj = True
    model = nobj.DynamicModel(mc, sd, tracks, names, obj_log2_hashmap=int(g["log2_hashmap"]))
    box = model.box_params(ts.cuda())
    want, x = _owner_reference(o, d, td, box.cpu())
    # ---- the conditions of the comparison, on the CPU
    margin = float((x.abs() - 1.0).abs().min())
    n_in = (x.abs() < 1.0).all(-1).sum(-1)
    print(f"owner case {(N, S, n_obj)}: margin {margin:.3e}, owned {int((want >= 0).sum())} of {N * S}, in two boxes {int((n_in >= 2).sum())}")
    assert margin > 1e-6                                    # no sample on a box face within rounding
    if n_obj >= 2:
        assert int((n_in >= 2).sum()) >= 1                  # the overlap decides something
    if n_obj >= 3:
        assert not bool((want == n_obj - 1).any())          # a track no sample reaches
    if (N, S, n_obj) != OWNER_CASES[0]:
        assert int((want >= 0).sum()) >= 10
    # ---- nlr_box_winner
    L = _lib.lib()
    od, dd, tdd = o.cuda(), d.cuda(), td.cuda()
    got = torch.full((N, S), -7, dtype=torch.int32, device="cuda")
    _lib.check(L.nlr_box_winner(_lib.ptr(tdd), _lib.ptr(od), _lib.ptr(dd), _lib.ptr(box), N, S, n_obj, _lib.ptr(got), None), "nlr_box_winner")
    assert torch.equal(got.cpu(), want)
    # ---- nlr_objects_apply: the same map, and scan + scatter on a density buffer that starts at -1 (a softplus is never -1)
    rays = _lib.NlrRays()
    rays.origins, rays.directions = od.data_ptr(), dd.data_ptr()
    dens = torch.full((N, S), -1.0, device="cuda")
    got2 = torch.full((N, S), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(L.nlr_objects_workspace_bytes(model._objects, N, S)), dtype=torch.uint8, device="cuda")
    _lib.check(L.nlr_objects_apply(model._objects, C.byref(rays), _lib.ptr(tdd), _lib.ptr(box), N, S, n_obj, _lib.ptr(dens), None, None, 0,
                                   _lib.ptr(got2), _lib.ptr(ws), ws.numel(), None), "nlr_objects_apply")
    torch.cuda.synchronize()
    assert torch.equal(got2.cpu(), want)
    assert torch.equal((dens != -1.0).cpu(), want >= 0)
    # ---- no tracks at all: every sample is free
    got.fill_(-7)
    _lib.check(L.nlr_box_winner(_lib.ptr(tdd), _lib.ptr(od), _lib.ptr(dd), None, N, S, 0, _lib.ptr(got), None), "nlr_box_winner")
    assert bool((got == -1).all())


@pytest.mark.gpu
def test_obj_mlp_stack_has_one_definition_and_two_binders():
    """`objects.ObjMLP` (loaded tensors) and `training.TrainableObjMLP` (modules) bind the same `obj_mlp_forward`: with the same
    weights every output is the same, bit for bit; a 1-D latent is the expanded one."""
    from nerflidar_hip import training as ntrain
    g = golden("obj_REF_small")
    mc, _, cids, cfgs, sd = _scene(g)
    cid = cids[0]
    a = nobj.ObjMLP(f"obj_mlp_{cid}", cfgs[cid], sd, "cuda")
    b = ntrain.TrainableObjMLP(cfgs[cid]).load_reference(sd, f"obj_mlp_{cid}.").cuda()
    gen = torch.Generator().manual_seed(5)
    n = 301
    pts = (torch.rand(n, 3, generator=gen) * 2 - 1).cuda()
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1).cuda()
    lat = torch.randn(n, cfgs[cid].latent_size, generator=gen).cuda()
    with torch.no_grad():
        ra, rb = a.forward(pts, dirs, lat), b(pts, dirs, lat)
        r1, re = a.forward(pts, dirs, lat[0]), a.forward(pts, dirs, lat[:1].expand(n, -1))
    assert list(ra) == list(rb) == ["density", "semantic", "rgb"]
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k
        assert torch.equal(r1[k], re[k]), k
    assert float(ra["density"].max()) > 0 and float(ra["rgb"].std()) > 0
