"""Track refinement (Config.track_refine, nuscenes_single.gin:19-20; train.py:244-268,468-471): TrackNet, its learning rate and
window, the checkpoint round trip - and on the GPU `nlr_obj_frame_backward` alone against float64 autograd through the oracle's
get_pose / box_pts, and the whole step against the reference's (fixture `train_step_TRACK`, tests/golden/make_golden_track.py)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden
from oracle import nlr_oracle as orc
from nerflidar_hip import checkpoints as nckpt, objects as nobj, training as ntrain


def _tracks(n_obj=3, T=5, seed=0):
    rng = np.random.default_rng(seed)
    tr = rng.normal(size=(n_obj, T, 9)).astype(np.float32)
    tr[:, :, 7] = np.linspace(0, 1, T)
    return tr


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_tracknet_forward_adds_the_offsets_to_centre_and_yaw_only():
    raw = _tracks()
    tn = ntrain.TrackNet(raw)
    assert tuple(tn.opt_r.shape) == (3, 5, 1) and tuple(tn.opt_t.shape) == (3, 5, 3)
    assert float(tn.opt_r.detach().abs().sum()) == 0 and float(tn.opt_t.detach().abs().sum()) == 0
    assert np.array_equal(tn().detach().numpy(), raw)
    assert sorted(tn.state_dict()) == ["opt_r", "opt_t"]              # the keys of Track_opt.state_dict() (posenet_v2.py:65-76)
    rng = np.random.default_rng(1)
    with torch.no_grad():
        tn.opt_r.copy_(torch.from_numpy(rng.normal(size=(3, 5, 1)).astype(np.float32)))
        tn.opt_t.copy_(torch.from_numpy(rng.normal(size=(3, 5, 3)).astype(np.float32)))
    out = tn()
    assert out.requires_grad
    want = raw.copy()
    want[:, :, :3] += tn.opt_t.detach().numpy()
    want[:, :, 3:4] += tn.opt_r.detach().numpy()
    assert np.array_equal(out.detach().numpy()[:, :, :4], want[:, :, :4])
    assert np.array_equal(out.detach().numpy()[:, :, 4:], raw[:, :, 4:])
    assert np.array_equal(tn.tracks.numpy(), raw)                     # the recorded tracks stay as they were


def test_create_tracknet_learning_rate_is_the_main_schedule_shifted_to_the_window():
    tn, opt, lr_fn = ntrain.create_tracknet(_tracks(), track_start_opt=5000, max_steps=25000, tn_lr_init=1e-4, tn_lr_final=1e-5)
    for step in (5000, 5001, 7500, 10000):
        assert lr_fn(step) == ntrain.learning_rate_decay(step - 5000, 1e-4, 1e-5, 25000 - 5000, 5000, 1e-8), step
    assert lr_fn(5000) < lr_fn(5001) < lr_fn(7500)
    g = opt.param_groups[0]
    assert tuple(g["betas"]) == (0.9, 0.99) and g["eps"] == 1e-15 and g["lr"] == 1e-4
    assert {id(p) for p in g["params"]} == {id(tn.opt_r), id(tn.opt_t)}
    tn2, _, lr2 = ntrain.create_tracknet(_tracks(), track_start_opt=200, max_steps=1200, tn_lr_init=1e-3, tn_lr_final=1e-4, lr_delay_steps=0)
    assert lr2(700) == ntrain.learning_rate_decay(500, 1e-3, 1e-4, 1000, 0, 1e-8)


class _StubModel(torch.nn.Module):
    """Stands in for TrainableModel in `training_step`: one parameter, records the `curr_track` it is called with."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(()))
        self.calls = []

    def forward(self, batch, train_frac=1.0, randomized=False, color_rays=None, **kw):
        self.calls.append(kw)
        track = kw.get("curr_track")
        x = self.w * (1.0 if track is None else (track[:, :, :4] * batch["c"]).sum())
        return [{"x": x}], []


def test_training_step_window_logic(monkeypatch):
    """train.py:245-266,468-471: no track up to the start of the window, the refined track with gradient inside it (learning rate
    set, TrackNet stepped), the refined track without gradient after it; (sic) step == start + 5000 matches neither comparison."""
    from nerflidar_hip import losses as nl
    monkeypatch.setattr(nl, "total_loss", lambda rend, hist, batch, **kw: {"data": rend[-1]["x"]})
    raw = _tracks()
    tn, tn_opt, lr_fn = ntrain.create_tracknet(raw, track_start_opt=100, max_steps=10000)
    with torch.no_grad():
        tn.opt_t.fill_(0.25)
        tn.opt_r.fill_(-0.5)
    model = _StubModel()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    batch = {"c": torch.from_numpy(np.random.default_rng(3).normal(size=(3, 5, 4)).astype(np.float32))}
    kw = dict(randomized=False, hash_decay_mult=0.0, tracknet=tn, tn_optimizer=tn_opt, tn_lr_fn=lr_fn, track_start_opt=100)
    refined = tn().detach().clone()

    def run(step):
        before = (tn.opt_r.detach().clone(), tn.opt_t.detach().clone())
        model.calls.clear()
        ntrain.training_step(model, opt, batch, step=step, **kw)
        (call,) = model.calls
        moved = not (torch.equal(before[0], tn.opt_r) and torch.equal(before[1], tn.opt_t))
        return call["curr_track"], moved

    for step in (0, 99, 100, 5100):                                   # before the window, its (excluded) ends
        track, moved = run(step)
        assert track is None and not moved, step
    for step in (5101, 9000):                                         # after it
        track, moved = run(step)
        assert track is not None and not track.requires_grad and not moved, step
        assert torch.equal(track, refined)
    tn_opt.param_groups[0]["lr"] = 123.0
    track, moved = run(101)                                           # inside
    assert track is not None and track.requires_grad and moved
    assert torch.equal(track.detach(), refined)
    assert tn_opt.param_groups[0]["lr"] == lr_fn(101)
    track, moved = run(5099)
    assert track.requires_grad and moved and tn_opt.param_groups[0]["lr"] == lr_fn(5099)
    # without a TrackNet the model is called exactly as before: no curr_track argument at all
    model.calls.clear()
    ntrain.training_step(model, opt, batch, randomized=False, hash_decay_mult=0.0)
    assert model.calls == [{}]
    with pytest.raises(ValueError, match="step"):
        ntrain.training_step(model, opt, batch, randomized=False, hash_decay_mult=0.0, tracknet=tn, tn_optimizer=tn_opt, tn_lr_fn=lr_fn)
    assert [ntrain.track_phase(s, 5000) for s in (5000, 5001, 9999, 10000, 10001)] == ["before", "refine", "refine", "before", "frozen"]


def test_tracknet_checkpoint_round_trip(tmp_path):
    raw = _tracks(4, 6, seed=5)
    tn, tn_opt, _ = ntrain.create_tracknet(raw)
    rng = np.random.default_rng(2)
    with torch.no_grad():
        tn.opt_r.copy_(torch.from_numpy(rng.normal(size=(4, 6, 1)).astype(np.float32) * 0.01))
        tn.opt_t.copy_(torch.from_numpy(rng.normal(size=(4, 6, 3)).astype(np.float32) * 0.01))
    path = nckpt.save_checkpoint(tmp_path, tn.state_dict(), 7000, optimizer_state=tn_opt.state_dict(), prefix="tracknet_ckpt_")
    assert os.path.basename(path) == "tracknet_ckpt_7000.ckpt"
    nckpt.save_checkpoint(tmp_path, {"opt_r": torch.zeros(4, 6, 1), "opt_t": torch.zeros(4, 6, 3)}, 6000, prefix="tracknet_ckpt_")
    nckpt.save_checkpoint(tmp_path, {"x": torch.zeros(1)}, 9000)      # the model's own checkpoint in the same directory
    sd, step = nckpt.load_checkpoint(tmp_path, prefix="tracknet_ckpt_")
    assert step == 7000 and sorted(sd) == ["opt_r", "opt_t"]
    tn2 = ntrain.TrackNet(raw)
    tn2.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    assert torch.equal(tn2(), tn())
    got = nckpt.refined_tracks_from_checkpoint(tmp_path, raw)
    assert got.dtype == np.float32 and np.array_equal(got, tn().detach().numpy())
    assert np.array_equal(nckpt.refined_tracks_from_checkpoint(tmp_path, raw, step=6000), raw)
    with pytest.raises(ValueError, match="opt_t"):
        nckpt.refined_tracks_from_checkpoint(tmp_path, raw[:3])
    from nerflidar_hip import render_lidar
    a = render_lidar.parse_args(["--synthetic-tracks", "2", "--tracknet-ckpt", str(tmp_path)])
    assert a.tracknet_ckpt == str(tmp_path)
    with pytest.raises(SystemExit):
        render_lidar.parse_args(["--tracknet-ckpt", str(tmp_path)])


def test_track_fixture_conditions():
    """What tests/golden/make_golden_track.py asserts when it writes the fixture, checked on the file."""
    assert os.path.getsize(os.path.join(GOLDEN, "train_step_TRACK.npz")) <= 400 * 1000
    g = golden("train_step_TRACK")
    n_obj, T = g["tracks"].shape[:2]
    assert g["opt_r"].shape == (n_obj, T, 1) and g["opt_t"].shape == (n_obj, T, 3)
    assert np.all(g["opt_r"] != 0) and np.all(g["opt_t"] != 0) and np.abs(g["opt_t"]).max() < 1e-3 and np.abs(g["opt_r"]).max() < 1e-2
    for t in range(n_obj):
        assert int((g["hist2_owner"] == t).sum()) > 0, f"track {t} owns no sample on the last level"
        # non-zero, and large enough for the per-track gates of the model test to be exact arithmetic (float32 normal numbers)
        assert np.abs(g["grad_opt_r"][t]).max() > 1e-36 and np.abs(g["grad_opt_t"][t]).max() > 1e-36, f"track {t} without gradient"
    for lvl in range(3):
        assert np.array_equal(g[f"hist{lvl}_owner"] >= 0, g[f"hist{lvl}_obj_mask"])
    # conditioning of the scene, measured by the generator on the reference alone: what an ulp-level change of the track moves
    assert g["ulp_moves_depth"] <= 2e-4 / 3 and g["ulp_moves_grad_opt_r"] <= 5e-3 / 3 and g["ulp_moves_grad_opt_t"] <= 5e-3 / 3


# ---- GPU: the kernel alone -------------------------------------------------------------------------------------------------
def _rays(N, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(N, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    v = d + 0.05 * rng.normal(size=(N, 3)).astype(np.float32)          # a view direction that is not the ray direction
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    return {"origins": (0.02 * rng.normal(size=(N, 3))).astype(np.float32), "directions": d, "viewdirs": v.astype(np.float32)}


def _big_box(batch, ray, T, wlh, theta=0.7, track_id=0, depth=0.25):
    """One track whose box (edges wlh) sits on `ray` at `depth` for all T records."""
    c = batch["origins"][ray] + depth * batch["directions"][ray]
    tr = np.zeros((T, 9), np.float32)
    for i, t in enumerate(np.linspace(0, 1, T)):
        tr[i] = np.concatenate([c + 0.01 * (t - 0.5), [theta + 0.2 * t], wlh, [t], [track_id]])
    return tr


def _case(name):
    """-> rays, tdist [N,S+1], timestamps [N], tracks [n_obj,T,9], and a cut of the owned list (None = all of it)."""
    cut = None
    if name in ("base", "K1", "K0"):
        N, S = 37, 9
        b = _rays(N, 1)
        tracks = nobj.synthetic_tracks(b, n_tracks=3, n_times=5, seed=1, size=(0.4, 0.3, 0.3), depth=(0.1, 0.3))
        cut = {"K1": 1, "K0": 0}.get(name)
    elif name == "T2":
        N, S = 37, 9
        b = _rays(N, 2)
        tracks = nobj.synthetic_tracks(b, n_tracks=3, n_times=2, seed=2, size=(0.4, 0.3, 0.3), depth=(0.1, 0.3))
    elif name == "blocks":                                             # several workgroups, runs that cross wave and workgroup ends
        N, S = 300, 16
        b = _rays(N, 3)
        tracks = nobj.synthetic_tracks(b, n_tracks=5, n_times=4, seed=3, size=(0.6, 0.5, 0.5), depth=(0.1, 0.3))
    elif name == "run":                                                # every ray owns all its S > 64 samples of the one track
        N, S = 3, 70
        b = _rays(N, 4)
        b["origins"][:] = b["origins"][0]
        b["directions"][:] = b["directions"][0]
        tracks = _big_box(b, 0, 5, [2.0, 2.5, 3.0])[None]
    elif name == "overlap":                                            # track 1 inside track 0: the owner is the LAST
        N, S = 37, 9
        b = _rays(N, 5)
        tracks = np.stack([_big_box(b, 0, 5, [2.0, 2.5, 3.0], 0.7, 0, depth=0.0), _big_box(b, 0, 5, [0.5, 0.6, 0.7], -1.1, 1, depth=0.0)])
    elif name == "nested":                                             # along a ray the owner goes 0 -> 1 -> 0: runs of one pair that are not adjacent
        N, S = 5, 40
        b = _rays(N, 8)
        b["origins"][:] = b["origins"][0]
        b["directions"][:] = b["directions"][0]
        tracks = np.stack([_big_box(b, 0, 5, [2.0, 2.5, 3.0], 0.7, 0), _big_box(b, 0, 5, [0.2, 0.25, 0.3], -1.1, 1)])
    elif name == "iters":                                              # more than 128 x 256 owned samples: every workgroup loops over its share
        N, S = 2500, 32
        b = _rays(N, 9)
        tracks = nobj.synthetic_tracks(b, n_tracks=4, n_times=6, seed=9, size=(1.2, 1.0, 1.0), depth=(0.1, 0.3))
    elif name == "ref":                                                # the size of a REF training batch's last level: more than 10^6 owned
        N, S = 36000, 32                                               # samples, a slot table of 3 x 20 x 7 = 420 floats, ~35 trips per workgroup,
        b = _rays(N, 10)                                               # owners that change and come back along a ray (box 1 inside box 0)
        tracks = np.stack([_big_box(b, 0, 20, [2.0, 2.5, 3.0], 0.7, 0, depth=0.0), _big_box(b, 0, 20, [0.5, 0.6, 0.7], -1.1, 1, depth=0.15),
                           _big_box(b, 1, 20, [0.3, 0.3, 0.3], 0.4, 2, depth=0.3)])
    elif name == "times":                                              # clamp and tie paths of get_pose
        N, S = 37, 9
        b = _rays(N, 6)
        tracks = np.stack([_big_box(b, 0, 5, [2.0, 2.5, 3.0], 0.7, 0, depth=0.0), _big_box(b, 0, 5, [0.5, 0.6, 0.7], -1.1, 1, depth=0.0)])
    elif name == "T300":                                               # 2 * 300 * 7 = 4200 floats: the large LDS table (the usual one holds 4096)
        N, S = 37, 9
        b = _rays(N, 12)
        tracks = nobj.synthetic_tracks(b, n_tracks=2, n_times=300, seed=12, size=(0.5, 0.4, 0.4), depth=(0.1, 0.3))
    elif name == "T3000":                                              # 2 * 3000 * 7 floats = 168 KB: beyond the LDS slot table
        N, S = 37, 9
        b = _rays(N, 7)
        tracks = nobj.synthetic_tracks(b, n_tracks=2, n_times=3000, seed=7, size=(0.5, 0.4, 0.4), depth=(0.1, 0.3))
    else:
        raise KeyError(name)
    rng = np.random.default_rng(11)
    tdist = np.sort(rng.uniform(0.01, 0.5, size=(N, S + 1)).astype(np.float32), axis=-1)
    ts = rng.uniform(0, 1, size=N).astype(np.float32)
    if name == "times":   # before the first record, after the last, on a record, midway between two, on the first / last record
        ts = np.resize(np.array([-0.3, 1.4, 0.5, 0.375, 0.0, 1.0, 0.125, 0.25], np.float32), N)
    return b, tdist, ts, np.ascontiguousarray(tracks, np.float32), cut


CASES = ["base", "T2", "K1", "K0", "blocks", "iters", "run", "overlap", "nested", "ref", "times", "T300", "T3000"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_obj_frame_backward_matches_float64_autograd(name):
    """`nlr_obj_frame_backward` against float64 autograd through `oracle.nlr_oracle.obj_get_pose` + `obj_box_pts` on the CPU,
    contracted with seeded cotangents on the owned list (owners from `nlr_box_winner`).  Per column 0..6:
    max|got - want| <= 2e-5 max|want| (the gate of the other f32 backward kernels); columns 7 and 8 exactly 0."""
    from nerflidar_hip import _lib
    b, tdist, ts, tracks, cut = _case(name)
    N, S = tdist.shape[0], tdist.shape[1] - 1
    n_obj, T = tracks.shape[:2]
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    o, d, v, td, tsd, trk = cu(b["origins"]), cu(b["directions"]), cu(b["viewdirs"]), cu(tdist), cu(ts), cu(tracks)
    box = torch.empty(N, n_obj, 8, device="cuda")
    winner = torch.empty(N, S, dtype=torch.int32, device="cuda")
    L = _lib.lib()
    _lib.check(L.nlr_track_box_params(_lib.ptr(trk), _lib.ptr(tsd), N, n_obj, T, _lib.ptr(box), _lib.current_stream()))
    _lib.check(L.nlr_box_winner(_lib.ptr(td), _lib.ptr(o), _lib.ptr(d), _lib.ptr(box), N, S, n_obj, _lib.ptr(winner), _lib.current_stream()))
    sel = (winner >= 0).nonzero()
    ri, si = sel[:, 0], sel[:, 1]
    tr = winner[ri, si].long()
    K_all = int(ri.shape[0])
    if name == "base":
        assert K_all > 64 and K_all % 64 != 0, K_all
        assert len(set(tr.tolist())) == n_obj
    if name == "blocks":
        assert K_all > 3 * 256, K_all
    if name == "run":
        assert K_all == N * S and S > 64
    if name == "ref":
        assert K_all >= 1_000_000 and n_obj * T * 7 > 256 and len(set(tr[:100000].tolist())) == 3, K_all
    if name == "iters":
        assert K_all > 128 * 256 + 256, K_all
    if name == "nested":
        row = winner[0].cpu().tolist()
        assert row[0] == 0 and row[-1] == 0 and 1 in row, row
    if name == "overlap":
        assert set(tr.tolist()) == {0, 1}
        p_cpu = orc.obj_box_pts((0.5 * (td[:, :-1] + td[:, 1:])[..., None] * d[:, None] + o[:, None]).cpu(), v.cpu(),
                                orc.obj_get_pose(tsd.cpu()[:, None], trk.cpu()))[0]
        both = (p_cpu.abs() < 0.99).all(-1).all(-1)                                   # well inside both boxes ...
        assert bool(both.any()) and bool((winner.cpu()[both] == 1).all())             # ... belongs to the last track
    if name in ("times", "T2", "T300", "T3000"):
        assert K_all > 0
    if name == "T300":
        assert 4096 < n_obj * T * 7 <= 39936
    if name == "T3000":
        assert n_obj * T * 7 * 4 > 160 * 1024 and L.nlr_obj_frame_backward_workspace_bytes(K_all, n_obj, T) == 0
    else:
        assert (L.nlr_obj_frame_backward_workspace_bytes(K_all, n_obj, T) > 0) == (K_all > 0)
    if cut is not None:
        ri, si, tr = ri[:cut], si[:cut], tr[:cut]
    K = int(ri.shape[0])
    gen = torch.Generator().manual_seed(17)
    g_pts, g_dirs = torch.randn(K, 3, generator=gen), torch.randn(K, 3, generator=gen)
    # float64 autograd on the CPU
    t64 = torch.from_numpy(tracks).double().requires_grad_(True)
    pose = orc.obj_get_pose(torch.from_numpy(ts).double()[:, None], t64)
    tm = 0.5 * (torch.from_numpy(tdist[:, :-1]).double() + torch.from_numpy(tdist[:, 1:]).double())
    pts_w = tm[..., None] * torch.from_numpy(b["directions"]).double()[:, None] + torch.from_numpy(b["origins"]).double()[:, None]
    p_o, d_o, _ = orc.obj_box_pts(pts_w, torch.from_numpy(b["viewdirs"]).double(), pose)
    rc, sc, tc = ri.cpu(), si.cpu(), tr.cpu()
    loss = (p_o[rc, sc, tc] * g_pts.double()).sum() + (d_o[rc, sc, tc] * g_dirs.double()).sum()
    want = torch.autograd.grad(loss, t64)[0].numpy() if K else np.zeros_like(tracks, np.float64)
    got = ntrain.obj_frame_backward(trk, tsd, o, d, v, td, ri.int().contiguous(), si.int().contiguous(), tr.int().contiguous(),
                                    g_pts.cuda(), g_dirs.cuda())
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == tracks.shape
    assert np.all(got[..., 7:] == 0)
    for c in range(7):
        err, scale = float(np.abs(got[..., c] - want[..., c]).max()), float(np.abs(want[..., c]).max())
        print(f"{name}: column {c}: max err {err:.3e}, max |want| {scale:.3e}, K = {K}")
        assert K == 0 or scale > 0, c
        assert err <= 2e-5 * scale, (name, c, err, scale)


# ---- GPU: through the model ------------------------------------------------------------------------------------------------
def _track_scene(g):
    from nerflidar_hip import losses as nl, weights as nweights, lidar as nlidar2, config as ncfg
    lg, seed = int(g["log2_hashmap"]), int(g["seed"])
    mc = ncfg.workload("REF", lg)
    mc.config.instance_obj, mc.config.latent_size = True, 128
    mc.__post_init__()
    names = {13: "vehicle.car", 14: "vehicle.truck", 15: "vehicle.bus.rigid", 11: "human.pedestrian.adult"}
    class_names = [names[int(c)] for c in g["class_ids"]]
    sd = nweights.synth_state_dict(mc, seed=seed, trained_like=True)
    cids = sorted(set(int(c) for c in g["class_ids"]))
    sd.update(nweights.synth_object_state_dict({c: ncfg.obj_mlp_config(c, latent_size=128, log2_hashmap=lg) for c in cids}, len(class_names), seed=seed))
    b = nlidar2.synthetic_sweep(width=int(g["width"]), seed=seed, beams=list(g["beams"]))
    batch = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    batch["timestamp"] = torch.from_numpy(g["timestamp"]).cuda()
    for k in ("rgb", "depth", "semantic", "mask", "patch_mask", "lidar_mask"):
        batch[k] = torch.from_numpy(g["sup_" + k]).cuda()
    masks = nl.nusc_masks(batch, lidar_supervision=True, instance_obj=True)
    assert torch.equal(masks["mask_rgb"].cpu(), torch.from_numpy(g["mask_rgb"]))
    batch.update(masks)
    tm = ntrain.TrainableModel(mc, tracks=g["tracks"], class_names=class_names, obj_log2_hashmap=lg).cuda().load_reference(sd)
    return tm, batch


@pytest.mark.gpu
def test_track_refinement_step_matches_the_reference_step():
    """The reference's step with a refined track that requires a gradient (`model(False, batch, ..., curr_track=track)`, track from
    train.py:251-256, loss block of train.py, `.backward()`: tests/golden/make_golden_track.py) against TrainableModel + TrackNet:
    owner maps exactly, loss terms to 2e-4, and `opt_r.grad` / `opt_t.grad` to 5e-3 of their norm with a cosine of at least 0.99999,
    the gates of every other gradient of this step (test_training.py)."""
    from nerflidar_hip import losses as nl
    g = golden("train_step_TRACK")
    tm, batch = _track_scene(g)
    tn = ntrain.TrackNet(g["tracks"]).cuda()
    with torch.no_grad():
        tn.opt_r.copy_(torch.from_numpy(g["opt_r"]))
        tn.opt_t.copy_(torch.from_numpy(g["opt_t"]))
    rend, hist = tm(batch, train_frac=float(g["train_frac"]), randomized=False, curr_track=tn())
    for lvl, h in enumerate(hist):
        assert torch.equal(h["obj_mask"].cpu(), torch.from_numpy(g[f"hist{lvl}_obj_mask"])), f"owner map of level {lvl}"
    terms = nl.total_loss(rend, hist, batch, depth_lam=0.1, sem_lam=0.01)
    terms["latent_reg"] = tm.latent_reg(float(g["latent_reg"]))
    loss = sum(terms.values())
    loss.backward()
    ntrain.clip_gradients(tm)
    ntrain.clip_gradients(tn)
    assert set(terms) == {k[5:] for k in g if k.startswith("loss_")}
    for k, v in terms.items():
        np.testing.assert_allclose(float(v.detach()), float(g["loss_" + k]), rtol=2e-4, atol=1e-7, err_msg=k)
    np.testing.assert_allclose(float(loss.detach()), float(g["loss"]), rtol=2e-4)
    np.testing.assert_allclose(rend[-1]["depth"].detach().cpu().numpy(), g["out_depth"], atol=2e-4, rtol=0)
    report = []
    for k, p in (("opt_r", tn.opt_r), ("opt_t", tn.opt_t)):
        assert p.grad is not None, f"{k}.grad is None: no gradient reached the tracks"
        got, want = p.grad.detach().cpu().double(), torch.from_numpy(g["grad_" + k]).double()
        rel = float((got - want).norm() / want.norm())
        cos = float((got * want).sum() / (got.norm() * want.norm()))
        ok = rel <= 5e-3 and cos >= 0.99999
        report.append(f"{'ok ' if ok else 'BAD'} {k}: rel {rel:.2e} cos {cos:.6f}")
        for t in range(got.shape[0]):   # and per track: the tracks' gradients differ by 30 orders of magnitude, the whole-tensor norm sees the largest only
            rel = float((got[t] - want[t]).norm() / want[t].norm())
            cos = float((got[t] * want[t]).sum() / (got[t].norm() * want[t].norm()))
            ok = rel <= 5e-3 and cos >= 0.99999
            report.append(f"{'ok ' if ok else 'BAD'} {k}[track {t}]: rel {rel:.2e} cos {cos:.6f} (max |want| {float(want[t].abs().max()):.1e})")
    print("\n".join(report))
    assert not [r for r in report if r.startswith("BAD")], "\n".join(report)


@pytest.mark.gpu
def test_a_track_without_gradient_leaves_the_step_bit_identical(monkeypatch):
    """`curr_track` given but not requiring a gradient: all renderings, the ray history and all parameter gradients are bit-identical to
    `curr_track=None` on the same tracks (the path without `_ObjFrame`).
    One kind of gradient has no bits to be identical to: a hash table's, which the grid scatter sums with float atomics, so that two
    runs of the SAME call differ in the order of additions (the test runs the baseline twice and prints what that alone moves).  For
    those the test pins what decides them instead: every call that makes a table gradient - `_EncodeFeatures.backward` of the static
    levels, `GridSpec.scatter` of the object grids - receives bit-identical inputs on both paths (cotangent, positions, table), in the
    same order.  The table gradients themselves are then held to the gate of the project's f32 backward kernels, 2e-5 of the largest
    entry."""
    from nerflidar_hip import gridencoder as ngrid, losses as nl
    g = golden("train_step_TRACK")
    tm, batch = _track_scene(g)
    calls = []
    enc_bwd, scatter = ntrain._EncodeFeatures.backward, ngrid.GridSpec.scatter

    def spy_enc(ctx, grad):
        calls.append(("encode", grad.detach().clone(), ctx.args[2].clone(), ctx.saved_tensors[0].clone()))
        return enc_bwd(ctx, grad)

    def spy_scatter(self, grad, x01, table, dy_dx):
        calls.append(("scatter", grad.detach().clone(), x01.detach().clone(), table.detach().clone()))
        return scatter(self, grad, x01, table, dy_dx)

    monkeypatch.setattr(ntrain._EncodeFeatures, "backward", staticmethod(spy_enc))
    monkeypatch.setattr(ngrid.GridSpec, "scatter", spy_scatter)

    def step(**kw):
        tm.zero_grad(set_to_none=True)
        calls.clear()
        rend, hist = tm(batch, train_frac=float(g["train_frac"]), randomized=False, **kw)
        sum(nl.total_loss(rend, hist, batch, depth_lam=0.1, sem_lam=0.01).values()).backward()
        return rend, hist, {k: p.grad.clone() for k, p in tm.named_parameters() if p.grad is not None}, list(calls)

    r0, h0, g0, c0 = step()
    _, _, g0b, _ = step()                                              # the same call again: what the atomics' order alone moves
    r1, h1, g1, c1 = step(curr_track=tm.tracks.clone())
    with torch.no_grad():
        r2, h2 = tm(batch, train_frac=float(g["train_frac"]), randomized=False, curr_track=tm.tracks.clone().requires_grad_(True))
    for a, b_ in ((r0, r1), (h0, h1), (r0, r2), (h0, h2)):
        for la, lb in zip(a, b_):
            assert set(la) == set(lb)
            for k in la:
                assert torch.equal(la[k], lb[k]), k
    assert set(g0) == set(g1) and len(g0) > 20
    tables = [k for k in g0 if k.endswith("encoder.embeddings")]
    assert len(tables) >= 4 and len(c0) == len(tables), (tables, [c[0] for c in c0])   # one maker per table: none escaped the spies
    assert len(c0) == len(c1)
    for i, (a, b_) in enumerate(zip(c0, c1)):                          # the makers of the table gradients: same calls, same input bits
        assert a[0] == b_[0], i
        for x, y in zip(a[1:], b_[1:]):
            assert torch.equal(x, y), (i, a[0])
    for k in g0:
        if k in tables:
            scale = float(g0[k].abs().max())
            same_call, cross = float((g0[k] - g0b[k]).abs().max()), float((g0[k] - g1[k]).abs().max())
            print(f"{k}: same call twice moves {same_call:.2e}, the two paths differ by {cross:.2e} (largest entry {scale:.2e})")
            assert cross <= 2e-5 * scale, k
        else:
            assert torch.equal(g0[k], g0b[k]) and torch.equal(g0[k], g1[k]), k
    # and with a gradient the values are still those bits: _ObjFrame's forward is the same expressions
    r3, h3 = tm(batch, train_frac=float(g["train_frac"]), randomized=False, curr_track=tm.tracks.clone().requires_grad_(True))
    for la, lb in zip(r0 + h0, r3 + h3):
        for k in la:
            assert torch.equal(la[k], lb[k].detach()), k


@pytest.mark.gpu
def test_training_step_refines_the_tracks_inside_the_window_only():
    g = golden("train_step_TRACK")
    tm, batch = _track_scene(g)
    opt = torch.optim.Adam(tm.parameters(), lr=1e-4, eps=1e-15)   # small steps: the three calls below see nearly the same model
    tn, tn_opt, lr_fn = ntrain.create_tracknet(g["tracks"], track_start_opt=5000, max_steps=25000)
    tn = tn.cuda()
    seen = []
    fwd = tm.forward
    tm.forward = lambda *a, **kw: (seen.append(kw.get("curr_track")), fwd(*a, **kw))[1]
    kw = dict(train_frac=0.5, randomized=False, depth_lam=0.1, sem_lam=0.01, tracknet=tn, tn_optimizer=tn_opt, tn_lr_fn=lr_fn, track_start_opt=5000)
    out = ntrain.training_step(tm, opt, batch, step=4000, **kw)
    assert np.isfinite(out["loss"]) and seen[-1] is None
    assert float(tn.opt_t.detach().abs().sum()) == 0 and float(tn.opt_r.detach().abs().sum()) == 0 and tn.opt_t.grad is None
    ntrain.training_step(tm, opt, batch, step=7000, **kw)
    assert seen[-1] is not None and seen[-1].requires_grad
    assert tn_opt.param_groups[0]["lr"] == lr_fn(7000)
    moved_t, moved_r = tn.opt_t.detach().clone(), tn.opt_r.detach().clone()
    assert float(moved_t.abs().max()) > 0 and float(moved_r.abs().max()) > 0
    # Adam's first step moves an entry whose gradient is well above eps by the learning rate
    assert float(moved_t.abs().max()) > 0.5 * lr_fn(7000) and float(moved_r.abs().max()) > 0.5 * lr_fn(7000)
    ntrain.training_step(tm, opt, batch, step=12000, **kw)
    assert torch.equal(tn.opt_t, moved_t) and torch.equal(tn.opt_r, moved_r)
    assert seen[-1] is not None and not seen[-1].requires_grad and torch.equal(seen[-1], tn().detach())
    assert not torch.equal(seen[-1][:, :, :4], tm.tracks[:, :, :4])   # the model rendered the refined track, not the recorded one
