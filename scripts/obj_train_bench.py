"""The dynamic-object training step with the torch object merge and with the fused object operator (header section 7e), at the REF
object batch of track_refine_bench.py / pose_obj_bench.py: 65 536 rays, 8 synthetic tracks with T = 20 recorded poses.
Step: `training.training_step(as_tensors=True)` of `TrainableModel(fused_mlp=True, fused_objects=False)` (the yardstick: the path of
the parent commit) and of `fused_objects=True`, two models in one process on one device, alternating, wall clock between device
synchronisations around `--steps` steps, five repetitions each, medians.
Operator: `nlr_obj_train_forward` (rgb form) and `nlr_obj_train_backward` alone on the last level's shape, HIP events around 10 calls
after 2 warm-up calls, five repetitions, with the number of owned samples.
--refine {none,track,pose,both}: the step inside the refinement windows - a `TrackNet` and / or a `PoseNet` with their optimisers, as
`training_step` runs them - on `fused_objects=False` (the yardstick: the parent commit's only way to run these steps) and on
`fused_objects=True, fused_object_frame=True`, by the same protocol; the operator part then also times `nlr_obj_train_backward_frame`
and the dense-list calls of `nlr_obj_frame_backward` / `nlr_obj_frame_backward_rays` at K = N * S.
    python scripts/obj_train_bench.py > profiles/obj_train_bench.txt
    for m in none track pose both; do python scripts/obj_train_bench.py --refine $m; done > profiles/obj_frame_bench.txt"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-lidar_amd")); sys.path.insert(0, ROOT)
import numpy as np, torch
from nerflidar_hip import _lib, config as nconfig, lidar as nlidar, objects as nobj, training as ntrain, weights as nweights

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=65536)
ap.add_argument("--tracks", type=int, default=8)
ap.add_argument("--records", type=int, default=20)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--refine", choices=("none", "track", "pose", "both"), default="none")
a = ap.parse_args()
dev = "cuda"
print(f"build {_lib.lib().nlr_build_sha().decode()}  device {torch.cuda.get_device_name(0)}", flush=True)
stat = lambda t: f"min {min(t):.3f}  median {float(np.median(t)):.3f}  max {max(t):.3f} ms"


def timed(fn, calls=10, warm=2):
    for _ in range(warm): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls): fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / calls


mc = nconfig.workload("REF", 12)
mc.config.instance_obj, mc.config.latent_size = True, 128
mc.__post_init__()
b = nlidar.synthetic_sweep(width=a.rays // 32, seed=0)
b["timestamp"] = nobj.synthetic_timestamps(b["origins"].shape[0], 0)
tracks_np = nobj.synthetic_tracks(b, n_tracks=a.tracks, n_times=a.records, seed=0)
batch = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
n, S = batch["origins"].shape[0], mc.level_samples()[-1]
n_obj = tracks_np.shape[0]
gen = torch.Generator(device=dev).manual_seed(0)
batch.update(rgb=torch.rand(n, 3, device=dev, generator=gen), depth=torch.rand(n, device=dev, generator=gen) * 0.5 + 0.05,
             semantic=torch.randint(0, 19, (n,), device=dev, generator=gen))
classes = (["vehicle.car", "vehicle.truck", "vehicle.bus.rigid"] * n_obj)[:n_obj]
sd = nweights.synth_state_dict(mc, seed=0, trained_like=True)
sd.update(nweights.synth_object_state_dict({c: nconfig.obj_mlp_config(c, latent_size=128, log2_hashmap=12) for c in sorted({nobj.query_class(c) for c in classes})},
                                           n_obj, seed=0))

# ---- the whole step, the two paths alternating ----------------------------------------------------------------------------------
refine_track, refine_pose = a.refine in ("track", "both"), a.refine in ("pose", "both")
frame = a.refine != "none"
if refine_pose:
    batch["glo_idx"] = torch.ones(n, dtype=torch.int64, device=dev)   # one camera pose, one LiDAR pose: every ray is the sweep's


def refine_kw():
    """A TrackNet / PoseNet with their optimisers and a step number inside both windows (track 5 000 .. 10 000, pose 4 000 .. 20 000)."""
    kw = {}
    if refine_track:
        tn, tn_opt, tn_lr = ntrain.create_tracknet(tracks_np, track_start_opt=5000, max_steps=25000)
        kw.update(tracknet=tn.to(dev), tn_optimizer=tn_opt, tn_lr_fn=tn_lr, track_start_opt=5000)
    if refine_pose:
        pn, pn_opt, pn_lr = ntrain.create_posenet(1, num_lidars=1, start_step=4000, end_step=20000)
        kw.update(posenet=pn.to(dev), pn_optimizer=pn_opt, pn_lr_fn=pn_lr, pose_window=(4000, 20000))
    if kw:
        kw["step"] = 7000
    return kw


models = {}
for fused in (False, True):
    tm = ntrain.TrainableModel(mc, fused_mlp=True, tracks=tracks_np, class_names=classes, obj_log2_hashmap=12, fused_objects=fused,
                               fused_object_frame=fused and frame).to(dev).load_reference(sd)
    models[fused] = (tm, torch.optim.Adam(tm.parameters(), lr=1e-3, eps=1e-15), refine_kw())
    torch.manual_seed(0)
    for _ in range(2): out = ntrain.training_step(*models[fused][:2], batch, **models[fused][2])
    print(f"fused_objects={fused}: loss after two steps {out['loss']:.6f}", flush=True)
ms = {False: [], True: []}
for _ in range(5):
    for fused in (False, True):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(a.steps): ntrain.training_step(*models[fused][:2], batch, as_tensors=True, **models[fused][2])
        torch.cuda.synchronize(); ms[fused].append((time.perf_counter() - t0) / a.steps * 1e3)
spread = lambda t: f"{(max(t) - min(t)) / float(np.median(t)) * 100:.1f} %"
print(f"step, {n} rays, {n_obj} tracks, fused_mlp=True, refine={a.refine}\n"
      f"  fused_objects=False (torch merge): {stat(ms[False])} per step, spread {spread(ms[False])}\n"
      f"  fused_objects=True{', fused_object_frame=True' if frame else '  (section 7e)'}: {stat(ms[True])} per step, spread {spread(ms[True])}\n"
      f"  median True / median False = {float(np.median(ms[True])) / float(np.median(ms[False])):.4f}", flush=True)

# ---- the operator alone, last level's shape ----------------------------------------------------------------------------------------
tm = models[True][0]
plan = tm._obj_plan
mlps = [getattr(tm, f"obj_mlp_{cid}") for cid in tm._class_list]
td = torch.sort(torch.rand(n, S + 1, device=dev, generator=gen) * 0.4 + 0.01, dim=-1)[0].contiguous()
box = nobj.track_box_params(tm.tracks, batch["timestamp"])
rays, keep = _lib.rays({k: batch[k] for k in ("origins", "directions", "viewdirs")}, n, optional=_lib.RAY_KEYS)
tabs = [m.encoder.embeddings.detach() for m in mlps]
lat = torch.stack([tm.latent_vector_dict[f"obj_latent_{t}"].detach() for t in range(n_obj)])
plan.pack([plan.flat(c, m).detach() for c, m in enumerate(mlps)])
need = _lib.lib().nlr_obj_train_workspace_bytes(plan.handle, n, S, 1)
ws = torch.empty(need, dtype=torch.uint8, device=dev)
dens, rgb, sem = torch.rand(n, S, device=dev), torch.rand(3, n, S, device=dev), torch.rand(19, n, S, device=dev)
gd, gr = torch.randn(n, S, device=dev), torch.randn(3, n, S, device=dev)
d_flats, d_lat, g_tabs = [torch.empty(k, device=dev) for k in plan.n_params], torch.empty_like(lat), [torch.zeros_like(t) for t in tabs]
fwd = lambda: ntrain.objects_forward(plan, tabs, lat, rays, td, box, dens, rgb, sem, workspace=ws)
bwd = lambda: _lib.call("nlr_obj_train_backward", plan.handle, ntrain._ptr_array(tabs), lat, rays, td, box, n, S, n_obj, gd, gr,
                        ntrain._ptr_array(d_flats), d_lat, ntrain._ptr_array(g_tabs), ws, ws.numel())
owned = int((fwd() >= 0).sum())
tf, tb = [], []
for _ in range(5):
    tf.append(timed(fwd)); tb.append(timed(bwd))
print(f"operator, {n} x {S} samples, {owned} owned, workspace {need / 2**30:.2f} GiB\n"
      f"  nlr_obj_train_forward:  {stat(tf)}\n"
      f"  nlr_obj_train_backward: {stat(tb)}", flush=True)
if frame:
    g_pts, g_dirs = torch.empty(n * S, 3, device=dev), torch.empty(n * S, 3, device=dev)
    bwf = lambda: _lib.call("nlr_obj_train_backward_frame", plan.handle, ntrain._ptr_array(tabs), lat, rays, td, box, n, S, n_obj, gd, gr,
                            ntrain._ptr_array(d_flats), d_lat, ntrain._ptr_array(g_tabs), g_pts, g_dirs, ws, ws.numel())
    winner = fwd()
    ri, si = ntrain._dense_sample_index(n, S, dev)
    trk, ts = winner.reshape(-1), batch["timestamp"].reshape(-1).float().contiguous()
    o3, d3, v3 = (batch[k].reshape(n, 3).float().contiguous() for k in ("origins", "directions", "viewdirs"))
    f7c = lambda: ntrain.obj_frame_backward(tm.tracks, ts, o3, d3, v3, td, ri, si, trk, g_pts, g_dirs)
    f7d = lambda: ntrain.obj_frame_backward_rays(box, v3, td, ri, si, trk, g_pts, g_dirs)
    tbf, t7c, t7d = [], [], []
    for _ in range(5):
        tbf.append(timed(bwf)); t7c.append(timed(f7c)); t7d.append(timed(f7d))
    print(f"  nlr_obj_train_backward_frame: {stat(tbf)}\n"
          f"  nlr_obj_frame_backward, dense list K = {n * S}: {stat(t7c)}\n"
          f"  nlr_obj_frame_backward_rays, dense list K = {n * S}: {stat(t7d)}", flush=True)
