"""Track refinement, the stage alone and the whole step, at the REF batch: 65 536 rays, 8 synthetic tracks with
T = 20 recorded poses, the samples of the last level that the tracks own.
Stage: the adjoint "cotangents of the box-frame points / directions of the owned samples -> d/d tracks", two forms on the same
tensors in one process:
  (a) plain torch autograd: a differentiable torch restatement of the box parameters (`objects.get_pose` + the constants of
      world2object) followed by the indexing ops of `objects.box_frame`; timed as backward alone (graph kept) and as forward + backward;
  (b) `nlr_obj_frame_backward`.
HIP events around 20 calls after 3 warm-up calls, five repetitions, (a) and (b) alternating; medians.  Both forms are first compared
with the same adjoint in float64 on the CPU; the script stops if the kernel misses the gate of its tests (2e-5 per column).
Step: `training.training_step` of the REF model with the dynamic-object branch, without a TrackNet and with one inside its window.
    python scripts/track_refine_bench.py > profiles/track_refine_bench.txt"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-lidar_amd")); sys.path.insert(0, ROOT)
import numpy as np, torch
from nerflidar_hip import _lib, config as nconfig, lidar as nlidar, objects as nobj, training as ntrain, weights as nweights

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=65536)
ap.add_argument("--tracks", type=int, default=8)
ap.add_argument("--records", type=int, default=20)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--no-step", action="store_true", help="the stage only")
a = ap.parse_args()
dev = "cuda"
print(f"build {_lib.lib().nlr_build_sha().decode()}  device {torch.cuda.get_device_name(0)}", flush=True)


def timed(fn, calls=20, warm=3):
    for _ in range(warm): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls): fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / calls


stat = lambda t: f"min {min(t):.3f}  median {float(np.median(t)):.3f}  max {max(t):.3f} ms"
mc = nconfig.workload("REF", 12)
mc.config.instance_obj, mc.config.latent_size = True, 128
mc.__post_init__()
b = nlidar.synthetic_sweep(width=a.rays // 32, seed=0)
b["timestamp"] = nobj.synthetic_timestamps(b["origins"].shape[0], 0)
tracks_np = nobj.synthetic_tracks(b, n_tracks=a.tracks, n_times=a.records, seed=0)
batch = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
n, S = batch["origins"].shape[0], mc.level_samples()[-1]
n_obj, T = tracks_np.shape[:2]

# ---- the stage alone ----------------------------------------------------------------------------------------------------------
g = torch.Generator(device=dev).manual_seed(0)
td = torch.sort(torch.rand(n, S + 1, device=dev, generator=g) * 0.4 + 0.01, dim=-1)[0].contiguous()
o, d, v = (batch[k].reshape(n, 3).contiguous().float() for k in ("origins", "directions", "viewdirs"))
ts = batch["timestamp"].reshape(-1).contiguous().float()
tracks = torch.from_numpy(tracks_np).to(dev)
L = _lib.lib()
box = torch.empty(n, n_obj, 8, device=dev)
winner = torch.empty(n, S, dtype=torch.int32, device=dev)
_lib.check(L.nlr_track_box_params(_lib.ptr(tracks), _lib.ptr(ts), n, n_obj, T, _lib.ptr(box), _lib.current_stream()))
_lib.check(L.nlr_box_winner(_lib.ptr(td), _lib.ptr(o), _lib.ptr(d), _lib.ptr(box), n, S, n_obj, _lib.ptr(winner), _lib.current_stream()))
sel = (winner >= 0).nonzero()
ri, si = sel[:, 0], sel[:, 1]
tr = winner[ri, si].long()
K = int(ri.shape[0])
ri32, si32, tr32 = ri.int().contiguous(), si.int().contiguous(), tr.int().contiguous()
g_p, g_d = torch.randn(K, 3, device=dev, generator=g), torch.randn(K, 3, device=dev, generator=g)


def torch_box(trk):
    """[N, n_obj, 8] box constants as differentiable torch ops (what nlr_track_box_params computes)."""
    pose = nobj.get_pose(ts[:, None], trk)
    cs, sn = torch.cos(pose[..., 3]), torch.sin(pose[..., 3])
    px = cs * -pose[..., 0] - sn * -pose[..., 1]
    py = sn * px + cs * -pose[..., 1]
    return torch.cat([torch.stack([cs, sn, px, py, -pose[..., 2]], dim=-1), 1.0 / (pose[..., 4:7] / 2.0 + 1e-9)], dim=-1)


def torch_forward():
    trk = tracks.clone().requires_grad_(True)
    p, dd = nobj.box_frame(o, d, v, td, torch_box(trk), ri, si, tr)
    return trk, (p * g_p).sum() + (dd * g_d).sum()


trk_kept, loss_kept = torch_forward()
run_a_bwd = lambda: torch.autograd.grad(loss_kept, trk_kept, retain_graph=True)[0]
run_a_full = lambda: (lambda t_l: torch.autograd.grad(t_l[1], t_l[0])[0])(torch_forward())
run_b = lambda: ntrain.obj_frame_backward(tracks, ts, o, d, v, td, ri32, si32, tr32, g_p, g_d)
ga, gb = run_a_bwd().cpu().double(), run_b().cpu().double()
# both forms against the same adjoint in float64 on the CPU; the kernel is held to the gate of its tests, 2e-5 of the column's largest entry
c64 = lambda x: x.cpu().double() if x.is_floating_point() else x.cpu()
t64 = c64(tracks).requires_grad_(True)
pose = nobj.get_pose(c64(ts)[:, None], t64)
cs64, sn64 = torch.cos(pose[..., 3]), torch.sin(pose[..., 3])
px64 = cs64 * -pose[..., 0] - sn64 * -pose[..., 1]
box64 = torch.cat([torch.stack([cs64, sn64, px64, sn64 * px64 + cs64 * -pose[..., 1], -pose[..., 2]], dim=-1), 1.0 / (pose[..., 4:7] / 2.0 + 1e-9)], dim=-1)
p64, d64 = nobj.box_frame(c64(o), c64(d), c64(v), c64(td), box64, ri.cpu(), si.cpu(), tr.cpu())
want = torch.autograd.grad((p64 * c64(g_p)).sum() + (d64 * c64(g_d)).sum(), t64)[0]
err = lambda x: [float((x[..., c] - want[..., c]).abs().max() / want[..., c].abs().max()) for c in range(7)]
err_a, err_b = err(ga), err(gb)
assert max(err_b) <= 2e-5, f"nlr_obj_frame_backward is off the float64 adjoint: {err_b}"
ta, tf, tb = [], [], []
for _ in range(5):
    ta.append(timed(run_a_bwd)); tf.append(timed(run_a_full)); tb.append(timed(run_b))
per_track = [int((tr == t).sum()) for t in range(n_obj)]
print(f"stage: {n} rays x {S} samples of the last level, {n_obj} tracks x {T} records, K = {K} owned samples (per track {per_track})\n"
      f"  (a) torch autograd, backward alone:     {stat(ta)}\n"
      f"  (a) torch autograd, forward + backward: {stat(tf)}\n"
      f"  (b) nlr_obj_frame_backward:             {stat(tb)}\n"
      f"  (b) median / (a) backward median = {float(np.median(tb)) / float(np.median(ta)):.4f}\n"
      f"  per column 0..6, max |form - float64 CPU adjoint| / max |float64|: (a) " + " ".join(f"{x:.1e}" for x in err_a) + "\n"
      f"                                                                    (b) " + " ".join(f"{x:.1e}" for x in err_b), flush=True)
del trk_kept, loss_kept, ga, gb, want, p64, d64, box64

# ---- the whole step -----------------------------------------------------------------------------------------------------------
if not a.no_step:
    gen = torch.Generator(device=dev).manual_seed(0)
    batch.update(rgb=torch.rand(n, 3, device=dev, generator=gen), depth=torch.rand(n, device=dev, generator=gen) * 0.5 + 0.05,
                 semantic=torch.randint(0, 19, (n,), device=dev, generator=gen))
    classes = (["vehicle.car", "vehicle.truck", "vehicle.bus.rigid"] * n_obj)[:n_obj]
    sd = nweights.synth_state_dict(mc, seed=0, trained_like=True)
    sd.update(nweights.synth_object_state_dict({c: nconfig.obj_mlp_config(c, latent_size=128, log2_hashmap=12) for c in sorted({nobj.query_class(c) for c in classes})},
                                               n_obj, seed=0))
    for label, refine in (("without a TrackNet            ", False), ("TrackNet inside its window    ", True)):
        tm = ntrain.TrainableModel(mc, fused_mlp=True, tracks=tracks_np, class_names=classes, obj_log2_hashmap=12).to(dev).load_reference(sd)
        opt = torch.optim.Adam(tm.parameters(), lr=1e-3, eps=1e-15)
        kw = {}
        if refine:
            tn, tn_opt, lr_fn = ntrain.create_tracknet(tracks_np)
            kw = dict(tracknet=tn.to(dev), tn_optimizer=tn_opt, tn_lr_fn=lr_fn, step=7000)
        torch.manual_seed(0)
        for _ in range(2): ntrain.training_step(tm, opt, batch, **kw)
        ms = []
        for _ in range(5):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.steps): out = ntrain.training_step(tm, opt, batch, as_tensors=True, **kw)
            torch.cuda.synchronize(); ms.append((time.perf_counter() - t0) / a.steps * 1e3)
        extra = f", max |opt_t| after the steps {float(tn.opt_t.detach().abs().max()):.2e}" if refine else ""
        print(f"step, {label}: {stat(ms)} per step{extra}", flush=True)
        del tm, opt
        torch.cuda.empty_cache()
