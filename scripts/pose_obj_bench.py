"""Pose refinement with dynamic objects, the stage alone and the whole step, at the REF batch of scripts/track_refine_bench.py: 65 536
rays, 8 synthetic tracks with T = 20 recorded poses, the samples of the last level that the tracks own.
Stage: the adjoint "cotangents of the box-frame points / directions of the owned samples -> d/d origins, directions, viewdirs", two
forms on the same list and cotangents in one process:
  (a) plain torch autograd through `objects.box_frame` (gather / index_put chain), timed as backward alone (graph kept) and as
      forward + backward;
  (b) `nlr_obj_frame_backward_rays`.
HIP events around 20 calls after 3 warm-up calls, five repetitions, (a) and (b) alternating; medians.  Both forms are first compared
with the same adjoint in float64 on the CPU; the script stops if the kernel misses the gate of its tests (2e-5 per output), and if
two runs of it differ in a bit.
Step: `training.training_step` of the REF model with the dynamic-object branch, without a PoseNet and with one inside its window.
--accuracy: run the GPU tests of tests/test_pose_refine_objects.py that compare a step with the reference's and print what they measured.
    python scripts/pose_obj_bench.py > profiles/pose_obj_bench.txt
    python scripts/pose_obj_bench.py --accuracy > profiles/pose_obj_accuracy.txt"""
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
ap.add_argument("--accuracy", action="store_true", help="the step against the reference's fixture instead (fp32 and fused path)")
a = ap.parse_args()
dev = "cuda"
print(f"build {_lib.lib().nlr_build_sha().decode()}  device {torch.cuda.get_device_name(0)}", flush=True)

if a.accuracy:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_pose_refine_objects as t
    t._record = t.ACCURACY_LINES.append   # (the list is printed once, below)
    for name in ("test_pose_refinement_step_with_objects_matches_the_reference_step", "test_pose_refinement_step_with_objects_on_the_fused_path"):
        try:
            getattr(t, name)()
            t.ACCURACY_LINES.append(f"{name}: passed")
        except (AssertionError, KeyError) as e:
            t.ACCURACY_LINES.append(f"{name}: FAILED {type(e).__name__} {str(e)[:300]}")
    print("\n".join(t.ACCURACY_LINES))
    raise SystemExit(0)


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
box = nobj.track_box_params(tracks, ts)
winner = torch.empty(n, S, dtype=torch.int32, device=dev)
_lib.check(_lib.lib().nlr_box_winner(_lib.ptr(td), _lib.ptr(o), _lib.ptr(d), _lib.ptr(box), n, S, n_obj, _lib.ptr(winner), _lib.current_stream()))
sel = (winner >= 0).nonzero()
ri, si = sel[:, 0], sel[:, 1]
tr = winner[ri, si].long()
K = int(ri.shape[0])
ri32, si32, tr32 = ri.int().contiguous(), si.int().contiguous(), tr.int().contiguous()
g_p, g_d = torch.randn(K, 3, device=dev, generator=g), torch.randn(K, 3, device=dev, generator=g)


def torch_forward():
    leaves = [t.clone().requires_grad_(True) for t in (o, d, v)]
    p, dd = nobj.box_frame(*leaves, td, box, ri, si, tr)
    return leaves, (p * g_p).sum() + (dd * g_d).sum()


leaves_kept, loss_kept = torch_forward()
run_a_bwd = lambda: torch.autograd.grad(loss_kept, leaves_kept, retain_graph=True)
run_a_full = lambda: (lambda l_l: torch.autograd.grad(l_l[1], l_l[0]))(torch_forward())
run_b = lambda: ntrain.obj_frame_backward_rays(box, v, td, ri32, si32, tr32, g_p, g_d)
ga, gb, gb2 = [x.cpu().double() for x in run_a_bwd()], [x.cpu().double() for x in run_b()], [x.cpu().double() for x in run_b()]
assert all(torch.equal(x, y) for x, y in zip(gb, gb2)), "two runs of nlr_obj_frame_backward_rays differ"
# both forms against the same adjoint in float64 on the CPU; the kernel is held to the gate of its tests, 2e-5 of the output's largest entry
c64 = lambda x: x.cpu().double() if x.is_floating_point() else x.cpu()
l64 = [c64(t).requires_grad_(True) for t in (o, d, v)]
p64, d64 = nobj.box_frame(*l64, c64(td), c64(box), ri.cpu(), si.cpu(), tr.cpu())
want = torch.autograd.grad((p64 * c64(g_p)).sum() + (d64 * c64(g_d)).sum(), l64)
err = lambda xs: [float((x - w).abs().max() / w.abs().max()) for x, w in zip(xs, want)]
err_a, err_b = err(ga), err(gb)
assert max(err_b) <= 2e-5, f"nlr_obj_frame_backward_rays is off the float64 adjoint: {err_b}"
ta, tf, tb = [], [], []
for _ in range(5):
    ta.append(timed(run_a_bwd)); tf.append(timed(run_a_full)); tb.append(timed(run_b))
owning = int((winner >= 0).any(-1).sum())
print(f"stage: {n} rays x {S} samples of the last level, {n_obj} tracks x {T} records, K = {K} owned samples on {owning} rays\n"
      f"  (a) torch autograd, backward alone:     {stat(ta)}\n"
      f"  (a) torch autograd, forward + backward: {stat(tf)}\n"
      f"  (b) nlr_obj_frame_backward_rays:        {stat(tb)}\n"
      f"  (b) median / (a) backward median = {float(np.median(tb)) / float(np.median(ta)):.4f}\n"
      f"  d_origins, d_directions, d_viewdirs: max |form - float64 CPU adjoint| / max |float64|: (a) " + " ".join(f"{x:.1e}" for x in err_a) + "\n"
      f"                                                                                      (b) " + " ".join(f"{x:.1e}" for x in err_b) + "\n"
      f"  (b) twice: identical bits", flush=True)
del leaves_kept, loss_kept, ga, gb, gb2, want, p64, d64

# ---- the whole step -----------------------------------------------------------------------------------------------------------
if not a.no_step:
    gen = torch.Generator(device=dev).manual_seed(0)
    batch.update(rgb=torch.rand(n, 3, device=dev, generator=gen), depth=torch.rand(n, device=dev, generator=gen) * 0.5 + 0.05,
                 semantic=torch.randint(0, 19, (n,), device=dev, generator=gen), glo_idx=(torch.arange(n, device=dev) % 4).float()[:, None])
    classes = (["vehicle.car", "vehicle.truck", "vehicle.bus.rigid"] * n_obj)[:n_obj]
    sd = nweights.synth_state_dict(mc, seed=0, trained_like=True)
    sd.update(nweights.synth_object_state_dict({c: nconfig.obj_mlp_config(c, latent_size=128, log2_hashmap=12) for c in sorted({nobj.query_class(c) for c in classes})},
                                               n_obj, seed=0))
    for label, refine in (("without a PoseNet            ", False), ("PoseNet inside its window    ", True)):
        tm = ntrain.TrainableModel(mc, fused_mlp=True, tracks=tracks_np, class_names=classes, obj_log2_hashmap=12).to(dev).load_reference(sd)
        opt = torch.optim.Adam(tm.parameters(), lr=1e-3, eps=1e-15)
        kw = {}
        if refine:
            pn, pn_opt, lr_fn = ntrain.create_posenet(4, num_lidars=0)
            kw = dict(posenet=pn.to(dev), pn_optimizer=pn_opt, pn_lr_fn=lr_fn, step=15000)
        torch.manual_seed(0)
        for _ in range(2): ntrain.training_step(tm, opt, batch, **kw)
        ms = []
        for _ in range(5):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.steps): out = ntrain.training_step(tm, opt, batch, as_tensors=True, **kw)
            torch.cuda.synchronize(); ms.append((time.perf_counter() - t0) / a.steps * 1e3)
        extra = f", max |t| after the steps {float(pn.t.detach().abs().max()):.2e}" if refine else ""
        print(f"step, {label}: {stat(ms)} per step{extra}", flush=True)
        del tm, opt
        torch.cuda.empty_cache()
