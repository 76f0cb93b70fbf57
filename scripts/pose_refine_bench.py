"""Pose refinement, the operator alone and the whole step, on the trained checkpoints (tests/golden/ckpt_trained_c2,
ckpt_trained: C2 and REFI; hash maps as trained) with analytic-scene LiDAR rays.
Operator: features of the last level with ray tensors that require a gradient, forward + backward, two routes on the same tensors in
one process:
  (a) unfused: cast + contraction as torch ops, then `GridEncoder` with its input gradient (`calc_grad_inputs`), erf weights and the
      mean in torch - the route that existed before;
  (b) fused: `encode_features_fused` (`nlr_encode_features_forward`, `_backward_ws`, `nlr_encode_features_backward_rays`), and the ray
      kernel alone.
HIP events around 10 calls after 2 warm-up calls, five repetitions, alternating; medians.  (b)'s ray gradients are printed against (a)'s.
Step: `training.training_step` without a PoseNet and with one inside its window; the difference is the price of pose refinement per step.
    python scripts/pose_refine_bench.py > profiles/pose_refine_bench.txt"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-lidar_amd")); sys.path.insert(0, ROOT)
import numpy as np, torch
from nerflidar_hip import _lib, checkpoints as nckpt, config as nconfig, scene as nscene, training as ntrain

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=16384)
ap.add_argument("--steps", type=int, default=5)
a = ap.parse_args()
dev = torch.device("cuda", 0)
print(f"build {_lib.lib().nlr_build_sha().decode()}  device {torch.cuda.get_device_name(0)}", flush=True)


def timed(fn, calls=10, warm=2):
    for _ in range(warm): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls): fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / calls


stat = lambda t: f"min {min(t):.3f}  median {float(np.median(t)):.3f}  max {max(t):.3f} ms"
KEYS = ntrain.POSE_RAY_KEYS


def torch_cast(b, td, n, m=3, std_scale=0.35):
    """render.py:129-168 + coord.py:51-63 as differentiable torch ops -> means / bound [N,S,n,3], stds / bound [N,S,n]"""
    t0, t1 = td[:, :-1], td[:, 1:]
    j = torch.arange(n, device=td.device)
    t = t0[..., None] + (t1 - t0)[..., None] * (j + 0.5) / n
    deg = 2 * torch.pi * m * j / n
    r = b["radii"].reshape(-1, 1, 1)
    lx, ly = r * t * torch.cos(deg) / 2, r * t * torch.sin(deg) / 2
    o, d, bx, by = (b[k].reshape(-1, 1, 1, 3) for k in KEYS)
    x = o + t[..., None] * d + lx[..., None] * bx + ly[..., None] * by
    std = std_scale * r * t
    m2 = (x * x).sum(-1, keepdim=True).clamp_min(1.1920928955078125e-07)
    inside = m2 <= 1
    z = torch.where(inside, x, ((2 * torch.sqrt(m2) - 1) / m2) * x)
    det = ((1 / m2) * (2 / torch.sqrt(m2) - 1 / m2) ** 2)[..., 0]
    return z / 2, torch.where(inside[..., 0], std, det ** (1 / 3) * std) / 2


for ck_name in ("ckpt_trained_c2", "ckpt_trained"):
    ck = os.path.join(ROOT, "tests", "golden", ck_name)
    summ = json.load(open(os.path.join(ck, "train_summary.json")))["summary"]
    sd, _ = nckpt.load_checkpoint(ck); sd, _ = nckpt.split_state_dict(sd)
    mc = nckpt.infer_model_config(sd, nconfig.workload(summ["workload"], summ["log2_hashmap"]))
    tm = ntrain.TrainableModel(mc, fused_mlp=True).to(dev).load_reference(sd)
    true = nscene.supervise(nscene.random_lidar_rays(a.rays, 0, 1, dev, 0), 0)
    batch, _, _ = nscene.perturb_frames(true, 4, 0)
    n, S = a.rays, mc.level_samples()[-1]
    print(f"\n{summ['workload']} ({ck_name}, maps 2^{summ['log2_hashmap']}), {n} rays x {mc.level_samples()} samples, sample_n = 7", flush=True)

    # ---- the operator alone, last level --------------------------------------------------------------------------------------
    with torch.no_grad():
        _, hist = tm(batch, randomized=False)
    td = hist[-1]["tdist"].contiguous()
    enc = tm.nerf_mlp.encoder
    cot = torch.randn(n, S, enc.output_dim, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    leaves = lambda: dict(batch, **{k: batch[k].detach().clone().requires_grad_(True) for k in KEYS})

    def run_unfused():
        b = leaves()
        means, stds = torch_cast(b, td, 7)
        f = ntrain.encode_features(enc, means, stds, True)
        return torch.autograd.grad((f * cot).sum(), [b[k] for k in KEYS] + [enc.embeddings])

    def run_fused():
        b = leaves()
        f = ntrain.encode_features_fused(enc, b, td, 7, 3, re_weights=True)
        return torch.autograd.grad((f * cot).sum(), [b[k] for k in KEYS] + [enc.embeddings])

    tab = enc.embeddings.detach().contiguous()
    rays_d, keep = _lib.rays(batch, n)
    gd = ntrain._EncodeFeatures._descs(enc, tab)
    outs = [torch.empty(n, 3, device=dev) for _ in range(4)]
    g2 = cot.reshape(n * S, -1).contiguous()

    def run_kernel():
        _lib.check(_lib.lib().nlr_encode_features_backward_rays(C.byref(rays_d), _lib.ptr(td), n, S, 7, 3, 0.35, None, C.byref(gd), 1, _lib.ptr(g2),
                                                                *[_lib.ptr(t) for t in outs], _lib.current_stream()))

    ga, gb = run_unfused(), run_fused()
    for k, x, y in zip(KEYS, ga, gb):
        ok = torch.isfinite(x).all(-1) & torch.isfinite(y).all(-1)     # (rows where either route is not finite are counted, not compared)
        x, y = x[ok], y[ok]
        print(f"  d_{k}: fused against unfused rel {float((x - y).norm() / x.norm()):.2e} cos {float((x * y).sum() / (x.norm() * y.norm())):.6f}"
              f"  ({int((~ok).sum())} rows not finite: unfused {int((~torch.isfinite(ga[KEYS.index(k)]).all(-1)).sum())}, fused {int((~torch.isfinite(gb[KEYS.index(k)]).all(-1)).sum())})")
    ta, tb, tk = [], [], []
    for _ in range(5):
        ta.append(timed(run_unfused)); tb.append(timed(run_fused)); tk.append(timed(run_kernel))
    print(f"  operator, forward + backward to rays and table, last level ({n * S * 7} multisample points):\n"
          f"    (a) unfused (torch cast, GridEncoder with input gradient): {stat(ta)}\n"
          f"    (b) fused (encode_features_fused):                         {stat(tb)}\n"
          f"    nlr_encode_features_backward_rays alone:                   {stat(tk)}\n"
          f"    (b) median / (a) median = {float(np.median(tb)) / float(np.median(ta)):.3f}", flush=True)
    del ga, gb

    # ---- the whole step ------------------------------------------------------------------------------------------------------
    med = {}
    for label, pose in (("without a PoseNet         ", False), ("PoseNet inside its window ", True)):
        tm = ntrain.TrainableModel(mc, fused_mlp=True).to(dev).load_reference(sd)
        opt = torch.optim.Adam(tm.parameters(), lr=1e-4, eps=1e-15)
        kw = {}
        if pose:
            pn, pn_opt, lr_fn = ntrain.create_posenet(4, 0, 0, 10 ** 6, t_ratio=1.0)
            kw = dict(posenet=pn.to(dev), pn_optimizer=pn_opt, pn_lr_fn=lr_fn, step=7000, pose_window=(0, 10 ** 6))
        torch.manual_seed(0)
        for _ in range(2): ntrain.training_step(tm, opt, batch, depth_lam=0.1, sem_lam=0.01, **kw)
        ms = []
        for _ in range(5):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.steps): ntrain.training_step(tm, opt, batch, as_tensors=True, depth_lam=0.1, sem_lam=0.01, **kw)
            torch.cuda.synchronize(); ms.append((time.perf_counter() - t0) / a.steps * 1e3)
        med[pose] = float(np.median(ms))
        print(f"  step, {label}: {stat(ms)} per step", flush=True)
        if pose:  # the ray kernel's share: its three calls of a step (one per level)
            from torch.profiler import profile, ProfilerActivity
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(3): ntrain.training_step(tm, opt, batch, as_tensors=True, depth_lam=0.1, sem_lam=0.01, **kw)
                torch.cuda.synchronize()
            k_ms = sum(e.self_device_time_total for e in prof.key_averages() if "nlr_encode_rays_kernel" in e.key) / 3 / 1e3
            print(f"  pose refinement costs {med[True] - med[False]:+.2f} ms per step; nlr_encode_rays_kernel (3 levels): {k_ms:.2f} ms per step, "
                  f"{100 * k_ms / med[True]:.1f} % of the step", flush=True)
        del tm, opt
        torch.cuda.empty_cache()
