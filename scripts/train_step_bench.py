"""Time of one whole-model training step (nerflidar_hip.training.training_step: forward with jitter, losses, backward through the
HIP backward kernels, Adam) on a batch of rays, fused NerfMLP against torch Linear modules, and of the NerfMLP stage inside it
(forward + backward + weight gradients of the fused NerfMLP, from events around those calls).
    python scripts/train_step_bench.py [workload=REF] [rays=4096] [--colourless-fraction F] [--masks-only] [--paths torch,fused,wgrad]
--colourless-fraction F: the last round(F * rays) rays carry no colour or semantic supervision (mask_rgb = sem_mask = 0, as
train.py:316-320 sets them for the LiDAR rays of a mixed batch) and the step is told so (training_step(color_rays=..)): they skip
the view MLP.  --masks-only: the same masks, but color_rays is not passed - what such a batch costs without the feature."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("workload", nargs="?", default="REF")
    ap.add_argument("rays", nargs="?", type=int, default=4096)
    ap.add_argument("--colourless-fraction", type=float, default=0.0, help="share of the batch, at its end, without colour supervision")
    ap.add_argument("--masks-only", action="store_true", help="apply the masks of --colourless-fraction but do not pass color_rays")
    ap.add_argument("--paths", default="torch,fused,wgrad", help="comma list of: torch (Linear modules), fused (MFMA fwd+bwd), wgrad (+ nlr_mlp_train_wgrad)")
    ap.add_argument("--steps", type=int, default=10, help="timed steps per repetition")
    ap.add_argument("--reps", type=int, default=1, help="repetitions; the median is reported")
    ap.add_argument("--json", action="store_true", help="also print one JSON line per path")
    return ap


def colourless_batch(batch, colourless):
    """mask_rgb / sem_mask = False on the last `colourless` rays (train.py:316-320); everything else stays supervised."""
    import torch
    n = batch["origins"].shape[0]
    keep = torch.arange(n, device=batch["origins"].device) < n - colourless
    return dict(batch, mask_rgb=keep, sem_mask=keep)


def main(argv=None):
    a = build_parser().parse_args(argv)
    if not 0.0 <= a.colourless_fraction <= 1.0:
        raise SystemExit("--colourless-fraction must lie in [0, 1]")
    sys.path.insert(0, os.path.join(ROOT, "nerf-lidar_amd")); sys.path.insert(0, ROOT)
    import numpy as np, torch
    from nerflidar_hip import config as nconfig, lidar as nlidar, weights as nweights, training as ntrain
    name, rays = a.workload, a.rays
    mc = nconfig.workload(name)
    sd = nweights.synth_state_dict(mc, seed=0, trained_like=True)
    b = nlidar.synthetic_sweep(width=rays // 32, seed=0)
    batch = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    n = batch["origins"].shape[0]
    g = torch.Generator(device="cuda").manual_seed(0)
    batch.update(rgb=torch.rand(n, 3, device="cuda", generator=g), depth=torch.rand(n, device="cuda", generator=g) * 0.5 + 0.05,
                 semantic=torch.randint(0, 19, (n,), device="cuda", generator=g))
    if mc.config.use_intensity:
        batch["intensity"] = torch.rand(n, device="cuda", generator=g)
    colourless = int(round(a.colourless_fraction * n))
    step_kw = {}
    if colourless:
        batch = colourless_batch(batch, colourless)
        if not a.masks_only:
            step_kw["color_rays"] = n - colourless
    print(f"workload {name}: {n} rays x {mc.level_samples()} samples, NerfMLP {mc.nerf_mlp.net_depth_viewdirs} x {mc.nerf_mlp.net_width_viewdirs}, "
          f"{colourless} rays without colour supervision" + (" (masks only)" if colourless and a.masks_only else ""))
    # the NerfMLP stage: events around _FusedMLP.forward and .backward (the backward holds the weight gradients in either form)
    spans = []
    def timed(fn):
        def wrapper(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*args, **kw)
            e1.record()
            spans.append((e0, e1))
            return out
        return staticmethod(wrapper)
    ntrain._FusedMLP.forward = timed(ntrain._FusedMLP.forward)
    ntrain._FusedMLP.backward = timed(ntrain._FusedMLP.backward)
    labels = {"torch": "torch Linear NerfMLP       ", "fused": "fused MFMA NerfMLP fwd+bwd ", "wgrad": "fused MFMA fwd+bwd + wgrad  "}
    for path in a.paths.split(","):
        fused, wgrad = path != "torch", path == "wgrad"
        tm = ntrain.TrainableModel(mc, fused_mlp=fused, fused_wgrad=wgrad).cuda().load_reference(sd)
        opt = torch.optim.Adam(tm.parameters(), lr=1e-3, eps=1e-15)
        # the SAME step on both paths: same weights, deterministic sample positions, no update (lr irrelevant: loss is of the forward).
        # (Round 2 printed the loss after 13 randomized Adam steps drawn from one running RNG stream, i.e. of two different random
        # trajectories: the 3-8 % "gap" at 4 096 rays was jitter noise, 0.1 % at 65 536 rays.  tests/test_training.py pins the step itself
        # on the reference: terms to 2e-4 unfused / 3e-2 fused.)
        from nerflidar_hip import losses as nl
        with torch.no_grad():
            r0, h0 = tm(batch, randomized=False)
            same = float(sum(nl.total_loss(r0, h0, batch).values()))
        torch.manual_seed(0)
        for _ in range(3): ntrain.training_step(tm, opt, batch, **step_kw)
        K = a.steps
        step_ms, stage_ms = [], []
        for _ in range(a.reps):
            spans.clear()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(K): out = ntrain.training_step(tm, opt, batch, as_tensors=True, **step_kw)   # the loop reads the terms once, after the last step
            torch.cuda.synchronize(); step_ms.append((time.perf_counter() - t0) / K * 1e3)
            stage_ms.append(sum(e0.elapsed_time(e1) for e0, e1 in spans) / K if spans else float("nan"))
        dt, stage = float(np.median(step_ms)), float(np.median(stage_ms))
        print(f"  {labels[path]}: {dt:8.2f} ms per step, {n/dt:8.1f} k rays/s, NerfMLP stage {stage:7.2f} ms, loss of the same deterministic step {same:.4f}, "
              f"after {3 + a.reps * K} randomized steps {float(out['loss']):.4f}")
        if a.json:
            print(json.dumps(dict(workload=name, rays=n, colourless=colourless, masks_only=bool(a.masks_only), path=path, step_ms=step_ms,
                                  stage_ms=stage_ms, step_ms_median=dt, stage_ms_median=stage)))
        del tm, opt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
