#!/usr/bin/env python3
"""Forward + backward of the ray-history losses (anti-aliased interlevel + distortion) on the HIP operator (nlr_ray_losses_forward /
_backward through `losses.ray_history_terms`) against the torch form on the same device, and the fused training step with either.

    python scripts/ray_losses_bench.py [--out profiles/ray_losses_bench.txt] [--no-step]

Shapes: REF 65 536 rays x (64, 64 | 32) and C2 16 384 rays x (64, 64 | 128) samples (proposal levels | final level), each with and
without an `obj_mask` on 10 % of the proposal samples.  Per call, device events around `--iters` calls (autograd wrapper and launches
included), the two backends alternating over `--repeats` windows after a warm-up of both.  The step: `training_step` of the fused REF
model on 65 536 rays with `ray_loss_backend="torch"` and `"hip"`, a host clock around `--steps` steps that end in a synchronise,
alternating.  Information, not a gate."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"REF": (65536, 32, (64, 64)), "C2": (16384, 128, (64, 64))}
PULSE = (0.03, 0.003)


def history(torch, N, S, props, masked, seed=0):
    gen = torch.Generator().manual_seed(seed)
    hist = []
    for li, n in enumerate(list(props) + [S]):
        sd = torch.sort(torch.rand(N, n + 1, generator=gen), -1).values
        sd[:, 0], sd[:, -1] = 0.0, 1.0
        w = torch.rand(N, n, generator=gen)
        w = w / w.sum(-1, keepdim=True) * (0.5 + 0.5 * torch.rand(N, 1, generator=gen))
        hist.append(dict(sdist=sd.cuda(), weights=w.cuda().requires_grad_(True)))
        if masked and li < len(props):
            hist[-1]["obj_mask"] = (torch.rand(N, n, generator=gen) < 0.1).cuda()
    return hist


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="training steps per window of the step comparison")
    ap.add_argument("--step-rays", type=int, default=65536)
    ap.add_argument("--no-step", action="store_true", help="skip the training-step comparison")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args(argv)
    sys.path.insert(0, os.path.join(ROOT, "nerf-lidar_amd"))
    import torch
    from nerflidar_hip import losses as nl
    if not torch.cuda.is_available():
        raise RuntimeError("ray_losses_bench needs a GPU: a time taken elsewhere says nothing")
    lines = [f"ray-history losses (0.01 * anti-aliased interlevel + 0.005 * distortion), forward + backward per call, {torch.cuda.get_device_name(0)}",
             f"device events around {a.iters} calls (autograd wrapper and launches included), {a.repeats} alternating windows after warm-up"]

    for name, (N, S, props) in SHAPES.items():
        for masked in (False, True):
            hist = history(torch, N, S, props, masked)

            def step(backend):
                anti, dist = nl.ray_history_terms(hist, PULSE, backend=backend)
                (0.01 * sum(anti) + 0.005 * dist).backward()
                for h in hist:
                    h["weights"].grad = None

            def timed(backend):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.iters):
                    step(backend)
                t1.record()
                torch.cuda.synchronize()
                return t0.elapsed_time(t1) * 1e3 / a.iters  # microseconds per call

            for b in ("hip", "torch"):
                for _ in range(5):
                    step(b)
            torch.cuda.synchronize()
            res = {"hip": [], "torch": []}
            for _ in range(a.repeats):
                for b in res:
                    res[b].append(timed(b))
            lines.append(f"{name} {N} x ({', '.join(map(str, props))} | {S}){', obj_mask 10 %' if masked else ''}")
            for b, v in res.items():
                lines.append(f"  {b:6s} median {statistics.median(v):9.1f} us   min {min(v):9.1f}   max {max(v):9.1f}")
            lines.append(f"  torch / hip (medians): {statistics.median(res['torch']) / statistics.median(res['hip']):.1f}")
            print("\n".join(lines[-4:]), flush=True)
            del hist
            torch.cuda.empty_cache()

    if not a.no_step:
        from nerflidar_hip import config as nconfig, lidar as nlidar, training as ntrain, weights as nweights
        mc = nconfig.workload("REF")
        b = nlidar.synthetic_sweep(width=a.step_rays // 32, seed=0)
        batch = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
        n = batch["origins"].shape[0]
        g = torch.Generator(device="cuda").manual_seed(0)
        batch.update(rgb=torch.rand(n, 3, device="cuda", generator=g), depth=torch.rand(n, device="cuda", generator=g) * 0.5 + 0.05,
                     semantic=torch.randint(0, 19, (n,), device="cuda", generator=g))
        tm = ntrain.TrainableModel(mc, fused_mlp=True).cuda().load_reference(nweights.synth_state_dict(mc, seed=0, trained_like=True))
        opt = torch.optim.Adam(tm.parameters(), lr=1e-3, eps=1e-15)
        for backend in ("torch", "hip"):
            for _ in range(3):
                ntrain.training_step(tm, opt, batch, ray_loss_backend=backend)
        res = {"torch": [], "hip": []}
        for _ in range(a.repeats):
            for backend in res:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    ntrain.training_step(tm, opt, batch, as_tensors=True, ray_loss_backend=backend)
                torch.cuda.synchronize()
                res[backend].append((time.perf_counter() - t0) / a.steps * 1e3)
        lines.append(f"fused training step, REF white-noise field, {n} rays x {mc.level_samples()} samples, {a.steps} steps per window, "
                     f"{a.repeats} alternating windows")
        for backend, v in res.items():
            lines.append(f"  ray_loss_backend={backend:6s} median {statistics.median(v):7.2f} ms per step   min {min(v):7.2f}   max {max(v):7.2f}")
        lines.append(f"  torch - hip (medians): {statistics.median(res['torch']) - statistics.median(res['hip']):.2f} ms per step")
        print("\n".join(lines[-4:]), flush=True)

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
