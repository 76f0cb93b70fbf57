"""Density normals beside the render they follow (profiles/density_normals_bench.txt).

Per workload - C2 (last level 32 768 rays x 128 samples, 40 features) and REFI (32 768 x 32, 40 features), each on seeded white-noise
tables and on the committed trained checkpoint (tests/golden/ckpt_trained_c2 / ckpt_trained, at the hash-map size it was trained
with) - one 32 x 1024 sweep:

  render    `Model.render_rays(want_history=True)` of the model WITHOUT normals
  normals   `normals.density_normals` on that render's last-level tdist and weights (all three outputs), with its workspace size and
            the number of ray chunks the 256 MiB budget gives

Timing: device events around `--steps` back-to-back calls after `--warmup` calls of the same shape, three repeats, minimum and median.
There is no earlier path to compare with: the figures are a measurement, not a gate.
    python scripts/normals_bench.py > profiles/density_normals_bench.txt"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-lidar_amd"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--workloads", default="C2,REFI")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--log2-hashmap", type=int, default=None, help="shrink the white-noise hash tables (rehearsal only)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from nerflidar_hip import _lib, checkpoints as nckpt, config as nconfig, lidar as nlidar, normals as nn_, weights as nweights
    from nerflidar_hip.models import Model
    if not torch.cuda.is_available():
        raise SystemExit("normals_bench measures on the GPU; there is no CPU path")

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ev = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ev.append(e0.elapsed_time(e1) / a.steps)
        return min(ev), float(np.median(ev))

    print(f"density normals beside the render, {torch.cuda.get_device_name(0)}, build {_lib.lib().nlr_build_sha().decode()[:16]}; "
          f"sweep 32 x {a.width}, {a.steps} calls per window after {a.warmup}, {a.repeats} windows: ms per call, min / median")
    batch = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in nlidar.synthetic_sweep(width=a.width, seed=0, scale_factor=1 / 250).items()}
    n = batch["origins"].shape[0]
    for wl in a.workloads.split(","):
        for kind in ("white-noise", "trained"):
            if kind == "trained":
                ck = os.path.join(ROOT, "tests", "golden", "ckpt_trained_c2" if wl == "C2" else "ckpt_trained")
                sd, _ = nckpt.split_state_dict(nckpt.load_checkpoint(ck)[0])
                mc = nckpt.infer_model_config(sd, nconfig.workload(wl, 13))
            else:
                mc = nconfig.workload(wl, a.log2_hashmap)
                sd = nweights.synth_state_dict(mc, seed=0, trained_like=False)
            mc.nerf_mlp.disable_density_normals = False
            model = Model(mc, sd)
            ns, model._normals = model._normals, None                   # the render is timed without the operator
            S, F = mc.level_samples()[-1], mc.nerf_mlp.grid_num_levels * mc.nerf_mlp.grid_level_dim
            r_min, r_med = timed(lambda: model.render_rays(batch, want_history=True))
            _, hist = model.render_rays(batch, want_history=True)
            td, w = hist[-1]["tdist"], hist[-1]["weights"]
            run = lambda: nn_.density_normals(ns.encoder, batch, td, ns.w0, ns.b0, ns.w2, weights=w, std_scale=mc.std_scale, re_weights=ns.re_weights)
            o_min, o_med = timed(run)
            per = nn_.rays_per_chunk(S, F)
            res = dict(workload=wl, tables=kind, rays=n, samples=S, features=F, log2_hashmap=mc.nerf_mlp.grid_log2_hashmap_size,
                       render_ms_min=round(r_min, 3), render_ms_median=round(r_med, 3), normals_ms_min=round(o_min, 3),
                       normals_ms_median=round(o_med, 3), normals_over_render=round(o_min / r_min, 3),
                       workspace_bytes_total=nn_.workspace_bytes(n, S, F), workspace_bytes_allocated=nn_.workspace_bytes(min(per, n), S, F),
                       ray_chunks=-(-n // per))
            print(json.dumps(res))
            del model
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
