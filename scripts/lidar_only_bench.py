"""LiDAR-only render against the full render (profiles/lidar_only_bench.txt).

Per workload - bench.py's C2 and REF (seeded white-noise tables, one 32 x 1024 sweep per step, moving origin) and the C2 architecture on
the committed trained checkpoint with its hash maps inflated to 2^21 rows (bench.py's `trained_scene` leg) - three figures, ms per sweep:

  (a) the full `render_rays`
  (b) `render_rays(lidar_only=True)`, with its kernel table from the library's HIP-event scopes (an untimed pass of its own)
  (c) the last level alone without colour through the stage entry points: `nlr_mlp_level(rgb = NULL, semantic, intensity)` +
      `nlr_composite_level(rgb = NULL)` on the sample distances the full render produced

(a) and (c) need nothing this mode added, so they also run on a build of an older commit: `--tree DIR` imports package and library from
another checkout (built there), and the script then skips (b).  Run it once per tree in the same session on the same device; the
profile quotes (a) and (c) from the parent commit's build and (b) from the build under test.

Timing: device events around `--steps` back-to-back sweeps after `--warmup` sweeps of the same shape, three repeats, minimum and median
reported; the host clock around the same window (ending in a synchronise) is printed beside it.  Rates use `flops.lidar_flops_per_ray`
for (b): executed work only."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--tree", default=ROOT, help="checkout whose nerf-lidar_amd/nerflidar_hip (package + built library) is measured")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--workloads", default="C2,REF,C2_trained")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--log2-hashmap", type=int, default=None, help="shrink the hash tables (rehearsal only)")
    ap.add_argument("--out", default=None, help="append the JSON result lines to this file")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.tree, "nerf-lidar_amd"))
    import numpy as np
    import torch
    from nerflidar_hip import _lib, checkpoints as nckpt, config as nconfig, flops as nflops, lidar as nlidar, weights as nweights
    from nerflidar_hip.models import Model
    if not torch.cuda.is_available():
        raise SystemExit("lidar_only_bench measures on the GPU; there is no CPU path")
    dev = "cuda:0"
    L = _lib.lib()
    have_lidar = "nlr_render_lidar" in _lib.EXPORTS
    knames = L.nlr_kernel_names().decode().split(",")
    sf = 1.0 / 250.0
    H = len(nlidar.LIDAR_ANGLES)

    def timed(fn):
        """ms per call: (min, median) over the repeats of device-event windows, and the host-clock figure of the last window"""
        for i in range(a.warmup):
            fn(i)
        torch.cuda.synchronize()
        ev, host = [], 0.0
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for i in range(a.steps):
                fn(a.warmup + i)
            e1.record()
            torch.cuda.synchronize()
            host = (time.perf_counter() - t0) / a.steps * 1e3
            ev.append(e0.elapsed_time(e1) / a.steps)
        return {"ms_min": min(ev), "ms_median": float(np.median(ev)), "ms_host_clock": host}

    for wl in a.workloads.split(","):
        if wl == "C2_trained":
            ck = os.path.join(ROOT, "tests", "golden", "ckpt_trained_c2")
            summ = json.load(open(os.path.join(ck, "train_summary.json")))["summary"]
            sd_all, _ = nckpt.load_checkpoint(ck)
            sd, _ = nckpt.split_state_dict(sd_all)
            mc = nckpt.infer_model_config(sd, nconfig.workload(summ["workload"], summ["log2_hashmap"]))
            for prefix, cfg_ in nweights.mlp_names(mc):
                sd[f"{prefix}.encoder.offsets"], sd[f"{prefix}.encoder.grid_sizes"], _ = nweights.grid_layout(cfg_)
            sd, mc = nweights.inflate_hashmaps(sd, mc, a.log2_hashmap or 21)
            first = 100   # sensor positions no training ray used
        else:
            mc = nconfig.workload(wl, a.log2_hashmap)
            sd = nweights.synth_state_dict(mc, seed=0, trained_like=True)
            first = 0
        model = Model(mc, sd, device=dev, precision=_lib.PREC_FAST)
        n_sw = 16
        secs = [nlidar.synthetic_sweep(width=a.width, seed=0, sweep_idx=first + si) for si in range(n_sw)]
        batch = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in secs[0].items()}
        origins = [torch.from_numpy(np.ascontiguousarray(s_["origins"])).to(dev) for s_ in secs]
        n = batch["origins"].shape[0]
        tile = torch.zeros(a.width, H, 7, device=dev)
        S = mc.level_samples()[-1]
        res = {"label": a.label, "workload": wl, "rays": n, "samples_last_level": S, "steps": a.steps, "warmup": a.warmup,
               "repeats": a.repeats, "build_sha": L.nlr_build_sha().decode()[:16]}

        def full(i):
            batch["origins"] = origins[i % n_sw]
            model.render_rays(batch, compute_extras=True, scale_factor=sf, packed=tile)

        res["a_full"] = timed(full)
        res["a_full"]["tflops"] = nflops.flops_per_ray(mc) * n / (res["a_full"]["ms_min"] * 1e-3) / 1e12

        if have_lidar:
            def lidar(i):
                batch["origins"] = origins[i % n_sw]
                model.render_rays(batch, compute_extras=True, scale_factor=sf, packed=tile, lidar_only=True)

            res["b_lidar_only"] = timed(lidar)
            res["b_lidar_only"]["route"] = L.nlr_debug_get(_lib.DBG_LAST_ROUTE)
            res["b_lidar_only"]["tflops_executed"] = nflops.lidar_flops_per_ray(mc) * n / (res["b_lidar_only"]["ms_min"] * 1e-3) / 1e12
            res["b_over_a"] = res["b_lidar_only"]["ms_min"] / res["a_full"]["ms_min"]
            for key, fn in (("kernel_ms_full", full), ("kernel_ms_lidar_only", lidar)):   # untimed passes: every launch bracketed
                ms, cnt = (C.c_float * _lib.NLR_K_COUNT)(), (C.c_uint32 * _lib.NLR_K_COUNT)()
                _lib.check(L.nlr_profile_begin(model._handle))
                for i in range(4):
                    fn(i)
                _lib.check(L.nlr_profile_end(model._handle, _lib.current_stream(), ms, cnt))
                res[key] = {knames[k]: round(ms[k] / 4, 4) for k in range(_lib.NLR_K_COUNT)}

        # (c) the last level alone, without colour, through the stage entry points
        batch["origins"] = origins[0]
        _, hist = model.render_rays(batch, compute_extras=True, scale_factor=sf, want_history=True)
        tdist = hist[-1]["tdist"].contiguous()
        del hist
        K = mc.nerf_mlp.class_num if mc.config.use_semantic else 0
        rays = _lib.NlrRays()
        keep = [batch[k].reshape(n, -1).contiguous().float() for k in ("origins", "directions", "viewdirs", "radii", "near", "far", "base_x", "base_y")]
        for k, t in zip(("origins", "directions", "viewdirs", "radii", "near", "far", "base_x", "base_y"), keep):
            setattr(rays, k, t.data_ptr())
        new = lambda *s, dtype=torch.float32: torch.empty(*s, device=dev, dtype=dtype)
        density, sem, inten = new(n, S), (new(K, n, S) if K else None), (new(n, S) if mc.config.use_intensity else None)
        o = {"depth": new(n), "acc": new(n), "distance_mean": new(n), "distance_median": new(n), "distance_percentile_5": new(n),
             "distance_percentile_95": new(n), "points": new(n, 3)}
        if K:
            o["semantic"], o["labels"] = new(n, K), new(n, dtype=torch.int32)
        if inten is not None:
            o["intensity"] = new(n)
        out = _lib.NlrOut()
        for k, t in o.items():
            setattr(out, k, t.data_ptr())
        out.packed, out.packed_w, out.packed_h = tile.data_ptr(), a.width, H
        ws = torch.empty(L.nlr_workspace_bytes(model._handle, n), dtype=torch.uint8, device=dev)
        lo, hi = mc.bg_intensity_range
        bg = lo if lo == hi else (lo + hi) / 2
        st = _lib.current_stream()

        def last_level(i):
            _lib.check(L.nlr_mlp_level(model._handle, mc.num_levels - 1, C.byref(rays), _lib.ptr(tdist), n, 7, 3, None, None,
                                       _lib.ptr(density), None, _lib.ptr(sem), _lib.ptr(inten), _lib.ptr(ws), ws.numel(), st), "nlr_mlp_level")
            _lib.check(L.nlr_composite_level(_lib.ptr(density), _lib.ptr(tdist), _lib.ptr(keep[1]), None, _lib.ptr(sem), _lib.ptr(inten),
                                             _lib.ptr(keep[5]), _lib.ptr(keep[0]), n, S, K, int(mc.opaque_background), bg, 1, sf, None,
                                             C.byref(out), None, st), "nlr_composite_level")

        res["c_last_level_no_rgb"] = timed(last_level)
        print("LIDAR_ONLY_BENCH " + json.dumps(res), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(res) + "\n")
        del model, ws, tile
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
