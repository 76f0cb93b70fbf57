#!/usr/bin/env python
"""Do two builds of the library compute the same BYTES in everything that reads a NerfMLP weight tape (csrc/nlr_tape.h)?
(profiles/mlp_tape_identity.txt)

  run     (GPU):  NLR_LIB_PATH=<lib> python scripts/mlp_tape_identity.py run OUT.npz      once per build, one process each
  compare (CPU):  python scripts/mlp_tape_identity.py compare A.npz B.npz                 one line per case, then ALL IDENTICAL
  create  (GPU):  NLR_LIB_PATH=<lib> python scripts/mlp_tape_identity.py create           5 timings of nlr_model_create + nlr_train_plan_create
                                                                                          for the bench model (C2, 2^19 entries)

A run keeps, per output array, its byte count and the SHA-256 of its bytes.  Random dense weights (every Linear N(0, 1 / fan_in), every
bias non-zero), hash tables of 2^12 entries U(-1, 1), one NerfMLP level of S = 32 samples.
  inference  N = 17 rays (M = 544 samples: two 256-sample tiles and a partial one).  View width 128 / 256 x depth 2 / 3 / 5 x heads none /
             semantic K = 19 / semantic K = 5 / intensity / both at 40 grid features, the no_sem_layer pass-through with and without
             intensity, 32 (padded to 64) and 64 grid features.  Per case: the per-sample outputs of nlr_mlp_level at the three
             precisions; nlr_render_rays and nlr_render_lidar at NLR_PREC_FAST (compositing and LiDAR-only tapes).
  training   nlr_train_pack, then nlr_mlp_train_forward_split / _backward_split / _wgrad_split on M = 544 rows (four 128-row tiles and 32
             rows) with M_color = 0, 288 (no tile boundary) and 544; widths 128 / 256 x heads none / semantic / both, 40 and 64 grid
             features, depth 3.  Outputs are pre-filled, so the columns a launch leaves alone compare too."""
import ctypes as C
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-lidar_amd"))
N, S = 17, 32
HEADS = {"none": dict(use_semantic=False), "sem19": dict(), "sem5": dict(class_num=5), "int": dict(use_semantic=False, use_intensity=True),
         "both": dict(use_intensity=True), "pass": dict(no_sem_layer=True), "pass+int": dict(no_sem_layer=True, use_intensity=True)}
GRID = {32: dict(grid_level_dim=2, grid_disired_resolution=16 * 2 ** 15), 40: dict(), 64: dict(grid_disired_resolution=16 * 2 ** 15)}


def model_config(W, D, heads, F):
    from nerflidar_hip.config import Config, MLPConfig, ModelConfig
    h = dict(HEADS[heads])
    mlp = MLPConfig(net_width_viewdirs=W, net_depth_viewdirs=D, grid_log2_hashmap_size=12, class_num=h.pop("class_num", 19), **GRID[F])
    mc = ModelConfig(num_prop_samples=(), num_nerf_samples=S, num_levels=1, config=Config(**h), nerf_mlp=mlp)
    assert mlp.grid_num_levels * mlp.grid_level_dim == F
    return mc


def dense(sd, seed):
    rng = np.random.default_rng(seed)
    out = dict(sd)
    for k, v in sd.items():
        if not k.startswith("nerf_mlp."):
            continue
        v = np.asarray(v)
        if "encoder" in k:
            out[k] = rng.uniform(-1.0, 1.0, v.shape).astype(v.dtype)
        elif k.endswith(".weight"):
            out[k] = rng.normal(0.0, 1.0 / np.sqrt(v.shape[1]), v.shape).astype(np.float32)
        elif k.endswith(".bias"):
            out[k] = (rng.uniform(0.1, 0.5, v.shape) * rng.choice([-1.0, 1.0], v.shape)).astype(np.float32)
    return out


def inference_cases():
    cases = [(W, D, h, 40) for W in (128, 256) for D in (2, 3, 5) for h in ("none", "sem19", "sem5", "int", "both")]
    cases += [(256, 2, "pass", 40), (128, 3, "pass+int", 40)]
    cases += [(W, D, "both", F) for F in (32, 64) for W, D in ((256, 2), (128, 5))]
    return cases


def run(out_path):
    import torch
    from nerflidar_hip import _lib, lidar as nlidar, weights as nweights
    from nerflidar_hip.models import Model
    from nerflidar_hip.training import _TrainPlan
    dev = torch.device("cuda:0")
    L, out = _lib.lib(), {}

    def keep(case, **arrays):
        for k, t in arrays.items():
            if t is None:
                continue
            b = t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
            out[f"{case} | {k}"] = np.frombuffer(hashlib.sha256(b).digest() + len(b).to_bytes(8, "little"), np.uint8)

    sw = nlidar.synthetic_sweep(width=8, seed=3, beams=nlidar.LIDAR_ANGLES[::4])
    idx = np.linspace(0, sw["origins"].shape[0] - 1, N).astype(np.int64)
    batch = {k: torch.from_numpy(np.ascontiguousarray(v[idx])).to(dev) for k, v in sw.items()}
    rays = _lib.NlrRays()
    for k in ("origins", "directions", "viewdirs", "radii", "near", "far", "base_x", "base_y"):
        setattr(rays, k, batch[k].data_ptr())
    tdist = torch.cumsum(torch.rand(N, S + 1, generator=torch.Generator().manual_seed(1)) * (4.0 / (S + 1)) + 1e-3, 1).to(dev)
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
    for W, D, heads, F in inference_cases():
        mc = model_config(W, D, heads, F)
        sd = dense(nweights.synth_state_dict(mc, seed=2, trained_like=True), W + D)
        K = mc.nerf_mlp.class_num if mc.config.use_semantic else 0
        for prec in (_lib.PREC_F32, _lib.PREC_MIXED, _lib.PREC_FAST):
            case = f"inference W{W} D{D} {heads} F{F} prec{prec}"
            model = Model(mc, sd, device=dev, precision=prec)
            new = lambda *sh: torch.full(sh, float("nan"), device=dev)
            o = dict(density=new(N, S), rgb=new(3, N, S), semantic=new(K, N, S) if K else None,
                     intensity=new(N, S) if mc.config.use_intensity else None)
            _lib.check(L.nlr_mlp_level(model._handle, 0, C.byref(rays), _lib.ptr(tdist), N, 7, 3, None, None, _lib.ptr(o["density"]),
                                       _lib.ptr(o["rgb"]), _lib.ptr(o["semantic"]), _lib.ptr(o["intensity"]), _lib.ptr(ws), ws.numel(), None), case)
            torch.cuda.synchronize()
            keep(case + " mlp_level", **o)
            if prec == _lib.PREC_FAST:
                r, _ = model.render_rays(batch, scale_factor=1 / 250)
                route = L.nlr_debug_get(_lib.DBG_LAST_ROUTE)
                rl, _ = model.render_rays(batch, scale_factor=1 / 250, lidar_only=True)
                torch.cuda.synchronize()
                keep(f"{case} render_rays route{route}", **r)
                keep(f"{case} render_lidar route{L.nlr_debug_get(_lib.DBG_LAST_ROUTE)}", **rl)
            del model

    M = N * S
    for W in (128, 256):
        for heads, F in (("none", 40), ("sem19", 40), ("both", 40), ("both", 64)):
            cfg = model_config(W, 3, heads, F).nerf_mlp
            plan = _TrainPlan(cfg)
            K = cfg.class_num if cfg.use_semantic else 0
            g = torch.Generator().manual_seed(W + F + K)
            rnd = lambda *sh: torch.randn(*sh, generator=g).to(dev)
            params, feats, enc = rnd(plan.n_params) * 0.08, rnd(M, F) * 0.5, torch.rand(N, 32, generator=g).to(dev) * 2 - 1
            gd, gr, gs, gi = rnd(M), rnd(3, M), rnd(K, M) if K else None, rnd(M) if cfg.use_intensity else None
            wws = torch.empty(int(L.nlr_mlp_train_wgrad_workspace_bytes(plan.handle, 0)), dtype=torch.uint8, device=dev)
            for Mc in (0, 288, M):
                case = f"training W{W} {heads} F{F} M_color{Mc}"
                fill = lambda *sh, dtype=torch.float32: torch.full(sh, 0.25, device=dev, dtype=dtype)
                o = dict(density=fill(M), rgb=fill(3, M), sem=fill(K, M) if K else None, inten=fill(M) if cfg.use_intensity else None,
                         acts=fill(M, plan.act_w, dtype=torch.bfloat16), gacts=fill(M, plan.act_w + 64, dtype=torch.bfloat16),
                         d_feat=fill(M, F), d_params=fill(plan.n_params))
                p, st = _lib.ptr, _lib.current_stream()
                _lib.check(L.nlr_train_pack(plan.handle, p(params), st), case)
                _lib.check(L.nlr_mlp_train_forward_split(plan.handle, p(feats), p(enc), M, Mc, S, p(o["density"]), p(o["rgb"]), p(o["sem"]),
                                                         p(o["inten"]), p(o["acts"]), st), case)
                _lib.check(L.nlr_mlp_train_backward_split(plan.handle, M, Mc, S, p(o["density"]), p(o["rgb"]), p(o["sem"]), p(o["acts"]), p(gd), p(gr),
                                                          p(gs), p(gi), p(o["gacts"]), p(o["d_feat"]), st), case)
                _lib.check(L.nlr_mlp_train_wgrad_split(plan.handle, M, Mc, S, p(feats), p(enc), p(o["acts"]), p(o["gacts"]), p(o["d_params"]), p(wws),
                                                       wws.numel(), st), case)
                torch.cuda.synchronize()
                keep(case, **o)
            del plan
    np.savez(out_path, **out)
    print(f"wrote {out_path}: {len(out)} arrays, library {_lib.LIB_PATH}")


def create():
    import torch
    from nerflidar_hip import _lib, config as nconfig, weights as nweights
    from nerflidar_hip.models import Model
    from nerflidar_hip.training import _TrainPlan
    mc = nconfig.workload("C2", 19)
    sd = nweights.synth_state_dict(mc, seed=0, trained_like=True)
    L, spent = _lib.lib(), [0.0]

    def timed(fn):  # the two library calls alone: the tables are uploaded by the Python side before nlr_model_create
        def call(*a):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = fn(*a)
            torch.cuda.synchronize()
            spent[0] += (time.perf_counter() - t0) * 1e3
            return rc
        return call

    L.nlr_model_create, L.nlr_train_plan_create = timed(L.nlr_model_create), timed(L.nlr_train_plan_create)
    times = []
    for i in range(6):  # (the first pass pays the context and the allocator: not reported)
        spent[0] = 0.0
        m, p = Model(mc, sd, device="cuda:0"), _TrainPlan(mc.nerf_mlp)
        times.append(spent[0])
        del m, p
    print(f"create {_lib.LIB_PATH}: nlr_model_create (C2, 3 levels) + nlr_train_plan_create, ms: " + " ".join(f"{t:.1f}" for t in times[1:]))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), "the two runs hold different cases"
    cases, bad = {}, 0
    for k in a.files:
        case, _ = k.split(" | ")
        same, total, nbytes = cases.get(case, (0, 0, 0))
        cases[case] = (same + int(np.array_equal(a[k], b[k])), total + 1, nbytes + int.from_bytes(a[k][32:].tobytes(), "little"))
    for case, (same, total, nbytes) in cases.items():
        bad += same != total
        print(f"{case}: {same} of {total} arrays identical ({nbytes} bytes)")
    print("ALL IDENTICAL" if not bad else f"{bad} CASES DIFFER")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] == "create":
        create()
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
