#!/usr/bin/env python
"""Accuracy of the render against the CPU oracle on two scenes, for comparing two builds of the library (profiles/mlp_fold_accuracy.txt):
the white-noise C2 model with small (2^14-row) tables and the committed trained checkpoint tests/golden/ckpt_trained_c2, 2 048 rays each.

  render  (GPU):  NLR_LIB_PATH=<lib> python scripts/mlp_fold_accuracy.py render OUT.npz     one file per build
  compare (CPU):  python scripts/mlp_fold_accuracy.py compare parent=A.npz fold=B.npz       oracle once per scene, one row per build

The oracle runs in `compare`, so the GPU session only renders."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-lidar_amd"))
sys.path.insert(0, ROOT)
N_RAYS = 2048
KEYS = ("rgb", "semantic", "intensity", "depth", "acc")


def scenes():
    from nerflidar_hip import checkpoints as nckpt, config as nconfig, lidar as nlidar, weights as nweights
    mc = nconfig.workload("C2", 14)
    sd = nweights.synth_state_dict(mc, seed=0, trained_like=True)
    sweep = nlidar.synthetic_sweep(width=1024, seed=0)
    idx = np.linspace(0, sweep["origins"].shape[0] - 1, N_RAYS).astype(np.int64)
    yield "white_noise_c2_log2_14", mc, sd, {k: np.ascontiguousarray(v[idx]) for k, v in sweep.items()}
    ck = os.path.join(ROOT, "tests", "golden", "ckpt_trained_c2")
    summ = json.load(open(os.path.join(ck, "train_summary.json")))["summary"]
    sd_all, _ = nckpt.load_checkpoint(ck)
    sd, _ = nckpt.split_state_dict(sd_all)
    mc = nckpt.infer_model_config(sd, nconfig.workload(summ["workload"], summ["log2_hashmap"]))
    for prefix, cfg in nweights.mlp_names(mc):
        sd[f"{prefix}.encoder.offsets"], sd[f"{prefix}.encoder.grid_sizes"], _ = nweights.grid_layout(cfg)
    sweep = nlidar.synthetic_sweep(width=1024, seed=0, sweep_idx=100)
    yield "trained_c2", mc, sd, {k: np.ascontiguousarray(v[idx]) for k, v in sweep.items()}


def render(out_path):
    import torch
    from nerflidar_hip import _lib
    from nerflidar_hip.models import Model
    out = {}
    for name, mc, sd, batch in scenes():
        model = Model(mc, sd, device="cuda:0", precision=_lib.PREC_FAST)
        r, _ = model.render_rays({k: torch.from_numpy(v).cuda() for k, v in batch.items()}, scale_factor=1 / 250)
        torch.cuda.synchronize()
        for k in KEYS + ("labels",):
            out[f"{name}.{k}"] = r[k].cpu().numpy()
    np.savez(out_path, **out)
    print("wrote", out_path)


def compare(named):
    import torch
    from oracle import nlr_oracle as orc
    runs = [(n.split("=", 1)[0], np.load(n.split("=", 1)[1])) for n in named]
    for name, mc, sd, batch in scenes():
        ref = orc.model_forward(sd, mc, {k: torch.from_numpy(v) for k, v in batch.items()})[0][-1]
        ref = {k: ref[k].numpy() for k in KEYS}
        lab = ref["semantic"].argmax(-1)
        top2 = np.sort(ref["semantic"], -1)
        margin = top2[:, -1] - top2[:, -2]
        for tag, z in runs:
            cols = []
            for k in KEYS:
                d = np.abs(z[f"{name}.{k}"].astype(np.float64) - ref[k])
                cols.append(f"{k} max {d.max():.3e} mean {d.mean():.3e}")
            bad = np.nonzero(z[f"{name}.labels"] != lab)[0]
            cols.append(f"labels != oracle: {len(bad)}" + (f" (rays {bad.tolist()}, oracle top-2 margins {margin[bad].tolist()})" if len(bad) else ""))
            print(f"{name:24s} {tag:8s} vs oracle: " + "; ".join(cols))
        if len(runs) == 2:
            (ta, a), (tb, b) = runs
            cols = []
            for k in KEYS:
                d = np.abs(a[f"{name}.{k}"].astype(np.float64) - b[f"{name}.{k}"])
                cols.append(f"{k} max {d.max():.3e}" + (" (same bits)" if np.array_equal(a[f"{name}.{k}"], b[f"{name}.{k}"]) else ""))
            bad = np.nonzero(a[f"{name}.labels"] != b[f"{name}.labels"])[0]
            cols.append(f"labels differ on {len(bad)} rays" + (f": {bad.tolist()}, margins {margin[bad].tolist()}" if len(bad) else ""))
            print(f"{name:24s} {ta} vs {tb}: " + "; ".join(cols))


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "render":
        render(sys.argv[2])
    elif len(sys.argv) >= 3 and sys.argv[1] == "compare":
        compare(sys.argv[2:])
    else:
        sys.exit(__doc__)
