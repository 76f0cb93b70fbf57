"""Train a model on the analytic scene (`nerflidar_hip.scene`) with LiDAR supervision, the way ZI/train.py trains on nuScenes sweeps,
and leave a checkpoint in the reference's format.

    python -m nerflidar_hip.train_scene --workload REFI --log2-hashmap 13 --steps 3000 --out ckpt_dir

The loop is train.py:180-190,272-459,559-566 without the dataset / accelerate / logging plumbing: per step the learning rate of
`training.create_optimizer` is written into the optimiser, a batch of LiDAR rays is drawn (`scene.random_lidar_rays`, the batch
contract of ZI/lidar_utils.py:8-33) and supervised by ray casting (`scene.supervise`: depth, intensity, semantic, rgb),
`training.training_step` takes the step (forward with jitter through the HIP kernels, the loss dictionary of train.py:326-446, backward
through the HIP backward kernels, Adam), and `checkpoints.save_checkpoint` writes `checkpoint_<step>.ckpt` at the end.  Afterwards the
checkpoint is read back through `checkpoints.model_from_checkpoint` and a held-out sweep is rendered on the fused inference path and
compared with the analytic ground truth (metres, label accuracy), so that a run reports whether the field it leaves is a scene.
With `--patch-size S` a `--patch-fraction` of every batch is pinhole pixel patches (`scene.random_patch_rays`) supervised only by the
smoothness terms of train.py:365-388; the batch is ordered pixel | patch | lidar (`batch_layout`) and the summary reports d_smo, s_smo.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import numpy as np
import torch

from . import checkpoints as nckpt
from . import config as nconfig
from . import lidar as nlidar
from . import scene as nscene
from . import training as ntrain


def evaluate(model, scale_factor: float, sweep_idx: int = 100, width: int = 1024, seed: int = 0):
    """Held-out sweep (a sensor position no training ray starts from) on the fused inference path against the analytic scene."""
    b = nlidar.synthetic_sweep(width=width, seed=seed, scale_factor=scale_factor, sweep_idx=sweep_idx)
    tb = {k: torch.from_numpy(v).to(model.device) for k, v in b.items()}
    gt = nscene.cast(tb["origins"], tb["directions"], nlidar.seeded_rotation(seed), scale_factor)
    r, _ = model.render_rays(tb, scale_factor=scale_factor)
    err_m = (r["depth"] - gt["depth"]).abs() / scale_factor
    out = dict(rays=int(err_m.numel()), depth_err_m_median=float(err_m.median()), depth_err_m_mean=float(err_m.mean()),
               depth_err_m_p90=float(err_m.quantile(0.9)), label_accuracy=float((r["labels"].long() == gt["semantic"]).float().mean()))
    if "intensity" in r:
        out["intensity_mae"] = float((r["intensity"] - gt["intensity"]).abs().mean())
    out["rgb_mae"] = float((r["rgb"] - gt["rgb"]).abs().mean())
    return out


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--workload", default="REFI", help="architecture (nerflidar_hip.config.workload): REF, REFI, C2, ...")
    ap.add_argument("--log2-hashmap", type=int, default=None, help="hash-map size of all three grids (default: the gin value 21)")
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--rays", type=int, default=16384, help="rays per step (Config.batch_size is 65 536, configs.py:29)")
    ap.add_argument("--fused", type=int, default=1, help="1: fused bf16 MFMA NerfMLP forward / backward; 0: torch Linear modules in fp32")
    ap.add_argument("--fused-wgrad", action="store_true",
                    help="weight gradients of the fused NerfMLP from nlr_mlp_train_wgrad (one MFMA kernel) instead of library GEMMs; requires --fused 1")
    ap.add_argument("--fused-ray-losses", action="store_true",
                    help="the anti-aliased interlevel and distortion losses from the HIP operator nlr_ray_losses_forward / _backward "
                         "(total_loss(ray_loss_backend='hip')) instead of torch ops")
    ap.add_argument("--lr-init", type=float, default=0.01)
    ap.add_argument("--lr-final", type=float, default=0.001)
    ap.add_argument("--lr-delay-steps", type=int, default=None, help="default: a fifth of the run (5 000 of 25 000 in configs.py:87)")
    ap.add_argument("--depth-lam", type=float, default=0.1, help="train.py:331-332: 0.1 before Config.end_step, 0.4 after")
    ap.add_argument("--sem-lam", type=float, default=0.01, help="train.py:409-410: 0.01 before Config.end_step, 0.04 after")
    ap.add_argument("--hash-decay", type=float, default=0.1)
    ap.add_argument("--scale-factor", type=float, default=1.0 / 250.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True, help="checkpoint directory")
    ap.add_argument("--log-every", type=int, default=200)
    ap.add_argument("--eval-every", type=int, default=0, help="also render the held-out sweep on the fused inference path every this many steps")
    ap.add_argument("--colourless-fraction", type=float, default=0.0,
                    help="the last round(F * rays) rays of every batch carry no colour or semantic supervision (mask_rgb = sem_mask = 0, as "
                         "train.py:316-320 sets them for LiDAR rays) and skip the view MLP (training_step(color_rays=..)); 0: off")
    ap.add_argument("--patch-size", type=int, default=0,
                    help="Config.patch_size (nuscenes_single.gin:10: 32): a --patch-fraction of every batch is pinhole pixel patches of this size "
                         "(scene.random_patch_rays) whose only supervision is the edge-aware smoothness of the rendered depth and class "
                         "probabilities (train.py:365-388: d_smo, s_smo); 0 or 1: no patches")
    ap.add_argument("--patch-fraction", type=float, default=0.25, help="share of the batch that is patch rays (datasets.py:357-399: a quarter)")
    ap.add_argument("--pose-refine", action="store_true",
                    help="pose refinement (Config.pose_refine, train.py:199-221): the rays of every batch belong to --pose-frames frames whose "
                         "poses carry a seeded error (scene.perturb_frames); a PoseNet learns the correction over the whole run and the "
                         "summary reports the pose error before and after")
    ap.add_argument("--pose-frames", type=int, default=4)
    ap.add_argument("--pn-lr-init", type=float, default=4e-5, help="configs.py:153")
    ap.add_argument("--pn-lr-final", type=float, default=2e-6, help="configs.py:154")
    return ap


def pose_error(posenet, seed: int, frames: int, dev, scale_factor: float, rays: int = 4096) -> float:
    """Hit-point error in metres (scene.hit_point_error_m) of a held-out batch under the PoseNet's current correction."""
    true = nscene.supervise(nscene.random_lidar_rays(rays, seed, 0, dev, seed, scale_factor), seed, scale_factor)
    bad, _, _ = nscene.perturb_frames(true, frames, seed)
    with torch.no_grad():
        return nscene.hit_point_error_m(ntrain.refine_batch(bad, posenet(bad["glo_idx"])), true, scale_factor)


def batch_layout(rays: int, colourless_fraction: float = 0.0, patch_size: int = 0, patch_fraction: float = 0.25):
    """(color_rays, n_patches, colourless) of a batch ordered  pixel | patch | lidar:  the rays with colour supervision, then
    n_patches = floor(patch_fraction * rays / patch_size^2) patches (patch_size > 1), then the colourless LiDAR rays.  The patches open
    the colourless tail, so `color_rays` (None when the whole batch has colour) is the row they start at."""
    from .losses import colourless_count
    colourless = colourless_count(rays, colourless_fraction)
    if not 0.0 <= patch_fraction <= 1.0:
        raise ValueError(f"patch fraction must lie in [0, 1], got {patch_fraction}")
    n_patches = int(patch_fraction * rays) // patch_size ** 2 if patch_size > 1 else 0
    if colourless + n_patches * patch_size ** 2 > rays:
        raise ValueError(f"{n_patches} patches of {patch_size}^2 rays and {colourless} colourless rays do not fit into {rays} rays")
    tail = colourless + n_patches * patch_size ** 2
    return (rays - tail if tail else None), n_patches, colourless


def make_batch(rays: int, seed: int, step: int, dev, scale_factor: float, colourless: int = 0, n_patches: int = 0, patch_size: int = 0):
    """The supervised batch of a step in the order of `batch_layout`; also returns patch_rays = (row0, n_patches) for
    `losses.total_loss`, or None without patches."""
    n_patch_rows = n_patches * patch_size ** 2
    lid = nscene.random_lidar_rays(rays - n_patch_rows, seed, step, dev, seed, scale_factor)
    if not n_patches:
        return nscene.supervise(lid, seed, scale_factor, colourless=colourless), None
    row0 = rays - colourless - n_patch_rows
    pat = nscene.random_patch_rays(n_patches, patch_size, seed, step, dev, seed, scale_factor)
    both = {k: torch.cat([lid[k][:row0], pat[k], lid[k][row0:]], 0) for k in lid}
    return nscene.supervise(both, seed, scale_factor, colourless=colourless + n_patch_rows, patch_rows=(row0, n_patch_rows)), (row0, n_patches)


def main(argv=None) -> int:
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.fused_wgrad and not a.fused:
        ap.error("--fused-wgrad requires --fused 1")
    if not 0.0 <= a.colourless_fraction <= 1.0:
        ap.error("--colourless-fraction must lie in [0, 1]")
    try:
        color_rays, n_patches, colourless = batch_layout(a.rays, a.colourless_fraction, a.patch_size, a.patch_fraction)
    except ValueError as e:
        ap.error(str(e))
    if not torch.cuda.is_available():
        raise RuntimeError("train_scene needs a GPU: the training operators have no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(a.seed)
    mc = nconfig.workload(a.workload, a.log2_hashmap)
    tm = ntrain.TrainableModel(mc, fused_mlp=bool(a.fused), fused_wgrad=a.fused_wgrad).to(dev)
    delay = a.lr_delay_steps if a.lr_delay_steps is not None else max(a.steps // 5, 1)
    opt, lr_fn = ntrain.create_optimizer(tm, a.lr_init, a.lr_final, a.steps, delay)
    pose_kw, posenet = {}, None
    if a.pose_refine:  # the window is the whole run: (0, steps + 1), as nuscenes_single.gin:6-7 starts it at step 0
        window = (0, a.steps + 1)
        posenet, pn_opt, pn_lr_fn = ntrain.create_posenet(a.pose_frames, 0, *window, pn_lr_init=a.pn_lr_init, pn_lr_final=a.pn_lr_final, t_ratio=1.0,
                                                          lr_delay_steps=delay)
        posenet = posenet.to(dev)
        pose_kw = dict(posenet=posenet, pn_optimizer=pn_opt, pn_lr_fn=pn_lr_fn, pose_window=window)
        pose_err_before = pose_error(posenet, a.seed, a.pose_frames, dev, a.scale_factor)
    t0 = time.time()
    log = []
    for step in range(1, a.steps + 1):                                     # train.py:180: steps count from 1
        for g in opt.param_groups:
            g["lr"] = lr_fn(step)                                          # train.py:187-190
        batch, patch_rays = make_batch(a.rays, a.seed, step, dev, a.scale_factor, colourless, n_patches, a.patch_size)
        patch_kw = dict(patch_size=a.patch_size, patch_rays=patch_rays) if patch_rays else {}
        if a.fused_ray_losses:
            patch_kw["ray_loss_backend"] = "hip"
        if posenet is not None:
            batch, _, _ = nscene.perturb_frames(batch, a.pose_frames, a.seed)
        train_frac = float(np.clip((step - 1) / max(a.steps - 1, 1), 0, 1))  # train.py:184
        terms = ntrain.training_step(tm, opt, batch, train_frac=train_frac, randomized=True, hash_decay_mult=a.hash_decay,
                                     depth_lam=a.depth_lam, sem_lam=a.sem_lam, as_tensors=True, color_rays=color_rays, step=step, **pose_kw, **patch_kw)
        if step % a.log_every == 0 or step == 1 or step == a.steps:          # the only host read of the loop
            torch.cuda.synchronize()
            rec = dict(step=step, lr=lr_fn(step), elapsed_s=round(time.time() - t0, 1), **{k: round(float(v), 6) for k, v in terms.items()})
            log.append(rec)
            print(json.dumps(rec), flush=True)
        if a.eval_every and step % a.eval_every == 0 and step < a.steps:
            from .models import Model
            ev = evaluate(Model(mc, tm.reference_state_dict(), device=dev), a.scale_factor, seed=a.seed)
            print(json.dumps(dict(step=step, held_out_sweep=ev)), flush=True)
    torch.cuda.synchronize()
    train_s = time.time() - t0
    path = nckpt.save_checkpoint(a.out, tm.reference_state_dict(), a.steps)
    # the round trip a user of the reference takes: file -> state_dict -> Model (weights packed for the fused kernels)
    model, step, ignored = nckpt.model_from_checkpoint(a.out, base=mc)
    ev = evaluate(model, a.scale_factor, seed=a.seed)
    summary = dict(workload=a.workload, log2_hashmap=a.log2_hashmap, steps=a.steps, rays_per_step=a.rays, fused=bool(a.fused), fused_wgrad=a.fused_wgrad,
                   fused_ray_losses=a.fused_ray_losses, colourless_fraction=a.colourless_fraction, train_seconds=round(train_s, 1), train_rays_per_s=round(a.steps * a.rays / train_s), checkpoint=path,
                   checkpoint_bytes=os.path.getsize(path), restored_step=step, held_out_sweep=ev, final_terms=log[-1])
    if n_patches:  # the final step's smoothness terms (also in final_terms): zero would mean the patches saw no valid pair
        summary.update(patch_size=a.patch_size, patches_per_step=n_patches, d_smo=log[-1].get("d_smo"), s_smo=log[-1].get("s_smo"))
    if posenet is not None:
        nckpt.save_posenet(a.out, posenet, a.steps, pn_opt)
        summary["pose_refine"] = dict(frames=a.pose_frames, hit_point_error_m_before=round(pose_err_before, 4),
                                      hit_point_error_m_after=round(pose_error(posenet, a.seed, a.pose_frames, dev, a.scale_factor), 4))
    print(json.dumps(summary), flush=True)
    with open(os.path.join(a.out, "train_summary.json"), "w") as f:
        json.dump(dict(summary=summary, log=log), f, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
