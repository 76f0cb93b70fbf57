#!/usr/bin/env python3
"""Generate tests/golden/train_step_POSE.npz: the reference's training step with POSE REFINEMENT (Config.pose_refine, configs.py:151;
train.py:199-221,463-466) on the static configuration (instance_obj off).

Like make_golden.py this runs only where the reference is installed, imports its Python unmodified (through make_golden's stubs)
and writes DATA only.  What differs from make_golden.gen_train_step:
  * the grid encoders hand back the gradient of their input positions (make_golden_track.RefGridEncoderTrainX: oracle grid kernels
    with dy_dx), which is how the loss reaches the ray tensors;
  * a `LearnPose` from train_utils.create_posenet with seeded, small, non-zero parameters; the refined batch is built by the lines
    train.py:208-221, executed from the reference's file;
  * the batch mixes camera rays (first) and LiDAR rays, two poses each; both kinds sample inside and outside the unit sphere;
  * `model(False, batch, ...)`, the loss block of train.py executed from the file, `.backward()`.
Stored: the posenet parameters and their gradients, every loss term, the rendered depth, the refined ray tensors and d loss / d each
of them.

Usage:  python tests/golden/make_golden_pose.py            (from the repo root)
"""
import os
import tempfile
import textwrap

import make_golden as mg  # noqa: E402  (stubs + the reference's modules; generates nothing on import)
import make_golden_track as mgt  # noqa: E402  (the grid encoder with position gradients)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

rmodels, REF = mg.rmodels, mg.REF
RAY_GRAD_KEYS = ("origins", "directions", "viewdirs", "base_x", "base_y")
RAY_KEYS = ("origins", "directions", "viewdirs", "radii", "near", "far", "base_x", "base_y")


def pose_batch_np(seed, width, beams, cam_w, cam_h):
    """Camera rays of a cam_w x cam_h image first, then a LiDAR sweep: the order of a nuScenes batch (datasets.py:352-390)."""
    from nerflidar_hip import camera as ncamera, lidar as nlidar
    cam = ncamera.synthetic_camera_batch(width=cam_w, height=cam_h, focal=6.0, seed=seed)
    lid = nlidar.synthetic_sweep(width=width, seed=seed, beams=beams)
    return {k: np.concatenate([cam[k].reshape(cam[k].shape[0], -1), lid[k].reshape(lid[k].shape[0], -1)], 0) for k in RAY_KEYS}, cam["origins"].shape[0]


def gen_train_step_pose(scale_r=2e-3, scale_t=2e-3):
    print("training-step fixture with pose refinement")
    for name in ("rawpy", "mediapy", "imageio", "tensorboardX", "plyfile", "trimesh", "nuscenes"):
        if name not in mg.sys.modules:
            try:
                __import__(name)
            except Exception:
                mg._stub(name)
    mg._stub("pycolmap", SceneManager=object)
    for _ in range(20):
        try:
            from internal import train_utils as rtu, configs as rcfg
            break
        except ModuleNotFoundError as e:
            mg._stub(e.name)
    from nerflidar_hip import config as nconfig, lidar as nlidar, weights as nweights
    lg, seed, width, cam_w, cam_h = 12, 5, 12, 8, 6
    mc = nconfig.workload("REF", lg)
    mc.config.use_intensity = True
    mc.__post_init__()
    sd_np = nweights.synth_state_dict(mc, seed=seed, trained_like=True)
    rmodels.GridEncoder = mgt.RefGridEncoderTrainX
    try:
        model = mg.build_ref_model(mc, sd_np)
    finally:
        rmodels.GridEncoder = mg.RefGridEncoder
    model.train()
    beams = nlidar.LIDAR_ANGLES[::4]
    batch_np, n_cam = pose_batch_np(seed, width, beams, cam_w, cam_h)
    N = batch_np["origins"].shape[0]
    batch = {k: torch.from_numpy(v) for k, v in batch_np.items()}
    rnd = mg.rnd
    lidar_mask = torch.zeros(N)
    lidar_mask[n_cam:] = 1
    sup = dict(rgb=rnd(95, 1, (N, 3)), depth=rnd(95, 2, (N,), 0.2, 1.8), intensity=rnd(95, 3, (N,), 0.0, 1.0),
               semantic=(rnd(95, 4, (N,)) * 19).floor().clamp(0, 18), mask=(rnd(95, 5, (N,)) > 0.7).float(),
               patch_mask=torch.zeros(N), lidar_mask=lidar_mask)
    sup["semantic"][::7] = 255
    sup["depth"][1::9] = 0.0
    batch.update({k: v.clone() for k, v in sup.items()})
    # two camera poses (ids 0, 1) and two LiDAR poses (ids 2, 3), interleaved along the rays of each kind
    num_cams, num_lidars = 2, 2
    glo_idx = torch.cat([torch.arange(n_cam) % num_cams, num_cams + torch.arange(N - n_cam) % num_lidars]).float()[:, None]
    batch["glo_idx"] = glo_idx
    config = rcfg.Config()
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "depth"))
    open(os.path.join(tmp, "depth", "x"), "w").write("1")
    config.data_dir, config.dataset_loader, config.patch_size = tmp, "nusc", 1
    config.lidar_supervision, config.only_lidar_supervison, config.pose_refine = True, False, True
    config.use_semantic, config.use_intensity, config.instance_obj, config.latent_size = True, True, False, 0
    config.hash_decay_mults, config.symmetrize = 0.0, False
    # inside the window (start_step, end_step) and past int(0.6 * end_step), where the depth and semantic terms are live again
    step = 15000
    assert config.start_step < step < config.end_step and step >= int(0.6 * config.end_step)
    train_frac = float(np.clip((step - 1) / (config.max_steps - 1), 0, 1))
    posenet, _, _ = rtu.create_posenet(num_cams, config, num_lidars=num_lidars)
    n_pose = num_cams + num_lidars
    with torch.no_grad():
        posenet.r.copy_(rnd(96, 1, (n_pose, 3), -scale_r, scale_r))
        posenet.t.copy_(rnd(96, 2, (n_pose, 3), -scale_t, scale_t))
    src = open(os.path.join(REF, "train.py")).read().split("\n")
    p0 = next(i for i, l in enumerate(src) if l.strip() == "bpp = batch['origins'].shape[0:1]")
    p1 = next(i for i, l in enumerate(src) if i > p0 and l.strip().startswith("batch['normals'] = (batch['normals']"))
    assert p1 - p0 == 13, (p0, p1)
    exec(compile(textwrap.dedent("\n".join(src[p0:p1 + 1])), "train.py[%d:%d]" % (p0 + 1, p1 + 1), "exec"),
         dict(torch=torch, batch=batch, posenet=posenet))
    for k in RAY_GRAD_KEYS:
        assert batch[k].requires_grad and not torch.equal(batch[k].detach(), torch.from_numpy(batch_np[k])), k
        batch[k].retain_grad()
    renderings, ray_history = model(False, batch, train_frac=train_frac, compute_extras=True, sample_n=7, sample_m=3, zero_glo=False,
                                    step=step, max_step=config.max_steps, curr_track=None)
    first = next(i for i, l in enumerate(src) if l.strip() == "losses = {}")
    last = next(i for i, l in enumerate(src) if l.strip() == "loss = sum(losses.values())")
    block = textwrap.dedent("\n".join(src[first:last + 1]))
    ns = dict(torch=torch, nn=nn, os=os, train_utils=rtu, config=config, batch=batch, renderings=renderings, ray_history=ray_history,
              model=model, module=model, step=step, start_step=config.start_step, end_step=config.end_step, latent_vector_dict={})
    exec(compile(block, "train.py[%d:%d]" % (first + 1, last + 1), "exec"), ns)
    losses, loss = ns["losses"], ns["loss"]
    loss.backward()
    for p_ in list(model.parameters()) + list(posenet.parameters()):
        if p_.grad is not None:
            p_.grad.nan_to_num_()
    assert mgt._RefGridFnX.position_grads > 0
    encs = [m_ for n_, m_ in model.named_modules() if n_.endswith("encoder")]
    assert len(encs) == 3 and all(isinstance(m_, mgt.RefGridEncoderTrainX) for m_ in encs)
    # inside / outside the unit sphere: both kinds of ray put samples on both sides (all levels' samples run through the encoders)
    for name, rows in (("camera", slice(0, n_cam)), ("lidar", slice(n_cam, N))):
        fracs = []
        for h in ray_history:
            td = h["tdist"].detach()
            mid = 0.5 * (td[:, :-1] + td[:, 1:])[..., None] * batch["directions"].detach()[:, None] + batch["origins"].detach()[:, None]
            fracs.append(float((mid.norm(dim=-1) > 1)[rows].float().mean()))
        print(f"   {name} rays: fraction of the samples outside the unit sphere per level: {[round(f, 3) for f in fracs]}")
        assert 0.02 < max(fracs) and min(fracs) < 0.98, (name, fracs)
    out = dict(log2_hashmap=np.array(lg), seed=np.array(seed), width=np.array(width), beams=np.array(beams), cam_w=np.array(cam_w),
               cam_h=np.array(cam_h), n_cam=np.array(n_cam), num_cams=np.array(num_cams), num_lidars=np.array(num_lidars),
               glo_idx=glo_idx, step=np.array(step), start_step=np.array(config.start_step), end_step=np.array(config.end_step),
               t_ratio=np.float32(config.t_ratio), train_frac=np.float32(train_frac), loss=loss.detach(),
               train_py_lines=np.array([first + 1, last + 1]), pose_py_lines=np.array([p0 + 1, p1 + 1]), mask_rgb=batch["mask_rgb"],
               pose_r=posenet.r.detach(), pose_t=posenet.t.detach(), grad_pose_r=posenet.r.grad, grad_pose_t=posenet.t.grad)
    for k in RAY_GRAD_KEYS:
        g = batch[k].grad
        assert g is not None and float(g.abs().sum()) > 0, k
        out["refined_" + k], out["grad_" + k] = batch[k].detach(), g
    for k, v in losses.items():
        out["loss_" + k] = v.detach()
    for k, v in sup.items():
        out["sup_" + k] = v
    out["out_depth"] = renderings[-1]["depth"].detach()
    print("   loss terms:", {k: float(v.detach()) for k, v in losses.items()}, "total", float(loss.detach()))
    print("   |grad r|, |grad t|:", float(posenet.r.grad.norm()), float(posenet.t.grad.norm()),
          {k: float(batch[k].grad.norm()) for k in RAY_GRAD_KEYS})
    mg.save("train_step_POSE", **out)
    size = os.path.getsize(os.path.join(mg.HERE, "train_step_POSE.npz"))
    assert size <= 400 * 1000, size


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    gen_train_step_pose()
