#!/usr/bin/env python3
"""Generate tests/golden/fn_smooth.npz and tests/golden/train_step_PATCH.npz: the reference's edge-aware smoothness terms on patch rays
(train.py:365-388; train_utils.py:330-348 edge_aware_loss_v2, :411-433 edge_aware_loss_for_semantic).

Like make_golden.py this runs only where the reference is installed, imports its Python unmodified (through make_golden's stubs) and
writes DATA only.
  * fn_smooth: the two functions called as train.py:381,386 calls them (rgb_patch [P,s,s,3], dep_patch [P,s,s,1], sem_patch [P,s,s,K],
    mask_patch = where(mask > 0, 0, 1) [P,s,s]) on four cases; per case the inputs, torch.nan_to_num of each value and the gradients
    of that with respect to depth and semantic (nan_to_num applied to them as well, as train_utils.clip_gradients does to what they
    reach).
  * train_step_PATCH: make_golden.gen_train_step's step (REF workload, all three heads) with Config.patch_size = 4 and two patches
    leading the batch, as the loader orders it (datasets.py:357-399); train.py:283-453 executed from the reference's file.

Usage:  python tests/golden/make_golden_smooth.py            (from the repo root)
"""
import os
import tempfile
import textwrap

import make_golden as mg  # noqa: E402  (stubs + the reference's modules; generates nothing on import)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

rmodels, REF, rnd = mg.rmodels, mg.REF, mg.rnd


def ref_train_modules():
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
            return rtu, rcfg
        except ModuleNotFoundError as e:
            mg._stub(e.name)
    raise RuntimeError("the reference's train_utils does not import")


def gen_fn_smooth():
    print("smoothness-term fixture")
    rtu, _ = ref_train_modules()
    out = {}
    cases = [(3, 4, 5, "random"), (2, 8, 19, "random"), (1, 2, 1, "all"), (2, 4, 3, "no_x_pair")]
    for ci, (P, s, K, kind) in enumerate(cases):
        n = P * s * s
        depth = rnd(120 + ci, 1, (n,), 0.2, 1.8).requires_grad_(True)
        # class probabilities; a single class would be the constant 1 (both terms' differences vanish), so K = 1 draws values in (0, 1)
        sem = (torch.softmax(rnd(120 + ci, 2, (n, K), -2.0, 2.0), -1) if K > 1 else rnd(120 + ci, 2, (n, K), 0.1, 1.0)).requires_grad_(True)
        rgb = rnd(120 + ci, 3, (n, 3))
        if kind == "random":        # batch['mask'] after train.py:287 is a bool; > 0 = NOT part of the terms
            mask = rnd(120 + ci, 4, (n,)) > 0.7
        elif kind == "all":
            mask = torch.zeros(n, dtype=torch.bool)
        else:                       # every second column masked out: no two x neighbours are both valid, y pairs remain
            mask = (torch.arange(n) % s) % 2 == 1
        shape = [P, s, s]
        mask_patch = torch.where(mask.reshape(*shape) > 0, 0, 1)                                     # train.py:374-375
        rgb_patch, dep_patch, sem_patch = rgb.reshape(*shape, -1), depth.reshape(*shape, -1), sem.reshape(*shape, -1)
        t_d = torch.nan_to_num(rtu.edge_aware_loss_v2(rgb_patch, dep_patch, mask=mask_patch))       # :381,383 without smo_lam
        t_s = torch.nan_to_num(rtu.edge_aware_loss_for_semantic(rgb_patch, sem_patch, mask=mask_patch))  # :386,388 without s_lam
        (t_d + t_s).backward()
        vx = mask_patch[:, :, :-1] * mask_patch[:, :, 1:]
        vy = mask_patch[:, :-1] * mask_patch[:, 1:]
        print(f"   case {ci} (P,s,K)=({P},{s},{K}) {kind}: T_d {float(t_d):.6f} T_s {float(t_s):.6f} x pairs {int(vx.sum())} y pairs {int(vy.sum())}")
        if kind == "no_x_pair":
            assert int(vx.sum()) == 0 and int(vy.sum()) > 0 and float(t_d) == 0 and float(t_s) == 0
        else:
            assert int(vx.sum()) > 0 and int(vy.sum()) > 0 and float(t_d) > 0 and float(t_s) > 0
        out.update({f"c{ci}_shape": np.array([P, s, K]), f"c{ci}_depth": depth, f"c{ci}_semantic": sem, f"c{ci}_rgb": rgb,
                    f"c{ci}_valid": mask_patch.reshape(-1).float(), f"c{ci}_t_d": t_d, f"c{ci}_t_s": t_s,
                    f"c{ci}_grad_depth": depth.grad.nan_to_num(), f"c{ci}_grad_semantic": sem.grad.nan_to_num()})
    mg.save("fn_smooth", n_cases=np.array(len(cases)), **out)


def gen_train_step_patch(patch_size=4, n_patch=2):
    print("training-step fixture with patch rays")
    rtu, rcfg = ref_train_modules()
    from nerflidar_hip import config as nconfig, lidar as nlidar, weights as nweights
    mc = nconfig.workload("REF", 12)
    mc.config.use_intensity = True
    mc.__post_init__()
    seed, width = 3, 12
    sd_np = nweights.synth_state_dict(mc, seed=seed, trained_like=True)
    rmodels.GridEncoder = mg.RefGridEncoderTrain
    try:
        model = mg.build_ref_model(mc, sd_np)
    finally:
        rmodels.GridEncoder = mg.RefGridEncoder
    model.train()
    beams = nlidar.LIDAR_ANGLES[::4]
    batch_np = nlidar.synthetic_sweep(width=width, seed=seed, beams=beams)
    N = batch_np["origins"].shape[0]
    n_rows = n_patch * patch_size ** 2
    assert n_rows < N
    batch = {k: torch.from_numpy(v) for k, v in batch_np.items()}
    patch_mask = torch.zeros(N)
    patch_mask[:n_rows] = 1                                  # patches lead the batch (datasets.py:357-399)
    lidar_mask = (rnd(97, 6, (N,)) > 0.5).float()
    lidar_mask[:n_rows] = 0                                  # LiDAR rays are appended last
    mask = (rnd(97, 5, (N,)) > 0.7).float()
    mask[:n_rows] = (rnd(97, 7, (n_rows,)) > 0.3).float()    # most patch pixels take part (the ORIGINAL mask non-zero, train.py:287,375)
    sup = dict(rgb=rnd(97, 1, (N, 3)), depth=rnd(97, 2, (N,), 0.2, 1.8), intensity=rnd(97, 3, (N,), 0.0, 1.0),
               semantic=(rnd(97, 4, (N,)) * 19).floor().clamp(0, 18), mask=mask, patch_mask=patch_mask, lidar_mask=lidar_mask)
    sup["semantic"][::7] = 255
    sup["depth"][1::9] = 0.0
    batch.update({k: v.clone() for k, v in sup.items()})
    config = rcfg.Config()
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "depth"))
    open(os.path.join(tmp, "depth", "x"), "w").write("1")
    config.data_dir, config.dataset_loader, config.patch_size = tmp, "nusc", patch_size
    config.lidar_supervision, config.only_lidar_supervison, config.pose_refine = True, False, False
    config.use_semantic, config.use_intensity, config.instance_obj, config.latent_size = True, True, False, 0
    config.hash_decay_mults, config.symmetrize = 0.0, False
    train_frac, step = 0.37, 5
    renderings, ray_history = model(False, batch, train_frac=train_frac, compute_extras=True, sample_n=7, sample_m=3, zero_glo=False,
                                    step=step, max_step=25000, curr_track=None)
    src = open(os.path.join(REF, "train.py")).read().split("\n")
    first = next(i for i, l in enumerate(src) if l.strip() == "losses = {}")
    last = next(i for i, l in enumerate(src) if l.strip() == "loss = sum(losses.values())")
    block = textwrap.dedent("\n".join(src[first:last + 1]))
    ns = dict(torch=torch, nn=nn, os=os, train_utils=rtu, config=config, batch=batch, renderings=renderings, ray_history=ray_history,
              model=model, module=model, step=step, start_step=config.start_step, end_step=config.end_step, latent_vector_dict={})
    exec(compile(block, "train.py[%d:%d]" % (first + 1, last + 1), "exec"), ns)
    losses, loss = ns["losses"], ns["loss"]
    assert int(ns["num_patch"]) == n_patch and float(losses["d_smo"]) > 0 and float(losses["s_smo"]) > 0, (ns["num_patch"], losses)
    assert not bool(batch["mask_rgb"][:n_rows].any())
    loss.backward()
    for p_ in model.parameters():            # train_utils.clip_gradients' unconditional nan_to_num_
        if p_.grad is not None:
            p_.grad.nan_to_num_()
    out = dict(workload=np.array("REF"), log2_hashmap=np.array(12), seed=np.array(seed), width=np.array(width), beams=np.array(beams),
               train_frac=np.float32(train_frac), loss=loss.detach(), train_py_lines=np.array([first + 1, last + 1]),
               patch_size=np.array(patch_size), n_patch=np.array(n_patch),
               anti_mult=np.float32(config.anti_interlevel_loss_mult), inter_mult=np.float32(config.interlevel_loss_mult),
               dist_mult=np.float32(config.distortion_loss_mult), pulse_width=np.asarray(config.pulse_width, np.float32),
               data_loss_type=np.array(config.data_loss_type), charb_padding=np.float32(config.charb_padding),
               data_coarse_mult=np.float32(config.data_coarse_loss_mult), data_mult=np.float32(config.data_loss_mult),
               mask_rgb=batch["mask_rgb"])
    for k, v in losses.items():
        out["loss_" + k] = v.detach()
    for k, v in sup.items():
        out["sup_" + k] = v
    out["out_depth"], out["out_rgb"] = renderings[-1]["depth"].detach(), renderings[-1]["rgb"].detach()
    named = dict(model.named_parameters())
    for k in ("nerf_mlp.density_layer.0.weight", "nerf_mlp.density_layer.2.bias", "nerf_mlp.lin_second_stage_0.weight",
              "nerf_mlp.lin_second_stage_1.weight", "nerf_mlp.rgb_layer.weight", "nerf_mlp.sem_layer.2.weight",
              "nerf_mlp.intensity_layer.0.weight", "nerf_mlp.encoder.embeddings", "prop_mlp_0.density_layer.0.weight",
              "prop_mlp_0.encoder.embeddings", "prop_mlp_1.density_layer.2.weight", "prop_mlp_1.encoder.embeddings"):
        g = named[k].grad
        assert g is not None and float(g.abs().sum()) > 0, k
        out["grad_" + k] = g
    print("   loss terms:", {k: float(v.detach()) for k, v in losses.items()}, "total", float(loss.detach()))
    mg.save("train_step_PATCH", **out)
    assert os.path.getsize(os.path.join(mg.HERE, "train_step_PATCH.npz")) <= 1000 * 1000


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    gen_fn_smooth()
    gen_train_step_patch()
