#!/usr/bin/env python3
"""Generate tests/golden/train_step_POSE_OBJ.npz: the reference's training step with POSE REFINEMENT (Config.pose_refine; train.py:199-221)
on the SHIPPED configuration, Config.instance_obj = True (nuscenes_single.gin:13): the loss reaches the ray tensors through the static
levels AND through the box-frame points and view directions of the samples inside the tracks' boxes (world2object, obj_utils.py:116-181,
as models.py:401-446 feeds the ObjMLPs).

Like make_golden.py this runs only where the reference is installed, imports its Python unmodified (through make_golden's stubs)
and writes DATA only.  Built from the pieces of its siblings:
  * the scene of make_golden._build_obj_model / the TRACK fixture (REF workload, log2_hashmap 12, latent codes, no intensity head,
    objects.synthetic_tracks), with two of the names it looks up bound differently for the call: the grid encoder (position gradients,
    make_golden_track.RefGridEncoderTrainX) and the rays (the batch of make_golden_pose.pose_batch_np: camera rays first, then a
    LiDAR sweep, two poses each);
  * a `LearnPose` with seeded, small, non-zero parameters, the refined batch built by the lines train.py:208-221 executed from the
    reference's file, `model(False, batch, ...)`, the loss block of train.py executed from the file, `.backward()`.
The step runs three times: with the pose parameters and the raw rays moved by ulp-level factors (conditioning of the scene, measured
on the reference alone), as it is (the fixture), and with `obj_utils.box_pts` wrapped, in this process, so that the box-frame points and directions are
detached from the rays (`grad_<k>_static`: what a build that ignores the box-frame path would compute).
Stored: what train_step_POSE stores (pose parameters and gradients, refined rays, d loss / d each ray tensor, loss terms, depth,
supervision), what train_step_TRACK stores about ownership (owner maps of the three levels), the tracks, class ids and timestamps.
The seed of the tracks is the first that meets the conditions asserted at the end (tests/test_pose_refine_objects.py re-checks them).

Usage:  python tests/golden/make_golden_pose_obj.py            (from the repo root)
"""
import os
import tempfile
import textwrap
import types

import make_golden as mg  # noqa: E402  (stubs + the reference's modules; generates nothing on import)
import make_golden_track as mgt  # noqa: E402  (the grid encoder with position gradients, the owner maps)
import make_golden_pose as mgp  # noqa: E402  (the mixed camera / LiDAR batch)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

REF = mg.REF
RAY_GRAD_KEYS = mgp.RAY_GRAD_KEYS
GRAD_KEYS = ("pose_r", "pose_t") + RAY_GRAD_KEYS
TRACK_SIZE = (0.2, 0.15, 0.15)
BATCH = dict(seed=5, width=12, cam_w=8, cam_h=6)


def _build(track_seed, track_size):
    """make_golden._build_obj_model(train=True) on the pose batch, with position gradients in every grid encoder."""
    from nerflidar_hip import lidar as nlidar, objects as nobj
    beams = nlidar.LIDAR_ANGLES[::4]
    batch_np, n_cam = mgp.pose_batch_np(BATCH["seed"], BATCH["width"], beams, BATCH["cam_w"], BATCH["cam_h"])
    keep = mg.RefGridEncoderTrain, nobj.synthetic_tracks, mg.nlidar
    mg.RefGridEncoderTrain = mgt.RefGridEncoderTrainX
    nobj.synthetic_tracks = lambda b, n_tracks, n_times, seed: keep[1](b, n_tracks=n_tracks, n_times=n_times, seed=track_seed, size=track_size)
    mg.nlidar = types.SimpleNamespace(LIDAR_ANGLES=nlidar.LIDAR_ANGLES, synthetic_sweep=lambda **kw: {k: v.copy() for k, v in batch_np.items()})
    try:
        model, batch, batch_np2, tracks, cids, lg, seed, _, _ = mg._build_obj_model(train=True)
    finally:
        mg.RefGridEncoderTrain, nobj.synthetic_tracks, mg.nlidar = keep
    encs = [m_ for n_, m_ in model.named_modules() if n_.endswith("encoder")]
    assert len(encs) >= 4 and all(isinstance(m_, mgt.RefGridEncoderTrainX) for m_ in encs), [type(m_) for m_ in encs]
    return model, batch, batch_np2, n_cam, tracks, cids, lg, seed, beams


def gen_train_step_pose_obj(scale_r=2e-3, scale_t=2e-3, seeds=range(64), track_size=TRACK_SIZE):
    print("training-step fixture with pose refinement and dynamic objects")
    for name in ("rawpy", "mediapy", "imageio", "tensorboardX", "plyfile", "trimesh", "nuscenes"):
        if name not in mg.sys.modules:
            try:
                __import__(name)
            except Exception:
                mg._stub(name)
    mg._stub("pycolmap", SceneManager=object)
    for _ in range(20):
        try:
            from internal import train_utils as rtu, configs as rcfg, obj_utils as robj
            break
        except ModuleNotFoundError as e:
            mg._stub(e.name)
    rnd = mg.rnd
    config = rcfg.Config()
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "depth"))
    open(os.path.join(tmp, "depth", "x"), "w").write("1")
    config.data_dir, config.dataset_loader, config.patch_size = tmp, "nusc", 1
    config.lidar_supervision, config.only_lidar_supervison, config.pose_refine = True, False, True
    config.use_semantic, config.use_intensity, config.instance_obj, config.latent_size = True, False, True, 128
    config.hash_decay_mults, config.symmetrize = 0.0, False
    # inside the window (start_step, end_step) and past int(0.6 * end_step), where the depth and semantic terms are live again
    step = 15000
    assert config.start_step < step < config.end_step and step >= int(0.6 * config.end_step)
    train_frac = float(np.clip((step - 1) / (config.max_steps - 1), 0, 1))
    num_cams, num_lidars = 2, 2
    n_pose = num_cams + num_lidars
    src = open(os.path.join(REF, "train.py")).read().split("\n")
    p0 = next(i for i, l in enumerate(src) if l.strip() == "bpp = batch['origins'].shape[0:1]")
    p1 = next(i for i, l in enumerate(src) if i > p0 and l.strip().startswith("batch['normals'] = (batch['normals']"))
    assert p1 - p0 == 13, (p0, p1)
    pose_code = compile(textwrap.dedent("\n".join(src[p0:p1 + 1])), "train.py[%d:%d]" % (p0 + 1, p1 + 1), "exec")
    first = next(i for i, l in enumerate(src) if l.strip() == "losses = {}")
    last = next(i for i, l in enumerate(src) if l.strip() == "loss = sum(losses.values())")
    loss_code = compile(textwrap.dedent("\n".join(src[first:last + 1])), "train.py[%d:%d]" % (first + 1, last + 1), "exec")
    model_kw = dict(train_frac=train_frac, compute_extras=True, sample_n=7, sample_m=3, zero_glo=False, step=step, max_step=config.max_steps,
                    curr_track=None)

    def scene(track_seed):
        model, raw, batch_np, n_cam, tracks, cids, lg, seed, beams = _build(track_seed, track_size)
        N = batch_np["origins"].shape[0]
        lidar_mask = torch.zeros(N)
        lidar_mask[n_cam:] = 1
        sup = dict(rgb=rnd(97, 1, (N, 3)), depth=rnd(97, 2, (N,), 0.05, 0.4), semantic=(rnd(97, 4, (N,)) * 19).floor().clamp(0, 18),
                   mask=(rnd(97, 5, (N,)) > 0.7).float(), patch_mask=torch.zeros(N), lidar_mask=lidar_mask)
        sup["semantic"][::7] = 255
        sup["depth"][1::9] = 0.0
        raw.update({k: v.clone() for k, v in sup.items()})
        # two camera poses (ids 0, 1) and two LiDAR poses (ids 2, 3), interleaved along the rays of each kind
        raw["glo_idx"] = torch.cat([torch.arange(n_cam) % num_cams, num_cams + torch.arange(N - n_cam) % num_lidars]).float()[:, None]
        posenet, _, _ = rtu.create_posenet(num_cams, config, num_lidars=num_lidars)
        with torch.no_grad():
            posenet.r.copy_(rnd(98, 1, (n_pose, 3), -scale_r, scale_r))
            posenet.t.copy_(rnd(98, 2, (n_pose, 3), -scale_t, scale_t))
        return types.SimpleNamespace(model=model, raw=raw, batch_np=batch_np, n_cam=n_cam, N=N, tracks=tracks, cids=cids, lg=lg, seed=seed,
                                     beams=beams, sup=sup, posenet=posenet)

    def refined(sc):
        batch = dict(sc.raw)
        exec(pose_code, dict(torch=torch, batch=batch, posenet=sc.posenet))
        for k in RAY_GRAD_KEYS:
            assert batch[k].requires_grad and not torch.equal(batch[k].detach(), sc.raw[k]), k
            batch[k].retain_grad()
        return batch

    def owned(sc):
        """owner maps of the refined batch (forward only) and the figures of conditions 1 - 3"""
        with torch.no_grad():
            batch = dict(sc.raw)
            exec(pose_code, dict(torch=torch, batch=batch, posenet=sc.posenet))
            _, hist = sc.model(False, batch, **model_kw)
            own = mgt._owner_maps(sc.model, batch, hist, sc.model.tracks)
        for lvl, h in enumerate(hist):
            assert torch.equal(own[lvl] >= 0, h["obj_mask"]), lvl
        rays = (own[-1] >= 0).any(-1)
        per_track = [int((own[-1] == t).sum()) for t in range(sc.tracks.shape[0])]
        return own, per_track, int(rays[:sc.n_cam].sum()), int(rays[sc.n_cam:].sum()), float(rays.float().mean())

    def run_step(sc):
        """refined batch + model(...) + the loss block of train.py + backward -> everything the fixture stores of one step"""
        for p_ in list(sc.model.parameters()) + list(sc.posenet.parameters()):
            p_.grad = None
        batch = refined(sc)
        rend, hist = sc.model(False, batch, **model_kw)
        ns = dict(torch=torch, nn=nn, os=os, train_utils=rtu, config=config, batch=batch, renderings=rend, ray_history=hist, model=sc.model,
                  module=sc.model, step=step, start_step=config.start_step, end_step=config.end_step, latent_vector_dict=sc.model.latent_vector_dict)
        exec(loss_code, ns)
        ns["loss"].backward()
        for p_ in list(sc.model.parameters()) + list(sc.posenet.parameters()):
            if p_.grad is not None:
                p_.grad.nan_to_num_()
        grads = {"pose_r": sc.posenet.r.grad.clone(), "pose_t": sc.posenet.t.grad.clone(), **{k: batch[k].grad.clone() for k in RAY_GRAD_KEYS}}
        return types.SimpleNamespace(batch=batch, rend=rend, hist=hist, losses=ns["losses"], loss=ns["loss"], grads=grads,
                                     depth=rend[-1]["depth"].detach().clone())

    rel = lambda a, b: float((a - b).norm() / a.norm())
    for track_seed in seeds:
        sc = scene(track_seed)
        own, per_track, cam_rays, lidar_rays, frac = owned(sc)
        print(f"   track seed {track_seed}: owned last-level samples per track {per_track}, owning rays: camera {cam_rays}, LiDAR {lidar_rays}, "
              f"fraction {frac:.3f}")
        if not (all(c > 0 for c in per_track) and cam_rays > 0 and lidar_rays > 0 and 0.10 <= frac <= 0.60):
            continue
        # conditioning: the same step with the pose parameters moved by one or two units in the last place of float32 - kept only if
        # that moves the reference's own depth and gradients by at most a third of the gates they are compared under
        # (the parameters are small beside the rays they are added to, so on their own they would leave most ray entries where they
        # are: the raw ray tensors move by the same factors, which is what a different multiply-add order in the batch update does)
        r_keep, t_keep = sc.posenet.r.detach().clone(), sc.posenet.t.detach().clone()
        rays_keep = {k: sc.raw[k] for k in RAY_GRAD_KEYS}
        ulp = lambda stream, shape: 1.0 + (2.0 * (rnd(99, stream, shape) > 0.5).float() - 1.0) * 2.0 ** -22
        with torch.no_grad():
            sc.posenet.r.mul_(ulp(1, (n_pose, 3)))
            sc.posenet.t.mul_(ulp(2, (n_pose, 3)))
        for i, k in enumerate(RAY_GRAD_KEYS):
            sc.raw[k] = rays_keep[k] * ulp(3 + i, tuple(rays_keep[k].shape))
        assert not torch.equal(sc.posenet.r.detach(), r_keep) and not torch.equal(sc.posenet.t.detach(), t_keep)
        moved = run_step(sc)
        with torch.no_grad():
            sc.posenet.r.copy_(r_keep)
            sc.posenet.t.copy_(t_keep)
        sc.raw.update(rays_keep)
        main = run_step(sc)
        cond = dict(depth=float((main.depth - moved.depth).abs().max()), **{"grad_" + k: rel(main.grads[k], moved.grads[k]) for k in GRAD_KEYS})
        print("   moved by an ulp-level change of the pose parameters and the raw rays:", cond)
        # the box-frame path switched off: box_pts' points and directions detached from the rays, in this process only
        box_pts = robj.box_pts
        robj.box_pts = lambda *a, **kw: (lambda o: (o[0].detach(), o[1].detach()) + tuple(o[2:]))(box_pts(*a, **kw))
        try:
            static = run_step(sc)
        finally:
            robj.box_pts = box_pts
        share = {k: rel(main.grads[k], static.grads[k]) for k in GRAD_KEYS}
        print("   share of the box-frame path in each gradient, |g - g_static| / |g|:", share)
        assert torch.equal(main.depth, static.depth) and float((main.loss - static.loss).abs()) == 0.0   # the values do not change
        base_same = {k: float((main.grads[k] - static.grads[k]).abs().max()) / float(main.grads[k].abs().max()) for k in ("base_x", "base_y")}
        print("   base_x / base_y between the two runs (the object branch has no multisamples), max |diff| / max |g|:", base_same)
        assert all(v <= 1e-5 for v in base_same.values()), base_same
        ok = (cond["depth"] <= 2e-4 / 3 and all(cond["grad_" + k] <= 5e-3 / 3 for k in GRAD_KEYS)
              and all(share[k] >= 0.05 for k in ("pose_r", "pose_t", "origins", "directions", "viewdirs")))
        if ok:
            break
        print("   -> conditions 4 / 5 not met, next seed")
    else:
        raise SystemExit("no track seed meets the conditions")
    own_after = mgt._owner_maps(sc.model, main.batch, main.hist, sc.model.tracks)
    for lvl in range(3):
        assert torch.equal(own[lvl], own_after[lvl]) and torch.equal(own[lvl] >= 0, main.hist[lvl]["obj_mask"]), lvl
    assert mgt._RefGridFnX.position_grads > 0
    from nerflidar_hip import objects as nobj
    n_obj, T = sc.tracks.shape[:2]
    assert np.array_equal(sc.tracks, nobj.synthetic_tracks({k: sc.batch_np[k] for k in ("origins", "directions")}, n_tracks=n_obj, n_times=T,
                                                           seed=track_seed, size=track_size))
    out = dict(log2_hashmap=np.array(sc.lg), seed=np.array(sc.seed), batch_seed=np.array(BATCH["seed"]), width=np.array(BATCH["width"]),
               beams=np.array(sc.beams), cam_w=np.array(BATCH["cam_w"]), cam_h=np.array(BATCH["cam_h"]), n_cam=np.array(sc.n_cam),
               num_cams=np.array(num_cams), num_lidars=np.array(num_lidars), glo_idx=sc.raw["glo_idx"], step=np.array(step),
               start_step=np.array(config.start_step), end_step=np.array(config.end_step), t_ratio=np.float32(config.t_ratio),
               train_frac=np.float32(train_frac), loss=main.loss.detach(), train_py_lines=np.array([first + 1, last + 1]),
               pose_py_lines=np.array([p0 + 1, p1 + 1]), mask_rgb=main.batch["mask_rgb"], latent_reg=np.float32(config.latent_reg),
               pose_r=sc.posenet.r.detach(), pose_t=sc.posenet.t.detach(), tracks=sc.tracks, track_seed=np.array(track_seed),
               class_ids=np.array(sc.cids), timestamp=sc.batch_np["timestamp"], owned_per_track=np.array(per_track),
               ulp_moves_depth=np.float32(cond["depth"]))
    for k in GRAD_KEYS:
        assert float(main.grads[k].abs().sum()) > 0, k
        out["grad_" + k], out["grad_" + k + "_static"] = main.grads[k], static.grads[k]
        out["ulp_moves_grad_" + k] = np.float32(cond["grad_" + k])
    for k in RAY_GRAD_KEYS:
        out["refined_" + k] = main.batch[k].detach()
    for k, v in main.losses.items():
        out["loss_" + k] = v.detach()
    for k, v in sc.sup.items():
        out["sup_" + k] = v
    for lvl, h in enumerate(main.hist):
        out[f"hist{lvl}_obj_mask"] = h["obj_mask"]
        out[f"hist{lvl}_owner"] = own[lvl]
    out["out_depth"] = main.depth
    print("   loss terms:", {k: float(v.detach()) for k, v in main.losses.items()}, "total", float(main.loss.detach()))
    print("   gradient norms:", {k: float(v.norm()) for k, v in main.grads.items()})
    mg.save("train_step_POSE_OBJ", **out)
    size = os.path.getsize(os.path.join(mg.HERE, "train_step_POSE_OBJ.npz"))
    assert size <= 400 * 1000, size


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    gen_train_step_pose_obj()
