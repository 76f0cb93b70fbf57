#!/usr/bin/env python3
"""Generate tests/golden/train_step_TRACK.npz: the reference's training step with TRACK REFINEMENT (Config.track_refine,
nuscenes_single.gin:19-20) on the batch of `make_golden.gen_train_step_obj`.

Like make_golden.py this runs only where the reference is installed, imports its Python unmodified (through make_golden's stubs)
and writes DATA only.  What differs from gen_train_step_obj:
  * the grid encoders hand back the gradient of their input positions (oracle grid kernels with dy_dx), which is how the loss
    reaches the box frame and, through world2object and get_pose, the tracks;
  * a `Track_opt` (posenet_v2.py:65-76) with seeded, small, non-zero offsets; the track handed to the model is built by the lines
    train.py:251-256, executed from the reference's file;
  * `model(False, batch, ..., curr_track=track)`, the loss block of train.py executed from the file, `.backward()`.
Stored: the offsets, their gradients, the loss terms, the owner maps of the three levels and the rendered depth.

Usage:  python tests/golden/make_golden_track.py            (from the repo root)
"""
import os
import tempfile
import textwrap

import make_golden as mg  # noqa: E402  (stubs + the reference's modules; generates nothing on import)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

orc, rmodels, REF = mg.orc, mg.rmodels, mg.REF


class _RefGridFnX(torch.autograd.Function):
    """Autograd through the CPU restatement of the grid kernels, position gradient included (gridencoder.cu: dy_dx in the forward,
    kernel_input_backward in the backward), as grid.py:24-89 wires them."""

    position_grads = 0   # backward calls that returned a position gradient

    @staticmethod
    def forward(ctx, x01, emb, enc):
        flat = x01.detach().contiguous().numpy()
        out, dy = orc.grid_encode_c(flat, emb.detach().numpy(), enc.offsets.numpy(), float(np.log2(enc.per_level_scale)), enc.base_resolution,
                                    enc.gridtype_id, enc.align_corners, enc.interp_id, want_dy_dx=bool(ctx.needs_input_grad[0]))
        ctx.enc, ctx.flat, ctx.n, ctx.dy = enc, flat, emb.shape[0], dy
        return torch.from_numpy(out).permute(1, 0, 2).reshape(flat.shape[0], enc.output_dim)

    @staticmethod
    def backward(ctx, g):
        enc = ctx.enc
        gl = g.reshape(g.shape[0], enc.num_levels, enc.level_dim).permute(1, 0, 2).contiguous().numpy()
        gt, gi = orc.grid_backward_c(gl, ctx.flat, enc.offsets.numpy(), ctx.n, enc.level_dim, float(np.log2(enc.per_level_scale)),
                                     enc.base_resolution, ctx.dy, enc.gridtype_id, enc.align_corners, enc.interp_id)
        _RefGridFnX.position_grads += gi is not None
        return (None if gi is None else torch.from_numpy(gi)), torch.from_numpy(gt), None


class RefGridEncoderTrainX(mg.RefGridEncoder):
    def forward(self, inputs, bound=1):
        x01 = (inputs + bound) / (2 * bound)
        prefix = list(x01.shape[:-1])
        return _RefGridFnX.apply(x01.reshape(-1, self.input_dim), self.embeddings, self).view(prefix + [self.output_dim])


TRACK_SEED = 27  # seed of the synthetic tracks: one that meets every condition asserted below

TRACK_SIZE = (0.2, 0.15, 0.15)   # edge lengths of the boxes before their seeded stretch (objects.synthetic_tracks)


def _owner_maps(model, batch, ray_history, track):
    """Per level: index of the LAST track whose box holds the interval midpoint (models.py:415,475), -1 outside every box."""
    from internal import obj_utils as robj
    out = []
    with torch.no_grad():
        pose = robj.get_pose(batch["timestamp"], track)
        for h in ray_history:
            tdist = h["tdist"]
            t_mid = 0.5 * (tdist[..., :-1] + tdist[..., 1:])
            pts_w = t_mid[..., None] * batch["directions"][:, None, :] + batch["origins"][:, None, :]
            _, _, imap = robj.box_pts(pts=pts_w, viewdirs=batch["viewdirs"], obj_pose=pose, sym=False)
            idx = torch.arange(imap.shape[-1])[None, None, :].expand_as(imap)
            out.append(torch.where(imap, idx, torch.full_like(idx, -1)).max(dim=-1)[0].to(torch.int8))
    return out


def gen_train_step_track(scale_t=2e-6, scale_r=2e-5, track_seed=TRACK_SEED, track_size=TRACK_SIZE):
    print("training-step fixture with track refinement")
    for name in ("rawpy", "mediapy", "imageio", "tensorboardX", "plyfile", "trimesh", "nuscenes"):
        if name not in mg.sys.modules:
            try:
                __import__(name)
            except Exception:
                mg._stub(name)
    mg._stub("pycolmap", SceneManager=object)
    for _ in range(20):
        try:
            from internal import train_utils as rtu, configs as rcfg, posenet_v2 as rpose
            break
        except ModuleNotFoundError as e:
            mg._stub(e.name)
    # _build_obj_model(train=True) with two of the names it looks up bound differently for the call: the GridEncoder it gives the
    # reference's MLPs, and the seed of the tracks (its own seed leaves track 0 without a sample on the last level)
    from nerflidar_hip import objects as nobj
    keep, keep_tracks = mg.RefGridEncoderTrain, nobj.synthetic_tracks
    mg.RefGridEncoderTrain = RefGridEncoderTrainX
    nobj.synthetic_tracks = lambda b, n_tracks, n_times, seed: keep_tracks(b, n_tracks=n_tracks, n_times=n_times, seed=track_seed, size=track_size)
    try:
        model, batch, batch_np, tracks, cids, lg, seed, width, beams = mg._build_obj_model(train=True)
    finally:
        mg.RefGridEncoderTrain, nobj.synthetic_tracks = keep, keep_tracks
    N = batch_np["origins"].shape[0]
    rnd = mg.rnd
    sup = dict(rgb=rnd(90, 1, (N, 3)), depth=rnd(90, 2, (N,), 0.05, 0.4), semantic=(rnd(90, 4, (N,)) * 19).floor().clamp(0, 18),
               mask=(rnd(90, 5, (N,)) > 0.7).float(), patch_mask=torch.zeros(N), lidar_mask=(rnd(90, 6, (N,)) > 0.5).float())
    sup["semantic"][::7] = 255
    sup["depth"][1::9] = 0.0
    batch.update({k: v.clone() for k, v in sup.items()})
    config = rcfg.Config()
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "depth"))
    open(os.path.join(tmp, "depth", "x"), "w").write("1")
    config.data_dir, config.dataset_loader, config.patch_size = tmp, "nusc", 1
    config.lidar_supervision, config.only_lidar_supervison, config.pose_refine = True, False, False
    config.use_semantic, config.use_intensity, config.instance_obj, config.latent_size = True, False, True, 128
    config.hash_decay_mults, config.symmetrize = 0.0, False
    train_frac, step = 0.61, 5009
    # Track_opt with seeded offsets, then the track of train.py:251-256 from the reference's file
    tracknet_module = rpose.Track_opt(bboxes=model.tracks)
    n_obj, T = model.tracks.shape[:2]
    with torch.no_grad():
        tracknet_module.opt_t.copy_(rnd(91, 1, (n_obj, T, 3), -scale_t, scale_t))
        tracknet_module.opt_r.copy_(rnd(91, 2, (n_obj, T, 1), -scale_r, scale_r))
    src = open(os.path.join(REF, "train.py")).read().split("\n")
    t0 = next(i for i, l in enumerate(src) if l.strip() == "refine_r = tracknet_module.opt_r.to(module.tracks.device)")
    t1 = next(i for i, l in enumerate(src) if i > t0 and l.strip() == "track[:,:,3:4] = raw_track[:,:,3:4] + refine_r")
    assert t1 - t0 == 5, (t0, t1)
    track_code = compile(textwrap.dedent("\n".join(src[t0:t1 + 1])), "train.py[%d:%d]" % (t0 + 1, t1 + 1), "exec")

    def build_track():
        ns_t = dict(torch=torch, tracknet_module=tracknet_module, module=model)
        exec(track_code, ns_t)
        return ns_t["track"]

    track = build_track()
    assert track.requires_grad
    # the unperturbed tracks' owner maps: the offsets must not move a sample across a box face
    with torch.no_grad():
        _, hist0 = model(False, batch, train_frac=train_frac, compute_extras=True, sample_n=7, sample_m=3, zero_glo=False, step=step,
                         max_step=25000, curr_track=None)
    own0 = _owner_maps(model, batch, hist0, model.tracks)
    first = next(i for i, l in enumerate(src) if l.strip() == "losses = {}")
    last = next(i for i, l in enumerate(src) if l.strip() == "loss = sum(losses.values())")
    block = textwrap.dedent("\n".join(src[first:last + 1]))

    def run_step(curr_track):
        """model(...) + the loss block of train.py + backward -> (renderings, ray_history, losses, loss); gradients start from zero"""
        for p_ in list(model.parameters()) + list(tracknet_module.parameters()):
            p_.grad = None
        rend_, hist_ = model(False, batch, train_frac=train_frac, compute_extras=True, sample_n=7, sample_m=3, zero_glo=False, step=step,
                             max_step=25000, curr_track=curr_track)
        ns = dict(torch=torch, nn=nn, os=os, train_utils=rtu, config=config, batch=batch, renderings=rend_, ray_history=hist_, model=model,
                  module=model, step=step, start_step=config.start_step, end_step=config.end_step, latent_vector_dict=model.latent_vector_dict)
        exec(compile(block, "train.py[%d:%d]" % (first + 1, last + 1), "exec"), ns)
        ns["loss"].backward()
        for p_ in list(model.parameters()) + list(tracknet_module.parameters()):
            if p_.grad is not None:
                p_.grad.nan_to_num_()
        return rend_, hist_, ns["losses"], ns["loss"]

    # Conditioning, measured on the reference alone: the same step with the refined track's pose columns moved by one or two units in
    # the last place of float32 (what a different cos / sin or multiply-add order does to them).  A fixture is kept only if that moves
    # the reference's own depth and track gradients by at most a third of the gates they are compared under (2e-4; 5e-3 of the norm):
    # the HIP path differs from the reference's CPU arithmetic in a few such places at once (cos / sin, sample positions, grid).
    ulp = torch.ones_like(track)
    ulp[:, :, :7] = 1.0 + (2.0 * (rnd(92, 1, (n_obj, T, 7)) > 0.5).float() - 1.0) * 2.0 ** -22
    rend_p, _, _, _ = run_step(build_track() * ulp)
    depth_p, g_r_p, g_t_p = rend_p[-1]["depth"].detach().clone(), tracknet_module.opt_r.grad.clone(), tracknet_module.opt_t.grad.clone()
    renderings, ray_history, losses, loss = run_step(track)
    cond = dict(depth=float((renderings[-1]["depth"].detach() - depth_p).abs().max()),
                opt_r=float((tracknet_module.opt_r.grad - g_r_p).norm() / tracknet_module.opt_r.grad.norm()),
                opt_t=float((tracknet_module.opt_t.grad - g_t_p).norm() / tracknet_module.opt_t.grad.norm()))
    print("   moved by an ulp-level change of the track:", cond)
    own = _owner_maps(model, batch, ray_history, track.detach())
    for lvl, (a, b) in enumerate(zip(own0, own)):
        assert torch.equal(a, b), f"the offsets change the owner map of level {lvl}: make them smaller"
        assert torch.equal(b >= 0, ray_history[lvl]["obj_mask"]), lvl
    per_track = [int((own[-1] == t).sum()) for t in range(n_obj)]
    assert all(c > 0 for c in per_track), f"every track must own samples on the last level: {per_track}"
    assert cond["depth"] <= 2e-4 / 3 and cond["opt_r"] <= 5e-3 / 3 and cond["opt_t"] <= 5e-3 / 3, f"ill-conditioned scene: {cond}"
    # the rebinding above took: the object grids are the encoders of this file and they handed back position gradients
    obj_encs = [m_ for n_, m_ in model.named_modules() if n_.startswith("obj_mlp_") and n_.endswith("encoder")]
    assert obj_encs and all(isinstance(m_, RefGridEncoderTrainX) for m_ in obj_encs), [type(m_) for m_ in obj_encs]
    assert _RefGridFnX.position_grads > 0 and np.array_equal(tracks, nobj.synthetic_tracks({k: batch_np[k] for k in ("origins", "directions")}, n_tracks=n_obj, n_times=T, seed=track_seed, size=track_size))
    g_r, g_t = tracknet_module.opt_r.grad, tracknet_module.opt_t.grad
    assert g_r is not None and g_t is not None
    for t in range(n_obj):
        # (float32 normal numbers: the test gates every track's gradient on its own norm, however small beside the others')
        assert float(g_r[t].abs().max()) > 1e-36 and float(g_t[t].abs().max()) > 1e-36, f"track {t} without gradient"
    out = dict(log2_hashmap=np.array(lg), seed=np.array(seed), width=np.array(width), beams=np.array(beams), tracks=tracks,
               class_ids=np.array(cids), timestamp=batch_np["timestamp"], train_frac=np.float32(train_frac), loss=loss.detach(),
               train_py_lines=np.array([first + 1, last + 1]), track_py_lines=np.array([t0 + 1, t1 + 1]),
               latent_reg=np.float32(config.latent_reg), mask_rgb=batch["mask_rgb"], opt_r=tracknet_module.opt_r.detach(),
               opt_t=tracknet_module.opt_t.detach(), grad_opt_r=g_r, grad_opt_t=g_t, owned_per_track=np.array(per_track),
               ulp_moves_depth=np.float32(cond["depth"]), ulp_moves_grad_opt_r=np.float32(cond["opt_r"]),
               ulp_moves_grad_opt_t=np.float32(cond["opt_t"]))
    for k, v in losses.items():
        out["loss_" + k] = v.detach()
    for k, v in sup.items():
        out["sup_" + k] = v
    for lvl, h in enumerate(ray_history):
        out[f"hist{lvl}_obj_mask"] = h["obj_mask"]
        out[f"hist{lvl}_owner"] = own[lvl]
    out["out_depth"] = renderings[-1]["depth"].detach()
    print("   loss terms:", {k: float(v.detach()) for k, v in losses.items()}, "total", float(loss.detach()))
    print("   owned samples per track on the last level:", per_track, " |grad opt_r| per track:", [float(g_r[t].abs().max()) for t in range(n_obj)],
          " |grad opt_t|:", [float(g_t[t].abs().max()) for t in range(n_obj)])
    mg.save("train_step_TRACK", **out)
    size = os.path.getsize(os.path.join(mg.HERE, "train_step_TRACK.npz"))
    assert size <= 400 * 1000, size


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    gen_train_step_track()
