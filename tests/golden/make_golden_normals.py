#!/usr/bin/env python3
"""Generate tests/golden/normals_fwd.npz: the reference's forward with DENSITY NORMALS (NerfMLP.disable_density_normals = False,
Config.analytic_gradient = True; ZI/models.py:1070-1094, :525-529, render.py:255-261).

Like make_golden.py this runs only where the reference is installed, imports its Python unmodified (through make_golden's stubs)
and writes DATA only.  What it sets up:
  * the grid encoders hand back the gradient of their input positions (make_golden_track.RefGridEncoderTrainX: oracle grid kernels
    with dy_dx, kernel_input_backward), which is what `autograd.grad(raw_density, means)` differentiates through; its autograd
    function is wrapped as once differentiable, because the reference asks with create_graph=True;
  * the reference `Model` from weights.synth_state_dict, instance_obj off, use_intensity on, NerfMLP.grid_disired_resolution = 128
    (L = 4 levels, 16 .. 128: the scale at which a face margin of 1e-4 cell separates float32 from float32), log2_hashmap = 12;
  * the ray mix of make_golden_pose.pose_batch_np: camera rays, then a 12-column sweep, so both branches of the contraction occur;
  * `model(False, batch, train_frac=1, compute_extras=True)` with grad enabled.
Stored: the batch recipe and the seed, the last level's tdist, weights, raw_grad_density and normals, renderings[-1]['normals'] and
['depth'], and the float64 `near` [N, S] mask of tests/test_normals.py (samples where a float32 evaluation may take another branch).

The file is not named fwd_*: the parity tests take every tests/golden/fwd_*.npz for a fixture of make_golden.gen_mlp_and_forward.

Usage:  python tests/golden/make_golden_normals.py            (from the repo root)
"""
import os
import sys

import make_golden as mg  # noqa: E402  (stubs + the reference's modules; generates nothing on import)
import make_golden_track as mgt  # noqa: E402  (the grid encoder with position gradients)
import make_golden_pose as mgp  # noqa: E402  (the ray mix)

import numpy as np  # noqa: E402
import torch  # noqa: E402

rmodels = mg.rmodels


class _RefGridFnOnce(torch.autograd.Function):
    """make_golden_track._RefGridFnX, its two halves called unchanged, marked once differentiable: the reference asks for the density
    gradient with create_graph=True (models.py:1086, for losses on normals), which hands the backward a cotangent that requires grad;
    the restated kernels work on numpy arrays and have no second derivative to offer.  The first derivative - all a forward reads - is
    the same."""
    forward = staticmethod(mgt._RefGridFnX.forward)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return mgt._RefGridFnX.backward(ctx, g)


class RefGridEncoderNormals(mgt.RefGridEncoderTrainX):
    def forward(self, inputs, bound=1):
        x01 = (inputs + bound) / (2 * bound)
        prefix = list(x01.shape[:-1])
        return _RefGridFnOnce.apply(x01.reshape(-1, self.input_dim), self.embeddings, self).view(prefix + [self.output_dim])


def gen_fwd_normals(seed=0, trained_like=True, save=True):
    # seed 0: 71 % of the last level's multisamples lie outside the unit sphere; with seed 5 (the pose fixture's) all of them lie inside
    print("forward fixture with density normals")
    from nerflidar_hip import config as nconfig, lidar as nlidar, weights as nweights
    from nerflidar_hip.gridencoder import GridEncoder
    lg, width, cam_w, cam_h = 12, 12, 8, 6
    mc = nconfig.workload("REF", lg)
    mc.config.use_intensity, mc.config.instance_obj, mc.config.analytic_gradient = True, False, True
    mc.nerf_mlp.disable_density_normals = False
    mc.nerf_mlp.grid_disired_resolution = 128
    mc.__post_init__()
    assert mc.nerf_mlp.grid_num_levels == 4 and mc.prop_mlp.disable_density_normals
    sd_np = nweights.synth_state_dict(mc, seed=seed, trained_like=trained_like)
    rmodels.GridEncoder = RefGridEncoderNormals
    try:
        model = mg.build_ref_model(mc, sd_np)
    finally:
        rmodels.GridEncoder = mg.RefGridEncoder
    assert model.nerf_mlp.disable_density_normals is False and model.nerf_mlp.analytic_gradient is True
    beams = nlidar.LIDAR_ANGLES[::4]
    batch_np, n_cam = mgp.pose_batch_np(seed, width, beams, cam_w, cam_h)
    batch = {k: torch.from_numpy(v) for k, v in batch_np.items()}
    before = mgt._RefGridFnX.position_grads
    with torch.enable_grad():
        renderings, ray_history = model(False, batch, train_frac=1, compute_extras=True)
    assert mgt._RefGridFnX.position_grads > before
    last = ray_history[-1]
    tdist, weights = last["tdist"].detach().float(), last["weights"].detach().float()
    raw_grad, normals = last["raw_grad_density"].detach().float(), last["normals"].detach().float()
    N, S = weights.shape
    assert raw_grad.shape == (N, S, 3) and normals.shape == (N, S, 3) and renderings[-1]["normals"].shape == (N, 3)
    assert all(h.get("normals") is None for h in ray_history[:-1])

    # the float64 `near` mask, by the definition and the code of the tests
    sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
    import test_normals as tn
    enc = GridEncoder.from_mlp_config(mc.nerf_mlp)
    with torch.no_grad():
        enc.embeddings.copy_(torch.from_numpy(np.asarray(sd_np["nerf_mlp.encoder.embeddings"], np.float32)))
    layers = [torch.from_numpy(np.asarray(sd_np["nerf_mlp.density_layer." + k], np.float32)) for k in ("0.weight", "0.bias")] + \
             [torch.from_numpy(np.asarray(sd_np["nerf_mlp.density_layer.2.weight"], np.float32)[0])]
    rays = [batch[k] for k in ("origins", "directions", "base_x", "base_y", "radii")]
    ref = tn._restate(rays, tdist, None, enc.embeddings.detach(), enc, 7, True, layers, torch.float64, weights=weights)
    near = tn._near(ref, enc)
    frac = float(near.float().mean())
    m2 = (ref["means"] ** 2).sum(-1)
    print(f"   N = {N}, S = {S}; near: {100 * frac:.2f} % of the samples; multisamples outside the unit sphere: {100 * float((m2 > 1).float().mean()):.1f} %")
    if not save:
        return
    assert frac <= 0.10, frac
    assert bool((m2 <= 1).any()) and bool((m2 > 1).any())
    err = float((ref["raw_grad"] - raw_grad.double())[~near].abs().max()) / float(raw_grad.abs().max())
    print(f"   float64 restatement against the reference outside near: {err:.2e} of max|G|")
    mg.save("normals_fwd", log2_hashmap=np.array(lg), seed=np.array(seed), width=np.array(width), beams=np.array(beams), cam_w=np.array(cam_w),
            cam_h=np.array(cam_h), n_cam=np.array(n_cam), grid_disired_resolution=np.array(128), tdist=tdist, weights=weights,
            raw_grad_density=raw_grad, normals=normals, out_normals=renderings[-1]["normals"].detach().float(),
            out_depth=renderings[-1]["depth"].detach().float(), near=near.numpy())
    size = os.path.getsize(os.path.join(mg.HERE, "normals_fwd.npz"))
    assert size <= 200 * 1000, size


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    gen_fwd_normals()
