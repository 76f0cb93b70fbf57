"""Patch rays in the training step (`Config.patch_size`, ZI/train.py:301-314,365-388): the rays of pixel patches carry no colour, depth
or semantic supervision; the edge-aware smoothness of the rendered depth (`d_smo`) and class probabilities (`s_smo`) stands in their
place.  tests/golden/train_step_PATCH.npz (make_golden_smooth.py) is the reference's own step with two 4 x 4 patches leading the batch."""
import numpy as np
import pytest
import torch

from conftest import golden
from nerflidar_hip import losses as nl


def _patch_step_model(g, fused=False):
    from nerflidar_hip import training as ntrain, weights as nweights, lidar as nlidar, config as ncfg
    mc = ncfg.workload("REF", int(g["log2_hashmap"]))
    mc.config.use_intensity = True
    mc.__post_init__()
    sd = nweights.synth_state_dict(mc, seed=int(g["seed"]), trained_like=True)
    b = nlidar.synthetic_sweep(width=int(g["width"]), seed=int(g["seed"]), beams=list(g["beams"]))
    batch = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    for k in ("rgb", "depth", "intensity", "semantic", "mask", "patch_mask", "lidar_mask"):
        batch[k] = torch.from_numpy(g["sup_" + k]).cuda()
    return ntrain.TrainableModel(mc, fused_mlp=fused).cuda().load_reference(sd), batch


@pytest.mark.gpu
def test_whole_training_step_with_patch_rays_matches_the_reference_step():
    """The reference's whole step with Config.patch_size = 4 - `model(...)` in training mode, train.py:283-453 executed from its file,
    `.backward()`, nan_to_num_ - against the unfused `TrainableModel` + `nusc_masks` + `total_loss(patch_size=4, patch_rays=(0, 2))`:
    every loss term incl. d_smo and s_smo to 2e-4, the parameter gradients to the gates of
    test_training.py::test_whole_training_step_matches_the_reference_step (5e-3 of their norm, cosine >= 0.99999)."""
    from nerflidar_hip import training as ntrain
    g = golden("train_step_PATCH")
    s, n_patch = int(g["patch_size"]), int(g["n_patch"])
    tm, batch = _patch_step_model(g)
    assert bool((batch["patch_mask"][:n_patch * s * s] == 1).all()) and not bool(batch["patch_mask"][n_patch * s * s:].any())
    masks = nl.nusc_masks(batch, lidar_supervision=True)
    assert torch.equal(masks["mask_rgb"].cpu(), torch.from_numpy(g["mask_rgb"]))
    batch.update(masks)
    rend, hist = tm(batch, train_frac=float(g["train_frac"]), randomized=False)
    terms = nl.total_loss(rend, hist, batch, data_kind=str(g["data_loss_type"]), charb_padding=float(g["charb_padding"]),
                          data_coarse_mult=float(g["data_coarse_mult"]), data_mult=float(g["data_mult"]),
                          interlevel_mult=float(g["inter_mult"]), anti_interlevel_mult=float(g["anti_mult"]),
                          pulse_width=g["pulse_width"].tolist(), distortion_mult=float(g["dist_mult"]), depth_lam=0.1, sem_lam=0.01,
                          patch_size=s, patch_rays=(0, n_patch))
    loss = sum(terms.values())
    loss.backward()
    ntrain.clip_gradients(tm)
    assert set(terms) == {k[5:] for k in g if k.startswith("loss_")} and {"d_smo", "s_smo"} <= set(terms)
    for k, v in terms.items():
        print(f"{k}: {float(v.detach()):.8g} reference {float(g['loss_' + k]):.8g}")
    for k, v in terms.items():
        np.testing.assert_allclose(float(v.detach()), float(g["loss_" + k]), rtol=2e-4, atol=1e-7, err_msg=k)
    np.testing.assert_allclose(float(loss.detach()), float(g["loss"]), rtol=2e-4)
    named = dict(tm.named_parameters())
    report = []
    for k in [k[5:] for k in g if k.startswith("grad_")]:
        want = torch.from_numpy(g["grad_" + k]).double()
        got = named[k].grad.detach().cpu().double()
        rel = float((got - want).norm() / want.norm())
        cos = float((got * want).sum() / (got.norm() * want.norm()))
        report.append(f"{'ok ' if rel <= 5e-3 and cos >= 0.99999 else 'BAD'} {k}: rel {rel:.2e} cos {cos:.5f}")
    print("\n".join(report))
    assert not [r for r in report if r.startswith("BAD")], "\n".join(report)


def _scene_step_setup(rays=1024, patch_size=4, colourless_fraction=0.25):
    from nerflidar_hip import training as ntrain, train_scene as nts, weights as nweights, config as ncfg
    mc = ncfg.workload("REF", 12)
    mc.config.use_intensity = True
    mc.__post_init__()
    tm = ntrain.TrainableModel(mc, fused_mlp=True).cuda().load_reference(nweights.synth_state_dict(mc, seed=0, trained_like=True))
    opt = torch.optim.Adam(tm.parameters(), lr=1e-3, eps=1e-15)
    color_rays, n_patches, colourless = nts.batch_layout(rays, colourless_fraction, patch_size, 0.25)
    batch, patch_rays = nts.make_batch(rays, 0, 1, torch.device("cuda"), 1.0 / 250.0, colourless, n_patches, patch_size)
    return tm, opt, batch, color_rays, patch_rays


@pytest.mark.gpu
def test_training_step_with_patch_rays_reads_nothing_back():
    """A fused `training_step` on a pixel | patch | lidar batch with `color_rays` and the smoothness terms under
    `torch.cuda.set_sync_debug_mode("error")`: the operator, its autograd wrapper and the slicing in `total_loss` read nothing back."""
    from nerflidar_hip import training as ntrain
    tm, opt, batch, color_rays, patch_rays = _scene_step_setup()
    kw = dict(color_rays=color_rays, patch_size=4, patch_rays=patch_rays)
    first = ntrain.training_step(tm, opt, batch, **kw)                # warm-up: lazy initialisations may read back
    assert {"d_smo", "s_smo"} <= set(first) and all(np.isfinite(v) for v in first.values()) and first["d_smo"] > 0 and first["s_smo"] > 0
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ntrain.training_step(tm, opt, batch, as_tensors=True, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(isinstance(v, torch.Tensor) and v.is_cuda and v.dim() == 0 for v in out.values())
    assert np.isfinite(float(out["loss"])) and float(out["d_smo"]) > 0


@pytest.mark.gpu
def test_step_without_patch_rays_is_unchanged_by_a_patch_mask_of_zeros():
    """No `patch_rays`: the loss terms of a step have the same bits whether or not the batch carries a `patch_mask` (all zeros) and
    the `patch_valid` key `nusc_masks` now returns, and no smoothness key appears."""
    g = golden("train_step_REF")
    outs = []
    for with_mask in (False, True):
        tm, batch = _patch_step_model(g)
        if not with_mask:
            del batch["patch_mask"]
        masks = nl.nusc_masks(batch, lidar_supervision=True)
        if not with_mask:
            del masks["patch_valid"]
        batch.update(masks)
        rend, hist = tm(batch, train_frac=float(g["train_frac"]), randomized=False)
        outs.append({k: v.detach().cpu().numpy() for k, v in nl.total_loss(rend, hist, batch).items()})
    assert set(outs[0]) == set(outs[1]) == {"data", "depth", "sem", "int", "interlevel", "distortion"}
    for k in outs[0]:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k


# ---- CPU: the command line and the batch order ------------------------------------------------------------------------------------------
def test_train_scene_parser_and_batch_order():
    from nerflidar_hip import train_scene as nts
    a = nts.build_parser().parse_args(["--out", "x"])
    assert (a.patch_size, a.patch_fraction) == (0, 0.25)
    assert nts.batch_layout(a.rays, a.colourless_fraction, a.patch_size, a.patch_fraction) == (None, 0, 0)
    a = nts.build_parser().parse_args(["--out", "x", "--rays", "200", "--patch-size", "4", "--patch-fraction", "0.25", "--colourless-fraction", "0.25"])
    color_rays, n_patches, colourless = nts.batch_layout(a.rays, a.colourless_fraction, a.patch_size, a.patch_fraction)
    assert (color_rays, n_patches, colourless) == (200 - 50 - 48, 3, 50)          # floor(50 / 16) patches; they open the colourless tail
    assert nts.batch_layout(65536, 0.25, 32, 0.25) == (65536 - 2 * 16384, 16, 16384)  # the shipped batch: 16 patches of 32 x 32
    with pytest.raises(ValueError):
        nts.batch_layout(100, 0.9, 4, 0.25)
    s = a.patch_size
    batch, patch_rays = nts.make_batch(a.rays, 0, 1, torch.device("cpu"), 1.0 / 250.0, colourless, n_patches, s)
    assert patch_rays == (color_rays, n_patches) and all(v.shape[0] == a.rays for v in batch.values())
    rows = slice(color_rays, color_rays + n_patches * s * s)
    none = ~(batch["mask_rgb"] | batch["depth_mask"] | batch["sem_mask"] | batch["lidar_mask"])
    assert bool(none[rows].all()) and not bool(none[:rows.start].any()) and not bool(none[rows.stop:].any())
    assert bool(batch["mask_rgb"][:color_rays].all()) and not bool(batch["mask_rgb"][color_rays:].any())
    assert bool(batch["lidar_mask"][rows.stop:].all()) and bool(batch["depth_mask"][rows.stop:].all())
    # a patch is one pinhole camera's s x s pixel block, row-major: one origin, x neighbours (j) along base_x, y neighbours (i) along base_y
    o = batch["origins"][rows].reshape(n_patches, s, s, 3)
    d = batch["directions"][rows].reshape(n_patches, s, s, 3)
    assert torch.equal(o, o[:, :1, :1].expand_as(o))
    bx, by = batch["base_x"][rows].reshape(n_patches, s, s, 3), batch["base_y"][rows].reshape(n_patches, s, s, 3)
    dx, dy = d[:, :, 1:] - d[:, :, :-1], d[:, 1:] - d[:, :-1]
    cos = lambda u, v: (u * v).sum(-1) / (u.norm(dim=-1) * v.norm(dim=-1))
    assert float(cos(dx, bx[:, :, :-1]).min()) > 0.999 and float(cos(dy, by[:, :-1]).min()) > 0.999
    # the colours the edge weights use come from the analytic scene; the torch path of the terms runs on this batch
    assert float(batch["rgb"][rows].min()) >= 0 and float(batch["rgb"][rows].max()) > 0
    rend = [dict(rgb=batch["rgb"], depth=batch["depth"] + 0.01 * torch.rand(a.rays), semantic=torch.softmax(torch.rand(a.rays, 19), -1))]
    terms = nl.total_loss(rend, [dict(sdist=torch.linspace(0, 1, 5).expand(a.rays, 5), weights=torch.full((a.rays, 4), 0.25))], batch,
                          patch_size=s, patch_rays=patch_rays)
    assert float(terms["d_smo"]) > 0 and float(terms["s_smo"]) > 0
