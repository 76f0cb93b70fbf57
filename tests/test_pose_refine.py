"""Pose refinement (Config.pose_refine, configs.py:151; train.py:199-243,463-466): PoseNet, its window and learning rate, the batch
update, the checkpoint round trip - and on the GPU `nlr_encode_features_backward_rays` alone against float64 autograd on the CPU,
the view-direction and compositing gradients, and the whole step against the reference's (fixture `train_step_POSE`,
tests/golden/make_golden_pose.py)."""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden
from grid_ref import _grid_lookup, _level_table
from oracle import nlr_oracle as orc
from nerflidar_hip import checkpoints as nckpt, training as ntrain

RAY_GRAD_KEYS = ("origins", "directions", "viewdirs", "base_x", "base_y")
ACCURACY_LINES = []   # what the GPU tests measured; scripts/pose_refine_accuracy.py runs them and writes this list to profiles/


def _record(line):
    print(line)
    ACCURACY_LINES.append(line)


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_posenet_has_the_reference_parameter_names():
    pn = ntrain.PoseNet(5, num_lidars=2)
    assert sorted(pn.state_dict()) == ["r", "t"]                       # LearnPose.state_dict() (posenet_v2.py:96-97)
    assert tuple(pn.r.shape) == (7, 3) and tuple(pn.t.shape) == (7, 3) and pn.r.requires_grad and pn.t.requires_grad
    pn2 = ntrain.PoseNet(2, num_lidars=1, learn_R=True, learn_t=False, init_c2w=np.tile(np.eye(4, dtype=np.float32), (3, 1, 1)))
    assert sorted(pn2.state_dict()) == ["init_c2w", "r", "t"] and not pn2.t.requires_grad and not pn2.init_c2w.requires_grad
    net, opt, lr_fn = ntrain.create_posenet(3, num_lidars=2, start_step=100, end_step=600, pn_lr_init=4e-5, pn_lr_final=2e-6, lr_delay_steps=50)
    assert tuple(net.r.shape) == (5, 3) and net.t_ratio == 0.25
    g = opt.param_groups[0]
    assert tuple(g["betas"]) == (0.9, 0.99) and g["eps"] == 1e-15 and g["lr"] == 4e-5
    for step in (100, 101, 350, 600):                                  # train_utils.py:288-298: the start step is subtracted
        assert lr_fn(step) == ntrain.learning_rate_decay(step - 100, 4e-5, 2e-6, 500, 50, 1e-8), step


def test_posenet_is_the_identity_at_initialisation():
    pn = ntrain.PoseNet(3, num_lidars=1, t_ratio=0.25)
    ids = torch.tensor([3, 0, 0, 2])
    P = pn(ids)
    assert P.shape == (4, 4, 4) and torch.equal(P.detach(), torch.eye(4).expand(4, 4, 4))
    batch = {k: torch.randn(4, 3, generator=torch.Generator().manual_seed(i)) for i, k in enumerate(RAY_GRAD_KEYS + ("normals",))}
    out = ntrain.refine_batch(batch, P)
    for k in batch:
        assert torch.equal(out[k].detach(), batch[k]), k
    P.sum().backward()                                                 # and the gradient at r = 0 is finite (|r| + 1e-15)
    assert bool(torch.isfinite(pn.r.grad).all()) and bool(torch.isfinite(pn.t.grad).all())
    # a rotation about z by a small angle, a translation scaled by t_ratio
    with torch.no_grad():
        pn.r[1] = torch.tensor([0.0, 0.0, 0.3])
        pn.t[1] = torch.tensor([1.0, 2.0, 3.0])
    P = pn(torch.tensor([1])).detach()[0]
    want = np.array([[np.cos(0.3), -np.sin(0.3), 0], [np.sin(0.3), np.cos(0.3), 0], [0, 0, 1]])
    np.testing.assert_allclose(P[:3, :3].numpy(), want, atol=1e-6)
    np.testing.assert_allclose(P[:3, 3].numpy(), [0.25, 0.5, 0.75], atol=1e-7)
    assert P[3].tolist() == [0, 0, 0, 1]


def _pose_rays(g):
    """The ray batch of tests/golden/make_golden_pose.py: camera rays first, then a LiDAR sweep."""
    from nerflidar_hip import camera as ncamera, lidar as nlidar
    cam = ncamera.synthetic_camera_batch(width=int(g["cam_w"]), height=int(g["cam_h"]), focal=6.0, seed=int(g["seed"]))
    lid = nlidar.synthetic_sweep(width=int(g["width"]), seed=int(g["seed"]), beams=list(g["beams"]))
    keys = ("origins", "directions", "viewdirs", "radii", "near", "far", "base_x", "base_y")
    b = {k: np.concatenate([cam[k].reshape(cam[k].shape[0], -1), lid[k].reshape(lid[k].shape[0], -1)], 0) for k in keys}
    assert cam["origins"].shape[0] == int(g["n_cam"])
    return b


def _fixture_posenet(g):
    pn = ntrain.PoseNet(int(g["num_cams"]), num_lidars=int(g["num_lidars"]), t_ratio=float(g["t_ratio"]))
    with torch.no_grad():
        pn.r.copy_(torch.from_numpy(g["pose_r"]))
        pn.t.copy_(torch.from_numpy(g["pose_t"]))
    return pn


def test_refine_batch_equals_the_reference_lines():
    """train.py:208-221, executed from the reference's file by the fixture's generator, against `refine_batch`."""
    g = golden("train_step_POSE")
    b = {k: torch.from_numpy(v) for k, v in _pose_rays(g).items()}
    b["glo_idx"] = torch.from_numpy(g["glo_idx"])
    b["normals"] = b["viewdirs"].clone()
    keep = {k: v.clone() for k, v in b.items()}
    pn = _fixture_posenet(g)
    out = ntrain.refine_batch(b, pn(b["glo_idx"].reshape(-1).int()))
    assert out is not b and set(out) == set(b)
    for k, v in keep.items():                                          # the caller's dict and tensors are untouched
        assert b[k] is not out[k] or k in ("radii", "near", "far", "glo_idx")
        assert torch.equal(b[k], v), k
    for k in RAY_GRAD_KEYS:
        assert out[k].requires_grad
        np.testing.assert_allclose(out[k].detach().numpy(), g["refined_" + k], rtol=0, atol=2e-7, err_msg=k)
        assert not np.array_equal(g["refined_" + k], keep[k].numpy()), k
    np.testing.assert_allclose(out["normals"].detach().numpy(), g["refined_viewdirs"], rtol=0, atol=2e-7)
    for k in ("radii", "near", "far"):
        assert torch.equal(out[k], keep[k])


def test_pose_fixture_conditions():
    assert os.path.getsize(os.path.join(GOLDEN, "train_step_POSE.npz")) <= 400 * 1000
    g = golden("train_step_POSE")
    n = int(g["num_cams"]) + int(g["num_lidars"])
    assert g["pose_r"].shape == (n, 3) and g["pose_t"].shape == (n, 3) and np.all(g["pose_r"] != 0) and np.all(g["pose_t"] != 0)
    assert np.abs(g["grad_pose_r"]).min() > 0 and np.abs(g["grad_pose_t"]).min() > 0
    N = g["glo_idx"].shape[0]
    assert 0 < int(g["n_cam"]) < N and set(g["glo_idx"].reshape(-1).tolist()) == set(range(n))
    assert np.all(g["sup_lidar_mask"][:int(g["n_cam"])] == 0) and np.all(g["sup_lidar_mask"][int(g["n_cam"]):] == 1)
    for k in RAY_GRAD_KEYS:
        assert g["grad_" + k].shape == (N, 3) and np.abs(g["grad_" + k]).max() > 0, k
    assert {k for k in g if k.startswith("loss_")} == {"loss_data", "loss_depth", "loss_sem", "loss_int", "loss_interlevel", "loss_distortion"}
    assert g["out_depth"].shape == (N,)
    assert int(g["start_step"]) < int(g["step"]) < int(g["end_step"])


def test_pose_phase_and_lambda_schedule_at_the_window_edges():
    w = (10000, 20000)
    assert [ntrain.pose_phase(s, w) for s in (0, 9999, 10000, 10001, 19999, 20000, 20001)] == \
        ["before", "before", "before", "refine", "refine", "before", "frozen"]        # (sic) the two ends match no comparison
    with pytest.raises(ValueError, match="step"):
        ntrain.pose_phase(None, w)
    lam = lambda s, **kw: tuple(ntrain.loss_lambdas(s, w, **kw).values())
    assert list(ntrain.loss_lambdas(5, w)) == ["depth_lam", "sem_lam"]                # keywords of losses.total_loss
    assert lam(10000) == (0.1, 0.01) and lam(10001) == (0.0, 0.0) and lam(11999) == (0.0, 0.0)
    assert lam(12000) == (0.1, 0.01) and lam(20000) == (0.1, 0.01) and lam(20001) == (0.4, 0.04)   # int(0.6 * 20000) = 12000
    assert lam(11000, pose_refine=False) == (0.1, 0.01) and lam(25000, pose_refine=False) == (0.4, 0.04)
    assert tuple(ntrain.loss_lambdas(2999, (0, 5000)).values()) == (0.0, 0.0) and tuple(ntrain.loss_lambdas(3000, (0, 5000)).values()) == (0.1, 0.01)


class _StubModel(torch.nn.Module):
    """Stands in for TrainableModel in `training_step`: one parameter, records the batch it is called with."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(()))
        self.batches = []

    def forward(self, batch, train_frac=1.0, randomized=False, color_rays=None, **kw):
        assert not kw
        self.batches.append(batch)
        return [{"x": self.w * (batch["origins"] * batch["c"]).sum() + (batch["directions"] * batch["c"]).sum()}], []


def test_training_step_pose_window_logic(monkeypatch):
    """train.py:199-243,463-466: the batch as it is up to the start of the window, refined with gradient inside it (learning rate
    set, PoseNet stepped), refined without gradient after it; the caller's batch is never modified."""
    from nerflidar_hip import losses as nl
    seen_kw = []
    monkeypatch.setattr(nl, "total_loss", lambda rend, hist, batch, **kw: (seen_kw.append(kw), {"data": rend[-1]["x"]})[1])
    pn, pn_opt, lr_fn = ntrain.create_posenet(2, num_lidars=1, start_step=100, end_step=200, lr_delay_steps=0)
    with torch.no_grad():
        pn.r.fill_(0.01)
        pn.t.fill_(0.02)
    model = _StubModel()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    gen = torch.Generator().manual_seed(4)
    batch = {k: torch.randn(6, 3, generator=gen) for k in RAY_GRAD_KEYS + ("c",)}
    batch["glo_idx"] = torch.tensor([0, 1, 2, 0, 1, 2]).float()[:, None]
    keep = {k: v.clone() for k, v in batch.items()}
    kw = dict(randomized=False, hash_decay_mult=0.0, posenet=pn, pn_optimizer=pn_opt, pn_lr_fn=lr_fn, pose_window=(100, 200))

    def run(step, **more):
        before = (pn.r.detach().clone(), pn.t.detach().clone())
        model.batches.clear()
        ntrain.training_step(model, opt, batch, step=step, **kw, **more)
        (seen,) = model.batches
        for k, v in keep.items():
            assert torch.equal(batch[k], v), k
        return seen, not (torch.equal(before[0], pn.r) and torch.equal(before[1], pn.t))

    for step in (0, 99, 100, 200):
        seen, moved = run(step)
        assert seen is batch and not moved, step
    for step in (201, 5000):
        with torch.no_grad():
            want = ntrain.refine_batch(batch, pn(batch["glo_idx"]))
        seen, moved = run(step)
        assert not moved and not seen["origins"].requires_grad and torch.equal(seen["origins"], want["origins"]), step
        assert torch.equal(seen["directions"], want["directions"]) and not torch.equal(seen["directions"], batch["directions"])
    pn_opt.param_groups[0]["lr"] = 123.0
    seen, moved = run(101)
    assert moved and seen["origins"].requires_grad and seen["base_y"].requires_grad and pn_opt.param_groups[0]["lr"] == lr_fn(101)
    assert seen_kw[-1] == {"depth_lam": 0.0, "sem_lam": 0.0}                           # 101 < int(0.6 * 200): the schedule of train.py:333,405
    seen, moved = run(199)
    assert moved and pn_opt.param_groups[0]["lr"] == lr_fn(199) and seen_kw[-1] == {"depth_lam": 0.1, "sem_lam": 0.01}
    run(150, depth_lam=0.3)                                                            # a caller's own weight wins
    assert seen_kw[-1] == {"depth_lam": 0.3, "sem_lam": 0.01}
    run(201)
    assert seen_kw[-1] == {"depth_lam": 0.4, "sem_lam": 0.04}
    # without a PoseNet the step is the one it was: the caller's batch, the caller's keywords
    model.batches.clear()
    ntrain.training_step(model, opt, batch, randomized=False, hash_decay_mult=0.0)
    assert model.batches[0] is batch and seen_kw[-1] == {}
    with pytest.raises(ValueError, match="step"):
        ntrain.training_step(model, opt, batch, randomized=False, hash_decay_mult=0.0, posenet=pn, pn_optimizer=pn_opt, pn_lr_fn=lr_fn)
    with pytest.raises(ValueError, match="pn_optimizer"):
        ntrain.training_step(model, opt, batch, randomized=False, hash_decay_mult=0.0, posenet=pn, step=150, pose_window=(100, 200))


def test_posenet_checkpoint_round_trip(tmp_path):
    pn, pn_opt, _ = ntrain.create_posenet(3, num_lidars=2)
    rng = np.random.default_rng(2)
    with torch.no_grad():
        pn.r.copy_(torch.from_numpy(rng.normal(size=(5, 3)).astype(np.float32) * 0.01))
        pn.t.copy_(torch.from_numpy(rng.normal(size=(5, 3)).astype(np.float32) * 0.01))
    path = nckpt.save_posenet(tmp_path, pn, 7000, pn_opt)
    assert os.path.basename(path) == "posenet_ckpt_7000.ckpt"
    nckpt.save_posenet(tmp_path, ntrain.PoseNet(3, num_lidars=2), 6000)
    nckpt.save_checkpoint(tmp_path, {"x": torch.zeros(1)}, 9000)      # the model's own checkpoint in the same directory
    sd, step = nckpt.load_checkpoint(tmp_path, prefix="posenet_ckpt_")
    assert step == 7000 and sorted(sd) == ["r", "t"]
    pn2 = ntrain.PoseNet(3, num_lidars=2, t_ratio=0.25)
    assert nckpt.restore_posenet(tmp_path, pn2) == 7000
    ids = torch.arange(5)
    assert torch.equal(pn2(ids), pn(ids))
    assert nckpt.restore_posenet(tmp_path, pn2, step=6000) == 6000 and torch.equal(pn2(ids).detach(), torch.eye(4).expand(5, 4, 4))
    with pytest.raises(ValueError, match="posenet checkpoint"):
        nckpt.restore_posenet(tmp_path, ntrain.PoseNet(3, num_lidars=1))
    from nerflidar_hip import train_scene
    a = train_scene.build_parser().parse_args(["--out", str(tmp_path), "--pose-refine", "--pose-frames", "3"])
    assert a.pose_refine and a.pose_frames == 3


# ---- the float64 reference of the kernel test (CPU, torch autograd) -----------------------------------------------------------
def _ref_features(rays, tdist, rand_deg, table, enc, n, re_w, dtype, want_pos=False):
    """Features [N, S, L*C] of the fused operator in `dtype`, differentiable in rays = (o, d, bx, by): oracle cast_rays +
    contract_mean_std, / bound (2), the lookup above, the erf weight of models.py:976, the mean over the multisamples."""
    o, d, bx, by, radii = [t.to(dtype) for t in rays]
    means, stds = orc.cast_rays(tdist.to(dtype), o, d, radii, bx, by, n=n, m=3, std_scale=0.35, rand_deg=None if rand_deg is None else rand_deg.to(dtype))
    z, zs = orc.contract_mean_std(means, stds)
    x01 = (z / 2 + 1) / 2
    f = _grid_lookup(x01.reshape(-1, 3), table.to(dtype), enc).reshape(x01.shape[:-1] + (enc.num_levels, -1))   # [N,S,n,L,C]
    if re_w:
        gs = enc.grid_sizes.to(dtype)
        f = f * torch.erf(1 / torch.clamp(torch.sqrt(8 * (zs / 2)[..., None] ** 2 * gs ** 2), min=1e-10))[..., None]
    f = f.mean(dim=2).flatten(-2, -1)
    return (f, x01, means) if want_pos else f


def _near_face(x01, enc, tol=1e-4):
    """[N] bool: does any (sample, multisample, level, axis) coordinate of the ray lie within `tol` cell of a cell face (float64)?"""
    bad = torch.zeros(x01.shape[0], dtype=torch.bool)
    for scale, *_ in _level_table(enc):
        pos = x01 * scale + (0.0 if enc.align_corners else 0.5)
        bad |= ((pos - torch.round(pos)).abs() < tol).flatten(1).any(-1)
    return bad


def _candidate_rays(N, S, n, seed, rand):
    rng = np.random.default_rng(seed)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    d = rng.normal(size=(N, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d *= rng.uniform(0.8, 1.25, size=(N, 1))                            # not unit: |d| is part of the map
    a = rng.normal(size=(N, 3))
    bx = np.cross(d, a)
    bx /= np.linalg.norm(bx, axis=-1, keepdims=True)
    by = np.cross(d, bx)
    by /= np.linalg.norm(by, axis=-1, keepdims=True)
    o = rng.uniform(-0.3, 0.3, size=(N, 3))
    radii = rng.uniform(0.005, 0.03, size=(N, 1))
    # |o| <= 0.52 and 0.8 <= |d| <= 1.25: an interval that ends at t <= 0.35 lies inside the unit sphere, one that starts at t >= 2.4
    # outside it.  S >= 3: the first and the last interval are such; S = 1: one interval from t <= 0.3 to t >= 2.2, whose multisamples
    # (sample_n = 7) lie on both sides
    if S >= 3:
        tdist = np.concatenate([rng.uniform(0.05, 0.15, size=(N, 1)), rng.uniform(0.2, 0.35, size=(N, 1)),
                                np.sort(rng.uniform(0.35, 2.4, size=(N, S - 3)), axis=-1), rng.uniform(2.4, 2.6, size=(N, 1)),
                                rng.uniform(2.8, 3.0, size=(N, 1))], -1)
    else:
        assert S == 1
        tdist = np.concatenate([rng.uniform(0.05, 0.3, size=(N, 1)), rng.uniform(2.2, 2.6, size=(N, 1))], -1)
    rd = f(rng.uniform(0, 1, size=(N, S, n))) if rand else None
    return [f(o), f(d), f(bx), f(by), f(radii)], f(tdist), rd


@functools.lru_cache(maxsize=None)
def _encoder(L, C, interp="linear", align=False, gridtype="hash"):
    """Base resolution 16, scale 2, 2^14 rows per level: the 17^3 level is dense, the finer ones are hashed."""
    from nerflidar_hip.gridencoder import GridEncoder
    enc = GridEncoder(num_levels=L, level_dim=C, per_level_scale=2, base_resolution=16, log2_hashmap_size=14, interpolation=interp,
                      align_corners=align, gridtype=gridtype)
    gen = torch.Generator().manual_seed(100 * L + C)
    with torch.no_grad():
        enc.embeddings.copy_(torch.rand(enc.embeddings.shape, generator=gen) * 2 - 1)
    return enc


@functools.lru_cache(maxsize=None)
def _pick_rays(S, n, L, C, rand, N, interp, align, gridtype):
    """N rays of a seeded pool and which of them are near a cell face.  A ray with a coordinate within 1e-4 cell of a face (in
    float64) is `near` and left out of the comparison (its float32 twin may sit in the neighbouring cell, where the derivative differs
    although the feature does not).  The pool is walked in order and rays are taken as they come, except that near-face rays are
    passed over once they make up a tenth of the batch: at S = 70, n = 7, L = 4 a ray has 5 880 coordinates and 7 of 10 pool rays
    are near a face, so no seed keeps a batch of 37 under the cap of 30 % by itself.  (Positions do not depend on the table.)"""
    enc = _encoder(L, C, interp, align, gridtype)
    pool = 12 * N
    rays, tdist, rd = _candidate_rays(pool, S, n, 1000 + S * 10 + n, rand)
    with torch.no_grad():
        _, x01, _ = _ref_features(rays, tdist, rd, enc.embeddings.detach(), enc, n, False, torch.float64, want_pos=True)
    near_pool = _near_face(x01, enc)
    pick, n_near = [], 0
    for i in range(pool):
        if len(pick) == N:
            break
        if near_pool[i]:
            if n_near >= N // 10:
                continue
            n_near += 1
        pick.append(i)
    assert len(pick) == N, f"the pool of {pool} rays holds fewer than {N} usable ones"
    pick = torch.tensor(pick)
    near = near_pool[pick]
    assert int(near.sum()) <= 0.3 * N
    return [t[pick].contiguous() for t in rays], tdist[pick].contiguous(), None if rd is None else rd[pick].contiguous(), near


@functools.lru_cache(maxsize=None)
def _kernel_case(S, n, L, C, half, re_w, rand, N=37, interp="linear", align=False, gridtype="hash"):
    """Rays, cotangent and the float64 / float32 CPU references of one case, computed once."""
    enc = _encoder(L, C, interp, align, gridtype)
    table = enc.embeddings.detach()
    table = table.half().float() if half else table
    rays, tdist, rd, near = _pick_rays(S, n, L, C, rand, N, interp, align, gridtype)
    cot = torch.randn(N, S, L * C, generator=torch.Generator().manual_seed(S + 7 * n))
    refs = {}
    for dtype in (torch.float64, torch.float32):
        leaf = [t.detach().clone().to(dtype).requires_grad_(True) for t in rays[:4]]
        f, x01, means = _ref_features(leaf + [rays[4]], tdist, rd, table, enc, n, re_w, dtype, want_pos=True)
        refs[dtype] = [g.double() for g in torch.autograd.grad((f * cot.to(dtype)).sum(), leaf)]
        if dtype == torch.float64:
            m2 = (means.detach() ** 2).sum(-1).flatten(1)
            both = ((m2 <= 1).any(-1) & (m2 > 1).any(-1))
            f64 = f.detach()
    return dict(enc=enc, table=table, rays=rays, tdist=tdist, rd=rd, near=near, cot=cot, want=refs[torch.float64], f32=refs[torch.float32],
                both=both, feats=f64, x01=x01.detach())


def test_reference_lookup_matches_the_oracle_and_the_cases_hold_what_they_claim():
    """The forward of the differentiable lookup against `oracle.grid_encode_numpy`; in every case at most 30 % of the rays are near a
    face, and both contraction branches occur on every ray."""
    for L, C in ((4, 4), (4, 1), (3, 2)):
        k = _kernel_case(33, 7, L, C, False, True, False)
        enc = k["enc"]
        x = k["x01"].reshape(-1, 3)
        got = _grid_lookup(x.float(), k["table"], enc).permute(1, 0, 2).numpy()
        want = orc.grid_encode_numpy(x.float().numpy(), k["table"].numpy(), enc._offsets_host.numpy(), float(np.log2(enc.per_level_scale)),
                                     enc.base_resolution, enc.gridtype_id, enc.align_corners)
        # a float32 position on the finest level (up to 129.5) carries an error of 2^-17, the two round x * scale + 0.5 differently,
        # and a feature changes by at most 2 (table values in [-1, 1]) per unit of each of the 3 coordinates: 6 * 2^-17 = 4.6e-5.
        # A wrong cell, corner or hash shows as an error of order 1.
        np.testing.assert_allclose(got, want, rtol=0, atol=4.6e-5)
        assert [h for *_, h in _level_table(enc)] == [False] + [True] * (L - 1)
    for S in (1, 3, 33, 64, 70):
        for n in (1, 7):
            k = _kernel_case(S, n, 4, 4, False, True, True)
            assert int(k["near"].sum()) <= 0.3 * 37
            if S * n > 1:
                assert bool(k["both"].all()), (S, n)


# ---- GPU: the kernel alone -------------------------------------------------------------------------------------------------
def _gpu_ray_grads(k, n, re_w, requires=(True, True, True, True), table_grad=False):
    """features and ray gradients of a case through `encode_features_fused` on the GPU."""
    enc = k["enc"]
    dev = torch.device("cuda")
    table = k["table"].to(dev)
    e2 = type("Enc", (), {})()                                         # the encoder's attributes with this case's table (f32 or f16 values)
    for a in ("num_levels", "output_dim", "base_resolution", "per_level_scale", "_offsets_host", "gridtype_id", "align_corners", "interp_id"):
        setattr(e2, a, getattr(enc, a))
    e2.embeddings = (table.half() if k.get("half") else table).requires_grad_(table_grad)
    o, d, bx, by, radii = [t.to(dev) for t in k["rays"]]
    leaves = [t.detach().clone().requires_grad_(r) for t, r in zip((o, d, bx, by), requires)]
    batch = dict(origins=leaves[0], directions=leaves[1], base_x=leaves[2], base_y=leaves[3], radii=radii, viewdirs=d, near=radii, far=radii)
    rd = None if k["rd"] is None else k["rd"].to(dev)
    f = ntrain.encode_features_fused(e2, batch, k["tdist"].to(dev), n, 3, rand_deg=rd, re_weights=re_w)
    grads = [None] * 4
    if any(requires) or table_grad:
        (f * k["cot"].to(dev)).sum().backward()
        grads = [t.grad for t in leaves]
    return f.detach(), grads, e2.embeddings.grad


KERNEL_CASES = [(S, n, L, C) for S in (1, 3, 33, 64, 70) for n in (1, 7) for (L, C) in ((4, 4), (4, 1), (3, 2))]


@pytest.mark.gpu
@pytest.mark.parametrize("S,n,L,C", KERNEL_CASES)
def test_encode_ray_gradient_matches_float64_autograd(S, n, L, C):
    """`nlr_encode_features_backward_rays` (through `_EncodeFeatures`) against float64 autograd on the CPU, N = 37, for f32 and f16
    tables, re_weights on and off, rand_deg on and off.  The gate is not a constant: per output tensor the same reference evaluated in
    float32 on the CPU deviates from float64 by some amount (the order of its sums is its own), and the kernel may deviate by at most
    4 x that, over the rays that are not near a cell face.  Every figure is printed beside 2e-5 max|want|, the gate of the other f32
    backward kernels."""
    names = ("d_origins", "d_directions", "d_base_x", "d_base_y")
    for half in (False, True):
        for re_w in (True, False):
            for rand in (False, True):
                k = dict(_kernel_case(S, n, L, C, half, re_w, rand), half=half)
                keep = ~k["near"]
                f, grads, _ = _gpu_ray_grads(k, n, re_w)
                torch.cuda.synchronize()
                ferr = float((f.cpu().double() - k["feats"]).abs().max())
                # the forward, as a check of the case itself (same inputs on both sides; a mismatch in the set-up shows as an error
                # of order 1): float32 positions on the finest level carry 2^-17 cell, once from x01 and once from x01 * scale + 0.5,
                # and a feature moves by at most 2 per cell and axis (table in [-1, 1]): 2 * 6 * 2^-17 = 9.2e-5
                assert ferr <= 9.2e-5, ("features", ferr)
                for name, got, want, f32 in zip(names, grads, k["want"], k["f32"]):
                    got = got.cpu().double()
                    assert got.shape == want.shape and bool(torch.isfinite(got).all())
                    err = float((got - want)[keep].abs().max())
                    yard = float((f32 - want)[keep].abs().max())
                    scale = float(want[keep].abs().max())
                    _record(f"kernel S={S} n={n} L={L} C={C} {'f16' if half else 'f32'} re_w={int(re_w)} rand={int(rand)} {name}: err {err:.3e} "
                            f"f32-reference {yard:.3e} (x{err / max(yard, 1e-300):.2f}) max|want| {scale:.3e} err/max {err / max(scale, 1e-300):.2e} "
                            f"left out {int(k['near'].sum())}/37")
                    # (sample_n = 1 without rand_deg: ly = 0, d_base_y is exactly 0 in all three)
                    assert err <= 4 * yard, (name, half, re_w, rand, err, yard)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["smoothstep", "align_corners", "tiled", "level_dim_8"])
def test_encode_ray_gradient_other_grids(variant):
    """The envelope of the forward: smoothstep interpolation, align_corners, the tiled grid type, 8 features per level; same gate, and
    the features themselves at the bound of test_encode_ray_gradient_matches_float64_autograd (derived there)."""
    kw = dict(smoothstep=dict(interp="smoothstep"), align_corners=dict(align=True), tiled=dict(gridtype="tiled"), level_dim_8={})[variant]
    k = dict(_kernel_case(33, 7, 3, 8 if variant == "level_dim_8" else 2, False, True, False, **kw), half=False)
    keep = ~k["near"]
    f, grads, _ = _gpu_ray_grads(k, 7, True)
    ferr = float((f.cpu().double() - k["feats"]).abs().max())
    _record(f"kernel {variant} features: err {ferr:.3e}")
    assert f.shape == k["feats"].shape and ferr <= 9.2e-5, ("features", ferr)
    for name, got, want, f32 in zip(("d_origins", "d_directions", "d_base_x", "d_base_y"), grads, k["want"], k["f32"]):
        err, yard = float((got.cpu().double() - want)[keep].abs().max()), float((f32 - want)[keep].abs().max())
        _record(f"kernel {variant} {name}: err {err:.3e} f32-reference {yard:.3e} max|want| {float(want[keep].abs().max()):.3e}")
        assert err <= 4 * yard, (name, err, yard)


@pytest.mark.gpu
def test_encode_ray_gradient_is_repeatable_and_optional_outputs_are_independent():
    """Two runs give the same 12 N floats bit for bit; asking for one tensor's gradient only gives the same bits for it; with no ray
    gradient requested the features and the table's gradient inputs are the bits of the path without the feature."""
    k = dict(_kernel_case(70, 7, 4, 4, False, True, True), half=False)
    f0, g0, t0 = _gpu_ray_grads(k, 7, True, table_grad=True)
    f1, g1, _ = _gpu_ray_grads(k, 7, True, table_grad=True)
    assert torch.equal(f0, f1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    for i in range(4):
        only = tuple(j == i for j in range(4))
        _, g, _ = _gpu_ray_grads(k, 7, True, requires=only)
        assert torch.equal(g[i], g0[i]) and all(g[j] is None for j in range(4) if j != i)
    f2, g2, t2 = _gpu_ray_grads(k, 7, True, requires=(False,) * 4, table_grad=True)
    assert torch.equal(f2, f0) and all(g is None for g in g2)
    # The table gradient is summed with float atomics at this size (no workspace for the binned scatter): two runs of the SAME call
    # differ in the order of additions, so there are no bits to be identical to.  t0 and t1 are such a pair; the run without ray
    # gradients is held to the gate of the f32 backward kernels on top of what they differ by.
    _, _, t1 = _gpu_ray_grads(k, 7, True, table_grad=True)
    spread, cross = float((t1 - t0).abs().max()), float((t2 - t0).abs().max())
    print(f"table gradient: the same call twice moves {spread:.2e}, with / without ray gradients {cross:.2e} (largest entry {float(t0.abs().max()):.2e})")
    assert cross <= 2e-5 * float(t0.abs().max()) + spread


@pytest.mark.gpu
def test_unsupported_grid_is_an_error_with_a_message():
    import ctypes as C
    from nerflidar_hip import _lib
    k = _kernel_case(3, 7, 3, 2, False, True, False)
    dev = torch.device("cuda")
    tab = torch.zeros(k["table"].shape[0] * 2 // 3, 3, device=dev)
    keep = [t.to(dev) for t in k["rays"]]
    order = dict(origins=keep[0], directions=keep[1], base_x=keep[2], base_y=keep[3], radii=keep[4], viewdirs=keep[1], near=keep[4], far=keep[4])
    rays, held = _lib.rays(order, 37)
    gd = ntrain._EncodeFeatures._descs(k["enc"], tab)
    g = torch.zeros(37 * 3, 9, device=dev)
    out = torch.zeros(37, 3, device=dev)
    rc = _lib.lib().nlr_encode_features_backward_rays(C.byref(rays), _lib.ptr(k["tdist"].to(dev)), 37, 3, 7, 3, 0.35, None, C.byref(gd), 1, _lib.ptr(g),
                                                      _lib.ptr(out), None, None, None, _lib.current_stream())
    assert rc != 0 and b"level_dim" in _lib.lib().nlr_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("level", ["nerf_mlp", "prop_mlp_0"])
def test_encode_ray_gradient_shipped_shapes(level):
    """L = 10, C = 4 (NerfMLP) and L = 6, C = 1 (first proposal level) with the trained tables of tests/golden/ckpt_trained, N = 64,
    S = 32, sample_n = 7, no ray left out.  Relative norm error and 1 - cosine against float64, each at most 4 x what the float32 CPU
    reference shows against float64."""
    from nerflidar_hip import config as nconfig
    sd, _ = nckpt.load_checkpoint(os.path.join(GOLDEN, "ckpt_trained"))
    sd, _ = nckpt.split_state_dict(sd)
    mc = nckpt.infer_model_config(sd, nconfig.workload("REFI", 13))
    from nerflidar_hip.gridencoder import GridEncoder
    enc = GridEncoder.from_mlp_config(mc.nerf_mlp if level == "nerf_mlp" else mc.prop_cfg(0))
    with torch.no_grad():
        enc.embeddings.copy_(torch.from_numpy(sd[level + ".encoder.embeddings"]).float())
    assert (enc.num_levels, enc.level_dim) == {"nerf_mlp": (10, 4), "prop_mlp_0": (6, 1)}[level]
    N, S, n = 64, 32, 7
    rays, tdist, _ = _candidate_rays(N, S, n, 77, False)
    table = enc.embeddings.detach().float()
    cot = torch.randn(N, S, enc.output_dim, generator=torch.Generator().manual_seed(5))
    refs = {}
    for dtype in (torch.float64, torch.float32):
        leaf = [t.detach().clone().to(dtype).requires_grad_(True) for t in rays[:4]]
        f = _ref_features(leaf + [rays[4]], tdist, None, table, enc, n, True, dtype)
        refs[dtype] = [g.double() for g in torch.autograd.grad((f * cot.to(dtype)).sum(), leaf)]
    k = dict(enc=enc, table=table, rays=rays, tdist=tdist, rd=None, cot=cot, half=False)
    _, grads, _ = _gpu_ray_grads(k, n, True)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    cosm = lambda a, b: 1.0 - float((a * b).sum() / (a.norm() * b.norm()))
    for name, got, want, f32 in zip(("d_origins", "d_directions", "d_base_x", "d_base_y"), grads, refs[torch.float64], refs[torch.float32]):
        got = got.cpu().double()
        r, c, r32, c32 = rel(got, want), cosm(got, want), rel(f32, want), cosm(f32, want)
        _record(f"shipped {level} L={enc.num_levels} C={enc.level_dim} {name}: rel {r:.3e} 1-cos {c:.3e}; f32-reference rel {r32:.3e} 1-cos {c32:.3e}")
        assert r <= 4 * r32 and c <= 4 * max(c32, 2.0 ** -52), (name, r, r32, c, c32)


# ---- GPU: the view-direction and compositing gradients ------------------------------------------------------------------------
def _small_model(fused, seed=3, intensity=True):
    from nerflidar_hip import config as ncfg, weights as nweights
    mc = ncfg.workload("REF", 12)
    mc.config.use_intensity = intensity
    mc.__post_init__()
    sd = nweights.synth_state_dict(mc, seed=seed, trained_like=True)
    return ntrain.TrainableModel(mc, fused_mlp=fused).cuda().load_reference(sd), mc


@pytest.mark.gpu
def test_composite_direction_gradient_matches_autograd_of_the_same_formula():
    """`volumetric_render` hands `dirs` the gradient of density dt |d| (render.py:176-178) computed from the kernel's d_density:
    against float64 autograd through the oracle's compositing; and the other outputs are the bits they were without it."""
    gen = torch.Generator().manual_seed(8)
    N, S = 37, 33
    density = torch.rand(N, S, generator=gen) * 3
    tdist = torch.sort(torch.rand(N, S + 1, generator=gen) * 2 + 0.05, -1).values
    dirs = torch.randn(N, 3, generator=gen)
    rgbs = torch.rand(N, S, 3, generator=gen)
    cot_rgb, cot_d, cot_a = torch.randn(N, 3, generator=gen), torch.randn(N, generator=gen), torch.randn(N, generator=gen)

    def run(with_grad):
        dn = density.cuda().requires_grad_(True)
        dr = dirs.cuda().requires_grad_(with_grad)
        r = ntrain.volumetric_render(dn, tdist.cuda(), dr, rgbs.cuda(), None, None, True, 1.0)
        ((r["rgb"] * cot_rgb.cuda()).sum() + (r["depth"] * cot_d.cuda()).sum() + (r["acc"] * cot_a.cuda()).sum()).backward()
        return {k: v.detach() for k, v in r.items()}, dn.grad, dr.grad

    r0, gd0, none = run(False)
    r1, gd1, gdir = run(True)
    assert none is None and torch.equal(gd0, gd1) and all(torch.equal(r0[k], r1[k]) for k in r0)
    d64 = dirs.double().requires_grad_(True)
    # d loss / d |d| through the weights only: every output is a function of the weights (and data), so contract the kernel's own
    # d_density the way the chain rule says and compare with autograd of sum_s d_density_s * density_s * |d| / |d|
    want = torch.autograd.grad(((gd1.cpu().double() * density.double()).sum(-1) * d64.norm(dim=-1) / dirs.double().norm(dim=-1)).sum(), d64)[0]
    err = float((gdir.cpu().double() - want).abs().max())
    _record(f"composite d_dirs: err {err:.3e} max|want| {float(want.abs().max()):.3e}")
    assert err <= 2e-5 * float(want.abs().max())
    # and a finite difference of the rendered depth along |d| confirms that the contraction is the right one
    eps = 1e-2
    rp = ntrain.volumetric_render(density.cuda(), tdist.cuda(), (dirs * (1 + eps)).cuda(), rgbs.cuda(), None, None, True, 1.0)
    rm = ntrain.volumetric_render(density.cuda(), tdist.cuda(), (dirs * (1 - eps)).cuda(), rgbs.cuda(), None, None, True, 1.0)
    fd = sum(((rp[k] - rm[k]).cpu().double() * c.double()).sum() for k, c in (("rgb", cot_rgb), ("depth", cot_d), ("acc", cot_a))) / (2 * eps)
    per_ray = (gdir.cpu().double() * dirs.double()).sum(-1)
    an = float(per_ray.sum())
    assert abs(float(fd) - an) <= 1e-2 * float(per_ray.abs().sum()) + 1e-3, (float(fd), an)


@pytest.mark.gpu
def test_fused_mlp_view_direction_gradient_and_unchanged_outputs():
    """`_FusedMLP` returns d loss / d enc only when enc requires one; its other results are the same bits either way, and the
    gradient agrees with the torch Linear stack's (fp32) to the accuracy of the bf16 chain."""
    tmf, mc = _small_model(True)
    tmu, _ = _small_model(False)
    from nerflidar_hip import lidar as nlidar
    b = {k: torch.from_numpy(v).cuda() for k, v in nlidar.synthetic_sweep(width=8, seed=3, beams=nlidar.LIDAR_ANGLES[::4]).items()}
    N = b["origins"].shape[0]
    td = torch.sort(torch.rand(N, 33, generator=torch.Generator().manual_seed(1)) * 1.5 + 0.01, -1).values.cuda()
    cot = torch.randn(N, 32, 3, generator=torch.Generator().manual_seed(2)).cuda()

    def run(level, with_grad):
        level.zero_grad(set_to_none=True)
        v = b["viewdirs"].clone().requires_grad_(with_grad)
        o = level(dict(b, viewdirs=v), td)
        (o["rgb"] * cot).sum().backward()
        return {k: t.detach() for k, t in o.items()}, v.grad, {k: p.grad.clone() for k, p in level.named_parameters() if p.grad is not None and "embeddings" not in k}

    o0, none, p0 = run(tmf.nerf_mlp, False)
    o1, gv, p1 = run(tmf.nerf_mlp, True)
    assert none is None and gv is not None
    assert all(torch.equal(o0[k], o1[k]) for k in o0) and set(p0) == set(p1) and all(torch.equal(p0[k], p1[k]) for k in p0)
    _, gu, _ = run(tmu.nerf_mlp, True)
    rel = float((gv - gu).norm() / gu.norm())
    cos = float((gv * gu).sum() / (gv.norm() * gu.norm()))
    _record(f"fused view-direction gradient against the fp32 Linear stack: rel {rel:.3e} cos {cos:.6f} (1 - cos {1 - cos:.2e})")
    # a measured gate (profiles/pose_refine_accuracy.txt: rel 8.2e-2, 1 - cos 3.4e-3 on an MI355X): twice those figures.  They are
    # of the order DESIGN quotes for the fused chain's weight gradients against fp32 (3.7e-2 / 7e-4); the direction's gradient is the
    # bf16 pre-activation gradients summed over a ray's samples and multiplied by pos_enc's 2^k slopes.
    assert rel <= 2 * 8.2e-2 and 1 - cos <= 2 * 3.4e-3


# ---- GPU: the step against the reference ------------------------------------------------------------------------------------
def _pose_scene(g, fused):
    from nerflidar_hip import losses as nl
    tm, mc = _small_model(fused, seed=int(g["seed"]))
    batch = {k: torch.from_numpy(v).cuda() for k, v in _pose_rays(g).items()}
    for k in ("rgb", "depth", "intensity", "semantic", "mask", "patch_mask", "lidar_mask"):
        batch[k] = torch.from_numpy(g["sup_" + k]).cuda()
    batch["glo_idx"] = torch.from_numpy(g["glo_idx"]).cuda()
    masks = nl.nusc_masks(batch, lidar_supervision=True)
    assert torch.equal(masks["mask_rgb"].cpu(), torch.from_numpy(g["mask_rgb"]))
    batch.update(masks)
    return tm, batch, _fixture_posenet(g).cuda()


def _pose_step(g, fused):
    """forward + loss + backward on the fixture's batch -> loss terms, depth, posenet and ray gradients"""
    from nerflidar_hip import losses as nl
    tm, batch, pn = _pose_scene(g, fused)
    refined = ntrain.refine_batch(batch, pn(batch["glo_idx"].reshape(-1).int()))
    for k in RAY_GRAD_KEYS:
        refined[k].retain_grad()
    rend, hist = tm(refined, train_frac=float(g["train_frac"]), randomized=False)
    terms = nl.total_loss(rend, hist, refined, **ntrain.loss_lambdas(int(g["step"]), (int(g["start_step"]), int(g["end_step"]))))
    loss = sum(terms.values())
    loss.backward()
    ntrain.clip_gradients(pn)
    grads = {"pose_r": pn.r.grad, "pose_t": pn.t.grad, **{k: refined[k].grad for k in RAY_GRAD_KEYS}}
    return terms, loss, rend[-1]["depth"].detach(), grads


def _grad_report(grads, g, tag):
    rows = {}
    for k, got in grads.items():
        assert got is not None, f"{k}: no gradient reached it"
        got, want = got.detach().cpu().double(), torch.from_numpy(g["grad_" + k]).double()
        rows[k] = (float((got - want).norm() / want.norm()), float((got * want).sum() / (got.norm() * want.norm())))
        _record(f"step {tag} {k}: rel {rows[k][0]:.2e} cos {rows[k][1]:.6f} (1 - cos {1 - rows[k][1]:.2e})")
    return rows


@pytest.mark.gpu
def test_pose_refinement_step_matches_the_reference_step():
    """The reference's step with a refined batch (posenet forward, train.py:208-221, `model(False, batch, ...)`, the loss block,
    `.backward()`: tests/golden/make_golden_pose.py) against refine_batch + TrainableModel on the fp32 path: loss terms to 2e-4,
    depth to 2e-4, the PoseNet's gradients and d loss / d each of the five ray tensors to 5e-3 of their norm with a cosine of at
    least 0.99999 (the gates of test_track_refine.py)."""
    g = golden("train_step_POSE")
    terms, loss, depth, grads = _pose_step(g, fused=False)
    assert set(terms) == {k[5:] for k in g if k.startswith("loss_")}
    for k, v in terms.items():
        np.testing.assert_allclose(float(v.detach()), float(g["loss_" + k]), rtol=2e-4, atol=1e-7, err_msg=k)
    np.testing.assert_allclose(float(loss.detach()), float(g["loss"]), rtol=2e-4)
    np.testing.assert_allclose(depth.cpu().numpy(), g["out_depth"], atol=2e-4, rtol=0)
    rows = _grad_report(grads, g, "fp32")
    bad = {k: v for k, v in rows.items() if not (v[0] <= 5e-3 and v[1] >= 0.99999)}
    assert not bad, bad


# fused bf16 step against the fixture on an MI355X: (rel, 1 - cos) per tensor
FUSED_MEASURED = {"pose_r": (1.60e-2, 8.7e-5), "pose_t": (1.26e-2, 7.9e-5), "origins": (3.41e-2, 5.71e-4), "directions": (3.30e-2, 5.39e-4),
                  "viewdirs": (7.49e-2, 2.773e-3), "base_x": (3.57e-2, 5.37e-4), "base_y": (4.24e-2, 8.67e-4)}


@pytest.mark.gpu
def test_pose_refinement_step_on_the_fused_path():
    """The same fixture through the fused bf16 NerfMLP; loss terms to 2e-2.  The gradients' gate is a measured one, per tensor: twice
    what an MI355X gave against the fixture (FUSED_MEASURED, profiles/pose_refine_accuracy.txt), where the fp32 path deviates by
    8e-5 .. 2.2e-4.  The figures are of the order DESIGN quotes for the fused chain's weight gradients against fp32 (rel 3.7e-2,
    1 - cos 7e-4); viewdirs, whose gradient passes pos_enc's 2^k slopes, is the largest."""
    g = golden("train_step_POSE")
    terms, loss, depth, grads = _pose_step(g, fused=True)
    for k, v in terms.items():
        np.testing.assert_allclose(float(v.detach()), float(g["loss_" + k]), rtol=2e-2, atol=1e-6, err_msg=k)
    rows = _grad_report(grads, g, "fused")
    bad = {k: v for k, v in rows.items() if not (v[0] <= 2 * FUSED_MEASURED[k][0] and 1 - v[1] <= 2 * FUSED_MEASURED[k][1])}
    assert not bad, bad


@pytest.mark.gpu
def test_rays_without_gradient_leave_the_step_bit_identical():
    """A batch of plain data makes exactly the calls it made before the feature; with ray gradients requested, the fused path's
    renderings and history are the same bits (the forward kernels are the same launches)."""
    from nerflidar_hip import losses as nl
    g = golden("train_step_POSE")
    tm, batch, pn = _pose_scene(g, fused=True)
    def plain():
        tm.zero_grad(set_to_none=True)
        r, h = tm(batch, train_frac=0.5, randomized=False)
        sum(nl.total_loss(r, h, batch).values()).backward()
        return r, h, {k: p.grad.clone() for k, p in tm.named_parameters() if p.grad is not None and "embeddings" not in k}

    r0, h0, p0 = plain()
    r0b, h0b, p0b = plain()                                            # the same call again: which gradients have bits to be identical to
    tm.zero_grad(set_to_none=True)
    with_grad = {k: (v.clone().requires_grad_(True) if k in RAY_GRAD_KEYS else v) for k, v in batch.items()}
    r1, h1 = tm(with_grad, train_frac=0.5, randomized=False)
    sum(nl.total_loss(r1, h1, with_grad).values()).backward()
    for la, lb in zip(r0 + h0, r1 + h1):
        for k in la:
            assert torch.equal(la[k].detach(), lb[k].detach()), k
    p1 = {k: p.grad.clone() for k, p in tm.named_parameters() if p.grad is not None and "embeddings" not in k}
    assert set(p0) == set(p1) == set(p0b)
    # Which gradients have bits to be identical to is a property of the kernels, not of one pair of runs: the PropMLP parameter gradients
    # are summed with float atomics (nlr_prop_mlp_bwd_param_kernel), in an order that changes from call to call - and a one-element
    # gradient such as density_layer.2.bias still repeats by chance in a few runs of ten; every other parameter gradient is summed in
    # a fixed order and must repeat
    atomic = [k for k in p0 if k.startswith("prop_mlp_")]
    repeatable = [k for k in p0 if k not in atomic]
    print(f"{sum(torch.equal(p0[k], p0b[k]) for k in p0)} of {len(p0)} parameter gradients repeat bit for bit between two plain steps")
    assert len(repeatable) > 0 and len(atomic) > 0
    for k in p0:
        if k in repeatable:
            assert torch.equal(p0[k], p0b[k]), k
            assert torch.equal(p0[k], p1[k]), k
        else:  # summed in an order that changes from call to call: the gate of the f32 backward kernels
            assert float((p0[k] - p1[k]).abs().max()) <= 2e-5 * float(p0[k].abs().max()) + float((p0[k] - p0b[k]).abs().max()), k
    assert all(with_grad[k].grad is not None and float(with_grad[k].grad.abs().max()) > 0 for k in RAY_GRAD_KEYS)
    # the dynamic-object branch is not wired to ray gradients
    from nerflidar_hip import config as ncfg
    mc = ncfg.workload("REF", 12)
    mc.config.instance_obj, mc.config.latent_size = True, 128
    mc.__post_init__()
    tracks = np.zeros((1, 2, 9), np.float32)
    tracks[:, :, 4:7], tracks[:, 1, 7] = 0.1, 1.0
    dyn = ntrain.TrainableModel(mc, tracks=tracks, class_names=["vehicle.car"], obj_log2_hashmap=12).cuda()
    with pytest.raises(NotImplementedError, match="box-frame"):
        dyn(dict(with_grad, timestamp=torch.zeros(batch["origins"].shape[0], device="cuda")), randomized=False)


# ---- GPU: it refines --------------------------------------------------------------------------------------------------------
REFINE_STEPS = 30


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
def test_pose_only_steps_reduce_the_pose_error(seed):
    """The trained field of tests/golden/ckpt_trained, frozen; 1024 analytic-scene LiDAR rays of 4 frames whose poses carry a seeded
    error; REFINE_STEPS pose-only steps of `training_step(posenet=..)`.  The hit-point error (scene.hit_point_error_m) after the
    steps is below the error before."""
    from nerflidar_hip import config as nconfig, scene as nscene
    dev = torch.device("cuda")
    sd, _ = nckpt.load_checkpoint(os.path.join(GOLDEN, "ckpt_trained"))
    sd, _ = nckpt.split_state_dict(sd)
    mc = nckpt.infer_model_config(sd, nconfig.workload("REFI", 13))
    tm = ntrain.TrainableModel(mc, fused_mlp=True).cuda().load_reference(sd)
    for p in tm.parameters():
        p.requires_grad_(False)
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros((), device=dev))], lr=0.0)   # nothing of the field steps
    true = nscene.supervise(nscene.random_lidar_rays(1024, seed, 1, dev, 0), 0)
    bad, r_true, t_true = nscene.perturb_frames(true, 4, seed)
    pn, pn_opt, lr_fn = ntrain.create_posenet(4, num_lidars=0, start_step=0, end_step=10 ** 6, pn_lr_init=2e-4, pn_lr_final=2e-4, t_ratio=1.0,
                                              lr_delay_steps=0)
    pn = pn.cuda()
    err = lambda: nscene.hit_point_error_m(ntrain.refine_batch(bad, pn(bad["glo_idx"])), true)
    with torch.no_grad():
        before = err()
        assert nscene.hit_point_error_m(ntrain.refine_batch(bad, nscene_true_pose(r_true, t_true, bad)), true) < 1e-3 * before
    for step in range(1, REFINE_STEPS + 1):
        out = ntrain.training_step(tm, opt, bad, randomized=False, hash_decay_mult=0.0, posenet=pn, pn_optimizer=pn_opt, pn_lr_fn=lr_fn, step=step,
                                   pose_window=(0, 10 ** 6), depth_lam=0.1, sem_lam=0.01, as_tensors=True)
    assert bool(torch.isfinite(out["loss"]))
    with torch.no_grad():
        after = err()
    _record(f"it refines, seed {seed}: {REFINE_STEPS} pose-only steps (Adam, lr 2e-4), hit-point error {before:.4f} m -> {after:.4f} m")
    assert after < before, (before, after)


def nscene_true_pose(r_true, t_true, bad):
    pn = ntrain.PoseNet(r_true.shape[0], num_lidars=0).cuda()
    with torch.no_grad():
        pn.r.copy_(r_true)
        pn.t.copy_(t_true)
    return pn(bad["glo_idx"])
