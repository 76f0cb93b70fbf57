"""An analytic street scene and its LiDAR ground truth (supervision for `training.training_step`; no dataset ships with the reference).

The reference trains on nuScenes sweeps: per LiDAR ray a range, an intensity and a class id (ZI/datasets.py:640-705, keys `depth`,
`intensity`, `semantic`, `lidar_mask`).  This module supplies the same keys for rays cast into a closed analytic scene - a ground
plane with road / sidewalk / terrain bands, four boundary walls, and axis-aligned boxes standing in for cars, a truck, poles,
vegetation and building blocks - so that a model can be TRAINED in this image and the whole chain (train -> checkpoint in the
reference's format -> fused render) runs on a field that looks like the reference's use: smooth, concentrated density, not
white-noise tables.

Geometry is stated in metres in the SENSOR-aligned frame (z up, the frame `lidar.get_directions` builds directions in);
`lidar.synthetic_sweep` rotates directions by `lidar.seeded_rotation(seed)` and works in scene units (metres * scale_factor), so
`cast` takes the rotation and the scale.  Everything is torch and runs on whatever device the rays live on.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import lidar as nlidar
from . import synth

# class ids of the 19-class label space the reference's semantic head uses (Cityscapes train ids; sky = 10 and car = 13 are the
# two the ray-drop stage singles out, RD/drop_simulation_rays.py:120-150)
ROAD, SIDEWALK, BUILDING, WALL, POLE, VEGETATION, TERRAIN, CAR, TRUCK = 0, 1, 2, 3, 5, 8, 9, 13, 14

GROUND_Z = -6.2                       # below every sensor position: sweep origins move by up to 0.01 * sqrt(3) scene units = 4.3 m
WALL_X, WALL_Y = 60.0, 35.0           # boundary walls: the scene is closed, every ray returns
# boxes: (centre xyz, size xyz, class)
_BOXES = [
    ((8.0, 3.2, GROUND_Z + 0.8), (4.6, 1.9, 1.6), CAR),
    ((-12.0, -3.4, GROUND_Z + 0.8), (4.4, 1.8, 1.6), CAR),
    ((22.0, -3.0, GROUND_Z + 0.75), (4.5, 1.9, 1.5), CAR),
    ((-30.0, 3.1, GROUND_Z + 0.8), (4.7, 2.0, 1.6), CAR),
    ((35.0, 3.5, GROUND_Z + 1.7), (9.0, 2.6, 3.4), TRUCK),
    ((5.0, 9.5, GROUND_Z + 3.0), (0.4, 0.4, 6.0), POLE),
    ((-18.0, -9.5, GROUND_Z + 3.0), (0.4, 0.4, 6.0), POLE),
    ((28.0, 9.5, GROUND_Z + 3.0), (0.4, 0.4, 6.0), POLE),
    ((-6.0, 14.0, GROUND_Z + 2.0), (5.0, 4.0, 4.0), VEGETATION),
    ((16.0, -15.0, GROUND_Z + 2.5), (6.0, 5.0, 5.0), VEGETATION),
    ((-40.0, 22.0, GROUND_Z + 7.0), (18.0, 14.0, 14.0), BUILDING),
    ((30.0, -26.0, GROUND_Z + 5.0), (22.0, 12.0, 10.0), BUILDING),
    ((-8.0, 27.0, GROUND_Z + 6.0), (16.0, 10.0, 12.0), BUILDING),
]
# per class: LiDAR reflectivity and an albedo for the colour target
_REFLECT = {ROAD: 0.18, SIDEWALK: 0.32, BUILDING: 0.55, WALL: 0.45, POLE: 0.85, VEGETATION: 0.38, TERRAIN: 0.25, CAR: 0.7, TRUCK: 0.6}
_ALBEDO = {ROAD: (0.25, 0.25, 0.27), SIDEWALK: (0.55, 0.53, 0.5), BUILDING: (0.7, 0.6, 0.5), WALL: (0.6, 0.6, 0.62), POLE: (0.3, 0.3, 0.3),
           VEGETATION: (0.2, 0.5, 0.2), TERRAIN: (0.45, 0.5, 0.3), CAR: (0.7, 0.15, 0.15), TRUCK: (0.85, 0.85, 0.9)}


def _tables(device):
    refl = torch.zeros(19, device=device)
    alb = torch.zeros(19, 3, device=device)
    for k, v in _REFLECT.items():
        refl[k] = v
    for k, v in _ALBEDO.items():
        alb[k] = torch.tensor(v, device=device)
    return refl, alb


def cast(origins: torch.Tensor, directions: torch.Tensor, rotation=None, scale_factor: float = 1.0 / 250.0) -> Dict[str, torch.Tensor]:
    """First hit of every ray.  origins / directions [N,3] in scene units / the rotated frame of `lidar.synthetic_sweep`
    (`rotation` = `lidar.seeded_rotation(seed)`, None for the sensor frame itself).  Returns
    depth [N] (scene units along the unit direction: what `renderings[-1]['depth']` is compared with, train.py:334),
    semantic [N] int64, intensity [N] in [0, 1], rgb [N,3], normal [N,3] (sensor frame)."""
    dev = origins.device
    o = origins.double() / scale_factor
    d = directions.double()
    if rotation is not None:
        R = torch.as_tensor(np.asarray(rotation), dtype=torch.float64, device=dev)
        o, d = o @ R, d @ R                       # d_world = d_sensor @ R^T  =>  d_sensor = d_world @ R
    n = o.shape[0]
    inf = torch.full((n,), float("inf"), dtype=torch.float64, device=dev)
    best_t, best_cls = inf.clone(), torch.full((n,), -1, dtype=torch.int64, device=dev)
    best_n = torch.zeros(n, 3, dtype=torch.float64, device=dev)

    def take(t, cls, normal):
        nonlocal best_t, best_cls, best_n
        ok = (t > 1e-6) & (t < best_t)
        best_t = torch.where(ok, t, best_t)
        best_cls = torch.where(ok, cls if isinstance(cls, torch.Tensor) else torch.full_like(best_cls, cls), best_cls)
        best_n = torch.where(ok[:, None], normal, best_n)

    safe = lambda x: torch.where(x.abs() < 1e-12, torch.full_like(x, 1e-12), x)
    # ground: class by lateral band of the hit point
    tg = (GROUND_Z - o[:, 2]) / safe(d[:, 2])
    yg = (o[:, 1] + tg * d[:, 1]).abs()
    cls_g = torch.where(yg < 7.0, ROAD, torch.where(yg < 12.0, SIDEWALK, TERRAIN))
    take(tg, cls_g, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=dev).expand(n, 3))
    # boundary walls
    for axis, pos, cls in ((0, WALL_X, WALL), (0, -WALL_X, WALL), (1, WALL_Y, BUILDING), (1, -WALL_Y, BUILDING)):
        t = (pos - o[:, axis]) / safe(d[:, axis])
        nrm = torch.zeros(3, dtype=torch.float64, device=dev)
        nrm[axis] = -np.sign(pos)
        take(t, cls, nrm.expand(n, 3))
    # boxes: slab test, all boxes at once ([N, B, 3])
    key = str(dev)
    if key not in _BOX_T:
        _BOX_T[key] = (torch.tensor([b[0] for b in _BOXES], dtype=torch.float64, device=dev),
                       torch.tensor([b[1] for b in _BOXES], dtype=torch.float64, device=dev) / 2,
                       torch.tensor([b[2] for b in _BOXES], dtype=torch.int64, device=dev))
    bc, bh, bcls = _BOX_T[key]
    inv = (1.0 / safe(d))[:, None, :]
    t0, t1 = (bc - bh - o[:, None, :]) * inv, (bc + bh - o[:, None, :]) * inv
    tn, ax = torch.minimum(t0, t1).max(dim=2)                       # entry parameter and the axis of the face entered
    tf = torch.maximum(t0, t1).min(dim=2).values
    tn = torch.where((tn < tf) & (tn > 1e-6), tn, inf[:, None])
    tb, ib = tn.min(dim=1)                                           # nearest box per ray
    axb = torch.gather(ax, 1, ib[:, None])
    nrm = torch.zeros(n, 3, dtype=torch.float64, device=dev)
    nrm.scatter_(1, axb, -torch.sign(torch.gather(d, 1, axb)))
    take(tb, bcls[ib], nrm)
    assert bool((best_cls >= 0).all()), "the scene is closed: every ray must hit something"
    refl, alb = _tables(dev)
    cosi = (-(d / d.norm(dim=-1, keepdim=True)) * best_n).sum(-1).clamp(0.0, 1.0)
    shade = (0.4 + 0.6 * cosi).float()
    # the ray is o + t * d with d as given (the renderer's t runs along `directions`, unit or not): t in metres -> scene units
    return dict(depth=(best_t * scale_factor).float(), semantic=best_cls, intensity=refl[best_cls] * shade, rgb=alb[best_cls] * shade[:, None], normal=best_n.float())


_POSITIONS: Dict[tuple, tuple] = {}
_BOX_T: Dict[str, tuple] = {}


def random_lidar_rays(n: int, seed: int, step: int, device, rot_seed: int = 0, scale_factor: float = 1.0 / 250.0,
                      origin_range: float = 0.01) -> Dict[str, torch.Tensor]:
    """A training batch of `n` LiDAR rays with the batch contract of `lidar.cast_lidar_ray_batch` (ZI/lidar_utils.py:8-33, incl. the
    Frobenius-norm `viewdirs` and `base_x = base_y = directions`): origins drawn from the sensor positions of
    `lidar.synthetic_sweep(sweep_idx = 0..63)`, beams from the nuScenes table, azimuths uniform.  Built on `device` (a few small
    kernels; on the host the same arithmetic costs more than the training step).  Deterministic in (seed, step) per device type."""
    dev = torch.device(device)
    g = torch.Generator(device=dev).manual_seed(seed * 1000003 + step)
    key = (rot_seed, origin_range, str(dev))
    if key not in _POSITIONS:
        pos = np.stack([synth.uniform(rot_seed, 9100 + i, (3,), -origin_range, origin_range) for i in range(64)]).astype(np.float64)
        _POSITIONS[key] = (torch.from_numpy(pos).to(dev), torch.tensor(nlidar.LIDAR_ANGLES, dtype=torch.float64, device=dev) / 180 * np.pi,
                           torch.from_numpy(nlidar.seeded_rotation(rot_seed)).to(dev))
    pos, beams, R = _POSITIONS[key]
    o = pos[torch.randint(0, 64, (n,), generator=g, device=dev)]
    th = beams[torch.randint(0, 32, (n,), generator=g, device=dev)]
    ph = torch.rand(n, generator=g, dtype=torch.float64, device=dev) * 2 * np.pi
    d = torch.stack([torch.cos(th) * torch.sin(ph), torch.cos(th) * torch.cos(ph), torch.sin(th)], -1).float().double() @ R.T
    f32 = lambda t: t.float().contiguous()
    col = lambda v: torch.full((n, 1), float(v), device=dev)
    d32 = f32(d)
    return dict(origins=f32(o), directions=d32, viewdirs=f32(d / torch.linalg.norm(d)),  # Frobenius norm of the whole array (sic)
                radii=col(0.0005), imageplane=torch.zeros(n, 2, device=dev), lossmult=col(1.0), near=col(2.0 * scale_factor),
                far=col(500.0 * scale_factor), cam_idx=col(-1.0), base_x=d32, base_y=d32, rgb=torch.zeros(n, 3, device=dev),
                semantic=torch.full((n,), 255.0, device=dev), mask=torch.ones(n, device=dev))


def random_patch_rays(n_patches: int, patch_size: int, seed: int, step: int, device, rot_seed: int = 0, scale_factor: float = 1.0 / 250.0,
                      origin_range: float = 0.01, width: int = 1600, height: int = 900, focal: float = 1266.0) -> Dict[str, torch.Tensor]:
    """`n_patches` pixel patches of patch_size x patch_size pinhole rays (`camera.pixels_to_rays`, ZI/camera_utils.py:454-564) into the
    scene, flattened patch-major as the reference's loader does (datasets.py:357-399): row (p * s + i) * s + j is the pixel in row i,
    column j of patch p.  Per patch a camera at one of the sensor positions of `random_lidar_rays`, level, with a random heading, and a
    random patch of its width x height image (the nuScenes camera's 1600 x 900 at f = 1266).  Same keys as `random_lidar_rays`, so the
    two concatenate; `supervise(.., patch_rows=)` gives the rows their colours from `cast`.  Deterministic in (seed, step)."""
    from . import camera as ncamera
    s = int(patch_size)
    if n_patches < 1 or s < 2 or s > min(width, height):
        raise ValueError(f"random_patch_rays: {n_patches} patches of size {s} in a {width} x {height} image")
    dev = torch.device(device)
    rng = np.random.default_rng([seed, step, 0x9A7C])
    pos = np.stack([synth.uniform(rot_seed, 9100 + i, (3,), -origin_range, origin_range) for i in range(64)]).astype(np.float64)
    R = nlidar.seeded_rotation(rot_seed)
    pixtocam = np.linalg.inv(np.array([[focal, 0, width / 2], [0, focal, height / 2], [0, 0, 1.0]]))
    jj, ii = np.meshgrid(np.arange(s), np.arange(s), indexing="xy")       # jj: column (x), ii: row (y); row-major = i * s + j
    parts = []
    for _ in range(n_patches):
        yaw = rng.uniform(0, 2 * np.pi)
        fwd, up = np.array([np.sin(yaw), np.cos(yaw), 0.0]), np.array([0.0, 0.0, 1.0])
        c2w = np.concatenate([R @ np.stack([np.cross(fwd, up), up, -fwd], axis=1), pos[rng.integers(64)][:, None]], axis=1)  # OpenGL camera: looks along -z
        x0, y0 = rng.integers(0, width - s + 1), rng.integers(0, height - s + 1)
        parts.append(ncamera.pixels_to_rays((x0 + jj).reshape(-1).astype(np.float64), (y0 + ii).reshape(-1).astype(np.float64), pixtocam, c2w))
    o, d, v, r, ip, bx, by = (np.concatenate([p[k] for p in parts], axis=0) for k in range(7))
    n = o.shape[0]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    col = lambda val: torch.full((n, 1), float(val), device=dev)
    return dict(origins=t(o), directions=t(d), viewdirs=t(v), radii=t(r), imageplane=t(ip), lossmult=col(1.0), near=col(2.0 * scale_factor),
                far=col(500.0 * scale_factor), cam_idx=col(0.0), base_x=t(bx), base_y=t(by), rgb=torch.zeros(n, 3, device=dev),
                semantic=torch.full((n,), 255.0, device=dev), mask=torch.ones(n, device=dev))


def supervise(batch: Dict[str, torch.Tensor], rot_seed: int = 0, scale_factor: float = 1.0 / 250.0, colourless: int = 0,
              patch_rows: Optional[Sequence[int]] = None) -> Dict[str, torch.Tensor]:
    """Adds the supervision keys train.py:283-424 reads for LiDAR rays (`rgb`, `depth`, `semantic`, `intensity`, and the masks
    `losses.total_loss` takes) to a ray batch, from the analytic scene.  colourless: the last that many rays get `mask_rgb` =
    `sem_mask` = False, as train.py:316-320 sets them for the LiDAR rays at the end of a mixed batch (depth and intensity stay
    supervised); pass `color_rays = N - colourless` to `training.training_step` with such a batch.
    patch_rows = (row0, n): these rows are patch rays (`random_patch_rays`): every mask is False on them, as train.py:310-314 takes
    `patch_mask == 1` out of the colour, depth and semantic masks and they are no LiDAR rays; their `rgb` is what the smoothness terms
    weigh edges with (`losses.total_loss(patch_size=, patch_rays=)`)."""
    n = batch["origins"].shape[0]
    gt = cast(batch["origins"].reshape(n, 3), batch["directions"].reshape(n, 3), nlidar.seeded_rotation(rot_seed), scale_factor)
    out = dict(batch)
    ones = torch.ones(n, dtype=torch.bool, device=gt["depth"].device)
    out.update(rgb=gt["rgb"], depth=gt["depth"], semantic=gt["semantic"], intensity=gt["intensity"], mask_rgb=ones, depth_mask=ones,
               sem_mask=ones, lidar_mask=ones)
    if colourless:
        if not 0 <= colourless <= n:
            raise ValueError(f"colourless must lie in [0, {n}], got {colourless}")
        keep = torch.arange(n, device=ones.device) < n - colourless
        out.update(mask_rgb=keep, sem_mask=keep)
    if patch_rows is not None:
        row0, rows = int(patch_rows[0]), int(patch_rows[1])
        if not 0 <= row0 <= row0 + rows <= n:
            raise ValueError(f"patch_rows = ({row0}, {rows}) outside the {n} rays")
        idx = torch.arange(n, device=ones.device)
        keep = (idx < row0) | (idx >= row0 + rows)
        out.update({k: out[k] & keep for k in ("mask_rgb", "depth_mask", "sem_mask", "lidar_mask")})
    return out


def perturb_frames(batch: Dict[str, torch.Tensor], n_frames: int, seed: int, rot: float = 0.01, trans: float = 0.002):
    """Gives the rays of `batch` to `n_frames` frames (ray i belongs to frame i mod n_frames: `glo_idx`) and moves every frame by
    a seeded pose error: a rotation of up to `rot` rad per axis-angle component and a translation of up to `trans` scene units per
    axis.  Returns (perturbed batch, r_true [n_frames, 3], t_true [n_frames, 3]): the correction a `training.PoseNet` with t_ratio
    = 1 has to learn, i.e. `training.refine_batch(perturbed, pose(r_true, t_true))` gives the rays of `batch` back.  Supervision keys
    stay with their rays."""
    from .training import PoseNet, POSE_RAY_KEYS
    dev = batch["origins"].device
    n = batch["origins"].shape[0]
    true = PoseNet(n_frames, num_lidars=0)
    with torch.no_grad():
        true.r.copy_(torch.from_numpy(synth.uniform(seed, 9400, (n_frames, 3), -rot, rot)))
        true.t.copy_(torch.from_numpy(synth.uniform(seed, 9401, (n_frames, 3), -trans, trans)))
        ids = torch.arange(n) % n_frames
        P = true(ids).to(dev)
        out = dict(batch)
        out["origins"] = batch["origins"].reshape(n, 3) - P[:, :3, 3]
        for k in POSE_RAY_KEYS[1:] + ("viewdirs",):                      # v = R^T v_true
            out[k] = (batch[k].reshape(n, 3, 1) * P[:, :3, :3]).sum(1)
        out["glo_idx"] = ids.float()[:, None].to(dev)
    return out, true.r.detach().clone(), true.t.detach().clone()


def hit_point_error_m(refined: Dict[str, torch.Tensor], true: Dict[str, torch.Tensor], scale_factor: float = 1.0 / 250.0) -> float:
    """Mean distance in metres between where the rays of `refined` and the rays of `true` put their supervised depth: the pose error
    as the scene sees it (rotation and translation in one unit)."""
    n = true["origins"].shape[0]
    hit = lambda b: b["origins"].reshape(n, 3) + true["depth"].reshape(n, 1) * b["directions"].reshape(n, 3)
    return float((hit(refined) - hit(true)).norm(dim=-1).mean() / scale_factor)
