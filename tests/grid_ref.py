"""The float64 reference of the multiresolution grid lookup (CPU, torch autograd), shared by the tests of the fused encode
(test_pose_refine.py) and of the stand-alone grid operator (test_grid_envelope.py).  A plain module, not a test file."""
import numpy as np
import torch


def _level_table(enc):
    """Per level: scale (float32 arithmetic of the kernel's host side), step, table rows, hashed or not (gridencoder.cu:66-84,138-139)."""
    off = enc._offsets_host.numpy().astype(np.int64)
    S = np.float32(np.log2(enc.per_level_scale))
    out = []
    for l in range(enc.num_levels):
        scale = float(np.float32(np.exp2(np.float32(l) * S)) * np.float32(enc.base_resolution) - np.float32(1.0))
        step = int(np.ceil(scale)) + 1 + (0 if enc.align_corners else 1)
        hs = int(off[l + 1] - off[l])
        stride, dims = 1, 0
        while dims < 3 and stride <= hs:
            stride *= step
            dims += 1
        out.append((scale, step, hs, int(off[l]), stride > hs))
    return out


def _grid_lookup(x01, table, enc):
    """Differentiable (in x01) trilinear lookup on every level: [P, 3] -> [P, L, C] in x01's dtype; a point outside [0, 1]^3 gives
    zeros.  The cell index is taken from the values (no gradient), the weights carry the gradient."""
    P = x01.shape[0]
    oob = ((x01 < 0) | (x01 > 1)).any(-1)
    feats = []
    for scale, step, hs, off, hashed in _level_table(enc):
        pos = x01 * scale + (0.0 if enc.align_corners else 0.5)
        pg = torch.floor(pos.detach())
        fr = pos - pg
        if enc.interp_id == 1:
            fr = fr * fr * (3 - 2 * fr)
        pg = pg.long().clamp_min(0)
        acc = 0
        for c8 in range(8):
            w = torch.ones(P, dtype=x01.dtype)
            pl = []
            for d in range(3):
                bit = (c8 >> d) & 1
                w = w * (fr[:, d] if bit else 1 - fr[:, d])
                pl.append(pg[:, d] + bit)
            if hashed and enc.gridtype_id == 0:
                idx = (pl[0] ^ ((pl[1] * 2654435761) & 0xFFFFFFFF) ^ ((pl[2] * 805459861) & 0xFFFFFFFF)) & 0xFFFFFFFF
            else:
                idx, stride = torch.zeros(P, dtype=torch.long), 1
                for d in range(3):
                    if stride <= hs:
                        idx = idx + pl[d] * stride
                        stride *= step
            idx = torch.where(oob, torch.zeros_like(idx), idx % hs + off)
            acc = acc + w[:, None] * table[idx]
        feats.append(torch.where(oob[:, None], torch.zeros_like(acc), acc))
    return torch.stack(feats, 1)


class GridSpec:
    """The attributes `_level_table` / `_grid_lookup` read from an encoder, for a grid given by its numbers alone."""

    def __init__(self, offsets, per_level_scale, base_resolution, gridtype=0, align_corners=False, interp=0):
        self._offsets_host = torch.from_numpy(np.ascontiguousarray(offsets, np.int32))
        self.num_levels = len(offsets) - 1
        self.per_level_scale = per_level_scale
        self.base_resolution = base_resolution
        self.gridtype_id, self.align_corners, self.interp_id = int(gridtype), bool(align_corners), int(interp)


def _points(n, seed):
    """Uniform points of the unit cube behind a fixed edge set: the cube's corners and faces, a coordinate one ulp below a face, and
    two groups of out-of-range points."""
    rng = np.random.default_rng(seed)
    x = rng.random((n, 3)).astype(np.float32)
    x[:8] = np.array([[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [0, 1, 0.25], [1, 0, 0], [0.999999, 0.5, 0.5],
                      [1e-7, 1e-7, 1e-7], [0.25, 0.75, 1.0]], np.float32)
    x[8:12, 0] = 1.0001   # out of range -> zeros (gridencoder.cu:110-135)
    x[12:16, 2] = -1e-6
    return x


def level_plan(offsets, C, S, H, gridtype, align, B):
    """(mode, step, lds_kind) per level as the library decides them (`nlr_grid_level_plan`, host arithmetic only)."""
    from nerflidar_hip import _lib
    off = np.ascontiguousarray(offsets, np.int32)
    L = len(off) - 1
    mode, step, kind = (np.zeros(L, np.uint32) for _ in range(3))
    _lib.check(_lib.lib().nlr_grid_level_plan(off.ctypes.data, L, C, float(S), H, int(gridtype), int(align), B, mode.ctypes.data, step.ctypes.data,
                                              kind.ctypes.data))
    return mode.tolist(), step.tolist(), kind.tolist()
