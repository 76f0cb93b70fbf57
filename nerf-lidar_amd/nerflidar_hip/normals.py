"""Density normals: per-sample and rendered surface normals from the density field (header section 12, csrc/nlr_normals.hip).

The reference's `MLP.forward` with `disable_density_normals = False` and `analytic_gradient = True` (ZI/models.py:1075-1094)
differentiates the raw density with respect to the multisample positions, averages over the multisamples and takes
`normals = -l2_normalize(raw_grad_density)`; `Model.forward` composites them with the last level's weights (models.py:525-529,
render.py:255-261).  `density_normals` is that, after a render, on the level's `tdist` and `weights`.

No autograd: the outputs are plain tensors.  Training through normals (normal supervision, the orientation loss) needs the second
derivative of the grid and is not part of this module.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib

OUTPUTS = ("raw_grad", "normals", "ray_normals")
HIDDEN = 64  # width of density_layer.0 the cotangent kernel is built for
# The operator's workspace holds the features and their cotangent, 2 * 4 * S * L*C bytes per ray (164 KiB for the 128 samples x 40
# features of C2); rays are processed in chunks whose workspace stays under this budget, and the buffer is reused from chunk to chunk.
WORKSPACE_BUDGET_BYTES = 256 << 20


def workspace_bytes(n: int, S: int, F: int) -> int:
    """`nlr_density_normals_workspace_bytes`: features and cotangent, [n * S, F] f32 each."""
    return 2 * int(n) * int(S) * int(F) * 4


def rays_per_chunk(S: int, F: int, budget: int = WORKSPACE_BUDGET_BYTES) -> int:
    """The largest ray count whose workspace fits `budget` (at least 1), capped so that a chunk's sample index fits 32 bits."""
    per_ray = workspace_bytes(1, S, F)
    return max(1, min(budget // per_ray, ((1 << 32) - (1 << 21)) // (8 * max(int(S), 1))))


def grid_desc(encoder, table: torch.Tensor) -> "_lib.NlrGridDesc":
    """The NlrGridDesc of `encoder` (the duck type `training.encode_features_fused` accepts) over the device table `table`."""
    gd = _lib.NlrGridDesc()
    gd.table, gd.table_dtype = table.data_ptr(), {torch.float32: 0, torch.float16: 1}[table.dtype]
    gd.num_levels, gd.level_dim = int(encoder.num_levels), int(table.shape[1])
    gd.base_resolution = int(encoder.base_resolution)
    gd.log2_per_level_scale = float(np.log2(encoder.per_level_scale))
    gd.offsets = encoder._offsets_host.data_ptr()
    gd.gridtype, gd.align_corners, gd.interp = int(encoder.gridtype_id), int(bool(encoder.align_corners)), int(encoder.interp_id)
    return gd


@torch.no_grad()
def density_normals(encoder, batch: Dict[str, torch.Tensor], tdist: torch.Tensor, w0: torch.Tensor, b0: torch.Tensor, w2: torch.Tensor,
                    weights: Optional[torch.Tensor] = None, sample_n: int = 7, sample_m: int = 3, std_scale: float = 0.35,
                    rand_deg: Optional[torch.Tensor] = None, re_weights: bool = True, want: Sequence[str] = OUTPUTS,
                    workspace_budget: int = WORKSPACE_BUDGET_BYTES, return_features: bool = False) -> Dict[str, torch.Tensor]:
    """Normals of the samples of `tdist` [N, S+1] and of the rays.

    encoder: `num_levels, base_resolution, per_level_scale, _offsets_host, gridtype_id, align_corners, interp_id, embeddings` (a
    `gridencoder.GridEncoder`, or any object with these), the table a CUDA f32 / f16 tensor.  batch: the ray tensors of `_lib.RAY_KEYS`
    on the device.  w0 [64, F], b0 [64]: `density_layer.0`; w2: `density_layer.2.weight` [WB, 64] (row 0 is read) or that row [64].
    weights [N, S]: the level's compositing weights, needed for "ray_normals".  rand_deg [N, S, sample_n]: the draws the render used.
    want: which of "raw_grad" [N, S, 3], "normals" [N, S, 3], "ray_normals" [N, 3] to compute; the dict holds exactly these, float32.
    Values do not depend on what else is requested, on the chunking or on the run: every sum has a fixed order.
    return_features: also "features" [N, S, F], what the operator encoded (for tests)."""
    want = tuple(want)
    unknown = [k for k in want if k not in OUTPUTS]
    if unknown:
        raise ValueError(f"density_normals: want = {want!r}, the outputs are {OUTPUTS}")
    if "ray_normals" in want and weights is None:
        raise ValueError("density_normals: 'ray_normals' is the weighted sum over a ray's samples: pass the level's weights")
    table = encoder.embeddings.detach()
    if not (table.is_cuda and tdist.is_cuda):
        raise RuntimeError("density_normals: the table and tdist must be CUDA tensors (no CPU fallback)")
    table = table.contiguous()
    dev = table.device
    n, S = int(tdist.shape[0]), int(tdist.shape[1]) - 1
    F = int(encoder.num_levels) * int(table.shape[1])
    f32 = lambda t: t.detach().to(dev, torch.float32).contiguous()
    w0, b0 = f32(w0), f32(b0)
    w2 = f32(w2[0] if w2.dim() == 2 else w2)
    hidden = int(w0.shape[0])
    if w0.shape != (hidden, F) or b0.shape != (hidden,) or w2.shape != (hidden,):
        raise ValueError(f"density_normals: density_layer.0 {tuple(w0.shape)} / {tuple(b0.shape)} and row 0 of density_layer.2 {tuple(w2.shape)} "
                         f"do not fit {F} features")
    td = f32(tdist)
    wts = None if weights is None else f32(weights).reshape(n, S)
    rd = None if rand_deg is None else f32(rand_deg).reshape(n, S, sample_n)
    out = {k: torch.empty((n, 3) if k == "ray_normals" else (n, S, 3), device=dev, dtype=torch.float32) for k in want}
    feats = torch.empty(n, S, F, device=dev, dtype=torch.float32) if return_features else None
    gd = grid_desc(encoder, table)
    flat = {k: batch[k].reshape(n, -1) for k in _lib.RAY_KEYS if batch.get(k) is not None}
    chunk = rays_per_chunk(S, F, workspace_budget) if n else 1
    ws = torch.empty(workspace_bytes(min(chunk, n), S, F), dtype=torch.uint8, device=dev)
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        rays, keep = _lib.rays({k: v[a:b] for k, v in flat.items()}, b - a, optional=("viewdirs", "near", "far"))
        part = [out[k][a:b] if k in out else None for k in OUTPUTS]
        _lib.call("nlr_density_normals", rays, td[a:b], b - a, S, sample_n, sample_m, std_scale, None if rd is None else rd[a:b], gd,
                  int(bool(re_weights)), hidden, w0, b0, w2, None if wts is None else wts[a:b], *part, ws, workspace_bytes(b - a, S, F))
        if feats is not None:
            feats[a:b] = ws[:(b - a) * S * F * 4].view(torch.float32).reshape(b - a, S, F)
        del keep
    if feats is not None:
        out["features"] = feats
    return out
