"""Training on the fused path (scope row f-3): the operators with HIP backward kernels and the modules that chain them.

  * differentiable compositing (`nlr_composite_level` / `nlr_composite_backward`) and the hash-decay regulariser;
  * the edge-aware smoothness terms of the patch rays (`nlr_patch_smooth_forward` / `_backward`, `patch_smooth`);
  * the two losses that read the ray history, anti-aliased interlevel and distortion (`nlr_ray_losses_forward` / `_backward`, `ray_losses`);
  * `gridencoder.GridEncoder` (HIP forward + backward + total-variation gradient, Z/gridencoder/grid.py:24-198);
  * the NerfMLP either as torch Linear modules or through the fused MFMA forward / backward (`_FusedMLP`);
  * `TrainableNerfLevel`, `TrainablePropLevel`, `TrainableModel`: the reference's `Model.forward` with autograd (proposal
    resampling carries no gradient in the reference either, `Model.stop_level_grad`), and `training_step`: the step of
    ZI/train.py:272-459 with the loss dictionary of `nerflidar_hip.losses`.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .config import obj_mlp_config
from .gridencoder import GridEncoder
from .objects import _pos_enc, box_frame, check_instance_obj, obj_mlp_forward, query_class, track_box_params, view_mlp


class _Composite(torch.autograd.Function):
    """compute_alpha_weights + volumetric_rendering (ZI/render.py:170-252): nlr_composite_level forward,
    nlr_composite_backward backward.  Per-sample inputs in the reference's layout ([N,S,3], [N,S,K], [N,S])."""

    @staticmethod
    def forward(ctx, density, tdist, dirs, rgbs, semantic, intensity, opaque_background, bg):
        n, S = density.shape
        dev, f32 = density.device, torch.float32
        d = density.contiguous().float()
        td = tdist.contiguous().float()
        dr = dirs.contiguous().float()
        rgb_cm = rgbs.permute(2, 0, 1).contiguous().float() if rgbs is not None else None       # [3,N,S]
        sem_cm = semantic.permute(2, 0, 1).contiguous().float() if semantic is not None else None  # [K,N,S]
        it = intensity.reshape(n, S).contiguous().float() if intensity is not None else None
        K = 0 if semantic is None else semantic.shape[-1]
        out = _lib.NlrOut()
        res = {"rgb": torch.empty(n, 3, device=dev), "depth": torch.empty(n, device=dev), "acc": torch.empty(n, device=dev)}
        if K:
            res["semantic"] = torch.empty(n, K, device=dev)
        if it is not None:
            res["intensity"] = torch.empty(n, device=dev)
        for k, t in res.items():
            setattr(out, k, t.data_ptr())
        weights = torch.empty(n, S, device=dev)
        _lib.call("nlr_composite_level", d, td, dr, rgb_cm, sem_cm, it, None, None, n, S, K, opaque_background, bg, 0, 0.0, weights, out, None)
        ctx.save_for_backward(d, td, dr, rgb_cm, sem_cm, it)
        ctx.meta = (n, S, K, int(opaque_background), float(bg))
        sem_out = res.get("semantic", torch.zeros(n, 0, device=dev))
        int_out = res.get("intensity", torch.zeros(0, device=dev))
        return res["rgb"], res["depth"], sem_out, int_out, res["acc"], weights

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_sem, g_int, g_acc, g_w):
        d, td, dr, rgb_cm, sem_cm, it = ctx.saved_tensors
        n, S, K, opaque, bg = ctx.meta
        dev = d.device
        c = lambda t: None if t is None else t.contiguous().float()
        g_rgb, g_depth, g_acc, g_w = c(g_rgb), c(g_depth), c(g_acc), c(g_w)
        g_sem = c(g_sem) if K else None
        g_int = c(g_int) if it is not None else None
        dd = torch.empty(n, S, device=dev)
        d_rgb = torch.empty(3, n, S, device=dev) if rgb_cm is not None else None
        d_sem = torch.empty(K, n, S, device=dev) if K else None
        d_int = torch.empty(n, S, device=dev) if it is not None else None
        _lib.call("nlr_composite_backward", d, td, dr, rgb_cm, sem_cm, it, n, S, K, opaque, bg, g_rgb, g_depth, g_sem, g_int, g_acc, g_w, dd,
                  d_rgb, d_sem, d_int)
        d_dirs = None
        if ctx.needs_input_grad[2]:
            # dirs enters as |d| in density * dt * |d| only (render.py:176-178): dL/d|d| = sum_s dd_s density_s / |d|, d|d|/dd = d / |d|
            d_dirs = dr * ((dd * d).sum(-1) / (dr * dr).sum(-1))[:, None]
        return (dd, None, d_dirs, None if d_rgb is None else d_rgb.permute(1, 2, 0), None if d_sem is None else d_sem.permute(1, 2, 0), d_int,
                None, None)


def volumetric_render(density, tdist, dirs, rgbs, semantic=None, intensity=None, opaque_background=True, bg=1.0) -> Dict[str, torch.Tensor]:
    """Differentiable `weights = compute_alpha_weights(...)`, `volumetric_rendering(...)` with the reference's keys
    (`rgb`, `depth`, `semantic`, `intensity`, `acc`) plus `weights` [N,S].  Gradients: density, rgbs, semantic, intensity, and
    `dirs` when it requires one (pose refinement), computed from the density gradient the backward kernel returns."""
    rgb, depth, sem, inten, acc, w = _Composite.apply(density, tdist, dirs, rgbs, semantic, intensity, opaque_background, bg)
    out = {"rgb": rgb, "depth": depth, "acc": acc, "weights": w}
    if semantic is not None:
        out["semantic"] = sem
    if intensity is not None:
        out["intensity"] = inten
    return out


class _HashDecay(torch.autograd.Function):
    _rows: Dict = {}

    @staticmethod
    def forward(ctx, embeddings, offsets_host):
        e = embeddings.contiguous().float()
        off = np.ascontiguousarray(np.asarray(offsets_host, np.int32))
        L, Cc = len(off) - 1, e.shape[1]
        ss = torch.empty(L, dtype=torch.float64, device=e.device)
        _lib.call("nlr_hash_decay_forward", e, off, L, Cc, ss)
        key = (off.tobytes(), e.device)
        rows = _HashDecay._rows.get(key)                                   # (uploaded once: a host copy per step is a synchronisation)
        if rows is None:
            rows = _HashDecay._rows[key] = torch.from_numpy(np.diff(off).astype(np.float64)).to(e.device)
        ctx.save_for_backward(e)
        ctx.off = off
        return (ss / rows.clamp_min(1)).sum().div(L * Cc).float()

    @staticmethod
    def backward(ctx, g):
        (e,) = ctx.saved_tensors
        off = ctx.off
        grad = torch.zeros_like(e)
        _lib.call("nlr_hash_decay_backward", e, off, len(off) - 1, e.shape[1], 1.0, grad)
        return grad.mul_(g), None   # (the upstream scalar stays on the device: float(g) would be a host read in every step)


def hash_decay_loss(encoders, mult: float = 1.0) -> torch.Tensor:
    """ZI/models.py:203-223 over `nerflidar_hip.gridencoder.GridEncoder` modules (static field; `Config.obj_nodecay` keeps the
    object grids out): mult * sum_enc mean_{level,channel} mean_{rows of level} embeddings^2."""
    total = None
    for enc in encoders:
        l = _HashDecay.apply(enc.embeddings, enc._offsets_host)
        total = l if total is None else total + l
    return mult * total


class _PatchSmooth(torch.autograd.Function):
    """nlr_patch_smooth_forward / _backward: the edge-aware smoothness terms of the patch rays (ZI/train.py:365-388) as one operator.
    Returns terms [2] = (T_d, T_s); gradients to depth and semantic, rgb and valid are data.  Nothing of size [P, s, s, K] is kept
    between the passes besides the inputs themselves, and the upstream gradient stays on the device."""
    _workspaces: Dict = {}  # device -> uint8 tensor, grown on demand (only the forward writes it, and reads it back in the same call)

    @staticmethod
    def _workspace(dev, P, K):
        need = int(_lib.lib().nlr_patch_smooth_workspace_bytes(P, K))
        ws = _PatchSmooth._workspaces.get(dev)
        if ws is None or ws.numel() < need:
            ws = _PatchSmooth._workspaces[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
        return ws

    @staticmethod
    def forward(ctx, depth, semantic, rgb, valid, s):
        d = depth.reshape(-1).contiguous().float()
        P = d.numel() // (s * s)
        sem = None if semantic is None else semantic.reshape(d.numel(), -1).contiguous().float()
        K = 1 if sem is None else sem.shape[1]
        c = rgb.reshape(d.numel(), 3).contiguous().float()
        v = None if valid is None else valid.reshape(-1).contiguous().float()
        terms, stats = torch.empty(2, device=d.device), torch.empty(8, device=d.device)
        ws = _PatchSmooth._workspace(d.device, P, K)
        _lib.call("nlr_patch_smooth_forward", d, sem, c, v, P, s, K, terms, stats, ws, ws.numel())
        ctx.save_for_backward(d, sem, c, v, stats)
        ctx.meta = (P, s, K, depth.shape, None if semantic is None else semantic.shape)
        return terms

    @staticmethod
    def backward(ctx, g_terms):
        d, sem, c, v, stats = ctx.saved_tensors
        P, s, K, d_shape, sem_shape = ctx.meta
        d_depth = torch.empty_like(d)
        d_sem = None if sem is None else torch.empty_like(sem)
        ws = _PatchSmooth._workspace(d.device, P, K)
        _lib.call("nlr_patch_smooth_backward", d, sem, c, v, P, s, K, stats, g_terms.contiguous().float(), d_depth, d_sem, ws, ws.numel())
        return d_depth.reshape(d_shape), None if d_sem is None else d_sem.reshape(sem_shape), None, None, None


def patch_smooth(depth, semantic, rgb, valid, patch_size: int):
    """(T_d, T_s) of `losses.patch_smoothness` on the HIP operator: float32 CUDA tensors, rows patch-major; semantic / valid may be
    None (T_s is then a constant 0).  The refusals are the library's (2 <= patch_size <= 64, at most 32 classes)."""
    terms = _PatchSmooth.apply(depth, semantic, rgb, valid, int(patch_size))
    return terms[0], terms[1]


class _RayLosses(torch.autograd.Function):
    """nlr_ray_losses_forward / _backward (header section 11): the distortion loss of the final level and the anti-aliased interlevel
    loss of every proposal level as one operator.  Arguments: pulse_width, final sdist, final weights, then (sdist, weights, obj_mask or
    None) per proposal level.  Returns terms [1 + n_prop] = (distortion, anti term of level 0, ..); gradients to the weights, every
    sdist and mask is data.  Between the passes it keeps w_target [N, S_i] per level and the counts; the upstream gradient stays on the
    device."""
    _workspaces: Dict = {}  # device -> uint8 tensor, grown on demand (only the forward writes it, and reads it back in the same call)

    @staticmethod
    def _workspace(dev, N, n_prop):
        need = int(_lib.lib().nlr_ray_losses_workspace_bytes(N, n_prop))
        ws = _RayLosses._workspaces.get(dev)
        if ws is None or ws.numel() < need:
            ws = _RayLosses._workspaces[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
        return ws

    @staticmethod
    def _args(sd, w, psd, pw, pm, pulse_width):
        N, S, n_prop = w.shape[0], w.shape[1], len(pw)
        mask_ptrs = (C.c_void_p * n_prop)(*[None if m is None else m.data_ptr() for m in pm]) if n_prop else None
        prop_S = np.asarray([p.shape[1] for p in pw], np.int32) if n_prop else None
        widths = np.asarray([float(r) for r in pulse_width[:n_prop]], np.float32) if n_prop else None
        return (sd, w, N, S, _ptr_array(psd) if n_prop else None, _ptr_array(pw) if n_prop else None, mask_ptrs, prop_S, widths, n_prop)

    @staticmethod
    def forward(ctx, pulse_width, sdist, weights, *levels):
        n_prop = len(levels) // 3
        if len(pulse_width) < n_prop:
            raise ValueError(f"ray_losses: {n_prop} proposal levels, {len(pulse_width)} pulse widths")
        rows = lambda t: t.reshape(-1, t.shape[-1]).contiguous().float()
        sd, w = rows(sdist), rows(weights)
        psd = [rows(t) for t in levels[0::3]]
        pw = [rows(t) for t in levels[1::3]]
        pm = [None if m is None else m.reshape(-1, m.shape[-1]).to(torch.bool).contiguous().view(torch.uint8) for m in levels[2::3]]  # bool: its bytes
        N, dev = w.shape[0], w.device
        for name, a, b in [("final", sd, w)] + [(f"proposal {i}", a, b) for i, (a, b) in enumerate(zip(psd, pw))]:
            if a.shape != (N, b.shape[1] + 1) or b.shape[0] != N:
                raise ValueError(f"ray_losses: {name} level has sdist {tuple(a.shape)} and weights {tuple(b.shape)} for {N} rays")
        for i, (m, b) in enumerate(zip(pm, pw)):
            if m is not None and m.shape != b.shape:
                raise ValueError(f"ray_losses: obj_mask of proposal {i} is {tuple(m.shape)}, its weights {tuple(b.shape)}")
        terms, stats = torch.empty(1 + n_prop, device=dev), torch.empty(2 * (1 + n_prop), device=dev)
        w_target = [torch.empty_like(p) for p in pw]
        ws = _RayLosses._workspace(dev, N, n_prop)
        args = _RayLosses._args(sd, w, psd, pw, pm, pulse_width)
        _lib.call("nlr_ray_losses_forward", *args, terms, stats, _ptr_array(w_target) if n_prop else None, ws, ws.numel())
        ctx.save_for_backward(sd, w, stats, *psd, *pw, *w_target, *[m for m in pm if m is not None])
        ctx.meta = (n_prop, tuple(pulse_width), [m is not None for m in pm], weights.shape, [t.shape for t in levels[1::3]])
        return terms

    @staticmethod
    def backward(ctx, g_terms):
        n_prop, pulse_width, has_mask, w_shape, pw_shapes = ctx.meta
        sd, w, stats, *rest = ctx.saved_tensors
        psd, pw, w_target, masks = rest[:n_prop], rest[n_prop:2 * n_prop], rest[2 * n_prop:3 * n_prop], list(rest[3 * n_prop:])
        pm = [masks.pop(0) if h else None for h in has_mask]
        d_w, d_pw = torch.empty_like(w), [torch.empty_like(p) for p in pw]
        ws = _RayLosses._workspace(w.device, w.shape[0], n_prop)
        args = _RayLosses._args(sd, w, psd, pw, pm, pulse_width)
        _lib.call("nlr_ray_losses_backward", *args, stats, g_terms.contiguous().float(), _ptr_array(w_target) if n_prop else None, d_w,
                  _ptr_array(d_pw) if n_prop else None, ws, ws.numel())
        out = [None, None, d_w.reshape(w_shape)]
        for d, shape in zip(d_pw, pw_shapes):
            out += [None, d.reshape(shape), None]
        return tuple(out)


def ray_losses(ray_history, pulse_width):
    """terms [1 + n_prop] on the device = (distortion loss, anti-aliased interlevel loss of every proposal level), unscaled, of a ray
    history (dicts with `sdist`, `weights` and optionally `obj_mask`; the last one is the final level) on the HIP operator: float32
    CUDA tensors.  Every `sdist` is data: one that requires a gradient is refused.  The refusals of the sizes are the library's
    (at most 4 proposal levels, 512 samples per level, pulse widths finite and > 0)."""
    if any(h["sdist"].requires_grad for h in ray_history):
        raise ValueError("ray_losses: an sdist of the ray history requires a gradient; the operator treats sdist as data (detach it)")
    levels = []
    for h in ray_history[:-1]:
        levels += [h["sdist"], h["weights"], h.get("obj_mask")]
    return _RayLosses.apply(tuple(pulse_width), ray_history[-1]["sdist"], ray_history[-1]["weights"], *levels)


# ---- a trainable NerfMLP level: fused cast/contract + HIP grid op (fwd/bwd) + torch Linear stack + HIP compositing (fwd/bwd) ----------
def cast_contract(batch: Dict[str, torch.Tensor], tdist: torch.Tensor, sample_n: int = 7, sample_m: int = 3, std_scale: float = 0.35,
                  rand_deg: Optional[torch.Tensor] = None):
    """Rows a-5 + a-6 (`nlr_cast_contract`): multisample means / bound [N,S,n,3] and stds / bound [N,S,n] of the intervals of
    `tdist`, as MLP.predict_density feeds them to the encoder (ZI/models.py:965-973).  Carries no gradient (tdist is detached in
    training, Model.stop_level_grad)."""
    n, S = tdist.shape[0], tdist.shape[1] - 1
    dev = tdist.device
    rays, keep = _lib.rays(batch, n)
    td = tdist.detach().contiguous().float()
    means = torch.empty(n, S, sample_n, 3, device=dev)
    stds = torch.empty(n, S, sample_n, device=dev)
    rd = None if rand_deg is None else rand_deg.reshape(n, S, sample_n).contiguous().float()   # U[0,1) draws, render.py:150
    _lib.call("nlr_cast_contract", rays, td, n, S, sample_n, sample_m, std_scale, rd, means, stds)
    return means, stds


def encode_features(encoder, means: torch.Tensor, stds: torch.Tensor, re_weights: bool = True) -> torch.Tensor:
    """ZI/models.py:974-979: grid features of every multisample, erf down-weighting by footprint, mean over the multisamples.
    Differentiable with respect to `encoder.embeddings` through the HIP grid operator's backward."""
    L = encoder.num_levels
    f = encoder(means.reshape(-1, 3), bound=1).reshape(means.shape[:-1] + (L, -1))          # [N,S,n,L,C]
    if re_weights:
        gs = encoder.grid_sizes.to(means.device).float()
        w = torch.erf(1 / torch.clamp(torch.sqrt(8 * stds[..., None] ** 2 * gs ** 2), min=1e-10))
        f = (f * w[..., None]).mean(dim=-3)
    else:
        f = f.mean(dim=-3) if f.dim() > 3 else f
    return f.flatten(-2, -1)


class _EncodeFeatures(torch.autograd.Function):
    """cast_rays -> contraction -> GridEncoder -> erf re-weighting -> mean over the multisamples (ZI/models.py:965-979) as one
    operator: `nlr_encode_features_forward` (the fused kernel of the inference path) and `nlr_encode_features_backward`
    (per-point feature gradients in one kernel, then the grid operator's scatter).  Differentiable with respect to the table, and -
    when `encode_features_fused` hands over `rays` = the batch's origins, directions, base_x, base_y because one of them requires a
    gradient (pose refinement) - with respect to those four through `nlr_encode_features_backward_rays`.  tdist carries no gradient
    in training (`Model.stop_level_grad`)."""

    @staticmethod
    def forward(ctx, table, encoder, batch, tdist, sample_n, sample_m, std_scale, rand_deg, re_weights, *rays):
        n, S = tdist.shape[0], tdist.shape[1] - 1
        dev = tdist.device
        if not table.is_cuda:  # (the table travels inside NlrGridDesc, where `call` does not look)
            raise RuntimeError("encode_features: the table must be a CUDA tensor (no CPU fallback)")
        rays_desc, keep = _lib.rays(batch, n)
        td = tdist.detach().contiguous().float()
        rd = None if rand_deg is None else rand_deg.reshape(n, S, sample_n).contiguous().float()
        tab = table.detach().contiguous()
        ctx.args = (encoder, rays_desc, keep, td, rd, int(sample_n), int(sample_m), float(std_scale), int(bool(re_weights)))
        ctx.save_for_backward(tab)
        ctx.ray_shapes = [(t.shape, t.dtype) for t in rays]
        feats = torch.empty(n * S, encoder.output_dim, device=dev)
        _lib.call("nlr_encode_features_forward", rays_desc, td, n, S, sample_n, sample_m, std_scale, rd, _EncodeFeatures._descs(encoder, tab),
                  bool(re_weights), feats)
        return feats.reshape(n, S, encoder.output_dim)

    @staticmethod
    def _descs(encoder, tab):
        """The NlrGridDesc of `encoder` over the table `tab` (the ray half is `_lib.rays`)."""
        gd = _lib.NlrGridDesc()
        gd.table, gd.table_dtype = tab.data_ptr(), {torch.float32: 0, torch.float16: 1}[tab.dtype]
        gd.num_levels, gd.level_dim = encoder.num_levels, tab.shape[1]
        gd.base_resolution = int(encoder.base_resolution)
        gd.log2_per_level_scale = float(np.log2(encoder.per_level_scale))
        gd.offsets = encoder._offsets_host.data_ptr()
        gd.gridtype, gd.align_corners, gd.interp = encoder.gridtype_id, int(bool(encoder.align_corners)), encoder.interp_id
        return gd

    @staticmethod
    def backward(ctx, g):
        (tab,) = ctx.saved_tensors
        encoder, rays, _keep, td, rd, sample_n, sample_m, std_scale, re_w = ctx.args
        n, S = td.shape[0], td.shape[1] - 1
        g = g.reshape(n * S, -1).contiguous().float()
        gd = _EncodeFeatures._descs(encoder, tab)
        d_table = None
        if not ctx.ray_shapes or ctx.needs_input_grad[0]:  # (with rays: skipped when the table wants none - pose-only steps on a frozen field)
            grad = torch.zeros(tab.shape, device=tab.device, dtype=torch.float32)
            pts = torch.empty(n * S * sample_n, 3, device=tab.device)                      # scratch: unit-cube positions of the multisamples
            gpt = torch.empty(n * S * sample_n, encoder.output_dim, device=tab.device)     # scratch: their feature gradients
            from .gridencoder import backward_workspace
            ws = backward_workspace(n * S * sample_n, tab.shape[1], encoder.num_levels, float(np.log2(encoder.per_level_scale)),
                                    int(encoder.base_resolution), encoder._offsets_host, encoder.gridtype_id, encoder.align_corners, tab.device)
            _lib.call("nlr_encode_features_backward_ws", rays, td, n, S, sample_n, sample_m, std_scale, rd, gd, re_w, g, pts, gpt, grad, ws,
                      0 if ws is None else ws.numel())
            d_table = grad.to(tab.dtype)
        if not ctx.ray_shapes:
            return (d_table,) + (None,) * 8
        if not any(ctx.needs_input_grad[9:13]):  # (the batch's viewdirs alone require a gradient)
            return (d_table,) + (None,) * 12
        d_rays = [torch.empty(n, 3, device=tab.device) if w else None for w in ctx.needs_input_grad[9:13]]
        _lib.call("nlr_encode_features_backward_rays", rays, td, n, S, sample_n, sample_m, std_scale, rd, gd, re_w, g, *d_rays)
        return (d_table,) + (None,) * 8 + tuple(None if t is None else t.reshape(shape).to(dtype) for t, (shape, dtype) in zip(d_rays, ctx.ray_shapes))


def encode_features_fused(encoder, batch, tdist, sample_n: int = 7, sample_m: int = 3, std_scale: float = 0.35, rand_deg=None,
                          re_weights: bool = True) -> torch.Tensor:
    """[N, S, L*C] features of the intervals of `tdist`: `cast_contract` + `encode_features` in one kernel each way.  Ray tensors
    that require a gradient (`rays_require_grad`) get one; otherwise the calls are the ones of a batch of plain data."""
    rays = tuple(batch[k] for k in POSE_RAY_KEYS) if rays_require_grad(batch) else ()
    return _EncodeFeatures.apply(encoder.embeddings, encoder, batch, tdist, sample_n, sample_m, std_scale, rand_deg, re_weights, *rays)


POSE_RAY_KEYS = ("origins", "directions", "base_x", "base_y")  # what the encode's ray gradient reaches (viewdirs: the view MLP's input)


def rays_require_grad(batch) -> bool:
    """Does the loss have to reach the batch's ray tensors (pose refinement, train.py:207-221)?"""
    return torch.is_grad_enabled() and any(isinstance(batch.get(k), torch.Tensor) and batch[k].requires_grad for k in POSE_RAY_KEYS + ("viewdirs",))


# ---- fused NerfMLP for training: nlr_mlp_train_forward / nlr_mlp_train_backward (csrc/nlr_mlp_train.hip) ---------------------------
def _check_color_rays(color_rays, n: int) -> Optional[int]:
    """`color_rays` of `TrainableNerfLevel.forward`: None, or an integer 0 <= color_rays <= n (the number of rays)."""
    if color_rays is None:
        return None
    if isinstance(color_rays, bool) or not isinstance(color_rays, (int, np.integer)) or not 0 <= int(color_rays) <= n:
        raise ValueError(f"color_rays must be None or an integer in [0, {n}] (the rays [color_rays, {n}) carry no colour supervision), "
                         f"got {color_rays!r}")
    return int(color_rays)


def _wgrad_bmm(level, M, f, e, acts, gacts, M_color=None):
    """The weight and bias gradients of the fused NerfMLP as split-K library GEMMs over the tensors the kernels saved: the list
    [dW, db, dW, db, ..] in the order of `TrainableNerfLevel._mlp_params`.  `_FusedMLP.backward` without `fused_wgrad` and
    `scripts/wgrad_bench.py` call this same code.  M_color (rows, None = M): the view layers and rgb_layer reduce over the first
    M_color rows only - the split kernels leave their columns of the later rows unwritten."""
    plan, dev = level._plan, f.device
    # the input blocks of the plan's layer table: columns of acts, the grid features, the direction encoding of the sample's ray
    # (first E columns) - the bf16 values the forward chain consumed
    srcs = (acts, f.to(torch.bfloat16), e[:, :level.cfg.dim_dir_enc].to(torch.bfloat16).repeat_interleave(level._S, dim=0))

    # ---- weight gradients: plain GEMMs over the saved tensors (f32 accumulate and result)
    grads = []

    def linear_over(Mr):
        """`lin` over the first Mr rows, with the split-K factor chosen from that row count."""
        ck = 1
        while ck < 128 and Mr % (2 * ck) == 0 and Mr // (2 * ck) >= 2048:
            ck *= 2

        def wgrad(gy, *xs):
            gb = gy[:Mr].reshape(ck, Mr // ck, gy.shape[1]).transpose(1, 2)
            return torch.cat([torch.bmm(gb, x[:Mr].reshape(ck, Mr // ck, x.shape[1])).float().sum(0) for x in xs], 1)

        ones = torch.ones(ck, 1, Mr // ck, device=dev, dtype=torch.bfloat16) if Mr else None

        def lin(gy, *xs):
            if Mr == 0:  # no row: zeros, as the kernel's rule for a NULL upstream gradient
                grads.append(torch.zeros(gy.shape[1], sum(x.shape[1] for x in xs), device=dev))
                grads.append(torch.zeros(gy.shape[1], device=dev))
                return
            grads.append(wgrad(gy, *xs))
            # bias gradient = 1^T gy, through the same split-K batched GEMM (a column reduction of a strided [M, out] view runs at
            # a tenth of the memory bandwidth as an elementwise reduce kernel)
            grads.append(torch.bmm(ones, gy[:Mr].reshape(ck, Mr // ck, gy.shape[1])).float().sum(0)[0])

        return lin

    lin, rows = linear_over(M), M
    for l in plan.linears:
        if l.color and M_color not in (None, rows):
            lin, rows = linear_over(M_color), M_color
        lin(gacts[:, l.g_col:l.g_col + l.n_out], *(srcs[src][:, col:col + n] for src, col, n in l.blocks))
    return grads


class _FusedMLP(torch.autograd.Function):
    """The Linear stack of ZI/models.py:1116-1251 (density trunk, heads, view MLP, rgb) as two MFMA-chain kernels.  The weight
    gradients are GEMMs over the tensors those kernels save: dW_l = (d pre-activation_l)^T . (input_l), M-long reductions: library
    GEMMs (`_wgrad_bmm`) or, with `fused_wgrad`, `nlr_mlp_train_wgrad` (csrc/nlr_mlp_wgrad.hip).  Always through the three `_split`
    entry points: with `level._color_rays` (an integer, `TrainableNerfLevel.forward(color_rays=..)`) the rows of the later rays run
    the trunk and the heads only, without it M_color = M, which is the unsplit call (header section 6b)."""

    @staticmethod
    def forward(ctx, feats, enc, level, *params):
        plan = level._plan
        M, S = feats.shape[0], level._S
        Mc = M if level._color_rays is None else level._color_rays * S
        dev = feats.device
        flat = torch.cat([p.detach().reshape(-1).float() for p in params])
        new = lambda *s, dtype=torch.float32: torch.empty(*s, device=dev, dtype=dtype)
        K = level.cfg.class_num if level.cfg.use_semantic else 0
        density, rgb = new(M), new(3, M)
        sem = new(K, M) if K else None
        inten = new(M) if level.cfg.use_intensity else None
        acts = new(M, plan.act_w, dtype=torch.bfloat16)
        f = feats.detach().contiguous().float()
        e = enc.detach().contiguous().float()
        _lib.call("nlr_train_pack", plan.handle, flat)
        _lib.call("nlr_mlp_train_forward_split", plan.handle, f, e, M, Mc, S, density, rgb, sem, inten, acts)
        ctx.level, ctx.M, ctx.Mc = level, M, Mc
        ctx.save_for_backward(f, e, density, rgb, sem if sem is not None else density.new_empty(0),
                              inten if inten is not None else density.new_empty(0), acts)
        outs = [density, rgb]
        outs.append(sem if sem is not None else density.new_empty(0))
        outs.append(inten if inten is not None else density.new_empty(0))
        return tuple(outs)

    @staticmethod
    def backward(ctx, g_density, g_rgb, g_sem, g_inten):
        level, M, Mc = ctx.level, ctx.M, ctx.Mc
        plan, cfg = level._plan, level.cfg
        f, e, density, rgb, sem, inten, acts = ctx.saved_tensors
        dev = f.device
        K = cfg.class_num if cfg.use_semantic else 0
        gp = lambda g, ref: None if (g is None or ref.numel() == 0) else g.contiguous().float()
        gd, gr, gs, gi = gp(g_density, density), gp(g_rgb, rgb), gp(g_sem, sem), gp(g_inten, inten)
        gacts = torch.empty(M, plan.act_w + 64, device=dev, dtype=torch.bfloat16)
        d_feat = torch.empty_like(f)
        _lib.call("nlr_mlp_train_backward_split", plan.handle, M, Mc, level._S, density, rgb, sem if sem.numel() else None, acts, gd, gr, gs, gi,
                  gacts, d_feat)
        if getattr(level, "_keep_debug", False):  # tests look at the kernels' raw results
            level._dbg = {k: v.detach() for k, v in dict(acts=acts, gacts=gacts, d_feat=d_feat, feats=f, enc=e, density=density, rgb=rgb,
                                                        sem=sem, inten=inten).items()}
        if level.fused_wgrad:
            # ---- weight gradients: one MFMA kernel + a slab reduce (nlr_mlp_train_wgrad); views of one [n_params] f32 buffer
            d_params = torch.empty(plan.n_params, device=dev, dtype=torch.float32)
            ws = level._wgrad_workspace(dev)
            _lib.call("nlr_mlp_train_wgrad_split", plan.handle, M, Mc, level._S, f, e, acts, gacts, d_params, ws, ws.numel())
            if getattr(level, "_keep_debug", False):
                level._dbg["d_params"] = d_params.detach()
            grads, off = [], 0
            for p in level._mlp_params():
                grads.append(d_params[off:off + p.numel()].view(p.shape))
                off += p.numel()
        else:
            grads = _wgrad_bmm(level, M, f, e, acts, gacts, Mc)
        d_enc = _enc_grad(level, gacts, Mc, e) if ctx.needs_input_grad[1] else None
        return (d_feat, d_enc, None) + tuple(grads)


def _enc_grad(level, gacts, M_color, e):
    """d loss / d enc [N, 32] of the fused NerfMLP from what its backward saved: for every Linear that reads the direction encoding
    (view layer 0, and the layer behind the skip concatenation), the pre-activation gradient summed over the ray's samples in f32,
    times that layer's weight columns for `enc` (the bf16 values the kernels multiplied with).  Rays beyond M_color rows ran no view
    MLP: zeros."""
    S, E = level._S, level.cfg.dim_dir_enc
    n_color = M_color // S
    d_enc = torch.zeros_like(e)
    params = level._mlp_params()
    for i, l in enumerate(level._plan.linears):
        col = 0
        for src, _, n in l.blocks:
            if src == 2 and n_color:
                gsum = gacts[:M_color, l.g_col:l.g_col + l.n_out].float().reshape(n_color, S, l.n_out).sum(1)
                w = params[2 * i].detach()[:, col:col + E].to(torch.bfloat16).float()
                d_enc[:n_color, :E] += gsum @ w
            col += n
    return d_enc


class _Linear(NamedTuple):
    """One row of `nlr_train_linear_table` (header section 6b); blocks: (src, col, n) with src 0 acts, 1 features, 2 enc."""
    g_col: int
    o_off: int
    n_out: int
    color: int
    blocks: tuple
    w_off: int
    b_off: int


class _TrainPlan:
    TABLE_ROW = 16  # uint32 per Linear

    def __init__(self, cfg):
        h, n = C.c_void_p(None), C.c_uint32(0)
        F = cfg.grid_num_levels * cfg.grid_level_dim
        _lib.check(_lib.lib().nlr_train_plan_create(F, cfg.net_width_viewdirs, cfg.bottleneck_width, cfg.net_depth_viewdirs, cfg.deg_view,
                                                    cfg.class_num, int(cfg.use_semantic and not cfg.no_sem_layer), int(cfg.use_intensity),
                                                    cfg.density_bias, cfg.rgb_premultiplier, cfg.rgb_bias, cfg.rgb_padding,
                                                    C.byref(h), C.byref(n)), "nlr_train_plan_create")
        self.handle, self.n_params = h, int(n.value)
        self.act_w = int(_lib.lib().nlr_train_act_width(h))
        rows = (C.c_uint32 * (self.TABLE_ROW * 32))()
        n = _lib.lib().nlr_train_linear_table(h, rows, len(rows))
        if n <= 0:
            _lib.check(n or -1, "nlr_train_linear_table")
        t = np.frombuffer(rows, dtype=np.uint32)[:n * self.TABLE_ROW].reshape(n, self.TABLE_ROW).tolist()
        self.linears = [_Linear(*r[:4], tuple(tuple(r[5 + 3 * k:8 + 3 * k]) for k in range(r[4])), *r[14:]) for r in t]

    def __del__(self):
        try:
            _lib.lib().nlr_train_plan_destroy(self.handle)
        except Exception:
            pass


class TrainableNerfLevel(torch.nn.Module):
    """The final (NerfMLP) level as a trainable module with the reference's parameter names (`encoder.embeddings`,
    `density_layer.0.weight`, `lin_second_stage_3.bias`, `sem_layer.2.weight`, ...; ZI/models.py:847-961), so that
    `load_state_dict({k[len('nerf_mlp.'):]: v ...})` takes a reference checkpoint and the trained weights go back into
    `nerflidar_hip.models.Model` for fused inference.  forward = MLP.forward (models.py:1036-1265, inference subset:
    disable_density_normals, no GLO) on the intervals of `tdist`; `render` adds the compositing."""

    def __init__(self, cfg, table_std: float = 1e-4, fused_mlp: bool = False, fused_wgrad: bool = False):
        """fused_mlp: run the Linear stack through nlr_mlp_train_forward / _backward (bf16 MFMA chains, f32 accumulation) instead
        of torch Linear modules; parameters, their names and their gradients are the same objects either way.  It also chooses the
        encode: the fused cast + encode operator with it, `cast_contract` + `GridEncoder` without - except for a batch whose ray
        tensors require a gradient (`rays_require_grad`), which runs the fused operator on the fp32 model too, because only that
        operator has a ray gradient (its features differ from the unfused route's by a few ulp).
        fused_wgrad (needs fused_mlp): the weight and bias gradients from nlr_mlp_train_wgrad (one MFMA kernel, f32 accumulation
        over all of M, bit-reproducible) instead of split-K library GEMMs."""
        super().__init__()
        nn = torch.nn
        self.cfg = cfg
        if fused_wgrad and not fused_mlp:
            raise ValueError("fused_wgrad=True needs fused_mlp=True: the weight-gradient kernel reads what the fused kernels save")
        self.fused_mlp = bool(fused_mlp)
        self.fused_wgrad = bool(fused_wgrad)
        self._wgrad_ws = {}  # device -> workspace of nlr_mlp_train_wgrad, allocated once
        # cast + encode + re-weight + mean as one operator (encode_features_fused).  Whatever this says, a batch whose ray tensors
        # require a gradient (pose refinement; viewdirs alone included) takes that operator: `cast_contract` carries no gradient
        self.fused_encode = bool(fused_mlp)
        self._plan = None
        self._color_rays = None  # set by forward(color_rays=..) for _FusedMLP, like _S
        if self.fused_mlp and cfg.use_semantic and cfg.no_sem_layer:
            raise NotImplementedError("fused training MLP: no_sem_layer=True is not wired (use fused_mlp=False)")
        if self.fused_mlp and cfg.skip_layer_dir != 0:
            # the fused kernels wire the skip concatenation into view layer 1 (nlr_mlp_train.hip); another position has the same
            # parameter count, so nothing downstream would notice (the inference path rejects it too, nlr_api.hip)
            raise NotImplementedError(f"fused training MLP: skip_layer_dir = {cfg.skip_layer_dir} is not wired, only 0 (use fused_mlp=False)")
        self.encoder = GridEncoder.from_mlp_config(cfg)
        feat = cfg.grid_num_levels * cfg.grid_level_dim
        self.density_layer = nn.Sequential(nn.Linear(feat, 64), nn.ReLU(), nn.Linear(64, cfg.bottleneck_width))
        in_rgb = cfg.bottleneck_width + cfg.dim_dir_enc
        last = in_rgb
        for i in range(cfg.net_depth_viewdirs):
            lin = nn.Linear(last, cfg.net_width_viewdirs)
            nn.init.kaiming_uniform_(lin.weight)
            self.add_module(f"lin_second_stage_{i}", lin)
            last = cfg.net_width_viewdirs + (in_rgb if i == cfg.skip_layer_dir else 0)
        self.rgb_layer = nn.Linear(last, cfg.num_rgb_channels)
        if not cfg.no_sem_layer and not cfg.fixed_semantic:  # built whether or not use_semantic reads it (ZI/models.py:954-957)
            self.sem_layer = nn.Sequential(nn.Linear(cfg.bottleneck_width, 64), nn.ReLU(), nn.Linear(64, cfg.class_num))
        if cfg.use_intensity:
            self.intensity_layer = nn.Sequential(nn.Linear(cfg.bottleneck_width, 64), nn.ReLU(), nn.Linear(64, 1))

    def load_reference(self, state_dict, prefix: str = "nerf_mlp."):
        sd = {k[len(prefix):]: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v)))
              for k, v in state_dict.items() if k.startswith(prefix) and not k.endswith(("encoder.offsets", "encoder.grid_sizes", "encoder.idx"))}
        missing, unexpected = self.load_state_dict(sd, strict=False)
        bad = [m for m in missing if not m.startswith("encoder.") or m == "encoder.embeddings"]
        if bad or unexpected:
            raise KeyError(f"state_dict mismatch: missing {bad}, unexpected {list(unexpected)}")
        return self

    def forward(self, batch: Dict[str, torch.Tensor], tdist: torch.Tensor, sample_n: int = 7, sample_m: int = 3,
                rand_deg: Optional[torch.Tensor] = None, color_rays: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """color_rays: None, or the number n of leading rays that carry colour supervision (0 <= n <= N; anything else raises
        ValueError).  The rays [n, N) - the LiDAR rays the reference appends to every batch, ZI/datasets.py:352-390 - then skip the
        view MLP (`lin_second_stage_*`, `rgb_layer`) forward and backward and come back with rgb = 0.  THE CALLER PROMISES that the
        loss ignores their colour: `batch['mask_rgb']` is zero on rays [n, N) (train.py:316-320).  Under that promise every gradient
        is the one the masked loss gives without `color_rays`; nothing here reads the mask (a step stays free of host reads)."""
        F = torch.nn.functional
        cfg = self.cfg
        nc = _check_color_rays(color_rays, tdist.shape[0])
        if self.fused_encode or rays_require_grad(batch):  # (the ray gradient exists on the fused operator only)
            feats = encode_features_fused(self.encoder, batch, tdist, sample_n, sample_m, rand_deg=rand_deg, re_weights=cfg.re_weights)
        else:
            means, stds = cast_contract(batch, tdist, sample_n, sample_m, rand_deg=rand_deg)
            feats = encode_features(self.encoder, means, stds, cfg.re_weights)
        if self.fused_mlp:
            return self._forward_fused(batch, feats, nc)
        x = self.density_layer(feats)
        out = {"density": F.softplus(x[..., 0] + cfg.density_bias)}
        if cfg.use_semantic:
            out["semantic"] = torch.softmax(x[..., 1:1 + cfg.class_num] if cfg.no_sem_layer else self.sem_layer(x), -1)
        if cfg.use_intensity:
            out["intensity"] = self.intensity_layer(x)[..., 0]
        enc = _pos_enc(batch["viewdirs"].reshape(x.shape[0], 3).float(), cfg.deg_view)
        n_all = x.shape[0]
        if nc is not None:  # the view MLP on the rays with colour supervision only
            x, enc = x[:nc], enc[:nc]
        rgb = view_mlp(cfg, lambda name, t: getattr(self, name)(t), x, enc[:, None, :].expand(-1, x.shape[1], -1))
        if nc is not None:  # rgb = 0 for the rest (a zeros block carries no gradient)
            rgb = torch.cat([rgb, rgb.new_zeros(n_all - nc, *rgb.shape[1:])], dim=0)
        out["rgb"] = rgb
        return out

    def _mlp_params(self):
        """The Linear parameters in the order of the plan's flat buffer (include/nerflidar_hip.h, section 6b)."""
        cfg = self.cfg
        mods = [self.density_layer[0], self.density_layer[2]]
        if cfg.use_semantic and not cfg.no_sem_layer:
            mods += [self.sem_layer[0], self.sem_layer[2]]
        if cfg.use_intensity:
            mods += [self.intensity_layer[0], self.intensity_layer[2]]
        mods += [getattr(self, f"lin_second_stage_{i}") for i in range(cfg.net_depth_viewdirs)] + [self.rgb_layer]
        out = []
        for m in mods:
            out += [m.weight, m.bias]
        return out

    def _wgrad_workspace(self, dev):
        """The slab workspace of nlr_mlp_train_wgrad on `dev`: its size depends on the plan only, so one allocation serves every step."""
        ws = self._wgrad_ws.get(dev)
        if ws is None:
            n = int(_lib.lib().nlr_mlp_train_wgrad_workspace_bytes(self._plan.handle, 0))
            ws = self._wgrad_ws[dev] = torch.empty(n, device=dev, dtype=torch.uint8)
        return ws

    def _forward_fused(self, batch, feats, color_rays=None):
        cfg = self.cfg
        n, S = feats.shape[0], feats.shape[1]
        self._color_rays = color_rays
        if self._plan is None:
            with torch.cuda.device(feats.device):  # nlr_train_plan_create allocates on the current device
                self._plan = _TrainPlan(cfg)
        self._S = S
        params = self._mlp_params()
        assert sum(p.numel() for p in params) == self._plan.n_params
        enc = torch.nn.functional.pad(_pos_enc(batch["viewdirs"].reshape(n, 3).float(), cfg.deg_view), (0, 32 - cfg.dim_dir_enc))
        density, rgb, sem, inten = _FusedMLP.apply(feats.reshape(n * S, -1), enc, self, *params)
        out = {"density": density.reshape(n, S), "rgb": rgb.reshape(3, n, S).permute(1, 2, 0)}
        if cfg.use_semantic:
            out["semantic"] = sem.reshape(-1, n, S).permute(1, 2, 0)
        if cfg.use_intensity:
            out["intensity"] = inten.reshape(n, S)
        return out

    def render(self, batch, tdist, opaque_background: bool = True, bg: float = 1.0, **kw):
        """forward + compositing; keywords (`color_rays` among them, see `forward`) go to `forward`."""
        o = self.forward(batch, tdist, **kw)
        r = volumetric_render(o["density"], tdist, batch["directions"].reshape(tdist.shape[0], 3), o["rgb"], o.get("semantic"),
                              o.get("intensity"), opaque_background, bg)
        return r, o


# ---- the whole model for training: Model.forward (ZI/models.py:239-576) with autograd, and the step of train.py:272-459 -------------
class _PropDensity(torch.autograd.Function):
    """raw density of a PropMLP, `density_layer(feats)[..., 0]`, through `nlr_prop_mlp_forward` / `_backward` (the hidden units are
    recomputed in the backward: only the features are saved)."""

    @staticmethod
    def forward(ctx, feats, w1, b1, w2, b2):
        f = feats.contiguous().float()
        M, F = f.shape
        raw = torch.empty(M, device=f.device)
        ps = [t.detach().contiguous().float() for t in (w1, b1, w2, b2)]
        _lib.call("nlr_prop_mlp_forward", f, *ps, M, F, raw)
        ctx.save_for_backward(f, *ps)
        return raw

    @staticmethod
    def backward(ctx, g):
        f, w1, b1, w2, b2 = ctx.saved_tensors
        M, F = f.shape
        g = g.contiguous().float()
        d_f = torch.empty_like(f) if ctx.needs_input_grad[0] else None
        d = [torch.empty_like(t) for t in (w1, b1, w2, b2)]
        _lib.call("nlr_prop_mlp_backward", f, w1, b1, w2, b2, g, M, F, d_f, *d)
        return (d_f, *d)


class TrainablePropLevel(torch.nn.Module):
    """A PropMLP (ZI/models.py:PropMLP: disable_rgb) with the reference's parameter names: `encoder.embeddings`,
    `density_layer.{0,2}.{weight,bias}`."""

    def __init__(self, cfg, fused: bool = True):
        """fused: the density network through `nlr_prop_mlp_forward` / `_backward` instead of two library GEMMs with 6-8 wide
        operands; same parameters, same gradients (fp32 both ways).  A batch whose ray tensors require a gradient takes the fused
        encode either way (`rays_require_grad`)."""
        super().__init__()
        nn = torch.nn
        self.cfg, self.fused = cfg, bool(fused)
        self.encoder = GridEncoder.from_mlp_config(cfg)
        self.density_layer = nn.Sequential(nn.Linear(cfg.grid_num_levels * cfg.grid_level_dim, 64), nn.ReLU(), nn.Linear(64, 1))

    load_reference = TrainableNerfLevel.load_reference

    def forward(self, batch, tdist, sample_n: int = 7, sample_m: int = 3, rand_deg=None) -> Dict[str, torch.Tensor]:
        if self.fused or rays_require_grad(batch):  # (the ray gradient exists on the fused operator only)
            feats = encode_features_fused(self.encoder, batch, tdist, sample_n, sample_m, rand_deg=rand_deg, re_weights=self.cfg.re_weights)
        else:
            means, stds = cast_contract(batch, tdist, sample_n, sample_m, rand_deg=rand_deg)
            feats = encode_features(self.encoder, means, stds, self.cfg.re_weights)
        if self.fused and feats.shape[-1] <= 16:
            l0, l2 = self.density_layer[0], self.density_layer[2]
            raw = _PropDensity.apply(feats.reshape(-1, feats.shape[-1]), l0.weight, l0.bias, l2.weight, l2.bias).reshape(feats.shape[:-1])
        else:
            raw = self.density_layer(feats)[..., 0]
        return {"density": torch.nn.functional.softplus(raw + self.cfg.density_bias)}


class TrainableObjMLP(torch.nn.Module):
    """One class's object network (ZI/models.py:MLP as `ObjMLP` configures it under the shipped gin, nuscenes_single.gin:36-44) as a
    trainable module with the reference's parameter names (`encoder.embeddings`, `density_layer.{0,2}`, `lin_second_stage_{i}`,
    `rgb_layer`): hash grid on box coordinates through the HIP operator (forward + backward), [grid | shape half of the latent] -> 64 ->
    bottleneck, view MLP on [bottleneck | pos_enc(dir) | texture half] with the skip concatenation, fixed one-hot semantic of the class.
    The differentiable twin of `objects.ObjMLP.forward`."""

    def __init__(self, cfg):
        super().__init__()
        from .weights import mlp_param_shapes
        nn = torch.nn
        self.cfg = cfg
        self.encoder = GridEncoder.from_mlp_config(cfg)
        for name, (o, i), kaiming in mlp_param_shapes(cfg):
            lin = nn.Linear(i, o)
            if kaiming:
                nn.init.kaiming_uniform_(lin.weight)
            mod, _, leaf = name.partition(".")
            if leaf:  # density_layer.0 / .2: an nn.Sequential with a ReLU between, like the reference's
                if not hasattr(self, mod):
                    self.add_module(mod, nn.Sequential())
                seq = getattr(self, mod)
                while len(seq) < int(leaf):
                    seq.append(nn.ReLU())
                seq.append(lin)
            else:
                self.add_module(name, lin)

    load_reference = TrainableNerfLevel.load_reference

    def forward(self, pts: torch.Tensor, viewdirs: torch.Tensor, latent: Optional[torch.Tensor]) -> Dict[str, torch.Tensor]:
        return obj_mlp_forward(self.cfg, self.encoder, lambda name, x: self.get_submodule(name)(x), pts, viewdirs, latent)


class _ObjFrame(torch.autograd.Function):
    """(tracks [n_obj, T, 9], origins, directions, viewdirs [N, 3]) -> (box-frame points, box-frame view directions) of the owned
    samples.  forward = `objects.box_frame` on the constants `nlr_track_box_params` made of the same tracks (the values of the path
    without gradient, bit for bit).  backward builds only what `ctx.needs_input_grad` asks for: the track gradient from
    `nlr_obj_frame_backward` (track refinement), the three ray gradients from `nlr_obj_frame_backward_rays` (pose refinement) - one
    reduction kernel each instead of the gather / index_put chain autograd would walk.  Either kind of input may be plain data."""

    @staticmethod
    def forward(ctx, tracks, ts, origins, dirs, viewdirs, td, box, ri, si, tr):
        ctx.save_for_backward(tracks.detach().contiguous(), ts, origins, dirs, viewdirs, td, box, ri.int().contiguous(),
                              si.int().contiguous(), tr.int().contiguous())
        return box_frame(origins, dirs, viewdirs, td, box, ri, si, tr)

    @staticmethod
    def backward(ctx, g_p, g_d):
        tracks, ts, origins, dirs, viewdirs, td, box, ri, si, tr = ctx.saved_tensors
        need = ctx.needs_input_grad
        g_tracks = obj_frame_backward(tracks, ts, origins, dirs, viewdirs, td, ri, si, tr, g_p, g_d) if need[0] else None
        g_rays = (None, None, None)
        if any(need[2:5]):
            g_rays = obj_frame_backward_rays(box, viewdirs, td, ri, si, tr, g_p, g_d, want=tuple(need[2:5]))
        return (g_tracks, None) + tuple(g_rays) + (None,) * 5


def obj_frame_backward(tracks, ts, origins, dirs, viewdirs, td, ri, si, tr, g_pts, g_dirs) -> torch.Tensor:
    """`nlr_obj_frame_backward`: d/d tracks [n_obj, T, 9] of the box-frame points / directions of the K owned samples (int32 lists
    ri, si, tr sorted by (ray, sample)) contracted with their cotangents g_pts, g_dirs [K, 3]."""
    n, S, K = td.shape[0], td.shape[1] - 1, ri.shape[0]
    n_obj, T = tracks.shape[0], tracks.shape[1]
    g_pts, g_dirs = g_pts.contiguous().float(), g_dirs.contiguous().float()
    out = torch.empty_like(tracks)
    need = _lib.lib().nlr_obj_frame_backward_workspace_bytes(K, n_obj, T)
    ws = torch.empty(need, dtype=torch.uint8, device=tracks.device) if need else None
    _lib.call("nlr_obj_frame_backward", tracks, ts, origins, dirs, viewdirs, td, n, S, n_obj, T, ri, si, tr, K, g_pts, g_dirs, out, ws, need)
    return out


def obj_frame_backward_rays(box, viewdirs, td, ri, si, tr, g_pts, g_dirs, want=(True, True, True)):
    """`nlr_obj_frame_backward_rays`: (d_origins, d_directions, d_viewdirs) [N, 3] of the box-frame points / directions of the K owned
    samples (int32 lists ri, si, tr sorted by (ray, sample); box [N, n_obj, 8] from `track_box_params`) contracted with their
    cotangents g_pts, g_dirs [K, 3].  An output that `want` leaves out is None and is neither computed nor written."""
    n, S, K = td.shape[0], td.shape[1] - 1, ri.shape[0]
    g_pts, g_dirs = (None if g is None else g.contiguous().float() for g in (g_pts, g_dirs))   # (None: the outputs that read it are not wanted)
    out = [torch.empty(n, 3, dtype=torch.float32, device=td.device) if w else None for w in want]
    _lib.call("nlr_obj_frame_backward_rays", box, viewdirs, td, n, S, box.shape[1], ri, si, tr, K, g_pts, g_dirs, *out)
    return tuple(out)


def _ptr_array(tensors):
    """Host array of device pointers (`T *const *` of the header)."""
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def objects_desc(mlps, track_class, latent_size: int, weights: bool = False, latents=None):
    """(`NlrObjectsDesc`, keep) of the `TrainableObjMLP`s `mlps` (one per class) and the tracks' classes.  weights = False: shapes and
    scalars only, what `nlr_obj_train_plan_create` and `nlr_obj_train_desc_layout` read.  True: also the Linears, the tables (the
    modules' own device tensors) and `latents` [n_tracks, latent_size] as host copies, what `nlr_objects_create` takes.  Hold `keep`
    while the descriptor is in use."""
    keep = []

    def linear(lin):
        w, b = (np.ascontiguousarray(t.detach().cpu().numpy(), np.float32) for t in (lin.weight, lin.bias))
        keep.extend([w, b])
        l = _lib.NlrLinear()
        l.weight, l.bias, (l.out_features, l.in_features) = w.ctypes.data, b.ctypes.data, w.shape
        return l
    descs = (_lib.NlrObjClassDesc * len(mlps))()
    for d, m in zip(descs, mlps):
        cfg, md = m.cfg, d.mlp
        md.grid = _EncodeFeatures._descs(m.encoder, m.encoder.embeddings)
        md.disable_rgb, md.bottleneck_width = int(cfg.disable_rgb), cfg.bottleneck_width
        md.net_depth_viewdirs, md.net_width_viewdirs = cfg.net_depth_viewdirs, cfg.net_width_viewdirs
        md.skip_layer_dir, md.deg_view, md.class_num = cfg.skip_layer_dir, cfg.deg_view, cfg.class_num
        md.density_bias, md.rgb_premultiplier = cfg.density_bias, cfg.rgb_premultiplier
        md.rgb_bias, md.rgb_padding, md.re_weights = cfg.rgb_bias, cfg.rgb_padding, int(cfg.re_weights)
        d.latent_size, d.split_latent, d.class_type = int(latent_size), int(cfg.split_latent), int(cfg.class_type)
        if weights:
            md.density0, md.density2 = linear(m.get_submodule("density_layer.0")), linear(m.get_submodule("density_layer.2"))
            for i in range(cfg.net_depth_viewdirs):
                md.view[i] = linear(m.get_submodule(f"lin_second_stage_{i}"))
            md.rgb_layer = linear(m.rgb_layer)
    tc = np.ascontiguousarray(track_class, np.int32)
    od = _lib.NlrObjectsDesc()
    od.n_classes, od.classes, od.n_tracks, od.track_class = len(mlps), descs, len(tc), tc.ctypes.data
    keep.extend([descs, tc])
    if weights and latents is not None:
        lt = np.ascontiguousarray(latents.detach().cpu().numpy(), np.float32)
        keep.append(lt)
        od.latents = lt.ctypes.data
    return od, keep


def _no_plan():
    return None


class _ObjTrainPlan:
    """`NlrObjTrainPlan` (header section 7e) of a model's object networks: made of the classes' shapes and the tracks' classes; knows the
    order of every class's flat parameter buffer (`flat`) and checks it against `nlr_obj_train_param_layout` once."""

    def __init__(self, mlps, track_class, latent_size: int, device):
        from .weights import mlp_param_shapes
        self.n_classes, self.device = len(mlps), torch.device(device)
        od, _keep = objects_desc(mlps, track_class, latent_size)  # (shapes only: the plan reads neither weights nor tables)
        n_params = np.zeros(len(mlps), np.int32)
        self.handle = C.c_void_p(None)
        _lib.call("nlr_obj_train_plan_create", od, self.handle, n_params, device=self.device)
        self.n_params = [int(v) for v in n_params]
        self.names = [[name for name, _, _ in mlp_param_shapes(m.cfg)] for m in mlps]
        self._ws = None
        for c, m in enumerate(mlps):  # the order `flat` concatenates in is the order the kernels read
            offs = (C.c_uint32 * 32)()
            cnt = _lib.lib().nlr_obj_train_param_layout(self.handle, c, offs, len(offs))
            if cnt <= 0:
                _lib.check(cnt or -1, "nlr_obj_train_param_layout")
            want, at = [], 0
            for name in self.names[c]:
                lin = m.get_submodule(name)
                want += [at, at + lin.weight.numel()]
                at += lin.weight.numel() + lin.bias.numel()
            if list(offs[:cnt]) != want or at != self.n_params[c]:
                raise RuntimeError(f"nlr_obj_train_param_layout: class {c} has offsets {list(offs[:cnt])} ({self.n_params[c]} parameters), "
                                   f"the module's Linears give {want} ({at})")

    def flat(self, c: int, m) -> torch.Tensor:
        """Class c's parameters as the flat buffer of the header, a differentiable `cat` of the module's own tensors."""
        return torch.cat([p.reshape(-1) for name in self.names[c] for p in (m.get_submodule(name).weight, m.get_submodule(name).bias)]).float()

    def pack(self, flats) -> None:
        _lib.call("nlr_obj_train_pack", self.handle, _ptr_array(flats), device=self.device)

    def workspace(self, n: int, S: int) -> torch.Tensor:
        """The forward-only workspace, kept between calls (a forward with a backward gets one of its own, `_ObjectsFused`)."""
        need = _lib.lib().nlr_obj_train_workspace_bytes(self.handle, n, S, 0)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    # a plan is a handle the library owns: a copied or unpickled model gets none and makes its own on first use
    def __deepcopy__(self, memo):
        return None

    def __reduce__(self):
        return (_no_plan, ())

    def __del__(self):
        try:
            _lib.lib().nlr_obj_train_plan_destroy(self.handle)
        except Exception:
            pass


def objects_forward(plan: _ObjTrainPlan, tables, latents, rays_desc, td, box, density, rgb=None, semantic=None, workspace=None):
    """`nlr_obj_train_forward` in place on density [N,S], rgb [3,N,S] / semantic [K,N,S] (None: the density-only form); returns the
    owner map [N,S] int32.  `workspace`: a tensor of `nlr_obj_train_workspace_bytes(.., 1)` bytes when a backward follows."""
    n, S = td.shape[0], td.shape[1] - 1
    winner = torch.full((n, S), -1, dtype=torch.int32, device=td.device)  # (no tracks, no samples: the call writes nothing)
    ws = plan.workspace(n, S) if workspace is None else workspace
    _lib.call("nlr_obj_train_forward", plan.handle, _ptr_array(tables), latents, rays_desc, td, box, n, S, box.shape[1], density, rgb, semantic,
              0 if semantic is None else semantic.shape[0], winner, ws, ws.numel())
    return winner


def _dense_sample_index(n: int, S: int, dev):
    """(ray_idx, sample_idx) int32 [n*S] of the dense list of header section 7e: m -> (m // S, m % S).  Made on the device, nothing is
    read back; two small kernels per backward, not worth keeping between steps."""
    m = torch.arange(n * S, dtype=torch.int32, device=dev)
    return torch.div(m, S, rounding_mode="floor").contiguous(), (m % S).contiguous()


class _ObjectsFused(torch.autograd.Function):
    """The object branch of the last level as one operator (header section 7e): (density [N,S], rgb [N,S,3], semantic [N,S,K] of the
    static field, latent table [n_tracks, latent_size], the classes' hash tables, the classes' flat parameter buffers) -> (merged
    density, rgb, semantic, owner mask).  forward = `nlr_obj_train_forward`; backward = `nlr_obj_train_backward` for tables, flat
    buffers and latent codes, and the upstream gradient with the owned samples zeroed for the static tensors (the merge overwrote
    them).
    Behind the flat buffers the call may carry the five tensors the box frame depends on - tracks [n_obj, T, 9], timestamps [N], origins,
    directions, viewdirs [N, 3] - any of which may be plain data.  When one of them needs a gradient the backward takes
    `nlr_obj_train_backward_frame`, which also writes the cotangents of the box-frame points and directions of every sample [N*S, 3],
    and hands them with the owner map to `obj_frame_backward` (tracks) / `obj_frame_backward_rays` (rays) as the dense list of the
    header: K = N*S entries, an unowned one with track -1.  Nothing is read back: K is a Python int and the owner map is the forward's.
    Without them, or when none needs a gradient, the box frame carries no gradient and the backward is `nlr_obj_train_backward`.
    The backward runs on the plan's weight images as the LAST `pack` left them (`TrainableModel.forward` packs once per forward): run a
    forward's backward before the same model's parameters change and its next forward packs again, as `training_step` does."""

    @staticmethod
    def forward(ctx, plan, rays_desc, keep, td, box, density, rgbs, sem, latents, *tables_flats_frame):
        nc = plan.n_classes
        if len(tables_flats_frame) not in (2 * nc, 2 * nc + 5):
            raise ValueError(f"_ObjectsFused: {nc} tables and {nc} flat buffers, then nothing or (tracks, timestamps, origins, directions, "
                             f"viewdirs); got {len(tables_flats_frame)} tensors")
        tabs = [t.detach() for t in tables_flats_frame[:nc]]
        frame = [t.detach().float().contiguous() for t in tables_flats_frame[2 * nc:]]
        n, S = td.shape[0], td.shape[1] - 1
        cf = torch.contiguous_format
        dens = density.detach().float().clone(memory_format=cf)
        rgb_t = rgbs.detach().float().permute(2, 0, 1).clone(memory_format=cf)
        sem_t = None if sem is None else sem.detach().float().permute(2, 0, 1).clone(memory_format=cf)
        lat = latents.detach().float().contiguous()
        need = _lib.lib().nlr_obj_train_workspace_bytes(plan.handle, n, S, 1)
        ws = torch.empty(need, dtype=torch.uint8, device=td.device)  # holds the lists until the backward: not shared between calls
        winner = objects_forward(plan, tabs, lat, rays_desc, td, box, dens, rgb_t, sem_t, workspace=ws)
        mask = winner >= 0
        ctx.save_for_backward(td, box, lat, ws, mask, winner, *tabs, *frame)
        ctx.misc = (plan, rays_desc, keep)
        ctx.mark_non_differentiable(mask)
        return dens, rgb_t.permute(1, 2, 0), None if sem_t is None else sem_t.permute(1, 2, 0), mask

    @staticmethod
    def backward(ctx, g_dens, g_rgb, g_sem, _g_mask):
        td, box, lat, ws, mask, winner, *rest = ctx.saved_tensors
        plan, rays_desc, _keep = ctx.misc
        nc = plan.n_classes
        tabs, frame = rest[:nc], rest[nc:]
        need = ctx.needs_input_grad[9 + 2 * nc:] if frame else ()   # (tracks, timestamps, origins, directions, viewdirs)
        n, S = td.shape[0], td.shape[1] - 1
        dev = td.device
        gd = torch.zeros(n, S, device=dev) if g_dens is None else g_dens.float().contiguous()
        gr = torch.zeros(3, n, S, device=dev) if g_rgb is None else g_rgb.float().permute(2, 0, 1).contiguous()
        d_flats = [torch.empty(k, device=dev) for k in plan.n_params]
        d_lat = torch.empty_like(lat)
        g_tabs = [torch.zeros_like(t) for t in tabs]
        g_frame = ()
        if not any(need):
            _lib.call("nlr_obj_train_backward", plan.handle, _ptr_array(tabs), lat, rays_desc, td, box, n, S, box.shape[1], gd, gr,
                      _ptr_array(d_flats), d_lat, _ptr_array(g_tabs), ws, ws.numel())
            g_frame = (None,) * len(frame)
        else:
            tracks, ts, origins, dirs, viewdirs = frame
            want_p, want_d = need[0] or need[2] or need[3], need[0] or need[4]
            g_pts = torch.empty(n * S, 3, device=dev) if want_p else None
            g_dirs = torch.empty(n * S, 3, device=dev) if want_d else None
            _lib.call("nlr_obj_train_backward_frame", plan.handle, _ptr_array(tabs), lat, rays_desc, td, box, n, S, box.shape[1], gd, gr,
                      _ptr_array(d_flats), d_lat, _ptr_array(g_tabs), g_pts, g_dirs, ws, ws.numel())
            ri, si = _dense_sample_index(n, S, dev)
            tr = winner.reshape(-1)
            g_tracks = obj_frame_backward(tracks, ts, origins, dirs, viewdirs, td, ri, si, tr, g_pts, g_dirs) if need[0] else None
            g_rays = (None, None, None)
            if any(need[2:5]):
                # an output that is not wanted is not computed, so the cotangent it alone would read may be missing
                g_rays = obj_frame_backward_rays(box, viewdirs, td, ri, si, tr, g_pts, g_dirs, want=tuple(need[2:5]))
            g_frame = (g_tracks, None) + tuple(g_rays)

        def static(g, m):
            return None if g is None else torch.where(m, torch.zeros_like(g), g)
        return (None,) * 5 + (static(g_dens, mask), static(g_rgb, mask[..., None]), static(g_sem, mask[..., None]), d_lat, *g_tabs, *d_flats,
                              *g_frame)


class TrainableModel(torch.nn.Module):
    """`Model` (ZI/models.py:31-576, no GLO) as a trainable module: submodules `prop_mlp_<i>` and `nerf_mlp` with the reference's
    parameter names, so a reference checkpoint loads with `load_reference` and the trained `state_dict()` goes straight into
    `nerflidar_hip.models.Model` for fused inference.  With `mc.config.instance_obj` (the shipped gin, nuscenes_single.gin:13) and
    `tracks` / `class_names` also the dynamic-object branch of models.py:401-477 in training form: `obj_mlp_<class id>` per class,
    `latent_vector_dict.obj_latent_<track>` per track (train_utils.py:459-471), evaluated on the samples inside the boxes of every level
    (detached on the proposal levels, models.py:447-449) and merged before compositing; `obj_mask` rides in the ray history for the
    interlevel term (train_utils.py:153-157).  Its `state_dict()` feeds `objects.DynamicModel` / `checkpoints.dynamic_model_from_checkpoint`.

    forward = the level loop of models.py:316-557 in training form: the sample positions come from the fused resampling kernel
    (`nlr_resample_level`; they carry no gradient, Model.stop_level_grad = True), cast / contraction from `nlr_cast_contract`,
    hash-grid features and their gradient from the HIP grid operator, the NerfMLP from torch Linear modules or the fused MFMA
    forward / backward (`fused_mlp=True`), compositing and its gradient from `nlr_composite_level` / `nlr_composite_backward`."""

    def __init__(self, mc, fused_mlp: bool = False, fused_wgrad: bool = False, tracks=None, class_names=None, obj_log2_hashmap: int = 21,
                 fused_objects: bool = False, fused_object_frame: bool = False):
        """fused_objects (with `instance_obj`): every level's object merge runs through the operator of header section 7e
        (`nlr_obj_train_forward` / `_backward`: owner map, per-class lists and the object networks on the device, weight / latent / table
        gradients from fixed-order reductions) instead of the torch chain of `_object_merge`; a step then reads nothing back to the host.
        Parameters, their names and `state_dict()` are the same either way.  Proposal levels replace the density only.  That is NOT what the
        reference's merge and `_object_merge` do: a PropMLP returns a black rgb (models.py:1119-1122) which they overwrite with the
        detached object rgb inside the boxes, so with `fused_objects=True` a proposal level's rendered rgb stays black there and a
        nonzero `data_coarse_mult` gives another coarse data loss than the reference's (the shipped value is 0: no difference).
        Tracks that require a gradient (track refinement) and ray tensors that require one (pose refinement) are refused on this path
        with NotImplementedError, unless `fused_object_frame=True`.
        fused_object_frame (needs `fused_objects=True`, else ValueError): the last level's fused operator also forms the cotangents of
        the box-frame points and directions (`nlr_obj_train_backward_frame`) and hands them to `nlr_obj_frame_backward` /
        `nlr_obj_frame_backward_rays` as a dense list over all N * S samples, so track and pose refinement run through the fused object
        path as well, still without a host read.  Proposal levels stay the density-only form without gradient (models.py:447-449).
        Values of a forward are the same bits with or without it, and whether or not anything requires a gradient."""
        super().__init__()
        if not mc.nerf_mlp.disable_density_normals:
            raise NotImplementedError("NerfMLP.disable_density_normals = False in training: losses on normals need the second derivative of the "
                                      "grid; normals are an inference output (models.Model, normals.density_normals)")
        self.mc = mc
        self.fused_objects = bool(fused_objects)
        self.fused_object_frame = bool(fused_object_frame)
        if self.fused_object_frame and not self.fused_objects:
            raise ValueError("fused_object_frame=True is an option of the fused object operator: pass fused_objects=True as well")
        self._obj_plan = None
        for i in range(mc.num_levels - 1):
            self.add_module(f"prop_mlp_{i}", TrainablePropLevel(mc.prop_cfg(i), fused=fused_mlp))
        import dataclasses
        ncfg = dataclasses.replace(mc.nerf_mlp, use_semantic=mc.config.use_semantic, use_intensity=mc.config.use_intensity,
                                   no_sem_layer=mc.config.no_sem_layer)
        self.nerf_mlp = TrainableNerfLevel(ncfg, fused_mlp=fused_mlp, fused_wgrad=fused_wgrad)
        self.instance_obj = bool(mc.config.instance_obj)
        if self.instance_obj:
            if tracks is None or class_names is None:
                raise ValueError("Config.instance_obj = True needs tracks [N_obj, T, 9] and one class name per track (dataset.bboxes)")
            check_instance_obj(mc.config)
            self.register_buffer("tracks", torch.as_tensor(np.asarray(tracks, np.float32)))
            self.class_ids = [query_class(c) for c in class_names]
            self._class_list = sorted(set(self.class_ids))
            self.register_buffer("_class_rank", torch.tensor([self._class_list.index(c) for c in self.class_ids]))
            for cid in self._class_list:
                self.add_module(f"obj_mlp_{cid}", TrainableObjMLP(obj_mlp_config(cid, latent_size=mc.config.latent_size, log2_hashmap=obj_log2_hashmap,
                                                                                 use_semantic=mc.config.use_semantic)))
            self.latent_vector_dict = torch.nn.ParameterDict(
                {f"obj_latent_{t}": torch.nn.Parameter(torch.nn.init.normal_(torch.empty(mc.config.latent_size))) for t in range(len(self.class_ids))})

    def levels(self):
        return [getattr(self, f"prop_mlp_{i}") for i in range(self.mc.num_levels - 1)] + [self.nerf_mlp]

    def load_reference(self, state_dict):
        for i in range(self.mc.num_levels - 1):
            getattr(self, f"prop_mlp_{i}").load_reference(state_dict, f"prop_mlp_{i}.")
        self.nerf_mlp.load_reference(state_dict, "nerf_mlp.")
        if self.instance_obj:
            for cid in self._class_list:
                getattr(self, f"obj_mlp_{cid}").load_reference(state_dict, f"obj_mlp_{cid}.")
            with torch.no_grad():
                for t in range(len(self.class_ids)):
                    v = state_dict[f"latent_vector_dict.obj_latent_{t}"]
                    self.latent_vector_dict[f"obj_latent_{t}"].copy_(v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v)))
        return self

    def reference_state_dict(self) -> Dict[str, np.ndarray]:
        """Parameters under the reference's names (what `Model(mc, sd)` / `DynamicModel` and `checkpoints.save_checkpoint` take)."""
        skip = ("encoder.offsets", "encoder.grid_sizes", "encoder.idx", "tracks", "_class_rank")
        return {k: v.detach().cpu().numpy() for k, v in self.state_dict().items() if not k.endswith(skip)}

    def latent_reg(self, latent_reg: float = 0.001) -> torch.Tensor:
        """train.py:395-399 + train_utils.latentReg (:456-457): sum over the tracks of latent_reg * ||code||.  (sic) the reference
        builds it with `torch.tensor([...])` from Python floats: a VALUE in the loss dictionary that carries no gradient - reproduced."""
        z = [p.detach().norm() for p in self.latent_vector_dict.values()]
        return latent_reg * torch.stack(z).sum()

    # -- dynamic objects (models.py:401-477) --------------------------------------------------------------------------------------
    def _object_merge(self, o: Dict[str, torch.Tensor], rgbs: torch.Tensor, batch, tdist: torch.Tensor, box: torch.Tensor, last: bool,
                      refine=None):
        """Overwrite density / rgb / semantic of the samples inside the tracks' boxes with their ObjMLP's output.  Returns
        (density, rgbs, semantic, obj_mask).  Owner of a sample = the last track whose box holds the interval midpoint
        (`nlr_box_winner`; the reference's track loop overwrites earlier tracks; the owner map is data).  The box-frame points and
        directions carry no gradient, unless refine = (tracks, timestamps) is given (last level only): then they go through
        `_ObjFrame`, which leads back to a track tensor that requires a gradient (track refinement) and to the ray tensors of
        `batch` that require one (pose refinement)."""
        n, S = tdist.shape[0], tdist.shape[1] - 1
        dev = tdist.device
        origins = batch["origins"].reshape(n, 3).contiguous().float()
        dirs = batch["directions"].reshape(n, 3).contiguous().float()
        viewdirs = batch["viewdirs"].reshape(n, 3).contiguous().float()
        winner = torch.empty(n, S, dtype=torch.int32, device=dev)
        td = tdist.detach().contiguous()
        _lib.call("nlr_box_winner", td, origins, dirs, box, n, S, box.shape[1], winner)
        mask = winner >= 0
        density, sem = o["density"], o.get("semantic") if last else None
        sel = mask.nonzero()
        if sel.shape[0] == 0:
            return density, rgbs, sem, mask
        ri, si = sel[:, 0], sel[:, 1]
        tr = winner[ri, si].long()
        if refine is not None:
            p_all, d_all = _ObjFrame.apply(refine[0], refine[1], origins, dirs, viewdirs, td, box, ri, si, tr)
        else:  # (ray tensors that require a gradient are data here: proposal levels, models.py:447-449)
            p_all, d_all = box_frame(origins.detach(), dirs.detach(), viewdirs.detach(), td, box, ri, si, tr)
        table = torch.stack([self.latent_vector_dict[f"obj_latent_{t}"] for t in range(len(self.class_ids))])
        lat_all = table[tr]
        rank = self._class_rank[tr]
        density, rgbs = density.clone(), rgbs.clone()
        sem = sem.clone() if sem is not None else None
        for r_, cid in enumerate(self._class_list):
            pick = (rank == r_).nonzero()[:, 0]
            if pick.numel() == 0:
                continue
            res = getattr(self, f"obj_mlp_{cid}")(p_all[pick], d_all[pick], lat_all[pick])
            if not last:                                   # models.py:447-449: no gradient into the object networks from proposal levels
                res = {k: v.detach() for k, v in res.items()}
            density[ri[pick], si[pick]] = res["density"]
            rgbs[ri[pick], si[pick]] = res["rgb"]
            if sem is not None and "semantic" in res:
                sem[ri[pick], si[pick]] = res["semantic"]
        return density, rgbs, sem, mask

    def _fused_objects_begin(self, batch, n: int, dev):
        """What the fused object operator needs for every level of one forward: the plan (made on first use), the classes' tables and
        flat parameter buffers (packed into the kernels' weight images once per forward), the latent table, the ray descriptor."""
        mlps = [getattr(self, f"obj_mlp_{cid}") for cid in self._class_list]
        if self._obj_plan is None or self._obj_plan.device != torch.device(dev):
            self._obj_plan = _ObjTrainPlan(mlps, [self._class_list.index(c) for c in self.class_ids], self.mc.config.latent_size, dev)
        plan = self._obj_plan
        flats = [plan.flat(c, m) for c, m in enumerate(mlps)]
        plan.pack([f.detach() for f in flats])
        tables = [m.encoder.embeddings for m in mlps]
        latents = torch.stack([self.latent_vector_dict[f"obj_latent_{t}"] for t in range(len(self.class_ids))])
        rays_desc, keep = _lib.rays({k: batch[k].detach() for k in ("origins", "directions", "viewdirs")}, n, optional=_lib.RAY_KEYS)
        return plan, flats, tables, latents, rays_desc, keep

    def _object_merge_fused(self, o: Dict[str, torch.Tensor], rgbs: torch.Tensor, tdist: torch.Tensor, box: torch.Tensor, last: bool, state,
                            frame=()):
        """`_object_merge` through `nlr_obj_train_forward`: nothing is read back.  Proposal levels: the density-only form under no
        gradient (models.py:447-449), the static density keeps its gradient outside the boxes.  Last level: `_ObjectsFused`, with
        frame = (tracks, timestamps, origins, directions, viewdirs) when the box frame is to carry a gradient (`fused_object_frame`)."""
        plan, flats, tables, latents, rays_desc, keep = state
        td = tdist.detach().contiguous()
        density = o["density"]
        if not last:
            with torch.no_grad():
                dens = density.detach().float().clone(memory_format=torch.contiguous_format)
                winner = objects_forward(plan, [t.detach() for t in tables], latents.detach().float().contiguous(), rays_desc, td, box, dens)
            mask = winner >= 0
            return torch.where(mask, dens, density), rgbs, None, mask
        sem = o.get("semantic")
        use_sem = sem is not None and all(getattr(self, f"obj_mlp_{cid}").cfg.use_semantic for cid in self._class_list)
        dens, rgbs, sem_m, mask = _ObjectsFused.apply(plan, rays_desc, keep, td, box, density, rgbs, sem if use_sem else None, latents, *tables,
                                                      *flats, *frame)
        return dens, rgbs, sem_m if use_sem else sem, mask

    def forward(self, batch: Dict[str, torch.Tensor], train_frac: float = 1.0, rand: Optional[torch.Generator] = None, randomized: bool = False,
                sample_n: int = 7, sample_m: int = 3, curr_track=None, color_rays: Optional[int] = None, object_ray_grads: bool = False):
        """-> (renderings, ray_history), one entry per level, like `Model.forward`.  randomized (or a generator in `rand`): per-ray
        jitter of the sample positions (stepfun.py:216) and per-multisample rotation (render.py:150), as `model(True, ...)` draws
        them in train.py:272.
        color_rays: None, or the number n of leading rays with colour supervision; the NerfMLP level skips its view MLP for the
        rays [n, N) and renders them black (`TrainableNerfLevel.forward`).  The caller promises `batch['mask_rgb']` = 0 on those
        rays.  With `instance_obj` the object networks still write their own rgb into the samples they own on such rays: harmless,
        the loss masks those rays.
        object_ray_grads: with `instance_obj` and ray tensors that require a gradient (pose refinement), whether the last level's
        box-frame points and directions lead back to origins / directions / viewdirs (`_ObjFrame`, `nlr_obj_frame_backward_rays`).
        Off, such a call is refused: a gradient that silently misses the object samples is not the reference's.  `training_step`
        turns it on.  Values are the same bits either way; a batch of plain data ignores it."""
        mc = self.mc
        color_rays = _check_color_rays(color_rays, batch["origins"].shape[0])
        n = batch["origins"].shape[0]
        dev = batch["origins"].device
        near, far = batch["near"].reshape(n).contiguous().float(), batch["far"].reshape(n).contiguous().float()
        dirs = batch["directions"].reshape(n, 3).contiguous().float()
        randomized = randomized or rand is not None
        prev_s = prev_w = None
        n_prev = 0
        renderings, history = [], []
        n_levels = len(mc.level_samples())
        box = None
        ray_grads = self.instance_obj and rays_require_grad(batch)
        if ray_grads and not object_ray_grads:
            raise NotImplementedError("ray tensors that require a gradient (pose refinement) with instance_obj=True: the box-frame path "
                                      "of the dynamic-object branch leads back to origins / directions / viewdirs only on request, "
                                      "pass object_ray_grads=True")
        fused_obj = self.instance_obj and self.fused_objects
        if fused_obj and ray_grads and not self.fused_object_frame:
            raise NotImplementedError("fused_objects=True with ray tensors that require a gradient (pose refinement, object_ray_grads=True): "
                                      "the fused object operator has no box-frame gradient, use fused_objects=False or pass "
                                      "fused_object_frame=True")
        if self.instance_obj:
            if "timestamp" not in batch:
                raise RuntimeError("batch['timestamp'] is missing (ZI/models.py:315)")
            tracks = (self.tracks if curr_track is None else torch.as_tensor(curr_track, device=dev, dtype=torch.float32)).contiguous()
            ts = batch["timestamp"].reshape(-1).to(dev, torch.float32).contiguous()
            box = track_box_params(tracks, ts)  # (tracks and ts are kept in this form for `refine`: the adjoint reads the same two tensors)
            # track refinement (train.py:244-268): a track that requires a gradient gets one from the last level's object samples
            # pose refinement (train.py:199-243) on request: ray tensors that require one get theirs through the same samples
            refine = (tracks, ts) if (tracks.requires_grad and torch.is_grad_enabled()) or ray_grads else None
            if fused_obj and refine is not None and not self.fused_object_frame:
                raise NotImplementedError("fused_objects=True with tracks that require a gradient (track refinement): the fused object "
                                          "operator has no box-frame gradient, use fused_objects=False or pass fused_object_frame=True")
            if fused_obj:
                fused_state = self._fused_objects_begin(batch, n, dev)
                fused_frame = ()
                if refine is not None:  # the tensors the box frame is made of, as `_object_merge` reads them
                    fused_frame = (tracks, ts) + tuple(batch[k].reshape(n, 3).float() for k in ("origins", "directions", "viewdirs"))
        for li, ((S, dilation, anneal), level) in enumerate(zip(mc.level_schedule(train_frac), self.levels())):
            last = li == n_levels - 1
            sdist, tdist = torch.empty(n, S + 1, device=dev), torch.empty(n, S + 1, device=dev)
            jit = torch.rand(n, device=dev, generator=rand) if randomized else None
            _lib.call("nlr_resample_level", prev_s, prev_w, n_prev, dilation, anneal, mc.resample_padding, S, jit, near, far, mc.power_lambda, n,
                      sdist, tdist)
            rd = torch.rand(n, S, sample_n, device=dev, generator=rand) if randomized else None
            o = level(batch, tdist, sample_n, sample_m, rand_deg=rd, **({"color_rays": color_rays} if last else {}))
            rgbs = o["rgb"] if last else torch.zeros(n, S, 3, device=dev)   # a PropMLP renders black (models.py:1119-1122)
            obj_mask = None
            if box is not None:
                if fused_obj:
                    dens_m, rgbs, sem_m, obj_mask = self._object_merge_fused(o, rgbs, tdist, box, last, fused_state, fused_frame if last else ())
                else:
                    dens_m, rgbs, sem_m, obj_mask = self._object_merge(o, rgbs, batch, tdist, box, last, refine if last else None)
                o = dict(o, density=dens_m)
                if sem_m is not None:
                    o["semantic"] = sem_m
            # background colour (models.py:488-500): the range's value if it is a point, its midpoint for a deterministic render,
            # otherwise one uniform draw per ray and channel - composited here (the kernel's background is a scalar)
            lo_bg, hi_bg = mc.bg_intensity_range
            bg, bg_rand = mc.deterministic_bg(), None
            if randomized and lo_bg != hi_bg:
                bg, bg_rand = 0.0, torch.rand(n, 3, device=dev, generator=rand) * (hi_bg - lo_bg) + lo_bg
            r = volumetric_render(o["density"], tdist, dirs, rgbs, o.get("semantic") if last else None, o.get("intensity") if last else None,
                                  bool(mc.opaque_background), bg)
            if bg_rand is not None:
                r["rgb"] = r["rgb"] + (1.0 - r["acc"]).clamp_min(0.0)[:, None] * bg_rand   # render.py:226-229
            weights = r.pop("weights")
            renderings.append(r)
            history.append(dict(sdist=sdist, tdist=tdist, weights=weights, density=o["density"]))
            if obj_mask is not None:
                history[-1]["obj_mask"] = obj_mask
            prev_s, prev_w, n_prev = sdist, weights.detach().contiguous(), S
        return renderings, history


def clip_gradients(model: torch.nn.Module, grad_max_norm: float = 0.0, grad_max_val: float = 0.0) -> None:
    """train_utils.py:243-253: clip by global norm, then by value, then - unconditionally - replace NaN / +-Inf gradients by
    0 / the largest finite values (`param.grad.nan_to_num_()`), so that one degenerate ray cannot poison the Adam state."""
    if grad_max_norm > 0:
        torch.nn.utils.clip_grad_norm_(model.parameters(), grad_max_norm)
    if grad_max_val > 0:
        torch.nn.utils.clip_grad_value_(model.parameters(), grad_max_val)
    for p in model.parameters():
        if p.grad is not None:
            p.grad.nan_to_num_()


def learning_rate_decay(step: int, lr_init: float = 0.01, lr_final: float = 0.001, max_steps: int = 25000, lr_delay_steps: int = 5000,
                        lr_delay_mult: float = 1e-8) -> float:
    """ZI/math.py:54-85 with the defaults of ZI/configs.py:85-88: log-linear decay from lr_init to lr_final over max_steps, eased in
    over lr_delay_steps by `mult + (1 - mult) sin(pi/2 * step / delay)`."""
    delay = lr_delay_mult + (1 - lr_delay_mult) * float(np.sin(0.5 * np.pi * np.clip(step / lr_delay_steps, 0, 1))) if lr_delay_steps > 0 else 1.0
    t = float(np.clip(step / max_steps, 0, 1))
    return delay * float(np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t))


def create_optimizer(model: torch.nn.Module, lr_init: float = 0.01, lr_final: float = 0.001, max_steps: int = 25000, lr_delay_steps: int = 5000,
                     lr_delay_mult: float = 1e-8, adam_beta1: float = 0.9, adam_beta2: float = 0.99, adam_eps: float = 1e-15):
    """train_utils.py:256-275: Adam(betas = (0.9, 0.99), eps = 1e-15) over all parameters and the learning-rate function the loop
    writes into every param_group before each step (train.py:187-190).  Returns (optimizer, lr_fn)."""
    opt = torch.optim.Adam(model.parameters(), lr=lr_init, betas=(adam_beta1, adam_beta2), eps=adam_eps)
    return opt, (lambda step: learning_rate_decay(step, lr_init, lr_final, max_steps, lr_delay_steps, lr_delay_mult))


class TrackNet(torch.nn.Module):
    """`Track_opt` (ZI/posenet_v2.py:65-76) with the reference's parameter names, so its `tracknet_ckpt_*` files load: one yaw
    offset `opt_r` [n_obj, T, 1] and one translation offset `opt_t` [n_obj, T, 3] per recorded pose of every track, zeros at the
    start.  The recorded `tracks` [n_obj, T, 9] ride along as a buffer outside the state dict (the reference keeps them as a plain
    attribute).  forward() = the refined track of train.py:251-256."""

    def __init__(self, tracks):
        super().__init__()
        tracks = torch.as_tensor(np.asarray(tracks.detach().cpu() if isinstance(tracks, torch.Tensor) else tracks, np.float32))
        if tracks.dim() != 3 or tracks.shape[-1] != 9:
            raise ValueError(f"tracks must be [n_obj, T, 9] (center3, theta_z, wlh3, timestamp, id), got {tuple(tracks.shape)}")
        self.register_buffer("tracks", tracks, persistent=False)
        self.opt_r = torch.nn.Parameter(torch.zeros(tracks.shape[0], tracks.shape[1], 1))
        self.opt_t = torch.nn.Parameter(torch.zeros(tracks.shape[0], tracks.shape[1], 3))

    def forward(self) -> torch.Tensor:
        track = self.tracks.clone()
        track[:, :, :3] = self.tracks[:, :, :3] + self.opt_t
        track[:, :, 3:4] = self.tracks[:, :, 3:4] + self.opt_r
        return track


TRACK_OPT_STEPS = 5000  # length of the refinement window (train.py:245,257,468: a literal there)


def create_tracknet(tracks, track_start_opt: int = 5000, max_steps: int = 25000, tn_lr_init: float = 1e-4, tn_lr_final: float = 1e-5,
                    lr_delay_steps: int = 5000, lr_delay_mult: float = 1e-8, adam_beta1: float = 0.9, adam_beta2: float = 0.99,
                    adam_eps: float = 1e-15):
    """train_utils.py:304-327: the TrackNet, its Adam (betas and eps of `create_optimizer`) and its learning-rate function, the
    main schedule shifted to the start of the window: learning_rate_decay(step - start, max_steps = max_steps - start).
    Returns (tracknet, optimizer, lr_fn)."""
    net = TrackNet(tracks)
    opt = torch.optim.Adam(net.parameters(), lr=tn_lr_init, betas=(adam_beta1, adam_beta2), eps=adam_eps)
    return net, opt, (lambda step: learning_rate_decay(step - track_start_opt, tn_lr_init, tn_lr_final, max_steps - track_start_opt,
                                                       lr_delay_steps, lr_delay_mult))


def track_phase(step: Optional[int], track_start_opt: int = 5000) -> str:
    """Where `step` lies relative to the refinement window of train.py:245-266: 'before' (the model renders its recorded tracks),
    'refine' for start < step < start + 5000 (refined track with gradient), 'frozen' for step > start + 5000 (refined track under
    no_grad).  (sic) step == start + 5000 matches neither comparison of the reference and renders the recorded tracks once more."""
    if step is None:
        raise ValueError("track refinement needs the step number (training_step(..., step=))")
    if track_start_opt < step < track_start_opt + TRACK_OPT_STEPS:
        return "refine"
    return "frozen" if step > track_start_opt + TRACK_OPT_STEPS else "before"


def current_track(tracknet: Optional[TrackNet], step: Optional[int], track_start_opt: int = 5000) -> Optional[torch.Tensor]:
    """The `curr_track` of train.py:244-268 for this step: None before the window (and without a TrackNet), the refined track with
    gradient inside it, the refined track without one after it."""
    if tracknet is None:
        return None
    phase = track_phase(step, track_start_opt)
    if phase == "refine":
        return tracknet()
    if phase == "frozen":
        with torch.no_grad():
            return tracknet()
    return None


class PoseNet(torch.nn.Module):
    """`LearnPose` (ZI/posenet_v2.py:78-121) with the reference's parameter names, so its `posenet_ckpt_*` files load: one
    axis-angle rotation `r` and one translation `t` per pose, the `num_cams` camera poses first and the `num_lidars` LiDAR poses
    behind them (`batch['glo_idx']` indexes this list), zeros at the start - the identity.  forward(ids) -> [len(ids), 4, 4], the
    correction make_c2w(r, t * t_ratio) of each id, right-multiplied by `init_c2w[id]` when initial poses were given."""

    def __init__(self, num_cams: int, num_lidars: int = 1, learn_R: bool = True, learn_t: bool = True, init_c2w=None, t_ratio: float = 1.0):
        super().__init__()
        self.num_cams, self.num_lidars, self.t_ratio = int(num_cams), int(num_lidars), t_ratio
        n = self.num_cams + self.num_lidars
        self.init_c2w = None
        if init_c2w is not None:
            self.init_c2w = torch.nn.Parameter(torch.as_tensor(init_c2w), requires_grad=False)
        self.r = torch.nn.Parameter(torch.zeros(n, 3), requires_grad=bool(learn_R))
        self.t = torch.nn.Parameter(torch.zeros(n, 3), requires_grad=bool(learn_t))

    def rotations(self) -> torch.Tensor:
        """Rodrigues' formula as posenet_v2.Exp writes it: I + sin|r| / |r| K + (1 - cos|r|) / |r|^2 K^2 with |r| + 1e-15."""
        r = self.r
        zero = torch.zeros_like(r[:, :1])
        K = torch.stack([torch.cat([zero, -r[:, 2:3], r[:, 1:2]], 1), torch.cat([r[:, 2:3], zero, -r[:, 0:1]], 1),
                         torch.cat([-r[:, 1:2], r[:, 0:1], zero], 1)], dim=1)
        a = r.norm(dim=-1)[:, None, None] + 1e-15
        return torch.eye(3, dtype=r.dtype, device=r.device)[None] + (torch.sin(a) / a) * K + ((1 - torch.cos(a)) / a ** 2) * (K @ K)

    def forward(self, ids: torch.Tensor) -> torch.Tensor:
        top = torch.cat([self.rotations(), (self.t * self.t_ratio).unsqueeze(2)], dim=2)             # [n, 3, 4]
        bottom = torch.zeros_like(top[:, :1])
        bottom[:, 0, 3] = 1.0
        ids = ids.reshape(-1).long()
        c2w = torch.cat([top, bottom], dim=1)[ids]
        return c2w if self.init_c2w is None else c2w @ self.init_c2w[ids]


def create_posenet(num_poses: int, num_lidars: int = 0, start_step: int = 10000, end_step: int = 20000, pn_lr_init: float = 4e-5,
                   pn_lr_final: float = 2e-6, t_ratio: float = 0.25, learn_R: bool = True, learn_t: bool = True, lr_delay_steps: int = 5000,
                   lr_delay_mult: float = 1e-8, adam_beta1: float = 0.9, adam_beta2: float = 0.99, adam_eps: float = 1e-15):
    """train_utils.py:278-301 with the defaults of configs.py:151-161: the PoseNet, its Adam (betas and eps of `create_optimizer`)
    and its learning-rate function, the main schedule shifted to the window: learning_rate_decay(step - start_step, max_steps =
    end_step - start_step).  Returns (posenet, optimizer, lr_fn)."""
    net = PoseNet(num_poses, num_lidars=num_lidars, learn_R=learn_R, learn_t=learn_t, t_ratio=t_ratio)
    opt = torch.optim.Adam(net.parameters(), lr=pn_lr_init, betas=(adam_beta1, adam_beta2), eps=adam_eps)
    return net, opt, (lambda step: learning_rate_decay(step - start_step, pn_lr_init, pn_lr_final, end_step - start_step, lr_delay_steps,
                                                       lr_delay_mult))


def refine_batch(batch: Dict[str, torch.Tensor], poses: torch.Tensor) -> Dict[str, torch.Tensor]:
    """train.py:207-221: a copy of `batch` with `origins` translated by poses[:, :3, 3] and `directions`, `viewdirs`, `base_x`,
    `base_y` (and `normals` when present) rotated by poses[:, :3, :3]; poses [N, 4, 4], one per ray.  The caller's dict and its
    tensors stay as they are."""
    n = batch["origins"].shape[:1]
    out = dict(batch)
    out["origins"] = batch["origins"] + poses[:, :3, 3].reshape(*n, 3)
    for k in ("directions", "viewdirs", "base_x", "base_y", "normals"):
        if k in batch:
            out[k] = (batch[k].reshape(-1, 1, 3) * poses[:, :3, :3]).sum(-1).reshape(*n, 3)
    return out


def pose_phase(step: Optional[int], pose_window=(10000, 20000)) -> str:
    """Where `step` lies relative to the window of train.py:201-243: 'refine' for start < step < end (refined batch with gradient),
    'frozen' for step > end (refined batch under no_grad), 'before' otherwise.  (sic) step == start and step == end match none of
    the reference's comparisons: the batch stays as it is."""
    if step is None:
        raise ValueError("pose refinement needs the step number (training_step(..., step=))")
    start, end = pose_window
    if start < step < end:
        return "refine"
    return "frozen" if step > end else "before"


def loss_lambdas(step: int, pose_window=(10000, 20000), pose_refine: bool = True) -> Dict[str, float]:
    """The weights of the depth and semantic terms over the run (train.py:331-333,404-405) as keywords of `losses.total_loss`:
    0 while the poses settle (start < step < int(0.6 * end), only with pose refinement), the full 0.4 / 0.04 after the window,
    0.1 / 0.01 otherwise."""
    start, end = pose_window
    if pose_refine and start < step < int(0.6 * end):
        return {"depth_lam": 0.0, "sem_lam": 0.0}
    return {"depth_lam": 0.4, "sem_lam": 0.04} if step > end else {"depth_lam": 0.1, "sem_lam": 0.01}


def pose_batch(batch, posenet: Optional[PoseNet], step: Optional[int], pose_window=(10000, 20000)):
    """The batch of train.py:199-243 for this step: itself before the window (and without a PoseNet), refined with gradient inside
    it, refined without one after it.  `batch['glo_idx']` names every ray's pose."""
    if posenet is None:
        return batch
    phase = pose_phase(step, pose_window)
    if phase == "before":
        return batch
    with torch.enable_grad() if phase == "refine" else torch.no_grad():
        return refine_batch(batch, posenet(batch["glo_idx"].reshape(-1).int()))


def training_step(model: TrainableModel, optimizer: torch.optim.Optimizer, batch: Dict[str, torch.Tensor], train_frac: float = 1.0,
                  randomized: bool = True, hash_decay_mult: float = 0.1, tv_weight: float = 0.0, grad_max_norm: float = 0.0,
                  grad_max_val: float = 0.0, latent_reg: float = 0.001, as_tensors: bool = False, color_rays: Optional[int] = None,
                  check_color_rays: bool = False, tracknet: Optional[TrackNet] = None, tn_optimizer: Optional[torch.optim.Optimizer] = None,
                  tn_lr_fn=None, step: Optional[int] = None, track_start_opt: int = 5000, posenet: Optional[PoseNet] = None,
                  pn_optimizer: Optional[torch.optim.Optimizer] = None, pn_lr_fn=None, pose_window=(10000, 20000), **loss_kw):
    """One optimiser step as train.py:272-459 takes it: forward with random jitter, the loss dictionary (`losses.total_loss` +
    hash decay), backward through the HIP backward kernels, optional total-variation gradient on the tables (grid.py:176-198),
    gradient clipping incl. the unconditional nan_to_num_ (train_utils.clip_gradients), step.  Returns the loss terms as floats, or
    with `as_tensors` as detached device scalars: reading them is the only host synchronisation of a step (without object tracks, or
    with them on a `TrainableModel(fused_objects=True)`; the torch object merge reads its owner lists back on every level), so a
    loop that logs every n-th step keeps the next step's launches ahead of the GPU in between.  Inside the refinement windows the
    same holds on a `TrainableModel(fused_objects=True, fused_object_frame=True)`: the box-frame cotangents of the fused object
    operator reach the TrackNet and the refined rays as a dense list over all samples, without a count or an index list on the host.
    color_rays: None, or the number n of leading rays with colour supervision (`TrainableModel.forward`): the caller promises
    `batch['mask_rgb']` = 0 on the rays [n, N), as train.py:316-320 sets it for the LiDAR rays at the end of a batch
    (`losses.nusc_masks(lidar_supervision=True)` and `scene.supervise(colourless=..)` build such masks).  check_color_rays (off by default: it reads the mask back, one host
    synchronisation) verifies the promise and raises ValueError when it is broken.
    tracknet / tn_optimizer / tn_lr_fn (`create_tracknet`) with `step`: track refinement as train.py:244-268,468-471 runs it.  Before
    the window (step <= track_start_opt) the model renders its recorded tracks; inside it the TrackNet's learning rate is set, its
    gradients are zeroed, the model renders the refined track with gradient and, after the model's own step, the TrackNet's
    gradients are clipped (the same `clip_gradients`) and its optimiser steps; after it the model renders the refined track under
    no_grad.  Without a tracknet the step is the one described above.
    posenet / pn_optimizer / pn_lr_fn (`create_posenet`) with `step` and pose_window = (start_step, end_step): pose refinement as
    train.py:199-243,463-466 runs it.  Before the window the batch is rendered as it is; inside it the PoseNet's learning rate is set,
    its gradients are zeroed, the batch is refined with gradient (`refine_batch`; the caller's batch is not modified), the loss
    reaches the PoseNet through the ray tensors and, after the model's own step, its gradients are clipped and its optimiser steps;
    after it the batch is refined under no_grad.  The depth and semantic weights follow `loss_lambdas` unless given.  A model with
    `instance_obj` is called with `object_ray_grads=True`, so the refined rays also get the share of the samples inside the tracks'
    boxes; with a tracknet as well both refinements run from the one forward, as train.py:199-268 does."""
    from . import losses as nlosses
    if check_color_rays and color_rays is not None:
        nlosses.check_colourless(batch, color_rays)
    refining = tracknet is not None and track_phase(step, track_start_opt) == "refine"
    if refining:
        if tn_optimizer is None or tn_lr_fn is None:
            raise ValueError("track refinement inside the window needs tn_optimizer and tn_lr_fn (create_tracknet)")
        for group in tn_optimizer.param_groups:
            group["lr"] = tn_lr_fn(step)
        tn_optimizer.zero_grad()
    posing = posenet is not None and pose_phase(step, pose_window) == "refine"
    if posing:
        if pn_optimizer is None or pn_lr_fn is None:
            raise ValueError("pose refinement inside the window needs pn_optimizer and pn_lr_fn (create_posenet)")
        for group in pn_optimizer.param_groups:
            group["lr"] = pn_lr_fn(step)
        pn_optimizer.zero_grad()
    if posenet is not None:
        batch = pose_batch(batch, posenet, step, pose_window)
        loss_kw = {**loss_lambdas(step, pose_window), **loss_kw}
    optimizer.zero_grad(set_to_none=True)
    track_kw = {} if tracknet is None else {"curr_track": current_track(tracknet, step, track_start_opt)}
    if posenet is not None and getattr(model, "instance_obj", False):  # the refined rays reach the object samples too (train.py:199-268)
        track_kw["object_ray_grads"] = True
    renderings, history = model(batch, train_frac=train_frac, randomized=randomized, color_rays=color_rays, **track_kw)
    terms = nlosses.total_loss(renderings, history, batch, **loss_kw)
    if hash_decay_mult > 0:  # (Config.obj_nodecay, nuscenes_single.gin:24: the object grids stay out)
        terms["hash_decay"] = hash_decay_loss([lv.encoder for lv in model.levels()], hash_decay_mult)
    if getattr(model, "instance_obj", False):
        terms["latent_reg"] = model.latent_reg(latent_reg)
    loss = sum(terms.values())
    loss.backward()
    if tv_weight > 0:
        for lv in model.levels():
            lv.encoder.grad_total_variation(tv_weight)
    clip_gradients(model, grad_max_norm, grad_max_val)
    optimizer.step()
    if refining:
        clip_gradients(tracknet, grad_max_norm, grad_max_val)
        tn_optimizer.step()
    if posing:
        clip_gradients(posenet, grad_max_norm, grad_max_val)
        pn_optimizer.step()
    out = {k: v.detach() for k, v in terms.items()}
    out["loss"] = loss.detach()
    return out if as_tensors else {k: float(v) for k, v in out.items()}
