"""Host-side mirror of the reference's render entry points, running on libnerflidar_hip.so.

`Model.forward` and `render_image` keep the signatures and return structures of
ZI/models.py:239-251,576 and ZI/models.py:1379-1507; all arithmetic of the level loop (resample ->
cast -> encode -> MLP -> composite) happens in one `nlr_render_rays` call per chunk.  PyTorch is
used only for device memory and streams.  There is no eager/CPU fallback: without the HIP
library or without a GPU these classes raise.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib
from .config import MLPConfig, ModelConfig
from .weights import grid_layout, mlp_names, mlp_param_shapes

_RAY_KEYS = _lib.RAY_KEYS
# the reference builds every MLP's GridEncoder with its defaults (hash, align_corners=False, linear; ZI/models.py:868): one statement
# for the render descriptor and for the encoder the normals operator is handed
_GRID_OPTIONS = dict(gridtype=0, align_corners=0, interp=0)


def _f32c(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


class Model:
    """Drop-in for ZI/models.py:Model at inference (instance_obj=False, num_glo_features=0).

    Args:
      mc: ModelConfig (gin names).  state_dict: reference-keyed parameters (numpy or torch, any
      device); hash tables are kept as float32 (or float16 if `table_dtype=torch.float16`) CUDA
      tensors in `self.tables[prefix]`, MLP weights are packed once into MFMA fragment order by
      `nlr_model_create`.
    """

    def __init__(self, mc: ModelConfig, state_dict: Dict[str, object], device="cuda:0",
                 precision: int = _lib.PREC_FAST, table_dtype=torch.float32):
        if mc.config.instance_obj:
            raise NotImplementedError("instance_obj=True (dynamic-object branch, ZI/models.py:306-315,401-477) "
                                      "is outside the fused path (SURVEY section 8f-1)")
        if mc.raydist_fn != "power_transformation":
            raise NotImplementedError("only raydist_fn='power_transformation' (the gin value) is supported")
        self.mc = mc
        self.config = mc.config
        self.device = torch.device(device)
        self.precision = precision
        self.training = False
        # performance hint (NlrRenderCfg.shuffled_rays, no effect on results): False = consecutive rays of a batch are neighbours in
        # space (sweeps, image tiles), the encode kernels then walk 8 adjacent rays together; True for shuffled batches
        self.shuffled_rays = False
        self.num_levels = mc.num_levels
        self.tables: Dict[str, torch.Tensor] = {}
        self._keep = []  # host arrays referenced by the descriptor during nlr_model_create
        self._handle = C.c_void_p(None)
        self._ws: Optional[torch.Tensor] = None
        sd = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in state_dict.items()}
        desc = _lib.NlrModelDesc()
        desc.num_levels = mc.num_levels
        samples = mc.level_samples()
        mlp_descs = []
        for li, (prefix, cfg) in enumerate(mlp_names(mc)):
            desc.num_samples[li] = samples[li]
            md = self._mlp_desc(prefix, cfg, sd, table_dtype)
            mlp_descs.append(md)
            desc.mlps[li] = C.pointer(md)
        desc.dilation_multiplier = mc.dilation_multiplier
        desc.dilation_bias = mc.dilation_bias
        desc.anneal_slope = mc.anneal_slope
        desc.resample_padding = mc.resample_padding
        desc.power_lambda = mc.power_lambda
        desc.std_scale = mc.std_scale
        lo, hi = mc.bg_intensity_range
        desc.bg_intensity = lo if lo == hi else (lo + hi) / 2  # models.py:488-493 (deterministic render)
        desc.opaque_background = int(mc.opaque_background)
        desc.mlp_precision = precision
        _lib.call("nlr_model_create", desc, self._handle, device=self.device)
        self._keep.clear()
        # density normals (ZI/models.py:1070-1094): device f32 copies of the last level's density layers and its grid, for the operator
        # of normals.py, which runs after the render and is f32 whatever `precision` is.  Off (the default): nothing is kept.
        self._normals = None
        if not mc.nerf_mlp.disable_density_normals:
            if not mc.config.analytic_gradient:
                raise NotImplementedError("Config.analytic_gradient = False with NerfMLP.disable_density_normals = False asks for the "
                                          "finite-difference normals (ZI/models.py:1097-1100), which are outside the fused path")
            self._normals = self._normals_state(list(mlp_names(mc))[-1], sd)

    @property
    def has_density_normals(self) -> bool:
        """Was the model built with `NerfMLP.disable_density_normals = False`?  Its history and extras then carry normals."""
        return self._normals is not None

    def _normals_state(self, last, sd):
        """What `normals.density_normals` takes besides rays, tdist and weights: the last level's encoder (duck type of
        `training.encode_features_fused`) over the model's own table, and density_layer.0 / row 0 of density_layer.2 on the device."""
        from types import SimpleNamespace
        prefix, cfg = last
        offsets, _, pls = grid_layout(cfg)
        enc = SimpleNamespace(num_levels=cfg.grid_num_levels, output_dim=cfg.grid_num_levels * cfg.grid_level_dim,
                              base_resolution=cfg.grid_base_resolution, per_level_scale=float(pls),
                              _offsets_host=torch.from_numpy(np.ascontiguousarray(offsets, np.int32)), gridtype_id=_GRID_OPTIONS["gridtype"],
                              align_corners=bool(_GRID_OPTIONS["align_corners"]), interp_id=_GRID_OPTIONS["interp"], embeddings=self.tables[prefix])
        dev = lambda a: torch.from_numpy(_f32c(a)).to(self.device)
        return SimpleNamespace(encoder=enc, w0=dev(sd[f"{prefix}.density_layer.0.weight"]), b0=dev(sd[f"{prefix}.density_layer.0.bias"]),
                               w2=dev(sd[f"{prefix}.density_layer.2.weight"][0]), re_weights=bool(cfg.re_weights))

    # -- descriptor assembly ---------------------------------------------------------------------
    def _linear(self, sd, name) -> _lib.NlrLinear:
        w, b = _f32c(sd[name + ".weight"]), _f32c(sd[name + ".bias"])
        self._keep += [w, b]
        l = _lib.NlrLinear()
        l.weight = w.ctypes.data
        l.bias = b.ctypes.data
        l.out_features, l.in_features = w.shape
        return l

    def _mlp_desc(self, prefix: str, cfg: MLPConfig, sd, table_dtype) -> _lib.NlrMlpDesc:
        md = _lib.NlrMlpDesc()
        offsets, _, pls = grid_layout(cfg)
        emb = sd[f"{prefix}.encoder.embeddings"]
        if emb.shape != (int(offsets[-1]), cfg.grid_level_dim):
            raise RuntimeError(f"{prefix}.encoder.embeddings has shape {emb.shape}, expected "
                               f"{(int(offsets[-1]), cfg.grid_level_dim)}")
        table = torch.from_numpy(_f32c(emb)).to(self.device, table_dtype).contiguous()
        self.tables[prefix] = table
        off = np.ascontiguousarray(offsets, np.int32)
        self._keep.append(off)
        g = md.grid
        g.table = table.data_ptr()
        g.table_dtype = 0 if table_dtype == torch.float32 else 1
        g.num_levels, g.level_dim = cfg.grid_num_levels, cfg.grid_level_dim
        g.base_resolution = cfg.grid_base_resolution
        g.log2_per_level_scale = float(np.log2(pls))
        g.offsets = off.ctypes.data
        g.gridtype, g.align_corners, g.interp = _GRID_OPTIONS["gridtype"], _GRID_OPTIONS["align_corners"], _GRID_OPTIONS["interp"]
        md.density0 = self._linear(sd, f"{prefix}.density_layer.0")
        md.density2 = self._linear(sd, f"{prefix}.density_layer.2")
        md.disable_rgb = int(cfg.disable_rgb)
        md.bottleneck_width = cfg.bottleneck_width
        md.net_depth_viewdirs, md.net_width_viewdirs = cfg.net_depth_viewdirs, cfg.net_width_viewdirs
        md.skip_layer_dir, md.deg_view = cfg.skip_layer_dir, cfg.deg_view
        md.density_bias, md.rgb_premultiplier = cfg.density_bias, cfg.rgb_premultiplier
        md.rgb_bias, md.rgb_padding = cfg.rgb_bias, cfg.rgb_padding
        md.re_weights = int(cfg.re_weights)
        md.class_num = cfg.class_num
        if not cfg.disable_rgb:
            if cfg.net_depth_viewdirs > _lib.NLR_MAX_VIEW_DEPTH:
                raise RuntimeError("net_depth_viewdirs too large")
            for i in range(cfg.net_depth_viewdirs):
                md.view[i] = self._linear(sd, f"{prefix}.lin_second_stage_{i}")
            md.rgb_layer = self._linear(sd, f"{prefix}.rgb_layer")
            md.use_semantic, md.no_sem_layer = int(cfg.use_semantic), int(cfg.no_sem_layer)
            if cfg.use_semantic and not cfg.no_sem_layer:
                md.sem0 = self._linear(sd, f"{prefix}.sem_layer.0")
                md.sem2 = self._linear(sd, f"{prefix}.sem_layer.2")
            md.use_intensity = int(cfg.use_intensity)
            if cfg.use_intensity:
                md.int0 = self._linear(sd, f"{prefix}.intensity_layer.0")
                md.int2 = self._linear(sd, f"{prefix}.intensity_layer.2")
        return md

    def __del__(self):
        try:
            if self._handle:
                _lib.lib().nlr_model_destroy(self._handle)
                self._handle = C.c_void_p(None)
        except Exception:
            pass

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        self.training = mode
        return self

    # -- the fused op --------------------------------------------------------------------------
    def _workspace(self, n: int) -> torch.Tensor:
        need = _lib.lib().nlr_workspace_bytes(self._handle, n)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _render_call(self, rays, n: int, cfg, out, lidar_only: bool = False) -> None:
        """The library call of `render_rays` (DynamicModel substitutes nlr_render_rays_dynamic / nlr_render_lidar_dynamic)."""
        ws = self._workspace(n)
        _lib.call("nlr_render_lidar" if lidar_only else "nlr_render_rays", self._handle, rays, n, cfg, out, ws, ws.numel())

    def render_rays(self, batch: Dict[str, torch.Tensor], train_frac: float = 1.0, compute_extras: bool = True,
                    sample_n: int = 7, sample_m: int = 3, want_history: bool = False, scale_factor: float = 0.0,
                    rand_jitter: Optional[List[torch.Tensor]] = None, rand_deg: Optional[List[torch.Tensor]] = None,
                    packed: Optional[torch.Tensor] = None, lidar_only: bool = False):
        """One `nlr_render_rays` call.  Returns (rendering dict of the last level, list of per-level dicts).

        lidar_only: one `nlr_render_lidar` call instead - for a caller that reads depth / semantic / intensity / labels / points and
        no colour.  Every other output is the same bits; the direction encoding and the view MLP are not run, `batch["viewdirs"]`
        is not needed, the dicts carry no "rgb" and slots 3..5 of a `packed` record hold 0.

        packed: optional float32 CUDA buffer for the 7-float-per-ray records (depth, intensity, acc, rgb, label) the
        compositing kernel writes besides the named outputs: shape [n, 7] (ray order) or [wp, H, 7] with wp * H == n
        (azimuth-major tile of a beam-major [H, wp] sector, see sharding.py); returned as r["packed"]."""
        n = batch["origins"].shape[0]
        rays, ray_keep = _lib.rays(batch, n, optional=("viewdirs",) if lidar_only else ())
        keep = [ray_keep]  # tensors whose addresses the descriptors carry
        dev, f32 = self.device, torch.float32
        K = self.mc.nerf_mlp.class_num if self.config.use_semantic else 0
        new = lambda *shape, dtype=f32: torch.empty(*shape, device=dev, dtype=dtype)
        out = _lib.NlrOut()
        r: Dict[str, torch.Tensor] = {"depth": new(n)} if lidar_only else {"rgb": new(n, 3), "depth": new(n)}
        if K:
            r["semantic"] = new(n, K)
        if self.config.use_intensity:
            r["intensity"] = new(n)
        if compute_extras:
            for k in ("acc", "distance_mean", "distance_median", "distance_percentile_5", "distance_percentile_95"):
                r[k] = new(n)
        if scale_factor > 0:
            r["points"] = new(n, 3)
            if K:
                r["labels"] = new(n, dtype=torch.int32)
        for k, t in r.items():
            setattr(out, k, t.data_ptr())
        if packed is not None:
            if not (packed.is_cuda and packed.dtype == f32 and packed.is_contiguous() and packed.numel() == n * 7):
                raise RuntimeError("packed must be a contiguous float32 CUDA tensor with 7 values per ray")
            out.packed = packed.data_ptr()
            if packed.dim() == 3:
                out.packed_w, out.packed_h = int(packed.shape[0]), int(packed.shape[1])
            r["packed"] = packed
        hist: List[Dict[str, torch.Tensor]] = []
        samples = self.mc.level_samples()
        for li, S in enumerate(samples):
            h: Dict[str, torch.Tensor] = {"depth": new(n)}
            if want_history:
                h.update(sdist=new(n, S + 1), tdist=new(n, S + 1), weights=new(n, S), density=new(n, S))
                if li < len(samples) - 1:  # the rest of a proposal level's rendering dict (ZI/models.py:514-531)
                    h.update(r_rgb=new(n, 3), r_acc=new(n))
                    if compute_extras:
                        for k in ("distance_mean", "distance_median", "distance_percentile_5", "distance_percentile_95"):
                            h["r_" + k] = new(n)
                if li == len(samples) - 1:  # the library writes per-sample heads channel-/class-major
                    if not lidar_only:
                        h["rgb"] = new(3, n, S)
                    if K:
                        h["semantic"] = new(K, n, S)
                    if self.config.use_intensity:
                        h["intensity"] = new(n, S)
            for k, t in h.items():
                setattr(out.history[li], k, t.data_ptr())
            hist.append(h)
        cfg = _lib.NlrRenderCfg()
        cfg.train_frac = float(train_frac)
        cfg.compute_extras = int(compute_extras)
        cfg.sample_n, cfg.sample_m = sample_n, sample_m
        cfg.scale_factor = float(scale_factor)
        cfg.shuffled_rays = int(bool(getattr(self, "shuffled_rays", False)))
        for li in range(len(samples)):
            if rand_jitter is not None:
                t = rand_jitter[li].reshape(n).contiguous().float()
                keep.append(t)
                cfg.rand_jitter[li] = t.data_ptr()
            if rand_deg is not None:
                t = rand_deg[li].reshape(n, samples[li], sample_n).contiguous().float()
                keep.append(t)
                cfg.rand_deg[li] = t.data_ptr()
        self._render_call(rays, n, cfg, out, lidar_only)
        if want_history:  # back to the reference's [N, S, C] layout (ZI/models.py:553-557)
            last = hist[-1]
            if self._normals is not None:  # ZI/models.py:1082-1094, :525-529: after the render, on the last level's own tdist / weights / rand_deg
                from .normals import density_normals
                ns = self._normals
                got = density_normals(ns.encoder, batch, last["tdist"], ns.w0, ns.b0, ns.w2, weights=last["weights"], sample_n=sample_n,
                                      sample_m=sample_m, std_scale=self.mc.std_scale, rand_deg=None if rand_deg is None else rand_deg[-1],
                                      re_weights=ns.re_weights, want=("raw_grad", "normals") + (("ray_normals",) if compute_extras else ()))
                last["normals"], last["raw_grad_density"] = got["normals"], got["raw_grad"]
                if compute_extras:
                    r["normals"] = got["ray_normals"]
            if "rgb" in last:
                last["rgb"] = last["rgb"].permute(1, 2, 0)
            if "semantic" in last:
                last["semantic"] = last["semantic"].permute(1, 2, 0)
        return r, hist

    # -- reference-compatible call --------------------------------------------------------------
    def forward(self, rand, batch, train_frac, compute_extras, zero_glo=True, sample_n=7, sample_m=3, step=0,
                max_step=25000, curr_track=None):
        """ZI/models.py:239-576.  Returns (renderings, ray_history), one entry per level.

        `rand`: falsy for deterministic rendering; otherwise a torch.Generator (or True) used to draw the
        per-ray jitter (stepfun.py:216) and per-multisample rotation (render.py:150) on the device.
        Every level's `renderings` entry carries the reference's keys (rgb, depth, acc, distance_* with compute_extras,
        ray_* bundles; semantic / intensity on the last level only, models.py:514-531).
        This is the reference's contract, rgb included: the LiDAR-only mode is an option of `render_rays` alone, and `render_image`,
        which calls this, does not have it either.
        """
        n = batch["origins"].shape[0]
        samples = self.mc.level_samples()
        rj = rd = None
        if rand:
            gen = rand if isinstance(rand, torch.Generator) else None
            rj = [torch.rand(n, 1, device=self.device, generator=gen) for _ in samples]
            rd = [torch.rand(n, S, sample_n, device=self.device, generator=gen) for S in samples]
        r, hist = self.render_rays(batch, train_frac, compute_extras, sample_n, sample_m, want_history=True,
                                   rand_jitter=rj, rand_deg=rd)
        renderings = []
        for li, h in enumerate(hist):
            last = li == len(hist) - 1
            rend = dict(r) if last else dict(depth=h["depth"], **{k[2:]: v for k, v in h.items() if k.startswith("r_")})
            if compute_extras:
                nv = self.config.vis_num_rays
                rend["ray_sdist"] = h["sdist"][:nv]
                rend["ray_weights"] = h["weights"][:nv]
                rend["ray_rgbs"] = hist[-1]["rgb"][:nv] if last else None
            renderings.append(rend)
        if compute_extras:  # models.py:559-570: proposal levels show the final average colour
            final_rgb = torch.sum(renderings[-1]["ray_rgbs"] * renderings[-1]["ray_weights"][..., None], dim=-2)
            for li in range(len(hist) - 1):
                S = samples[li]
                renderings[li]["ray_rgbs"] = torch.broadcast_to(final_rgb[:, None, :], (final_rgb.shape[0], S, 3))
        ray_history = [{k: v for k, v in h.items() if k != "depth" and not k.startswith("r_")} for h in hist]
        return renderings, ray_history

    __call__ = forward


class CapturedRender:
    """One `Model.render_rays` call (the whole static sweep: ~10 kernel launches, no host read-back) captured into a HIP graph.

    A LiDAR simulator renders sweep after sweep from ray buffers it refills in place, so the launch sequence never changes; replaying
    it costs one graph launch instead of ~10 kernel launches plus their argument marshalling (at 8 azimuth sectors a rank's step is
    ~1 ms of GPU work against ~0.3 ms of host enqueue).  The ray batch, the optional `packed` tile and the returned output
    tensors are the buffers of the captured call: refill the inputs in place, `replay()`, read `out` / `hist`.  Keywords go to
    `render_rays` unchanged (`lidar_only=True` captures the LiDAR-only sweep: `out` then has no "rgb").

    The captured launches carry the raw address of the workspace arena (per-level intermediates).  The capture therefore OWNS that
    arena: it is allocated for this capture, kept alive by it, and detached from the model, so that a later eager `render_rays` -
    larger, or on another stream - allocates and uses its own arena instead of freeing or racing the one the graph writes.  Replays of
    ONE capture must still be ordered with respect to each other (same stream, or events), like any kernel sequence over fixed buffers."""

    def __init__(self, model: "Model", batch: Dict[str, torch.Tensor], **kw):
        if model.has_density_normals:
            raise NotImplementedError("CapturedRender of a model with NerfMLP.disable_density_normals = False: the normals operator allocates "
                                      "its outputs and workspace per call and is not part of a captured sweep")
        self.model, self.batch = model, batch
        side = torch.cuda.Stream(model.device)
        self.graph = torch.cuda.CUDAGraph()
        model._ws = None                     # a private arena for this capture (the model's previous one is released)
        with torch.cuda.stream(side):
            model.render_rays(batch, **kw)  # sizes the workspace outside the capture
            side.synchronize()
            with torch.cuda.graph(self.graph, stream=side):
                self.out, self.hist = model.render_rays(batch, **kw)
        self._ws = model._ws                 # the address baked into the graph: alive as long as the capture is
        model._ws = None                     # eager calls get their own
        torch.cuda.current_stream(model.device).wait_stream(side)

    def replay(self):
        """Enqueue the captured sweep on the current stream; returns the (static) output dict."""
        self.graph.replay()
        return self.out


class _SingleProcess:
    """Stand-in for accelerate.Accelerator when rendering in one process."""
    process_index = 0
    num_processes = 1
    is_main_process = True

    def gather(self, t):
        return t


def _chunk_plan(total: int, chunk: int, world: int, rank: int):
    """Static schedule of a render: for every chunk of `chunk` rays, (first ray, rays in the chunk, this process's row range
    inside the chunk after zero-ray padding to a multiple of the process count).  ZI/models.py:1416-1437."""
    plan = []
    for first in range(0, total, chunk):
        count = min(chunk, total - first)
        share = -(-count // world)
        plan.append((first, count, rank * share, (rank + 1) * share))
    return plan


def _rows(flat: Dict[str, torch.Tensor], first: int, count: int, lo: int, hi: int) -> Dict[str, torch.Tensor]:
    """Rows [lo, hi) of the zero-padded chunk [first, first + count) of every ray tensor."""
    real = max(min(hi, count) - lo, 0)  # rows of this share that are real rays; the rest is padding
    out = {}
    for k, v in flat.items():
        part = v[first + lo:first + lo + real]
        if real < hi - lo:  # zero rays, as the reference appends them
            part = torch.cat([part, v.new_zeros((hi - lo - real,) + tuple(v.shape[1:]))])
        out[k] = part
    return out


class _Assembler:
    """Writes each chunk's (gathered, un-padded) tensors into whole-render buffers allocated on first sight of a key."""

    def __init__(self, total: int):
        self.total = total
        self.buffers: Dict[str, object] = {}

    def put(self, key: str, first: int, value):
        if isinstance(value, list):  # per-level ray bundles: kept as parts, only a few rays of them survive
            slot = self.buffers.setdefault(key, [[] for _ in value])
            for parts, v in zip(slot, value):
                parts.append(v)
            return
        buf = self.buffers.get(key)
        if buf is None:
            buf = self.buffers[key] = value.new_empty((self.total,) + tuple(value.shape[1:]))
        buf[first:first + value.shape[0]] = value


def _gather_packed(acc, tensors: List[torch.Tensor], world: int) -> List[torch.Tensor]:
    """ONE collective for a chunk: every tensor of this process's share (equal shapes on every process: shares are padded) flattened
    into one float32 buffer, `acc.gather` of that buffer, and the processes' pieces cut back out and concatenated along dim 0 - what
    `acc.gather(t)` returns for each tensor separately (ZI/models.py:1454-1457 issues one all_gather per key: ~12 per chunk, ~1 150
    latency-bound collectives for a 4-camera 1024 x 768 render on 8 GPUs).  Values travel as float32, the dtype of every rendering key."""
    flat = torch.cat([t.reshape(-1).to(torch.float32) for t in tensors])
    got = acc.gather(flat[None])                       # [world, total]
    out, off = [], 0
    for t in tensors:
        n = t.numel()
        out.append(got[:, off:off + n].reshape((world * t.shape[0],) + tuple(t.shape[1:])).to(t.dtype))
        off += n
    return out


@torch.no_grad()
def render_image(model: Model, accelerator, batch, rand, config, train_frac=1, verbose=True, return_weights=False,
                 image=True, render_instance=False, instance_id=None, packed_gather=True):
    """Signature and result of ZI/models.py:1379-1507.  The sweep / image is rendered chunk by chunk
    (`config.render_chunk_size` rays); with several processes each renders a contiguous share of every chunk and
    `accelerator.gather` reassembles it.  `accelerator` may be None (one process) or any object with `process_index`,
    `num_processes`, `gather` (accelerate.Accelerator works).  packed_gather (default): ONE `gather` per chunk carrying every key
    (`_gather_packed`); False: the reference's call pattern, one `gather` per key per chunk - same result bit for bit.  For LiDAR
    sweeps on several GPUs prefer `sharding.render_sweep_sharded`: one collective per SWEEP."""
    if render_instance:
        # Not a gap of this path: the reference's branch cannot run.  render_image(render_instance=True) -> Model.obj_rendering
        # (ZI/models.py:579-794) -> obj_utils.box_pts(..., transform=False) (models.py:662), whose transform=False arm is
        # `import pdb; pdb.set_trace()` followed by a read of the never-assigned `pts_o` (ZI/obj_utils.py:216-217).  Probed by
        # running the reference here (tests/golden/make_golden.py:probe_obj_rendering): BdbQuit at obj_utils.py:217 <- models.py:662.
        raise NotImplementedError("render_instance: the reference's Model.obj_rendering stops in a pdb.set_trace() and then reads an unassigned "
                                  "variable (ZI/obj_utils.py:216-217, reached from ZI/models.py:662); there is no behaviour to reproduce")
    acc = accelerator or _SingleProcess()
    world, rank = acc.num_processes, acc.process_index
    lead = tuple(batch["origins"].shape[:2]) if image else (batch["origins"].shape[0],)
    total = int(np.prod(lead))
    flat = {k: v.reshape(total, -1) for k, v in batch.items() if v is not None}
    model.eval()
    out = _Assembler(total)
    for first, count, lo, hi in _chunk_plan(total, config.render_chunk_size, world, rank):
        renderings, ray_history = model(rand, _rows(flat, first, count, lo, hi), train_frac=train_frac,
                                        compute_extras=True, zero_glo=True)

        # this process's share of every key, in a fixed order: (key, level or None, tensor)
        items = []
        for key, val in renderings[-1].items():
            if key.startswith("ray_"):
                items += [(key, li, level[key].contiguous()) for li, level in enumerate(renderings)]
            else:
                items.append((key, None, val.contiguous()))
        if return_weights:
            items.append(("weights", None, ray_history[-1]["weights"].contiguous()))
        if world == 1:
            wholes = [t for _, _, t in items]
        elif packed_gather:
            wholes = [t[:count] for t in _gather_packed(acc, [t for _, _, t in items], world)]
        else:
            wholes = [acc.gather(t)[:count] for _, _, t in items]
        bundles: Dict[str, list] = {}
        for (key, li, _), t in zip(items, wholes):
            if li is None:
                out.put(key, first, t)
            else:
                bundles.setdefault(key, []).append(t)
        for key, levels in bundles.items():
            out.put(key, first, levels)
    rendering = {}
    for key, buf in out.buffers.items():
        if isinstance(buf, list):
            rendering[key] = [torch.cat(parts) for parts in buf]
        elif "hash" in key:
            rendering[key] = buf
        else:
            rendering[key] = buf.reshape(lead + tuple(buf.shape[1:])) if image else buf.reshape(total, -1)
    bundles = [k for k in rendering if k.startswith("ray_")]
    if bundles:  # the same random subset of rays for every bundle (models.py:1495-1503)
        have = rendering[bundles[0]][0].shape[0]
        pick = torch.randperm(have)[:config.vis_num_rays]
        for k in bundles:
            rendering[k] = [level[pick.to(level.device)] for level in rendering[k]]
    model.train()
    return rendering
