"""Algorithmic work of the render path: GEMM MACs only, transcendental and
elementwise work excluded.  Used by bench.py for the roofline numerator."""
from __future__ import annotations

from .config import MLPConfig, ModelConfig
from .weights import mlp_param_shapes


def macs_per_sample(cfg: MLPConfig) -> int:
    return sum(o * i for _, (o, i), _ in mlp_param_shapes(cfg))


def lidar_macs_per_sample(cfg: MLPConfig) -> int:
    """MACs a LiDAR-only render executes per sample of this MLP: density trunk and the semantic / intensity heads; the view MLP
    (lin_second_stage_*) and the rgb layer are not run."""
    return sum(o * i for name, (o, i), _ in mlp_param_shapes(cfg) if not (name.startswith("lin_second_stage_") or name == "rgb_layer"))


def _folded_shapes(cfg: MLPConfig):
    """Linear shapes of the program `NLR_PREC_FAST` runs for a NerfMLP (nlr_mlp_kernel.h, FOLD): density_layer.2 is multiplied into
    every layer that reads the bottleneck (head layers 0, view layer 0, the skip columns of the layer behind the skip concat), which
    then read the 64-wide hidden vector of the trunk; of density_layer.2 itself the raw-density row is left.  Counted like
    `macs_per_sample`: real rows and columns, no padding to MFMA tiles, one MAC per product (the split-bf16 layers issue three)."""
    if cfg.disable_rgb:  # PropMLP: not folded
        return [(name, shape) for name, shape, _ in mlp_param_shapes(cfg)]
    wb, depth = cfg.bottleneck_width, cfg.net_depth_viewdirs
    reads_b = {"sem_layer.0", "intensity_layer.0", "lin_second_stage_0"}
    if 0 <= cfg.skip_layer_dir < depth:
        reads_b.add(f"lin_second_stage_{cfg.skip_layer_dir + 1}" if cfg.skip_layer_dir + 1 < depth else "rgb_layer")
    out = []
    for name, (o, i), _ in mlp_param_shapes(cfg):
        if name == "density_layer.2":
            o = 1
        elif name in reads_b:
            i = i - wb + 64
        out.append((name, (o, i)))
    return out


def executed_macs_per_sample(cfg: MLPConfig) -> int:
    """MACs per sample of the folded program (`NLR_PREC_FAST`).  `macs_per_sample` keeps counting the MODEL's MACs - the numerator of
    bench.py's `roofline.frac` - so after the fold that fraction is no longer the executed MFMA rate; quote both."""
    return sum(o * i for _, (o, i) in _folded_shapes(cfg))


def executed_lidar_macs_per_sample(cfg: MLPConfig) -> int:
    """The LiDAR-only twin: folded trunk + heads, no view MLP, no rgb layer."""
    return sum(o * i for name, (o, i) in _folded_shapes(cfg) if not (name.startswith("lin_second_stage_") or name == "rgb_layer"))


def lidar_flops_per_ray(mc: ModelConfig) -> int:
    """`flops_per_ray` of `render_rays(lidar_only=True)`: EXECUTED work only.  A rate quoted for the LiDAR-only mode uses this
    count - the skipped view MLP is not work done."""
    s = mc.level_samples()
    total = 0
    for li in range(mc.num_levels):
        last = li == mc.num_levels - 1
        cfg = mc.nerf_mlp if last else mc.prop_cfg(li)
        total += s[li] * (lidar_macs_per_sample(cfg) if last else macs_per_sample(cfg))
    return 2 * total


def flops_per_ray(mc: ModelConfig) -> int:
    s = mc.level_samples()
    total = 0
    for li in range(mc.num_levels):
        cfg = mc.prop_cfg(li) if li < mc.num_levels - 1 else mc.nerf_mlp
        total += s[li] * macs_per_sample(cfg)
    return 2 * total


def gather_bytes_per_ray(mc: ModelConfig, sample_n: int = 7, table_bytes: int = 4) -> int:
    """sum_l S_l * n * L_l * 8 corners * C_l * sizeof  (algorithmic, before any caching)."""
    s = mc.level_samples()
    total = 0
    for li in range(mc.num_levels):
        cfg = mc.prop_cfg(li) if li < mc.num_levels - 1 else mc.nerf_mlp
        total += s[li] * sample_n * cfg.grid_num_levels * 8 * cfg.grid_level_dim * table_bytes
    return total
