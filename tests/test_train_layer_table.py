"""nlr_train_linear_table (header section 6b): the plan's layer table, the single description of the fused training NerfMLP, against
`nlr_train_param_layout`, the modules of `TrainableNerfLevel._mlp_params()` and, for the smallest plan, the rows written out by hand."""
import ctypes as C

import numpy as np
import pytest
import torch

from nerflidar_hip import _lib, training as ntrain
from nerflidar_hip.config import MLPConfig

ROW = 16  # uint32 per Linear: g_col, o_off, n_out, color, n_blocks, 3 x (src, col, n), w_off, b_off
K = 5
PLANS = {"W128-D2-noheads": dict(net_width_viewdirs=128, net_depth_viewdirs=2),
         "W128-D3-sem": dict(net_width_viewdirs=128, net_depth_viewdirs=3, use_semantic=True),
         "W256-D4-both": dict(net_width_viewdirs=256, net_depth_viewdirs=4, use_semantic=True, use_intensity=True)}
# W = 128, D = 2, no heads, F = 10 levels x 4 = 40 grid features, E = 3 + 6 * 4 = 27 encoding columns; acts = [hid 64 | bottleneck 256 |
# x_0 128 | x_1 128] (act_w = 576), gacts = the same columns, then [d head outputs 32 | d rgb_layer outputs 32]
BY_HAND = [
    # g_col o_off n_out color blocks  (src, col, n) x 3                      w_off   b_off
    [0,     0,    64,   0,    1,      1, 0, 40,    0, 0, 0,     0, 0, 0,     0,      2560],    # density_layer.0 <- features
    [64,    0,    256,  0,    1,      0, 0, 64,    0, 0, 0,     0, 0, 0,     2624,   19008],   # density_layer.2 <- hid
    [320,   0,    128,  1,    2,      0, 64, 256,  2, 0, 27,    0, 0, 0,     19264,  55488],   # lin_second_stage_0 <- bottleneck | enc
    [448,   0,    128,  1,    3,      0, 320, 128, 0, 64, 256,  2, 0, 27,    55616,  108224],  # .._1 <- x_0 | bottleneck | enc
    [608,   0,    3,    1,    1,      0, 448, 128, 0, 0, 0,     0, 0, 0,     108352, 108736],  # rgb_layer <- x_1
]


def _table(plan):
    L = _lib.lib()
    offs = (C.c_uint32 * 64)()
    n_offs = L.nlr_train_param_layout(plan.handle, offs, len(offs))
    rows = (C.c_uint32 * (ROW * 32))()
    n = L.nlr_train_linear_table(plan.handle, rows, len(rows))
    assert n > 0 and n_offs > 0
    return np.array(rows[:n * ROW], dtype=np.int64).reshape(n, ROW), list(offs[:n_offs])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PLANS))
def test_layer_table_matches_layout_modules_and_columns(name):
    cfg = MLPConfig(class_num=K, no_sem_layer=False, grid_log2_hashmap_size=12, **PLANS[name])
    lvl = ntrain.TrainableNerfLevel(cfg, fused_mlp=True)
    with torch.cuda.device(0):
        plan = ntrain._TrainPlan(cfg)
    t, offs = _table(plan)
    assert len(t) == len(offs) // 2 and len(offs) % 2 == 0
    assert t[:, 14].tolist() == offs[0::2] and t[:, 15].tolist() == offs[1::2]
    params = lvl._mlp_params()
    weights, biases = params[0::2], params[1::2]
    assert len(weights) == len(t)
    view = {id(getattr(lvl, f"lin_second_stage_{i}").weight) for i in range(cfg.net_depth_viewdirs)} | {id(lvl.rgb_layer.weight)}
    for r, w, b in zip(t, weights, biases):
        n_blocks = int(r[4])
        assert 1 <= n_blocks <= 3 and (r[5 + 3 * n_blocks:14] == 0).all()
        assert sum(int(r[7 + 3 * k]) for k in range(n_blocks)) == w.shape[1], r
        assert r[2] == w.shape[0] == b.shape[0], r
        assert r[3] == (1 if id(w) in view else 0), r
    aw = plan.act_w
    by_weight = {id(w): r for r, w in zip(t, weights)}
    assert by_weight[id(lvl.rgb_layer.weight)][0] == aw + 32
    if cfg.use_semantic:
        assert by_weight[id(lvl.sem_layer[2].weight)][0] == aw
    if cfg.use_intensity:
        assert by_weight[id(lvl.intensity_layer[2].weight)][0] == aw + K
    # what the host side reads is the same table
    assert [(l.g_col, l.o_off, l.n_out, l.color, l.w_off, l.b_off) for l in plan.linears] == [tuple(r[[0, 1, 2, 3, 14, 15]]) for r in t]
    assert [l.blocks for l in plan.linears] == [tuple(tuple(r[5 + 3 * k:8 + 3 * k]) for k in range(r[4])) for r in t]
    if name == "W128-D2-noheads":
        assert aw == 576 and plan.n_params == 108739
        assert t.tolist() == BY_HAND
