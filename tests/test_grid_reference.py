"""CPU checks of the grid operator's yardsticks: the C oracle (`oracle/grid_oracle.c`) against the float64 lookup of grid_ref.py at
every option the ABI accepts, and the per-level index plan (`nlr_grid_level_plan`) the kernels run under.  No GPU."""
import numpy as np
import pytest
import torch

from grid_ref import GridSpec, _grid_lookup, _level_table, _points, level_plan
from oracle import nlr_oracle as orc
from nerflidar_hip import config as nconfig, weights as nweights

COMBOS = [(g, a, i) for g in (0, 1) for a in (0, 1) for i in (0, 1)]    # gridtype (hash, tiled) x align_corners x interp (linear, smoothstep)


def _ulp32(v):
    return float(np.spacing(np.float32(v)))


@pytest.mark.parametrize("pls", [2.0, 1.7])
@pytest.mark.parametrize("C", [1, 8])
@pytest.mark.parametrize("gridtype,align,interp", COMBOS)
def test_oracle_forward_and_input_gradient_against_float64(gridtype, align, interp, C, pls):
    """`grid_encode_c` (+ dy_dx, through `grid_backward_c`'s input gradient) against the float64 lookup and its autograd: L = 4, H = 16,
    2^14 rows, integer and non-integer level scales, 3 000 points with the edge set of `_points`."""
    L, H, B = 4, 16, 3000
    offsets = nweights.level_table(L, H, 14, pls, align_corners=bool(align))[0]
    spec = GridSpec(offsets, pls, H, gridtype, align, interp)
    rng = np.random.default_rng(17 + C)
    table = (rng.random((int(offsets[-1]), C)) * 2 - 1).astype(np.float32)
    x = _points(B, 21)
    S = float(np.log2(pls))
    out, dy = orc.grid_encode_c(x, table, offsets, S, H, gridtype, bool(align), interp, want_dy_dx=True)
    xd = torch.from_numpy(x).double().requires_grad_(True)
    want = _grid_lookup(xd, torch.from_numpy(table).double(), spec)                       # [B, L, C]
    scales = [s for s, *_ in _level_table(spec)]
    tmax = float(np.abs(table).max())
    # A float32 position carries one rounding of x * scale + half (half an ulp of the scale; pos - floor is exact), a feature moves by
    # at most 2 max|table| per cell and axis, 1.5 x that under smoothstep, on 3 axes: 4.5 ulp max|table|; the rest of the 12 ulp is for
    # the float32 weights and the 8-term sum.  A wrong cell, corner or hash shows as an error of order max|table|.
    ferr = float(np.abs(out.transpose(1, 0, 2) - want.detach().numpy()).max())
    fbound = 12 * _ulp32(max(scales)) * tmax
    oob = ((x < 0) | (x > 1)).any(-1)
    assert oob.sum() == 8 and (out[:, oob] == 0).all() and (dy[oob] == 0).all()
    # input gradient: away from cell faces only (the float32 twin of a point within 1e-3 cell of a face may sit in the next cell,
    # where the derivative differs although the feature does not)
    near = np.zeros(B, bool)
    for s in scales:
        pos = x.astype(np.float64) * s + (0.0 if align else 0.5)
        near |= (np.abs(pos - np.round(pos)) < 1e-3).any(-1)
    grad = rng.standard_normal((L, B, C)).astype(np.float32)
    _, gi = orc.grid_backward_c(grad, x, offsets, int(offsets[-1]), C, S, H, dy_dx=dy, gridtype=gridtype, align_corners=bool(align), interp=interp)
    (gwant,) = torch.autograd.grad((want * torch.from_numpy(grad).double().permute(1, 0, 2)).sum(), xd)
    # per level the derivative is scale x (4 weighted differences) x pd: the position error (half an ulp of the scale, taken as a whole
    # one) moves pd = 6 p (1 - p) by at most 6 and the two other axes' weights by 1.5 (pd) x 1.5 (slope) each: 10.5 ulp(scale) relative
    # to scale x 2 max|table|; about 24 float32 operations on the way and the L * C-term sum add (24 + L C) 2^-24 of the same
    per_level = np.array([2 * tmax * s * (10.5 * _ulp32(s) + (24 + L * C) * 2.0 ** -24) for s in scales])
    gbound = (np.abs(grad).sum(-1) * per_level[:, None]).sum(0)                           # [B]
    gerr = np.abs(gi - gwant.numpy()).max(-1)
    keep = ~near & ~oob
    print(f"gridtype={gridtype} align={align} interp={interp} C={C} pls={pls}: forward err {ferr:.3e} (bound {fbound:.3e}); input gradient "
          f"err/bound {float((gerr / gbound)[keep].max()):.3f}, rel {float(gerr[keep].max() / np.abs(gwant.numpy()).max()):.3e}; left out {int(near.sum())}/{B}")
    assert ferr <= fbound
    assert near.sum() <= 0.1 * B
    assert (gerr[keep] <= gbound[keep]).all()
    assert np.abs(gi[oob]).max() == 0


def _reference_index(gridtype, step, hs, p):
    """gridencoder.cu:66-84 for one corner p (python ints)."""
    stride, index = 1, 0
    for d in range(3):
        if stride > hs:
            break
        index += p[d] * stride
        stride *= step
    if gridtype == 0 and stride > hs:
        index = (p[0] ^ (p[1] * 2654435761 & 0xFFFFFFFF) ^ (p[2] * 805459861 & 0xFFFFFFFF)) & 0xFFFFFFFF
    return index % hs


@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("gridtype", [0, 1])
def test_dense_levels_stay_inside_their_table(gridtype, align):
    """A level in mode 0 is indexed x + y step + z step^2 with no modulo: that must be the reference's walk-then-modulo for every corner
    a kernel can ask for, up to the upper corner of the cell of a coordinate of exactly 1 (cmax).  The index grows with every coordinate,
    so the corner (cmax, cmax, cmax) decides; the reference's own index is computed for the extreme corners as well."""
    seen0 = demoted = 0
    for H in (16, 33, 140):
        for log2 in (14, 19, 22):
            for pls in (2.0, 1.7):
                for L in (1, 5):
                    offsets = nweights.level_table(L, H, log2, pls, align_corners=bool(align))[0]
                    S = float(np.log2(pls))
                    scale, res = orc.level_scale(L, S, H)
                    for C in (1, 4):
                        mode, step, kind = level_plan(offsets, C, S, H, gridtype, align, 1 << 18)
                        for l in range(L):
                            hs = int(offsets[l + 1] - offsets[l])
                            st = int(res[l]) + (0 if align else 1)
                            assert step[l] == st
                            cmax = int(np.floor(np.float32(np.float32(1.0) * scale[l] + np.float32(0.0 if align else 0.5)))) + 1
                            walk = st ** 3 <= hs
                            if mode[l] == 0:
                                seen0 += 1
                                assert walk and cmax * (1 + st + st * st) < hs, (H, log2, pls, l, st, hs, cmax)
                                for p in ((cmax, cmax, cmax), (cmax, 0, 0), (0, cmax, 0), (0, 0, cmax), (cmax - 1, cmax, cmax)):
                                    assert _reference_index(gridtype, st, hs, p) == p[0] + p[1] * st + p[2] * st * st
                                assert kind[l] == (1 if hs * C <= 36864 else 2 if st <= 129 else 0)
                            elif mode[l] == 1:                                             # the reference hashes, into a power of two
                                assert gridtype == 0 and not walk and hs & (hs - 1) == 0
                                assert kind[l] == (2 if st <= 129 else 0)
                            else:
                                assert mode[l] == 2 and kind[l] == 0
                                demoted += walk
    assert seen0 > 0
    # without align_corners cmax <= step - 1 and every level the walk covers is dense; with it, a level with an integer scale (level 0
    # always) has cmax = step: one past the lattice, folded back by the reference's modulo, so it is not mode 0
    assert (demoted > 0) == bool(align)


# (workload, grid) -> (mode, step, lds_kind at B = 2^18) per level with align_corners = 0, as computed by the commit before the mode rule
# looked at cmax: the rule change must not move any of them
def _steps(L):
    return tuple(16 * 2 ** l + 1 for l in range(L))


def _plan(L, kinds, gridtype):
    return ((0, 0, 0) + ((1,) if gridtype == 0 else (2,)) * (L - 3), _steps(L), kinds + (0,) * (L - len(kinds)))


_NERF = {0: (1, 2, 2, 2), 1: (1, 2, 2)}   # lds_kind of the leading levels (the rest 0), per gridtype
_PROP = {0: (1, 1, 2, 2), 1: (1, 1, 2)}
PARENT_PLANS = {(name, which, g): _plan(L, (_NERF if which == "nerf" else _PROP)[g], g)
                for name in ("C2", "REF", "P_F32", "P_F20") for g in (0, 1)
                for which, L in (("nerf", 16 if name == "P_F32" else 10), ("prop0", 6), ("prop1", 8))}


@pytest.mark.parametrize("gridtype", [0, 1])
@pytest.mark.parametrize("name", ["C2", "REF", "P_F32", "P_F20"])
def test_plans_of_the_workloads_are_unchanged_without_align_corners(name, gridtype):
    mc = nconfig.workload(name)
    for which, cfg in (("nerf", mc.nerf_mlp), ("prop0", mc.prop_cfg(0)), ("prop1", mc.prop_cfg(1))):
        offsets, _, pls = nweights.grid_layout(cfg)
        got = level_plan(offsets, cfg.grid_level_dim, float(np.log2(pls)), cfg.grid_base_resolution, gridtype, 0, 1 << 18)
        assert tuple(map(tuple, got)) == PARENT_PLANS[name, which, gridtype], (name, which)
