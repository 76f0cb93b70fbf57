"""The stand-alone grid operator (csrc/nlr_grid.hip) at every option its C ABI accepts: gridtype hash / tiled, align_corners, linear /
smoothstep interpolation, level_dim 1 / 2 / 4 / 8, f32 / f16 tables, and every route of the table gradient (x-pair and one-corner
atomics, the LDS copy, the tagged LDS cache on dense and on hashed levels, the bins), each against oracle/grid_oracle.c.

Every table carries guard rows behind its last level (NaN where the kernels read, a sentinel where they add; the sentinel is asserted
bit-unchanged), and every test that claims a route reads it from `nlr_grid_level_plan` / `nlr_grid_backward_workspace_bytes`.
NLR_GRID_ENVELOPE_LOG=<file> appends the measured figures."""
import functools
import os

import numpy as np
import pytest
import torch

from grid_ref import _points, level_plan
from oracle import nlr_oracle as orc
from nerflidar_hip import _lib, weights as nweights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COMBOS = [(g, a, i) for g in (0, 1) for a in (0, 1) for i in (0, 1)]    # gridtype (hash, tiled) x align_corners x interp (linear, smoothstep)
SENTINEL = 12345.678
_LOG = os.environ.get("NLR_GRID_ENVELOPE_LOG")
P_MID = np.array([0.51, 0.52, 0.53], np.float32)   # shares its cell with 0.5 (where the kernels park invalid lanes) on the three coarsest levels


def _record(line):
    print(line)
    if _LOG:
        with open(_LOG, "a") as f:
            f.write(line + "\n")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def npy(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _grid(L, H, log2, pls, align):
    """offsets, S, and the guard: 2 (step^2 + step + 1) rows of the finest level the dense walk covers (a stray upper corner of such a
    level lies at most step^2 + step + 1 rows past it)."""
    offsets = nweights.level_table(L, H, log2, pls, align_corners=bool(align))[0]
    return offsets, float(np.log2(pls)), _guard_rows(offsets, float(np.log2(pls)), H, align)


def _guard_rows(offsets, S, H, align):
    _, res = orc.level_scale(len(offsets) - 1, S, H)
    guard = 64
    for l in range(len(offsets) - 1):
        step = int(res[l]) + (0 if align else 1)
        if step ** 3 <= int(offsets[l + 1] - offsets[l]):
            guard = 2 * (step * step + step + 1)
    return guard


def _table(offsets, C, guard, seed):
    """[rows + guard, C] f32 in [-1, 1], the guard rows NaN."""
    n = int(offsets[-1])
    t = np.full((n + guard, C), np.nan, np.float32)
    t[:n] = np.random.default_rng(seed).random((n, C)) * 2 - 1
    return t


def _grad_table(n, C, guard):
    gt = torch.zeros(n + guard, C, device=DEV)
    gt[n:] = SENTINEL
    return gt


def _guard_intact(gt, n):
    return bool((gt[n:].view(torch.int32) == torch.tensor(SENTINEL).view(torch.int32).item()).all())


def _forward(xd, td, dtype_id, off, C, L, S, H, opts, layout, want_dy):
    B = xd.shape[0]
    out = torch.full((L, B, C) if layout == 0 else (B, L * C), float("nan"), device=DEV)
    dy = torch.full((B, L * 3 * C), float("nan"), device=DEV) if want_dy else None
    _lib.check(_lib.lib().nlr_grid_encode_forward(_lib.ptr(xd), _lib.ptr(td), dtype_id, off.ctypes.data, _lib.ptr(out), B, 3, C, L, S, H, _lib.ptr(dy),
                                                  opts[0], opts[1], opts[2], layout, None))
    torch.cuda.synchronize()
    got = npy(out) if layout == 0 else npy(out).reshape(B, L, C).transpose(1, 0, 2)
    return got, (npy(dy) if want_dy else None)


# ---- forward + dy_dx ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 4, 8])
@pytest.mark.parametrize("gridtype,align,interp", COMBOS)
def test_forward_and_dy_dx_every_option(gridtype, align, interp, C):
    """`nlr_grid_fwd_kernel`, f32 and f16 tables, both output layouts, with and without dy_dx: outputs bit-equal to the oracle, dy_dx at
    the tolerance of test_grid_forward_bit_exact; integer (2) and non-integer (1.7) level scales."""
    L, H, B = 4, 16, 2000
    opts = (gridtype, align, interp)
    x = _points(B, 31)
    xd = cu(x)
    for pls in (2.0, 1.7):
        offsets, S, guard = _grid(L, H, 14, pls, align)
        off = np.ascontiguousarray(offsets, np.int32)
        n = int(offsets[-1])
        table = _table(offsets, C, guard, 40 + C)
        for dtype_id in (0, 1):
            td = cu(table) if dtype_id == 0 else cu(table).half()
            ref, ref_dy = orc.grid_encode_c(x, npy(td.float())[:n], offsets, S, H, gridtype, bool(align), interp, want_dy_dx=True)
            for layout in (0, 1):
                got, dy = _forward(xd, td, dtype_id, off, C, L, S, H, opts, layout, True)
                np.testing.assert_array_equal(got, ref)
                np.testing.assert_allclose(dy, ref_dy, rtol=1e-5, atol=1e-4)
                assert (got[:, 8:16] == 0).all() and (dy[8:16] == 0).all()           # out-of-range points
                got2, _ = _forward(xd, td, dtype_id, off, C, L, S, H, opts, layout, False)
                np.testing.assert_array_equal(got2, ref)
        assert np.abs(ref).max() > 0.5 and np.abs(ref_dy).max() > 1.0


# ---- table gradient: shared pieces -------------------------------------------------------------------------------------------------
def _oracle_grads(grad, x, offsets, C, S, H, opts):
    n = int(offsets[-1])
    kw = dict(gridtype=opts[0], align_corners=bool(opts[1]), interp=opts[2])
    ref, _ = orc.grid_backward_c(grad, x, offsets, n, C, S, H, **kw)
    ref_abs, _ = orc.grid_backward_c(np.abs(grad), x, offsets, n, C, S, H, **kw)
    return ref, ref_abs


def _backward(gd, xd, off, n, C, L, S, H, opts, layout, guard, ws=None, nbytes=0):
    gt = _grad_table(n, C, guard)
    B = xd.shape[0]
    _lib.check(_lib.lib().nlr_grid_encode_backward_ws(_lib.ptr(gd), _lib.ptr(xd), off.ctypes.data, _lib.ptr(gt), B, 3, C, L, S, H, None, None, opts[0], opts[1],
                                                      opts[2], layout, _lib.ptr(ws), nbytes, None))
    torch.cuda.synchronize()
    assert _guard_intact(gt, n), "the guard rows behind the last level were written"
    return npy(gt[:n])


def _check_table_gradient(tag, got, ref, ref_abs, quiet=False):
    """The bound of the existing backward tests: float atomics add in another order than the oracle's loop, so the error is held
    against the sum of |contributions| of an entry (the oracle run on |grad|)."""
    err = np.abs(got - ref)
    ratio = float(np.max(err / (ref_abs + 1e-3)))
    if not quiet:
        _record(f"{tag}: max err / sum|terms| {ratio:.3e} (bound 2e-6), max err {float(err.max()):.3e}")
    assert np.isfinite(got).all(), tag
    assert (err <= 2e-6 * ref_abs + 1e-6).all(), f"{tag}: max err / sum|terms| {ratio:.3e}"
    return ratio


def _layout(grad, layout):
    L, B, C = grad.shape
    return grad if layout == 0 else np.ascontiguousarray(grad.transpose(1, 0, 2).reshape(B, L * C))


# ---- table gradient, small batch: the atomic scatter kernels and their run aggregation -----------------------------------------------
def _run_sequence(n, seed):
    """Points built for `nlr_run_atomic` (runs of equal addresses inside a 16-lane row are merged): 3 loose points so that the runs do
    not start on a row, then k copies of one point for k = 2, 16, 17, 40 (inside a row, a whole row, across a row, across a wave; the
    17 with a jitter that keeps the cell on the coarse levels only), an A, B, A, B alternation (equal but not adjacent: no merge), a run
    in the cell where invalid lanes are parked with an out-of-range point in its middle, then loose points."""
    rng = np.random.default_rng(seed)
    x = rng.random((max(n, 128), 3)).astype(np.float32)
    i = 3
    for k, jitter in ((2, 0), (16, 0), (17, 4e-3), (40, 0)):
        p = rng.random(3).astype(np.float32) * 0.8 + 0.1
        x[i:i + k] = p + (rng.random((k, 3)).astype(np.float32) * jitter if jitter else 0)
        i += k
    a, b = rng.random((2, 3)).astype(np.float32)
    x[i:i + 16:2], x[i + 1:i + 16:2] = a, b
    i += 16
    x[i:i + 11] = P_MID
    x[i + 5] = (1.0001, 0.5, 0.5)
    x[0], x[1] = (1, 1, 1), (0, 1, 0.25)                               # the cube's far corner and a face
    return x[:n]


SMALL_B = (1, 15, 16, 17, 63, 64, 65, 257)


@pytest.mark.parametrize("C", [1, 2, 4, 8])
@pytest.mark.parametrize("gridtype,align,interp", COMBOS)
def test_table_gradient_small_batch(gridtype, align, interp, C):
    """`nlr_grid_bwd_xpair_kernel` (C <= 4) and `nlr_grid_bwd_kernel` (C = 8, and C <= 4 under NLR_DBG_NO_XPAIR_SCATTER), both gradient
    layouts, batches around the row / wave / workgroup sizes.  Every batch ends in a run on its last valid lane, in the cell where the
    clamped lanes behind it are parked."""
    L, H = 4, 16
    opts = (gridtype, align, interp)
    offsets, S, guard = _grid(L, H, 14, 2.0, align)
    off = np.ascontiguousarray(offsets, np.int32)
    n = int(offsets[-1])
    lib = _lib.lib()
    worst = 0.0
    for B in SMALL_B:
        assert level_plan(offsets, C, S, H, gridtype, align, B)[2] == [0] * L     # no LDS level: every level through the atomic scatter
        x = _run_sequence(B, 50 + B).copy()
        x[max(B - 3, 0):] = P_MID
        grad = np.random.default_rng(60 + B).standard_normal((L, B, C)).astype(np.float32)
        ref, ref_abs = _oracle_grads(grad, x, offsets, C, S, H, opts)
        xd = cu(x)
        for layout in (0, 1):
            gd = cu(_layout(grad, layout))
            for one_corner in ((0, 1) if C <= 4 else (0,)):
                try:
                    lib.nlr_debug_set(_lib.DBG_NO_XPAIR_SCATTER, one_corner)
                    assert lib.nlr_debug_get(_lib.DBG_NO_XPAIR_SCATTER) == one_corner
                    got = _backward(gd, xd, off, n, C, L, S, H, opts, layout, guard)
                finally:
                    lib.nlr_debug_set(_lib.DBG_NO_XPAIR_SCATTER, 0)
                kernel = "one-corner" if one_corner or C == 8 else "x-pair"
                worst = max(worst, _check_table_gradient(f"small batch {opts} C={C} B={B} layout={layout} {kernel}", got, ref, ref_abs, quiet=True))
    _record(f"small batch {opts} C={C}: max err / sum|terms| over {len(SMALL_B)} batch sizes, both layouts and kernels {worst:.3e} (bound 2e-6)")
    assert np.abs(ref).max() > 1.0


# ---- table gradient, large batch: the LDS copy, the LDS cache, the bins ---------------------------------------------------------------
def _large_points(B, order, seed):
    rng = np.random.default_rng(seed)
    if order == "ray":                       # 512 rays of consecutive points: runs of equal cells
        n_r = 512
        o = rng.random((n_r, 1, 3)) * 0.6 + 0.2
        d = rng.standard_normal((n_r, 1, 3))
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        t = np.linspace(-0.2, 0.2, -(-B // n_r))[None, :, None]
        x = (o + d * t).reshape(-1, 3)[:B].astype(np.float32)
    else:
        x = rng.random((B, 3)).astype(np.float32)
    x[:16] = _points(16, 5)                  # corners (a coordinate of exactly 1 among them), faces and out-of-range points
    x[16:144] = _run_sequence(128, seed)     # a run in the cell where invalid lanes are parked, an out-of-range point in its middle
    x[B - 3:] = P_MID                        # ... and one that ends on the last valid lane
    return x


def _claims(mode, kind):
    """What a plan shows: kind 1 = the LDS copy (dense levels only), kind 2 = the LDS cache, kind 0 = scattered."""
    names = {(1, 0): "direct", (2, 0): "cache on a dense level", (2, 1): "cache on a hashed level"}
    return {"scattered" if k == 0 else names[k, m] for m, k in zip(mode, kind)}


def _large_case(tag, offsets, S, H, C, opts, guard, orders, want_claims=None, want_modes=None):
    """One grid through every route of a large batch: atomics + LDS kernel, the same with the bins, both again without the LDS cache;
    ray-ordered points in the [L, B, C] gradient layout, random ones in [B, L * C]."""
    L = len(offsets) - 1
    off = np.ascontiguousarray(offsets, np.int32)
    n = int(offsets[-1])
    B = (1 << 18) // C + 4096 + 37           # the smallest batch that takes the LDS path (+ a ragged tail)
    lib = _lib.lib()
    mode, step, kind = level_plan(offsets, C, S, H, opts[0], opts[1], B)
    if want_claims is not None:
        assert want_claims <= _claims(mode, kind), (tag, mode, step, kind)
    if want_modes is not None:
        assert mode == want_modes, (tag, mode)
    for order in orders:
        x = _large_points(B, order, 70 + C)
        grad = np.random.default_rng(71).standard_normal((L, B, C)).astype(np.float32)
        ref, ref_abs = _oracle_grads(grad, x, offsets, C, S, H, opts)
        layout = int(order == "random")      # the ray-ordered batch in the [L, B, C] gradient layout, the random one in [B, L * C]
        xd, gd = cu(x), cu(_layout(grad, layout))
        try:
            lib.nlr_debug_set(_lib.DBG_BINNED_C4, int(C == 4))
            for no_cache in (0, 1):
                lib.nlr_debug_set(_lib.DBG_NO_SCATTER_CACHE, no_cache)
                kind_now = level_plan(offsets, C, S, H, opts[0], opts[1], B)[2]
                assert (2 not in kind_now) if no_cache else (kind_now == kind)
                got = _backward(gd, xd, off, n, C, L, S, H, opts, layout, guard)
                _check_table_gradient(f"large batch {tag} {opts} C={C} {order} atomics{' no-cache' if no_cache else ''}", got, ref, ref_abs)
                if 0 in kind_now:            # a scattered level: the bins take it when the caller brings the workspace
                    need = lib.nlr_grid_backward_workspace_bytes(B, C, L, S, H, off.ctypes.data, opts[0], opts[1])
                    assert need > 0, (tag, kind_now)
                    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
                    got = _backward(gd, xd, off, n, C, L, S, H, opts, layout, guard, ws, need)
                    _check_table_gradient(f"large batch {tag} {opts} C={C} {order} bins{' no-cache' if no_cache else ''}", got, ref, ref_abs)
        finally:
            lib.nlr_debug_set(_lib.DBG_NO_SCATTER_CACHE, 0)
            lib.nlr_debug_set(_lib.DBG_BINNED_C4, 0)
        assert np.abs(ref[: int(offsets[1])]).max() > 1.0


@pytest.mark.parametrize("C", [1, 2, 4])
@pytest.mark.parametrize("gridtype,align,interp", COMBOS)
def test_table_gradient_large_batch(gridtype, align, interp, C):
    """L = 5, H = 16.  Without align_corners, scale 2 and 2^16 rows show the LDS copy (18^3), the cache on a dense level (34^3), the
    cache on a hashed level (step 66) and scattered levels (steps 130, 258; every tiled level past its table).  With align_corners
    every level with an integer scale leaves the dense mode (its upper corner at x = 1 lies past the lattice), so the same is shown with
    scale 1.2 and 2^15 rows (steps 16, 20, 24, 28, 34), and scale 2 runs as well: dense-sized levels through the generic index."""
    opts = (gridtype, align, interp)
    want = {"direct", "scattered"} | ({"cache on a dense level"} if C >= 2 else set()) | ({"cache on a hashed level"} if gridtype == 0 else set())
    if not align:
        offsets, S, guard = _grid(5, 16, 16, 2.0, 0)
        _large_case("scale 2, 2^16", offsets, S, 16, C, opts, guard, ("ray", "random"), want)
    else:
        offsets, S, guard = _grid(5, 16, 15, 1.2, 1)
        _large_case("scale 1.2, 2^15", offsets, S, 16, C, opts, guard, ("ray", "random"), want)
        offsets, S, guard = _grid(5, 16, 16, 2.0, 1)
        _large_case("scale 2, 2^16", offsets, S, 16, C, opts, guard, ("ray",), want_modes=[2, 2] + ([1, 1, 1] if gridtype == 0 else [2, 2, 2]))


def test_table_gradient_hashed_level_of_odd_size():
    """Hand-made offsets: a hashed level of 12 000 rows (not a power of two) takes the generic index (mode 2) on a hash grid."""
    offsets = np.array([0, 5832, 5832 + 12000, 5832 + 12000 + 16384], np.int32)
    _large_case("12 000-row hashed level", offsets, 1.0, 16, 2, (0, 0, 0), _guard_rows(offsets, 1.0, 16, 0), ("ray",), {"direct", "scattered"},
                want_modes=[0, 2, 1])


@pytest.mark.parametrize("H,align", [(32, 0), (33, 1)])
def test_table_gradient_level_that_fills_the_lds_copy(H, align):
    """33^3 = 35 937 entries of the 36 864 the LDS copy holds, C = 1.  Without align_corners (H = 32, step 33) the level is accumulated in
    LDS.  With align_corners (H = 33) the upper corner of x = 1 has the dense index 37 059, past the level and past the LDS copy itself:
    the level takes the generic index and is scattered."""
    offsets, S, guard = _grid(2, H, 17, 1.7, align)
    assert int(offsets[1]) == 35944
    _large_case(f"H={H}", offsets, S, H, 1, (0, align, 0), guard, ("random",), {"scattered"} if align else {"direct"}, want_modes=[2, 1] if align else [0, 1])


# ---- input gradient -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 8])
def test_input_gradient_from_a_smoothstep_forward(C):
    """`nlr_grid_input_bwd_kernel` on the dy_dx of a smoothstep forward, both gradient layouts, against the oracle's."""
    L, H, B = 4, 16, 2000
    opts = (0, 0, 1)
    offsets, S, guard = _grid(L, H, 14, 2.0, 0)
    off = np.ascontiguousarray(offsets, np.int32)
    n = int(offsets[-1])
    x = _points(B, 32)
    xd, td = cu(x), cu(_table(offsets, C, guard, 80))
    _, dy = _forward(xd, td, 0, off, C, L, S, H, opts, 0, True)
    grad = np.random.default_rng(81).standard_normal((L, B, C)).astype(np.float32)
    _, ref_gi = orc.grid_backward_c(grad, x, offsets, n, C, S, H, dy_dx=dy, interp=1)
    dyd = cu(dy)
    for layout in (0, 1):
        gd = cu(_layout(grad, layout))
        gt, gi = _grad_table(n, C, guard), torch.full((B, 3), float("nan"), device=DEV)
        _lib.check(_lib.lib().nlr_grid_encode_backward(_lib.ptr(gd), _lib.ptr(xd), off.ctypes.data, _lib.ptr(gt), B, 3, C, L, S, H, _lib.ptr(dyd), _lib.ptr(gi),
                                                       0, 0, 1, layout, None))
        torch.cuda.synchronize()
        assert _guard_intact(gt, n)
        np.testing.assert_allclose(npy(gi), ref_gi, rtol=1e-4, atol=1e-4)
    assert np.abs(ref_gi).max() > 10 and (ref_gi[8:16] == 0).all()


# ---- total variation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 4, 8])
@pytest.mark.parametrize("gridtype,align", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_total_variation_every_option(gridtype, align, C):
    """`nlr_grid_tv_kernel` against the oracle; points at 0 and at 1 on every axis (no left / no right neighbour)."""
    L, H, B = 4, 16, 4000
    offsets, S, guard = _grid(L, H, 14, 2.0, align)
    off = np.ascontiguousarray(offsets, np.int32)
    n = int(offsets[-1])
    x = _points(B, 33)
    for d in range(3):
        x[16 + 2 * d, d], x[17 + 2 * d, d] = 0.0, 1.0
    table = _table(offsets, C, guard, 90 + C)
    g0 = (np.random.default_rng(91).standard_normal((n, C)) * 1e-3).astype(np.float32)
    ref = orc.grid_tv_c(x, table[:n], g0, offsets, 1e-2, S, H, gridtype, bool(align))
    gd = _grad_table(n, C, guard)
    gd[:n] = cu(g0)
    xd, td = cu(x), cu(table)
    _lib.check(_lib.lib().nlr_grad_total_variation(_lib.ptr(xd), _lib.ptr(td), _lib.ptr(gd), off.ctypes.data, 1e-2, B, 3, C, L, S, H, gridtype, align, None))
    torch.cuda.synchronize()
    assert _guard_intact(gd, n)
    np.testing.assert_allclose(npy(gd[:n]), ref, rtol=2e-4, atol=2e-6)   # float atomics + v_rsq_f32 for 1/sqrt
    assert np.abs(ref - g0).max() > 1e-3
