"""`nlr_resample_kernel` at the sizes where its lane runs begin, end and advance.

The kernel gives one 64-lane wavefront to a ray and finds every integer rank it needs (the merge position of the 3n+1 dilated
fenceposts, the covering range [j0, j1) of each dilated bin, the CDF interval of each of the S samples) per contiguous run of queries:
one full binary search for the first query of a lane's run, and for every further query a search narrowed to what the previous query
and the next lane's first query leave open.  What can go wrong is a run boundary (a lane's run ending inside a list, the last lane
of a list, idle lanes) or a narrowed search that starts from a wrong bound, so n_prev and S run over sizes where 3n+1, 3n and S lie
below, at and just above a multiple of 64 ((3 * 21 + 1) = 64, 3 * 64 = 192, S = 63 / 64 / 65), the smallest sizes (n_prev = 1, 2;
S = 2, 3) and the largest the library accepts (n_prev = 512, S = 1024), with and without dilation, with and without jitter.

Reference: oracle.nlr_oracle (`max_dilate_weights` -> trim -> `resample_logits` -> `sample_intervals` -> `s_to_t`), float32, on the
same inputs.  Tolerance: atol 2e-5 on sdist, the figure tests/test_sample_counts.py holds this operator to
(`test_resample_padding_enters_the_logits_not_the_sample_positions`).  The inverse CDF turns an error e of the CDF into e / density
of s, so the rows are built with a density that stays within a factor 3 of uniform on every bin of non-zero width (w proportional
to width * (0.5 + rand)); bins without mass are either of zero width or lie where no sample position can fall (before / after the
only occupied bin: the CDF is exactly 0 / 1 there and 0 < u < 1).  tdist takes the same atol: near / far are chosen so that
|dt / ds| <= 1 over the whole ray (asserted below in float64), and so an error of s arrives in t no larger."""
import functools

import numpy as np
import pytest
import torch

from oracle import nlr_oracle as orc
from nerflidar_hip import _lib

DEV = "cuda:0"
ATOL = 2e-5
LAM = -1.5
N_PREV = (1, 2, 21, 22, 63, 64, 65, 512)
SAMPLES = (2, 3, 63, 64, 65, 1024)
D_TIE = 0.03125                                     # 2 / 64: on the 1/64 grid t_i - d == t_j and t_i + d == t_j happen exactly
NEAR = np.array([0.2, 0.05, 0.3], np.float32)
FAR = np.array([0.7, 0.5, 0.9], np.float32)


def T(a):
    return torch.from_numpy(np.array(a))


def _conditioned_weights(t, rng):
    """w proportional to width * (0.5 + rand): density within a factor 3 of uniform, zero-width bins without weight."""
    w = np.diff(t, axis=-1) * (0.5 + rng.random((t.shape[0], t.shape[1] - 1)))
    tot = w.sum(-1, keepdims=True)
    return (w / np.where(tot > 0, tot, 1.0)).astype(np.float32)


def _generic(n, rng):
    """Row 0 spans [0, 1] exactly, row 1 lies inside, row 2 has a zero-width bin at each end and one in the middle."""
    t = np.sort(rng.random((3, n + 1)), axis=-1).astype(np.float32)
    t[0, 0], t[0, -1] = 0.0, 1.0
    if n >= 4:
        t[2, 1], t[2, -2], t[2, n // 2] = t[2, 0], t[2, -1], t[2, n // 2 + 1]
    return t, _conditioned_weights(t, rng)


def _grid(n, rng):
    """Fenceposts on multiples of 1/64 (repeats = zero-width bins; with D_TIE fenceposts of the three lists coincide exactly: the
    tie rules t before t0 before t1).  Row 1: two equal neighbours and a third exactly D_TIE above them."""
    grid = np.arange(0, 65, dtype=np.float32) / 64
    t = np.sort(rng.choice(grid, size=(3, n + 1), replace=True), axis=-1).astype(np.float32)
    t[0, 0], t[0, -1] = 0.0, 1.0
    if n >= 2:
        t[1, 0], t[1, 1], t[1, 2:] = 0.25, 0.25, np.maximum(t[1, 2:], 0.25 + D_TIE)
        t[1, 2] = 0.25 + D_TIE
        t[1] = np.sort(t[1])
    else:
        t[1] = (0.25, 0.25 + D_TIE)
    for r in range(3):                               # a row needs one bin of non-zero width to carry mass
        if t[r, 0] == t[r, -1]:
            t[r, -1] = t[r, 0] + D_TIE
    return t, _conditioned_weights(t, rng)


def _one_bin(n, rng):
    """All weight in one bin (first, middle, last); the others keep their width and have no mass."""
    t = np.sort(rng.random((3, n + 1)), axis=-1).astype(np.float32)
    w = np.zeros((3, n), np.float32)
    for r, j in enumerate((0, n // 2, n - 1)):
        w[r, j] = 1.0
    return t, w


def _all_equal(n, rng):
    """Every fencepost of a row at one value (0, 0.4, 1): zero-width bins only, every logit -inf without dilation."""
    t = np.repeat(np.array([[0.0], [0.4], [1.0]], np.float32), n + 1, axis=1)
    return t, np.full((3, n), 1.0 / n, np.float32)


BUILDERS = {"generic": _generic, "grid": _grid, "one_bin": _one_bin, "all_equal": _all_equal}


@functools.lru_cache(maxsize=None)
def _rows(kind, n):
    rng = np.random.default_rng(7000 + 10 * n + sorted(BUILDERS).index(kind))
    t, w = BUILDERS[kind](n, rng)
    t.setflags(write=False)
    w.setflags(write=False)
    return t, w


@functools.lru_cache(maxsize=None)
def _jitter():
    j = np.array([0.1, 0.5, 0.9], np.float32)
    j.setflags(write=False)
    return j


@functools.lru_cache(maxsize=None)
def _reference(kind, n, dilation, S, jitter):
    """(sdist, tdist) of the float32 oracle chain, read-only."""
    t, w = (T(a) for a in _rows(kind, n))
    if dilation > 0:
        t, w = orc.max_dilate_weights(t, w, dilation, (0., 1.), renormalize=True)
        t, w = t[..., 1:-1], w[..., 1:-1]            # the caller drops the first and last fencepost / weight
    rand_u = T(_jitter())[:, None] if jitter else None
    s = orc.sample_intervals(t, orc.resample_logits(t, w, 1.0, 0.0), S, (0., 1.), rand_u=rand_u)
    _, s_to_t = orc.construct_ray_warps(T(NEAR)[:, None], T(FAR)[:, None], LAM)
    out = s.numpy(), s_to_t(s).numpy()
    for a in out:
        a.setflags(write=False)
    return out


def _resample(t, w, dilation, S, jitter, order=(0, 1, 2)):
    order = list(order)
    n = w.shape[1]
    cu = lambda a: T(a[order]).contiguous().to(DEV)
    sd = torch.full((3, S + 1), float("nan"), device=DEV)
    td = torch.full((3, S + 1), float("nan"), device=DEV)
    pt, pw, nr, fr = cu(t), cu(w), cu(NEAR), cu(FAR)
    jt = cu(_jitter()) if jitter else None
    rc = _lib.lib().nlr_resample_level(_lib.ptr(pt), _lib.ptr(pw), n, float(dilation), 1.0, 0.0, S, _lib.ptr(jt), _lib.ptr(nr),
                                       _lib.ptr(fr), LAM, 3, _lib.ptr(sd), _lib.ptr(td), None)
    _lib.check(rc)
    torch.cuda.synchronize()
    return sd.cpu().numpy(), td.cpu().numpy()


def _check(kind, n, dilation, S, jitter):
    t, w = _rows(kind, n)
    ref_s, ref_t = _reference(kind, n, dilation, S, jitter)
    sd, td = _resample(t, w, dilation, S, jitter)
    assert np.isfinite(ref_s).all() and np.isfinite(ref_t).all(), (kind, n, dilation, S, jitter)
    es, et = np.abs(sd - ref_s).max(), np.abs(td - ref_t).max()
    print(f"{kind:9s} n_prev {n:3d} S {S:4d} dilation {dilation:<7g} jitter {int(jitter)}: max |ds| {es:.2e}  max |dt| {et:.2e}")
    np.testing.assert_allclose(sd, ref_s, atol=ATOL, rtol=0, err_msg=str((kind, n, dilation, S, jitter)))
    np.testing.assert_allclose(td, ref_t, atol=ATOL, rtol=0, err_msg=str((kind, n, dilation, S, jitter)))
    assert (np.diff(sd, axis=-1) >= 0).all() and sd.min() >= 0 and sd.max() <= 1


def test_warp_does_not_stretch_s():
    """|dt / ds| <= 1 on [0, 1] for the three (near, far) pairs, in float64: the sdist tolerance holds for tdist."""
    s = torch.linspace(0, 1, 4001, dtype=torch.float64)[None, :]
    _, s_to_t = orc.construct_ray_warps(T(NEAR.astype(np.float64))[:, None], T(FAR.astype(np.float64))[:, None], LAM)
    slope = np.diff(s_to_t(s).numpy(), axis=-1) / np.diff(s.numpy(), axis=-1)
    assert slope.min() > 0 and slope.max() <= 1.0, slope.max()


@pytest.mark.gpu
@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("n_prev", N_PREV)
def test_run_boundaries_against_the_oracle(n_prev, S):
    """Generic rows and rows on the 1/64 grid (exact ties between the three lists, zero-width bins), dilation 0 and D_TIE; jitter
    on for the generic rows of the dilated case and off elsewhere (the jitter only shifts u, so one leg per size carries it)."""
    for kind in ("generic", "grid"):
        for dilation in (0.0, D_TIE):
            _check(kind, n_prev, dilation, S, jitter=(kind == "generic" and dilation > 0))


@pytest.mark.gpu
@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("n_prev,S", [(1, 2), (21, 64), (22, 65), (64, 63), (65, 3), (512, 1024)])
def test_hard_rows_against_the_oracle(n_prev, S, jitter):
    """All fenceposts equal, all weight in one bin, and a dilation larger than the domain (every t - d clips to 0, every t + d to 1)."""
    _check("all_equal", n_prev, 0.0, S, jitter)       # every logit -inf: the reference and the kernel both return the fencepost
    _check("all_equal", n_prev, D_TIE, S, jitter)
    _check("one_bin", n_prev, 0.0, S, jitter)
    _check("one_bin", n_prev, D_TIE, S, jitter)
    for kind in ("generic", "grid", "one_bin", "all_equal"):
        _check(kind, n_prev, 1.5, S, jitter)


@pytest.mark.gpu
@pytest.mark.parametrize("n_prev,S", [(21, 64), (64, 65), (65, 63), (512, 1024)])
def test_rows_do_not_depend_on_the_ray_order(n_prev, S):
    """A ray's row is a function of that ray alone: the same three rays in another order give the same rows bit for bit."""
    for kind, dilation, jitter in (("generic", D_TIE, True), ("grid", D_TIE, False), ("generic", 0.0, False)):
        t, w = _rows(kind, n_prev)
        sd, td = _resample(t, w, dilation, S, jitter)
        order = (2, 0, 1)
        sp, tp = _resample(t, w, dilation, S, jitter, order)
        assert np.array_equal(sp.view(np.uint32), sd[list(order)].view(np.uint32)), (kind, dilation)
        assert np.array_equal(tp.view(np.uint32), td[list(order)].view(np.uint32)), (kind, dilation)
