"""Compositing (forward, backward, segment-record tail) at every sample count the library accepts, against float64.

`nlr_composite_kernel` and `nlr_composite_bwd_kernel` give one 64-lane wavefront to a ray; lane l owns the samples
[l * per, (l + 1) * per) with per = ceil(S / 64), four rays share a workgroup.  The fixtures of tests/test_hip_parity.py and
tests/test_training.py reach per = 1 and 2 only.  Here S runs over every per in 1..8, full and ragged, with rays built to sit on
the edges of that layout (zero-width intervals at a lane boundary and at S - 2, a single occupied sample at the first sample of a
middle lane, mass in the last sample only, empty / saturated / faint rays, |d| = 50 and 1e-3, tied semantic classes).

Acceptance rule (per output, per ray): max |gpu - o64| <= 4 * E32(class) + 8 ulp_f32 * scale(ray), where o32 / o64 are the oracle
(oracle/nlr_oracle.py, pinned to the reference by tests/test_oracle_golden.py and tests/test_training.py) on float32 / float64
tensors, E32(class) is the largest max |o32 - o64| over the rays of the ray's class in that case and scale(ray) = max(max |o64|, 1)
(gradients: the ray's own max |o64|, no floor).  E32 is taken over seven float32 evaluations of the oracle that differ in the exp
alone: torch.exp, every result one float32 step up, every result one step down, and four seeded per-element choices of up / down.
Reason: a device expf is accurate to 1 ulp (HIP's documented bound), while torch.exp on the CPU is correctly rounded on nearly every
input, so one run measures torch's exp and not float32.  alpha = 1 - exp(-dd) turns one ulp of exp (6e-8) into 6e-8 / dd of alpha (the
reference's own formula), acc sums those errors and depth averages them.  Measured on the float32 oracle alone (no kernel), largest
class, one run -> seven runs: acc at S = 512 5.8e-7 -> 3.5e-5 (|d| = 50), depth at S = 512 transparent 3.9e-6 -> 1.0e-4 (faint),
distance_mean at S = 512 7.4e-7 -> 6.5e-5, acc at S = 64 and on the generic class unchanged at 1e-7 .. 1e-6.  Every line of
profiles/sample_counts_accuracy.txt carries both figures.
The factor 4 covers the summation order (per-lane partials + wave scan against a
sequential cumsum, both a small multiple of S ulp), the 8 ulp floor the rays where the float32 oracle happens to be exact.
One more term comes from the number format alone: 2^-126, the smallest normal float32.  The gradient of a saturated ray is e^-100 or
less; below 2^-126 float32 keeps no relative precision (subnormals are 2^-149 apart) and a device exp may flush to zero, so nothing
can be asked there.  It decides 1 to 3 rays in six backward cases (S = 2, 63, 96), all with exact gradients below 2^-126.
The percentile check lets the returned value move by 4 ulp: see `_pct_window` for the float32 oracle's own figures.
Every test prints what it compares (pytest -s): the table of one run is profiles/sample_counts_accuracy.txt."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

from oracle import nlr_oracle as orc
from nerflidar_hip import _lib, config as nconfig, lidar as nlidar, weights as nweights

DEV = "cuda:0"


def T(a):
    """A tensor with its own memory (the cached inputs and references are read-only arrays)."""
    return torch.from_numpy(np.array(a))


ULP = float(np.finfo(np.float32).eps)       # 2^-23
TINY = float(np.finfo(np.float32).tiny)     # 2^-126: below it float32 has no relative precision (and a GPU exp may flush to zero)
FAR = 2.5
SCALE_FACTOR = 0.004
SAMPLE_COUNTS = (1, 2, 63, 64, 65, 96, 127, 129, 200, 256, 320, 449, 511, 512)
ALL_K = ((0, True), (0, False), (1, True), (19, True), (19, False), (32, False))     # (class_num, intensity) at S = 200 and 512
FWD_CASES = [(S, K, it, opq) for S in SAMPLE_COUNTS for K, it in (ALL_K if S in (200, 512) else ((19, True),)) for opq in (True, False)]
FWD_KEYS = ("weights", "rgb", "depth", "semantic", "intensity", "acc", "distance_mean", "points")
PCT_KEYS = ("distance_percentile_5", "distance_median", "distance_percentile_95")
PCT_P = tuple(float(np.float32(p) / np.float32(100)) for p in (5, 50, 95))           # tensor([5, 50, 95]) / 100 in float32
GUARD = 64


def _per(S):
    return (S + 63) // 64


def _softmax64(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


# ---- the shared input builder (plain numpy) ---------------------------------------------------------------------------------------
def _rays(S, K, seed):
    """float32 inputs of one case: tdist [N,S+1] sorted in [0.05, 2], density, dirs, rgbs, sem (softmax rows), intensity, far = 2.5,
    origins, cotangents, and per ray its class name (`cls`) and, on the label-tie rays, the label a tie must give (`tie_label`, else -1).
    Three rays per class with different draws, rows permuted so that classes mix inside a 4-ray workgroup, generic rays appended until
    N % 4 == 1 (the last workgroup holds one ray)."""
    rng = np.random.default_rng(1000 * seed + S)
    per = _per(S)
    # The optical depth of the thinnest non-empty rays: 1e-2, i.e. acc ~ 1e-2, far from acc ~ eps where clamp_min(eps) makes float32
    # and float64 disagree by O(1); and at least 8e-5 per sample, since alpha = 1 - exp(-dd) turns the one ulp (6e-8) a float32 exp may
    # be off into 6e-8 / dd of alpha, which the density gradient of such a ray carries undamped (3e-3 at S = 512 with 1e-2 in all).
    thin = 1e-2 * max(1.0, S / 128)
    names = ["generic", "zero_width", "empty", "saturated", "last_only", "one_sample", "faint", "long", "short", "ties"]
    if S < 4:
        names.remove("zero_width")
    if K < 2:
        names.remove("ties")
    cls = [c for c in names for _ in range(3)]
    while len(cls) % 4 != 1:
        cls.append("generic")
    N = len(cls)
    tdist = np.sort(rng.uniform(0.05, 2.0, (N, S + 1)), axis=-1).astype(np.float32)
    density = (rng.random((N, S)) ** 4 * 40).astype(np.float32)
    dirs = rng.standard_normal((N, 3))
    dirs = dirs / np.linalg.norm(dirs, axis=-1, keepdims=True) * rng.uniform(0.8, 1.25, (N, 1))
    logits = rng.standard_normal((N, S, max(K, 1))) * 1.5
    tie_label = np.full(N, -1, np.int64)
    seen = {}
    for r, c in enumerate(cls):
        j = seen[c] = seen.get(c, -1) + 1                        # 0, 1, 2 within the class
        if c == "zero_width":
            lane = min(max(1, (S // per) * (j + 1) // 4), (S - 1) // per)
            for k in sorted({per * lane, S - 2, j}):             # a lane boundary, S - 2, and one more place
                tdist[r, k + 1] = tdist[r, k]
        elif c == "empty":
            density[r] = 0.0
        elif c == "saturated":
            density[r] = 1e4
        elif c == "last_only":
            density[r] = 0.0
            density[r, S - 1] = 50.0
        elif c == "one_sample":
            density[r] = 0.0
            density[r, per * (S // (2 * per))] = 50.0            # the first sample of a middle lane
        elif c == "faint":                                       # acc ~ 1e-2 in float64: well above eps = 1.19e-7 (see `thin`)
            length = (float(tdist[r, S]) - float(tdist[r, 0])) * np.linalg.norm(dirs[r])
            density[r] = -np.log1p(-thin * (1 + 0.3 * j)) / length
        elif c == "long":
            dirs[r] *= 50.0 / np.linalg.norm(dirs[r])
        elif c == "short":
            dirs[r] *= 1e-3 / np.linalg.norm(dirs[r])
        elif c == "ties":
            a, b = [(0, 1), (2, K - 2), (1, K - 1)][j] if K >= 4 else (0, 1)
            shared = rng.standard_normal(S)
            if j == 1 and K >= 4:                                # the tied pair loses to class K-1, which dominates alone
                logits[r, :, a] = logits[r, :, b] = shared
                logits[r, :, K - 1] += 6.0
                tie_label[r] = K - 1
            else:                                                # the tied pair dominates: the label is the lower index
                logits[r, :, a] = logits[r, :, b] = shared + 5.0
                tie_label[r] = min(a, b)
    # Conditioning, as for the faint class: a transparent ray whose optical depth is below thin / 2 (one or two draws of u^4 * 40 at
    # S <= 2, or |d| = 1e-3) is scaled up to `thin`.
    tau = (density.astype(np.float64) * np.diff(tdist.astype(np.float64), axis=-1)).sum(-1) * np.linalg.norm(dirs, axis=-1)
    for r, c in enumerate(cls):
        if c != "empty" and tau[r] < thin / 2:
            density[r] *= np.float32(thin / tau[r])
    sem = _softmax64(logits).astype(np.float32)                  # equal logit columns give bitwise equal probabilities
    out = {"tdist": tdist, "density": density, "dirs": dirs.astype(np.float32), "rgbs": rng.random((N, S, 3)).astype(np.float32),
           "sem": sem[..., :K], "intensity": rng.random((N, S)).astype(np.float32), "far": np.full(N, FAR, np.float32),
           "origins": rng.uniform(-0.5, 0.5, (N, 3)).astype(np.float32)}
    for k, sh in (("rgb", (N, 3)), ("depth", (N,)), ("semantic", (N, K)), ("intensity", (N,)), ("acc", (N,)), ("weights", (N, S))):
        out["cot_" + k] = rng.standard_normal(sh).astype(np.float32)
    perm = np.random.default_rng(7).permutation(N)
    out = {k: np.ascontiguousarray(v[perm]) for k, v in out.items()}
    out["cls"] = np.array(cls)[perm]
    out["tie_label"] = tie_label[perm]
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _inputs(S, K):
    return _rays(S, K, seed=3)


# ---- CPU references: the oracle on float32 and on float64 tensors, once per case ------------------------------------------------
def _oracle_forward(g, K, has_int, opaque, dtype, leaves=False):
    t = lambda k: T(g[k]).to(dtype)
    dens, rgbs, sem, inten = t("density"), t("rgbs"), (t("sem") if K else None), (t("intensity") if has_int else None)
    if leaves:
        for x in (dens, rgbs, sem, inten):
            if x is not None:
                x.requires_grad_(True)
    w = orc.compute_alpha_weights(dens, t("tdist"), t("dirs"), opaque)
    r = orc.volumetric_rendering(rgbs, w, t("tdist"), 1.0, t("far")[:, None], True, semantic=sem, intensity=inten)
    r["weights"] = w
    return r, (dens, rgbs, sem, inten)


_TORCH_EXP = torch.exp
EXP_VARIANTS = (None, "up", "down", 1, 2, 3, 4)


class _exp_within_one_ulp:
    """Context: while the oracle runs, torch.exp of a float32 tensor returns a neighbour of its result: every element one float32
    step up, every element one step down, or up / down per element from a seeded draw (None: torch.exp as it is).  exp(0) and exp(-inf) stay exact."""

    def __init__(self, variant):
        self.variant = variant
        self.gen = torch.Generator().manual_seed(int(variant)) if isinstance(variant, int) else None

    def __call__(self, x):
        y = _TORCH_EXP(x)
        if y.dtype != torch.float32 or self.variant is None:
            return y
        with torch.no_grad():
            up = torch.nextafter(y, torch.full_like(y, torch.inf))
            down = torch.nextafter(y, torch.zeros_like(y))
            if self.variant == "up":
                z = up
            elif self.variant == "down":
                z = down
            else:
                z = torch.where(torch.rand(y.shape, generator=self.gen) < 0.5, up, down)
            step = torch.where((x == 0) | ~torch.isfinite(x), torch.zeros_like(y), z - y)     # exp(0) = 1 and exp(-inf) = 0 are exact

        return y + step          # exactly z; the gradient is that of exp

    def __enter__(self):
        torch.exp = self
        return self

    def __exit__(self, *exc):
        torch.exp = _TORCH_EXP


@functools.lru_cache(maxsize=None)
def _forward_ref(S, K, has_int, opaque):
    """64 -> outputs of the oracle on float64 tensors (as float64 numpy arrays), plus `cw`: the clipped CDF [N, S+3] of the percentile
    search; 32 -> the same on float32 tensors; "e32" -> per output and ray, the largest |o32 - o64| over the evaluations of
    `EXP_VARIANTS`."""
    g = _inputs(S, K)

    def run(gi, dtype):
        with torch.no_grad():
            r, _ = _oracle_forward(gi, K, has_int, opaque, dtype)
            r["points"] = (T(gi["origins"]).to(dtype) + r["depth"][:, None] * T(gi["dirs"]).to(dtype)) / \
                torch.tensor(SCALE_FACTOR, dtype=torch.float32).to(dtype)
            bg_w = (1 - r["acc"][:, None]).clamp_min(0.)
            r["cw"] = orc.integrate_weights(torch.cat([r["weights"], bg_w], dim=-1))
        return {k: v.double().numpy() for k, v in r.items()}

    out = {64: run(g, torch.float64), 32: run(g, torch.float32)}
    out["e32"] = {k: np.zeros(g["density"].shape[0]) for k in out[64]}
    out["e32_1"] = {}
    for variant in EXP_VARIANTS:
        with _exp_within_one_ulp(variant):
            o32 = run(g, torch.float32)
        for k in o32:
            out["e32"][k] = np.maximum(out["e32"][k], _per_ray_max(o32[k] - out[64][k]))
            if variant is None:
                out["e32_1"][k] = _per_ray_max(o32[k] - out[64][k])
    for d in out.values():
        for a in d.values():
            a.setflags(write=False)
    return out


def _loss(r, w, g, keys):
    """tests/test_training.py::_loss over the outputs in `keys` (every output and the weights by default)."""
    tot = 0.0
    for k in keys:
        x = w if k == "weights" else r[k]
        tot = tot + (x * T(g["cot_" + k]).to(x.device, x.dtype)).sum()
    return tot


ALL_COT = ("rgb", "depth", "semantic", "intensity", "acc", "weights")


@functools.lru_cache(maxsize=None)
def _backward_ref(S, K, has_int, opaque, keys=ALL_COT, with_rgbs=True):
    """64 / 32 -> gradients of the loss with respect to density / rgbs / sem / intensity (None where the input is absent) through the
    oracle on float64 / float32 leaves; "e32" as in `_forward_ref`."""
    g = _inputs(S, K)
    keys = tuple(k for k in keys if not (k == "semantic" and not K) and not (k == "intensity" and not has_int))

    def run(gi, dtype):
        r, leaves = _oracle_forward(gi, K, has_int, opaque, dtype, leaves=True)
        if not with_rgbs:     # training.volumetric_render(rgbs=None): the rgb output is bg_w * bg alone
            r["rgb"] = (1 - r["acc"][:, None]).clamp_min(0.) * torch.ones(1, 3, dtype=dtype)
        used = [x for x in leaves if x is not None]
        grads = torch.autograd.grad(_loss(r, r["weights"], gi, keys), used, allow_unused=True)
        it = iter(grads)
        res = {}
        for name, x in zip(("density", "rgbs", "sem", "intensity"), leaves):
            gx = next(it) if x is not None else None
            res[name] = None if x is None else (np.zeros(tuple(x.shape)) if gx is None else gx.double().numpy())
        return res

    out = {64: run(g, torch.float64), 32: run(g, torch.float32)}
    out["e32"] = {k: np.zeros(g["density"].shape[0]) for k, v in out[64].items() if v is not None}
    out["e32_1"] = {}
    for variant in EXP_VARIANTS:
        with _exp_within_one_ulp(variant):
            o32 = run(g, torch.float32)
        for k in out["e32"]:
            out["e32"][k] = np.maximum(out["e32"][k], _per_ray_max(o32[k] - out[64][k]))
            if variant is None:
                out["e32_1"][k] = _per_ray_max(o32[k] - out[64][k])
    return out


def _per_ray_max(a):
    a = np.abs(np.asarray(a, np.float64))
    return a.reshape(a.shape[0], -1).max(-1) if a.size else np.zeros(a.shape[0])


def _class_max(per_ray, cls):
    """Per ray: the maximum of `per_ray` over the rays of its class."""
    out = np.zeros_like(per_ray)
    for c in np.unique(cls):
        out[cls == c] = per_ray[cls == c].max()
    return out


def _ratio(err, bound):
    return np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))


def _accept(case, name, got, e32_ray, o64, cls, floor=1.0, e32_single=None):
    """The acceptance rule of the module docstring; prints one line per output: case, output, E32 (seven runs; one run), the GPU error,
    the worst ratio of a ray's error to its bound, and the same against the bound from the single float32 run without 2^-126."""
    e32 = _class_max(e32_ray, cls)
    scale = np.maximum(_per_ray_max(o64), floor)
    bound = 4 * e32 + 8 * ULP * scale + TINY
    err = _per_ray_max(np.asarray(got, np.float64) - o64)
    ok = np.isfinite(err) & (err <= bound)
    ratio = _ratio(err, bound)
    i = int(np.argmax(ratio))
    one = ""
    if e32_single is not None:
        e1 = _class_max(e32_single, cls)
        r1 = _ratio(err, 4 * e1 + 8 * ULP * scale)
        one = (f"; one run: E32 {e1.max():.3e} worst err/bound {r1.max():.3f}, {int((r1 > 1).sum())} rays beyond; "
               f"seven runs without 2^-126: {int((err > bound - TINY).sum())} rays beyond")
    print(f"{case} {name}: E32 {e32.max():.3e} gpu_err {err.max():.3e} worst err/bound {ratio[i]:.3f} (ray {i}, {cls[i]})" + one)
    assert ok.all(), (f"{case} {name}: rays {np.flatnonzero(~ok).tolist()} ({sorted(set(cls[~ok]))}) beyond 4 E32 + 8 ulp scale + 2^-126: "
                      f"err {err[~ok]} bound {bound[~ok]}")
    return bound


# ---- CPU self-checks: they hold the inputs, not the kernels -------------------------------------------------------------------
@pytest.mark.parametrize("S", SAMPLE_COUNTS)
def test_builder_yields_finite_float64_references(S):
    K = 19
    g = _inputs(S, K)
    N = g["density"].shape[0]
    per = _per(S)
    assert N % 4 == 1 and (np.diff(g["tdist"], axis=-1) >= 0).all() and g["tdist"].min() >= 0.05 and g["tdist"].max() <= 2.0
    want = {"generic", "empty", "saturated", "last_only", "one_sample", "faint", "long", "short", "ties"} | ({"zero_width"} if S >= 4 else set())
    assert set(g["cls"]) == want and all((g["cls"] == c).sum() >= 3 for c in want)
    for c in range(0, N - 3, 4):       # the permutation mixes classes inside the 4-ray workgroups
        assert len(set(g["cls"][c:c + 4])) >= 2
    if S >= 4:
        zw = g["tdist"][g["cls"] == "zero_width"]
        assert ((np.diff(zw, axis=-1) == 0).sum(-1) >= 2).all() and (zw[:, S - 1] == zw[:, S - 2]).all()
        assert all(any(zw[i, k + 1] == zw[i, k] for k in range(per, S - 1, per)) for i in range(3))
    one = g["density"][g["cls"] == "one_sample"]
    assert ((one > 0).sum(-1) == 1).all() and (np.argmax(one, -1) % per == 0).all()
    np.testing.assert_allclose(g["sem"].sum(-1), 1.0, atol=1e-6)
    for opaque in (True, False):
        ref = _forward_ref(S, K, True, opaque)[64]
        for k, v in ref.items():
            assert np.isfinite(v).all(), (k, opaque)
        if not opaque:
            faint = ref["acc"][g["cls"] == "faint"]
            assert (faint > 5e-3).all() and (faint < 2e-2 * max(1.0, S / 128)).all()
        grads = _backward_ref(S, K, True, opaque)[64]
        for k, v in grads.items():
            assert np.isfinite(v).all(), (k, opaque)
    # the tie rays: two bitwise equal class columns (the oracle's own strided sums may still order them differently, so only the
    # kernel is held to the exact tie rule), and the expected label is the maximum up to that tie
    for r in np.flatnonzero(g["cls"] == "ties"):
        cols = g["sem"][r].T
        twins = [(a, b) for a in range(K) for b in range(a + 1, K) if (cols[a] == cols[b]).all()]
        assert len(twins) == 1
        sem64 = _forward_ref(S, K, True, False)[64]["semantic"][r]
        lab = g["tie_label"][r]
        assert sem64[lab] >= sem64.max() * (1 - 1e-12) and (lab == twins[0][0] or sem64[lab] > 1.5 * sem64[twins[0][0]])


@pytest.mark.parametrize("S", SAMPLE_COUNTS)
def test_float32_oracle_error_per_class_is_small(S):
    """A condition on the inputs: within every class the float32 oracle is within 2e-3 (relative to the ray's own scale) of the
    float64 one, in every forward output and every gradient.  Otherwise 4 * E32 would admit a wrong kernel (this is why the faint
    rays have acc ~ 1e-2 and not ~ eps, where clamp_min(eps) makes the two precisions disagree by O(1))."""
    K = 19
    g = _inputs(S, K)
    for opaque in (True, False):
        f = _forward_ref(S, K, True, opaque)
        for k in FWD_KEYS:
            rel = f["e32"][k] / np.maximum(_per_ray_max(f[64][k]), 1.0)
            assert rel.max() <= 2e-3, (k, opaque, rel.max(), g["cls"][rel.argmax()])
        assert f["e32"]["cw"].max() <= 2e-3
        b = _backward_ref(S, K, True, opaque)
        for k in ("density", "rgbs", "sem", "intensity"):
            scale = _per_ray_max(b[64][k])
            err = b["e32"][k]
            ok = err <= 2e-3 * scale + TINY                     # (TINY: see the module docstring)
            assert ok.all(), (k, opaque, err[~ok], scale[~ok], g["cls"][~ok])


def _pct_window(v):
    """How far the percentile check lets a returned float32 distance v move before it evaluates the CDF: 4 ulp of max(|v|, 1).  v is
    ta[i0] + off * (ta[i1] - ta[i0]) in float32 (one division, one product, one sum), and where all the mass sits in one interval of
    width 2 / S one ulp of v is 1e-5 of F.  Measured on the float32 ORACLE's own percentiles (`test_float32_oracle_percentiles_...`,
    K = 19 cases): with v taken exactly 342 of 2 724 rays miss the CDF-space rule, by up to 277 x tol (S = 96, opaque, last-only); with
    this window none does, worst 0.20 x tol."""
    return 4 * ULP * max(abs(float(v)), 1.0)


def _cdf_miss(t, c, v, p, window):
    """max(F((v - window)-) - p, p - F((v + window)+), 0) on the float64 CDF through (t, c)."""
    fm = _cdf_sides(t, c, max(v - window, t[0]))[0]
    fp = _cdf_sides(t, c, min(v + window, t[-1]))[1]
    return max(fm - p, p - fp, 0.0)


def test_float32_oracle_percentiles_need_the_value_window():
    """The CDF-space percentile rule applied to the float32 oracle's own percentiles (no kernel involved), tol from the single float32
    run: with the returned value taken exactly the float32 oracle itself misses; with `_pct_window` it passes everywhere.  Prints the
    counts that stand in `_pct_window` and in profiles/sample_counts_accuracy.txt."""
    rays = exact_miss = 0
    worst_exact = worst_window = 0.0
    for S, K, has_int, opaque in FWD_CASES:
        if (K, has_int) != (19, True):
            continue
        g = _inputs(S, K)
        ref = _forward_ref(S, K, has_int, opaque)
        N = g["density"].shape[0]
        t_aug = np.concatenate([g["tdist"].astype(np.float64), np.full((N, 1), FAR)], axis=-1)
        tol = 4 * _class_max(ref["e32_1"]["cw"], g["cls"]) + 8 * ULP
        for key, p in zip(PCT_KEYS, PCT_P):
            for r in range(N):
                v = ref[32][key][r]
                m0 = _cdf_miss(t_aug[r], ref[64]["cw"][r], v, p, 0.0) / tol[r]
                m1 = _cdf_miss(t_aug[r], ref[64]["cw"][r], v, p, _pct_window(v)) / tol[r]
                rays += 1
                exact_miss += m0 > 1
                worst_exact, worst_window = max(worst_exact, m0), max(worst_window, m1)
    print(f"float32 oracle percentiles under the CDF-space rule: {rays} rays; v exact: {exact_miss} beyond tol, worst {worst_exact:.1f} x tol; "
          f"v within 4 ulp: worst {worst_window:.2f} x tol")
    assert exact_miss > 0 and worst_window <= 1.0


def test_resample_padding_enters_the_logits_not_the_sample_positions():
    """ZI/models.py:352-355: logits = anneal * log(weights + resample_padding), -inf for zero-width bins; ZI/stepfun.py:203-206: the
    deterministic sample positions are linspace(1/(2S), 1 - 1/(2S) - eps, S) whatever the padding.  `orc.resample_logits` +
    `orc.sample_intervals` against that formula restated in float64 numpy (np.interp inverts the CDF, stepfun.py:164-172)."""
    rng = np.random.default_rng(5)
    n, m, S = 6, 40, 24
    t = np.sort(rng.random((n, m + 1)), axis=-1).astype(np.float32)
    t[1, 10] = t[1, 9]
    w = rng.random((n, m)).astype(np.float32)
    w[2, :20] = 0.0
    w = w / w.sum(-1, keepdims=True)
    u = orc.sample_u(S).double().numpy()
    pad = 1 / (2 * S)
    np.testing.assert_allclose(u, np.linspace(pad, 1. - pad - orc.EPS, S), atol=1e-7, rtol=0)
    for anneal, padding in ((1.0, 0.0), (0.25, 0.0), (0.7, 0.01), (0.25, 0.01)):
        got = orc.sample_intervals(T(t), orc.resample_logits(T(t), T(w), anneal, padding), S, (0., 1.)).numpy()
        for i in range(n):
            t64, w64 = t[i].astype(np.float64), w[i].astype(np.float64)
            with np.errstate(divide="ignore"):
                lg = np.where(t64[1:] > t64[:-1], anneal * np.log(w64 + padding), -np.inf)
            p = np.exp(lg - lg.max())
            p = p / p.sum()
            cw = np.concatenate([[0.0], np.minimum(1, np.cumsum(p[:-1])), [1.0]])
            cen = np.interp(u, cw, t64)
            mid = (cen[1:] + cen[:-1]) / 2
            want = np.concatenate([[max(2 * cen[0] - mid[0], 0.0)], mid, [min(2 * cen[-1] - mid[-1], 1.0)]])
            np.testing.assert_allclose(got[i], want, atol=2e-5, rtol=0)
    # the padding changes the result (it is not dropped), and zero-weight bins receive samples only with it
    a = orc.sample_intervals(T(t), orc.resample_logits(T(t), T(w), 1.0, 0.0), S, (0., 1.)).numpy()
    b = orc.sample_intervals(T(t), orc.resample_logits(T(t), T(w), 1.0, 0.01), S, (0., 1.)).numpy()
    assert a[2].min() >= t[2, 20] - 1e-6 and b[2].min() < t[2, 20] - 1e-3


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def cu(a):
    return T(a).contiguous().to(DEV)


def npy(t):
    return t.detach().cpu().numpy()


def _guarded(n_elems, dtype, fill):
    """A buffer of n_elems with GUARD elements behind it: (view of the payload, whole buffer)."""
    whole = torch.full((n_elems + GUARD,), fill, dtype=dtype, device=DEV)
    return whole[:n_elems], whole


def _composite_level(g, S, K, has_int, opaque, with_sem=True):
    """nlr_composite_level as tests/test_hip_parity.py::test_composite calls it, every output NaN-filled with a guard behind it."""
    N = g["density"].shape[0]
    ins = {k: cu(g[k]) for k in ("density", "tdist", "dirs", "far", "origins")}
    rgbs = cu(g["rgbs"].transpose(2, 0, 1))                              # channel-major [3,N,S]
    sem = cu(g["sem"].transpose(2, 0, 1)) if K and with_sem else None    # class-major [K,N,S]
    inten = cu(g["intensity"]) if has_int else None
    shapes = dict(rgb=3, depth=1, semantic=max(K, 1), intensity=1, acc=1, distance_mean=1, distance_median=1, distance_percentile_5=1,
                  distance_percentile_95=1, points=3)
    out = _lib.NlrOut()
    res, whole = {}, {}
    for k, c in shapes.items():
        res[k], whole[k] = _guarded(N * c, torch.float32, float("nan"))
        setattr(out, k, res[k].data_ptr())
    res["labels"], whole["labels"] = _guarded(N, torch.int32, -7)
    out.labels = res["labels"].data_ptr()
    res["weights"], whole["weights"] = _guarded(N * S, torch.float32, float("nan"))
    rc = _lib.lib().nlr_composite_level(_lib.ptr(ins["density"]), _lib.ptr(ins["tdist"]), _lib.ptr(ins["dirs"]), _lib.ptr(rgbs), _lib.ptr(sem),
                                        _lib.ptr(inten), _lib.ptr(ins["far"]), _lib.ptr(ins["origins"]), N, S, K, int(opaque), 1.0, 1,
                                        SCALE_FACTOR, _lib.ptr(res["weights"]), C.byref(out), None, None)
    torch.cuda.synchronize()
    return rc, {k: npy(v) for k, v in res.items()}, {k: npy(v[-GUARD:]) for k, v in whole.items()}, shapes


def _cdf_sides(t, c, v):
    """(F(v-), F(v+)) of the piecewise-linear CDF through the fenceposts t (non-decreasing) and values c: they differ only where
    fenceposts repeat (a zero-width interval carries a jump)."""
    lo, hi = np.searchsorted(t, v, side="left"), np.searchsorted(t, v, side="right")
    if lo < hi:                                   # v is a fencepost: t[lo .. hi-1] == v
        return c[lo], c[hi - 1]
    f = c[lo - 1] + (c[lo] - c[lo - 1]) * (v - t[lo - 1]) / (t[lo] - t[lo - 1])
    return f, f


@pytest.mark.gpu
@pytest.mark.parametrize("S,K,has_int,opaque", FWD_CASES)
def test_composite_forward_against_float64(S, K, has_int, opaque):
    """Every output under the acceptance rule; the percentiles in CDF space (F(v-) - tol <= p <= F(v+) + tol with F the float64
    piecewise-linear CDF, tol = 4 E32(cw) + 8 ulp), where v is taken as known to 4 ulp of max(|v|, 1): it is a float32 formed by one
    division, one product and one sum of float32 (ta[i0] + off * (ta[i1] - ta[i0])), and where the CDF is steep (all the mass in an
    interval of width 2 / S) one ulp of v is 1e-5 of F; labels; tails."""
    g = _inputs(S, K)
    cls, N = g["cls"], g["density"].shape[0]
    ref = _forward_ref(S, K, has_int, opaque)
    e32, o64 = ref["e32"], ref[64]
    case = f"fwd S={S} K={K} int={int(has_int)} {'opaque' if opaque else 'transparent'}"
    rc, got, guards, shapes = _composite_level(g, S, K, has_int, opaque)
    _lib.check(rc)

    # tails: every promised element written, nothing behind the N-th ray touched
    for k, v in guards.items():
        assert (v == -7).all() if k == "labels" else np.isnan(v).all(), f"{case}: {k} written past ray {N - 1}"
    written = set(shapes) | {"weights"}
    if not K:
        written -= {"semantic"}
        assert (got["labels"] == -7).all(), "K = 0: the labels buffer must stay untouched"
        assert np.isnan(got["semantic"]).all()
    if not has_int:
        written -= {"intensity"}
        assert np.isnan(got["intensity"]).all()
    for k in written:
        assert np.isfinite(got[k]).all(), f"{case}: {k} has unwritten or non-finite elements"

    bounds = {}
    for k in FWD_KEYS:
        if k in written:
            bounds[k] = _accept(case, k, got[k].reshape(N, -1), e32[k], o64[k].reshape(N, -1), cls, e32_single=ref["e32_1"][k])

    # percentiles in CDF space: p must lie between the one-sided CDF values at the returned distance
    t_aug = np.concatenate([g["tdist"].astype(np.float64), np.full((N, 1), FAR)], axis=-1)
    cw_tol = 4 * _class_max(e32["cw"], cls) + 8 * ULP
    cw_tol1 = 4 * _class_max(ref["e32_1"]["cw"], cls) + 8 * ULP
    for key, p in zip(PCT_KEYS, PCT_P):
        v = got[key].astype(np.float64)
        worst = nowin = 0.0
        for r in range(N):
            assert t_aug[r, 0] <= v[r] <= t_aug[r, -1], f"{case} {key}: ray {r} ({cls[r]}) {v[r]} outside [{t_aug[r, 0]}, {t_aug[r, -1]}]"
            miss = _cdf_miss(t_aug[r], o64["cw"][r], v[r], p, _pct_window(v[r]))
            nowin = max(nowin, _cdf_miss(t_aug[r], o64["cw"][r], v[r], p, 0.0) / cw_tol1[r])
            worst = max(worst, miss / cw_tol[r])
            assert miss <= cw_tol[r], f"{case} {key}: ray {r} ({cls[r]}) v {v[r]} p {p} misses the CDF by {miss}, tol {cw_tol[r]}"
        print(f"{case} {key}: E32(cw) {cw_tol.max() / 4:.3e} worst CDF miss/tol {worst:.3f}; one run, v taken exactly: worst miss/tol {nowin:.3f}")
        gen = cls == "generic"
        _accept(case, key + "[generic]", got[key][gen], e32[key][gen], o64[key][gen], cls[gen], e32_single=ref["e32_1"][key][gen])

    if K:
        sem64 = np.sort(o64["semantic"], axis=-1)
        margin = sem64[:, -1] - sem64[:, -2] if K > 1 else np.full(N, np.inf)
        sure = margin > bounds["semantic"]
        assert sure.sum() >= N // 2
        np.testing.assert_array_equal(got["labels"][sure], o64["semantic"].argmax(-1)[sure])
        ties = g["tie_label"] >= 0
        np.testing.assert_array_equal(got["labels"][ties], g["tie_label"][ties])
        if K == 1:
            assert (got["labels"] == 0).all()
        print(f"{case} labels: {int(sure.sum())} rays beyond the margin, {int(ties.sum())} tie rays")


@pytest.mark.gpu
def test_percentile_search_takes_the_last_fencepost_of_a_flat_cdf():
    """`cw[mid] <= p` in the percentile search (searchsorted(right=True) in the oracle): with one occupied sample whose weight is
    exactly 0.5 the CDF equals p = 0.5f on every fencepost behind it, and the median is the LAST of them, tdist[S] (`<` would give the
    first).  dd = (2 ln2f) * 0.5 * |(1,0,0)| = ln2f exactly, exp(-ln2f) is within 0.07 ulp of 0.5, so any exp within 0.9 ulp gives a
    weight of exactly 0.5; the test states that precondition before it uses it."""
    for S in (8, 200):
        per = _per(S)
        k = per * (S // (2 * per))
        N = 5
        tdist = np.empty((N, S + 1), np.float32)
        tdist[:, :k + 1] = np.linspace(0.25, 0.5, k + 1, dtype=np.float32)
        tdist[:, k + 1:] = np.linspace(1.0, 2.0, S - k, dtype=np.float32)
        density = np.zeros((N, S), np.float32)
        density[:, k] = np.float32(2) * np.float32(np.log(2.0))
        g = {"tdist": tdist, "density": density, "dirs": np.tile(np.array([[1, 0, 0]], np.float32), (N, 1)),
             "rgbs": np.zeros((N, S, 3), np.float32), "far": np.full(N, FAR, np.float32), "origins": np.zeros((N, 3), np.float32)}
        rc, got, _, _ = _composite_level(g, S, 0, False, False)
        _lib.check(rc)
        got = {key: v.reshape(N, -1) if key == "weights" else v for key, v in got.items()}
        assert (got["weights"][:, k] == 0.5).all(), "precondition: the occupied sample's weight is exactly 0.5"
        with torch.no_grad():
            w = orc.compute_alpha_weights(T(density), T(tdist), T(g["dirs"]), False)
            r = orc.volumetric_rendering(T(g["rgbs"]), w, T(tdist), 1.0, T(g["far"])[:, None], True)
        assert (w[:, k] == 0.5).all() and (r["distance_median"] == 2.0).all()
        np.testing.assert_array_equal(got["distance_median"], np.full(N, 2.0, np.float32))
        np.testing.assert_allclose(got["distance_percentile_5"], r["distance_percentile_5"].numpy(), atol=1e-6, rtol=0)
        np.testing.assert_allclose(got["distance_percentile_95"], r["distance_percentile_95"].numpy(), atol=1e-6, rtol=0)


def _volumetric_render(g, S, K, has_int, opaque, with_rgbs=True):
    from nerflidar_hip import training
    leaves = {"density": cu(g["density"]).requires_grad_(True), "rgbs": cu(g["rgbs"]).requires_grad_(True) if with_rgbs else None,
              "sem": cu(g["sem"]).requires_grad_(True) if K else None, "intensity": cu(g["intensity"]).requires_grad_(True) if has_int else None}
    r = training.volumetric_render(leaves["density"], cu(g["tdist"]), cu(g["dirs"]), leaves["rgbs"], leaves["sem"], leaves["intensity"],
                                   opaque_background=opaque, bg=1.0)
    return r, leaves


def _check_gradients(case, S, K, has_int, opaque, keys=ALL_COT, with_rgbs=True):
    g = _inputs(S, K)
    cls = g["cls"]
    ref = _backward_ref(S, K, has_int, opaque, keys, with_rgbs)
    r, leaves = _volumetric_render(g, S, K, has_int, opaque, with_rgbs)
    keys = tuple(k for k in keys if k == "weights" or k in r)
    _loss(r, r["weights"], g, keys).backward()
    torch.cuda.synchronize()
    for name, x in leaves.items():
        if x is None or (name == "rgbs" and not with_rgbs):
            continue
        got = npy(x.grad) if x.grad is not None else np.zeros(tuple(x.shape), np.float32)
        assert np.isfinite(got).all(), f"{case} d_{name}: non-finite"
        _accept(case, "d_" + name, got, ref["e32"][name], ref[64][name], cls, floor=0.0, e32_single=ref["e32_1"][name])
    return leaves


@pytest.mark.gpu
@pytest.mark.parametrize("opaque", [True, False])
@pytest.mark.parametrize("S", SAMPLE_COUNTS)
def test_composite_backward_against_float64_autograd(S, opaque):
    K, has_int = 19, True
    case = f"bwd S={S} K={K} {'opaque' if opaque else 'transparent'}"
    leaves = _check_gradients(case, S, K, has_int, opaque)
    if opaque:
        assert float(leaves["density"].grad[:, S - 1].abs().max()) == 0.0     # the opaque last interval does not come from the density
    # sem_detach: the semantic and intensity cotangents alone leave the density gradient exactly zero
    g = _inputs(S, K)
    r, lv = _volumetric_render(g, S, K, has_int, opaque)
    _loss(r, r["weights"], g, ("semantic", "intensity")).backward()
    assert float(lv["density"].grad.abs().max()) == 0.0 and float(lv["rgbs"].grad.abs().max()) == 0.0
    assert float(lv["sem"].grad.abs().max()) > 0.0 and float(lv["intensity"].grad.abs().max()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("opaque", [True, False])
@pytest.mark.parametrize("path", ["only_g_weights", "only_g_depth", "no_rgbs", "K0_with_intensity", "K32_without_intensity"])
def test_composite_backward_partial_paths(path, opaque):
    S = 200
    K, has_int, keys, with_rgbs = {"only_g_weights": (19, True, ("weights",), True), "only_g_depth": (19, True, ("depth",), True),
                                   "no_rgbs": (19, True, ALL_COT, False), "K0_with_intensity": (0, True, ALL_COT, True),
                                   "K32_without_intensity": (32, False, ALL_COT, True)}[path]
    _check_gradients(f"bwd S={S} {path} {'opaque' if opaque else 'transparent'}", S, K, has_int, opaque, keys, with_rgbs)


@pytest.mark.gpu
def test_composite_refuses_sample_and_class_counts_outside_its_range():
    """S = 0, S = 513 (both kernels) and K = 33 (forward): a non-zero code, a message from nlr_last_error, outputs untouched."""
    L = _lib.lib()
    N = 9
    # every input is large enough for the largest refused shape: a call that slipped through would still stay inside its buffers
    dens, td, dirs = torch.ones(N * 513, device=DEV), torch.arange(N * 514, device=DEV, dtype=torch.float32), torch.ones(N * 3, device=DEV)
    big = torch.zeros(33 * N * 513, device=DEV)
    for S, K, word in ((0, 19, b"S=0"), (513, 19, b"S=513"), (64, 33, b"class_num 33")):
        out = _lib.NlrOut()
        res = {k: torch.full((N * c,), -7.0, device=DEV) for k, c in dict(rgb=3, depth=1, semantic=33, acc=1).items()}
        for k, t in res.items():
            setattr(out, k, t.data_ptr())
        wts = torch.full((N * 513,), -7.0, device=DEV)
        rc = L.nlr_composite_level(_lib.ptr(dens), _lib.ptr(td), _lib.ptr(dirs), _lib.ptr(big), _lib.ptr(big), None, None, None, N, S, K, 1, 1.0,
                                   0, 0.0, _lib.ptr(wts), C.byref(out), None, None)
        torch.cuda.synchronize()
        assert rc != 0 and word in L.nlr_last_error(), (S, K, rc, L.nlr_last_error())
        assert all(bool((t == -7.0).all()) for t in list(res.values()) + [wts])
    for S, word in ((0, b"S=0"), (513, b"S=513")):
        outs = [torch.full((n,), -7.0, device=DEV) for n in (N * 513, 3 * N * 513, N * 513)]
        gz = torch.zeros(N * 513, device=DEV)
        rc = L.nlr_composite_backward(_lib.ptr(dens), _lib.ptr(td), _lib.ptr(dirs), _lib.ptr(big), None, _lib.ptr(big), N, S, 0, 1, 1.0,
                                      _lib.ptr(gz), _lib.ptr(gz), None, _lib.ptr(gz), _lib.ptr(gz), _lib.ptr(gz), _lib.ptr(outs[0]),
                                      _lib.ptr(outs[1]), None, _lib.ptr(outs[2]), None)
        torch.cuda.synchronize()
        assert rc != 0 and word in L.nlr_last_error(), (S, rc, L.nlr_last_error())
        assert all(bool((t == -7.0).all()) for t in outs)


# ---- C. the segment-record route (whole renders whose last level has S_last samples) ---------------------------------------------
def _seg_setup(S_last):
    mc = dataclasses.replace(nconfig.workload("REFI", 12), num_nerf_samples=S_last)
    sd = nweights.synth_state_dict(mc, seed=3, trained_like=True)
    sweep = nlidar.synthetic_sweep(width=10, seed=2, beams=nlidar.LIDAR_ANGLES[::4])      # 80 rays
    idx = np.linspace(0, 79, 33).astype(np.int64)
    return mc, sd, {k: np.ascontiguousarray(v[idx]) for k, v in sweep.items()}


@functools.lru_cache(maxsize=None)
def _seg_oracle(S_last):
    mc, sd, batch = _seg_setup(S_last)
    rend, _ = orc.model_forward(sd, mc, {k: T(v) for k, v in batch.items()})
    ref = {k: v.numpy() for k, v in rend[-1].items()}
    for a in ref.values():
        a.setflags(write=False)
    return ref


def _gate(name, got, ref, mean_tol, max_tol=None, thr=None, frac=0.0):
    """tests/test_mlp_fold.py::_gate."""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).reshape(-1)
    f_ = float(np.mean(d > thr)) if thr is not None else 0.0
    print(f"{name}: mean {d.mean():.3e} max {d.max():.3e}" + (f" fraction > {thr}: {f_:.4f}" if thr is not None else ""))
    assert d.mean() <= mean_tol, f"{name}: mean {d.mean():.3e} (<= {mean_tol})"
    assert f_ <= frac, f"{name}: fraction > {thr}: {f_:.4f} (<= {frac})"
    if max_tol is not None:
        assert d.max() <= max_tol, f"{name}: max {d.max():.3e} (<= {max_tol})"


def _oracle_gates(tag, r, ref):
    """The gates of tests/test_mlp_fold.py::test_render_rays_against_the_oracle, unchanged."""
    _gate(f"{tag} depth", npy(r["depth"]), ref["depth"], 2e-4, 1e-2, thr=1e-3, frac=0.035)
    assert np.percentile(np.abs(npy(r["depth"]) - ref["depth"]), 95) <= 1e-3
    _gate(f"{tag} acc", npy(r["acc"]), ref["acc"], 1e-6, 1e-5)
    _gate(f"{tag} intensity", npy(r["intensity"]), ref["intensity"], 1e-4, 1e-3)
    _gate(f"{tag} semantic", npy(r["semantic"]), ref["semantic"], 1e-4, 1e-2, thr=1e-3, frac=0.01)
    np.testing.assert_array_equal(npy(r["labels"]), ref["semantic"].argmax(-1))
    _gate(f"{tag} rgb", npy(r["rgb"]), ref["rgb"], 2e-3, 2e-2)   # bf16 view MLP


def _route():
    return _lib.lib().nlr_debug_get(_lib.DBG_LAST_ROUTE)


@pytest.mark.gpu
@pytest.mark.parametrize("S_last", [96, 256, 512])
def test_segment_route_at_wide_lane_layouts(S_last):
    """per = 2 with 16 idle lanes (96), per = 4 and 8 (256, 512: a ray spans one or two whole 256-sample MLP tiles): the fused render
    against the ray_history render of the same model and against the oracle."""
    from nerflidar_hip.models import Model
    mc, sd, batch_np = _seg_setup(S_last)
    ref = _seg_oracle(S_last)
    model = Model(mc, sd, device=DEV, precision=_lib.PREC_FAST)
    batch = {k: cu(v) for k, v in batch_np.items()}
    r, _ = model.render_rays(batch, scale_factor=1 / 250)
    torch.cuda.synchronize()
    assert _route() == _lib.ROUTE_FULL_FUSED
    ru, hist = model.render_rays(batch, scale_factor=1 / 250, want_history=True)
    rl, _ = model.render_rays(batch, scale_factor=1 / 250, lidar_only=True)
    torch.cuda.synchronize()
    assert _route() == _lib.ROUTE_LIDAR_FUSED
    _oracle_gates(f"seg S={S_last}", r, ref)

    for k in ("depth", "acc", "distance_median", "points"):
        np.testing.assert_array_equal(npy(r[k]), npy(ru[k]))
    np.testing.assert_array_equal(npy(r["labels"]), npy(ru["labels"]))
    # the history route's own per-sample heads composited in float64: the error each route has against the same exact sums
    h = hist[-1]
    w64 = orc.compute_alpha_weights(h["density"].cpu().double(), h["tdist"].cpu().double(), batch["directions"].cpu().double(), mc.opaque_background)
    exact = orc.volumetric_rendering(h["rgb"].cpu().double(), w64, h["tdist"].cpu().double(), 1.0, batch["far"].cpu().double(), False,
                                     semantic=h["semantic"].cpu().double(), intensity=h["intensity"].cpu().double())
    for k in ("rgb", "semantic", "intensity"):
        d = float(np.abs(npy(r[k]) - npy(ru[k])).max())
        e_f = float(np.abs(npy(r[k]) - exact[k].numpy()).max())
        e_u = float(np.abs(npy(ru[k]) - exact[k].numpy()).max())
        print(f"seg S={S_last} {k}: fused vs history {d:.3e}; against float64 sums of the history heads: fused {e_f:.3e} history {e_u:.3e}")
        np.testing.assert_allclose(npy(r[k]), npy(ru[k]), rtol=0, atol=2e-6)

    assert set(rl) == set(r) - {"rgb"}
    for k in rl:
        assert torch.equal(rl[k], r[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("S_last", [48, 160, 192])
def test_sample_counts_without_a_segment_layout_take_the_unfused_route(S_last):
    """48: S % 32 != 0; 160 and 192: per = 3 and 32 % per != 0.  The per-sample route, at the same oracle gates, bit-equal to its own
    ray_history render in every shared key."""
    from nerflidar_hip.models import Model
    mc, sd, batch_np = _seg_setup(S_last)
    ref = _seg_oracle(S_last)
    model = Model(mc, sd, device=DEV, precision=_lib.PREC_FAST)
    batch = {k: cu(v) for k, v in batch_np.items()}
    r, _ = model.render_rays(batch, scale_factor=1 / 250)
    torch.cuda.synchronize()
    assert _route() == _lib.ROUTE_FULL
    r = {k: v.clone() for k, v in r.items()}
    ru, _ = model.render_rays(batch, scale_factor=1 / 250, want_history=True)
    torch.cuda.synchronize()
    _oracle_gates(f"unfused S={S_last}", r, ref)
    assert set(r) <= set(ru) or set(ru) <= set(r)
    for k in set(r) & set(ru):
        assert torch.equal(r[k], ru[k]), k
