"""The edge-aware smoothness terms of the patch rays (ZI/train.py:365-388): `losses.patch_smoothness` - its torch restatement and the HIP
operator nlr_patch_smooth_forward / _backward (header section 10) - against the reference's edge_aware_loss_v2 /
edge_aware_loss_for_semantic (tests/golden/fn_smooth.npz, make_golden_smooth.py) and against the restatement in float64.

Tolerances are the ones `fn_losses.npz` is held to (test_losses.py, DESIGN "Losses and the step"): values rtol 2e-5, gradients rtol 2e-4
with an absolute floor of 2e-8 + 1e-5 max|gradient| (an element of the gradient is a difference of terms of the size of its largest
elements, a_i - mean_j a_j D_j: its rounding error scales with those, not with itself)."""
import inspect

import numpy as np
import pytest
import torch

from conftest import golden
from nerflidar_hip import losses as nl

NO_X_PAIR = 3  # the fixture case whose mask leaves no two x neighbours valid


def _case(g, ci, dtype=torch.float32, device="cpu"):
    P, s, K = (int(v) for v in g[f"c{ci}_shape"])
    t = lambda k: torch.from_numpy(g[f"c{ci}_{k}"]).to(device=device, dtype=dtype)
    return (P, s, K), t("depth").requires_grad_(True), t("semantic").requires_grad_(True), t("rgb"), t("valid")


def _close(got, want, what):
    """(T_d, T_s, d_depth, d_semantic) against the same four: the tolerances of the module docstring."""
    for name, a, b in zip(("T_d", "T_s"), got[:2], want[:2]):
        np.testing.assert_allclose(float(a), float(b), rtol=2e-5, atol=1e-9, err_msg=f"{what} {name}")
    for name, a, b in zip(("d_depth", "d_semantic"), got[2:], want[2:]):
        if b is None:
            assert a is None, f"{what} {name}"
            continue
        b = np.asarray(b, np.float64)
        np.testing.assert_allclose(np.asarray(a, np.float64), b, rtol=2e-4, atol=2e-8 + 1e-5 * np.abs(b).max(), err_msg=f"{what} {name}")


def _run(depth, sem, rgb, valid, s, backend):
    """(T_d, T_s, d_depth, d_semantic) of T_d + T_s as numpy / floats; depth and sem are leaves."""
    t_d, t_s = nl.patch_smoothness(depth, sem, rgb, valid, s, backend=backend)
    grads = torch.autograd.grad(t_d + t_s, [depth] + ([sem] if sem is not None else []), allow_unused=True)
    np_ = lambda x, like: (torch.zeros_like(like) if x is None else x).detach().cpu().numpy()
    return (float(t_d.detach()), float(t_s.detach()), np_(grads[0], depth), None if sem is None else np_(grads[1], sem))


@pytest.mark.parametrize("ci", [0, 1, 2, 3])
def test_torch_restatement_matches_the_reference_terms(ci):
    g = golden("fn_smooth")
    (P, s, K), depth, sem, rgb, valid = _case(g, ci)
    got = _run(depth, sem, rgb, valid, s, "torch")
    _close(got, (g[f"c{ci}_t_d"], g[f"c{ci}_t_s"], g[f"c{ci}_grad_depth"], g[f"c{ci}_grad_semantic"]), f"case {ci}")
    if ci == NO_X_PAIR:
        assert got[0] == 0.0 and got[1] == 0.0 and not got[2].any() and not got[3].any()
    else:
        assert got[0] > 0 and got[1] > 0 and np.abs(g[f"c{ci}_grad_depth"]).max() > 0 and np.abs(g[f"c{ci}_grad_semantic"]).max() > 0


def test_total_loss_with_default_arguments_returns_the_keys_it_did():
    """No patch arguments: the dictionary has the keys it had before the smoothness terms existed, whatever the batch carries; the
    new keys appear with patch_size > 1 and patch_rays only, `s_smo` only with a semantic rendering."""
    n, S, K, s = 32, 6, 4, 4
    gen = torch.Generator().manual_seed(0)
    r = lambda *sh: torch.rand(*sh, generator=gen)
    sd = torch.sort(r(n, S + 1), -1).values
    w = r(n, S) / S
    rend = [dict(rgb=r(n, 3)), dict(rgb=r(n, 3), depth=r(n) + 0.5, semantic=torch.softmax(r(n, K), -1), intensity=r(n))]
    hist = [dict(sdist=sd, weights=w), dict(sdist=sd, weights=w)]
    batch = dict(rgb=r(n, 3), depth=r(n), semantic=torch.randint(0, K, (n,), generator=gen).float(), intensity=r(n), mask=torch.ones(n),
                 patch_mask=torch.zeros(n), lidar_mask=torch.zeros(n))
    batch.update(nl.nusc_masks(batch))
    before = {"data", "depth", "sem", "int", "interlevel", "distortion"}
    assert set(nl.total_loss(rend, hist, batch)) == before
    assert set(nl.total_loss(rend, hist, batch, patch_size=s)) == before            # no patch_rays
    assert set(nl.total_loss(rend, hist, batch, patch_rays=(0, 2))) == before        # patch_size = 0
    with_patches = nl.total_loss(rend, hist, batch, patch_size=s, patch_rays=(0, 2))
    assert set(with_patches) == before | {"d_smo", "s_smo"}
    t_d, t_s = nl.patch_smoothness(rend[-1]["depth"][:32], rend[-1]["semantic"][:32], batch["rgb"][:32], batch["patch_valid"][:32], s)
    assert float(with_patches["d_smo"]) == float(0.01 * t_d) > 0 and float(with_patches["s_smo"]) == float(0.01 * t_s) > 0
    no_sem = [rend[0], {k: v for k, v in rend[1].items() if k != "semantic"}]
    assert set(nl.total_loss(no_sem, hist, batch, patch_size=s, patch_rays=(0, 2))) == (before - {"sem"}) | {"d_smo"}
    sig = inspect.signature(nl.total_loss).parameters
    assert (sig["patch_size"].default, sig["patch_rays"].default, sig["smo_lam"].default, sig["s_lam"].default) == (0, None, 0.01, 0.01)


# ---- the HIP operator -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ci", [0, 1, 2, 3])
def test_kernel_matches_the_reference_terms(ci):
    g = golden("fn_smooth")
    (P, s, K), depth, sem, rgb, valid = _case(g, ci, device="cuda")
    got = _run(depth, sem, rgb, valid, s, "hip")
    _close(got, (g[f"c{ci}_t_d"], g[f"c{ci}_t_s"], g[f"c{ci}_grad_depth"], g[f"c{ci}_grad_semantic"]), f"case {ci}")
    if ci == NO_X_PAIR:
        assert got[0] == 0.0 and got[1] == 0.0 and not got[2].any() and not got[3].any()


def _inputs(P, s, K, seed, device="cuda"):
    gen = torch.Generator().manual_seed(seed)
    n = P * s * s
    depth = (0.2 + 1.6 * torch.rand(n, generator=gen)).to(device)
    sem = torch.softmax(4 * torch.rand(n, K, generator=gen) - 2, -1) if K > 1 else 0.1 + 0.9 * torch.rand(n, K, generator=gen)
    rgb = torch.rand(n, 3, generator=gen).to(device)
    valid = (torch.rand(n, generator=gen) > 0.3).float().to(device)
    return depth, sem.to(device), rgb, valid


_F64 = {}


def _float64(shape, mode):
    """The float64 restatement on the float32 inputs of a shape and mode: computed once, shared."""
    if (shape, mode) not in _F64:
        depth, sem, rgb, valid = (t.cpu().double() for t in _inputs(*shape, seed=7))
        _F64[shape, mode] = _run(depth.requires_grad_(True), None if mode == "no_semantic" else sem.requires_grad_(True), rgb,
                                 valid if mode == "invalid30" else None, shape[1], "torch")
    return _F64[shape, mode]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["all_valid", "invalid30", "no_semantic"])
@pytest.mark.parametrize("shape", [(1, 2, 1), (2, 3, 4), (2, 5, 1), (3, 32, 19), (1, 64, 32)])
def test_kernel_matches_the_float64_restatement(shape, mode):
    """Sizes: the smallest patch, odd sizes below one pass of the 256 threads, one class / one slice of classes / several slices incl. a
    partial one (19 + depth = 5 slices of 4), more than one patch, the shipped shape and the largest patch and class count."""
    depth, sem, rgb, valid = _inputs(*shape, seed=7)
    got = _run(depth.requires_grad_(True), None if mode == "no_semantic" else sem.requires_grad_(True), rgb,
               valid if mode == "invalid30" else None, shape[1], "hip")
    want = _float64(shape, mode)
    print(f"{shape} {mode}: T_d {got[0]:.7g} / {want[0]:.7g}  T_s {got[1]:.7g} / {want[1]:.7g}  max |d_depth err| "
          f"{np.abs(got[2] - want[2]).max():.3g} of {np.abs(want[2]).max():.3g}")
    _close(got, want, f"{shape} {mode}")
    assert want[0] > 0 and (want[1] > 0) == (mode != "no_semantic")


@pytest.mark.gpu
def test_degenerate_inputs_give_exact_zeros():
    P, s, K = 2, 6, 3
    depth, sem, rgb, valid = _inputs(P, s, K, seed=11)
    # constant depth: every difference of the normalised depth is 0, sign(0) = 0
    const = torch.full_like(depth, 0.73).requires_grad_(True)
    t_d, t_s, d_depth, d_sem = _run(const, sem.requires_grad_(True), rgb, valid, s, "hip")
    assert t_d == 0.0 and not d_depth.any() and t_s > 0 and d_sem.any()
    # no valid pixel; one valid column (y pairs only)
    column = torch.zeros(P, s, s, device="cuda")
    column[:, :, 2] = 1
    for v in (torch.zeros_like(valid), column.reshape(-1)):
        got = _run(depth.detach().requires_grad_(True), sem.detach().requires_grad_(True), rgb, v, s, "hip")
        assert got[0] == 0.0 and got[1] == 0.0 and not got[2].any() and not got[3].any()


@pytest.mark.gpu
def test_two_runs_give_identical_bits_and_depth_does_not_depend_on_the_semantic_input():
    P, s, K = 3, 32, 19
    depth, sem, rgb, valid = _inputs(P, s, K, seed=13)
    runs = [_run(depth.detach().requires_grad_(True), sem.detach().requires_grad_(True), rgb, valid, s, "hip") for _ in range(2)]
    bits = lambda x: np.asarray(x, np.float32).view(np.uint32)
    for a, b in zip(*runs):
        assert np.array_equal(bits(a), bits(b))
    alone = _run(depth.detach().requires_grad_(True), None, rgb, valid, s, "hip")
    assert np.array_equal(bits(alone[0]), bits(runs[0][0])) and np.array_equal(bits(alone[2]), bits(runs[0][2])) and alone[1] == 0.0


@pytest.mark.gpu
def test_refusals_return_invalid_and_launch_nothing():
    """Every refusal of header section 10: NLR_ERR_INVALID (-1), a message naming the argument, canary-filled outputs untouched."""
    from nerflidar_hip import _lib
    P, s, K = 2, 4, 3
    depth, sem, rgb, valid = _inputs(P, s, K, seed=17)
    L = _lib.lib()
    need = int(L.nlr_patch_smooth_workspace_bytes(P, K))
    assert need > 0 and int(L.nlr_patch_smooth_workspace_bytes(P, 32)) > need
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    canary = lambda *sh: torch.full(sh, -7.5, device="cuda")
    terms, stats, g_terms, d_depth, d_sem = canary(2), canary(8), torch.ones(2, device="cuda"), canary(P * s * s), canary(P * s * s, K)
    fwd = dict(depth=depth, semantic=sem, rgb=rgb, valid=valid, P=P, s=s, K=K, terms=terms, stats=stats, workspace=ws, workspace_bytes=need)
    bwd = dict(depth=depth, semantic=sem, rgb=rgb, valid=valid, P=P, s=s, K=K, stats=torch.zeros(8, device="cuda"), g_terms=g_terms,
               d_depth=d_depth, d_semantic=d_sem, workspace=ws, workspace_bytes=need)
    bad = [("s", 1), ("s", 65), ("K", 0), ("K", 33), ("P", 0), ("depth", None), ("rgb", None), ("workspace", None), ("workspace_bytes", need - 1)]
    cases = [("nlr_patch_smooth_forward", fwd, bad + [("terms", None), ("stats", None)]),
             ("nlr_patch_smooth_backward", bwd, bad + [("stats", None), ("g_terms", None), ("d_depth", None), ("d_semantic", None)])]
    for fn, good, bads in cases:
        names = [p.name for p in _lib.signatures()[fn].params[:-1]]
        assert names == list(good), (names, list(good))
        for key, value in bads:
            args = [value if k == key else v for k, v in good.items()]
            with pytest.raises(RuntimeError) as e:
                _lib.call(fn, *args)
            word = {"s": "s =", "K": "K =", "P": "P ="}.get(key, key)
            assert "(-1)" in str(e.value) and word in str(e.value), (fn, key, str(e.value))
    torch.cuda.synchronize()
    for t in (terms, stats, d_depth, d_sem):
        assert bool((t == -7.5).all())
    assert bool((ws == 0x5A).all())
