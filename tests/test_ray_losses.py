"""The two losses that read the ray history as one HIP operator (header section 11, csrc/nlr_ray_losses.hip, `training.ray_losses`,
`losses.ray_history_terms`, `total_loss(ray_loss_backend=)`): the anti-aliased interlevel term of every proposal level and the distortion
term of the final level, values and gradients with respect to the weights - against the reference's own values (tests/golden/
fn_losses.npz), against the torch restatement of `losses.py` in float64 on the same float32 inputs, and inside the whole step.

Tolerances (the ones `fn_losses.npz` is held to, test_losses._check): gradients rtol 2e-4 with an absolute floor of 2e-8 + 1e-5 max|g|;
values rtol 2e-5 against the fixture and 5e-5 against float64 (the float32 torch restatement itself is off by up to 9.6e-6 there, a
kernel with another summation order gets 5x that).  w_target, what the forward hands the backward, is compared elementwise against
float64 relative to max|w_target| of the case, at 4x the error of the float32 torch restatement on the same inputs (measured on the
CPU, `W_TARGET_F32_ERR` below)."""
import inspect

import numpy as np
import pytest
import torch

from conftest import golden
from nerflidar_hip import _lib
from nerflidar_hip import losses as nl

PULSE = (0.03, 0.003, 0.03, 0.003)  # the shipped widths, repeated for levels 3 and 4
# (N, S, proposal S): smallest; tiny with two levels; just over half a wave of knots, odd; both sides of the 64-lane boundary; the REF shape
# with more rays than one workgroup holds; the C2 shape; the limits; no proposal level; four levels
SHAPES = [(1, 1, (1,)), (3, 2, (3, 2)), (5, 33, (64,)), (7, 65, (63, 64)), (70, 32, (64, 64)), (2, 128, (64, 64)), (2, 512, (512,)), (3, 32, ()),
          (3, 16, (8, 8, 8, 8))]
# max |w_target(float32 torch restatement) - w_target(float64)| / max |w_target(float64)| over the levels of a shape, measured on the CPU
# with the inputs of `_inputs(shape)`; the kernel's gate is 4x this
W_TARGET_F32_ERR = {(1, 1, (1,)): 1.11e-07, (3, 2, (3, 2)): 4.54e-06, (5, 33, (64,)): 1.99e-06, (7, 65, (63, 64)): 7.65e-06,
                    (70, 32, (64, 64)): 6.03e-06, (2, 128, (64, 64)): 6.71e-06, (2, 512, (512,)): 6.05e-06, (3, 32, ()): 0.0,
                    (3, 16, (8, 8, 8, 8)): 7.91e-06}


def _inputs(shape, seed=7):
    """The history of a shape as CPU float32 dicts, proposal levels first: sdist = sort(rand) with its ends at 0 and 1, weights = rand
    normalised per ray to a sum drawn from [0.5, 1], obj_mask = rand < 0.3 with element [0, 0] unmasked."""
    N, S, props = shape
    gen = torch.Generator().manual_seed(seed)
    hist = []
    for n in list(props) + [S]:
        sd = torch.sort(torch.rand(N, n + 1, generator=gen), -1).values
        sd[:, 0], sd[:, -1] = 0.0, 1.0
        w = torch.rand(N, n, generator=gen)
        w = w / w.sum(-1, keepdim=True) * (0.5 + 0.5 * torch.rand(N, 1, generator=gen))
        m = torch.rand(N, n, generator=gen) < 0.3
        m[0, 0] = False
        hist.append(dict(sdist=sd, weights=w, obj_mask=m))
    del hist[-1]["obj_mask"]
    return hist


def _to(hist, device="cpu", dtype=torch.float32, masks=True):
    """A copy of a history on `device` in `dtype`, its weights leaves that require a gradient."""
    out = []
    for h in hist:
        d = dict(sdist=h["sdist"].to(device=device, dtype=dtype), weights=h["weights"].detach().to(device=device, dtype=dtype).requires_grad_(True))
        if masks and "obj_mask" in h:
            d["obj_mask"] = h["obj_mask"].to(device)
        out.append(d)
    return out


def _run(hist, backend, pulse=PULSE):
    """(anti terms [n_prop], distortion, gradient of (sum of the anti terms + distortion) per level) as float64 numpy."""
    anti, dist = nl.ray_history_terms(hist, pulse, backend=backend)
    anti = torch.stack(list(anti)) if len(anti) else torch.zeros(0, dtype=dist.dtype, device=dist.device)
    grads = torch.autograd.grad(anti.sum() + dist, [h["weights"] for h in hist], allow_unused=True)
    grads = [(torch.zeros_like(h["weights"]) if g is None else g).detach().cpu().double().numpy() for g, h in zip(grads, hist)]
    return anti.detach().cpu().double().numpy(), float(dist.detach()), grads


def _w_target_torch(hist, pulse=PULSE):
    """w_target of every proposal level as `losses.anti_interlevel_terms` builds it, in the dtype of the history."""
    c, w = hist[-1]["sdist"], hist[-1]["weights"].detach()
    pdf = (w / (c[..., 1:] - c[..., :-1])).clamp_max(10)
    out = []
    for i, h in enumerate(hist[:-1]):
        knots, val = nl.blur_stepfun(c, pdf, pulse[i])
        area = 0.5 * (val[..., 1:] + val[..., :-1]) * torch.diff(knots, dim=-1)
        cdf = torch.cat([torch.zeros_like(area[..., :1]), torch.cumsum(area, dim=-1)], dim=-1)
        out.append(torch.diff(nl._quad_cdf_at(h["sdist"], knots, val, cdf), dim=-1).cpu().double().numpy())
    return out


def _close(got, want, what, value_rtol):
    """(anti, dist, grads) against the same: values to `value_rtol`, gradients to the tolerance of test_losses._check; returns the
    largest value error and the largest gradient error as a share of its tolerance."""
    worst_v, worst_g = 0.0, 0.0
    for name, a, b in [(f"anti term {i}", a, b) for i, (a, b) in enumerate(zip(got[0], want[0]))] + [("distortion", got[1], want[1])]:
        np.testing.assert_allclose(a, b, rtol=value_rtol, atol=1e-9, err_msg=f"{what} {name}")
        worst_v = max(worst_v, abs(a - b) / max(abs(b), 1e-30))
    for li, (a, b) in enumerate(zip(got[2], want[2])):
        tol = 2e-8 + 1e-5 * np.abs(b).max() + 2e-4 * np.abs(b)
        worst_g = max(worst_g, float((np.abs(a - b) / tol).max()))
        np.testing.assert_allclose(a, b, rtol=2e-4, atol=2e-8 + 1e-5 * np.abs(b).max(), err_msg=f"{what} gradient of level {li}")
    return worst_v, worst_g


def _fixture_history(g, masked, device="cpu"):
    hist = []
    for li in range(3):
        hist.append(dict(sdist=torch.from_numpy(g[f"sdist{li}"]).to(device), weights=torch.from_numpy(g[f"weights{li}"]).to(device).requires_grad_(True)))
        if masked and li < 2:
            hist[-1]["obj_mask"] = torch.from_numpy(g[f"obj_mask{li}"]).to(device)
    return hist


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------------
def test_the_three_functions_are_declared_and_exported():
    names = ["nlr_ray_losses_workspace_bytes", "nlr_ray_losses_forward", "nlr_ray_losses_backward"]
    sigs = _lib.signatures()
    assert all(n in sigs for n in names) and all(hasattr(_lib.lib(), n) for n in names)
    assert sigs["nlr_ray_losses_forward"].launcher and sigs["nlr_ray_losses_backward"].launcher and not sigs[names[0]].launcher
    kinds = {p.name: p.kind for p in sigs["nlr_ray_losses_forward"].params}
    assert (kinds["prop_sdist"], kinds["prop_obj_mask"], kinds["w_target"], kinds["prop_S_host"], kinds["pulse_width_host"]) == \
        ("handles", "handles", "handles", "host", "host")
    assert (_lib.DEFINES["NLR_RAY_LOSSES_MAX_PROP"], _lib.DEFINES["NLR_RAY_LOSSES_MAX_S"]) == (4, 512)
    L = _lib.lib()
    assert int(L.nlr_ray_losses_workspace_bytes(1, 0)) > 0
    assert int(L.nlr_ray_losses_workspace_bytes(65536, 2)) > int(L.nlr_ray_losses_workspace_bytes(65536, 1)) > int(L.nlr_ray_losses_workspace_bytes(16, 1))


@pytest.mark.parametrize("masked", [False, True])
def test_torch_backend_is_the_existing_functions_bit_for_bit(masked):
    g = golden("fn_losses")
    pw = g["pulse_width"].tolist()
    hist = _fixture_history(g, masked)
    anti, dist = nl.ray_history_terms(hist, pw, backend="torch")
    assert len(anti) == 2 and all(t.dim() == 0 for t in anti)
    bits = lambda t: t.detach().numpy().view(np.uint32)
    for mult in (1.0, float(g["anti_mult"])):
        old = nl.anti_interlevel_loss(hist, mult, pw)
        assert np.array_equal(bits(mult * (0.0 + anti[0] + anti[1])), bits(old))
        old_d = nl.distortion_loss(hist, mult)
        assert np.array_equal(bits(mult * dist), bits(old_d))
    # "auto" on CPU tensors is "torch"
    anti2, dist2 = nl.ray_history_terms(hist, pw)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(anti, anti2)) and np.array_equal(bits(dist), bits(dist2))
    # and the gradients of the old entry point are the fixture's, as before
    grads = torch.autograd.grad(nl.anti_interlevel_loss(hist, float(g["anti_mult"]), pw), [hist[0]["weights"], hist[1]["weights"]])
    tag = "anti_masked" if masked else "anti"
    for li, gr in enumerate(grads):
        want = g[f"{tag}_g{li}"]
        np.testing.assert_allclose(gr.numpy(), want, rtol=2e-4, atol=2e-8 + 1e-5 * np.abs(want).max())


def _step_inputs(n=32, S=6, K=4):
    gen = torch.Generator().manual_seed(0)
    r = lambda *sh: torch.rand(*sh, generator=gen)
    sd = [torch.sort(r(n, s + 1), -1).values for s in (S + 2, S)]
    rend = [dict(rgb=r(n, 3)), dict(rgb=r(n, 3), depth=r(n) + 0.5, semantic=torch.softmax(r(n, K), -1), intensity=r(n))]
    hist = [dict(sdist=sd[0], weights=r(n, S + 2) / S), dict(sdist=sd[1], weights=r(n, S) / S)]
    batch = dict(rgb=r(n, 3), depth=r(n), semantic=torch.randint(0, K, (n,), generator=gen).float(), intensity=r(n), mask=torch.ones(n),
                 patch_mask=torch.zeros(n), lidar_mask=torch.zeros(n))
    batch.update(nl.nusc_masks(batch))
    return rend, hist, batch


def test_total_loss_with_default_arguments_is_what_it_was():
    """Same keys, and `interlevel` / `distortion` with the bits of the functions `total_loss` called before the argument existed."""
    rend, hist, batch = _step_inputs()
    assert inspect.signature(nl.total_loss).parameters["ray_loss_backend"].default == "torch"
    bits = lambda t: t.detach().numpy().view(np.uint32)
    for kw in (dict(), dict(interlevel_mult=0.5, anti_interlevel_mult=0.0), dict(distortion_mult=0.0), dict(ray_loss_backend="torch"),
               dict(ray_loss_backend="auto")):          # ("auto" on CPU tensors is the torch path)
        out = nl.total_loss(rend, hist, batch, **kw)
        want = {"data", "depth", "sem", "int", "interlevel", "distortion"} - ({"distortion"} if kw.get("distortion_mult") == 0.0 else set())
        assert set(out) == want, kw
        inter = nl.interlevel_loss(hist, 0.5) if "interlevel_mult" in kw else nl.anti_interlevel_loss(hist, 0.01, (0.03, 0.003))
        assert np.array_equal(bits(out["interlevel"]), bits(inter)), kw
        if "distortion" in out:
            assert np.array_equal(bits(out["distortion"]), bits(nl.distortion_loss(hist, 0.005))), kw
    with pytest.raises(ValueError, match="ray_loss_backend"):
        nl.total_loss(rend, hist, batch, ray_loss_backend="cuda")


def test_hip_backend_refuses_cpu_tensors_and_an_sdist_that_requires_grad():
    rend, hist, batch = _step_inputs()
    with pytest.raises(ValueError, match="float32 CUDA tensors"):
        nl.total_loss(rend, hist, batch, ray_loss_backend="hip")
    with pytest.raises(ValueError, match="float32 CUDA tensors"):
        nl.ray_history_terms(hist, PULSE, backend="hip")
    with pytest.raises(ValueError, match="backend"):
        nl.ray_history_terms(hist, PULSE, backend="triton")
    from nerflidar_hip import training as ntrain
    hist[0]["sdist"] = hist[0]["sdist"].clone().requires_grad_(True)
    with pytest.raises(ValueError, match="sdist"):
        ntrain.ray_losses(hist, PULSE)


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
def test_operator_matches_the_reference_values_and_gradients(masked):
    """fn_losses.npz: 48 rays, S = 64 / 64 / 32, one zero-width bin with w > 0 per level; `interlevel` and `distortion` as the reference
    scales them, under the tolerances of test_losses._check."""
    g = golden("fn_losses")
    hist = _fixture_history(g, masked, "cuda")
    anti, dist = nl.ray_history_terms(hist, g["pulse_width"].tolist(), backend="hip")
    assert isinstance(anti, torch.Tensor) and anti.shape == (2,) and anti.is_cuda and dist.dim() == 0
    inter, dl = float(g["anti_mult"]) * anti.sum(), float(g["dist_mult"]) * dist
    tag = "anti_masked" if masked else "anti"
    print(f"interlevel {float(inter.detach()):.8g} reference {float(g[tag + '_loss']):.8g}   distortion {float(dl.detach()):.8g} reference {float(g['dist_loss']):.8g}")
    np.testing.assert_allclose(float(inter.detach()), float(g[f"{tag}_loss"]), rtol=2e-5, atol=1e-9)
    np.testing.assert_allclose(float(dl.detach()), float(g["dist_loss"]), rtol=2e-5, atol=1e-9)
    grads = torch.autograd.grad(inter + dl, [h["weights"] for h in hist])
    for li, (gr, key) in enumerate(zip(grads, (f"{tag}_g0", f"{tag}_g1", "dist_g2"))):
        want = g[key]
        tol = 2e-8 + 1e-5 * np.abs(want).max() + 2e-4 * np.abs(want)
        print(f"level {li}: largest gradient error {float((np.abs(gr.cpu().numpy() - want) / tol).max()):.3f} of its tolerance")
        np.testing.assert_allclose(gr.cpu().numpy(), want, rtol=2e-4, atol=2e-8 + 1e-5 * np.abs(want).max(), err_msg=f"{tag} level {li}")


_F64 = {}


def _float64(shape, masked):
    """The float64 restatement on the float32 inputs of a shape: computed once, shared."""
    if (shape, masked) not in _F64:
        _F64[shape, masked] = _run(_to(_inputs(shape), dtype=torch.float64, masks=masked), "torch")
    if shape not in _F64:
        _F64[shape] = _w_target_torch(_to(_inputs(shape), dtype=torch.float64))
    return _F64[shape, masked], _F64[shape]


def _forward_raw(hist, pulse=PULSE):
    """nlr_ray_losses_forward through `_lib.call` on a CUDA history: (terms, stats, w_target list)."""
    from nerflidar_hip.training import _RayLosses, _ptr_array
    sd, w = hist[-1]["sdist"].contiguous(), hist[-1]["weights"].detach().contiguous()
    psd = [h["sdist"].contiguous() for h in hist[:-1]]
    pw = [h["weights"].detach().contiguous() for h in hist[:-1]]
    pm = [h["obj_mask"].contiguous().view(torch.uint8) if "obj_mask" in h else None for h in hist[:-1]]
    n_prop = len(pw)
    terms, stats = torch.empty(1 + n_prop, device="cuda"), torch.empty(2 * (1 + n_prop), device="cuda")
    w_target = [torch.empty_like(p) for p in pw]
    ws = torch.empty(int(_lib.lib().nlr_ray_losses_workspace_bytes(w.shape[0], n_prop)), dtype=torch.uint8, device="cuda")
    _lib.call("nlr_ray_losses_forward", *_RayLosses._args(sd, w, psd, pw, pm, pulse), terms, stats, _ptr_array(w_target) if n_prop else None, ws,
              ws.numel())
    return terms, stats, w_target


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{s}-{'_'.join(map(str, p)) or 'none'}" for n, s, p in SHAPES])
def test_operator_matches_the_float64_restatement(shape, masked):
    """Values to 5e-5, gradients to the tolerance of test_losses._check, w_target to 4x the float32 torch restatement's own error
    (`W_TARGET_F32_ERR`, relative to max |w_target| of the shape: 1.1e-7 at (1, 1, (1,)), 2.0e-6 .. 7.9e-6 at the other shapes, so gates of
    4.4e-7 and 8.0e-6 .. 3.2e-5).  Measured on the MI355X: values within 8.0e-6, gradients within 0.19 of their tolerance (worst:
    (2, 512, (512,))), w_target errors equal to the float32 torch restatement's at every shape (the scans carry float64 sums, as torch's
    CPU cumsum does; with float32 sums one gradient element of (7, 65, (63, 64)) was at 1.27 of its tolerance)."""
    cpu = _inputs(shape)
    want, want_wt = _float64(shape, masked)
    hist = _to(cpu, "cuda", masks=masked)
    got = _run(hist, "hip")
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]) and want[1] > 0 and (shape[1] == 1 or (want[0] > 0).all())
    worst_v, worst_g = _close(got, want, f"{shape} masked={masked}", 5e-5)
    terms, stats, w_target = _forward_raw(hist)
    counts = stats[1 + len(shape[2]):].cpu().numpy()
    assert counts[0] == shape[0] and all(c == (int((~h["obj_mask"]).sum()) if masked else h["weights"].numel()) for c, h in zip(counts[1:], cpu))
    wt_err = 0.0
    for got_wt, ref in zip(w_target, want_wt):
        wt_err = max(wt_err, float(np.abs(got_wt.cpu().double().numpy() - ref).max() / np.abs(ref).max()))
    print(f"{shape} masked={masked}: value error {worst_v:.3g} (gate 5e-5), gradient error {worst_g:.3f} of its tolerance, "
          f"w_target error {wt_err:.3g} (gate {4 * W_TARGET_F32_ERR[shape]:.3g})")
    assert wt_err <= 4 * W_TARGET_F32_ERR[shape]


def _degenerate(edit, shape=(6, 32, (64, 16)), masked=True):
    """The history of `shape` after `edit(hist)` (CPU float32 dicts, edited in place): (operator result, float32 torch restatement)."""
    cpu = _inputs(shape, seed=11)
    edit(cpu)
    return _run(_to(cpu, "cuda", masks=masked), "hip"), _run(_to(cpu, masks=masked), "torch"), cpu


@pytest.mark.gpu
def test_a_level_without_kept_samples_is_nan_with_a_zero_gradient():
    def edit(h):
        h[1]["obj_mask"][:] = True
    got, want, _ = _degenerate(edit)
    assert np.isnan(got[0][1]) and np.isnan(want[0][1]) and not got[2][1].any() and not want[2][1].any()
    assert np.isfinite(got[0][0]) and np.isfinite(got[1]) and got[2][0].any() and got[2][2].any()
    got[0][1] = want[0][1] = 0.0
    _close(got, want, "level 1 all masked", 5e-5)


@pytest.mark.gpu
def test_zero_width_final_bins():
    # w > 0: the pdf is clamped to 10, everything finite
    def edit(h):
        h[2]["sdist"][1, 8] = h[2]["sdist"][1, 7]
        h[2]["sdist"][4, 1] = h[2]["sdist"][4, 0]
    got, want, _ = _degenerate(edit)
    assert np.isfinite(got[0]).all() and all(np.isfinite(g).all() for g in got[2])
    _close(got, want, "zero-width bin with w > 0", 5e-5)

    # w = 0: 0 / 0 poisons that ray, and nothing else
    # (without masks: on torch a masked sample of that ray gets 0 * NaN = NaN, the operator writes the 0 the header promises)
    def edit0(h):
        edit(h)
        h[2]["weights"][1, 7] = 0.0
    got, want, _ = _degenerate(edit0, masked=False)
    assert np.isnan(got[0]).all() and np.isnan(want[0]).all() and np.isfinite(got[1])
    for li in (0, 1):
        assert np.isnan(got[2][li][1]).all() and np.isnan(want[2][li][1]).all()
        rest = np.delete(np.arange(6), 1)
        assert np.isfinite(got[2][li][rest]).all()
        np.testing.assert_allclose(got[2][li][rest], want[2][li][rest], rtol=2e-4, atol=2e-8 + 1e-5 * np.abs(want[2][li][rest]).max())
    np.testing.assert_allclose(got[1], want[1], rtol=5e-5)
    np.testing.assert_allclose(got[2][2], want[2][2], rtol=2e-4, atol=2e-8 + 1e-5 * np.abs(want[2][2]).max())


@pytest.mark.gpu
def test_queries_on_knots_and_duplicate_queries():
    r = [np.float32(p) for p in PULSE]

    def edit(h):
        c = h[2]["sdist"]
        for ray, j, k, sign in ((0, 5, 9, -1), (2, 40, 20, 1), (3, 1, 2, -1)):  # cp[j] = c[k] -+ float32(r): exactly on a knot
            h[0]["sdist"][ray, j] = float(np.float32(c[ray, k]) + np.float32(sign) * r[0])
        h[1]["sdist"][5, 3] = float(np.float32(c[5, 12]) - r[1])
        h[1]["sdist"][4, 7] = h[1]["sdist"][4, 6]                                # duplicates
        h[0]["sdist"][1, 30:33] = h[0]["sdist"][1, 30]
        for lvl in (0, 1):
            h[lvl]["sdist"].copy_(torch.sort(h[lvl]["sdist"].clamp(0, 1), -1).values)
    got, want, cpu = _degenerate(edit)
    assert float(cpu[0]["sdist"][0].eq(np.float32(cpu[2]["sdist"][0, 9]) - r[0]).sum()) == 1       # the planted query survived the sort
    assert np.isfinite(got[0]).all()
    _close(got, want, "queries on knots, duplicate queries", 5e-5)


@pytest.mark.gpu
def test_two_runs_give_identical_bits_and_distortion_does_not_depend_on_the_proposal_levels():
    cpu = _inputs((70, 32, (64, 64)), seed=13)
    runs = [_run(_to(cpu, "cuda"), "hip") for _ in range(2)]
    flat = lambda r: np.concatenate([np.asarray(r[0], np.float32), np.asarray([r[1]], np.float32)] + [g.astype(np.float32).ravel() for g in r[2]])
    assert np.array_equal(flat(runs[0]).view(np.uint32), flat(runs[1]).view(np.uint32))
    alone = _run(_to(cpu[-1:], "cuda"), "hip")
    assert alone[0].size == 0 and np.float32(alone[1]).view(np.uint32) == np.float32(runs[0][1]).view(np.uint32)
    assert np.array_equal(alone[2][0].astype(np.float32).view(np.uint32), runs[0][2][2].astype(np.float32).view(np.uint32))


@pytest.mark.gpu
def test_refusals_return_invalid_and_launch_nothing():
    """Every refusal of header section 11: NLR_ERR_INVALID (-1), a message naming the argument, canary-filled outputs and workspace
    untouched."""
    from nerflidar_hip.training import _ptr_array
    import ctypes as C
    N, S, props = 5, 8, (6, 4)
    hist = _to(_inputs((N, S, props)), "cuda")
    need = int(_lib.lib().nlr_ray_losses_workspace_bytes(N, 2))
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    canary = lambda *sh: torch.full(sh, -7.5, device="cuda")
    terms, stats, d_w = canary(3), canary(6), canary(N, S)
    w_target, d_pw = [canary(N, s) for s in props], [canary(N, s) for s in props]
    psd, pw = [h["sdist"] for h in hist[:2]], [h["weights"].detach() for h in hist[:2]]
    masks = [h["obj_mask"].view(torch.uint8) for h in hist[:2]]
    arr = lambda ts: (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
    common = dict(sdist=hist[2]["sdist"], weights=hist[2]["weights"].detach(), N=N, S=S, prop_sdist=_ptr_array(psd), prop_weights=_ptr_array(pw),
                  prop_obj_mask=arr(masks), prop_S_host=np.asarray(props, np.int32), pulse_width_host=np.asarray(PULSE[:2], np.float32), n_prop=2)
    fwd = dict(common, terms=terms, stats=stats, w_target=_ptr_array(w_target), workspace=ws, workspace_bytes=need)
    bwd = dict(common, stats=torch.ones(6, device="cuda"), g_terms=torch.ones(3, device="cuda"), w_target=_ptr_array(w_target), d_weights=d_w,
               d_prop_weights=_ptr_array(d_pw), workspace=ws, workspace_bytes=need)
    f32 = lambda *v: np.asarray(v, np.float32)
    bad = [("sdist", None, "sdist"), ("weights", None, "weights"), ("N", 0, "N ="), ("S", 0, "S ="), ("S", 513, "S ="), ("n_prop", 5, "n_prop ="),
           ("prop_sdist", None, "prop_sdist"), ("prop_weights", None, "prop_weights"), ("prop_S_host", None, "prop_S_host"),
           ("pulse_width_host", None, "pulse_width_host"), ("prop_sdist", arr([psd[0], None]), "prop_sdist[1]"),
           ("prop_weights", arr([None, pw[1]]), "prop_weights[0]"), ("prop_S_host", np.asarray([6, 0], np.int32), "prop_S_host[1]"),
           ("prop_S_host", np.asarray([513, 4], np.int32), "prop_S_host[0]"), ("pulse_width_host", f32(0.03, 0.0), "pulse_width_host[1]"),
           ("pulse_width_host", f32(-0.03, 0.003), "pulse_width_host[0]"), ("pulse_width_host", f32(np.inf, 0.003), "pulse_width_host[0]"),
           ("pulse_width_host", f32(0.03, np.nan), "pulse_width_host[1]"), ("workspace", None, "workspace"),
           ("workspace_bytes", need - 1, "workspace_bytes"), ("w_target", None, "w_target"), ("w_target", arr([w_target[0], None]), "w_target[1]"),
           ("stats", None, "stats")]
    cases = [("nlr_ray_losses_forward", fwd, bad + [("terms", None, "terms")]),
             ("nlr_ray_losses_backward", bwd, bad + [("g_terms", None, "g_terms"), ("d_weights", None, "d_weights"),
                                                     ("d_prop_weights", None, "d_prop_weights"), ("d_prop_weights", arr([None, d_pw[1]]), "d_prop_weights[0]")])]
    for fn, good, bads in cases:
        names = [p.name for p in _lib.signatures()[fn].params[:-1]]
        assert names == list(good), (names, list(good))
        for key, value, word in bads:
            args = [value if k == key else v for k, v in good.items()]
            with pytest.raises(RuntimeError) as e:
                _lib.call(fn, *args)
            assert "(-1)" in str(e.value) and word in str(e.value), (fn, key, str(e.value))
    torch.cuda.synchronize()
    for t in [terms, stats, d_w] + w_target + d_pw:
        assert bool((t == -7.5).all())
    assert bool((ws == 0x5A).all())
    # and the same arguments unharmed launch: the masks array and its entries may be NULL, n_prop = 0 takes NULL arrays
    _lib.call("nlr_ray_losses_forward", *fwd.values())
    _lib.call("nlr_ray_losses_forward", *dict(fwd, prop_obj_mask=None).values())
    _lib.call("nlr_ray_losses_forward", *dict(fwd, prop_obj_mask=arr([None, masks[1]])).values())
    none = dict(fwd, prop_sdist=None, prop_weights=None, prop_obj_mask=None, prop_S_host=None, pulse_width_host=None, n_prop=0, w_target=None)
    _lib.call("nlr_ray_losses_forward", *none.values())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(terms[:1]).all())


# ---- the step -----------------------------------------------------------------------------------------------------------------------------
def _gradient_report(tm, g, skip=()):
    named = dict(tm.named_parameters())
    report = []
    for k in [k[5:] for k in g if k.startswith("grad_") and k not in skip]:
        want = torch.from_numpy(g["grad_" + k]).double()
        got = named[k].grad.detach().cpu().double()
        rel = float((got - want).norm() / want.norm())
        cos = float((got * want).sum() / (got.norm() * want.norm()))
        report.append(f"{'ok ' if rel <= 5e-3 and cos >= 0.99999 else 'BAD'} {k}: rel {rel:.2e} cos {cos:.5f}")
    print("\n".join(report))
    assert report and not [r for r in report if r.startswith("BAD")], "\n".join(report)


@pytest.mark.gpu
def test_whole_training_step_through_the_operator_matches_the_reference_step():
    """tests/test_training.py::test_whole_training_step_matches_the_reference_step (unfused) with `ray_loss_backend="hip"`: every loss term
    to 2e-4, the parameter gradients to 5e-3 of their norm with a cosine of at least 0.99999."""
    from nerflidar_hip import training as ntrain, weights as nweights, lidar as nlidar, config as ncfg
    g = golden("train_step_REF")
    mc = ncfg.workload("REF", int(g["log2_hashmap"]))
    mc.config.use_intensity = True
    mc.__post_init__()
    sd = nweights.synth_state_dict(mc, seed=int(g["seed"]), trained_like=True)
    b = nlidar.synthetic_sweep(width=int(g["width"]), seed=int(g["seed"]), beams=list(g["beams"]))
    batch = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    for k in ("rgb", "depth", "intensity", "semantic", "mask", "patch_mask", "lidar_mask"):
        batch[k] = torch.from_numpy(g["sup_" + k]).cuda()
    batch.update(nl.nusc_masks(batch, lidar_supervision=True))
    tm = ntrain.TrainableModel(mc, fused_mlp=False).cuda().load_reference(sd)
    rend, hist = tm(batch, train_frac=float(g["train_frac"]), randomized=False)
    assert not any(h["sdist"].requires_grad for h in hist)
    terms = nl.total_loss(rend, hist, batch, data_kind=str(g["data_loss_type"]), charb_padding=float(g["charb_padding"]),
                          data_coarse_mult=float(g["data_coarse_mult"]), data_mult=float(g["data_mult"]),
                          interlevel_mult=float(g["inter_mult"]), anti_interlevel_mult=float(g["anti_mult"]),
                          pulse_width=g["pulse_width"].tolist(), distortion_mult=float(g["dist_mult"]), depth_lam=0.1, sem_lam=0.01,
                          ray_loss_backend="hip")
    loss = sum(terms.values())
    loss.backward()
    ntrain.clip_gradients(tm)
    assert set(terms) == {k[5:] for k in g if k.startswith("loss_")}
    for k, v in terms.items():
        print(f"{k}: {float(v.detach()):.8g} reference {float(g['loss_' + k]):.8g}")
    for k, v in terms.items():
        np.testing.assert_allclose(float(v.detach()), float(g["loss_" + k]), rtol=2e-4, atol=1e-7, err_msg=k)
    np.testing.assert_allclose(float(loss.detach()), float(g["loss"]), rtol=2e-4)
    _gradient_report(tm, g)


@pytest.mark.gpu
def test_whole_training_step_with_dynamic_objects_through_the_operator():
    """The shipped configuration's step (test_training.py::test_whole_training_step_with_dynamic_objects_matches_the_reference_step) with
    `ray_loss_backend="hip"`: `obj_mask` in the history of both proposal levels; terms to 2e-4, gradients to that test's gates."""
    from nerflidar_hip import training as ntrain, weights as nweights, lidar as nlidar, config as ncfg
    g = golden("train_step_OBJ")
    lg, seed = int(g["log2_hashmap"]), int(g["seed"])
    mc = ncfg.workload("REF", lg)
    mc.config.instance_obj, mc.config.latent_size = True, 128
    mc.__post_init__()
    names = {13: "vehicle.car", 14: "vehicle.truck", 15: "vehicle.bus.rigid", 11: "human.pedestrian.adult"}
    class_names = [names[int(c)] for c in g["class_ids"]]
    sd = nweights.synth_state_dict(mc, seed=seed, trained_like=True)
    cids = sorted(set(int(c) for c in g["class_ids"]))
    sd.update(nweights.synth_object_state_dict({c: ncfg.obj_mlp_config(c, latent_size=128, log2_hashmap=lg) for c in cids}, len(class_names), seed=seed))
    b = nlidar.synthetic_sweep(width=int(g["width"]), seed=seed, beams=list(g["beams"]))
    batch = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    batch["timestamp"] = torch.from_numpy(g["timestamp"]).cuda()
    for k in ("rgb", "depth", "semantic", "mask", "patch_mask", "lidar_mask"):
        batch[k] = torch.from_numpy(g["sup_" + k]).cuda()
    batch.update(nl.nusc_masks(batch, lidar_supervision=True, instance_obj=True))
    tm = ntrain.TrainableModel(mc, tracks=g["tracks"], class_names=class_names, obj_log2_hashmap=lg).cuda().load_reference(sd)
    rend, hist = tm(batch, train_frac=float(g["train_frac"]), randomized=False)
    assert all("obj_mask" in h for h in hist[:-1]) and bool(hist[0]["obj_mask"].any())
    terms = nl.total_loss(rend, hist, batch, depth_lam=0.1, sem_lam=0.01, ray_loss_backend="hip")
    terms["latent_reg"] = tm.latent_reg(float(g["latent_reg"]))
    loss = sum(terms.values())
    loss.backward()
    ntrain.clip_gradients(tm)
    assert set(terms) == {k[5:] for k in g if k.startswith("loss_")}
    for k, v in terms.items():
        np.testing.assert_allclose(float(v.detach()), float(g["loss_" + k]), rtol=2e-4, atol=1e-7, err_msg=k)
    np.testing.assert_allclose(float(loss.detach()), float(g["loss"]), rtol=2e-4)
    _gradient_report(tm, g, skip=("grad_latents",))


@pytest.mark.gpu
def test_fused_training_step_with_the_operator_reads_nothing_back():
    """A fused `training_step(..., ray_loss_backend="hip")` under `torch.cuda.set_sync_debug_mode("error")` after one warm-up step: the
    operator, its autograd wrapper and `total_loss` read nothing back."""
    from nerflidar_hip import training as ntrain, scene as nscene, weights as nweights, config as ncfg
    mc = ncfg.workload("REF", 12)
    mc.config.use_intensity = True
    mc.__post_init__()
    tm = ntrain.TrainableModel(mc, fused_mlp=True).cuda().load_reference(nweights.synth_state_dict(mc, seed=0, trained_like=True))
    opt = torch.optim.Adam(tm.parameters(), lr=1e-3, eps=1e-15)
    batch = nscene.supervise(nscene.random_lidar_rays(2048, 0, 1, torch.device("cuda")))
    first = ntrain.training_step(tm, opt, batch, ray_loss_backend="hip")     # warm-up: lazy initialisations may read back
    assert {"interlevel", "distortion"} <= set(first) and all(np.isfinite(v) for v in first.values()) and first["interlevel"] > 0
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ntrain.training_step(tm, opt, batch, as_tensors=True, ray_loss_backend="hip")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(isinstance(v, torch.Tensor) and v.is_cuda and v.dim() == 0 for v in out.values())
    assert np.isfinite(float(out["loss"])) and float(out["interlevel"]) > 0 and float(out["distortion"]) > 0
