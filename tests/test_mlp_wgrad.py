"""nlr_mlp_train_wgrad (csrc/nlr_mlp_wgrad.hip): the weight and bias gradients of the fused training NerfMLP as one MFMA kernel plus a
slab reduce, against float64 GEMMs over the tensors the forward / backward kernels saved, and against the split-K library GEMMs
(`training._wgrad_bmm`) that remain the default."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from nerflidar_hip import _lib, training as ntrain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nlr_mlp_train_wgrad", "nlr_mlp_train_wgrad_workspace_bytes")


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------
def test_wgrad_entry_points_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "nerflidar_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    declared = set(re.findall(r"\b(nlr_[a-z_0-9]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW:
        assert name in declared, f"{name} not declared in include/nerflidar_hip.h"
        assert name in _lib.EXPORTS, f"{name} not in _lib.EXPORTS"
        assert hasattr(L, name), f"{name} not exported by the library"
    assert L.nlr_mlp_train_wgrad_workspace_bytes.restype is C.c_size_t
    assert L.nlr_mlp_train_wgrad_workspace_bytes(None, 0) == 0


def test_fused_wgrad_needs_fused_mlp_and_defaults_to_off():
    import inspect
    from nerflidar_hip import config as nconfig
    cfg = nconfig.workload("REF", 12).nerf_mlp
    with pytest.raises(ValueError):
        ntrain.TrainableNerfLevel(cfg, fused_mlp=False, fused_wgrad=True)
    for cls in (ntrain.TrainableNerfLevel, ntrain.TrainableModel):
        assert inspect.signature(cls.__init__).parameters["fused_wgrad"].default is False


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------
def _bf16_ste(t):
    return t + (t.to(torch.bfloat16).float() - t).detach()


def _level_forward_bf16_operands(lvl, batch, tdist):
    """TrainableNerfLevel.forward with every Linear's input and weight rounded to bf16 (the arithmetic of the fused kernels) in torch
    ops: the autograd reference of tests/test_training.py::test_fused_training_mlp_matches_torch_autograd."""
    from nerflidar_hip.objects import _pos_enc
    F = torch.nn.functional
    cfg = lvl.cfg
    lin = lambda m, x: F.linear(_bf16_ste(x), _bf16_ste(m.weight), m.bias)
    means, stds = ntrain.cast_contract(batch, tdist)
    f = ntrain.encode_features(lvl.encoder, means, stds, cfg.re_weights)
    x = lin(lvl.density_layer[2], F.relu(lin(lvl.density_layer[0], f)))
    out = {"density": F.softplus(x[..., 0] + cfg.density_bias)}
    if cfg.use_semantic:
        out["semantic"] = torch.softmax(lin(lvl.sem_layer[2], F.relu(lin(lvl.sem_layer[0], x))), -1)
    if cfg.use_intensity:
        out["intensity"] = lin(lvl.intensity_layer[2], F.relu(lin(lvl.intensity_layer[0], x)))[..., 0]
    enc = _pos_enc(batch["viewdirs"].reshape(x.shape[0], 3).float(), cfg.deg_view)
    h = torch.cat([x, enc[:, None, :].expand(-1, x.shape[1], -1)], dim=-1)
    inputs = h
    for i in range(cfg.net_depth_viewdirs):
        h = F.relu(lin(getattr(lvl, f"lin_second_stage_{i}"), h))
        if i == cfg.skip_layer_dir:
            h = torch.cat([h, inputs], dim=-1)
    rgb = torch.sigmoid(cfg.rgb_premultiplier * lin(lvl.rgb_layer, h) + cfg.rgb_bias)
    out["rgb"] = rgb * (1 + 2 * cfg.rgb_padding) - cfg.rgb_padding
    return out


def _scene(wl, S, width=6, stride=8, rays=None):
    """The inputs of test_fused_training_mlp_matches_torch_autograd (same seeds, same table gain, same cotangents); `rays` keeps the
    first few rays of the sweep only."""
    from nerflidar_hip import config as nconfig, lidar as nlidar, weights as nweights
    mc = nconfig.workload(wl, 12)
    sd = nweights.synth_state_dict(mc, seed=5, trained_like=False)
    for k in sd:
        if k.endswith("encoder.embeddings"):
            sd[k] = (sd[k] * 3e3).astype(np.float32)
    b = nlidar.synthetic_sweep(width=width, seed=5, beams=nlidar.LIDAR_ANGLES[::stride])
    if rays is not None:
        b = {k: v[:rays] for k, v in b.items()}
    N = b["origins"].shape[0]
    rng = np.random.default_rng(0)
    tdist = torch.from_numpy(np.sort(rng.uniform(0.01, 1.5, (N, S + 1)).astype(np.float32), axis=-1)).cuda()
    batch = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    cfg = mc.nerf_mlp
    cot = {"density": rng.normal(size=(N, S)), "rgb": rng.normal(size=(N, S, 3))}
    if cfg.use_semantic:
        cot["semantic"] = rng.normal(size=(N, S, cfg.class_num))
    if cfg.use_intensity:
        cot["intensity"] = rng.normal(size=(N, S))
    cot = {k: torch.from_numpy(v.astype(np.float32)).cuda() for k, v in cot.items()}
    return cfg, sd, batch, tdist, cot, N


def _run_level(cfg, sd, batch, tdist, cot, fused_wgrad):
    lvl = ntrain.TrainableNerfLevel(cfg, fused_mlp=True, fused_wgrad=fused_wgrad).load_reference(sd).cuda()
    lvl._keep_debug = True
    o = lvl(batch, tdist)
    sum((o[k] * cot[k]).sum() for k in cot).backward()
    torch.cuda.synchronize()
    return lvl


def _linears(cfg, aw):
    """The table of the header (section 6b, wgrad): per Linear in flat order (gacts column, rows, input blocks); an input block is
    ("acts", column, width), ("feat", 0, F) or ("enc", 0, E)."""
    W, WB, D = cfg.net_width_viewdirs, cfg.bottleneck_width, cfg.net_depth_viewdirs
    K = cfg.class_num if cfg.use_semantic else 0
    HH = (64 if K else 0) + (64 if cfg.use_intensity else 0)
    c_hid, c_hbe, c_q, c_x = 0, 64, 64 + WB, 64 + WB + HH
    assert aw == c_x + D * W
    F, E = cfg.grid_num_levels * cfg.grid_level_dim, cfg.dim_dir_enc
    hbe, enc = ("acts", c_hbe, WB), ("enc", 0, E)
    t = [(c_hid, 64, [("feat", 0, F)]), (c_hbe, WB, [("acts", c_hid, 64)])]
    r0 = 0
    if K:
        t += [(c_q, 64, [hbe]), (aw, K, [("acts", c_q, 64)])]
        r0 = 64
    if cfg.use_intensity:
        t += [(c_q + r0, 64, [hbe]), (aw + K, 1, [("acts", c_q + r0, 64)])]
    t += [(c_x, W, [hbe, enc]), (c_x + W, W, [("acts", c_x, W), hbe, enc])]
    t += [(c_x + l * W, W, [("acts", c_x + (l - 1) * W, W)]) for l in range(2, D)]
    t += [(aw + 32, 3, [("acts", c_x + (D - 1) * W, W)])]
    return t


def _want_f64(cfg, dbg, S):
    """float64 weight and bias gradients from the saved tensors, flat in parameter order, with the per-element bound
    M 2^-23 sum_m |g x| + one f32 ulp of the value."""
    A, G = dbg["acts"].double().cpu(), dbg["gacts"].double().cpu()
    M, aw = A.shape
    src = {"acts": A, "feat": dbg["feats"].to(torch.bfloat16).double().cpu(),
           "enc": dbg["enc"].to(torch.bfloat16).double().cpu().repeat_interleave(S, dim=0)}
    want, bound = [], []
    for g0, n_out, blocks in _linears(cfg, aw):
        g = G[:, g0:g0 + n_out]
        x = torch.cat([src[s][:, c:c + n] for s, c, n in blocks], 1)
        for w, b in ((g.t() @ x, g.abs().t() @ x.abs()), (g.sum(0), g.abs().sum(0))):
            want.append(w.reshape(-1).numpy())
            bound.append(b.reshape(-1).numpy())
    want, bound = np.concatenate(want), np.concatenate(bound)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return want, M * 2.0 ** -23 * bound + ulp


def _flat_grads(lvl):
    return torch.cat([p.grad.reshape(-1).float() for p in lvl._mlp_params()]).double().cpu().numpy()


CASES = [("C2", 32, {}), ("REF", 32, {}), ("P_W128I", 64, {}), ("P_NOSEM", 32, {}), ("P_D3", 32, {}),
         ("C2", 32, dict(width=7, stride=11)), ("REF", 32, dict(rays=3))]


@pytest.mark.gpu
@pytest.mark.parametrize("wl,S,kw", CASES, ids=[f"{w}-{s}-{'-'.join(f'{k}{v}' for k, v in kw.items()) or 'base'}" for w, s, kw in CASES])
def test_wgrad_kernel_matches_float64_on_the_saved_tensors(wl, S, kw):
    """Every weight and bias gradient against `gacts.double().T @ x.double()` over the tensors the kernels saved.
    Per element: |got - want| <= M 2^-23 sum_m |gacts[m,o] x[m,i]| + one f32 ulp of want (an f32 sum of M exact products in any order,
    unit roundoff doubled for the MFMA's adder).  As one flat vector: relative norm error at most 1/100 of what the library-GEMM
    path (`fused_wgrad=False`, bf16 partial results) leaves on the same tensors."""
    cfg, sd, batch, tdist, cot, N = _scene(wl, S, **kw)
    M = N * S
    if kw.get("stride") == 11:
        assert M % 128 != 0 and M > 128, M
    if "rays" in kw:
        assert M < 128, M
    old = _run_level(cfg, sd, batch, tdist, cot, False)
    new = _run_level(cfg, sd, batch, tdist, cot, True)
    for k in ("acts", "gacts", "d_feat"):
        assert torch.equal(old._dbg[k], new._dbg[k]), f"{k} differs between fused_wgrad=False and True"
    assert "d_params" in new._dbg and "d_params" not in old._dbg
    want, bound = _want_f64(cfg, new._dbg, S)
    got, got_bmm = _flat_grads(new), _flat_grads(old)
    assert got.shape == want.shape == (new._plan.n_params,)
    np.testing.assert_array_equal(new._dbg["d_params"].double().cpu().numpy(), got)
    err = np.abs(got - want)
    worst = int(np.argmax(err / bound))
    nrm = float(np.linalg.norm(want))
    e_new, e_bmm = float(np.linalg.norm(got - want)) / nrm, float(np.linalg.norm(got_bmm - want)) / nrm
    print(f"wgrad {wl} S={S} M={M}: err_new {e_new:.3e}  err_bmm {e_bmm:.3e}  ratio {e_bmm / max(e_new, 1e-300):.0f}  "
          f"worst element {err[worst]:.3e} of bound {bound[worst]:.3e}")
    assert (err <= bound).all(), f"{wl}: element {worst}: |got - want| = {err[worst]:.3e} > bound {bound[worst]:.3e} ({int((err > bound).sum())} elements)"
    assert e_new <= e_bmm / 100, f"{wl}: err_new {e_new:.3e} > err_bmm {e_bmm:.3e} / 100"
    read = {id(p) for p in new._mlp_params()}
    for (name, p), (_, po) in zip(new.named_parameters(), old.named_parameters()):
        if id(p) not in read and not name.startswith("encoder."):
            assert p.grad is None and po.grad is None, name   # built but not read (sem_layer without use_semantic)


def _call_wgrad(lvl, dbg, gacts=None, S=None, d_params=None, ws_bytes=None, null=()):
    plan = lvl._plan
    M = dbg["acts"].shape[0]
    ws = lvl._wgrad_workspace(dbg["acts"].device)
    args = dict(features=dbg["feats"], enc=dbg["enc"], acts=dbg["acts"], gacts=dbg["gacts"] if gacts is None else gacts)
    for k in null:
        args[k] = None
    if d_params is None:
        d_params = torch.full((plan.n_params,), float("nan"), device="cuda")
    rc = _lib.lib().nlr_mlp_train_wgrad(plan.handle, M, lvl._S if S is None else S, _lib.ptr(args["features"]), _lib.ptr(args["enc"]),
                                        _lib.ptr(args["acts"]), _lib.ptr(args["gacts"]), _lib.ptr(d_params), _lib.ptr(ws),
                                        ws.numel() if ws_bytes is None else ws_bytes, _lib.current_stream())
    torch.cuda.synchronize()
    return rc, d_params


@pytest.fixture(scope="module")
def c2_level():
    cfg, sd, batch, tdist, cot, N = _scene("C2", 32)
    return _run_level(cfg, sd, batch, tdist, cot, True)


@pytest.mark.gpu
def test_wgrad_is_bit_reproducible(c2_level):
    rc1, a = _call_wgrad(c2_level, c2_level._dbg)
    rc2, b = _call_wgrad(c2_level, c2_level._dbg)
    assert rc1 == 0 and rc2 == 0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(a.view(torch.int32), c2_level._dbg["d_params"].view(torch.int32))


@pytest.mark.gpu
def test_wgrad_writes_every_element(c2_level):
    lvl, d = c2_level, c2_level._dbg
    cfg, plan = lvl.cfg, lvl._plan
    rc, out = _call_wgrad(lvl, d)   # d_params pre-filled with NaN
    assert rc == 0 and not bool(torch.isnan(out).any())
    # the backward without head cotangents: the head columns of gacts are zero, and so are the head gradients, exactly
    assert cfg.use_semantic or cfg.use_intensity
    M = d["acts"].shape[0]
    g = torch.Generator(device="cuda").manual_seed(1)
    gd, gr = torch.randn(M, device="cuda", generator=g), torch.randn(3, M, device="cuda", generator=g)
    gacts = torch.empty_like(d["gacts"])
    d_feat = torch.empty_like(d["d_feat"])
    sem = d["sem"] if d["sem"].numel() else None
    _lib.check(_lib.lib().nlr_mlp_train_backward(plan.handle, M, lvl._S, _lib.ptr(d["density"]), _lib.ptr(d["rgb"]), _lib.ptr(sem),
                                                 _lib.ptr(d["acts"]), _lib.ptr(gd), _lib.ptr(gr), None, None, _lib.ptr(gacts),
                                                 _lib.ptr(d_feat), _lib.current_stream()), "nlr_mlp_train_backward")
    rc, out = _call_wgrad(lvl, d, gacts=gacts)
    assert rc == 0 and not bool(torch.isnan(out).any())
    heads = {id(p) for m in ([lvl.sem_layer] if cfg.use_semantic else []) + ([lvl.intensity_layer] if cfg.use_intensity else [])
             for p in m.parameters()}
    off, n_head = 0, 0
    for p in lvl._mlp_params():
        if id(p) in heads:
            assert float(out[off:off + p.numel()].abs().max()) == 0.0
            n_head += p.numel()
        off += p.numel()
    assert n_head > 0 and float(out.abs().max()) > 0.0


@pytest.mark.gpu
def test_wgrad_refusals_launch_nothing(c2_level):
    lvl, d = c2_level, c2_level._dbg
    M = d["acts"].shape[0]
    need = int(_lib.lib().nlr_mlp_train_wgrad_workspace_bytes(lvl._plan.handle, M))
    assert need == lvl._wgrad_workspace(d["acts"].device).numel() and 0 < need < 256 << 20
    assert need == int(_lib.lib().nlr_mlp_train_wgrad_workspace_bytes(lvl._plan.handle, 64 * M))   # does not grow with M
    assert M % 5 != 0
    for kw, word in ((dict(ws_bytes=need - 1), "workspace"), (dict(null=("gacts",)), "gacts"), (dict(S=5), "M % S")):
        pre = torch.full((lvl._plan.n_params,), 7.0, device="cuda")
        rc, out = _call_wgrad(lvl, d, d_params=pre, **kw)
        msg = _lib.lib().nlr_last_error().decode()
        assert rc != 0 and word in msg, (kw, rc, msg)
        assert bool((out == 7.0).all()), kw


@pytest.mark.gpu
@pytest.mark.parametrize("wl", ["C2", "REF"])
def test_fused_wgrad_end_to_end_matches_torch_autograd_and_trains(wl):
    """Part (3) and the Adam steps of test_fused_training_mlp_matches_torch_autograd with fused_wgrad=True, at that test's gates."""
    S = 32
    cfg, sd, batch, tdist, cot, N = _scene(wl, S)
    ref = ntrain.TrainableNerfLevel(cfg).load_reference(sd).cuda()
    fus = ntrain.TrainableNerfLevel(cfg, fused_mlp=True, fused_wgrad=True).load_reference(sd).cuda()
    for name, lvl in (("ref", ref), ("fus", fus)):
        o = _level_forward_bf16_operands(lvl, batch, tdist) if name == "ref" else lvl(batch, tdist)
        sum((o[k] * cot[k]).sum() for k in cot).backward()
    for (name, p), (_, pf) in zip(ref.named_parameters(), fus.named_parameters()):
        if p.grad is None:
            assert pf.grad is None, name
            continue
        assert pf.grad is not None, name
        got, want = pf.grad.float().cpu().numpy(), p.grad.float().cpu().numpy()
        err = float(np.linalg.norm(got - want)) / max(float(np.linalg.norm(want)), 1e-30)
        assert err <= 4e-2, f"{wl} grad {name}: relative norm error {err:.3e} > 4e-2"
    opt = torch.optim.Adam(fus.parameters(), lr=2e-3)
    losses = []
    for _ in range(8):
        opt.zero_grad()
        r, _ = fus.render(batch, tdist)
        loss = ((r["depth"] - 0.7) ** 2).mean() + ((r["rgb"] - 0.25) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0], losses


@pytest.mark.gpu
def test_training_step_with_fused_wgrad_reads_nothing_back():
    """test_training_step_reads_nothing_back_until_its_terms_are_asked_for with the weight-gradient kernel in the step."""
    from nerflidar_hip import config as nconfig, scene as nscene, weights as nweights
    mc = nconfig.workload("REF", 12)
    mc.config.use_intensity = True
    mc.__post_init__()
    tm = ntrain.TrainableModel(mc, fused_mlp=True, fused_wgrad=True).cuda().load_reference(nweights.synth_state_dict(mc, seed=0, trained_like=True))
    assert tm.nerf_mlp.fused_wgrad
    opt = torch.optim.Adam(tm.parameters(), lr=1e-3, eps=1e-15)
    batch = nscene.supervise(nscene.random_lidar_rays(2048, 0, 1, torch.device("cuda")))
    first = ntrain.training_step(tm, opt, batch)   # warm-up: lazy initialisations may read back
    assert all(np.isfinite(v) for v in first.values())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ntrain.training_step(tm, opt, batch, as_tensors=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(isinstance(v, torch.Tensor) and v.is_cuda and v.dim() == 0 for v in out.values())
    assert np.isfinite(float(out["loss"]))
