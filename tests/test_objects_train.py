"""The object branch of a level as a training operator (header section 7e: `nlr_obj_train_forward` / `_backward`,
`training._ObjectsFused`, `TrainableModel(fused_objects=True)`): the reference's dynamic-object step through it, no host read in a step,
the operator against a float64 restatement next to the unfused f32 path, forward values against `nlr_objects_apply`, repeatability,
the ABI's refusals, the refusals in Python; on the CPU the parameter layout and the rewritten `anti_interlevel_loss`."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from nerflidar_hip import config as nconfig, losses as nl, objects as nobj, weights as nweights

LAT = 16  # latent size of the operator tests (the step tests use the fixture's 128)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def _layout(cfg):
    """(offsets, n_params) of the flat buffer as section 7e states it, from `weights.mlp_param_shapes`."""
    offs, at = [], 0
    for name, (o, i), _ in nweights.mlp_param_shapes(cfg):
        offs += [at, at + o * i]
        at += o * i + o
    return offs, at


LAYOUT_CASES = [(2, 0, True, 128), (2, 4, True, 128), (3, 1, True, 16), (4, 2, False, 8), (1, 0, True, 0)]


def _layout_cfg(depth, skip, split, lat):
    import dataclasses
    return dataclasses.replace(nconfig.obj_mlp_config(13, latent_size=lat, log2_hashmap=10), net_depth_viewdirs=depth, skip_layer_dir=skip,
                               split_latent=split)


@pytest.mark.parametrize("depth,skip,split,lat", LAYOUT_CASES)
def test_param_layout_follows_the_linear_shapes(depth, skip, split, lat):
    """`nlr_obj_train_desc_layout` (host arithmetic, no device) against `weights.mlp_param_shapes(obj_mlp_config(..))`: the shipped
    ObjMLP (skip concatenation behind layer 0: 19 555 parameters), no concatenation inside the depth, a `skip_layer_dir` inside three
    and four layers, an unsplit latent code, no latent code."""
    from nerflidar_hip import _lib, training as ntrain
    cfg = _layout_cfg(depth, skip, split, lat)
    od, keep = ntrain.objects_desc([ntrain.TrainableObjMLP(cfg)], [0, 0], lat)
    offs = (C.c_uint32 * 32)()
    n = _lib.lib().nlr_obj_train_desc_layout(C.byref(od), 0, offs, 32)
    want, total = _layout(cfg)
    assert n == len(want) + 1 and list(offs[:n]) == want + [total]
    if (depth, skip, split, lat) == LAYOUT_CASES[0]:
        assert total == (64 * 78 + 64) + (64 * 64 + 64) + (32 * 143 + 32) + (32 * 175 + 32) + (3 * 32 + 3) == 19555
    assert _lib.lib().nlr_obj_train_desc_layout(C.byref(od), 0, offs, 3) == -1 and b"too small" in _lib.lib().nlr_last_error()
    assert _lib.lib().nlr_obj_train_desc_layout(C.byref(od), 1, offs, 32) == -1


def test_layer_table_at_the_edges_of_the_envelope():
    """The one layer table of the object network (csrc/nlr_obj_layers.h, read through `nlr_obj_train_desc_layout`) against
    `weights.mlp_param_shapes`, the independent Python statement, at the envelope's edges: depth 1, depth 4 with the skip concatenation
    behind every layer 0..3, no latent code, next to `LAYOUT_CASES`.  A depth of 0 or 5 is refused with the message of today."""
    from nerflidar_hip import _lib, training as ntrain
    L = _lib.lib()
    cases = LAYOUT_CASES + [(1, 0, True, 16), (1, 4, False, 16)] + [(4, s, split, 16) for s in range(4) for split in (True, False)]
    cases += [(d, s, True, 0) for d, s in ((1, 0), (2, 0), (4, 3))]
    offs = (C.c_uint32 * 32)()
    for depth, skip, split, lat in cases:
        cfg = _layout_cfg(depth, skip, split, lat)
        od, keep = ntrain.objects_desc([ntrain.TrainableObjMLP(cfg)], [0, 0], lat)
        n = L.nlr_obj_train_desc_layout(C.byref(od), 0, offs, 32)
        want, total = _layout(cfg)
        assert n == 2 * (depth + 3) + 1 == len(want) + 1 and list(offs[:n]) == want + [total], (depth, skip, split, lat)
    od, keep = ntrain.objects_desc([ntrain.TrainableObjMLP(_layout_cfg(2, 4, True, 16))], [0, 0], 16)
    for depth in (0, 5):
        od.classes[0].mlp.net_depth_viewdirs = depth
        assert L.nlr_obj_train_desc_layout(C.byref(od), 0, offs, 32) == -2   # NLR_ERR_UNSUPPORTED
        assert L.nlr_last_error().decode() == f"obj_train_desc_layout: net_depth_viewdirs {depth} outside [1,4]"


@pytest.mark.gpu
@pytest.mark.parametrize("depth,skip,split,lat", LAYOUT_CASES[:4])
def test_plan_layout_is_the_descriptor_layout(depth, skip, split, lat):
    """The plan's own table (`nlr_obj_train_param_layout`, made of the packed images' offsets) gives the same offsets and count."""
    from nerflidar_hip import _lib, training as ntrain
    cfg = _layout_cfg(depth, skip, split, lat)
    plan = ntrain._ObjTrainPlan([ntrain.TrainableObjMLP(cfg)], [0, 0], lat, "cuda")   # (its constructor compares with the module too)
    offs = (C.c_uint32 * 32)()
    n = _lib.lib().nlr_obj_train_param_layout(plan.handle, 0, offs, 32)
    want, total = _layout(cfg)
    assert list(offs[:n]) == want and plan.n_params == [total]
    import copy
    assert copy.deepcopy(plan) is None   # a copied model makes its own plan: the handle is never shared


def _anti_old(ray_history, mult, pulse_width):
    """`anti_interlevel_loss` with the boolean-mask selection it had before (train_utils.py:153-157)."""
    c, w = ray_history[-1]["sdist"].detach(), ray_history[-1]["weights"].detach()
    pdf = (w / (c[..., 1:] - c[..., :-1])).clamp_max(10)
    total = 0.0
    for i, h in enumerate(ray_history[:-1]):
        knots, val = nl.blur_stepfun(c, pdf, pulse_width[i])
        area = 0.5 * (val[..., 1:] + val[..., :-1]) * torch.diff(knots, dim=-1)
        cdf = torch.cat([torch.zeros_like(area[..., :1]), torch.cumsum(area, dim=-1)], dim=-1)
        term = (torch.diff(nl._quad_cdf_at(h["sdist"], knots, val, cdf), dim=-1) - h["weights"]).clamp_min(0) ** 2 / (h["weights"] + 1e-5)
        total = total + (term[~h["obj_mask"]] if "obj_mask" in h else term).mean()
    return mult * total


def _random_history(seed, n=23, S=(9, 7, 5), masked=0.3):
    gen = torch.Generator().manual_seed(seed)
    hist = []
    for s in S:
        sd = torch.sort(torch.rand(n, s + 1, generator=gen), dim=-1)[0]
        w = torch.softmax(torch.randn(n, s, generator=gen), dim=-1).requires_grad_(True)
        hist.append(dict(sdist=sd, weights=w, obj_mask=torch.rand(n, s, generator=gen) < masked))
    return hist


def test_anti_interlevel_loss_selects_without_indexing():
    """The `torch.where` / count form against the boolean-index expression on a random mask: value and gradient to f32 summation
    accuracy; an all-masked level is the mean of nothing (nan), as before."""
    hist = _random_history(3)
    a = nl.anti_interlevel_loss(hist, 0.7, [0.03, 0.003])
    b = _anti_old(hist, 0.7, [0.03, 0.003])
    np.testing.assert_allclose(float(a), float(b), rtol=2e-6)
    ga = torch.autograd.grad(a, [h["weights"] for h in hist[:-1]])
    gb = torch.autograd.grad(b, [h["weights"] for h in hist[:-1]])
    for x, y in zip(ga, gb):
        np.testing.assert_allclose(x.numpy(), y.numpy(), rtol=1e-5, atol=1e-7 * float(y.abs().max()))
        assert float(x[hist[0]["obj_mask"]].abs().max() if x.shape == hist[0]["obj_mask"].shape else 0.0) == 0.0
    hist[0]["obj_mask"][:] = True
    assert torch.isnan(nl.anti_interlevel_loss(hist, 1.0, [0.03, 0.003])) and torch.isnan(_anti_old(hist, 1.0, [0.03, 0.003]))


def test_anti_interlevel_loss_with_obj_mask_matches_the_fixture():
    """`fn_losses.npz` with `obj_mask` on both proposal levels: value and gradient of the rewritten term, through the fixture's own
    check (tests/test_losses.py)."""
    from test_losses import _check, _history
    g = golden("fn_losses")
    hist = _history(g)
    hist[0]["obj_mask"], hist[1]["obj_mask"] = torch.from_numpy(g["obj_mask0"]), torch.from_numpy(g["obj_mask1"])
    _check(nl.anti_interlevel_loss(hist, float(g["anti_mult"]), g["pulse_width"].tolist()), hist, g, "anti_masked", levels=(0, 1))


# ---- GPU: the reference's step ---------------------------------------------------------------------------------------------------
def _obj_step_scene():
    """Model, batch and fixture of `test_whole_training_step_with_dynamic_objects_matches_the_reference_step` (tests/test_training.py)."""
    from nerflidar_hip import lidar as nlidar
    g = golden("train_step_OBJ")
    lg, seed = int(g["log2_hashmap"]), int(g["seed"])
    mc = nconfig.workload("REF", lg)
    mc.config.instance_obj, mc.config.latent_size = True, 128
    mc.__post_init__()
    names = {13: "vehicle.car", 14: "vehicle.truck", 15: "vehicle.bus.rigid", 11: "human.pedestrian.adult"}
    class_names = [names[int(c)] for c in g["class_ids"]]
    sd = nweights.synth_state_dict(mc, seed=seed, trained_like=True)
    cids = sorted(set(int(c) for c in g["class_ids"]))
    sd.update(nweights.synth_object_state_dict({c: nconfig.obj_mlp_config(c, latent_size=128, log2_hashmap=lg) for c in cids}, len(class_names), seed=seed))
    b = nlidar.synthetic_sweep(width=int(g["width"]), seed=seed, beams=list(g["beams"]))
    batch = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    batch["timestamp"] = torch.from_numpy(g["timestamp"]).cuda()
    for k in ("rgb", "depth", "semantic", "mask", "patch_mask", "lidar_mask"):
        batch[k] = torch.from_numpy(g["sup_" + k]).cuda()
    batch.update(nl.nusc_masks(batch, lidar_supervision=True, instance_obj=True))
    return g, mc, sd, class_names, lg, batch


_STEP = {}


def _fused_step():
    """The body of `test_whole_training_step_with_dynamic_objects_matches_the_reference_step` with `fused_objects=True`, run once."""
    if _STEP:
        return _STEP
    from nerflidar_hip import training as ntrain
    g, mc, sd, class_names, lg, batch = _obj_step_scene()
    tm = ntrain.TrainableModel(mc, tracks=g["tracks"], class_names=class_names, obj_log2_hashmap=lg, fused_objects=True).cuda().load_reference(sd)
    rend, hist = tm(batch, train_frac=float(g["train_frac"]), randomized=False)
    terms = nl.total_loss(rend, hist, batch, depth_lam=0.1, sem_lam=0.01)
    terms["latent_reg"] = tm.latent_reg(float(g["latent_reg"]))
    loss = sum(terms.values())
    loss.backward()
    ntrain.clip_gradients(tm)
    plain = ntrain.TrainableModel(mc, tracks=g["tracks"], class_names=class_names, obj_log2_hashmap=lg)
    _STEP.update(g=g, masks=[h["obj_mask"].cpu() for h in hist], terms={k: float(v.detach()) for k, v in terms.items()}, loss=float(loss.detach()),
                 depth=rend[-1]["depth"].detach().cpu().numpy(), rgb=rend[-1]["rgb"].detach().cpu().numpy(),
                 grads={k: p.grad.detach().cpu() for k, p in tm.named_parameters() if p.grad is not None}, n_tracks=len(class_names),
                 same_names=set(tm.state_dict()) == set(plain.state_dict()))
    return _STEP


@pytest.mark.gpu
def test_reference_step_through_the_fused_object_operator():
    """The reference's dynamic-object step (fixture train_step_OBJ) with `fused_objects=True`: owner maps of the three levels exactly,
    loss terms and total to 2e-4, every gradient of the fixture - ObjMLP trunk, view layers, rgb layer, hash table, the latent codes of
    all tracks, static parameters - to 5e-3 of its norm and cosine 0.99999: the unfused path's gates."""
    st = _fused_step()
    g = st["g"]
    for lvl, m in enumerate(st["masks"]):
        assert torch.equal(m, torch.from_numpy(g[f"hist{lvl}_obj_mask"])), f"owner map of level {lvl}"
    assert set(st["terms"]) == {k[5:] for k in g if k.startswith("loss_")}
    for k, v in st["terms"].items():
        print(f"{k}: {v:.8g} (reference {float(g['loss_' + k]):.8g})")
        np.testing.assert_allclose(v, float(g["loss_" + k]), rtol=2e-4, atol=1e-7, err_msg=k)
    np.testing.assert_allclose(st["loss"], float(g["loss"]), rtol=2e-4)
    grads = st["grads"]
    got_lat = torch.stack([grads[f"latent_vector_dict.obj_latent_{t}"] for t in range(st["n_tracks"])])
    checks = [(k[5:], grads[k[5:]], torch.from_numpy(g[k])) for k in g if k.startswith("grad_") and k != "grad_latents"]
    checks.append(("latent_vector_dict (all tracks)", got_lat, torch.from_numpy(g["grad_latents"])))
    report = []
    for k, got, want in checks:
        got, want = got.double(), want.double()
        rel = float((got - want).norm() / want.norm())
        cos = float((got * want).sum() / (got.norm() * want.norm()))
        report.append(f"{'ok ' if rel <= 5e-3 and cos >= 0.99999 else 'BAD'} {k}: rel {rel:.2e} cos {cos:.6f}")
    print("\n".join(report))
    assert not [r for r in report if r.startswith("BAD")], "\n".join(report)
    assert grads["prop_mlp_0.encoder.embeddings"].abs().sum() > 0
    assert st["same_names"]   # state_dict() keeps the reference's parameter names


@pytest.mark.gpu
def test_reference_step_renderings_through_the_fused_object_operator():
    """`out_depth` / `out_rgb` of the same step within 2e-4 of the fixture.  The forward sums every Linear in the reference's order
    (one FMA chain from zero, bias last); measured on an MI355X: depth 8.6e-5, rgb 2.9e-5.  (With the chains started at the bias, as
    the inference kernel sums, one of the 64 rays was 3.6e-4 off: 2e-5 of a level-0 density moves a sample position of the next level.)"""
    st = _fused_step()
    g = st["g"]
    print("max |depth - reference|", float(np.abs(st["depth"] - g["out_depth"]).max()), "max |rgb - reference|", float(np.abs(st["rgb"] - g["out_rgb"]).max()))
    np.testing.assert_allclose(st["rgb"], g["out_rgb"], atol=2e-4, rtol=0)
    np.testing.assert_allclose(st["depth"], g["out_depth"], atol=2e-4, rtol=0)


@pytest.mark.gpu
def test_fused_object_step_reads_nothing_back():
    """A dynamic-object `training_step(as_tensors=True)` on `TrainableModel(fused_mlp=True, fused_objects=True)` runs under
    `torch.cuda.set_sync_debug_mode("error")` after one warm-up step; the same step with `fused_objects=False` raises there (the torch
    merge reads its owner lists back)."""
    from nerflidar_hip import training as ntrain
    g, mc, sd, class_names, lg, batch = _obj_step_scene()

    def step(fused_objects):
        tm = ntrain.TrainableModel(mc, fused_mlp=True, tracks=g["tracks"], class_names=class_names, obj_log2_hashmap=lg,
                                   fused_objects=fused_objects).cuda().load_reference(sd)
        opt = torch.optim.Adam(tm.parameters(), lr=1e-4, capturable=True)
        run = lambda: ntrain.training_step(tm, opt, batch, train_frac=float(g["train_frac"]), randomized=False, as_tensors=True)
        run()  # warm-up: plan, workspaces, the optimiser's state
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            return run()
        finally:
            torch.cuda.set_sync_debug_mode("default")

    out = step(True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out["loss"]))
    with pytest.raises(RuntimeError):
        step(False)


# ---- GPU: the operator on small scenes -------------------------------------------------------------------------------------------
from test_objects import OWNER_CASES, _owner_scene  # noqa: E402

# (N, S, n_obj, class of every track): the owner cases of tests/test_objects.py on two classes, a class that owns nothing (its only track
# is the one `_owner_scene` moves out of reach), and a class that owns more than one workgroup's first pass of 192 samples times the grid
# the launch takes for N * S samples, not a multiple of 64.
OP_CASES = [(N, S, n, [t % 2 for t in range(n)]) for N, S, n in OWNER_CASES] + [(37, 5, 3, [0, 0, 1]), (2047, 32, 2, [0, 0])]
BIG = 2047  # that case: boxes of 4 x 4 x 4 hold every sample, 65 504 = 1023.5 x 64 of them, above the 256 x 192 of the first pass


def _op_scene(N, S, n_obj, cls, seed=0, **cfg_kw):
    import dataclasses
    from nerflidar_hip import _lib, training as ntrain
    torch.manual_seed(100 + seed)
    cids = [13, 14][: max(cls) + 1]
    mlps = []
    for cid in cids:
        m = ntrain.TrainableObjMLP(dataclasses.replace(nconfig.obj_mlp_config(cid, latent_size=LAT, log2_hashmap=12), **cfg_kw))
        with torch.no_grad():
            m.encoder.embeddings.uniform_(-0.5, 0.5)   # white noise: both sides see the same owner map
        mlps.append(m.cuda())
    o, d, td, ts, tracks = _owner_scene(N, S, n_obj)
    if N == BIG:
        tracks[:, :, 4:7] = 4.0
    vd = F.normalize(d, dim=-1)
    latents = torch.randn(n_obj, LAT)
    box = nobj.track_box_params(torch.from_numpy(np.asarray(tracks, np.float32)).cuda(), ts.cuda())
    plan = ntrain._ObjTrainPlan(mlps, cls, LAT, "cuda")
    K = mlps[0].cfg.class_num
    gen = torch.Generator().manual_seed(7 + seed)
    stat = dict(density=torch.rand(N, S, generator=gen), rgb=torch.rand(N, S, 3, generator=gen), sem=torch.rand(N, S, K, generator=gen))
    cot = dict(density=torch.randn(N, S, generator=gen), rgb=torch.randn(N, S, 3, generator=gen))
    rays, keep = _lib.rays(dict(origins=o.cuda(), directions=d.cuda(), viewdirs=vd.cuda()), N, optional=_lib.RAY_KEYS)
    return dict(mlps=mlps, plan=plan, o=o, d=d, vd=vd, td=td, box=box, latents=latents, cls=cls, stat=stat, cot=cot, rays=rays, keep=keep, K=K)


def _fused(sc, want_grad=True):
    from nerflidar_hip import training as ntrain
    plan, mlps = sc["plan"], sc["mlps"]
    for m in mlps:
        m.zero_grad(set_to_none=True)
    flats = [plan.flat(c, m) for c, m in enumerate(mlps)]
    plan.pack([f.detach() for f in flats])
    lat = sc["latents"].cuda().requires_grad_(True)
    stat = {k: v.cuda().requires_grad_(True) for k, v in sc["stat"].items()}
    dens, rgb, sem, mask = ntrain._ObjectsFused.apply(plan, sc["rays"], sc["keep"], sc["td"].cuda(), sc["box"], stat["density"], stat["rgb"], stat["sem"],
                                                      lat, *[m.encoder.embeddings for m in mlps], *flats)
    out = dict(density=dens.detach().cpu(), rgb=rgb.detach().cpu(), sem=sem.detach().cpu(), mask=mask.cpu())
    if want_grad:
        ((dens * sc["cot"]["density"].cuda()).sum() + (rgb * sc["cot"]["rgb"].cuda()).sum() + sem.sum()).backward()
        out["grads"] = _grads(mlps, lat.grad.cpu())
        out["g_stat"] = {k: v.grad.cpu() for k, v in stat.items()}
    return out


def _grads(mlps, g_lat):
    out = {"latents": g_lat.double()}
    for c, m in enumerate(mlps):
        for k, p in m.named_parameters():
            out[f"class{c}.{k}"] = torch.zeros(p.shape, dtype=torch.float64) if p.grad is None else p.grad.detach().cpu().double()
    return out


def _merge(sc, mask_winner, f64):
    """The merge of `TrainableModel._object_merge` on the owner map `mask_winner`: `objects.box_frame` + `objects.obj_mlp_forward` per
    class + index writes.  f64 = False: the unfused f32 path on the device (`TrainableObjMLP`); True: the yardstick, float64 on the CPU
    with tests/grid_ref.py for the grid and double `F.linear` binders."""
    import grid_ref
    dt, dev = (torch.float64, "cpu") if f64 else (torch.float32, "cuda")
    mlps = sc["mlps"]
    for m in mlps:
        m.zero_grad(set_to_none=True)
    lat = sc["latents"].to(dev, dt).requires_grad_(True)
    winner = mask_winner.to(dev)
    sel = (winner >= 0).nonzero()
    ri, si = sel[:, 0], sel[:, 1]
    tr = winner[ri, si].long()
    cv = lambda t: t.to(dev, dt)
    p_all, d_all = nobj.box_frame(cv(sc["o"]), cv(sc["d"]), cv(sc["vd"]), cv(sc["td"]), cv(sc["box"].cpu()), ri, si, tr)
    dens, rgb, sem = (cv(sc["stat"][k]).clone() for k in ("density", "rgb", "sem"))
    rank = torch.tensor(sc["cls"], device=dev)[tr]
    params64 = []
    for c, m in enumerate(mlps):
        pick = (rank == c).nonzero()[:, 0]
        if f64:
            P = {k: p.detach().cpu().double().requires_grad_(True) for k, p in m.named_parameters()}
            params64.append(P)
            if pick.numel() == 0:
                continue
            enc = lambda x, bound=1, P=P, m=m: grid_ref._grid_lookup((x + 1) / 2, P["encoder.embeddings"], m.encoder).reshape(x.shape[0], -1)
            lin = lambda name, x, P=P: F.linear(x, P[name + ".weight"], P[name + ".bias"])
            res = nobj.obj_mlp_forward(m.cfg, enc, lin, p_all[pick], d_all[pick], lat[tr[pick]])
            res = {k: v.double() for k, v in res.items()}
        else:
            if pick.numel() == 0:
                continue
            res = m(p_all[pick], d_all[pick], lat[tr[pick]])
        dens[ri[pick], si[pick]] = res["density"]
        rgb[ri[pick], si[pick]] = res["rgb"]
        sem[ri[pick], si[pick]] = res["semantic"].to(dt)
    ((dens * cv(sc["cot"]["density"])).sum() + (rgb * cv(sc["cot"]["rgb"])).sum()).backward()
    out = dict(density=dens.detach().cpu(), rgb=rgb.detach().cpu(), sem=sem.detach().cpu())
    if f64:
        out["grads"] = {"latents": lat.grad}
        for c, P in enumerate(params64):
            out["grads"].update({f"class{c}.{k}": torch.zeros_like(p) if p.grad is None else p.grad for k, p in P.items()})
    else:
        out["grads"] = _grads(mlps, lat.grad.cpu())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("N,S,n_obj,cls", OP_CASES)
def test_operator_against_float64(N, S, n_obj, cls):
    """Values and every gradient of the operator against a float64 CPU restatement, per tensor as a fraction of the tensor's norm:
    (b) the fused operator may be at most 2 x (a) the unfused f32 path + 1e-6 away from it - what another summation order can cost.
    Conditions checked first: no sample within 1e-6 of a box face, every class that should own samples owns >= 10.  Forward values
    against `nlr_objects_apply` on an `NlrObjects` of the same weights (`_inference`) and against the unfused f32 path: owner map and
    semantic exact, density 3e-4 + 5e-5 |d|, rgb 2e-5."""
    _check_operator(N, S, n_obj, cls)


@pytest.mark.gpu
def test_operator_against_float64_with_the_skip_concatenation_inside_the_depth():
    """The same comparison on a view MLP of depth 3 whose layer 1 takes the concatenated input again (`skip_layer_dir` = 0): the
    shipped ObjMLP never concatenates (depth 2, skip 4), the envelope allows it."""
    _check_operator(37, 5, 4, [0, 1, 0, 1], net_depth_viewdirs=3, skip_layer_dir=0)


def _inference(sc):
    """`nlr_objects_apply` (header section 7b) on an `NlrObjects` made of the same Linears, tables and latent codes, on the same rays,
    tdist and box constants: merged density [N,S], rgb [N,S,3], semantic [N,S,K] and the owner map."""
    from nerflidar_hip import _lib, training as ntrain
    od, keep = ntrain.objects_desc(sc["mlps"], sc["cls"], LAT, weights=True, latents=sc["latents"])
    objs = C.c_void_p(None)
    _lib.call("nlr_objects_create", od, objs, device="cuda")
    try:
        td = sc["td"].cuda()
        N, S = td.shape[0], td.shape[1] - 1
        dens = sc["stat"]["density"].cuda().clone()
        rgb, sem = (sc["stat"][k].cuda().permute(2, 0, 1).clone(memory_format=torch.contiguous_format) for k in ("rgb", "sem"))
        win = torch.full((N, S), -7, dtype=torch.int32, device="cuda")
        ws = torch.empty(int(_lib.lib().nlr_objects_workspace_bytes(objs, N, S)), dtype=torch.uint8, device="cuda")
        _lib.call("nlr_objects_apply", objs, sc["rays"], td, sc["box"], N, S, sc["box"].shape[1], dens, rgb, sem, sem.shape[0], win, ws, ws.numel())
        torch.cuda.synchronize()
        return dict(density=dens.cpu(), rgb=rgb.permute(1, 2, 0).cpu(), sem=sem.permute(1, 2, 0).cpu(), winner=win.cpu())
    finally:
        _lib.lib().nlr_objects_destroy(objs)


def _check_operator(N, S, n_obj, cls, **cfg_kw):
    from test_objects import _owner_reference
    sc = _op_scene(N, S, n_obj, cls, **cfg_kw)
    want, x = _owner_reference(sc["o"], sc["d"], sc["td"], sc["box"].cpu())
    assert float((x.abs() - 1.0).abs().min()) > 1e-6
    got = _fused(sc)
    assert torch.equal(got["mask"], want >= 0)
    owned = [int(((want >= 0) & (torch.tensor(cls)[want.clamp_min(0).long()] == c)).sum()) for c in range(max(cls) + 1)]
    print(f"case {(N, S, n_obj, cls)}: owned per class {owned}")
    if (N, S, n_obj) != OWNER_CASES[0]:   # `want` is the CPU's owner map: a class it gives samples owns at least 10, and some class does
        assert sum(owned) >= 10 and all(k == 0 or k >= 10 for k in owned), owned
    else:   # 3 rays x 2 samples, kept for the one-box tail of the owner kernel: it cannot own 10, it must own something
        assert sum(owned) >= 1, owned
    if cls == [0, 0, 1]:
        assert owned[1] == 0 and owned[0] >= 10, owned   # the class whose only track is out of reach
    if N == BIG:
        assert owned[0] % 64 != 0 and owned[0] > 192 * min(256, (N * S + 191) // 192), owned
    f32 = _merge(sc, want, False)
    f64 = _merge(sc, want, True)
    m = want >= 0
    # forward values against `nlr_objects_apply` on the same weights (the training forward sums its Linears in another order): owner
    # map and semantic exact, density 3e-4 + 5e-5 |d|, rgb 2e-5 - everywhere, so the unowned samples are compared too
    inf = _inference(sc)
    assert torch.equal(inf["winner"], want) and torch.equal(got["mask"], inf["winner"] >= 0)
    di = (got["density"] - inf["density"]).abs()
    print(f"against nlr_objects_apply: density max diff {float(di.max()):.3e} (max density {float(inf['density'][m].abs().max()) if m.any() else 0:.3e}), "
          f"rgb max diff {float((got['rgb'] - inf['rgb']).abs().max()):.3e}")
    assert bool((di <= 3e-4 + 5e-5 * inf["density"].abs()).all()), float(di.max())
    assert float((got["rgb"] - inf["rgb"]).abs().max()) <= 2e-5
    assert torch.equal(got["sem"], inf["sem"])
    # and against the unfused f32 path, the same bounds (those of test_device_side_object_branch_matches_the_torch_stage_loop)
    dd = (got["density"][m] - f32["density"][m]).abs()
    assert bool((dd <= 3e-4 + 5e-5 * f32["density"][m].abs()).all()), float(dd.max())
    assert float((got["rgb"][m] - f32["rgb"][m]).abs().max() if m.any() else 0.0) <= 2e-5
    assert torch.equal(got["sem"][m], f32["sem"][m])
    for k in ("density", "rgb", "sem"):   # outside the boxes the static tensors come back unchanged, with their gradient
        assert torch.equal(got[k][~m], sc["stat"][k][~m])
    assert torch.equal(got["g_stat"]["density"], torch.where(m, torch.zeros(()), sc["cot"]["density"]))
    assert torch.equal(got["g_stat"]["rgb"], torch.where(m[..., None], torch.zeros(()), sc["cot"]["rgb"]))
    lines, bad = [], []
    tensors = [("density", got["density"].double(), f32["density"].double(), f64["density"]), ("rgb", got["rgb"].double(), f32["rgb"].double(), f64["rgb"])]
    tensors += [(k, got["grads"][k], f32["grads"][k], f64["grads"][k]) for k in f64["grads"]]
    for k, b_, a_, ref in tensors:
        nrm = float(ref.norm())
        if nrm == 0.0:
            assert float(b_.abs().max()) == 0.0, k   # (a class or track that owns nothing: exact zeros)
            continue
        ea, eb = float((a_ - ref).norm()) / nrm, float((b_ - ref).norm()) / nrm
        lines.append(f"{(N, S, n_obj)} {k}: unfused {ea:.3e} fused {eb:.3e}")
        if not eb <= 2 * ea + 1e-6:
            bad.append(lines[-1])
    print("\n".join(lines))
    out = os.environ.get("NLR_OBJ_TRAIN_ACCURACY")   # a file to append the table to: how profiles/obj_train_accuracy.txt is made
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")
    assert not bad, "\n".join(bad)
    # a track without owned samples: an exact zero row
    for t in range(n_obj):
        if not bool((want == t).any()):
            assert float(got["grads"]["latents"][t].abs().max()) == 0.0


@pytest.mark.gpu
def test_backward_is_repeatable_and_misses_are_a_no_op():
    """Two backward passes on the same inputs give the same bits in the parameter and latent gradients.  Rays that miss every box:
    the static tensors come back unchanged, the gradients are exact zeros, the table gradient is untouched."""
    sc = _op_scene(130, 7, 9, [t % 2 for t in range(9)])
    a, b = _fused(sc), _fused(sc)
    for k in a["grads"]:
        if not k.endswith("encoder.embeddings"):
            assert torch.equal(a["grads"][k], b["grads"][k]), k
    assert float(a["grads"]["class0.density_layer.0.weight"].abs().max()) > 0
    sc["box"][..., 2:5] += 100.0   # every box out of every ray's reach
    miss = _fused(sc)
    assert not bool(miss["mask"].any())
    for k in ("density", "rgb", "sem"):
        assert torch.equal(miss[k], sc["stat"][k])
    for k, v in miss["grads"].items():
        assert float(v.abs().max()) == 0.0, k


@pytest.mark.gpu
def test_abi_refusals_launch_nothing():
    """Every refusal of section 7e returns its status with a message; outputs pre-filled with a sentinel stay filled.  n_obj = 0, N = 0
    and S = 0 return NLR_OK from both entry points and touch nothing."""
    from nerflidar_hip import _lib
    sc = _op_scene(37, 5, 3, [0, 1, 0])
    plan, L = sc["plan"], _lib.lib()
    N, S, n_obj = 37, 5, 3
    dev = "cuda"
    td, box = sc["td"].cuda(), sc["box"]
    tabs = [m.encoder.embeddings.detach() for m in sc["mlps"]]
    lat = sc["latents"].cuda()
    tp = lambda ts: (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
    sent = -7.0
    dens, rgb = torch.full((N, S), sent, device=dev), torch.full((3, N, S), sent, device=dev)
    win = torch.full((N, S), -7, dtype=torch.int32, device=dev)
    need = int(L.nlr_obj_train_workspace_bytes(plan.handle, N, S, 1))
    assert need > int(L.nlr_obj_train_workspace_bytes(plan.handle, N, S, 0)) > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    d_par = [torch.full((k,), sent, device=dev) for k in plan.n_params]
    d_lat, g_tab = torch.full((n_obj, LAT), sent, device=dev), [torch.zeros_like(t) for t in tabs]
    gd, gr = torch.zeros(N, S, device=dev), torch.zeros(3, N, S, device=dev)
    p = _lib.ptr

    def fwd(plan_h=plan.handle, tables=tabs, latents=lat, rays=sc["rays"], tdist=td, bx=box, n=N, s=S, no=n_obj, density=dens, winner=win, wsb=need):
        return L.nlr_obj_train_forward(plan_h, None if tables is None else tp(tables), p(latents), None if rays is None else C.byref(rays), p(tdist),
                                       bx if isinstance(bx, int) else p(bx), n, s, no, p(density), p(rgb), None, 0, p(winner), p(ws), wsb, None)

    def bwd(g_density=gd, g_rgb=gr, dp=d_par, dl=d_lat, gt=g_tab, no=n_obj, wsb=need, bx=box, n=N, s=S):
        return L.nlr_obj_train_backward(plan.handle, tp(tabs), p(lat), C.byref(sc["rays"]), p(td), bx if isinstance(bx, int) else p(bx), n, s, no,
                                        p(g_density), p(g_rgb), None if dp is None else tp(dp), p(dl), None if gt is None else tp(gt), p(ws), wsb, None)

    msg = lambda: L.nlr_last_error().decode()
    for f, kw, word in [(fwd, dict(plan_h=None), "plan"), (fwd, dict(tables=None), "tables"), (fwd, dict(tables=[tabs[0], None]), "tables[1]"),
                        (fwd, dict(latents=None), "latents"), (fwd, dict(rays=None), "rays"), (fwd, dict(tdist=None), "tdist"),
                        (fwd, dict(bx=None), "box_params"), (fwd, dict(density=None), "density"), (fwd, dict(winner=None), "winner"),
                        (fwd, dict(no=2), "n_obj"), (fwd, dict(bx=box.data_ptr() + 4), "16-byte"),
                        (bwd, dict(g_density=None), "g_density"), (bwd, dict(g_rgb=None), "g_rgb"), (bwd, dict(dp=None), "d_params"),
                        (bwd, dict(dp=[d_par[0], None]), "d_params[1]"), (bwd, dict(dl=None), "d_latents"), (bwd, dict(gt=None), "grad_tables"),
                        (bwd, dict(no=4), "n_obj"), (bwd, dict(bx=box.data_ptr() + 4), "16-byte")]:
        rc = f(**kw)
        assert rc == -1 and word in msg(), (rc, word, msg())
    assert fwd(wsb=16) == -4 and "workspace" in msg()           # the forward alone takes the backward = 0 size ...
    assert bwd(wsb=int(L.nlr_obj_train_workspace_bytes(plan.handle, N, S, 0))) == -4 and "workspace" in msg()   # ... the backward does not
    big = 1 << 16
    assert fwd(n=big, s=big) == -1 and "32-bit" in msg()
    for kw in (dict(no=0), dict(n=0), dict(s=0)):   # the no-op of the pair: forward and backward
        assert fwd(**kw) == 0 and bwd(**kw) == 0
    torch.cuda.synchronize()
    for t in [dens, rgb, d_lat] + d_par:
        assert bool((t == sent).all())
    assert bool((win == -7).all()) and all(float(t.abs().max()) == 0.0 for t in g_tab)


@pytest.mark.gpu
def test_fused_objects_refuses_track_and_pose_refinement():
    """`fused_objects=True` with a track that requires a gradient, and with `object_ray_grads=True` on rays that require one: the
    box-frame cotangents are not wired on this path - NotImplementedError naming the argument."""
    from nerflidar_hip import training as ntrain
    g, mc, sd, class_names, lg, batch = _obj_step_scene()
    tm = ntrain.TrainableModel(mc, tracks=g["tracks"], class_names=class_names, obj_log2_hashmap=lg, fused_objects=True).cuda().load_reference(sd)
    track = torch.from_numpy(np.asarray(g["tracks"], np.float32)).cuda().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="fused_objects"):
        tm(batch, train_frac=float(g["train_frac"]), curr_track=track)
    rb = dict(batch, origins=batch["origins"].clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="fused_objects"):
        tm(rb, train_frac=float(g["train_frac"]), object_ray_grads=True)
