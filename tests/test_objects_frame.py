"""Box-frame cotangents of the fused object operator (header section 7e: `nlr_obj_train_backward_frame`, `training._ObjectsFused` with
the frame tensors, `TrainableModel(fused_objects=True, fused_object_frame=True)`): the operator against a float64 restatement next to
the unfused f32 path, repeatability, the ABI's refusals, the dense list through `nlr_obj_frame_backward` / `_rays`, the reference's
track- and pose-refinement steps through the fused path, no host read in a refinement step, the opt-in."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from nerflidar_hip import objects as nobj

from test_objects import OWNER_CASES, _owner_reference, _owner_scene
from test_objects_train import LAT, OP_CASES, _op_scene

FACE = 4e-6    # samples whose float64 unit-cube coordinate lies this close to a cell face (any level, any axis) are left out of g_pts
CANARY = 7.0
NAMES = {13: "vehicle.car", 14: "vehicle.truck", 15: "vehicle.bus.rigid", 11: "human.pedestrian.adult"}


# ---- the operator through the ABI -------------------------------------------------------------------------------------------------
def _frame_call(sc, pts=True, dirs=True, frame=True):
    """`nlr_obj_train_forward` (rgb form, backward workspace) and then `nlr_obj_train_backward_frame` (frame = False:
    `nlr_obj_train_backward`) on the scene of `_op_scene`, with the scene's cotangents of density and rgb.  g_pts / g_dirs are
    pre-filled with CANARY; an output that is not wanted is passed as NULL."""
    from nerflidar_hip import _lib, training as ntrain
    plan, mlps = sc["plan"], sc["mlps"]
    plan.pack([plan.flat(c, m).detach() for c, m in enumerate(mlps)])
    td, box = sc["td"].cuda(), sc["box"]
    N, S, n_obj = td.shape[0], td.shape[1] - 1, box.shape[1]
    tabs = [m.encoder.embeddings.detach() for m in mlps]
    lat = sc["latents"].cuda()
    cf = torch.contiguous_format
    ws = torch.empty(int(_lib.lib().nlr_obj_train_workspace_bytes(plan.handle, N, S, 1)), dtype=torch.uint8, device="cuda")
    dens = sc["stat"]["density"].cuda().clone()
    rgb = sc["stat"]["rgb"].cuda().permute(2, 0, 1).clone(memory_format=cf)
    winner = ntrain.objects_forward(plan, tabs, lat, sc["rays"], td, box, dens, rgb, None, workspace=ws)
    gd = sc["cot"]["density"].cuda().contiguous()
    gr = sc["cot"]["rgb"].cuda().permute(2, 0, 1).clone(memory_format=cf)
    d_flats = [torch.full((k,), CANARY, device="cuda") for k in plan.n_params]
    d_lat = torch.full_like(lat, CANARY)
    g_tabs = [torch.zeros_like(t) for t in tabs]
    g_pts = torch.full((N * S, 3), CANARY, device="cuda") if pts else None
    g_dirs = torch.full((N * S, 3), CANARY, device="cuda") if dirs else None
    head = (plan.handle, ntrain._ptr_array(tabs), lat, sc["rays"], td, box, N, S, n_obj, gd, gr, ntrain._ptr_array(d_flats), d_lat,
            ntrain._ptr_array(g_tabs))
    if frame:
        _lib.call("nlr_obj_train_backward_frame", *head, g_pts, g_dirs, ws, ws.numel())
    else:
        _lib.call("nlr_obj_train_backward", *head, ws, ws.numel())
    torch.cuda.synchronize()
    return dict(winner=winner.cpu(), g_pts=None if g_pts is None else g_pts.cpu(), g_dirs=None if g_dirs is None else g_dirs.cpu(),
                d_flats=[t.cpu() for t in d_flats], d_lat=d_lat.cpu())


def _merge_frame(sc, winner, f64):
    """`_merge` of tests/test_objects_train.py with the box-frame points and directions as LEAVES: -> (d loss / d p_all, d loss / d d_all
    [K, 3] in (ray, sample) order, p_all, ri, si).  f64 = True: the yardstick, float64 on the CPU with tests/grid_ref.py for the grid;
    False: the unfused f32 path on the device (`TrainableObjMLP`, the HIP grid operator's input gradient)."""
    import grid_ref
    dt, dev = (torch.float64, "cpu") if f64 else (torch.float32, "cuda")
    mlps = sc["mlps"]
    for m in mlps:
        m.zero_grad(set_to_none=True)
    lat = sc["latents"].to(dev, dt)
    winner = winner.to(dev)
    sel = (winner >= 0).nonzero()
    ri, si = sel[:, 0], sel[:, 1]
    tr = winner[ri, si].long()
    cv = lambda t: t.to(dev, dt)
    p_all, d_all = nobj.box_frame(cv(sc["o"]), cv(sc["d"]), cv(sc["vd"]), cv(sc["td"]), cv(sc["box"].cpu()), ri, si, tr)
    p_all, d_all = p_all.detach().requires_grad_(True), d_all.detach().requires_grad_(True)
    dens, rgb = (cv(sc["stat"][k]).clone() for k in ("density", "rgb"))
    rank = torch.tensor(sc["cls"], device=dev)[tr]
    for c, m in enumerate(mlps):
        pick = (rank == c).nonzero()[:, 0]
        if pick.numel() == 0:
            continue
        if f64:
            P = {k: p.detach().cpu().double() for k, p in m.named_parameters()}
            enc = lambda x, bound=1, P=P, m=m: grid_ref._grid_lookup((x + 1) / 2, P["encoder.embeddings"], m.encoder).reshape(x.shape[0], -1)
            lin = lambda name, x, P=P: F.linear(x, P[name + ".weight"], P[name + ".bias"])
            res = nobj.obj_mlp_forward(m.cfg, enc, lin, p_all[pick], d_all[pick], lat[tr[pick]])
        else:
            res = m(p_all[pick], d_all[pick], lat[tr[pick]])
        dens[ri[pick], si[pick]] = res["density"].to(dt)
        rgb[ri[pick], si[pick]] = res["rgb"].to(dt)
    if ri.numel():
        ((dens * cv(sc["cot"]["density"])).sum() + (rgb * cv(sc["cot"]["rgb"])).sum()).backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return zero(p_all).detach().cpu().double(), zero(d_all).detach().cpu().double(), p_all.detach().cpu().double(), ri.cpu(), si.cpu()


def _near_face(p64, encoder):
    """[K] bool: some coordinate of (p + 1) / 2 lies within FACE of a cell face on some level (FACE * scale_l in cell units)."""
    import grid_ref
    x01 = (p64 + 1) / 2
    near = torch.zeros(p64.shape[0], dtype=torch.bool)
    for scale, *_ in grid_ref._level_table(encoder):
        pos = x01 * scale + (0.0 if encoder.align_corners else 0.5)
        near |= ((pos - torch.round(pos)).abs() < FACE * scale).any(-1)
    return near


def _check_frame(N, S, n_obj, cls, **cfg_kw):
    sc = _op_scene(N, S, n_obj, cls, **cfg_kw)
    want, x = _owner_reference(sc["o"], sc["d"], sc["td"], sc["box"].cpu())
    assert float((x.abs() - 1.0).abs().min()) > 1e-6
    both = _frame_call(sc)
    assert torch.equal(both["winner"], want)
    owned = want >= 0
    g_pts, g_dirs = both["g_pts"].reshape(N, S, 3), both["g_dirs"].reshape(N, S, 3)
    # rows of unowned samples: exact zeros (every row is overwritten: the canary is gone)
    assert float(g_pts[~owned].abs().max() if (~owned).any() else 0.0) == 0.0 and float(g_dirs[~owned].abs().max() if (~owned).any() else 0.0) == 0.0
    assert not bool((g_pts == CANARY).any()) and not bool((g_dirs == CANARY).any())
    # against float64, next to the unfused f32 path
    rp, rd, p64, ri, si = _merge_frame(sc, want, True)
    ap, ad, _, ri32, si32 = _merge_frame(sc, want, False)
    assert torch.equal(ri, ri32) and torch.equal(si, si32)
    near = _near_face(p64, sc["mlps"][0].encoder)
    K, kept = int(ri.numel()), int((~near).sum())
    share = 1.0 - kept / K
    print(f"case {(N, S, n_obj, cls)} {cfg_kw}: {K} owned samples, {K - kept} within {FACE:g} of a cell face ({100 * share:.2f} %), {kept} kept")
    assert share <= 0.10 and kept >= (1 if (N, S, n_obj) == OWNER_CASES[0] else 10), (K, kept)
    bp, bd = g_pts[ri, si].double(), g_dirs[ri, si].double()
    lines, bad = [], []
    for name, b_, a_, ref in (("g_pts", bp[~near], ap[~near], rp[~near]), ("g_dirs", bd, ad, rd)):
        nrm = float(ref.norm())
        assert nrm > 0.0, name
        ea, eb = float((a_ - ref).norm()) / nrm, float((b_ - ref).norm()) / nrm
        lines.append(f"{(N, S, n_obj)} {cfg_kw or ''} {name}: unfused {ea:.3e} fused {eb:.3e}")
        if not eb <= 2 * ea + 1e-6:
            bad.append(lines[-1])
    print("\n".join(lines))
    import os
    out = os.environ.get("NLR_OBJ_FRAME_ACCURACY")   # a file to append the table to: how profiles/obj_frame_accuracy.txt is made
    if out:
        with open(out, "a") as f:
            f.write(f"{(N, S, n_obj)} {cfg_kw or ''}: {K} owned, {K - kept} left out of g_pts ({100 * share:.2f} %)\n" + "\n".join(lines) + "\n")
    assert not bad, "\n".join(bad)
    # the parameter and latent gradients are those of nlr_obj_train_backward, whatever is requested; an output does not depend on the other
    plain, only_p, only_d = _frame_call(sc, frame=False), _frame_call(sc, dirs=False), _frame_call(sc, pts=False)
    for other in (both, only_p, only_d):
        assert torch.equal(other["d_lat"], plain["d_lat"])
        assert all(torch.equal(u, v) for u, v in zip(other["d_flats"], plain["d_flats"]))
    assert not bool((plain["d_lat"] == CANARY).any())
    assert only_p["g_dirs"] is None and only_d["g_pts"] is None
    assert torch.equal(only_p["g_pts"], both["g_pts"]) and torch.equal(only_d["g_dirs"], both["g_dirs"])


@pytest.mark.gpu
@pytest.mark.parametrize("N,S,n_obj,cls", OP_CASES)
def test_frame_cotangents_against_float64(N, S, n_obj, cls):
    """g_pts / g_dirs of `nlr_obj_train_backward_frame` against float64 autograd of the merge with the box-frame points and directions
    as leaves, per tensor as a fraction of the yardstick's norm: the fused deviation is at most 2 x that of the unfused f32 path + 1e-6,
    the gate of test_operator_against_float64.  The trilinear derivative jumps at cell faces, and the three computations place a point
    within rounding of a face in different cells: samples whose float64 unit-cube coordinate lies within 4e-6 of a face (any level, any
    axis; 2.7 x the f32 error of (po + 1) / 2) are left out of g_pts, at most 10 % of a case with at least 10 kept (3 x 2: at least 1).
    Rows of unowned samples are exact zeros.  d_params / d_latents keep the bits of `nlr_obj_train_backward` with both, one or no
    frame output, and each output keeps its bits without the other."""
    _check_frame(N, S, n_obj, cls)


@pytest.mark.gpu
def test_frame_cotangents_with_two_view_layers_on_the_encoding():
    """Depth 3 with `skip_layer_dir` = 0: view layers 0 and 1 both take the direction encoding."""
    _check_frame(37, 5, 4, [0, 1, 0, 1], net_depth_viewdirs=3, skip_layer_dir=0)


@pytest.mark.gpu
def test_frame_cotangents_with_the_rgb_layer_on_the_encoding():
    """Depth 2 with `skip_layer_dir` = 1: view layer 0 and `rgb_layer` take the direction encoding."""
    _check_frame(37, 5, 4, [0, 1, 0, 1], net_depth_viewdirs=2, skip_layer_dir=1)


@pytest.mark.gpu
def test_frame_cotangents_are_repeatable_and_misses_give_zeros():
    """Two calls on 130 x 7 with 9 tracks give the same bits in g_pts and g_dirs; rays that miss every box give all-zero buffers."""
    sc = _op_scene(130, 7, 9, [t % 2 for t in range(9)])
    a, b = _frame_call(sc), _frame_call(sc)
    assert torch.equal(a["g_pts"], b["g_pts"]) and torch.equal(a["g_dirs"], b["g_dirs"])
    assert float(a["g_pts"].abs().max()) > 0 and float(a["g_dirs"].abs().max()) > 0
    sc["box"][..., 2:5] += 100.0   # every box out of every ray's reach
    miss = _frame_call(sc)
    assert not bool((miss["winner"] >= 0).any())
    assert float(miss["g_pts"].abs().max()) == 0.0 and float(miss["g_dirs"].abs().max()) == 0.0


@pytest.mark.gpu
def test_frame_entry_refuses_what_the_backward_refuses():
    """Every refusal of `nlr_obj_train_backward` from the new entry point, with nothing launched: canary-filled g_pts / g_dirs and
    parameter gradients come back untouched.  N = 0, S = 0 and n_obj = 0 return NLR_OK and touch nothing."""
    from nerflidar_hip import _lib
    sc = _op_scene(37, 5, 3, [0, 1, 0])
    plan, L = sc["plan"], _lib.lib()
    N, S, n_obj = 37, 5, 3
    dev = "cuda"
    td, box = sc["td"].cuda(), sc["box"]
    tabs = [m.encoder.embeddings.detach() for m in sc["mlps"]]
    lat = sc["latents"].cuda()
    tp = lambda ts: (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
    need = int(L.nlr_obj_train_workspace_bytes(plan.handle, N, S, 1))
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    d_par = [torch.full((k,), CANARY, device=dev) for k in plan.n_params]
    d_lat, g_tab = torch.full((n_obj, LAT), CANARY, device=dev), [torch.zeros_like(t) for t in tabs]
    gd, gr = torch.zeros(N, S, device=dev), torch.zeros(3, N, S, device=dev)
    g_pts, g_dirs = torch.full((N * S, 3), CANARY, device=dev), torch.full((N * S, 3), CANARY, device=dev)
    p = _lib.ptr

    def bwd(plan_h=plan.handle, tables=tabs, latents=lat, rays=sc["rays"], tdist=td, g_density=gd, g_rgb=gr, dp=d_par, dl=d_lat, gt=g_tab,
            no=n_obj, wsb=need, bx=box, n=N, s=S):
        return L.nlr_obj_train_backward_frame(plan_h, None if tables is None else tp(tables), p(latents), None if rays is None else C.byref(rays),
                                              p(tdist), bx if isinstance(bx, int) else p(bx), n, s, no, p(g_density), p(g_rgb),
                                              None if dp is None else tp(dp), p(dl), None if gt is None else tp(gt), p(g_pts), p(g_dirs), p(ws),
                                              wsb, None)

    msg = lambda: L.nlr_last_error().decode()
    for kw, word in [(dict(plan_h=None), "plan"), (dict(tables=None), "tables"), (dict(tables=[tabs[0], None]), "tables[1]"),
                     (dict(latents=None), "latents"), (dict(rays=None), "rays"), (dict(tdist=None), "tdist"), (dict(bx=None), "box_params"),
                     (dict(g_density=None), "g_density"), (dict(g_rgb=None), "g_rgb"), (dict(dp=None), "d_params"),
                     (dict(dp=[d_par[0], None]), "d_params[1]"), (dict(dl=None), "d_latents"), (dict(gt=None), "grad_tables"),
                     (dict(gt=[g_tab[0], None]), "grad_tables[1]"), (dict(no=4), "n_obj"), (dict(bx=box.data_ptr() + 4), "16-byte")]:
        rc = bwd(**kw)
        assert rc == -1 and word in msg() and "obj_train_backward_frame" in msg(), (rc, word, msg())
    assert bwd(wsb=int(L.nlr_obj_train_workspace_bytes(plan.handle, N, S, 0))) == -4 and "workspace" in msg()
    big = 1 << 16
    assert bwd(n=big, s=big) == -1 and "32-bit" in msg()
    for kw in (dict(no=0), dict(n=0), dict(s=0)):
        assert bwd(**kw) == 0
    torch.cuda.synchronize()
    for t in [g_pts, g_dirs, d_lat] + d_par:
        assert bool((t == CANARY).all())
    assert all(float(t.abs().max()) == 0.0 for t in g_tab)


# ---- the dense list through 7c / 7d ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_dense_list_gives_what_the_compact_list_gives():
    """`obj_frame_backward` and `obj_frame_backward_rays` on the 37 x 5 x 4 case with the dense list of section 7e (K = N * S, track -1
    and zero cotangents at unowned samples) against the compact sorted list of the owned samples with the same cotangents: the track
    gradient to 2e-5 of each column's maximum (the gate of test_obj_frame_backward_matches_float64_autograd).
    The ray gradients: an entry with track -1 adds nothing, and a row with one or two owned samples has the same bits from both lists.
    A row with three or more does NOT, although no term differs: `nlr_obj_frame_bwd_rays_kernel` gives lane r of the ray's 16 the
    entries r, r + 16, .. of the ray's stretch of the list and adds the lanes by a butterfly.  In the dense list an owned sample sits
    at its sample index, in the compact one at its rank among the ray's owned samples, so the same terms are paired in another order
    (measured on an MI355X: 3.8e-6 on entries of 1e2, half an ulp).  For those rows the two results are two orderings of one f32 sum
    of n <= S terms, each within (n - 1) u sum |term| of the exact sum, u = 2^-24: they may differ by 2 (S - 1) u sum |term|, with the
    terms themselves taken from the kernel (one call per sample index)."""
    from nerflidar_hip import training as ntrain
    N, S, n_obj = 37, 5, 4
    sc = _op_scene(N, S, n_obj, [0, 1, 0, 1])
    _, _, _, ts, tracks = _owner_scene(N, S, n_obj)   # (the scene `_op_scene` was made of)
    tracks = torch.from_numpy(np.asarray(tracks, np.float32)).cuda()
    ts = ts.reshape(-1).cuda().contiguous()
    got = _frame_call(sc)
    winner = got["winner"].cuda()
    g_pts, g_dirs = got["g_pts"].cuda(), got["g_dirs"].cuda()
    o, d, vd, td = (sc[k].cuda().contiguous() for k in ("o", "d", "vd", "td"))
    ri_d, si_d = ntrain._dense_sample_index(N, S, "cuda")
    assert torch.equal(ri_d.cpu().long(), torch.arange(N * S) // S) and torch.equal(si_d.cpu().long(), torch.arange(N * S) % S)
    dense = (ri_d, si_d, winner.reshape(-1).contiguous(), g_pts, g_dirs)
    sel = (winner >= 0).nonzero()
    ri, si = sel[:, 0], sel[:, 1]
    assert 10 <= ri.numel() < N * S
    compact = (ri.int().contiguous(), si.int().contiguous(), winner[ri, si].contiguous(), g_pts.reshape(N, S, 3)[ri, si].contiguous(),
               g_dirs.reshape(N, S, 3)[ri, si].contiguous())
    t_dense, t_comp = (ntrain.obj_frame_backward(tracks, ts, o, d, vd, td, *lst).cpu().double() for lst in (dense, compact))
    assert float(t_comp.abs().max()) > 0
    for c in range(9):
        scale, err = float(t_comp[..., c].abs().max()), float((t_dense[..., c] - t_comp[..., c]).abs().max())
        print(f"track column {c}: dense against compact {err:.2e}, largest entry {scale:.2e}")
        assert err <= 2e-5 * scale, (c, err, scale)
    r_dense, r_comp = (ntrain.obj_frame_backward_rays(sc["box"], vd, td, *lst) for lst in (dense, compact))
    # the single terms of every row: one call per sample index k with the owned samples of that index (at most one per ray: the row is
    # that term plus zeros, exactly) -> the sum of their magnitudes, in float64
    mag = [torch.zeros(N, 3, dtype=torch.float64) for _ in range(3)]
    for k in range(S):
        pick = (si == k).nonzero()[:, 0]
        if pick.numel():
            for m_, t_ in zip(mag, ntrain.obj_frame_backward_rays(sc["box"], vd, td, *[t[pick].contiguous() for t in compact])):
                m_ += t_.cpu().double().abs()
    per_ray = torch.bincount(ri.cpu(), minlength=N)
    assert int((per_ray > 2).sum()) > 0 and int(((per_ray > 0) & (per_ray <= 2)).sum()) > 0   # both kinds of row occur
    for name, a, b, m_ in zip(("d_origins", "d_directions", "d_viewdirs"), r_dense, r_comp, mag):
        a, b = a.cpu(), b.cpu()
        diff = (a.double() - b.double()).abs()
        print(f"{name}: dense against compact {float(diff.max()):.2e}, largest entry {float(b.abs().max()):.2e}, "
              f"{int((diff > 0).any(-1).sum())} of {int((per_ray > 2).sum())} rows with three or more owned samples differ")
        assert float(b.abs().max()) > 0
        few = per_ray <= 2
        assert torch.equal(a[few], b[few]), name
        assert bool((diff <= 2 * (S - 1) * 2.0 ** -24 * 1.01 * m_).all()), (name, float(diff.max()))


# ---- through the model ----------------------------------------------------------------------------------------------------------------
def _fused_twin(tm, g, fused_mlp=False):
    """`tm` (a TrainableModel of a fixture's scene) again with the fused object operator and its box-frame gradient, same parameters."""
    from nerflidar_hip import training as ntrain
    class_names = [NAMES[int(c)] for c in g["class_ids"]]
    twin = ntrain.TrainableModel(tm.mc, fused_mlp=fused_mlp, tracks=g["tracks"], class_names=class_names, obj_log2_hashmap=int(g["log2_hashmap"]),
                                 fused_objects=True, fused_object_frame=True).cuda()
    twin.load_state_dict(tm.state_dict())
    return twin


def _rel_cos(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).norm() / want.norm()), float((got * want).sum() / (got.norm() * want.norm()))


@pytest.mark.gpu
def test_track_refinement_step_through_the_fused_object_operator():
    """The reference's track-refinement step (fixture train_step_TRACK) on `TrainableModel(fused_mlp=False, fused_objects=True,
    fused_object_frame=True)`, the gates of test_track_refinement_step_matches_the_reference_step: owner maps exact, loss terms and
    total 2e-4, depth 2e-4, `opt_r.grad` / `opt_t.grad` within 5e-3 of their norm with cosine >= 0.99999, as a whole and per track.
    The unfused path's figures are printed next to them."""
    from nerflidar_hip import losses as nl, training as ntrain
    from test_track_refine import _track_scene
    g = golden("train_step_TRACK")
    plain, batch = _track_scene(g)
    fused = _fused_twin(plain, g)

    def step(tm):
        tn = ntrain.TrackNet(g["tracks"]).cuda()
        with torch.no_grad():
            tn.opt_r.copy_(torch.from_numpy(g["opt_r"]))
            tn.opt_t.copy_(torch.from_numpy(g["opt_t"]))
        rend, hist = tm(batch, train_frac=float(g["train_frac"]), randomized=False, curr_track=tn())
        terms = nl.total_loss(rend, hist, batch, depth_lam=0.1, sem_lam=0.01)
        terms["latent_reg"] = tm.latent_reg(float(g["latent_reg"]))
        loss = sum(terms.values())
        loss.backward()
        ntrain.clip_gradients(tm)
        ntrain.clip_gradients(tn)
        return rend, hist, terms, loss, tn

    rend, hist, terms, loss, tn = step(fused)
    _, _, _, _, tn_plain = step(plain)
    for lvl, h in enumerate(hist):
        assert torch.equal(h["obj_mask"].cpu(), torch.from_numpy(g[f"hist{lvl}_obj_mask"])), f"owner map of level {lvl}"
    assert set(terms) == {k[5:] for k in g if k.startswith("loss_")}
    for k, v in terms.items():
        np.testing.assert_allclose(float(v.detach()), float(g["loss_" + k]), rtol=2e-4, atol=1e-7, err_msg=k)
    np.testing.assert_allclose(float(loss.detach()), float(g["loss"]), rtol=2e-4)
    np.testing.assert_allclose(rend[-1]["depth"].detach().cpu().numpy(), g["out_depth"], atol=2e-4, rtol=0)
    report = []
    for k in ("opt_r", "opt_t"):
        got, ref, want = getattr(tn, k).grad, getattr(tn_plain, k).grad, torch.from_numpy(g["grad_" + k])
        assert got is not None, f"{k}.grad is None: no gradient reached the tracks"
        rows = [(k, got, ref, want)] + [(f"{k}[track {t}]", got[t], ref[t], want[t]) for t in range(want.shape[0])]
        for name, a, b, w in rows:
            (rel, cos), (rel_u, cos_u) = _rel_cos(a, w), _rel_cos(b, w)
            ok = rel <= 5e-3 and cos >= 0.99999
            report.append(f"{'ok ' if ok else 'BAD'} {name}: rel {rel:.2e} cos {cos:.6f} (unfused: rel {rel_u:.2e} cos {cos_u:.6f})")
    print("\n".join(report))
    assert not [r for r in report if r.startswith("BAD")], "\n".join(report)


@pytest.mark.gpu
def test_pose_refinement_step_through_the_fused_object_operator():
    """The reference's pose-refinement step with objects (fixture train_step_POSE_OBJ) on the same model flags, called with
    `object_ray_grads=True`, the gates of test_pose_refinement_step_with_objects_matches_the_reference_step: `pose_r`, `pose_t` and the
    five ray tensors within 5e-3 of their norm with cosine >= 0.99999.  With a track that also requires a gradient both refinements run
    from one forward and the ray gradients keep their bits."""
    from nerflidar_hip import losses as nl, training as ntrain
    from test_pose_refine_objects import RAY_GRAD_KEYS, _scene
    g = golden("train_step_POSE_OBJ")
    plain, batch, pn = _scene(g, False)
    fused = _fused_twin(plain, g)

    def step(tm, track=None):
        tm.zero_grad(set_to_none=True)
        pn.zero_grad(set_to_none=True)
        refined = ntrain.refine_batch(batch, pn(batch["glo_idx"].reshape(-1).int()))
        for k in RAY_GRAD_KEYS:
            refined[k].retain_grad()
        kw = {} if track is None else {"curr_track": track}
        rend, hist = tm(refined, train_frac=float(g["train_frac"]), randomized=False, object_ray_grads=True, **kw)
        terms = nl.total_loss(rend, hist, refined, **ntrain.loss_lambdas(int(g["step"]), (int(g["start_step"]), int(g["end_step"]))))
        terms["latent_reg"] = tm.latent_reg(float(g["latent_reg"]))
        sum(terms.values()).backward()
        ntrain.clip_gradients(pn)
        return {"pose_r": pn.r.grad.clone(), "pose_t": pn.t.grad.clone(), **{k: refined[k].grad.clone() for k in RAY_GRAD_KEYS}}, hist

    grads, hist = step(fused)
    grads_plain, _ = step(plain)
    for lvl, h in enumerate(hist):
        assert torch.equal(h["obj_mask"].cpu(), torch.from_numpy(g[f"hist{lvl}_obj_mask"])), f"owner map of level {lvl}"
    report = []
    for k, got in grads.items():
        (rel, cos), (rel_u, cos_u) = _rel_cos(got, torch.from_numpy(g["grad_" + k])), _rel_cos(grads_plain[k], torch.from_numpy(g["grad_" + k]))
        ok = rel <= 5e-3 and cos >= 0.99999
        report.append(f"{'ok ' if ok else 'BAD'} {k}: rel {rel:.2e} cos {cos:.6f} (unfused: rel {rel_u:.2e} cos {cos_u:.6f})")
    print("\n".join(report))
    assert not [r for r in report if r.startswith("BAD")], "\n".join(report)
    # a track that requires a gradient as well: one forward serves both, and the ray gradients keep their bits
    track = fused.tracks.clone().requires_grad_(True)
    both, _ = step(fused, track)
    assert track.grad is not None and float(track.grad.abs().max()) > 0
    for k in grads:
        print(f"{k}: with the track gradient differs by {float((both[k] - grads[k]).abs().max()):.2e}")
    for k in grads:
        assert torch.equal(both[k], grads[k]), k


def _sync_free_step(fused, pose):
    """One `training_step(as_tensors=True)` inside the refinement window under `torch.cuda.set_sync_debug_mode("error")`, after one
    warm-up step, on the scene of train_step_OBJ; optimisers with capturable = True."""
    from nerflidar_hip import training as ntrain
    from test_objects_train import _obj_step_scene
    g, mc, sd, class_names, lg, batch = _obj_step_scene()
    tm = ntrain.TrainableModel(mc, fused_mlp=True, tracks=g["tracks"], class_names=class_names, obj_log2_hashmap=lg, fused_objects=fused,
                               fused_object_frame=fused).cuda().load_reference(sd)
    opt = torch.optim.Adam(tm.parameters(), lr=1e-4, capturable=True)
    kw = dict(train_frac=float(g["train_frac"]), randomized=False, as_tensors=True)
    if pose:
        n = batch["origins"].shape[0]
        pn = ntrain.PoseNet(1, num_lidars=1).cuda()
        batch = dict(batch, glo_idx=torch.ones(n, dtype=torch.int64, device="cuda"))
        kw.update(posenet=pn, pn_optimizer=torch.optim.Adam(pn.parameters(), lr=1e-5, capturable=True), pn_lr_fn=lambda s: 1e-5, step=11000,
                  pose_window=(10000, 20000))
    else:
        tn = ntrain.TrackNet(g["tracks"]).cuda()
        kw.update(tracknet=tn, tn_optimizer=torch.optim.Adam(tn.parameters(), lr=1e-5, capturable=True), tn_lr_fn=lambda s: 1e-5, step=7000,
                  track_start_opt=5000)
    run = lambda: ntrain.training_step(tm, opt, batch, **kw)
    run()  # warm-up: plans, workspaces, the optimisers' state
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return out, (pn if pose else tn)


@pytest.mark.gpu
def test_track_refinement_step_reads_nothing_back():
    """A `training_step(as_tensors=True)` with a TrackNet inside its window on the fused-frame model runs under
    `torch.cuda.set_sync_debug_mode("error")`, and the TrackNet has moved; the same step with `fused_objects=False` raises there."""
    out, tn = _sync_free_step(True, pose=False)
    assert bool(torch.isfinite(out["loss"]))
    assert float(tn.opt_t.detach().abs().max()) > 0 and float(tn.opt_r.detach().abs().max()) > 0
    with pytest.raises(RuntimeError):
        _sync_free_step(False, pose=False)


@pytest.mark.gpu
def test_pose_refinement_step_reads_nothing_back():
    """The same with a PoseNet inside its window: the refined rays get their object share without a host read."""
    out, pn = _sync_free_step(True, pose=True)
    assert bool(torch.isfinite(out["loss"]))
    assert float(pn.r.detach().abs().max()) > 0 and float(pn.t.detach().abs().max()) > 0


# ---- the opt-in -------------------------------------------------------------------------------------------------------------------
def test_fused_object_frame_needs_fused_objects():
    from nerflidar_hip import config as nconfig, training as ntrain
    mc = nconfig.workload("REF", 10)
    with pytest.raises(ValueError, match="fused_objects"):
        ntrain.TrainableModel(mc, fused_object_frame=True)
    import inspect
    assert inspect.signature(ntrain.TrainableModel.__init__).parameters["fused_object_frame"].default is False


@pytest.mark.gpu
def test_refusal_stays_the_default_and_names_both_arguments():
    """Without `fused_object_frame` a fused-objects model still refuses a track or rays that require a gradient, and the message names
    the way out."""
    from nerflidar_hip import training as ntrain
    from test_objects_train import _obj_step_scene
    g, mc, sd, class_names, lg, batch = _obj_step_scene()
    tm = ntrain.TrainableModel(mc, tracks=g["tracks"], class_names=class_names, obj_log2_hashmap=lg, fused_objects=True).cuda().load_reference(sd)
    track = torch.from_numpy(np.asarray(g["tracks"], np.float32)).cuda().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="fused_objects.*fused_object_frame=True"):
        tm(batch, train_frac=float(g["train_frac"]), curr_track=track)
    rb = dict(batch, origins=batch["origins"].clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="fused_objects.*fused_object_frame=True"):
        tm(rb, train_frac=float(g["train_frac"]), object_ray_grads=True)
