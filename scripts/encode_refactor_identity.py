#!/usr/bin/env python
"""Do two builds of the library compute the same BYTES in everything that passes through csrc/nlr_encode.hip and nlr_encode_rays.hip?
(profiles/encode_refactor_identity.txt)

  run     (GPU):  NLR_LIB_PATH=<lib> python scripts/encode_refactor_identity.py run OUT.npz      once per build, one process each
  compare (CPU):  python scripts/encode_refactor_identity.py compare A.npz B.npz                 one line per case, then ALL IDENTICAL

A run keeps, per output array, its byte count and the SHA-256 of its bytes (the arrays themselves are ~0.5 GB per build).

Shapes: N = 173 rays x S = 48 samples (8 304 samples = 259.5 workgroups of the 8-lane kernels: one full round of 8 x 32 chunks of
nlr_xcd_block, an identity-order tail, a partial last workgroup, a ray count that is no multiple of 8) and N = 5 x S = 3; with and
without rand_deg.
  forward    nlr_encode_features_forward: sample_n 1, 7, 8, 9, 16 (both lane mappings) x C 1, 2, 4, 8 x f32 / f16 tables x re_weights
             0 / 1 x fast route / NLR_DBG_FORCE_GENERIC, and two grids that are generic by themselves (smoothstep, align_corners)
  training   nlr_cast_contract, nlr_encode_features_backward_ws (the outputs of its expand kernel: positions and per-point feature
             gradients) and nlr_encode_features_backward_rays at sample_n = 7, C 1, 2, 4, 8, both dtypes.  The table gradient is summed
             with float atomics by the grid operator (csrc/nlr_grid.hip), whose order differs between two runs of ONE build: it is
             reported as a largest difference, not as bytes.
  render     Model.render_rays with history (the proposal launcher and the piece-major layout): C2 / 2^14, P_F32 / 2^15, P_F20 / 2^12
             on the 48-column sweep of the fast / generic test, both dtypes, both routes, NLR_DBG_RAY_GROUPS 0, 1, 2, sample_n 7 and 9;
             every rendering key and every level's sdist, tdist, density, weights."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-lidar_amd"))
SHAPES = ((173, 48), (5, 3))


def run(out_path):
    import torch
    from nerflidar_hip import _lib, config as nconfig, lidar as nlidar, training as ntrain, weights as nweights
    from nerflidar_hip.gridencoder import GridEncoder, backward_workspace
    from nerflidar_hip.models import _RAY_KEYS, Model
    dev = torch.device("cuda:0")
    L, out, loose = _lib.lib(), {}, {}

    def keep(case, **arrays):
        for k, t in arrays.items():
            b = t.detach().cpu().contiguous().numpy().tobytes()
            out[f"{case} | {k}"] = np.frombuffer(hashlib.sha256(b).digest() + len(b).to_bytes(8, "little"), np.uint8)

    def encoder(C_, half, interp="linear", align=False):
        enc = GridEncoder(num_levels=4, level_dim=C_, per_level_scale=2, base_resolution=16, log2_hashmap_size=14, interpolation=interp,
                          align_corners=align)
        tab = torch.rand(enc.embeddings.shape, generator=torch.Generator().manual_seed(C_)) * 2 - 1
        return enc, (tab.half() if half else tab).to(dev)

    def rays_of(N, S, n, rand):
        sw = nlidar.synthetic_sweep(width=64, seed=3)
        idx = np.linspace(0, sw["origins"].shape[0] - 1, N).astype(np.int64)
        batch = {k: torch.from_numpy(np.ascontiguousarray(sw[k][idx])).to(dev) for k in _RAY_KEYS}
        g = torch.Generator().manual_seed(N * 100 + S)
        # intervals on both sides of the contraction's |x| = 1
        tdist = torch.cumsum(torch.rand(N, S + 1, generator=g) * (6.0 / (S + 1)) + 1e-3, 1).to(dev)
        rd = torch.rand(N, S, n, generator=g).to(dev) if rand else None
        return batch, tdist, rd

    def forced(generic):
        _lib.check(L.nlr_debug_set(_lib.DBG_FORCE_GENERIC, generic))

    try:
        for N, S in SHAPES:
            for rand in (0, 1):
                for n in (1, 7, 8, 9, 16):
                    batch, tdist, rd = rays_of(N, S, n, rand)
                    grids = [(f"C{c} {'f16' if h else 'f32'}", encoder(c, h), (0, 1)) for c in (1, 2, 4, 8) for h in (0, 1)]
                    grids += [("smoothstep C2 f32", encoder(2, 0, interp="smoothstep"), (0,)), ("align_corners C2 f32", encoder(2, 0, align=True), (0,))]
                    for gname, (enc, tab), routes in grids:
                        (rays, held), gd = _lib.rays(batch, N), ntrain._EncodeFeatures._descs(enc, tab)
                        case = f"N{N} S{S} rand{rand} n{n} {gname}"
                        for re_w in (0, 1):
                            for generic in routes:
                                forced(generic)
                                f = torch.full((N * S, enc.output_dim), float("nan"), device=dev)
                                _lib.check(L.nlr_encode_features_forward(C.byref(rays), _lib.ptr(tdist), N, S, n, 3, 0.35, _lib.ptr(rd), C.byref(gd), re_w,
                                                                         _lib.ptr(f), _lib.current_stream()), "forward")
                                keep(f"forward {case} re_w{re_w} {'generic' if generic else 'fast'}", features=f)
                        forced(0)
                        if n != 7 or len(routes) == 1:
                            continue
                        means, stds = torch.empty(N, S, n, 3, device=dev), torch.empty(N, S, n, device=dev)
                        _lib.check(L.nlr_cast_contract(C.byref(rays), _lib.ptr(tdist), N, S, n, 3, 0.35, _lib.ptr(rd), _lib.ptr(means), _lib.ptr(stds),
                                                       _lib.current_stream()), "cast_contract")
                        g = torch.randn(N * S, enc.output_dim, generator=torch.Generator().manual_seed(7)).to(dev)
                        pts, gpt = torch.empty(N * S * n, 3, device=dev), torch.empty(N * S * n, enc.output_dim, device=dev)
                        grad = torch.zeros(tab.shape, device=dev)
                        ws = backward_workspace(N * S * n, tab.shape[1], enc.num_levels, float(np.log2(enc.per_level_scale)), int(enc.base_resolution),
                                                enc._offsets_host, enc.gridtype_id, enc.align_corners, dev)
                        _lib.check(L.nlr_encode_features_backward_ws(C.byref(rays), _lib.ptr(tdist), N, S, n, 3, 0.35, _lib.ptr(rd), C.byref(gd), 1, _lib.ptr(g),
                                                                     _lib.ptr(pts), _lib.ptr(gpt), _lib.ptr(grad), _lib.ptr(ws), 0 if ws is None else ws.numel(),
                                                                     _lib.current_stream()), "backward_ws")
                        d = [torch.empty(N, 3, device=dev) for _ in range(4)]
                        _lib.check(L.nlr_encode_features_backward_rays(C.byref(rays), _lib.ptr(tdist), N, S, n, 3, 0.35, _lib.ptr(rd), C.byref(gd), 1, _lib.ptr(g),
                                                                       *[_lib.ptr(t) for t in d], _lib.current_stream()), "backward_rays")
                        keep(f"training {case}", means=means, stds=stds, points=pts, point_grads=gpt, d_origins=d[0], d_directions=d[1], d_base_x=d[2],
                             d_base_y=d[3])
                        loose[f"training {case} | grad_table"] = grad.cpu().numpy()
        sweep = {k: torch.from_numpy(v).to(dev) for k, v in nlidar.synthetic_sweep(width=48, seed=4, beams=nlidar.LIDAR_ANGLES[::2]).items()}
        for wl, log2 in (("C2", 14), ("P_F32", 15), ("P_F20", 12)):
            mc = nconfig.workload(wl, log2)
            sd = nweights.synth_state_dict(mc, seed=2, trained_like=True)
            for dt in (torch.float32, torch.float16):
                model = Model(mc, sd, device=dev, table_dtype=dt)
                for n in (7, 9):
                    for generic in (0, 1):
                        for groups in (0, 1, 2):
                            forced(generic)
                            _lib.check(L.nlr_debug_set(_lib.DBG_RAY_GROUPS, groups))
                            case = f"render {wl} {str(dt).split('.')[1]} n{n} {'generic' if generic else 'fast'} ray_groups{groups}"
                            try:
                                r, h = model.render_rays(sweep, compute_extras=True, scale_factor=1 / 250, want_history=True, sample_n=n)
                            except RuntimeError as e:
                                print(f"{case}: refused ({str(e)[:100]})")
                                continue
                            torch.cuda.synchronize()
                            keep(case, **r, **{f"level{i}.{k}": lv[k] for i, lv in enumerate(h) for k in ("sdist", "tdist", "density", "weights")})
    finally:
        L.nlr_debug_set(_lib.DBG_FORCE_GENERIC, 0)
        L.nlr_debug_set(_lib.DBG_RAY_GROUPS, 0)
    np.savez(out_path, **out, **{"LOOSE " + k: v for k, v in loose.items()})
    print(f"wrote {out_path}: {len(out)} arrays, library {_lib.LIB_PATH}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), "the two runs hold different cases"
    cases, bad = {}, 0
    for k in a.files:
        if k.startswith("LOOSE "):
            continue
        case, _ = k.split(" | ")
        same, total, nbytes = cases.get(case, (0, 0, 0))
        cases[case] = (same + int(np.array_equal(a[k], b[k])), total + 1, nbytes + int.from_bytes(a[k][32:].tobytes(), "little"))
    for case, (same, total, nbytes) in cases.items():
        bad += same != total
        print(f"{case}: {same} of {total} arrays identical ({nbytes} bytes)")
    for k in a.files:
        if k.startswith("LOOSE "):
            d, m = float(np.abs(a[k].astype(np.float64) - b[k]).max()), float(np.abs(a[k]).max())
            print(f"{k[6:]} (float atomics): largest difference {d:.3e}, largest entry {m:.3e}")
    print("ALL IDENTICAL" if not bad else f"{bad} CASES DIFFER")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
