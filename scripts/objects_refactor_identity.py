#!/usr/bin/env python
"""Do two builds of the library compute the same BYTES in everything that passes through csrc/nlr_objects.hip and
csrc/nlr_objects_train.h?  (profiles/objects_forward_identity.txt)

  run     (GPU):  NLR_LIB_PATH=<lib> python scripts/objects_refactor_identity.py run OUT.npz     once per build, one process each
  compare (CPU):  python scripts/objects_refactor_identity.py compare A.npz B.npz                 one line per case, then ALL IDENTICAL

A run keeps, per output array, its byte count and the SHA-256 of its bytes.

  inference  the five OWNER_CASES of tests/test_objects.py (scenes of tests/test_objects_train.py: two classes, latent size 16) through
             nlr_objects_apply - rgb form and density-only form, f32 and f16 tables: density, rgb, semantic, owner map; the fixture
             obj_REF_small through nlr_render_rays_dynamic at the three precisions and nlr_render_lidar_dynamic: every rendering key
             and every level's density, weights and owner mask
  training   the OP_CASES of tests/test_objects_train.py (with the class that owns nothing and the 2047 x 32 case) and its depth-3 /
             skip-0 case through nlr_obj_train_forward (both forms) and nlr_obj_train_backward: density, rgb, semantic, owner map,
             d_params, d_latents and the whole workspace after the backward (zeroed before the forward: counts, owner map, lists,
             acts, gacts, slabs, totals).  grad_tables is summed with float atomics, whose order differs between two passes of ONE
             build: it is kept from PASSES passes and reported as largest differences - between the builds (pass i against pass i,
             the largest over i) and between any two passes of the first build (the spread, measured on that build alone); the
             former may be at most twice the latter."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-lidar_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
PASSES = 6


def run(out_path):
    import torch
    import test_objects as tobj
    import test_objects_train as ttrain
    from conftest import golden
    from nerflidar_hip import _lib, objects as nobj, training as ntrain
    L, out, loose = _lib.lib(), {}, {}
    tp = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    def keep(case, **arrays):
        for k, t in arrays.items():
            b = t.detach().cpu().contiguous().numpy().tobytes()
            out[f"{case} | {k}"] = np.frombuffer(hashlib.sha256(b).digest() + len(b).to_bytes(8, "little"), np.uint8)

    # ---- nlr_objects_apply on the owner cases
    for N, S, n_obj in tobj.OWNER_CASES:
        sc = ttrain._op_scene(N, S, n_obj, [t % 2 for t in range(n_obj)])
        td, box, K = sc["td"].cuda(), sc["box"], sc["K"]
        for half in (0, 1):
            od, held = ntrain.objects_desc(sc["mlps"], sc["cls"], ttrain.LAT, weights=True, latents=sc["latents"])
            tabs = [m.encoder.embeddings.detach().half().contiguous() for m in sc["mlps"]]
            if half:
                for c, t in enumerate(tabs):
                    od.classes[c].mlp.grid.table, od.classes[c].mlp.grid.table_dtype = t.data_ptr(), 1
            objs = C.c_void_p(None)
            _lib.call("nlr_objects_create", od, objs, device="cuda")
            try:
                ws = torch.zeros(int(L.nlr_objects_workspace_bytes(objs, N, S)), dtype=torch.uint8, device="cuda")
                for form in ("rgb", "density"):
                    dens = sc["stat"]["density"].cuda().clone()
                    rgb, sem = (sc["stat"][k].cuda().permute(2, 0, 1).clone(memory_format=torch.contiguous_format) for k in ("rgb", "sem"))
                    win = torch.full((N, S), -7, dtype=torch.int32, device="cuda")
                    _lib.call("nlr_objects_apply", objs, sc["rays"], td, box, N, S, n_obj, dens, rgb if form == "rgb" else None, sem, K, win, ws,
                              ws.numel())
                    torch.cuda.synchronize()
                    keep(f"apply {(N, S, n_obj)} {'f16' if half else 'f32'} {form} form", density=dens, rgb=rgb, semantic=sem, owner=win)
            finally:
                L.nlr_objects_destroy(objs)
    # ---- the fixture through the render loop
    g = golden("obj_REF_small")
    mc, b, cids, cfgs, sd = tobj._scene(g)
    mc.config.instance_obj = True
    batch = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    for precision in (0, 1, 2):
        model = nobj.DynamicModel(mc, sd, g["tracks"], tobj.NAMES, precision=precision, obj_log2_hashmap=int(g["log2_hashmap"]))
        for lidar_only in ((False, True) if precision == 2 else (False,)):
            r, h = model.render_rays(batch, compute_extras=True, want_history=True, lidar_only=lidar_only)
            torch.cuda.synchronize()
            keep(f"{'nlr_render_lidar_dynamic' if lidar_only else 'nlr_render_rays_dynamic'} obj_REF_small precision {precision}",
                 **{k: v for k, v in r.items() if torch.is_tensor(v)},
                 **{f"level{i}.{k}": lv[k] for i, lv in enumerate(h) for k in ("density", "weights", "obj_mask") if k in lv})
    # ---- the training operator
    cases = [(c, {}) for c in ttrain.OP_CASES] + [((37, 5, 4, [0, 1, 0, 1]), dict(net_depth_viewdirs=3, skip_layer_dir=0))]
    for (N, S, n_obj, cls), kw in cases:
        sc = ttrain._op_scene(N, S, n_obj, cls, **kw)
        plan, mlps, K = sc["plan"], sc["mlps"], sc["K"]
        case = f"train {(N, S, n_obj, cls)}{' depth 3 skip 0' if kw else ''}"
        flats = [plan.flat(c, m).detach().contiguous() for c, m in enumerate(mlps)]
        plan.pack(flats)
        tabs = [m.encoder.embeddings.detach() for m in mlps]
        td, box, lat = sc["td"].cuda(), sc["box"], sc["latents"].cuda()
        need = int(L.nlr_obj_train_workspace_bytes(plan.handle, N, S, 1))
        ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
        gd, gr = sc["cot"]["density"].cuda().contiguous(), sc["cot"]["rgb"].cuda().permute(2, 0, 1).contiguous()
        for form in ("density", "rgb"):   # (the rgb form last: the backward follows it)
            dens = sc["stat"]["density"].cuda().clone()
            rgb, sem = (sc["stat"][k].cuda().permute(2, 0, 1).clone(memory_format=torch.contiguous_format) for k in ("rgb", "sem"))
            win = torch.full((N, S), -7, dtype=torch.int32, device="cuda")
            _lib.check(L.nlr_obj_train_forward(plan.handle, tp(tabs), _lib.ptr(lat), C.byref(sc["rays"]), _lib.ptr(td), _lib.ptr(box), N, S, n_obj,
                                               _lib.ptr(dens), _lib.ptr(rgb) if form == "rgb" else None, _lib.ptr(sem), K, _lib.ptr(win), _lib.ptr(ws),
                                               need, None), "nlr_obj_train_forward")
            torch.cuda.synchronize()
            keep(f"{case} forward {form} form", density=dens, rgb=rgb, semantic=sem, owner=win)
        for rep in range(PASSES):
            d_par = [torch.full((k,), -7.0, device="cuda") for k in plan.n_params]
            d_lat, g_tab = torch.full((n_obj, ttrain.LAT), -7.0, device="cuda"), [torch.zeros_like(t) for t in tabs]
            _lib.check(L.nlr_obj_train_backward(plan.handle, tp(tabs), _lib.ptr(lat), C.byref(sc["rays"]), _lib.ptr(td), _lib.ptr(box), N, S, n_obj,
                                                _lib.ptr(gd), _lib.ptr(gr), tp(d_par), _lib.ptr(d_lat), tp(g_tab), _lib.ptr(ws), need, None),
                       "nlr_obj_train_backward")
            torch.cuda.synchronize()
            keep(f"{case} backward pass {rep}", d_latents=d_lat, workspace=ws, **{f"d_params[{c}]": t for c, t in enumerate(d_par)})
            for c, t in enumerate(g_tab):
                loose[f"{case} | grad_tables[{c}] pass {rep}"] = t.cpu().numpy()
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
        if k.startswith("LOOSE ") and k.endswith(" pass 0"):
            ks = [k[:-1] + str(i) for i in range(PASSES)]
            between = max(float(np.abs(a[x].astype(np.float64) - b[x]).max()) for x in ks)
            spread = max(float(np.abs(a[x].astype(np.float64) - a[y]).max()) for i, x in enumerate(ks) for y in ks[i + 1:])
            ok = between <= 2 * spread
            bad += not ok
            print(f"{k[6:-7]} (float atomics): between the builds {between:.3e}, between passes of the first build {spread:.3e}, "
                  f"largest entry {float(np.abs(a[k]).max()):.3e}{'' if ok else '  ABOVE TWICE THE SPREAD'}")
    print("ALL IDENTICAL" if not bad else f"{bad} CASES DIFFER")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
