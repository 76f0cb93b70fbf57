"""Time of the weight-gradient stage of the fused training NerfMLP alone, both ways on the same saved tensors in one process:
(a) the split-K library GEMMs (`training._wgrad_bmm`, what `_FusedMLP.backward` runs by default), (b) `nlr_mlp_train_wgrad` (one MFMA
kernel + slab reduce).  Shapes of scripts/train_mlp_bench.py.  The fused forward and backward run once; then HIP events around 20
calls after 3 warm-up calls, five repetitions, (a) and (b) alternating.
    python scripts/wgrad_bench.py > profiles/wgrad_ab.txt"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-lidar_amd")); sys.path.insert(0, ROOT)
import numpy as np, torch
from nerflidar_hip import _lib, config as nconfig, training
torch.manual_seed(0)
dev = "cuda"
F = torch.nn.functional
print(f"build {_lib.lib().nlr_build_sha().decode()}  device {torch.cuda.get_device_name(0)}", flush=True)


def timed(fn, calls=20, warm=3):
    for _ in range(warm): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls): fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) / calls


for wl, N, S in (("REF", 4096, 32), ("C2", 4096, 128), ("C2", 16384, 128)):
    mc = nconfig.workload(wl, 12)
    cfg = mc.nerf_mlp
    M = N * S
    feats = (torch.randn(N, S, cfg.grid_num_levels * cfg.grid_level_dim, device=dev) * 0.3).requires_grad_(True)
    batch = {"viewdirs": F.normalize(torch.randn(N, 3, device=dev), dim=-1)}
    lv = training.TrainableNerfLevel(cfg, fused_mlp=True).to(dev)
    lv._keep_debug = True
    o = lv._forward_fused(batch, feats)
    sum((v * torch.randn_like(v)).sum() for v in o.values()).backward()
    d = lv._dbg
    f, e, acts, gacts = d["feats"], d["enc"], d["acts"], d["gacts"]
    del o
    lv.zero_grad(set_to_none=True); feats.grad = None
    plan = lv._plan
    ws = lv._wgrad_workspace(torch.device(dev, 0))
    d_params = torch.empty(plan.n_params, device=dev)
    st = _lib.current_stream()

    def run_bmm():
        return training._wgrad_bmm(lv, M, f, e, acts, gacts)

    def run_kernel():
        _lib.check(_lib.lib().nlr_mlp_train_wgrad(plan.handle, M, S, _lib.ptr(f), _lib.ptr(e), _lib.ptr(acts), _lib.ptr(gacts), _lib.ptr(d_params),
                                                  _lib.ptr(ws), ws.numel(), st), "nlr_mlp_train_wgrad")

    run_kernel()
    flat = torch.cat([g.reshape(-1) for g in run_bmm()])
    dev_rel = float((flat - d_params).norm() / flat.norm())
    ta, tb = [], []
    for _ in range(5):
        ta.append(timed(run_bmm)); tb.append(timed(run_kernel))
    n_w = sum(p.numel() for i, p in enumerate(lv._mlp_params()) if i % 2 == 0)
    rd, fl = M * (2 * plan.act_w + 64) * 2 + M * f.shape[1] * 4, 2.0 * M * n_w
    stat = lambda t: f"min {min(t):.3f}  median {float(np.median(t)):.3f}  max {max(t):.3f} ms"
    med = float(np.median(tb))
    print(f"{wl} {N} rays x {S} samples (M = {M}, act_w = {plan.act_w}, {plan.n_params} parameters, workspace {ws.numel() / 2**20:.1f} MiB)\n"
          f"  (a) library GEMMs (33-launch bmm form): {stat(ta)}\n"
          f"  (b) nlr_mlp_train_wgrad:                {stat(tb)}\n"
          f"  (b) median / (a) min = {med / min(ta):.3f}; (b) reads {rd / 1e9:.2f} GB once and does {fl / 1e12:.3f} TFLOP: achieved "
          f"{rd / med / 1e6:.0f} GB/s, {fl / med / 1e9:.0f} TFLOP/s; |(a) - (b)| / |(a)| = {dev_rel:.2e}", flush=True)
    del lv, d, f, e, acts, gacts, feats, flat, ws, d_params
    torch.cuda.empty_cache()
