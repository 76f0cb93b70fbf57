"""Time of a full C2 sweep render through the generic level body (NLR_DBG_FORCE_GENERIC: nlr_encode8g_kernel / nlr_prop8g_kernel)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-lidar_amd"))
import torch
from nerflidar_hip import _lib, config as nconfig, lidar as nlidar, weights as nweights
from nerflidar_hip.models import Model
mc = nconfig.workload("C2"); sd = nweights.synth_state_dict(mc, seed=0, trained_like=True)
model = Model(mc, sd, precision=_lib.PREC_FAST)
batch = {k: torch.from_numpy(v).cuda() for k, v in nlidar.synthetic_sweep(width=1024, seed=0).items()}
_lib.check(_lib.lib().nlr_debug_set(_lib.DBG_FORCE_GENERIC, 1))
try:
    for _ in range(3): model.render_rays(batch, scale_factor=1 / 250)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(10): model.render_rays(batch, scale_factor=1 / 250)
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 10
finally:
    _lib.lib().nlr_debug_set(_lib.DBG_FORCE_GENERIC, 0)
print(f"C2 sweep, generic level body: {dt * 1e3:.3f} ms per sweep")
