"""`nlr_resample_kernel` alone at the three launches of a C2 sweep, for one build (the library `NLR_LIB_PATH` names, else the
tree's): N = 32 768 rays, (n_prev -> S) = (0 -> 64), (64 -> 64), (64 -> 128), dilation and anneal of `config.workload("C2")`.
The kernel is launched through the library's internal launcher (`nlr_launch_resample`, u uploaded once; `nlr_resample_level`
uploads u and synchronises in every call, which would be timed with it), HIP events around 200 launches after 20 warm-up launches.
Two inputs: "noise" (weights = rand^4 per bin, what the white-noise benchmark scene gives) and "peak" (one surface: a narrow
Gaussian in s, what a trained scene gives); each level resamples the previous level's own output.
    NLR_LIB_PATH=<lib> python scripts/resample_ab.py [TAG] [--dump OUT.npz] [--launches K]     one line per launch shape
Run the builds alternating, one process each.  With --dump the sdist / tdist of every launch go to OUT.npz (two builds' files are
compared with numpy.array_equal); --launches K times K launches after K // 10 warm-up launches (scripts/pmc_resample.sh: 10)."""
import ctypes as C
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-lidar_amd")); sys.path.insert(0, ROOT)
import numpy as np, torch
from nerflidar_hip import _lib, config as nconfig

tag = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else "build"
dump = sys.argv[sys.argv.index("--dump") + 1] if "--dump" in sys.argv else None
launches = int(sys.argv[sys.argv.index("--launches") + 1]) if "--launches" in sys.argv else 200
dev = "cuda"
N = 32768
L = _lib.lib()
# int nlr_launch_resample(const float*, const float*, unsigned, float, float, float, unsigned, const float*, const float*, float,
#                         const float*, const float*, float, unsigned, float*, float*, hipStream_t)
launch = getattr(L, "_Z19nlr_launch_resamplePKfS0_jfffjS0_S0_fS0_S0_fjPfS1_P12ihipStream_t")
launch.restype = C.c_int
launch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float,
                   C.c_void_p, C.c_void_p, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
L.nlr_sample_u.argtypes = [C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
L.nlr_sample_u.restype = None
mc = nconfig.workload("C2", 14)
sched = list(mc.level_schedule(1.0))
assert [s for s, _, _ in sched] == [64, 64, 128], sched
print(f"# {tag}: build {L.nlr_build_sha().decode()}  device {torch.cuda.get_device_name(0)}", flush=True)
g = torch.Generator(device="cpu").manual_seed(0)
near = torch.full((N,), 0.008, device=dev)
far = torch.full((N,), 2.0, device=dev)


def weights_for(kind, sdist):
    n = sdist.shape[1] - 1
    if kind == "noise":
        w = torch.rand(N, n, generator=g) ** 4
    else:
        mid = ((sdist[:, 1:] + sdist[:, :-1]) / 2).cpu()
        c = torch.rand(N, 1, generator=g) * 0.8 + 0.1
        w = torch.exp(-0.5 * ((mid - c) / 0.01) ** 2) * (sdist[:, 1:] - sdist[:, :-1]).cpu() + 1e-12
    return (w / w.sum(-1, keepdim=True)).to(dev).contiguous()


def run(prev_s, prev_w, n_prev, S, dilation, anneal):
    uh = (C.c_float * 1024)()
    L.nlr_sample_u(S, 0, uh, None)
    u = torch.tensor(list(uh[:S]), device=dev)
    sd = torch.empty(N, S + 1, device=dev)
    td = torch.empty(N, S + 1, device=dev)
    st = _lib.current_stream()
    def go():
        rc = launch(_lib.ptr(prev_s), _lib.ptr(prev_w), n_prev, dilation, anneal, mc.resample_padding, S, _lib.ptr(u), None, 0.0,
                    _lib.ptr(near), _lib.ptr(far), mc.power_lambda, N, _lib.ptr(sd), _lib.ptr(td), st)
        assert rc == 0, L.nlr_last_error()
    for _ in range(launches // 10): go()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches): go()
    b.record(); b.synchronize()
    return a.elapsed_time(b) / launches * 1e3, sd, td


out = {}
for kind in ("noise", "peak"):
    prev_s = prev_w = None
    n_prev = 0
    for li, (S, dilation, anneal) in enumerate(sched):
        us, sd, td = run(prev_s, prev_w, n_prev, S, float(dilation), float(anneal))
        print(f"{tag:7s} {kind:5s} level {li} ({n_prev:2d} -> {S:3d}) dilation {dilation:.6f}  {us:8.2f} us / launch", flush=True)
        out[f"{kind}_L{li}_sdist"], out[f"{kind}_L{li}_tdist"] = sd.cpu().numpy(), td.cpu().numpy()
        prev_s, prev_w, n_prev = sd, weights_for(kind, sd), S
if dump:
    np.savez(dump, **out)
