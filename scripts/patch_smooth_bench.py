#!/usr/bin/env python3
"""Forward + backward of the patch-smoothness operator (nlr_patch_smooth_forward / _backward through `losses.patch_smoothness`) against
its torch restatement on the same device, at the shipped shape: 16 patches of 32 x 32 pixels, 19 classes.

    python scripts/patch_smooth_bench.py [--out profiles/patch_smooth_bench.txt]

Per call, device events around `--iters` calls (autograd wrapper and launches included), the two backends alternating over `--repeats`
windows after a warm-up of both.  Information, not a gate."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--patches", type=int, default=16)
    ap.add_argument("--patch-size", type=int, default=32)
    ap.add_argument("--classes", type=int, default=19)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args(argv)
    sys.path.insert(0, os.path.join(ROOT, "nerf-lidar_amd"))
    import torch
    from nerflidar_hip import losses as nl
    if not torch.cuda.is_available():
        raise RuntimeError("patch_smooth_bench needs a GPU: a time taken elsewhere says nothing")
    P, s, K = a.patches, a.patch_size, a.classes
    gen = torch.Generator().manual_seed(0)
    n = P * s * s
    depth = (0.2 + 1.6 * torch.rand(n, generator=gen)).cuda().requires_grad_(True)
    sem = torch.softmax(4 * torch.rand(n, K, generator=gen) - 2, -1).cuda().requires_grad_(True)
    rgb = torch.rand(n, 3, generator=gen).cuda()
    valid = (torch.rand(n, generator=gen) > 0.3).float().cuda()

    def step(backend):
        t_d, t_s = nl.patch_smoothness(depth, sem, rgb, valid, s, backend=backend)
        (0.01 * t_d + 0.01 * t_s).backward()
        depth.grad = sem.grad = None

    def timed(backend):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            step(backend)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3 / a.iters  # microseconds per call

    for b in ("hip", "torch"):
        for _ in range(30):
            step(b)
    torch.cuda.synchronize()
    res = {"hip": [], "torch": []}
    for _ in range(a.repeats):
        for b in res:
            res[b].append(timed(b))
    lines = [f"patch smoothness, forward + backward per call, (P, s, K) = ({P}, {s}, {K}), {torch.cuda.get_device_name(0)}",
             f"device events around {a.iters} calls (autograd wrapper and launches included), {a.repeats} alternating windows after warm-up"]
    for b, v in res.items():
        lines.append(f"{b:6s} median {statistics.median(v):8.1f} us   min {min(v):8.1f}   max {max(v):8.1f}")
    lines.append(f"torch / hip (medians): {statistics.median(res['torch']) / statistics.median(res['hip']):.1f}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
