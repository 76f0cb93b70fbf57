"""What the GPU tests of pose refinement measure, as one file: runs `pytest tests/test_pose_refine.py -m gpu` in this process and
writes the lines the test module collects in ACCURACY_LINES (every figure a test compares with its gate, recorded before the
assertion), under a summary of the maxima.  The exit status is pytest's.
    python scripts/pose_refine_accuracy.py > profiles/pose_refine_accuracy.txt"""
import contextlib, io, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import pytest

with contextlib.redirect_stdout(io.StringIO()) as captured:   # pytest's own report goes to stderr below, the file holds the figures only
    rc = pytest.main([os.path.join(ROOT, "tests", "test_pose_refine.py"), "-m", "gpu", "-q", "-p", "no:cacheprovider"])
sys.stderr.write(captured.getvalue()[-3000:])
lines = sys.modules["test_pose_refine"].ACCURACY_LINES
kern = [l for l in lines if l.startswith("kernel S=")]
ratio = max(float(re.search(r"\(x([0-9.eE+-]+)\)", l).group(1)) for l in kern)
rel = max(float(re.search(r"err/max ([0-9.eE+-]+)", l).group(1)) for l in kern)
from nerflidar_hip import _lib
import torch
print(f"""Pose refinement: what tests/test_pose_refine.py measures on the GPU ({torch.cuda.get_device_name(0)}, build {_lib.lib().nlr_build_sha().decode()[:16]}); pytest exit status {int(rc)}.
kernel lines: nlr_encode_features_backward_rays against float64 autograd on the CPU, N = 37; err = max |kernel - float64| over the rays
  not near a cell face, f32-reference = the same for the float32 CPU reference (the yardstick; the gate is 4 x it), err/max = err / max |float64|.
  Over all {len(kern)} (case, tensor) lines: largest err / f32-reference = x{ratio:.2f} (gate x4), largest err/max = {rel:.2e}
  (beside the 2e-5 max|want| gate of the other f32 backward kernels; the test asserts the 4 x yardstick form).
shipped lines: L = 10, C = 4 and L = 6, C = 1 on tests/golden/ckpt_trained, N = 64, S = 32, no ray left out.
step lines: train_step_POSE.npz through refine_batch + TrainableModel, fp32 path (gates 5e-3 / 0.99999) and fused bf16 path.
it refines: frozen field, 1024 rays of 4 frames, pose-only steps: step count, hit-point error before -> after.
{len(lines)} lines follow, in the order the tests ran.
""")
print("\n".join(lines))
raise SystemExit(int(rc))
