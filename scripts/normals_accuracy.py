"""What the GPU tests of the density normals measure, as one file: runs `pytest tests/test_normals.py -m gpu` in this process and
writes the lines the test module collects in ACCURACY_LINES (every figure a test compares with its gate, recorded before the
assertion), under a summary of the maxima.  The exit status is pytest's.
    python scripts/normals_accuracy.py > profiles/density_normals_accuracy.txt"""
import contextlib, io, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "nerf-lidar_amd"), ROOT]   # as tests/conftest.py: the module is read back below
import pytest

with contextlib.redirect_stdout(io.StringIO()) as captured:   # pytest's own report goes to stderr below, the file holds the figures only
    rc = pytest.main([os.path.join(ROOT, "tests", "test_normals.py"), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider"])
sys.stderr.write(captured.getvalue()[-6000:])
lines = sys.modules["test_normals"].ACCURACY_LINES
op = [l for l in lines if l.startswith("operator S=")]
ratio = max([float(re.search(r"\(x([0-9.eE+-]+)\)", l).group(1)) for l in op] or [float("nan")])
rel = max([float(re.search(r"err/max ([0-9.eE+-]+)", l).group(1)) for l in op if "err/max" in l] or [float("nan")])
from nerflidar_hip import _lib
import torch
print(f"""Density normals: what tests/test_normals.py measures on the GPU ({torch.cuda.get_device_name(0)}, build {_lib.lib().nlr_build_sha().decode()[:16]}); pytest exit status {int(rc)}.
operator lines: nlr_density_normals against the float64 restatement on the CPU, N = 37; err = the maximum over the samples that are not
  `near` (raw_grad: max abs; normals: max |dn| where |G| >= 1e-3 max|G|; ray_normals: max abs), f32-reference = the same for the float32 CPU
  restatement (the yardstick; the gate is 4 x it), err/max = err / max |G|.
  Over all {len(op)} (case, output) lines: largest err / f32-reference = x{ratio:.2f} (gate x4), largest raw_grad err/max = {rel:.2e}.
fine levels lines: L = 10, quantiles of |dn| over all samples against the same quantiles of the float32 CPU restatement (gate 4 x).
fixture lines: the operator on tests/golden/normals_fwd.npz (the reference's own tdist, weights and normals) beside the float32 CPU
  restatement against the same fixture (gate 4 x).
{len(lines)} lines follow, in the order the tests ran.
""")
print("\n".join(lines))
raise SystemExit(int(rc))
