"""What tests/test_grid_envelope.py measures on the GPU, as one file: runs the module with NLR_GRID_ENVELOPE_LOG set (every table-gradient
figure is recorded before its assertion) and, on the CPU, the yardstick the 2e-6 bound would fall back to: the float32 oracle on a
permuted point order against itself (the order sensitivity of the sums), relative to the same sum of |terms|.  The exit status is pytest's.
    python scripts/grid_envelope_accuracy.py > profiles/grid_envelope_accuracy.txt"""
import contextlib, io, os, re, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
log = os.path.join(tempfile.mkdtemp(), "figures.txt")
os.environ["NLR_GRID_ENVELOPE_LOG"] = log
import numpy as np
import pytest

with contextlib.redirect_stdout(io.StringIO()) as captured:
    rc = pytest.main([os.path.join(ROOT, "tests", "test_grid_envelope.py"), "-m", "gpu", "-q", "-p", "no:cacheprovider"])
sys.stderr.write(captured.getvalue()[-3000:])
lines = open(log).read().splitlines() if os.path.exists(log) else []
ratio = lambda ls: max([float(re.search(r"([0-9.]+e[+-][0-9]+) \(bound", l).group(1)) for l in ls] or [float("nan")])
import test_grid_envelope as tg
from oracle import nlr_oracle as orc

yard = []
for C, opts, (L, H, log2, pls) in ((1, (0, 0, 0), (5, 16, 16, 2.0)), (4, (0, 0, 1), (5, 16, 16, 2.0)), (2, (1, 1, 1), (5, 16, 15, 1.2))):
    offsets, S, _ = tg._grid(L, H, log2, pls, opts[1])
    B = (1 << 18) // C + 4096 + 37
    x = tg._large_points(B, "ray", 70 + C)
    grad = np.random.default_rng(71).standard_normal((L, B, C)).astype(np.float32)
    ref, ref_abs = tg._oracle_grads(grad, x, offsets, C, S, H, opts)
    perm = np.random.default_rng(72).permutation(B)
    ref_p, _ = tg._oracle_grads(np.ascontiguousarray(grad[:, perm]), x[perm], offsets, C, S, H, opts)
    yard.append((C, opts, pls, float(np.max(np.abs(ref_p - ref) / (ref_abs + 1e-3)))))
from nerflidar_hip import _lib
import torch
print(f"""Grid operator envelope: what tests/test_grid_envelope.py measures on the GPU ({torch.cuda.get_device_name(0)}, build {_lib.lib().nlr_build_sha().decode()[:16]}); pytest exit status {int(rc)}.
Table gradient against oracle/grid_oracle.c: max over the table of |kernel - oracle| / (sum of |terms| of the entry + 1e-3); the tests
assert err <= 2e-6 sum|terms| + 1e-6 per entry.
  small batches (x-pair and one-corner atomics, 8 batch sizes, both layouts), {len([l for l in lines if l.startswith('small')])} option lines: largest {ratio([l for l in lines if l.startswith('small')]):.3e}
  large batches (LDS copy, LDS cache, bins, atomics), {len([l for l in lines if l.startswith('large')])} route lines: largest {ratio([l for l in lines if l.startswith('large')]):.3e}
No option exceeds the bound, so none is held to the fall-back (4 x the order sensitivity of the float32 oracle).  That yardstick, for
the record - the oracle on a permuted point order against itself, same measure, B = 2^18 / C + 4133 ray-ordered points:""")
for C, opts, pls, y in yard:
    print(f"  C={C} (gridtype, align_corners, interp)={opts} scale {pls}: {y:.3e}")
print(f"{len(lines)} lines follow, in the order the tests ran.\n")
print("\n".join(lines))
raise SystemExit(int(rc))
