"""GPU: examples/device_frontend.py --local-ba --device-ba -- the estimator step is KeyframeMap.add_keyframe -> local_ba(ks): the windows are emitted,
solved by slam_local_ba_batch_dev and applied where they lie in HBM.  The example runs as a user would run it, in a child process, plain and with
--per-stream-keyframes: it exits 0, reports at least one solved window per stream, and the motion it prints is within the bar
tests/test_gpu_device_frontend_ba.py uses (0.03 max(1, |expected|) + 0.02 m)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 2


@pytest.mark.parametrize("extra", [[], ["--per-stream-keyframes"]], ids=["lockstep", "per_stream"])
def test_example_with_device_ba(extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "device_frontend.py"), "--local-ba", "--device-ba", "--frames", "12", "--streams", str(S)] + extra,
                       capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    num = r"\[([-\d., e]+)\]"
    motion = {int(m.group(1)): (np.array([float(v) for v in m.group(2).split(",")]), np.array([float(v) for v in m.group(3).split(",")]))
              for m in re.finditer(r"stream (\d+): translation " + num + r" m, expected " + num + r" m", r.stdout)}
    solved = {int(m.group(1)): int(m.group(2)) for m in re.finditer(r"stream (\d+): (\d+) local-BA windows solved", r.stdout)}
    assert sorted(motion) == sorted(solved) == list(range(S)), r.stdout[-1500:]
    for s in range(S):
        got, want = motion[s]
        assert solved[s] >= 1, (s, r.stdout[-1500:])
        assert np.abs(got - want).max() < 0.03 * max(1.0, np.abs(want).max()) + 0.02, (s, got, want)
    assert len(re.findall(r"local BA stream \d+: window of \d+ poses, \d+ points, \d+ observations", r.stdout)) >= S
