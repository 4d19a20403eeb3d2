"""GPU: k_rows_cum (the product planes' dim-2 filter and integral image in one launch) builds the same planes, bit for bit, as
k_iir_rows_ck + k_cum_fused (SLAMHIP_NO_ROWS_CUM=1).  The knob is read once per process, so every build runs in a process of its
own and leaves its planes in an .npz file."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PL = ("layers", "Iy", "Ix", "Iyy", "Ixx", "Iyx")

BUILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, %(root)r)
import slam_jl_amd as slam
from slam_jl_amd import synthetic as syn
H, W, S, u8, reps = %(H)d, %(W)d, %(S)d, %(u8)r, %(reps)d
rng = np.random.default_rng(11)
base = syn.texture_canvas(H, W, seed=4, margin=0)
fr = [np.clip(base + 0.05 * rng.standard_normal((H, W)), 0, 1) for _ in range(min(S, 8))]
if u8:
    fr = [np.round(f * 255).astype(np.uint8) for f in fr]
dev = [torch.from_numpy(np.ascontiguousarray(fr[s %% len(fr)].T)).cuda() for s in range(S)]
torch.cuda.synchronize()
pb = slam.PyramidBatch((H, W), levels=3, S=S)
keep = sorted({0, 1, S // 2, S - 1})
out = {}
for r in range(reps):                                            # the cached graph, replayed
    pb.update_([d.data_ptr() for d in dev], u8=u8)
    for s in keep:
        for l in range(4):
            for nm in %(pl)r:
                g = pb.pyramids[s].plane(nm, l)
                if r == 0:
                    out["%%d_%%s_%%d" %% (s, nm, l)] = g
                else:
                    assert np.array_equal(g, out["%%d_%%s_%%d" %% (s, nm, l)]), ("replay", r, s, nm, l)
np.savez(%(path)r, **out)
print("OK")
'''


def _build(tmp_path, tag, env, H, W, S, u8, reps=1):
    path = str(tmp_path / (tag + ".npz"))
    code = BUILD % dict(root=ROOT, H=H, W=W, S=S, u8=u8, reps=reps, pl=PL, path=path)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-800:] + r.stderr[-1500:]
    return dict(np.load(path))


def _off(env):
    return dict(env, SLAMHIP_NO_ROWS_CUM="1")


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("H,W,S,u8", [(370, 1226, 128, True), (370, 1226, 8, True), (376, 1241, 8, False), (480, 640, 8, True)])
def test_rows_cum_equals_separate_kernels(tmp_path, H, W, S, u8):
    env = {}
    _assert_same(_build(tmp_path, "on", env, H, W, S, u8, reps=3), _build(tmp_path, "off", _off(env), H, W, S, u8))


@pytest.mark.parametrize("ckmin", ["0", "100000"])
def test_rows_cum_on_both_sides_of_the_checkpoint_threshold(tmp_path, ckmin):
    env = {"SLAMHIP_CK_MIN_MB": ckmin}                           # 0: every level on the checkpointed kernels; 100000: none
    _assert_same(_build(tmp_path, "on", env, 185, 613, 8, True), _build(tmp_path, "off", _off(env), 185, 613, 8, True))


def test_rows_cum_planes_equal_oracle(tmp_path):
    from oracle import oracle as orc
    from slam_jl_amd import synthetic as syn
    H, W, S = 376, 1241, 8
    got = _build(tmp_path, "on", {}, H, W, S, False, reps=2)
    rng = np.random.default_rng(11)
    base = syn.texture_canvas(H, W, seed=4, margin=0)
    fr = [np.clip(base + 0.05 * rng.standard_normal((H, W)), 0, 1) for _ in range(S)]
    for s in (0, S - 1):
        ref = orc.pyr_build(np.asfortranarray(fr[s]), 3, 1.0, 1)
        for l in range(4):
            for nm in PL:
                assert np.array_equal(got["%d_%s_%d" % (s, nm, l)], ref.plane(nm, l)), (s, nm, l)
