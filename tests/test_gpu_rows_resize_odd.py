"""GPU: the imresize! fused into k_iir_rows_ck at ODD level heights (k_iir_rows_ck_odd: H = 2 Hd - 1, row pairs on any lane, bands
of 63 rows) builds the same planes, bit for bit, as the plain store + k_resize (SLAMHIP_NO_ROWS_RESIZE_ODD=1), as a target-only
build's layer chain, and as the oracle.  The knobs are read once per process, so every build runs in a process of its own and leaves
its planes in an .npz file.  (That the default run launches no k_resize and the knob run does is recorded in
profiles/r08a_rows_resize_odd_kernels_*.csv: two runs of the old path would compare equal too.)"""
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
H, W, S, u8, reps, target = %(H)d, %(W)d, %(S)d, %(u8)r, %(reps)d, %(target)r
rng = np.random.default_rng(11)
base = syn.texture_canvas(H, W, seed=4, margin=0)
fr = [np.clip(base + 0.05 * rng.standard_normal((H, W)), 0, 1) for _ in range(min(S, 8))]
if u8:
    fr = [np.round(f * 255).astype(np.uint8) for f in fr]
dev = [torch.from_numpy(np.ascontiguousarray(fr[s %% len(fr)].T)).cuda() for s in range(S)]
torch.cuda.synchronize()
pb = slam.PyramidBatch((H, W), levels=3, S=S)
keep = sorted({0, 1, S // 2, S - 1})
names = ("layers",) if target else %(pl)r
out = {}
for r in range(reps):                                            # the cached graph, replayed
    pb.update_([d.data_ptr() for d in dev], u8=u8, target_only=target)
    for s in keep:
        for l in range(1 if target else 0, 4):
            for nm in names:
                g = pb.pyramids[s].plane(nm, l)
                if r == 0:
                    out["%%d_%%s_%%d" %% (s, nm, l)] = g
                else:
                    assert np.array_equal(g, out["%%d_%%s_%%d" %% (s, nm, l)]), ("replay", r, s, nm, l)
np.savez(%(path)r, **out)
print("OK")
'''

CK0 = {"SLAMHIP_CK_MIN_MB": "0"}         # small batches: every level on the checkpointed kernels (their lower levels are under the 40 MB gate)


def _build(tmp_path, tag, env, H, W, S, u8, reps=1, target=False):
    path = str(tmp_path / (tag + ".npz"))
    code = BUILD % dict(root=ROOT, H=H, W=W, S=S, u8=u8, reps=reps, pl=PL, path=path, target=target)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-800:] + r.stderr[-1500:]
    return dict(np.load(path))


def _off(env):
    return dict(env, SLAMHIP_NO_ROWS_RESIZE_ODD="1")


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _frames(H, W, S, u8):
    from slam_jl_amd import synthetic as syn
    rng = np.random.default_rng(11)
    base = syn.texture_canvas(H, W, seed=4, margin=0)
    fr = [np.clip(base + 0.05 * rng.standard_normal((H, W)), 0, 1) for _ in range(S)]
    return [np.round(f * 255).astype(np.uint8) / 255.0 for f in fr] if u8 else fr


# (370, 1226, 128): the headline's batch, heights 370 / 185 / 93 / 47.  S = 8: (185, 613) and (93, 307) are odd at level 0 and have
# pairs that start on lanes 63 and 127; (129, 200): H = 129 -> 65 -> 33; (376, 1241) halves evenly (the exact-2:1 path alone).
# S = 4 takes the launch over all four planes of a level (no k_rows_cum fork), which keeps k_resize at odd heights: the knob must not matter.
@pytest.mark.parametrize("H,W,S,u8,env", [
    (370, 1226, 128, True, {}),
    (370, 1226, 8, True, CK0),
    (185, 613, 8, True, CK0),
    (129, 200, 8, False, CK0),
    (93, 307, 8, True, CK0),
    (376, 1241, 8, False, CK0),
    (185, 613, 4, True, CK0),
    (93, 307, 4, False, CK0),
])
def test_fused_resize_at_odd_heights_equals_k_resize(tmp_path, H, W, S, u8, env):
    _assert_same(_build(tmp_path, "on", env, H, W, S, u8, reps=3), _build(tmp_path, "off", _off(env), H, W, S, u8))


def test_target_only_layers_equal_the_full_build(tmp_path):
    H, W, S = 370, 1226, 8
    full = _build(tmp_path, "full", CK0, H, W, S, True)
    tgt = _build(tmp_path, "tgt", CK0, H, W, S, True, reps=3, target=True)
    tgt_off = _build(tmp_path, "tgt_off", _off(CK0), H, W, S, True, target=True)
    assert len(tgt) == 4 * 3                                      # streams 0, 1, 4, 7 x levels 1-3
    for k in tgt:
        assert np.array_equal(tgt[k], full[k]), k
        assert np.array_equal(tgt[k], tgt_off[k]), k


@pytest.mark.parametrize("H,W,u8", [(370, 1226, True), (185, 613, False)])
def test_planes_equal_oracle(tmp_path, H, W, u8):
    from oracle import oracle as orc
    S = 8
    got = _build(tmp_path, "on", CK0, H, W, S, u8, reps=2)
    fr = _frames(H, W, S, u8)
    for s in (0, S - 1):
        ref = orc.pyr_build(np.asfortranarray(fr[s]), 3, 1.0, 1)
        for l in range(4):
            for nm in PL:
                assert np.array_equal(got["%d_%s_%d" % (s, nm, l)], ref.plane(nm, l)), (s, nm, l)
