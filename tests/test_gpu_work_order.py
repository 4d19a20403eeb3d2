"""GPU: the order of the tracking kernel's work list (k_kpset_worklist: sorted by x-band, row, slot -- csrc/work_order.hpp) changes
which keypoint runs when, never what the lists hold.  SLAMHIP_WORK_BAND is read once per process, so every order runs in a child
process of its own (the four start together) and leaves its lists in an .npz file.

test 1: the kpset cycle under slot order, the default band, a 1-px band (pure x sort) and a band wider than the image (pure y sort):
        every field of every stream's list equal after every step.
test 2: the work list itself, read back through the library's test-only route: a permutation of each stream's live slots inside the
        stream's segment, keys non-decreasing, ties in slot order, ntot the sum; slot order for a set beyond the sort's LDS budget."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = {"slot": "0", "default": None, "x_sort": "1", "y_sort": "100000"}
FIELDS = ("yx", "is_3d", "xyz", "ids", "stereo_yx", "has_stereo")

CYCLE = r'''
import sys, numpy as np, torch
sys.path.insert(0, %(root)r)
import slam_jl_amd as slam
from slam_jl_amd import synthetic as syn
H, W, S, LEVELS, KF, NT = 185, 300, 4, 3, 5, 11
params = slam.Params(stereo=True, max_nb_keypoints=300)
cam = slam.Camera(*syn.KITTI_CAM, height=H, width=W)
ex = slam.Extractor.from_params(params, cam)
cap = ex.max_points + ex.grid_resolution[0] * ex.grid_resolution[1] + 8
disparity = 6.0
left, right, flows = syn.stereo_stream((H, W), NT + S, seed=21, step=(3.1, -6.3), disparity=disparity)   # fast: keypoints leave the image
flows = np.asarray(flows)
u8 = lambda im: np.ascontiguousarray(np.round(im * 255).astype(np.uint8).T)
keep_alive = []
def batch(frames, t, **kw):
    d = torch.from_numpy(np.stack([u8(frames[t + s]) for s in range(S)])).cuda(); torch.cuda.synchronize(); keep_alive.append(d)
    b = slam.PyramidBatch((H, W), levels=LEVELS, S=S)
    b.update_([d.data_ptr() + s * H * W for s in range(S)], u8=True, **kw)
    return b
rng = np.random.default_rng(5)
out = {}
ks = slam.KeypointSet(S, cap)
def dump(tag):
    for s in range(S):
        d = ks.download(s)
        for f in %(fields)r:
            out["%%s_s%%d_%%s" %% (tag, s, f)] = d[f]
camt = syn.KITTI_CAM
T21 = np.eye(4); T21[0, 3] = -disparity * 30.0 / camt[0]
sp_stereo = slam.stream_params(S, cam=camt, shift_yx=np.tile([0.0, -disparity], (S, 1)))
def shift_params(t):
    sh = np.array([flows[t + s] - flows[t - 1 + s] for s in range(S)]) + rng.normal(0, 0.5, (S, 2))
    return slam.stream_params(S, cam=camt, shift_yx=sh)

# stage 1: uploaded lists of 0, 1, 257 and cap keypoints (positions all over the image, 60 %% with a map point) through a temporal match,
# a stereo match and the triangulation
b0, b1, r1 = batch(left, 0), batch(left, 1), batch(right, 1, target_only=True)
for s, n in enumerate((0, 1, 257, cap)):
    yx = np.stack([rng.uniform(1, H, n), rng.uniform(1, W, n)], axis=1)
    ks.upload(s, yx, rng.random(n) < 0.6, xyz=rng.normal(0, 1, (n, 3)))
ks.flow_match(b0, b1, params, shift_params(1), prior=2)
dump("u_match")
ks.stereo_match(b1, r1, params, sp_stereo, prior=2)
ks.triangulate(camt, camt, T21, np.eye(4), max_error=3.0)
dump("u_stereo")

# stage 2: two key-frame periods of the cycle from empty lists: detect, four temporal matches (lost tracks leave), cull, detect / append,
# stereo match, triangulate -- the lists become queues of several detect generations
for s in range(S):
    ks.upload(s, np.zeros((0, 2)), np.zeros(0, bool))
prev = None
for t in range(1, NT):
    cur = batch(left, t)
    kf = (t - 1) %% KF == 0
    if prev is not None and ks.counts().sum() > 0:
        ks.flow_match(prev, cur, params, shift_params(t), prior=2, n_bound=int(ks.counts().sum()))
    if kf:
        fl = torch.from_numpy((rng.random(S * cap) < 0.15).astype(np.uint8)).cuda(); torch.cuda.synchronize(); keep_alive.append(fl)
        ks.remove(fl.data_ptr())
        ks.detect(ex, cur)
        ks.stereo_match(cur, batch(right, t, target_only=True), params, sp_stereo, prior=2)
        ks.triangulate(camt, camt, T21, np.eye(4), max_error=3.0)
    dump("t%%d" %% t)
    out["t%%d_counts" %% t] = ks.counts()
    prev = cur
ks.close()
np.savez(%(path)r, **out)
print("OK")
'''

WORKLIST = r'''
import sys, ctypes as C, numpy as np
sys.path.insert(0, %(root)r)
import slam_jl_amd as slam
from slam_jl_amd import _lib as L
lib = L.load()
fn = lib.slamhip_test_kpset_worklist                             # exported for this test only: not in slamhip.h, not in the binding table
fn.restype = C.c_int
fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, L.i32p, L.i32p, L.i32p]
H, W = 185, 300
rng = np.random.default_rng(9)
out = {}
def positions(n):
    yx = np.stack([rng.uniform(-4, H + 4, n), rng.uniform(-4, W + 4, n)], axis=1)
    anchors = np.stack([rng.uniform(1, H, 4), rng.uniform(1, W, 4)], axis=1)
    m = rng.random(n) < 0.3
    yx[m] = anchors[rng.integers(0, 4, int(m.sum()))]              # many keypoints in one band and row: ties
    k = rng.random(n)
    yx[k < 0.02, 0] = np.nan; yx[(k > 0.02) & (k < 0.04), 1] = np.nan; yx[(k > 0.04) & (k < 0.05)] = np.inf; yx[(k > 0.05) & (k < 0.06)] = -1e300
    return yx
def run(tag, cap, counts):
    S = len(counts)
    ks = slam.KeypointSet(S, cap)
    for s, n in enumerate(counts):
        yx = positions(n)
        ks.upload(s, yx, np.zeros(n, bool))
        out["%%s_yx%%d" %% (tag, s)] = yx
    work = np.full(S * cap, -1, np.int32)                        # (receives the set's whole array: zero behind the list, as created)
    ntot = np.zeros(1, np.int32); band = np.zeros(1, np.int32)
    ks.ctx.check(fn(ks.ctx.h, ks.h, H, W, L.ptr(work, L.i32p), L.ptr(ntot, L.i32p), L.ptr(band, L.i32p)))
    out[tag + "_work"] = work; out[tag + "_ntot"] = ntot; out[tag + "_band"] = band; out[tag + "_cap"] = np.array([cap]); out[tag + "_counts"] = np.array(counts)
    ks.close()
cap = 600
for r, counts in enumerate([(0, 1, 63), (64, 65, 255), (256, 257, 512), (513, cap, 0), (cap, cap, cap)]):
    run("r%%d" %% r, cap, counts)
run("big", 8193, (5, 8193, 300))                                 # 8193 slots pad to 16384 words: beyond the 64 KB of LDS -> slot order
np.savez(%(path)r, **out)
print("OK")
'''


def _spawn(code, env_band):
    env = dict(os.environ)
    env.pop("SLAMHIP_WORK_BAND", None)
    if env_band is not None:
        env["SLAMHIP_WORK_BAND"] = env_band
    return subprocess.Popen([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)


def _finish(p):
    so, se = p.communicate(timeout=600)
    assert p.returncode == 0 and so.strip().endswith("OK"), so[-800:] + se[-2000:]


@pytest.fixture(scope="module")
def cycles(tmp_path_factory):
    d = tmp_path_factory.mktemp("work_order")
    paths = {k: str(d / (k + ".npz")) for k in ORDERS}
    procs = {k: _spawn(CYCLE % dict(root=ROOT, fields=FIELDS, path=paths[k]), band) for k, band in ORDERS.items()}
    for p in procs.values():
        _finish(p)
    return {k: dict(np.load(paths[k])) for k in ORDERS}


def test_cycle_does_real_work(cycles):
    """the reference run (slot order) is a real cycle: lists of several generations, tracks lost, stereo matches and map points made"""
    a = cycles["slot"]
    n = [len(a["u_match_s%d_ids" % s]) for s in range(4)]
    cap = 300 + 6 * 9 + 8
    assert n[0] == 0 and n[1] <= 1 and 0 < n[2] <= 257 and 0 < n[3] < cap, n     # uploaded lists: some keypoints tracked, some lost at the border
    for s in range(4):
        c = [int(a["t%d_counts" % t][s]) for t in range(1, 11)]
        assert c[0] > 100 and c[4] < c[0], (s, c)                            # a detected list; tracks lost over the period
        ids = a["t10_s%d_ids" % s]
        assert (np.diff(ids) > 0).all() and ids[0] < c[0] <= ids[-1], s      # generation 1 survivors in front, later generations behind
        assert a["t6_s%d_has_stereo" % s].mean() > 0.3 and a["t6_s%d_is_3d" % s].mean() > 0.3, s


@pytest.mark.parametrize("order", ["default", "x_sort", "y_sort"])
def test_same_lists_under_every_order(cycles, order):
    a, b = cycles["slot"], cycles[order]
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (order, k)


def _clamp(v, hi):
    top = min(max(hi, 0), 65535)
    if v != v:
        return top
    if not v >= 1.0:
        return 0
    return top if v >= top else int(v)


def _key(y, x, H, W, band):
    return ((_clamp(x, W) // band) << 16) | _clamp(y, H)


@pytest.fixture(scope="module")
def worklists(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("work_list") / "lists.npz")
    _finish(_spawn(WORKLIST % dict(root=ROOT, path=path), None))
    return dict(np.load(path))


@pytest.mark.parametrize("tag", ["r0", "r1", "r2", "r3", "r4"])
def test_work_list_is_a_sorted_permutation(worklists, tag):
    w = worklists
    H, W = 185, 300
    cap, counts, band = int(w[tag + "_cap"][0]), [int(c) for c in w[tag + "_counts"]], int(w[tag + "_band"][0])
    work = w[tag + "_work"]
    assert band >= 16                                            # the default order is a banded one
    assert int(w[tag + "_ntot"][0]) == sum(counts)
    off = 0
    for s, n in enumerate(counts):
        seg = work[off:off + n].astype(np.int64)
        assert np.array_equal(np.sort(seg), s * cap + np.arange(n)), (tag, s)          # every live slot of stream s once, nothing else
        yx = w["%s_yx%d" % (tag, s)]
        keys = np.array([_key(yx[q - s * cap, 0], yx[q - s * cap, 1], H, W, band) for q in seg], dtype=np.int64)
        word = keys * (1 << 32) + seg                            # (key, slot) ascending = keys non-decreasing, ties in slot order
        assert (np.diff(word) > 0).all(), (tag, s)
        if n >= 255:
            assert len(np.unique(keys)) < n and len(np.unique(keys >> 16)) > 3, (tag, s)   # the case has ties and several bands
        off += n
    assert (work[off:] == 0).all()                               # nothing written past the list (the array is created zeroed)


def test_work_list_beyond_the_lds_budget_keeps_slot_order(worklists):
    w = worklists
    cap, counts = int(w["big_cap"][0]), [int(c) for c in w["big_counts"]]
    assert int(w["big_band"][0]) == 0 and int(w["big_ntot"][0]) == sum(counts)
    want = np.concatenate([s * cap + np.arange(n) for s, n in enumerate(counts)])
    assert np.array_equal(w["big_work"][:len(want)], want) and (w["big_work"][len(want):] == 0).all()
