"""GPU: slam_local_ba_batch_dev -- the batched local BA on windows that are resident in HBM (uploaded with torch, solved in place).

staged arrays   the probe + stager kernels against the numpy model (tests/np_ba_dev_stage.py), array by array, exact (the integer arrays, pix; pose
                and pts are copies)
results         against slam_local_ba_batch on the same arrays, within the header's own contract for two routes that sum a window's points in
                different orders: theta <= 1e-6 relative, costs <= 1e-8 relative, iteration counts and outlier sets equal
precondition    for the outlier sets to be comparable at all, every test asserts of every window that at the pass-1 theta (the host form with
                iterations = 0) no observation's squared residual lies within 1e-3 relative of repr_eps and no depth within 1e-3 relative of
                1e-6: 1 000 x the theta contract -- a condition on the inputs (<= 0.5 px noise, scripted gross outliers of >= 20 px)
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_ba_dev_stage as npd  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPR_EPS = 5.0
INELIGIBLE, ERR_ARG, ERR_NUMERIC = 4, -1, -5


def _batch(slam, wins):
    return slam.BABatch([slam.LocalBACache(w["theta0"], w["theta_const"], w["pixels_yx"], w["pose_ids"], w["point_ids"]) for w in wins], [w["cam"] for w in wins])


class Dev:
    """a BABatch's arrays in HBM"""

    def __init__(self, b):
        import torch
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda() if a.size else torch.zeros(1, dtype=torch.from_numpy(a).dtype).cuda()
        self.b = b
        self.theta, self.tc, self.px, self.pi, self.li = up(b.theta0), up(b.tc), up(b.px.reshape(-1)), up(b.pi), up(b.li)
        self.outl = torch.full((max(int(b.On.sum()), 1),), 7, dtype=torch.uint8).cuda()          # 7: "never written"
        torch.cuda.synchronize()

    def ptrs(self):
        return [t.data_ptr() for t in (self.theta, self.tc, self.px, self.pi, self.li, self.outl)]

    def solve(self, slam, **kw):
        import torch
        status, stats = slam.bundle_adjustment_batch_dev_(self.b.cams, self.b.Pn, self.b.Mn, self.b.On, *self.ptrs(), **kw)
        torch.cuda.synchronize()
        return status, stats, self.theta.cpu().numpy(), self.outl.cpu().numpy()


def _residuals(w, theta):
    """squared residual and depth of every observation at theta (RotZYX, x = R X + t; pixels (y, x))"""
    from slam_jl_amd.synthetic import _rot_batch
    P = w["P"]; fx, fy, cx, cy = w["cam"]
    pose = theta[:6 * P].reshape(P, 6); pts = theta[6 * P:].reshape(-1, 3)
    R = _rot_batch(pose[:, :3])
    p, j = w["pose_ids"] - 1, w["point_ids"] - 1
    xc = np.einsum("oij,oj->oi", R[p], pts[j]) + pose[p, 3:]
    ry = w["pixels_yx"][:, 0] - (fy * xc[:, 1] / xc[:, 2] + cy); rx = w["pixels_yx"][:, 1] - (fx * xc[:, 0] / xc[:, 2] + cx)
    return ry * ry + rx * rx, xc[:, 2]


def _assert_margin(slam, wins):
    """the precondition for equal outlier sets (module docstring), on the host form's pass-1 theta"""
    b = _batch(slam, wins)
    st = b.solve(iterations=0, repr_eps=REPR_EPS)
    assert not st.any(), st
    for z, w in enumerate(wins):
        if w["O"] == 0:
            continue
        r2, depth = _residuals(w, b.theta[b.th_off[z]:b.th_off[z + 1]])
        assert (np.abs(r2 - REPR_EPS) > 1e-3 * REPR_EPS).all(), (z, float(np.abs(r2 - REPR_EPS).min()))
        assert (np.abs(depth - 1e-6) > 1e-3 * 1e-6).all(), z
        assert np.array_equal(b.outl[b.ob_off[z]:b.ob_off[z + 1]].astype(bool), (depth < 1e-6) | (r2 > REPR_EPS)), z      # (the residual model above is the solver's)


def _assert_same(ref, z, th, ol, st, tag=""):
    """window z of the host form `ref` (a solved BABatch) against the device form's theta / flags / stats row"""
    rth, rol, rst = ref.window(z)
    assert np.array_equal(ol.astype(bool), rol), (tag, z)
    assert int(st[3]) == rst["iters_pass1"] and int(st[4]) == rst["iters_pass2"], (tag, z, st, rst)
    for a, key in ((st[0], "ssr_init"), (st[1], "ssr_pass1"), (st[2], "ssr_final")):
        assert abs(a - rst[key]) <= 1e-8 * rst[key], (tag, z, key, a, rst[key])
    assert int(st[5]) == rst["n_outliers"]
    assert np.abs(th - rth).max() <= 1e-6 * max(1.0, np.abs(rth).max()), (tag, z, float(np.abs(th - rth).max()))


@pytest.fixture(scope="module")
def main(slam, syn):
    """the shared window set, the host form's solution of it and the device form's, computed once"""
    wins = npd.window_set(syn)
    ref = _batch(slam, wins); st = ref.solve(repr_eps=REPR_EPS)
    assert not st.any(), st
    d = Dev(_batch(slam, wins))
    return dict(wins=wins, ref=ref, dev=d, out=d.solve(slam, repr_eps=REPR_EPS))


def test_staged_arrays_equal_the_model(slam, syn):
    wins = npd.window_set(syn)
    d = Dev(_batch(slam, wins)); b = d.b
    lib = slam.default_context(0).lib; ctx = slam.default_context(0)
    fn = lib.slam_debug_ba_dev_staged
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 10 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
    for z, w in enumerate(wins):
        P, M, O = w["P"], w["M"], w["O"]
        buf = np.zeros(1 << 20, dtype=np.uint8); info = np.zeros(16, dtype=np.int64)
        rc = fn(ctx.h, b.S, b.cams.ctypes.data, b.Pn.ctypes.data, b.Mn.ctypes.data, b.On.ctypes.data, *d.ptrs(), z, buf.ctypes.data, buf.size, info.ctypes.data)
        assert rc == 0, (z, rc, lib.slam_last_error(ctx.h))
        want = npd.stage(P, M, O, w["theta0"], w["theta_const"], w["pixels_yx"], w["pose_ids"], w["point_ids"])
        names = ["pose", "pts", "pconst", "pix", "opose", "opoint", "pt_start", "pt_id", "opk", "pfs", "fobs", "fgrp"]
        got = {}
        for name, off in zip(names, info[:12]):
            ref = want[name]
            got[name] = buf[off:off + ref.nbytes].view(ref.dtype)
            assert np.array_equal(got[name], ref), (z, name)
        assert info[12] <= buf.size and (info[13], info[14], info[15]) == (want["ksplit"], want["p0"], want["nb"]), (z, info[12:], want["ksplit"])
        order = np.concatenate([np.flatnonzero(w["theta_const"] != 0), np.flatnonzero(w["theta_const"] == 0)])      # the documented relabelling, not the model's copy of it
        got.update(ksplit=int(info[13]), p0=int(info[14]), nb=int(info[15]), order=order)
        npd.check_staged(w, got)                      # and the staged arrays describe the window that went in


def test_results_equal_the_host_form(slam, main):
    _assert_margin(slam, main["wins"])
    status, stats, theta, outl = main["out"]
    assert not status.any(), status
    ref = main["ref"]
    for z in range(len(main["wins"])):
        _assert_same(ref, z, theta[ref.th_off[z]:ref.th_off[z + 1]], outl[ref.ob_off[z]:ref.ob_off[z + 1]], stats[z])
        assert outl[ref.ob_off[z]:ref.ob_off[z + 1]].max() <= 1       # every flag was written
        g = main["wins"][z]["gross_outliers"]
        assert outl[ref.ob_off[z]:ref.ob_off[z + 1]][g].all(), z      # the scripted gross outliers are found


def test_ineligible_windows_get_the_code_and_stay_untouched(slam, syn):
    """one free pose among several, six free poses, no observations: SLAM_BA_DEV_INELIGIBLE, arrays bit-unchanged; the one window the kernel takes
    runs alone in its list"""
    wins = npd.ineligible_set(syn)
    _assert_margin(slam, wins[:3])
    ref = _batch(slam, wins[:3]); ref.solve(repr_eps=REPR_EPS)
    d = Dev(_batch(slam, wins))
    status, stats, theta, outl = d.solve(slam, repr_eps=REPR_EPS)
    assert status.tolist() == [INELIGIBLE, INELIGIBLE, 0, INELIGIBLE], status
    b = d.b
    for z in (0, 1, 3):
        assert np.array_equal(theta[b.th_off[z]:b.th_off[z + 1]], b.theta0[b.th_off[z]:b.th_off[z + 1]])
        assert (outl[b.ob_off[z]:b.ob_off[z + 1]] == 7).all() and not stats[z].any()
    _assert_same(ref, 2, theta[b.th_off[2]:b.th_off[3]], outl[b.ob_off[2]:b.ob_off[3]], stats[2])


def test_argument_errors_are_found_on_the_device_and_the_neighbours_solved(slam, syn):
    wins = npd.window_set(syn)
    good_a, good_b = wins[3], wins[4]
    ung = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in wins[4].items()}
    i = int(np.flatnonzero(np.diff(ung["point_ids"]) > 0)[3])                       # the last observation of a point <-> the first of the next
    for key in ("pose_ids", "point_ids"):
        ung[key][[i, i + 1]] = ung[key][[i + 1, i]]
    ung["pixels_yx"][[i, i + 1]] = ung["pixels_yx"][[i + 1, i]]
    tw = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in wins[2].items()}
    fo = np.flatnonzero(tw["theta_const"][tw["pose_ids"] - 1] == 0)
    i = int(fo[5]); j = i + 1 if tw["point_ids"][i + 1] == tw["point_ids"][i] else i - 1
    assert tw["point_ids"][j] == tw["point_ids"][i]
    tw["pose_ids"][j] = tw["pose_ids"][i]                                           # same point, same free pose twice
    batch = [good_a, ung, good_b, tw]
    _assert_margin(slam, [good_a, good_b])
    ref = _batch(slam, [good_a, good_b]); ref.solve(repr_eps=REPR_EPS)
    d = Dev(_batch(slam, batch)); b = d.b
    status, stats, theta, outl = d.solve(slam, repr_eps=REPR_EPS)
    assert status.tolist() == [0, ERR_ARG, 0, ERR_ARG], status
    for z in (1, 3):
        assert np.array_equal(theta[b.th_off[z]:b.th_off[z + 1]], b.theta0[b.th_off[z]:b.th_off[z + 1]]) and (outl[b.ob_off[z]:b.ob_off[z + 1]] == 7).all()
    for z, zr in ((0, 0), (2, 1)):
        _assert_same(ref, zr, theta[b.th_off[z]:b.th_off[z + 1]], outl[b.ob_off[z]:b.ob_off[z + 1]], stats[z])


def test_a_failed_factorisation_leaves_the_device_arrays_unchanged(slam, syn):
    """a NaN map point that a free pose observes poisons the reduced system: SLAM_ERR_NUMERIC, theta and the flags as they were; its neighbour is solved"""
    wins = npd.window_set(syn)[3:5]
    bad = dict(wins[1]); th = bad["theta0"].copy()
    j = int(bad["point_ids"][np.flatnonzero(bad["theta_const"][bad["pose_ids"] - 1] == 0)[0]]) - 1
    th[6 * bad["P"] + 3 * j + 1] = np.nan; bad["theta0"] = th
    _assert_margin(slam, wins[:1])
    ref = _batch(slam, wins[:1]); ref.solve(repr_eps=REPR_EPS)
    d = Dev(_batch(slam, [wins[0], bad])); b = d.b
    status, stats, theta, outl = d.solve(slam, repr_eps=REPR_EPS)
    assert status.tolist() == [0, ERR_NUMERIC], status
    assert np.array_equal(theta[b.th_off[1]:], b.theta0[b.th_off[1]:], equal_nan=True) and (outl[b.ob_off[1]:b.ob_off[2]] == 7).all()
    _assert_same(ref, 0, theta[:b.th_off[1]], outl[:b.ob_off[1]], stats[0])


_KNOB = r'''
import sys, ctypes, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import slam_jl_amd as slam
from slam_jl_amd import synthetic as syn, _lib
import np_ba_dev_stage as npd
import test_gpu_ba_batch_dev as T
wins = npd.window_set(syn)
d = T.Dev(T._batch(slam, wins))
status, stats, theta, outl = d.solve(slam, repr_eps=T.REPR_EPS)
lib = _lib.load(); lib.slam_debug_ba_xretries.restype = ctypes.c_long
print("RETRIES", lib.slam_debug_ba_xretries())
assert not status.any(), status
np.savez(%(out)r, theta=theta, outl=outl, stats=stats)
print("OK")
'''


@pytest.mark.parametrize("tag,env", [("one", {"SLAMHIP_BA_WINDOW_ONE": "1"}), ("giveup", {"SLAMHIP_BA_XWAIT_US": "0"})])
def test_solver_route_knobs_keep_the_results(slam, main, tmp_path, tag, env):
    """one workgroup per window; and the halves of the two-workgroup form giving up at once, so that the call is solved again -- which is right only
    if the windows are staged again (the first attempt moved the parameters inside the staged region)"""
    _assert_margin(slam, main["wins"])
    out = str(tmp_path / (tag + ".npz"))
    r = subprocess.run([sys.executable, "-c", _KNOB % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-800:] + r.stderr[-1500:]
    retries = int(r.stdout.split("RETRIES")[1].split()[0])
    assert (retries >= 1) == (tag == "giveup"), (tag, retries)
    got = np.load(out); ref = main["ref"]
    for z in range(len(main["wins"])):
        _assert_same(ref, z, got["theta"][ref.th_off[z]:ref.th_off[z + 1]], got["outl"][ref.ob_off[z]:ref.ob_off[z + 1]], got["stats"][z], tag)
