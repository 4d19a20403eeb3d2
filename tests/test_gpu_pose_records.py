"""GPU: the six array seams of the pose stage (slam_p3p_ransac(_batch), slam_five_point_ransac(_batch), slam_pnp_ba(_batch)) through their C
entry points, on point lists made with numpy from a known pose: what crosses the result records (csrc/pose_records.hpp) arrives in the right
output, whichever nullable outputs are given; nothing is written outside an output array (eight guard elements on either side of each); the
"nothing to sample from" results are the documented ones; a batch equals its problems' single calls field for field.
scripts/probes/pose_dump.py runs the same cases and dumps every output, for a byte comparison of two builds of the library."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = [0, 2, 3, 4, 5, 8, 65]
ITERS = [0, 1, 16]
TRIPLES = [(65, 0, 8), (5, 0, 3), (4, 0, 2)]               # S = 3 with the empty problem in the middle; every n of NS appears
G = 8                                                       # guard elements on either side of every output array
SENTINEL = {np.dtype(np.float64): -777.25, np.dtype(np.uint8): 0xA5, np.dtype(np.int32): -12345}
MIN_N = {"p3p": 3, "5pt": 5}                                # fewer points than a sample needs: nothing to sample from

# outputs in the order of the C signature: (name, elements per problem or "n": one per point, dtype, nullable)
f64, u8, i32 = np.float64, np.uint8, np.int32
OUTPUTS = {
    "p3p": [("KP", 12, f64, False), ("Rt", 12, f64, True), ("inliers", "n", u8, False), ("n_inliers", 1, i32, False), ("error", 1, f64, True), ("best_iter", 1, i32, True)],
    "5pt": [("E", 9, f64, True), ("P", 12, f64, False), ("inliers", "n", u8, False), ("n_inliers", 1, i32, False), ("error", 1, f64, True), ("best_iter", 1, i32, True)],
    "pnp": [("pose", 16, f64, False), ("err_init", 1, f64, True), ("err_final", 1, f64, True), ("outliers", "n", u8, False), ("n_outliers", 1, i32, True)],
}
NULLABLE = {seam: [o[0] for o in outs if o[3]] for seam, outs in OUTPUTS.items()}
CAM = (718.856, 718.856, 607.1928, 185.2157)
K = np.array([[CAM[0], 0, CAM[2]], [0, CAM[1], CAM[3]], [0, 0, 1.0]])


def _rotzyx(a, b, c):
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    return np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]]) @ np.array([[1, 0, 0], [0, cc, -sc], [0, sc, cc]])


def problem(n):
    """n map points seen from a known pose (and from a second one, for the two-view seam); every eighth observation is a gross outlier"""
    rng = np.random.default_rng(2300 + n)
    fx, fy, cx, cy = CAM
    R, t = _rotzyx(0.04, -0.07, 0.025), np.array([0.4, -0.15, 0.8])
    u, v, z = rng.uniform(20, 1221, n), rng.uniform(20, 356, n), rng.uniform(4, 50, n)
    Xc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    Xw = (Xc - t) @ R
    px = np.stack([u, v], 1) + rng.normal(0, 0.2, (n, 2))
    px[7::8] += 25.0
    bear = np.stack([(px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy, np.ones(n)], 1)
    R2, t2 = _rotzyx(0.01, -0.03, 0.005), np.array([0.3, -0.05, -1.1])
    X2 = Xc @ R2.T + t2
    px2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], 1) + rng.normal(0, 0.2, (n, 2))
    px2[7::8] += 25.0
    # the refinement is a least-squares fit: its list has few outliers, displaced in alternating directions, so that they do not drag the first pass
    # far enough to flag the good observations as well (the RANSAC lists above carry one outlier in eight, all displaced alike)
    pix = np.stack([v, u], 1) + rng.normal(0, 0.2, (n, 2))
    pix[15::16] += np.where(np.arange(len(pix[15::16])) % 2 == 0, 1.0, -1.0)[:, None] * np.array([9.0, -7.0])
    pose0 = np.eye(4); pose0[:3, :3] = _rotzyx(0.05, -0.082, 0.033); pose0[:3, 3] = t + (0.05, -0.04, 0.08)
    tuples = lambda k: np.stack([rng.permutation(n)[:k] for _ in range(max(ITERS))]).astype(i32) if n >= k else np.full((max(ITERS), k), -1, i32)
    c = np.ascontiguousarray
    return dict(n=n, pts=c(Xw), px=c(px), pdn=c(bear / np.linalg.norm(bear, axis=1, keepdims=True)), s3=tuples(3),
                px1=c(np.stack([u, v], 1)), px2=c(px2), pd1=c((np.stack([u, v], 1) - [cx, cy]) / [fx, fy]), pd2=c((px2 - [cx, cy]) / [fx, fy]), s5=tuples(5),
                pix_yx=c(pix), pose0=pose0)


PROBLEMS = {n: problem(n) for n in NS}


def run(slam, seam, ns, iters, batch, null=()):
    """One call of `seam` on the problems of sizes `ns` (batch: the _batch entry point; else len(ns) == 1).  Returns {output: array} of the outputs
    that were given (not in `null`), S rows each; asserts the return code and that every guard element is untouched."""
    from slam_jl_amd import _lib as L
    ctx = slam.default_context(0)
    probs = [PROBLEMS[n] for n in ns]
    S, ntot = len(probs), sum(ns)
    off = np.concatenate([[0], np.cumsum(ns)]).astype(i32)
    cat = lambda key, w: np.ascontiguousarray(np.concatenate([p[key].reshape(-1, w) for p in probs]))
    bufs, ptrs = {}, []
    for name, cnt, dt, _ in OUTPUTS[seam]:
        m = ntot if cnt == "n" else cnt * S
        bufs[name] = np.full(m + 2 * G, SENTINEL[np.dtype(dt)], dt)
        t = {f64: L.f64p, u8: L.u8p, i32: L.i32p}[dt]
        ptrs.append(None if name in null else bufs[name][G:].ctypes.data_as(t))
    Kf = np.ascontiguousarray(np.stack([K.T] * S))
    if seam == "p3p":
        sm = np.ascontiguousarray(np.stack([p["s3"][:iters] for p in probs]))
        a = (L.ptr(cat("pts", 3)), L.ptr(cat("px", 2)), L.ptr(cat("pdn", 3)))
        rc = (ctx.lib.slam_p3p_ransac_batch(ctx.h, S, L.ptr(off, L.i32p), *a, L.ptr(Kf), 3.0, L.ptr(sm, L.i32p), iters, *ptrs) if batch else
              ctx.lib.slam_p3p_ransac(ctx.h, *a, ntot, L.ptr(Kf), 3.0, L.ptr(sm, L.i32p), iters, *ptrs))
    elif seam == "5pt":
        sm = np.ascontiguousarray(np.stack([p["s5"][:iters] for p in probs]))
        a = (L.ptr(cat("px1", 2)), L.ptr(cat("px2", 2)), L.ptr(cat("pd1", 2)), L.ptr(cat("pd2", 2)))
        rc = (ctx.lib.slam_five_point_ransac_batch(ctx.h, S, L.ptr(off, L.i32p), *a, L.ptr(Kf), L.ptr(Kf), 3.0, L.ptr(sm, L.i32p), iters, *ptrs) if batch else
              ctx.lib.slam_five_point_ransac(ctx.h, *a, ntot, L.ptr(Kf), L.ptr(Kf), 3.0, L.ptr(sm, L.i32p), iters, *ptrs))
    else:
        poses = np.ascontiguousarray(np.stack([p["pose0"].T for p in probs]))      # column-major per problem
        a = (L.ptr(cat("pix_yx", 2)), L.ptr(cat("pts", 3)))
        if batch:
            cams = np.ascontiguousarray(np.tile(CAM, (S, 1)))
            rc = ctx.lib.slam_pnp_ba_batch(ctx.h, S, L.ptr(off, L.i32p), L.ptr(cams), L.ptr(poses), *a, min(iters, 5), iters, 1e-6, 5.0, *ptrs)
        else:
            rc = ctx.lib.slam_pnp_ba(ctx.h, *CAM, L.ptr(poses), *a, ntot, min(iters, 5), iters, 1e-6, 5.0, *ptrs)
    ctx.check(rc)
    out = {}
    for name, cnt, dt, _ in OUTPUTS[seam]:
        b, s = bufs[name], SENTINEL[np.dtype(dt)]
        assert (b[:G] == s).all() and (b[len(b) - G:] == s).all(), (seam, ns, iters, batch, null, name, "guard overwritten")
        inner = b[G:len(b) - G]
        if name in null:
            assert (inner == s).all()
        else:
            out[name] = [inner[off[z]:off[z + 1]].copy() for z in range(S)] if cnt == "n" else list(inner.reshape(S, cnt).copy())
    return out


def call_sets():
    """(ns, batch) of every call shape: each n alone through the single and the batch entry point, and the S = 3 batches"""
    return [((n,), False) for n in NS] + [((n,), True) for n in NS] + [(t, True) for t in TRIPLES]


_single = {}


def single(slam, seam, n, iters):
    """the single-call result of one problem with every output given: computed once, shared"""
    key = (seam, n, iters)
    if key not in _single:
        _single[key] = {k: v[0] for k, v in run(slam, seam, (n,), iters, False).items()}
    return _single[key]


CASES = [(seam, iters) for seam in OUTPUTS for iters in ITERS]
IDS = ["%s-iters%d" % c for c in CASES]


@pytest.mark.parametrize("seam,iters", CASES, ids=IDS)
def test_batch_equals_single_calls_field_for_field(slam, seam, iters):
    for ns, batch in call_sets():
        if not batch:
            continue
        got = run(slam, seam, ns, iters, True)
        for z, n in enumerate(ns):
            want = single(slam, seam, n, iters)
            assert set(got) == set(want)
            for name in want:
                assert got[name][z].dtype == want[name].dtype and np.array_equal(got[name][z], want[name]), (seam, ns, iters, z, name)


@pytest.mark.parametrize("seam,iters", CASES, ids=IDS)
def test_null_outputs_leave_the_given_ones_unchanged(slam, seam, iters):
    for ns, batch in call_sets():
        full = run(slam, seam, ns, iters, batch)
        for name in NULLABLE[seam]:
            got = run(slam, seam, ns, iters, batch, null=(name,))
            assert set(got) == set(full) - {name}
            for k in got:
                for z in range(len(ns)):
                    assert np.array_equal(got[k][z], full[k][z]), (seam, ns, iters, batch, name, k, z)


@pytest.mark.parametrize("seam,iters", [c for c in CASES if c[0] != "pnp"], ids=[i for c, i in zip(CASES, IDS) if c[0] != "pnp"])
def test_nothing_to_sample_from(slam, seam, iters):
    """zero pose (and E), zero mask, 0 inliers, error 0, best_iter == -1 -- from the host's early exit and from the kernels alike"""
    seen = 0
    for ns, batch in call_sets():
        got = run(slam, seam, ns, iters, batch)
        for z, n in enumerate(ns):
            if n >= MIN_N[seam] and iters > 0:
                continue
            seen += 1
            for name, cnt, dt, _ in OUTPUTS[seam]:
                want = np.full(n if cnt == "n" else cnt, -1 if name == "best_iter" else 0, dt)
                assert np.array_equal(got[name][z], want), (seam, ns, iters, batch, z, name, got[name][z])
    assert seen >= 5
    if iters == 16:                                         # and a problem that can be sampled is not empty (one tuple alone may give no pose): the records carry something
        r = single(slam, seam, 65, iters)
        assert r["best_iter"][0] >= 0 and r["n_inliers"][0] > 0 and r["inliers"].sum() == r["n_inliers"][0]


@pytest.mark.parametrize("iters", ITERS)
def test_refinement_of_fewer_than_five_points_is_the_identity(slam, iters):
    """pnp_bundle_adjustment's own exit (fewer than 5 inliers): the identity pose; with 65 points and iterations the pose moves and the error falls"""
    for n in NS:
        r = single(slam, "pnp", n, iters)
        if n < 5:
            assert np.array_equal(r["pose"], np.eye(4).ravel()) and r["n_outliers"][0] >= 0
    r = single(slam, "pnp", 65, iters)
    assert r["outliers"].sum() == r["n_outliers"][0] and np.array_equal(r["pose"][[3, 7, 11, 15]], [0.0, 0.0, 0.0, 1.0])
    if iters == 16:
        assert r["err_final"][0] < r["err_init"][0] and not np.array_equal(r["pose"], np.eye(4).ravel())
