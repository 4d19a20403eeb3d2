"""The case list of the stereo triangulation behind two lenses (test helper): slam_kpset_triangulate_lens's lists, built in numpy, and its model.

The rig: two cameras with different intrinsics and different distortions (CAM1 / DIST1, CAM2 / DIST2: the second set has the opposite tangential
signs), the right camera 0.11 m from the left one (10 cm to the right, 4.6 cm ahead, a yaw of 0.2 degrees).  A keypoint's raw pixels are the lens model
(pdn_to_pixel, csrc/geom_device.hpp) applied to the pinhole projections of a known 3-D point into both cameras.  The reference's undistort_point
(camera.jl:98-125) is that same forward model, so what mapper.jl:162-177 triangulates -- kp.undistorted_pixel / kp.right_undistorted_pixel -- is the
model applied once more; the DLT's point is not the scene's, and nothing here needs it to be.

Candidates are drawn from a seeded generator -- points 1.5 .. 12 m ahead, a share with a row moved by up to 5 px (the reprojection gates), a share
0.1 .. 0.15 m ahead of the left camera (behind the right one's min_depth), a share with the two columns swapped (negative disparity: behind both) --
classified by gates() below, and a list takes, in the generator's order, the first candidates of every class it wants and whose four gate
quantities all lie at least MARGIN from their thresholds.  Then flags: some keypoints are 3-D already, some have no stereo match.

STREAMS: S = 3, cap 64; stream 0 about 40 keypoints, stream 1 none, stream 2 all 64."""
import numpy as np

CAM1, DIST1 = (458.0, 457.0, 367.0, 248.0), (-0.28, 0.07, 2e-4, 2e-5)
CAM2, DIST2 = (460.0, 456.0, 371.0, 245.0), (-0.27, 0.065, -2e-4, -2e-5)
MAX_ERROR, MIN_DEPTH, MARGIN = 3.0, 0.1, 1e-6
S, CAP = 3, 64
SIZES = (40, 0, 64)
CLASSES = ("pass", "depth1", "depth2", "left", "right")     # what a candidate meets, gates in the kernel's order


def rig():
    """T21 (camera 1 -> camera 2) and Twc per stream"""
    a = np.deg2rad(0.2)
    T21 = np.eye(4)
    T21[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    T21[:3, 3] = [-0.1, 0.0, -0.0458]
    Twc = np.tile(np.eye(4), (S, 1, 1))
    for s in range(S):
        b = 0.1 * (s + 1)
        Twc[s, :3, :3] = [[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]]
        Twc[s, :3, 3] = [1.0 + s, -2.0, 0.5 * s]
    return T21, Twc


def lens(cam, dist, yx):
    """pdn_to_pixel(cam, dist, (y - cy) / fy, (x - cx) / fx) in numpy, for building raw pixels"""
    fx, fy, cx, cy = cam
    k1, k2, p1, p2 = dist
    yx = np.asarray(yx, dtype=np.float64).reshape(-1, 2)
    ny, nx = (yx[:, 0] - cy) / fy, (yx[:, 1] - cx) / fx
    s0, s1 = ny * ny, nx * nx
    r2 = s0 + s1
    rd = 1.0 + k1 * r2 + k2 * (r2 * r2)
    p = ny * nx
    dtx = 2 * p1 * p + p2 * (r2 + 2 * s0); dty = p1 * (r2 + 2 * s1) + 2 * p2 * p
    return np.stack([(rd * ny + dty) * fy + cy, (rd * nx + dtx) * fx + cx], axis=1)


def pinhole(cam, X):
    return np.stack([cam[1] * X[:, 1] / X[:, 2] + cam[3], cam[0] * X[:, 0] / X[:, 2] + cam[2]], axis=1)


def undistorted(orc, cam, dist, yx):
    """orc.undistort_point of every row"""
    return np.array([orc.undistort_point(cam, dist, p) for p in np.asarray(yx, dtype=np.float64).reshape(-1, 2)]).reshape(-1, 2)


def gates(orc, T21, u1, u2):
    """the four gate quantities of mapper.jl:160-176 for undistorted pairs, from the oracle's DLT point with every gate open:
    -> (z1, z2, d1, d2, cls): depths in both cameras, reprojection distances, and the first gate that fails ("pass": none)"""
    from slam_jl_amd.triangulation import projection_matrices
    P1, P2 = projection_matrices(CAM1, CAM2, T21)
    X, ok = orc.triangulate(P1, P2, T21, CAM1, CAM2, u1, u2, max_error=1e300, min_depth=-1e300)
    assert ok.all()
    R = X @ T21[:3, :3].T + T21[:3, 3]
    with np.errstate(all="ignore"):
        d1 = np.linalg.norm(u1 - pinhole(CAM1, X), axis=1); d2 = np.linalg.norm(u2 - pinhole(CAM2, R), axis=1)
    cls = np.where(X[:, 2] < MIN_DEPTH, "depth1", np.where(R[:, 2] < MIN_DEPTH, "depth2", np.where(d1 > MAX_ERROR, "left", np.where(d2 > MAX_ERROR, "right", "pass"))))
    return X[:, 2], R[:, 2], d1, d2, cls


def margin_of(z1, z2, d1, d2):
    """the smallest distance of the four gate quantities from their thresholds (NaN where one of them is not a number)"""
    return np.minimum(np.minimum(np.abs(z1 - MIN_DEPTH), np.abs(z2 - MIN_DEPTH)), np.minimum(np.abs(d1 - MAX_ERROR), np.abs(d2 - MAX_ERROR)))


def candidates(seed, n):
    """-> raw left pixels, raw right pixels (n, 2) each"""
    rng = np.random.default_rng(seed)
    T21, _ = rig()
    kind = rng.random(n)
    X = np.stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-0.8, 0.8, n), rng.uniform(1.5, 12.0, n)], axis=1)
    near = (kind >= 0.55) & (kind < 0.7)                       # a hand's breadth ahead of the left camera: the right one, 4.6 cm ahead, has it too close
    X[near] = np.stack([rng.uniform(0.01, 0.05, int(near.sum())), rng.uniform(-0.02, 0.02, int(near.sum())), rng.uniform(0.1, 0.15, int(near.sum()))], axis=1)
    p1 = lens(CAM1, DIST1, pinhole(CAM1, X)); p2 = lens(CAM2, DIST2, pinhole(CAM2, X @ T21[:3, :3].T + T21[:3, 3]))
    moved = (kind >= 0.25) & (kind < 0.55)                      # a row moved by up to 5 px, in the left or in the right image
    side = rng.random(n) < 0.5
    dy = rng.uniform(-5.0, 5.0, n)
    p1[moved & side, 0] += dy[moved & side]; p2[moved & ~side, 0] += dy[moved & ~side]
    swapped = kind >= 0.7                                       # the columns exchanged: negative disparity, the rays meet behind the cameras
    swapped &= kind < 0.8
    p1[swapped, 1], p2[swapped, 1] = p2[swapped, 1].copy(), p1[swapped, 1].copy()
    return p1, p2


def build(orc, dists=(DIST1, DIST2), seed=77):
    """-> per stream dict(yx, stereo_yx, is_3d, has_stereo, xyz, cls, margin): the lists to upload and, per keypoint, the class and the margin under
    `dists` (the lenses the call is given; the raw pixels are always made with DIST1 / DIST2)"""
    T21, _ = rig()
    out = []
    for s, n in enumerate(SIZES):
        p1, p2 = candidates(seed + s, 40 * max(n, 1))
        z1, z2, d1, d2, cls = gates(orc, T21, undistorted(orc, CAM1, dists[0], p1), undistorted(orc, CAM2, dists[1], p2))
        margin = margin_of(z1, z2, d1, d2)
        want = {c: (n - 16 if c == "pass" else 4) for c in CLASSES}          # four of every failing class, the rest pass
        take = []
        for i in range(len(cls)):
            if len(take) < n and margin[i] >= MARGIN and np.isfinite(margin[i]) and want[cls[i]] > 0:
                want[cls[i]] -= 1; take.append(i)
        take = np.array(sorted(take), dtype=np.int64)
        assert len(take) == n, (s, want)
        rng = np.random.default_rng(seed + 100 + s)
        is3 = rng.random(n) < 0.15
        has = rng.random(n) >= 0.12
        xyz = np.where(is3[:, None], rng.uniform(-5, 5, (n, 3)), 0.0)
        out.append(dict(yx=p1[take], stereo_yx=p2[take], is_3d=is3, has_stereo=has, xyz=xyz, cls=cls[take], margin=margin[take]))
    return out


def model(orc, lst, Twc, dists=(DIST1, DIST2)):
    """slam_kpset_triangulate_lens on one list: the C oracle's stereo triangulation fed with orc.undistort_point of both pixels
    -> (is_3d, has_stereo, xyz, acted: the keypoints that were triangulated)"""
    from slam_jl_amd.triangulation import projection_matrices
    T21, _ = rig()
    P1, P2 = projection_matrices(CAM1, CAM2, T21)
    cand = lst["has_stereo"] & ~lst["is_3d"]
    is3, has, xyz = lst["is_3d"].copy(), lst["has_stereo"].copy(), lst["xyz"].copy()
    if cand.any():
        X, ok = orc.triangulate(P1, P2, T21, CAM1, CAM2, undistorted(orc, CAM1, dists[0], lst["yx"][cand]), undistorted(orc, CAM2, dists[1], lst["stereo_yx"][cand]),
                                MAX_ERROR, MIN_DEPTH)
        idx = np.flatnonzero(cand)
        is3[idx[ok]] = True; has[idx[~ok]] = False
        xyz[idx[ok]] = X[ok] @ Twc[:3, :3].T + Twc[:3, 3]
    return is3, has, xyz, cand
