"""Scripted key-frame sequences for the key-frame map tests (test helper): per stream a list of key-frames, each a pose Tcw and a keypoint
list (ids ascending, yx, is_3d, xyz) as KeypointSet.download returns it.  Between key-frames some keypoints are dropped and new ones are
appended behind (fresh, larger ids); is_3d is monotone per id.  The geometry is consistent -- world points seen through a pinhole camera that
moves along x, pixels with a fraction of a pixel of noise -- so that the windows are solvable; every number is a function of (seed, id, key-frame).

`sizes` fixes the list length at every key-frame (the GPU test puts 0, 1, 63, 64, 65 and cap there).  A track is born `long` with a
probability of its own: long tracks survive most drops and give old key-frames covisibility with the newest; `p3` of the newborn are 3-D at
birth (a stereo triangulation: the single-observer points of a window), the others are promoted later or never (2-D tracks shared with an old
key-frame give it a covisibility score without a 3-D point: the low-score co-key-frame that is skipped)."""
import numpy as np

CAM = (400.0, 400.0, 320.0, 240.0)
DIST = (-0.02, 0.003, 0.0005, -0.0003)


def _u(seed, *k):
    """a uniform number in [0, 1) from a hash of the integers k (splitmix64 steps)"""
    h = (int(seed) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    for v in k:
        h = (h ^ (int(v) & 0xFFFFFFFFFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF
        h = (h + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        h = ((h ^ (h >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        h = ((h ^ (h >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        h ^= h >> 31
    return (h >> 11) / 9007199254740992.0


def pose(seed, k):
    """Tcw of key-frame k: 0.35 units along x per key-frame, a slow yaw and a little pitch"""
    a, b = 0.012 * k + 0.004 * _u(seed, 901, k), 0.006 * np.sin(0.9 * k)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    T = np.eye(4)
    T[:3, :3] = Rx @ Ry
    T[:3, 3] = -T[:3, :3] @ np.array([0.35 * k, 0.02 * k, 0.05 * k])
    return T


def world_point(seed, i):
    return np.array([-3.0 + 9.0 * _u(seed, 1, i), -2.5 + 5.0 * _u(seed, 2, i), 5.0 + 8.0 * _u(seed, 3, i)])


def make_stream(seed, sizes, p_drop=0.25, p_long=0.25, p3=0.5, p_promote=0.3, purge_at=None):
    """-> [dict(Tcw, ids, yx, is_3d, xyz)] for key-frames 0 .. len(sizes) - 1"""
    alive, next_id, out = [], 0, []                              # alive: [id, is_3d, long]
    for k, n in enumerate(sizes):
        keep = []
        for t in alive:
            if k == purge_at:                                    # only the long 2-D tracks survive: older key-frames keep a score, without a 3-D point
                if t[2] and not t[1]:
                    keep.append(t)
            elif _u(seed, 11, t[0], k) >= (0.04 if t[2] else p_drop):
                keep.append(t)
        while len(keep) > n:                                     # the list length is the script's: drop further, by hash
            keep.pop(int(_u(seed, 12, len(keep), k) * len(keep)))
        for t in keep:
            if not t[1] and not t[2] and _u(seed, 13, t[0], k) < p_promote:       # (a long 2-D track stays 2-D)
                t[1] = True
        while len(keep) < n:
            lng = _u(seed, 14, next_id) < p_long
            keep.append([next_id, _u(seed, 15, next_id) < (0.7 if lng else p3), lng])
            next_id += 1
        alive = keep
        T = pose(seed, k)
        ids = np.array([t[0] for t in alive], dtype=np.int64)
        X = np.array([world_point(seed, i) for i in ids]).reshape(-1, 3)
        Xc = X @ T[:3, :3].T + T[:3, 3]
        yx = np.stack([CAM[1] * Xc[:, 1] / Xc[:, 2] + CAM[3], CAM[0] * Xc[:, 0] / Xc[:, 2] + CAM[2]], axis=1) if len(ids) else np.zeros((0, 2))
        yx = yx + np.array([[0.4 * (_u(seed, 21, i, k) - 0.5), 0.4 * (_u(seed, 22, i, k) - 0.5)] for i in ids]).reshape(-1, 2)
        # the list's map point: the world point with a triangulation error that changes from key-frame to key-frame
        xyz = X + np.array([[0.03 * (_u(seed, 31, i, k) - 0.5), 0.03 * (_u(seed, 32, i, k) - 0.5), 0.08 * (_u(seed, 33, i, k) - 0.5)] for i in ids]).reshape(-1, 3)
        out.append(dict(Tcw=T, ids=ids, yx=np.ascontiguousarray(yx), is_3d=np.array([t[1] for t in alive], dtype=bool), xyz=np.ascontiguousarray(xyz)))
    return out


def outlier_pattern(seed, win):
    """Outlier flags of a gathered window (obs_kf, obs_kp; tracked_ba.gather's dict or np_kfmap's) by a hash of (key-frame, keypoint): about one
    observation in six (two in five outside the covisibility map: there are few), and EVERY observation of the keypoints the hash singles out (about one in thirteen), so that points are removed."""
    kf, kp, cov = np.asarray(win["obs_kf"]), np.asarray(win["obs_kp"]), np.asarray(win["obs_in_covmap"])
    return np.array([_u(seed, 41, a, b) < (0.17 if c else 0.4) or _u(seed, 42, b) < 0.077 for a, b, c in zip(kf, kp, cov)], dtype=bool)


def refined(seed, win):
    """a stand-in for the solver's theta: the window's own, every number moved by a hash of its index (update only copies)"""
    th = np.asarray(win["theta"], dtype=np.float64)
    return th + np.array([1e-3 * (_u(seed, 51, i) - 0.5) for i in range(len(th))])


PURGE_AT = (3, None, None)               # stream 0 loses every track but the long 2-D ones at key-frame 3
# The scenarios both test files run: (name, R, mcap, min_cov_score per stream, sizes per stream).  S = 3, cap = 100.
CAP = 100
SCENARIOS = {
    # nothing is forgotten: 7 key-frames in a ring of 8, ids below mcap
    "plain": dict(R=8, mcap=1024, minc=(8, 12, 6), seeds=(3, 5, 8), dists=(None, DIST, None),
                  sizes=((60, 64, 70, 65, 80, 100, 90), (30, 33, 35, 12, 30, 40, 45), (1, 63, 64, 65, 100, 0, 40))),
    # the ring wraps: 7 key-frames in 4 slots
    "ring": dict(R=4, mcap=1024, minc=(8, 12, 6), seeds=(3, 5, 8), dists=(None, DIST, None),
                 sizes=((60, 64, 70, 65, 80, 100, 90), (30, 33, 35, 12, 30, 40, 45), (1, 63, 64, 65, 100, 0, 40))),
    # the table wraps: fewer entries than the last id
    "table": dict(R=8, mcap=128, minc=(8, 12, 6), seeds=(3, 5, 8), dists=(None, DIST, None),
                  sizes=((60, 64, 70, 65, 80, 100, 90), (30, 33, 35, 12, 30, 40, 45), (1, 63, 64, 65, 100, 0, 40))),
}


def scenario(name):
    sc = SCENARIOS[name]
    return sc, [make_stream(seed, sizes, purge_at=PURGE_AT[s]) for s, (seed, sizes) in enumerate(zip(sc["seeds"], sc["sizes"]))]
