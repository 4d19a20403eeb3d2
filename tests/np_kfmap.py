"""The bounded key-frame map of one stream (test helper; never imported by the product): tests/tracked_ba.py's add_keyframe / is_bad /
covisibility / remove_obs / remove_mappoint / gather / update restated over a ring of R key-frames and a table of mcap points, the layout of
csrc/kfmap.hpp, so that its state compares with slam_kfmap's read-backs array for array.

What the bounds add to tracked_ba.py (mismatch = 0):
  * key-frame k lives in slot k % R; recording into an occupied slot first forgets the old key-frame (remove_keyframe!, map_manager.jl:184-209):
    every point it observed loses that observer;
  * point `id` lives in entry id % mcap; a newer id that lands on an occupied entry replaces it, an older id that finds its entry taken is an
    orphan -- recorded in the slab, without a point, skipped wherever tracked_ba skips `mp is None`;
  * `gone` is a flag of the point's entry (it outlives the point's removal, not the entry's replacement);
  * a window without an observation (the first key-frame) is no window (gather returns None, as for nb_3d < min_cov_score);
  * update() skips a key-frame the ring has forgotten since the gather, and a point whose entry another id holds.
While kf < R and ids < mcap none of these acts and the model equals tracked_ba.Record (tests/test_kfmap_model_host.py)."""
import math

import numpy as np

N_COVISIBLE = 5
F_3D, F_OBS, F_BA, F_GONE, F_DEAD = 1, 2, 4, 8, 16


def theta_of(Tcw):
    """pose_to_angles<4> (csrc/pose_records.hpp): RotZYX angles of Rcw, then tcw"""
    T = np.asarray(Tcw, dtype=np.float64)
    t1 = math.atan2(T[1, 0], T[0, 0]); s1, c1 = math.sin(t1), math.cos(t1)
    return np.array([t1, math.atan2(-T[2, 0], math.sqrt(T[0, 0] * T[0, 0] + T[1, 0] * T[1, 0])),
                     math.atan2(T[0, 2] * s1 - T[1, 2] * c1, T[1, 1] * c1 - T[0, 1] * s1), T[0, 3], T[1, 3], T[2, 3]])


def undistort(cam, dist, yx):
    """undistort_point (camera.jl:98-125) in the arithmetic of undistort_px (csrc/geom_device.hpp)"""
    fx, fy, cx, cy = cam
    k1, k2, p1, p2 = dist
    yx = np.asarray(yx, dtype=np.float64).reshape(-1, 2)
    ny = (yx[:, 0] - cy) / fy; nx = (yx[:, 1] - cx) / fx
    s0 = ny * ny; s1 = nx * nx; r2 = s0 + s1
    rd = (1.0 + k1 * r2) + k2 * (r2 * r2)
    pp = ny * nx
    dtx = 2 * p1 * pp + p2 * (r2 + 2 * s0); dty = p1 * (r2 + 2 * s1) + 2 * p2 * pp
    return np.stack([(rd * ny + dty) * fy + cy, (rd * nx + dtx) * fx + cx], axis=1)


class Map:
    def __init__(self, cap, R, mcap, cam=(1.0, 1.0, 0.0, 0.0), dist=None, min_cov_score=25, theta_fn=theta_of, undistort_fn=undistort):
        self.cap, self.R, self.mcap = cap, R, mcap
        self.cam = tuple(float(v) for v in cam)
        self.dist = None if dist is None or not np.any(dist) else tuple(float(v) for v in dist)
        self.min_cov_score = min_cov_score
        self.theta_fn, self.undistort_fn = theta_fn, undistort_fn
        self.tag = np.full(R, -1, dtype=np.int64); self.theta = np.zeros((R, 6)); self.n = np.zeros(R, dtype=np.int64)
        self.ids = np.zeros((R, cap), dtype=np.int64); self.upx = np.zeros((R, cap, 2)); self.live = np.zeros((R, cap), dtype=bool)
        self.ptag = np.full(mcap, -1, dtype=np.int64); self.xyz = np.zeros((mcap, 3)); self.mask = [0] * mcap
        self.flags = np.zeros(mcap, dtype=np.uint8)
        self.cur = -1

    # ---- look-ups ----
    def entry(self, kpid):
        """the table entry of point kpid, or None (no such point: never recorded, replaced, or removed)"""
        e = int(kpid) % self.mcap
        return e if self.ptag[e] == kpid and not self.flags[e] & F_DEAD else None

    def find_live(self, b, kpid):
        n = int(self.n[b])
        i = int(np.searchsorted(self.ids[b, :n], kpid))
        return i if i < n and self.ids[b, i] == kpid and self.live[b, i] else None

    def observers(self, e):
        return sorted(int(self.tag[b]) for b in range(self.R) if self.mask[e] >> b & 1 and self.tag[b] >= 0)

    def slot(self, kfid):
        b = kfid % self.R
        return b if self.tag[b] == kfid else None

    # ---- read-backs, in the form of slam_kfmap_download_keyframe / _points ----
    def keyframe(self, kfid):
        b = self.slot(kfid)
        if b is None:
            return None
        n = int(self.n[b])
        return dict(theta=self.theta[b].copy(), ids=self.ids[b, :n].copy(), upx=self.upx[b, :n].copy(), live=self.live[b, :n].copy())

    def points(self):
        es = sorted((int(self.ptag[e]), e) for e in range(self.mcap) if self.ptag[e] >= 0 and not self.flags[e] & F_DEAD)
        f = np.array([self.flags[e] for _, e in es], dtype=np.uint8)
        return dict(ids=np.array([i for i, _ in es], dtype=np.int64), xyz=np.array([self.xyz[e] for _, e in es]).reshape(-1, 3),
                    is_3d=(f & F_3D) != 0, observed=(f & F_OBS) != 0, ba=(f & F_BA) != 0, gone=(f & F_GONE) != 0,
                    observers=[tuple(self.observers(e)) for _, e in es])

    def gone(self):
        return tuple(sorted(int(self.ptag[e]) for e in range(self.mcap) if self.ptag[e] >= 0 and self.flags[e] & F_GONE))


def add_keyframe(m, kfid, Tcw, lst):
    ids = np.asarray(lst["ids"], dtype=np.int64)
    yx = np.asarray(lst["yx"], dtype=np.float64).reshape(-1, 2)
    f3, xyz = np.asarray(lst["is_3d"]).astype(bool), np.asarray(lst["xyz"], dtype=np.float64).reshape(-1, 3)
    n, r = len(ids), kfid % m.R
    assert n <= m.cap and np.all(np.diff(ids) > 0)
    if m.tag[r] >= 0 and m.tag[r] != kfid:                       # forget the key-frame whose slot this one takes
        for i in range(int(m.n[r])):
            if m.live[r, i]:
                e = int(m.ids[r, i]) % m.mcap
                if m.ptag[e] == m.ids[r, i]:
                    m.mask[e] &= ~(1 << r)
    m.flags &= np.uint8(~F_OBS & 0xFF)
    skip = np.array([m.ptag[int(i) % m.mcap] == i and bool(m.flags[int(i) % m.mcap] & F_GONE) for i in ids], dtype=bool)
    before = m.ptag.copy()
    dead = (m.flags & F_DEAD) != 0
    for i, sk in zip(ids, skip):                                 # the largest id that maps to an entry owns it
        if not sk:
            e = int(i) % m.mcap
            m.ptag[e] = max(m.ptag[e], i)
    up = yx if m.dist is None else m.undistort_fn(m.cam, m.dist, yx)
    m.tag[r] = kfid; m.theta[r] = m.theta_fn(Tcw); m.n[r] = n; m.cur = kfid
    m.ids[r, :n] = ids; m.upx[r, :n] = up; m.live[r, :n] = ~skip
    for k in range(n):
        i, e = int(ids[k]), int(ids[k]) % m.mcap
        if skip[k] or m.ptag[e] != i:
            continue
        if before[e] != i or dead[e]:                            # a new point
            m.xyz[e] = xyz[k]; m.mask[e] = 1 << r; m.flags[e] = F_OBS | (F_3D if f3[k] else 0)
        else:
            m.mask[e] |= 1 << r
            if f3[k] and not m.flags[e] & F_BA:
                m.xyz[e] = xyz[k]
            m.flags[e] |= F_OBS | (F_3D if f3[k] else 0)


def is_bad(m, e):
    nobs = bin(m.mask[e]).count("1")
    if nobs < 2 and not m.flags[e] & F_OBS and (m.flags[e] & F_3D or nobs == 0):
        m.flags[e] &= np.uint8(~F_3D & 0xFF)
        return True
    return False


def remove_mappoint(m, e):
    kpid = int(m.ptag[e])
    for b in range(m.R):
        if m.mask[e] >> b & 1 and m.tag[b] >= 0:
            i = m.find_live(b, kpid)
            if i is not None:
                m.live[b, i] = False
    m.mask[e] = 0
    m.flags[e] = F_DEAD | (F_GONE if m.flags[e] & (F_OBS | F_GONE) else 0)


def covmap(tag, cov):
    """sorted(cov, reverse=True)[:5]: the at most N_COVISIBLE newest slots of `cov` (slot -> score; tag[b] = the slot's key-frame id), newest first"""
    return sorted(cov, key=lambda b: -tag[b])[:N_COVISIBLE]


def ascending(tag):
    """the slots that hold a key-frame, ascending by key-frame id"""
    return sorted((b for b in range(len(tag)) if tag[b] >= 0), key=lambda b: tag[b])


def meet(order, b):
    """slot b's 1-based pose id: dense, in first-encounter order"""
    if b not in order:
        order[b] = len(order) + 1
    return order[b]


def window_const(tag_b, in_covmap, score, minc):
    return bool(tag_b == 0 or not in_covmap or score < minc)


def gather(m):
    """The window of the newest key-frame -> dict as tracked_ba.gather's (plus what update() needs of the ring), or None"""
    kfid, R, minc = m.cur, m.R, m.min_cov_score
    if kfid < 0:
        return None
    r0 = kfid % R
    nb3, cov = 0, {}
    for i in range(int(m.n[r0])):
        if not m.live[r0, i]:
            continue
        e = m.entry(m.ids[r0, i])
        if e is None:
            continue
        nb3 += bool(m.flags[e] & F_3D)
        for b in range(R):
            if b != r0 and m.mask[e] >> b & 1 and m.tag[b] >= 0:
                cov[b] = cov.get(b, 0) + 1
    if nb3 < minc:
        return None
    cov[r0] = nb3
    co = covmap(m.tag, cov)
    asc = ascending(m.tag)
    order = {}                                                   # slot -> 1-based pose id
    went, bad = {}, []
    pts, obs = [], []                                            # (kpid, entry), (pixel, slot, point id, kpid)
    for rc in co:
        if cov[rc] == 0:
            continue
        if rc not in order and (cov[rc] < minc or m.tag[rc] == 0):
            continue
        for i in range(int(m.n[rc])):
            if not m.live[rc, i]:
                continue
            kpid = int(m.ids[rc, i])
            e = m.entry(kpid)
            if e is None or not m.flags[e] & F_3D or e in went:
                continue
            if is_bad(m, e):
                went[e] = -1; bad.append(kpid)
                continue
            pts.append((kpid, e)); went[e] = len(pts)
            for b in asc:
                if not m.mask[e] >> b & 1:
                    continue
                j = m.find_live(b, kpid)
                if j is None:
                    m.mask[e] &= ~(1 << b)                       # remove_obs of an observation whose pixel is gone
                    continue
                meet(order, b)
                obs.append((m.upx[b, j].copy(), b, len(pts), kpid))
    if not obs:
        return None
    P, M, O = len(order), len(pts), len(obs)
    theta = np.empty(6 * P + 3 * M)
    tconst = np.zeros(P, dtype=np.uint8)
    poses_remap = np.zeros(P, dtype=np.int64)
    for b, o in order.items():
        theta[6 * (o - 1):6 * o] = m.theta[b]
        tconst[o - 1] = window_const(m.tag[b], b in co, cov.get(b, 0), minc)
        poses_remap[o - 1] = m.tag[b]
    for j, (kpid, e) in enumerate(pts):
        theta[6 * P + 3 * j:6 * P + 3 * j + 3] = m.xyz[e]
    return dict(kfid=kfid, theta=theta, theta_const=tconst, pixels=np.array([o[0] for o in obs]).reshape(O, 2),
                poses_ids=np.array([order[o[1]] for o in obs], dtype=np.int64), points_ids=np.array([o[2] for o in obs], dtype=np.int64),
                obs_kf=np.array([m.tag[o[1]] for o in obs], dtype=np.int64), obs_kp=np.array([o[3] for o in obs], dtype=np.int64),
                obs_in_covmap=np.array([o[1] in co for o in obs], dtype=bool), poses_remap=poses_remap,
                points_remap=np.array([p[0] for p in pts], dtype=np.int64), bad=set(bad))


def update(m, win, theta, outliers, lst=None):
    """tracked_ba.update on the bounded map; with `lst` (a downloaded list: ids, is_3d, xyz, ...) returns the list as the device leaves it"""
    P = len(win["poses_remap"])
    for i, k in enumerate(win["poses_remap"]):
        b = m.slot(int(k))
        if b is not None:
            m.theta[b] = theta[6 * i:6 * i + 6]
    for i in np.flatnonzero(np.asarray(outliers, dtype=bool)):
        kf, kp = int(win["obs_kf"][i]), int(win["obs_kp"][i])
        e, b = m.entry(kp), m.slot(kf)
        if win["obs_in_covmap"][i] and b is not None:
            j = m.find_live(b, kp)
            if j is not None:
                m.live[b, j] = False
            if e is not None:
                m.mask[e] &= ~(1 << b)
        if kf == win["kfid"] and e is not None:
            m.flags[e] = (m.flags[e] & np.uint8(~F_OBS & 0xFF)) | F_GONE
    kept = set()
    for i, kp in enumerate(win["points_remap"]):
        e = m.entry(int(kp))
        if e is None:
            continue
        if is_bad(m, e):
            remove_mappoint(m, e)
        else:
            m.xyz[e] = theta[6 * P + 3 * i:6 * P + 3 * i + 3]; m.flags[e] |= F_BA
            kept.add(int(kp))
    for kp in win["bad"]:
        e = m.entry(int(kp))
        if e is not None and is_bad(m, e):
            remove_mappoint(m, e)
    if lst is None:
        return None
    ids = np.asarray(lst["ids"], dtype=np.int64)
    own = np.array([m.ptag[int(i) % m.mcap] == i for i in ids], dtype=bool)
    keep = np.array([not (o and m.flags[int(i) % m.mcap] & F_GONE) for i, o in zip(ids, own)], dtype=bool)
    out = {k: np.asarray(v)[keep].copy() for k, v in lst.items()}
    for k, i in enumerate(out["ids"]):
        if out["is_3d"][k] and int(i) in kept:
            out["xyz"][k] = m.xyz[int(i) % m.mcap]
    return out
