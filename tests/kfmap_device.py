"""The device key-frame map beside its numpy model (test helper): the one driver of the tests/test_gpu_kfmap_*.py files that run a scripted `*Run`
model class (tests/kfmap_*_scripts.py) with a slam KeyframeMap + KeypointSet through the same steps and compare every read-back after each.

DeviceSide is a mixin: `class Dev(DeviceSide, rs.RowsRun)`.  It creates the device objects from the run's own S / cap / R / mcap, overrides the
run's steps (add, match, merge, ba) so that each also runs on the device and is checked against the model, and holds the checkers.  The checkers
are plain functions of (km, ks, models, ...) as well, for the hand-built cases that have no run; tests/test_kfmap_device_check_host.py runs them on
the CPU against a stand-in device made from the model, clean and with one field changed at a time.

Every comparison is array_equal unless a tolerance is passed: upx_tol / px_tol / proj_tol are for a map behind a lens, whose undistorted pixels
and projections the device forms in its own arithmetic.  A key-frame's angles are computed on the device too: hand_over_theta holds them to
ANGLE_TOL once and gives the device's bits to the model, so that everything later -- windows included -- compares exactly.

Importing this module needs neither torch nor a GPU; torch is imported in DeviceSide's constructor."""
import numpy as np
import pytest

import kfmap_lmm_scripts as ls
import np_kfmap_local_map as nl
import np_kfmap_rows as nr

ANGLE_TOL = 1e-12                        # a key-frame's angles: atan2 of the device against numpy's
PX_TOL = 1e-9                            # px: pixels and projections behind a lens
DCAP = 64                                # rows per stream of the descriptor block add() hands over
POINT_KEYS = ("ids", "xyz", "is_3d", "observed", "ba", "gone")
LIST_KEYS = ("ids", "yx", "is_3d", "xyz")
STAGED_KEYS = ("lm_ids", "kp_ids", "best_kp", "best_dist")


def within(a, b, tol):
    """array_equal where tol == 0, else the same shape and every element within tol"""
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b) if tol == 0 else a.shape == b.shape and bool(np.all(np.abs(a - b) <= tol))


def hand_over_theta(km, m, s, k):
    """key-frame k of stream s: translation exactly, angles within ANGLE_TOL; the device's bits then become model m's"""
    th, ref = km.download_keyframe(s, k)["theta"], m.theta[k % m.R]
    assert np.array_equal(th[3:], ref[3:]) and np.all(np.abs(th[:3] - ref[:3]) <= ANGLE_TOL), (s, k)
    m.theta[k % m.R] = th


def upload_descriptors(torch, km, S, dcap, per_stream):
    """km.add_descriptors of {stream: (first id, rows)}; the other streams announce three rows of an id the map never held: they must not be taken"""
    desc = np.full((S, dcap, 4), 0x5555555555555555, dtype=np.uint64)
    info = np.tile(np.array([10 ** 6, 3], dtype=np.int64), (S, 1))
    for s, (first, rows) in per_stream.items():
        info[s] = (first, len(rows)); desc[s, :len(rows)] = rows
    desc_dev = torch.from_numpy(desc.view(np.int64)).cuda(); info_dev = torch.from_numpy(info).cuda()
    km.add_descriptors(desc_dev.data_ptr(), info_dev.data_ptr(), dcap)
    km.ctx.synchronize()                                         # (the tensors live until the kernel has read them)


def stored_set(km, s, k):
    """local_map_ids of key-frame k of stream s, or the error's text"""
    try:
        return km.local_map_ids(s, k)
    except Exception as e:                                       # noqa: BLE001 (SlamHipError; the stand-in device raises its own)
        return str(e)


def check_set(km, m, H, s, k):
    """the stored local map of key-frame k of stream s against the model's history H: the set, or one of the two accepted error texts"""
    got, want = stored_set(km, s, k), H.ids(m, k)
    if want is None:
        assert isinstance(got, str) and ("not in the ring" in got or "no local map was stored" in got), (s, k, got)
    else:
        assert not isinstance(got, str) and got.dtype == np.int64 and np.array_equal(got, want), (s, k)


def check_sets(km, models, nkf, H):
    """check_set for every key-frame id the ring can hold, one past the newest included"""
    for s, m in enumerate(models):
        for k in range(max(nkf[s] - m.R, 0), nkf[s] + 1):
            check_set(km, m, H[s], s, k)


def check_map(km, ks, models, lists=None, nkf=None, upx_tol=0.0, pixels=None, rows=None, sets=None):
    """Every ring slot from max(nkf - R, 0) through ONE PAST the newest key-frame (present or absent on both sides), the points and the live lists
    of every stream against the models.  nkf: key-frames recorded per stream (default m.cur + 1); pixels(s, k): the model's raw pixels where the
    store is on; rows[s]: the model's descriptor dict where the row store is on; sets[s]: the model's History where the history is on."""
    for s, m in enumerate(models):
        n = m.cur + 1 if nkf is None else nkf[s]
        for k in range(max(n - m.R, 0), n + 1):
            d, w = km.download_keyframe(s, k), m.keyframe(k)
            assert (d is None) == (w is None), (s, k)
            if pixels is not None:
                px, wpx = km.keyframe_pixels(s, k), pixels(s, k)
                assert (px is None) == (wpx is None) == (w is None), (s, k)
                assert px is None or (px.shape == (len(w["ids"]), 2) and np.array_equal(px, wpx)), (s, k)
            if sets is not None:
                check_set(km, m, sets[s], s, k)
            if w is not None:
                assert all(np.array_equal(d[key], w[key]) for key in ("theta", "ids", "live")) and within(d["upx"], w["upx"], upx_tol), (s, k)
        d, w = km.download_points(s), m.points()
        assert all(np.array_equal(d[key], w[key]) for key in POINT_KEYS) and d["observers"] == w["observers"], s
        if ks is not None and lists is not None and lists[s] is not None:
            d = ks.download(s)
            assert len(d["ids"]) == len(lists[s]["ids"]) and all(np.array_equal(d[key], lists[s][key]) for key in LIST_KEYS), s
        if rows is not None:
            assert nr.same_rows(km.descriptor_rows(s), nr.descriptor_rows(m, rows[s])), s


def check_staged(km, want, streams, proj_tol=0.0):
    """what the last local_map_match staged for `streams` (debug_local_map) against the model's results"""
    for s in streams:
        d, w = km.debug_local_map(s), want[s]
        assert all(np.array_equal(d[key], w[key]) for key in STAGED_KEYS), s
        assert np.array_equal(np.isnan(d["proj_yx"]), np.isnan(w["proj_yx"])), s
        ok = ~np.isnan(w["proj_yx"])
        assert within(d["proj_yx"][ok], w["proj_yx"][ok], proj_tol), s


def check_merge(got, want):
    """the (S, 4) counts of a merge: applied, skipped, renamed, status"""
    assert np.array_equal(got, want), (got, want)


def device_bytes(km, ks, streams, nkf, staged=True, sets=False):
    """what can be read back of the streams' share of the allocations, as bytes: the points, the live list, every key-frame id up to one past the
    newest, optionally the staged lists and the stored sets"""
    out = []
    for s in streams:
        d = [km.download_points(s), ks.download(s)] + [km.download_keyframe(s, k) for k in range(nkf[s] + 1)] + ([km.debug_local_map(s)] if staged else [])
        kept = [(k, v if isinstance(v, str) else v.tobytes()) for k in range(nkf[s] + 1) for v in [stored_set(km, s, k)]] if sets else []
        out.append(repr([(sorted((k, np.asarray(v).tobytes() if not isinstance(v, list) else repr(v)) for k, v in x.items()) if x is not None else None) for x in d]) + repr(kept))
    return out


def assemble(p, s):
    """the arrays of the host-array path from DOWNLOADS of stream s's map -- download_keyframe for ids and live bytes, the pixels the match reads
    (keyframe_pixels where the raw-pixel store is on, else upx), download_points -- and the script's descriptor rows, stated on dicts and sets ->
    (problem = (frame, keypoints, keyframes, local_map, params), the local-map ids, the keypoint ids); None where there is nothing to match"""
    cur, R = int(p.km.newest()[s]), p.m[s].R
    kfs = {k: d for k in range(max(cur - R + 1, 0), cur + 1) for d in [p.km.download_keyframe(s, k)] if d is not None}
    px = {k: p.km.keyframe_pixels(s, k) if p.has_pixels else d["upx"] for k, d in kfs.items()}
    pts = p.km.download_points(s)
    point = {int(i): j for j, i in enumerate(pts["ids"])}
    rows = p.script_rows[s]
    live = {k: {int(i): tuple(q) for i, q, lv in zip(d["ids"], px[k], d["live"]) if lv} for k, d in kfs.items()}
    if cur not in kfs:
        return None
    cov = set()
    for i in live[cur]:
        if i in point:
            cov |= {o for o in pts["observers"][point[i]] if o != cur and o in kfs}
    lm = sorted({i for o in cov for i in live[o] if i in point and pts["is_3d"][point[i]] and i in rows and cur not in pts["observers"][point[i]]})
    order = sorted(kfs)
    row = {k: j for j, k in enumerate(order)}
    kp_ids = [i for i in live[cur] if i in point and i in rows]
    if not cov or not lm or not kp_ids:
        return None
    keypoints = [{"pixel": live[cur][i], "descriptors": rows[i].reshape(1, 4),
                  "observers": [(row[o], live[o][i]) for o in pts["observers"][point[i]] if o in kfs and i in live[o]]} for i in kp_ids]
    local_map = [{"position": pts["xyz"][point[i]], "descriptors": rows[i].reshape(1, 4), "observers": [row[o] for o in pts["observers"][point[i]] if o in kfs]} for i in lm]
    nb3 = sum(1 for i in live[cur] if i in point and pts["is_3d"][point[i]])
    frame = {"Tcw": nl.tcw_of(kfs[cur]["theta"]), "cam": p.cam, "cell_size": ls.CELL, "nb_3d_kpts": nb3}
    return (frame, keypoints, np.array([nl.tcw_of(kfs[k]["theta"]) for k in order]), local_map, ls.PARAMS), lm, kp_ids


class DeviceSide:
    """The device map with its keypoint set beside a `*Run`'s models, driven by the same scripted steps.  Class attributes a file may set: dcap;
    device_pairs (merge() takes the pairs where the last match left them in HBM); the tolerances of a map behind a lens."""
    dcap = DCAP
    device_pairs = False
    cam = ls.CAM10                       # the camera of the match (a run behind a lens has its own)
    upx_tol = px_tol = proj_tol = 0.0
    has_pixels = False

    def __init__(self, slam, *args, descriptors=True, descriptor_rows=None, lm_history=False, **kw):
        import torch
        self.torch, self.slam = torch, slam
        super().__init__(*args, **kw)
        m, S = self.m[0], len(self.m)
        self.ks = slam.KeypointSet(S, m.cap)
        self.km = slam.KeyframeMap(S, m.cap, R=m.R, mcap=m.mcap)
        if descriptors:
            self.km.enable_descriptors()
        if descriptor_rows is not None:
            self.km.enable_descriptor_rows(descriptor_rows)
        if lm_history:
            self.km.enable_local_map_history()
        self.has_descriptors, self.has_rows, self.has_history = descriptors, descriptor_rows is not None, lm_history
        self.Tcw = np.tile(np.eye(4), (S, 1, 1))
        self.script_rows = [dict() for _ in range(S)]            # id -> row, as the script handed them out (assemble()'s descriptors)
        self.dev_counts = self.dev_wins = None

    def close(self):
        self.km.close(); self.ks.close()

    @property
    def kset(self):
        """the keypoint set where the run's lists follow the map's steps, else None"""
        return self.ks if getattr(self, "mode", None) == "follow" else None

    # ---- add_keyframe + add_descriptors ----
    def upload_descriptors(self, per_stream, dcap):
        for s, (first, rows) in per_stream.items():
            self.script_rows[s].update({int(first) + j: r for j, r in enumerate(rows)})
        upload_descriptors(self.torch, self.km, len(self.m), dcap, per_stream)

    def device_add(self, frames, mask, cam4, dist, per_stream_desc=None):
        """frames {s: list}: uploaded, made a key-frame and recorded for the streams of `mask`; per_stream_desc {s: (first id, rows)} or None"""
        S = len(self.m)
        for s, f in frames.items():
            self.ks.upload(s, f["yx"], f["is_3d"], f["xyz"], f["ids"])
            self.Tcw[s] = f["Tcw"]
        sp = self.slam.stream_params(S, Tcw=self.Tcw, cam=cam4, dist=np.tile(np.zeros(4) if dist is None else np.array(dist), (S, 1)))
        with self.ks.selected(mask):
            self.ks.keyframe()
            self.km.add_keyframe(self.ks, sp)
            if per_stream_desc is not None:
                self.upload_descriptors(per_stream_desc, self.dcap)
        for s in frames:
            hand_over_theta(self.km, self.m[s], s, self.nkf[s] - 1)

    def took_parts(self, took):
        """the model's add() result {s: (list, (first id, rows))} -> (lists, descriptors)"""
        return {s: t[0] for s, t in took.items()}, ({s: t[1] for s, t in took.items()} if self.has_descriptors else None)

    def add(self, mask=None):
        took = super().add(mask)
        frames, desc = self.took_parts(took)
        self.device_add(frames, mask, self.m[0].cam, self.m[0].dist, desc)
        return took

    # ---- local_map_match ----
    def device_match(self, **kw):
        return self.km.local_map_match(self.cam, ls.CELL, ls.PARAMS.max_projection_distance, ls.PARAMS.max_descriptor_distance, **kw)

    def check_match(self, got, want, staged=True):
        status, pairs, dist = got
        assert list(status) == [w["status"] for w in want]
        assert all(w["margin"] >= 1e-9 for w in want)
        for s, w in enumerate(want):
            assert pairs[s].dtype == np.int64 and np.array_equal(pairs[s], w["pairs"]) and np.array_equal(dist[s], w["dist"]), s
        if staged:
            check_staged(self.km, want, [s for s in range(len(want)) if self.sel[s]], self.proj_tol)
        if self.has_history:
            check_sets(self.km, self.m, self.nkf, self.H)

    def match(self, max_local=None, **kw):
        """the model's match, the device's checked against it: results, staged lists, stored sets"""
        want = super().match(max_local=max_local, **kw)
        self.check_match(self.device_match(max_local=max_local), want)
        return want

    # ---- merge ----
    def merge(self, pairs, device_pairs=None, **kw):
        want = super().merge(pairs, **kw).copy()
        on_device = self.device_pairs if device_pairs is None else device_pairs
        self.dev_counts = self.km.merge(self.kset, None if on_device else [np.asarray(p, dtype=np.int64).reshape(-1, 2) for p in pairs])
        check_merge(self.dev_counts, want)
        return want

    # ---- gather + update ----
    def device_gather(self, ref):
        """the device's windows, checked against the model's `ref` {stream: window}"""
        wins, status = self.km.gather(np.full(len(self.m), self.m[0].min_cov_score, dtype=np.int32))
        self.check_windows(wins, status, ref)
        self.dev_wins = wins

    def check_windows(self, wins, status, ref):
        """ten arrays with their dtypes and the status vector; pixels within px_tol where they come through the device's undistort_px.  (The
        poses' angles are the device's own bits: add() gave them to the model.)"""
        assert list(status) == [3 if not self.sel[s] else (0 if s in ref else 1) for s in range(len(self.m))]
        assert [w.stream for w in wins] == sorted(ref)
        for w in wins:
            r, c = ref[w.stream], w.cache
            for a, b in ((c.theta_const, r["theta_const"]), (c.poses_ids, r["poses_ids"]), (c.points_ids, r["points_ids"]), (w.poses_remap, r["poses_remap"]),
                         (w.points_remap, r["points_remap"]), (w.obs_kf, r["obs_kf"]), (w.obs_kp, r["obs_kp"]), (w.obs_in_covmap, r["obs_in_covmap"]),
                         (c.theta, r["theta"])):
                assert a.dtype == b.dtype and np.array_equal(a, b), w.stream
            assert c.pixels.dtype == r["pixels"].dtype and within(c.pixels, r["pixels"], self.px_tol), w.stream
            assert len(r["poses_remap"]) >= 1 and c.poses_ids.min() >= 1 and c.points_ids.min() >= 1

    def device_update(self, sols):
        """sols {stream: (theta, outliers)} for the windows of the last device_gather"""
        self.km.update(self.dev_wins, [sols[w.stream][0] for w in self.dev_wins], [sols[w.stream][1] for w in self.dev_wins], ks=self.kset)

    def ba(self):
        """-> the model's {stream: (window, theta, outliers)}, applied on both sides"""
        sol = super().ba()
        self.device_gather({s: v[0] for s, v in sol.items()})
        self.device_update({s: v[1:] for s, v in sol.items()})
        return sol

    # ---- the read-backs ----
    def check(self):
        """every ring slot, the points, the live lists and the enabled stores of every stream against the models"""
        check_map(self.km, self.ks, self.m, getattr(self, "lists", None), self.nkf, self.upx_tol, self.pixels if self.has_pixels else None,
                  self.D if self.has_rows else None, self.H if self.has_history else None)

    def device_bytes(self, streams, staged=True):
        return device_bytes(self.km, self.ks, streams, self.nkf, staged, self.has_history)


def device_fixture(cls, name, through=None):
    """the fixture `name`: a factory of cls(slam, ...) whose products are closed at teardown.  through(*a, cls=..., **kw) -> (run, ...): a
    script's own maker (kfmap_tri_scripts.make) that builds the run from the class it is given."""
    @pytest.fixture(name=name)
    def fixture(slam):
        made = []

        def make(*a, **kw):
            if through is None:
                made.append(cls(slam, *a, **kw))
                return made[-1]
            out = through(*a, cls=lambda **k: cls(slam, **k), **kw)
            made.append(out[0])
            return out
        yield make
        for p in made:
            p.close()
    return fixture
