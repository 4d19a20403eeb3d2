"""The key-frame map of S lock-stepped streams in HBM (slam_kfmap, include/slamhip.h): what local_bundle_adjustment!
(src/estimator.jl:317-347) reads and writes of the map manager -- _get_ba_parameters (:143-266), _update_ba_parameters! (:268-306) -- for
streams whose keypoints live in a KeypointSet.  add_keyframe() fills it from the lists, gather() returns the windows of the newest
key-frames as LocalBACaches for bundle_adjustment_batch_, update() takes the solution back into the map and the live lists."""
import ctypes as C
import time
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from .bundle_adjustment import LocalBACache
from .keypoint_set import KP_PAR

N_COVISIBLE = 5                         # local_bundle_adjustment!: up to 5 latest covisible key-frames


def _per_stream(x, dtype, S, width=None):
    """a per-stream argument as the C seam takes it: a contiguous (S,) or (S, width) array; a scalar (or one row) stands for every stream"""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=dtype), (S,) if width is None else (S, width)))


class _Windows(C.Structure):
    """slam_kfmap_windows"""
    _fields_ = [("cap_windows", C.c_int32), ("cap_poses", C.c_int32), ("cap_points", C.c_int32), ("cap_obs", C.c_int32),
                ("status", L.i32p), ("win_stream", L.i32p), ("Pn", L.i32p), ("Mn", L.i32p), ("On", L.i32p),
                ("theta", L.f64p), ("theta_const", L.u8p), ("pixels_yx", L.f64p), ("pose_ids", L.i64p), ("point_ids", L.i64p),
                ("poses_remap", L.i64p), ("points_remap", L.i64p), ("obs_kf", L.i64p), ("obs_kp", L.i64p), ("obs_in_covmap", L.u8p)]


@dataclass
class Window:
    """One gathered window: the solver's arrays (cache) and the bookkeeping that names them -- poses_remap / points_remap: the key-frame /
    keypoint id of a dense id; per observation its key-frame, keypoint and whether the key-frame is in the covisibility map."""
    stream: int
    cache: LocalBACache
    poses_remap: np.ndarray
    points_remap: np.ndarray
    obs_kf: np.ndarray
    obs_kp: np.ndarray
    obs_in_covmap: np.ndarray


class KeyframeMap:
    def __init__(self, S, cap, R=32, mcap=16384, ctx=None):
        self.ctx = ctx or L.default_context()
        self.S, self.cap, self.R, self.mcap = S, cap, R, mcap
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.slam_kfmap_create(self.ctx.h, S, cap, R, mcap, C.byref(h)))
        self.h = h
        self.last_gather_ms = 0.0
        self._bufs = None

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.slam_kfmap_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_keyframe(self, ks, sp, ctx=None):
        """Record the key-frame ks.keyframe() has just made, for the streams ks has selected.  sp: stream_params(...) with Tcw and the camera /
        distortion entries filled.  Enqueue-only."""
        c = ctx or self.ctx
        sp = np.ascontiguousarray(sp, dtype=np.float64).reshape(self.S, KP_PAR)
        c.check(c.lib.slam_kfmap_add_keyframe(c.h, self.h, ks.h, L.ptr(sp)))

    def gather(self, min_cov_score, max_poses=None, max_points=None, max_obs=None, max_windows=None, ctx=None):
        """-> (windows, status): the Window of every stream of the last add_keyframe that has one, ascending by stream, and the (S,) status
        codes (0 window, 1 none, 2 does not fit the capacities, 3 not selected).  min_cov_score: one threshold or S of them; max_*: the total
        capacities of the arrays the windows are gathered into (default: what S windows can at most need).  Synchronous."""
        c = ctx or self.ctx
        S = self.S
        minc = _per_stream(min_cov_score, np.int32, S)
        nW = S if max_windows is None else int(max_windows)
        nP = S * self.R if max_poses is None else int(max_poses)
        nM = S * min(self.mcap, N_COVISIBLE * self.cap) if max_points is None else int(max_points)
        nO = min(nM * self.R, 4_000_000) if max_obs is None else int(max_obs)
        if self._bufs is None or self._bufs[0] != (nW, nP, nM, nO):     # the arrays the library fills: made once per capacity, reused by every gather
            i32, i64 = (lambda n: np.zeros(max(n, 1), dtype=np.int32)), (lambda n: np.zeros(max(n, 1), dtype=np.int64))
            self._bufs = ((nW, nP, nM, nO), (i32(S), i32(nW), i32(nW), i32(nW), i32(nW), np.zeros(max(6 * nP + 3 * nM, 1)), np.zeros(max(nP, 1), dtype=np.uint8),
                                            np.zeros(max(2 * nO, 1)), i64(nO), i64(nO), i64(nP), i64(nM), i64(nO), i64(nO), np.zeros(max(nO, 1), dtype=np.uint8)))
        status, ws, Pn, Mn, On, theta, tc, px, pi, li, pr, lr, okf, okp, oc = self._bufs[1]
        out = _Windows(nW, nP, nM, nO, L.ptr(status, L.i32p), L.ptr(ws, L.i32p), L.ptr(Pn, L.i32p), L.ptr(Mn, L.i32p), L.ptr(On, L.i32p),
                       L.ptr(theta), L.ptr(tc, L.u8p), L.ptr(px), L.ptr(pi, L.i64p), L.ptr(li, L.i64p), L.ptr(pr, L.i64p), L.ptr(lr, L.i64p),
                       L.ptr(okf, L.i64p), L.ptr(okp, L.i64p), L.ptr(oc, L.u8p))
        n = C.c_int32(0)
        t0 = time.perf_counter()
        c.check(c.lib.slam_kfmap_ba_gather(c.h, self.h, L.ptr(minc, L.i32p), C.byref(out), C.byref(n)))
        self.last_gather_ms = (time.perf_counter() - t0) * 1e3   # wall time of the synchronous call itself (scripts/probes/prof_kfmap.py)
        wins, t0, p0, m0, o0 = [], 0, 0, 0, 0
        for w in range(n.value):
            P, M, O = int(Pn[w]), int(Mn[w]), int(On[w])
            cache = LocalBACache(theta[t0:t0 + 6 * P + 3 * M].copy(), tc[p0:p0 + P].copy(), px[2 * o0:2 * (o0 + O)].reshape(O, 2).copy(),
                                 pi[o0:o0 + O].copy(), li[o0:o0 + O].copy())
            wins.append(Window(int(ws[w]), cache, pr[p0:p0 + P].copy(), lr[m0:m0 + M].copy(), okf[o0:o0 + O].copy(), okp[o0:o0 + O].copy(),
                               oc[o0:o0 + O].astype(bool)))
            t0 += 6 * P + 3 * M; p0 += P; m0 += M; o0 += O
        return wins, status.copy()

    def update(self, windows, thetas=None, outliers=None, ks=None, ctx=None):
        """_update_ba_parameters! for the pending windows of the listed streams.  windows: Windows (or stream indices); thetas / outliers: one
        array per window, default the windows' caches as bundle_adjustment_batch_ left them.  ks: the KeypointSet whose live lists follow
        (refined positions in, removed ids out).  Enqueue-only."""
        c = ctx or self.ctx
        streams = np.ascontiguousarray([w.stream if isinstance(w, Window) else int(w) for w in windows], dtype=np.int32)
        if thetas is None:
            thetas = [w.cache.theta for w in windows]
        if outliers is None:
            outliers = [w.cache.outliers for w in windows]
        th = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.float64).reshape(-1) for t in thetas] + [np.zeros(1)]))
        ol = np.ascontiguousarray(np.concatenate([np.asarray(o).astype(np.uint8).reshape(-1) for o in outliers] + [np.zeros(1, dtype=np.uint8)]))
        c.check(c.lib.slam_kfmap_ba_update(c.h, self.h, ks.h if ks is not None else None, len(streams), L.ptr(streams, L.i32p), L.ptr(th), L.ptr(ol, L.u8p)))

    def local_ba(self, min_cov_score, cams, ks=None, iters_fast=5, iterations=10, repr_eps=5.0, ctx=None):
        """The estimator step in one call, the windows never leaving HBM (`slam_kfmap_local_ba`): what gather -> bundle_adjustment_batch_ ->
        update(ks) do for the streams of the last add_keyframe.  cams: one (fx, fy, cx, cy) / Camera or S of them.  -> (status, stats): per stream
        0 solved and applied, 1 no window, 3 not selected, SLAM_ERR_NUMERIC (-5: the map untouched for that stream); stats (S, 8) as
        `slam_local_ba_batch`'s.  `last_windows()` has the windows' sizes."""
        c = ctx or self.ctx
        S = self.S
        minc = _per_stream(min_cov_score, np.int32, S)
        one = hasattr(cams, "intrinsics") or np.ndim(cams) == 1
        cm = np.ascontiguousarray([(q.intrinsics if hasattr(q, "intrinsics") else q) for q in ([cams] * S if one else cams)], dtype=np.float64).reshape(S, 4)
        status = np.zeros(S, dtype=np.int32); stats = np.zeros((S, 8))
        c.check(c.lib.slam_kfmap_local_ba(c.h, self.h, ks.h if ks is not None else None, L.ptr(minc, L.i32p), L.ptr(cm), int(iters_fast), int(iterations),
                                          float(repr_eps), L.ptr(status, L.i32p), L.ptr(stats)))
        return status, stats

    def last_windows(self):
        """(S, 3) P, M, O of the window every stream had in the last local_ba (zeros: none)"""
        pmo = np.zeros((self.S, 3), dtype=np.int32)
        self.ctx.check(self.ctx.lib.slam_kfmap_last_windows(self.h, L.ptr(pmo, L.i32p)))
        return pmo

    def filter(self, filtering_ratio, min_cov_score, first_kfid=20, want_removed=True, ctx=None):
        """map_filtering! (src/estimator.jl:358-406) for the streams of the last add_keyframe: a covisible key-frame with fewer than
        min_cov_score // 2 3-D points, or with more than filtering_ratio of them seen by more than four key-frames, is removed.
        filtering_ratio / min_cov_score: one value or S of them; first_kfid: no filtering before that key-frame (the reference's 20).
        -> per stream the ascending list of removed key-frame ids (synchronous), or None with want_removed=False (enqueue-only)."""
        c = ctx or self.ctx
        S = self.S
        ratio = _per_stream(filtering_ratio, np.float64, S)
        minc = _per_stream(min_cov_score, np.int32, S)
        if not want_removed:
            c.check(c.lib.slam_kfmap_filter(c.h, self.h, L.ptr(ratio), L.ptr(minc, L.i32p), int(first_kfid), None))
            return None
        words = np.zeros(S, dtype=np.uint64)
        c.check(c.lib.slam_kfmap_filter(c.h, self.h, L.ptr(ratio), L.ptr(minc, L.i32p), int(first_kfid), L.ptr(words, L.u64p)))
        self.last_removed_masks = words
        if not words.any():
            return [[] for _ in range(S)]
        cur = self.newest(ctx=c)                                 # a bit names a residue: the id is the one in (cur - R, cur) with it
        return [sorted(int(cur[s]) - ((int(cur[s]) - b) % self.R) for b in range(self.R) if int(words[s]) >> b & 1) for s in range(S)]

    def triangulate_temporal(self, cam, ks=None, max_error=3.0, min_depth=0.1, min_parallax=20.0, want_counts=True, ctx=None):
        """triangulate_temporal! (src/mapper.jl:185-262) from the map's own key-frames, for the streams of the last add_keyframe (call it right
        after): every 2-D point of the newest key-frame with an earlier observer is triangulated against its FIRST observer as it is now (the
        smallest key-frame id among the point's observers), with the poses the last bundle adjustment left in the map.  Accepted: the point gets
        its position and becomes 3-D, and with ks the list slot that carries its id takes xyz and is_3d.  Rejected (a gate fails with a parallax
        above min_parallax): the newest key-frame's observation leaves the map; THE LIST KEEPS THE KEYPOINT (ks.triangulate_temporal drops it).
        cam: one (fx, fy, cx, cy) / Camera or S of them.  -> (S, 4) int32: candidates, triangulated, observations removed, skipped (fewer than
        two observers, or the first observer's pixel is gone) per stream (synchronous), or None with want_counts=False (enqueue-only)."""
        c = ctx or self.ctx
        S = self.S
        one = hasattr(cam, "intrinsics") or np.ndim(cam) == 1
        cm = np.ascontiguousarray([(q.intrinsics if hasattr(q, "intrinsics") else q) for q in ([cam] * S if one else cam)], dtype=np.float64).reshape(S, 4)
        counts = np.zeros((S, 4), dtype=np.int32) if want_counts else None
        c.check(c.lib.slam_kfmap_triangulate_temporal(c.h, self.h, ks.h if ks is not None else None, L.ptr(cm), float(max_error), float(min_depth),
                                                      float(min_parallax), L.ptr(counts, L.i32p) if want_counts else None))
        return counts

    def newest(self, ctx=None):
        """(S,) the id of every stream's newest key-frame, -1 where there is none yet"""
        c = ctx or self.ctx
        cur = np.zeros(self.S, dtype=np.int32)
        c.check(c.lib.slam_kfmap_newest(c.h, self.h, L.ptr(cur, L.i32p)))
        return cur

    def remove_keyframe(self, s, kfid, ctx=None):
        """remove_keyframe! (src/map_manager.jl:184-209) of key-frame kfid of stream s; not in the ring: nothing; the newest: SlamHipError"""
        c = ctx or self.ctx
        c.check(c.lib.slam_kfmap_remove_keyframe(c.h, self.h, int(s), int(kfid)))

    def download_keyframe(self, s, kfid, ctx=None):
        """dict(theta, ids, upx, live) of key-frame kfid of stream s, or None when the ring does not hold it"""
        c = ctx or self.ctx
        theta = np.zeros(6); ids = np.zeros(self.cap, dtype=np.int64); upx = np.zeros((self.cap, 2)); live = np.zeros(self.cap, dtype=np.uint8)
        n = C.c_int(0)
        c.check(c.lib.slam_kfmap_download_keyframe(c.h, self.h, int(s), int(kfid), L.ptr(theta), L.ptr(ids, L.i64p), L.ptr(upx), L.ptr(live, L.u8p), self.cap, C.byref(n)))
        if n.value < 0:
            return None
        return dict(theta=theta, ids=ids[:n.value].copy(), upx=upx[:n.value].copy(), live=live[:n.value].astype(bool))

    def download_points(self, s, ctx=None):
        """dict(ids, xyz, is_3d, observed, ba, gone, observers) of stream s's map points in id order; observers: a tuple of key-frame ids per point"""
        c = ctx or self.ctx
        m = self.mcap
        ids = np.zeros(m, dtype=np.int64); xyz = np.zeros((m, 3)); fl = np.zeros(m, dtype=np.uint8)
        off = np.zeros(m + 1, dtype=np.int32); okf = np.zeros(m * self.R, dtype=np.int32)
        n = C.c_int(0)
        c.check(c.lib.slam_kfmap_download_points(c.h, self.h, int(s), L.ptr(ids, L.i64p), L.ptr(xyz), L.ptr(fl, L.u8p), L.ptr(off, L.i32p),
                                                 L.ptr(okf, L.i32p), m, m * self.R, C.byref(n)))
        k = n.value
        f = fl[:k]
        return dict(ids=ids[:k].copy(), xyz=xyz[:k].copy(), is_3d=(f & 1) != 0, observed=(f & 2) != 0, ba=(f & 4) != 0, gone=(f & 8) != 0,
                    observers=[tuple(int(v) for v in okf[off[j]:off[j + 1]]) for j in range(k)])

    # ---- descriptors and the local-map match (slam_kfmap_enable_descriptors / _add_descriptors / _local_map_match) ----
    def enable_descriptors(self, n_bits=256, ctx=None):
        """Give every table entry a descriptor row (n_bits = 256, the only width the match handles).  Opt-in; a second call is a no-op."""
        c = ctx or self.ctx
        c.check(c.lib.slam_kfmap_enable_descriptors(c.h, self.h, int(n_bits)))

    def add_descriptors(self, desc_ptr, info_ptr, dcap, ctx=None):
        """Right after add_keyframe: the rows ks.detect_describe has just written (desc_ptr: device pointer to S x dcap x 4 uint64, info_ptr: device
        pointer to S x 2 int64, e.g. torch_tensor.data_ptr()) go to the points of their ids, for the streams of that add_keyframe.  Enqueue-only."""
        c = ctx or self.ctx
        c.check(c.lib.slam_kfmap_add_descriptors(c.h, self.h, C.c_void_p(int(desc_ptr)), C.c_void_p(int(info_ptr)), int(dcap)))

    def local_map_match(self, cam, cell_size, max_projection_distance, max_descriptor_distance, max_local=None, cap_pairs=None, ctx=None):
        """update_frame_covisibility! + match_local_map! for the newest key-frames of the streams of the last add_keyframe, staged and matched in
        HBM.  cam: (10,) or (S, 10) = fx fy cx cy k1 k2 p1 p2 height width (lens distortion only after enable_pixels()); cell_size and the two distances: one value or S.
        max_local: the bound of a stream's local map (default 10 cap, the reference's 10 max_nb_keypoints).
        -> (status (S,), pairs: per stream an (n, 2) int64 array of (keypoint id, local-map point id) ascending by keypoint id, dist: per stream
        the (n,) winning descriptor distances).  status 0 matched, 1 nothing to match, 2 local map larger than max_local.  Synchronous."""
        c = ctx or self.ctx
        S = self.S
        cam = _per_stream(cam, np.float64, S, 10)
        cell = _per_stream(cell_size, np.int32, S)
        mpd = _per_stream(max_projection_distance, np.float64, S)
        mdd = _per_stream(max_descriptor_distance, np.float64, S)
        max_local = 10 * self.cap if max_local is None else int(max_local)
        cap_pairs = S * self.cap if cap_pairs is None else int(cap_pairs)
        status = np.zeros(S, dtype=np.int32); n = np.zeros(S, dtype=np.int32)
        pairs = np.zeros((max(cap_pairs, 1), 2), dtype=np.int64); dist = np.zeros(max(cap_pairs, 1))
        c.check(c.lib.slam_kfmap_local_map_match(c.h, self.h, L.ptr(cam), L.ptr(cell, L.i32p), L.ptr(mpd), L.ptr(mdd), max_local, L.ptr(status, L.i32p),
                                                 L.ptr(n, L.i32p), L.ptr(pairs, L.i64p), L.ptr(dist), cap_pairs))
        at = np.concatenate([[0], np.cumsum(n)])
        return status, [pairs[at[s]:at[s + 1]].copy() for s in range(S)], [dist[at[s]:at[s + 1]].copy() for s in range(S)]

    def enable_pixels(self, ctx=None):
        """Keep the raw pixel (kp.pixel) of every observation beside the undistorted one (slam_kfmap_enable_pixels, 16 R cap bytes per stream): from
        then on local_map_match works on raw pixels, as find_best_match and the frame grid do, and takes cameras with lens distortion; merge moves
        the raw pixels with the observations.  Call it before the first add_keyframe.  Opt-in; a second call is a no-op."""
        c = ctx or self.ctx
        c.check(c.lib.slam_kfmap_enable_pixels(c.h, self.h))

    def keyframe_pixels(self, s, kfid, ctx=None):
        """(n, 2) the raw pixels (y, x) of key-frame kfid of stream s in the order of download_keyframe's ids, or None when the ring does not hold it.
        SlamHipError without enable_pixels().  Synchronous."""
        c = ctx or self.ctx
        px = np.zeros((self.cap, 2)); n = C.c_int(0)
        c.check(c.lib.slam_kfmap_download_pixels(c.h, self.h, int(s), int(kfid), L.ptr(px), self.cap, C.byref(n)))
        return None if n.value < 0 else px[:n.value].copy()

    def enable_local_map_history(self, ctx=None):
        """Keep frame.local_map_ids of every key-frame of the ring in HBM (slam_kfmap_enable_local_map_history): from then on local_map_match applies
        the replace-or-union rule (src/map_manager.jl:350-354) and takes in the set of the oldest covisible key-frame (src/mapper.jl:274-286), so a
        point can reach the match after every key-frame that observes it has stopped being covisible.  Sets grow along that chain: use
        max_local >= mcap with it.  Opt-in; a second call is a no-op."""
        c = ctx or self.ctx
        c.check(c.lib.slam_kfmap_enable_local_map_history(c.h, self.h))

    def local_map_ids(self, s, kfid, ctx=None):
        """(n,) int64, ascending: the set local_map_match stored for key-frame kfid of stream s.  SlamHipError where the ring does not hold the
        key-frame or no set was stored for it (its match was skipped).  Synchronous."""
        c = ctx or self.ctx
        ids = np.zeros(self.mcap, dtype=np.int64); n = C.c_int32(0)
        c.check(c.lib.slam_kfmap_download_local_map_ids(c.h, self.h, int(s), int(kfid), L.ptr(ids, L.i64p), self.mcap, C.byref(n)))
        return ids[:n.value].copy()

    def merge(self, ks=None, pairs=None, want_counts=True, ctx=None):
        """merge_matches -> merge_mappoints -> update_keypoint! (src/mapper.jl:296-310, src/map_manager.jl:378-427, src/frame.jl:290-307): the pairs
        (keypoint id, local-map point id) are applied in HBM -- the keypoint is renamed in every key-frame that observes it, the touched slabs are put
        back in id order, the old point leaves the table.  pairs=None: the result of the last local_map_match where it lies on the device; else a list
        of S (n, 2) int64 arrays (one-to-one per stream).  ks: the KeypointSet whose live lists follow the renames (without one the old ids are marked
        gone).  -> (S, 4) int32: pairs applied, pairs skipped, observations renamed, status per stream (synchronous), or None with
        want_counts=False (enqueue-only)."""
        c = ctx or self.ctx
        S = self.S
        n_ptr = p_ptr = None
        if pairs is not None:
            if len(pairs) != S:
                raise ValueError(f"merge: {len(pairs)} pair arrays for {S} streams")
            per = [np.asarray(p, dtype=np.int64).reshape(-1, 2) for p in pairs]
            n = np.ascontiguousarray([len(p) for p in per], dtype=np.int32)
            flat = np.ascontiguousarray(np.concatenate(per + [np.zeros((1, 2), dtype=np.int64)]))
            n_ptr, p_ptr = L.ptr(n, L.i32p), L.ptr(flat, L.i64p)
        merged = np.zeros((S, 4), dtype=np.int32) if want_counts else None
        c.check(c.lib.slam_kfmap_merge(c.h, self.h, ks.h if ks is not None else None, n_ptr, p_ptr, L.ptr(merged, L.i32p) if want_counts else None))
        return merged

    # ---- descriptor rows (slam_kfmap_enable_descriptor_rows / _download_descriptor_rows) ----
    def enable_descriptor_rows(self, max_rows=4, ctx=None):
        """A point keeps one descriptor row per key-frame, at most max_rows (2 .. 8) of them, the reference's keyframes_descriptors: a merge hands
        prev's rows to the surviving point, a removed observation takes its key-frame's row along, and local_map_match takes the minimum distance
        over all pairs of rows.  Beyond max_rows the rows of the largest key-frame ids stay.  After enable_descriptors(); opt-in; a second call with
        the same max_rows is a no-op, another value a SlamHipError."""
        c = ctx or self.ctx
        c.check(c.lib.slam_kfmap_enable_descriptor_rows(c.h, self.h, int(max_rows)))
        self.max_rows = int(max_rows)

    def descriptor_rows(self, s, ctx=None):
        """dict(ids (n,), described (n,) bool, keys: per point the (k,) int32 key-frame ids of its rows, ascending, rows: per point the (k, 4) uint64
        rows in that order, dropped: the rows the bound has dropped on stream s) for the points download_points lists, in id order.  Synchronous."""
        c = ctx or self.ctx
        m, D = self.mcap, getattr(self, "max_rows", 1)
        ids = np.zeros(m, dtype=np.int64); has = np.zeros(m, dtype=np.uint8); off = np.zeros(m + 1, dtype=np.int32)
        keys = np.zeros(m * D, dtype=np.int32); rows = np.zeros((m * D, 4), dtype=np.uint64)
        n = C.c_int32(0); dropped = C.c_int32(0)
        c.check(c.lib.slam_kfmap_download_descriptor_rows(c.h, self.h, int(s), L.ptr(ids, L.i64p), L.ptr(has, L.u8p), L.ptr(off, L.i32p), L.ptr(keys, L.i32p),
                                                          L.ptr(rows, L.u64p), m, m * D, C.byref(n), C.byref(dropped)))
        k = n.value
        return dict(ids=ids[:k].copy(), described=has[:k] != 0, keys=[keys[off[j]:off[j + 1]].copy() for j in range(k)],
                    rows=[rows[off[j]:off[j + 1]].copy() for j in range(k)], dropped=int(dropped.value))

    def debug_local_map(self, s, ctx=None):
        """Test hook (slam_debug_kfmap_local_map, not part of the C header): what the last local_map_match staged for stream s ->
        dict(lm_ids (M,), proj_yx (M, 2), best_kp (M,), best_dist (M,), kp_ids (N,)); empty arrays unless the stream's status was 0."""
        c = ctx or self.ctx
        fn = c.lib.slam_debug_kfmap_local_map
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int, L.i64p, L.f64p, L.i32p, L.f64p, L.i64p, C.c_int, C.c_int, L.i32p]
        cap_lm = self.mcap                                       # a local map has at most one point per table entry
        lm = np.zeros(cap_lm, dtype=np.int64); proj = np.zeros((cap_lm, 2)); bk = np.zeros(cap_lm, dtype=np.int32); bd = np.zeros(cap_lm)
        kp = np.zeros(self.cap, dtype=np.int64); cnt = np.zeros(2, dtype=np.int32)
        c.check(fn(c.h, self.h, int(s), L.ptr(lm, L.i64p), L.ptr(proj), L.ptr(bk, L.i32p), L.ptr(bd), L.ptr(kp, L.i64p), cap_lm, self.cap, L.ptr(cnt, L.i32p)))
        N, M = int(cnt[0]), int(cnt[1])
        return dict(lm_ids=lm[:M].copy(), proj_yx=proj[:M].copy(), best_kp=bk[:M].copy(), best_dist=bd[:M].copy(), kp_ids=kp[:N].copy())

    def reset(self, s, ctx=None):
        c = ctx or self.ctx
        c.check(c.lib.slam_kfmap_reset(c.h, self.h, int(s)))

