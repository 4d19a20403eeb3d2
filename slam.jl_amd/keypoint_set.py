"""Device-resident keypoint lists of S lock-stepped streams (slam_kpset, include/slamhip.h): the arrays behind
Frame.keypoints (src/frame.jl) for the calls of the front-end / mapper hot path -- optical_flow_matching!
(src/map_manager.jl:451-564), extract_keypoints! (:98-113), triangulate_stereo! (src/mapper.jl:142-183) -- kept in HBM
between calls.  Only `counts()`, `frame_stats()` (the statistics the key-frame decision reads), the pose calls, `upload()` and `download()`
touch the host."""
import contextlib
import ctypes as C

import numpy as np

from . import _lib as L
from .optical_flow import _check_match, _tune


# the per-stream parameter slot of csrc/kpset.hpp (tests/test_keypoint_set_host.py keeps the two in step)
KP_PAR, KP_PAR_CAM, KP_PAR_DIST, KP_PAR_SHIFT = 32, 16, 20, 24


def stream_params(S, Tcw=None, cam=None, dist=None, shift_yx=None):
    """S x KP_PAR per-stream call parameters: [0..15] Tcw (column-major), fx fy cx cy at KP_PAR_CAM, k1 k2 p1 p2 at KP_PAR_DIST, the prior shift (y, x) at KP_PAR_SHIFT."""
    p = np.zeros((S, KP_PAR))
    p[:, KP_PAR_CAM:KP_PAR_CAM + 2] = 1.0
    if Tcw is not None:
        T = np.asarray(Tcw, dtype=np.float64).reshape(-1, 4, 4)
        p[:, :16] = np.broadcast_to(T, (S, 4, 4)).transpose(0, 2, 1).reshape(S, 16)       # column-major
    if cam is not None:
        p[:, KP_PAR_CAM:KP_PAR_CAM + 4] = np.asarray(cam, dtype=np.float64)
    if dist is not None:
        p[:, KP_PAR_DIST:KP_PAR_DIST + 4] = np.asarray(dist, dtype=np.float64)
    if shift_yx is not None:
        p[:, KP_PAR_SHIFT:KP_PAR_SHIFT + 2] = np.asarray(shift_yx, dtype=np.float64).reshape(-1, 2)
    return np.ascontiguousarray(p)


def _with_rcomp(sp, S):
    """a copy of sp with R_compensation as the seams read it, a dense column-major 3 x 3 at [0..8]: repacked from the 4 x 4 Tcw slot (column-major, stride 4)"""
    sp = np.ascontiguousarray(sp, dtype=np.float64).reshape(S, KP_PAR).copy()
    sp[:, :9] = sp[:, :16].reshape(S, 4, 4)[:, :3, :3].reshape(S, 9)            # [col][row]
    return sp


def _sp_ptr(stream_params_):
    """(array kept alive, pointer or None) of a match's optional stream parameters"""
    sp = None if stream_params_ is None else np.ascontiguousarray(stream_params_, dtype=np.float64)
    return sp, (L.ptr(sp) if sp is not None else None)


class KeypointSet:
    def __init__(self, S, cap, ctx=None):
        self.ctx = ctx or L.default_context()
        self.S, self.cap = S, cap
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.slam_kpset_create(self.ctx.h, S, cap, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.slam_kpset_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host <-> device (initialisation, tests, host consumers) ----
    def _fetch(self, call, *spec):
        """one download seam: cap-long outputs of the (trailing shape, pointer type) in `spec`, call(pointers..., cap, byref(n)), trimmed to n"""
        out = [np.zeros((self.cap,) + shape, dtype=np.dtype(t._type_)) for shape, t in spec]
        n = C.c_int(0)
        call(*[L.ptr(a, t) for a, (_, t) in zip(out, spec)], self.cap, C.byref(n))
        return [a[:n.value].copy() for a in out]

    def upload(self, s, yx, is_3d, xyz=None, ids=None, ctx=None):
        c = ctx or self.ctx
        yx = np.ascontiguousarray(yx, dtype=np.float64).reshape(-1, 2)
        f = np.ascontiguousarray(np.asarray(is_3d).astype(np.uint8))
        x = None if xyz is None else np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        i = None if ids is None else np.ascontiguousarray(ids, dtype=np.int64)
        c.check(c.lib.slam_kpset_upload(c.h, self.h, s, L.ptr(yx), L.ptr(f, L.u8p), L.ptr(x) if x is not None else None,
                                        L.ptr(i, L.i64p) if i is not None else None, len(yx)))

    def download(self, s, ctx=None):
        """dict(yx, is_3d, xyz, ids, stereo_yx, has_stereo) of stream s"""
        c = ctx or self.ctx
        yx, f, xyz, ids, syx, hs = self._fetch(lambda *a: c.check(c.lib.slam_kpset_download(c.h, self.h, s, *a)),
                                               ((2,), L.f64p), ((), L.u8p), ((3,), L.f64p), ((), L.i64p), ((2,), L.f64p), ((), L.u8p))
        return dict(yx=yx, is_3d=f.astype(bool), xyz=xyz, ids=ids, stereo_yx=syx, has_stereo=hs.astype(bool))

    def counts(self, ctx=None):
        """the S list lengths: the one small device -> host copy of a step (synchronises the context's stream)"""
        c = ctx or self.ctx
        out = np.zeros(self.S, dtype=np.int32)
        c.check(c.lib.slam_kpset_counts(c.h, self.h, L.ptr(out, L.i32p)))
        return out

    # ---- the streams the six key-frame seams act on (slam_kpset_select) ----
    def select(self, mask, ctx=None):
        """The streams detect / detect_describe / keyframe / stereo_match / triangulate / triangulate_temporal act on: mask = S entries, non-zero
        (or True) = selected -- the `required` of keyframe_required as it is -- or None = every stream.  Every other call acts on all streams.  The
        selection is a property of the set and holds until the next select(); an unselected stream comes out of the six seams byte for byte as it
        went in.  Enqueue-only; the mask is staged, the caller's array is free on return."""
        c = ctx or self.ctx
        if mask is None:
            c.check(c.lib.slam_kpset_select(c.h, self.h, None))
            return
        m = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.uint8)
        if m.shape != (self.S,):
            raise ValueError(f"select: {m.size} entries for {self.S} streams")
        c.check(c.lib.slam_kpset_select(c.h, self.h, L.ptr(m, L.u8p)))

    def selection(self):
        """the current selection as (S,) bool (all True when none is set)"""
        m = np.zeros(self.S, dtype=np.uint8)
        self.ctx.check(self.ctx.lib.slam_kpset_selection(self.h, L.ptr(m, L.u8p)))
        return m.astype(bool)

    @contextlib.contextmanager
    def selected(self, mask, ctx=None):
        """with ks.selected(mask): ...  -- the key-frame seams inside act on `mask`; the previous selection is restored on the way out"""
        before = self.selection()
        self.select(mask, ctx=ctx)
        try:
            yield self
        finally:
            self.select(before, ctx=ctx)

    # ---- enqueue-only calls ----
    def flow_match(self, from_batch, to_batch, params, stream_params_=None, prior=0, pyramid_levels_3d=1, iterations=30, n_bound=0, ctx=None):
        c = ctx or self.ctx
        sp, sp_ptr = _sp_ptr(stream_params_)
        rc = c.lib.slam_kpset_flow_match(c.h, self.h, from_batch.pyramids[0].h, to_batch.pyramids[0].h, sp_ptr,
                                         prior, *_tune(params, pyramid_levels_3d, iterations), int(n_bound))
        _check_match(c, rc)

    def stereo_match(self, left_batch, right_batch, params, stream_params_=None, prior=0, pyramid_levels_3d=1, iterations=30,
                     epipolar_error=2.0, n_bound=0, ctx=None, compact=False):
        """compact: right_batch is a COMPACT batch (PyramidBatch.update_selected_ under the set's current selection; it may have fewer members
        than the set has streams): stream s's target is its member rank(s) (slam_kpset_stereo_match_compact).  A batch built for another
        selection, or by an ordinary update_ since, raises."""
        c = ctx or self.ctx
        sp, sp_ptr = _sp_ptr(stream_params_)
        fn = c.lib.slam_kpset_stereo_match_compact if compact else c.lib.slam_kpset_stereo_match
        rc = fn(c.h, self.h, left_batch.pyramids[0].h, right_batch.pyramids[0].h, sp_ptr,
                prior, *_tune(params, pyramid_levels_3d, iterations), float(epipolar_error), int(n_bound))
        _check_match(c, rc)

    def remove(self, flags_dev_ptr, ctx=None):
        """flags_dev_ptr: device pointer to S x cap bytes (1 = remove), e.g. torch_tensor.data_ptr()"""
        c = ctx or self.ctx
        c.check(c.lib.slam_kpset_remove(c.h, self.h, C.c_void_p(flags_dev_ptr)))

    def detect(self, e, batch, sigma_mask=3.0, min_response=1e-4, ctx=None):
        c = ctx or self.ctx
        c.check(c.lib.slam_kpset_detect(c.h, self.h, batch.pyramids[0].h, e.max_points, e.radius, e.grid_resolution[0], e.grid_resolution[1],
                                        e.cell_size, float(sigma_mask), float(min_response)))

    def detect_describe(self, e, batch, desc_ptr, info_ptr, dcap, pattern=None, sigma=np.sqrt(2.0), window=9, sigma_mask=3.0, min_response=1e-4,
                        ctx=None):
        """extract_keypoints! with describe (map_manager.jl:98-113) on the lists (slam_kpset_detect_describe): the candidates describe() would
        drop at the border are not appended, the appended ones are described.  desc_ptr: device pointer to S x dcap x (n_bits / 64) uint64,
        info_ptr: device pointer to S x 2 int64 (first id, number appended), e.g. torch_tensor.data_ptr(); the j-th keypoint this call
        appends to stream s has its descriptor at [s, j].  dcap >= cells * ceil(max_points / cells).  Enqueue-only."""
        from .extractor import brief_pattern
        c = ctx or self.ctx
        pat = np.ascontiguousarray(brief_pattern() if pattern is None else pattern, dtype=np.int32).reshape(-1, 4)
        c.check(c.lib.slam_kpset_detect_describe(c.h, self.h, batch.pyramids[0].h, e.max_points, e.radius, e.grid_resolution[0], e.grid_resolution[1],
                                                 e.cell_size, float(sigma_mask), float(min_response), L.ptr(pat, L.i32p), len(pat), float(sigma),
                                                 int(window), C.c_void_p(desc_ptr), C.c_void_p(info_ptr), int(dcap)))

    def triangulate(self, cam1, cam2, T21, Twc, max_error, min_depth=0.1, n_bound=0, ctx=None, dist1=None, dist2=None):
        """triangulate_stereo! on the lists.  dist1 / dist2: k1 k2 p1 p2 of the left / right lens (None: none) -- with either given the pixels
        of both views are undistorted, each through its own camera, before the DLT and the gates (slam_kpset_triangulate_lens); with both
        None the pixels are used as stored (slam_kpset_triangulate)."""
        from .triangulation import projection_matrices
        c = ctx or self.ctx
        P1, P2 = projection_matrices(cam1, cam2, T21)
        P1 = np.asfortranarray(P1); P2 = np.asfortranarray(P2); T = np.asfortranarray(T21, dtype=np.float64)
        c1 = np.ascontiguousarray(cam1, dtype=np.float64); c2 = np.ascontiguousarray(cam2, dtype=np.float64)
        W = np.asarray(Twc, dtype=np.float64).reshape(-1, 4, 4)
        W = np.ascontiguousarray(np.broadcast_to(W, (self.S, 4, 4)).transpose(0, 2, 1).reshape(self.S, 16))
        if dist1 is None and dist2 is None:
            c.check(c.lib.slam_kpset_triangulate(c.h, self.h, L.ptr(P1), L.ptr(P2), L.ptr(T), L.ptr(c1), L.ptr(c2), L.ptr(W),
                                                 float(max_error), float(min_depth), int(n_bound)))
            return
        d1 = np.ascontiguousarray(np.zeros(4) if dist1 is None else dist1, dtype=np.float64).reshape(4)
        d2 = np.ascontiguousarray(np.zeros(4) if dist2 is None else dist2, dtype=np.float64).reshape(4)
        c.check(c.lib.slam_kpset_triangulate_lens(c.h, self.h, L.ptr(P1), L.ptr(P2), L.ptr(T), L.ptr(c1), L.ptr(c2), L.ptr(d1), L.ptr(d2), L.ptr(W),
                                                  float(max_error), float(min_depth), int(n_bound)))

    def keyframe(self, ctx=None):
        """create_keyframe! for the lists: the current positions become the previous key-frame's observations (slam_kpset_keyframe)"""
        c = ctx or self.ctx
        c.check(c.lib.slam_kpset_keyframe(c.h, self.h))

    def upload_keyframe(self, s, kyx, has_kf, ctx=None):
        c = ctx or self.ctx
        k = np.ascontiguousarray(kyx, dtype=np.float64).reshape(-1, 2)
        f = np.ascontiguousarray(np.asarray(has_kf).astype(np.uint8))
        c.check(c.lib.slam_kpset_upload_keyframe(c.h, self.h, s, L.ptr(k), L.ptr(f, L.u8p), len(k)))

    def upload_stereo(self, s, stereo_yx, has_stereo, ctx=None):
        """the stereo observations of stream s's list (download() reads them back): stereo_yx (n, 2) in the right image, has_stereo (n,) flags"""
        c = ctx or self.ctx
        k = np.ascontiguousarray(stereo_yx, dtype=np.float64).reshape(-1, 2)
        f = np.ascontiguousarray(np.asarray(has_stereo).astype(np.uint8)).reshape(-1)
        if len(f) != len(k):
            raise ValueError(f"upload_stereo: {len(k)} stereo pixels for {len(f)} flags")
        c.check(c.lib.slam_kpset_upload_stereo(c.h, self.h, s, L.ptr(k), L.ptr(f, L.u8p), len(k)))

    def download_keyframe(self, s, ctx=None):
        c = ctx or self.ctx
        k, f = self._fetch(lambda *a: c.check(c.lib.slam_kpset_download_keyframe(c.h, self.h, s, *a)), ((2,), L.f64p), ((), L.u8p))
        return k, f.astype(bool)

    def upload_first(self, s, first_yx, first_kf, kf_count, ctx=None):
        c = ctx or self.ctx
        f = np.ascontiguousarray(first_yx, dtype=np.float64).reshape(-1, 2)
        k = np.ascontiguousarray(first_kf, dtype=np.int32)
        c.check(c.lib.slam_kpset_upload_first(c.h, self.h, s, L.ptr(f), L.ptr(k, L.i32p), len(f), int(kf_count)))

    def download_first(self, s, ctx=None):
        """(first_yx, first_kf, key-frame counter) of stream s: where and by which key-frame each keypoint was first observed"""
        c = ctx or self.ctx
        kc = C.c_int(0)
        f, k = self._fetch(lambda *a: c.check(c.lib.slam_kpset_download_first(c.h, self.h, s, *a, C.byref(kc))), ((2,), L.f64p), ((), L.i32p))
        return f, k, kc.value

    def triangulate_temporal(self, sp, kf_cw, Twc, kf_cur, kf_lo=None, max_error=3.0, min_depth=0.1, min_parallax=20.0, n_bound=0, ctx=None):
        """triangulate_temporal! (mapper.jl:185-262) on the lists (slam_kpset_triangulate_temporal).  kf_cw: (S, nkf, 4, 4) world ->
        camera poses of the key-frames, key-frame id k of stream s at [s, k % nkf]; Twc: (S, 4, 4) camera -> world of the frame;
        kf_cur: (S,) the frame's key-frame id; kf_lo: (S,) oldest id still in the table (default kf_cur - nkf + 1).  The per-observer
        matrices of mapper.jl:226-231 are formed here (numpy), as the Julia caller would form them."""
        c = ctx or self.ctx
        sp = np.ascontiguousarray(sp, dtype=np.float64).reshape(self.S, KP_PAR)
        kf_cw = np.asarray(kf_cw, dtype=np.float64).reshape(self.S, -1, 4, 4)
        nkf = kf_cw.shape[1]
        Twc = np.broadcast_to(np.asarray(Twc, dtype=np.float64).reshape(-1, 4, 4), (self.S, 4, 4))
        kf_cur = np.ascontiguousarray(np.broadcast_to(np.asarray(kf_cur, dtype=np.int32), (self.S,)))
        kf_lo = np.ascontiguousarray(np.maximum(kf_cur - nkf + 1, 0) if kf_lo is None else np.broadcast_to(np.asarray(kf_lo, dtype=np.int32), (self.S,)), dtype=np.int32)
        tab = np.zeros((self.S, nkf, 4, 16))
        for s in range(self.S):
            fx, fy, cx, cy = sp[s, KP_PAR_CAM:KP_PAR_CAM + 4]
            K4 = np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
            for k in range(nkf):
                rel = kf_cw[s, k] @ Twc[s]                                # observer_kf.cw * frame.wc
                rel_inv = np.linalg.inv(rel)
                for j, M in enumerate((K4 @ rel_inv, rel_inv, rel, np.linalg.inv(kf_cw[s, k]))):
                    tab[s, k, j] = M.T.reshape(16)                        # column-major
        tab = np.ascontiguousarray(tab.reshape(self.S, nkf, 64))
        c.check(c.lib.slam_kpset_triangulate_temporal(c.h, self.h, L.ptr(sp), L.ptr(tab), int(nkf), L.ptr(kf_cur, L.i32p), L.ptr(kf_lo, L.i32p),
                                                      float(max_error), float(min_depth), float(min_parallax), int(n_bound)))

    def compute_pose_5pt(self, sp, min_parallax=5.0, max_repr_error=3.0, iters=128, seed=0, ctx=None, fetch=True):
        """compute_pose_5pt! (front_end.jl:242-332) for every stream on the device-resident lists (slam_kpset_compute_pose_5pt):
        returns (Rt (S, 3, 4) key-frame -> frame with |t| = 1, status (S,), inlier counts (S,), average parallax (S,), list lengths
        after the removals (S,)).  sp: stream_params(...) with R_compensation in the rotation part of the Tcw slot (rows / columns
        0..2) and the camera / distortion entries filled."""
        c = ctx or self.ctx
        sp = _with_rcomp(sp, self.S)
        if not fetch:                                            # enqueue only: the filter acts on the lists, nothing comes back
            c.check(c.lib.slam_kpset_compute_pose_5pt(c.h, self.h, L.ptr(sp), float(min_parallax), float(max_repr_error), int(iters),
                                                      int(seed) & 0xFFFFFFFFFFFFFFFF, None, None, None, None, None))
            return None
        P = np.zeros((self.S, 12)); status = np.zeros(self.S, dtype=np.int32); ninl = np.zeros(self.S, dtype=np.int32)
        par = np.zeros(self.S); counts = np.zeros(self.S, dtype=np.int32)
        c.check(c.lib.slam_kpset_compute_pose_5pt(c.h, self.h, L.ptr(sp), float(min_parallax), float(max_repr_error), int(iters),
                                                  int(seed) & 0xFFFFFFFFFFFFFFFF, L.ptr(P), L.ptr(status, L.i32p), L.ptr(ninl, L.i32p),
                                                  L.ptr(par), L.ptr(counts, L.i32p)))
        return P.reshape(self.S, 4, 3).transpose(0, 2, 1).copy(), status, ninl, par, counts

    def frame_stats(self, sp, flags, cell_size, shape, fetch=True, stats_dev_ptr=None, ctx=None):
        """What check_new_kf_required (flags = 1) / check_ready_for_init! (flags = 2) read of the frame, for every stream
        (slam_kpset_frame_stats): (S, 8) array of [list length, nb_3d_kpts, nb_stereo_kpts, keypoints the previous key-frame observes,
        nb_occupied_cells, n_parallax, mean parallax, median parallax] (front_end.jl:412-452, frame.jl:321-337).  flags: bit 0
        compensate_rotation, bit 1 only_2d.  sp: stream_params(...) as for compute_pose_5pt (R_compensation in the rotation part of the
        Tcw slot, camera / distortion filled); shape = (height, width) of the image.  The call is the step's one device -> host copy;
        fetch=False only enqueues (results in stats_dev_ptr, a device pointer to S x 8 doubles, or in a buffer of the set) and returns None."""
        c = ctx or self.ctx
        sp = _with_rcomp(sp, self.S)
        out = np.zeros((self.S, 8)) if fetch else None
        c.check(c.lib.slam_kpset_frame_stats(c.h, self.h, L.ptr(sp), int(flags), int(cell_size), int(shape[0]), int(shape[1]),
                                             C.c_void_p(stats_dev_ptr) if stats_dev_ptr else None, L.ptr(out) if fetch else None))
        return out

    def compute_pose(self, sp, threshold=3.0, iters=256, seed=0, pnp_iters_fast=5, pnp_iterations=10, depth_eps=1e-6, repr_eps=None, ctx=None):
        """compute_pose! (front_end.jl:132-219) for every stream on the device-resident lists (slam_kpset_compute_pose): returns
        (poses (S, 4, 4) world -> camera, status (S,), P3P inlier counts (S,), list lengths after the outlier removals (S,)).
        sp: stream_params(...) with the camera / distortion entries filled; repr_eps defaults to `threshold`
        (max_reprojection_error on both, front_end.jl:166,206)."""
        c = ctx or self.ctx
        sp = np.ascontiguousarray(sp, dtype=np.float64).reshape(self.S, KP_PAR)
        poses = np.zeros((self.S, 16)); status = np.zeros(self.S, dtype=np.int32); ninl = np.zeros(self.S, dtype=np.int32)
        counts = np.zeros(self.S, dtype=np.int32)
        c.check(c.lib.slam_kpset_compute_pose(c.h, self.h, L.ptr(sp), float(threshold), int(iters), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                              int(pnp_iters_fast), int(pnp_iterations), float(depth_eps),
                                              float(threshold if repr_eps is None else repr_eps),
                                              L.ptr(poses), L.ptr(status, L.i32p), L.ptr(ninl, L.i32p), L.ptr(counts, L.i32p)))
        return poses.reshape(self.S, 4, 4).transpose(0, 2, 1).copy(), status, ninl, counts


def keyframe_required(stats, frames_delta, prev_kf_nb_3d, has_prev_kf, params, local_ba_on=False):
    """check_new_kf_required (front_end.jl:361-393) per stream (slam_keyframe_required; host arithmetic, no device): stats = the (S, 8)
    array of KeypointSet.frame_stats(flags=1), frames_delta = frame id - key-frame id, prev_kf_nb_3d = the key-frame's own nb_3d_kpts,
    has_prev_kf = the key-frame is in the map; params: Params (max_nb_keypoints, initial_parallax).  Returns (required (S,) bool,
    rule (S,) uint8: 0 no key-frame, 1 sparse cells, 2 few 3-D keypoints, 3 enough 3-D keypoints, 4 the parallax rule)."""
    st = np.ascontiguousarray(stats, dtype=np.float64).reshape(-1, 8)
    S = len(st)
    b = lambda a, t: np.ascontiguousarray(np.broadcast_to(np.asarray(a).astype(t), (S,)))
    fd, pk, hp = b(frames_delta, np.int32), b(prev_kf_nb_3d, np.int32), b(has_prev_kf, np.uint8)
    req = np.zeros(S, dtype=np.uint8); rule = np.zeros(S, dtype=np.uint8)
    lib = L.load()
    rc = lib.slam_keyframe_required(S, L.ptr(st), L.ptr(fd, L.i32p), L.ptr(pk, L.i32p), L.ptr(hp, L.u8p), int(params.max_nb_keypoints),
                                    float(params.initial_parallax), 1 if local_ba_on else 0, L.ptr(req, L.u8p), L.ptr(rule, L.u8p))
    if rc != 0:
        raise L.SlamHipError(f"libslamhip error {rc}: {lib.slam_last_error(None).decode()}")
    return req.astype(bool), rule


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x ^ (x >> 31)


def _samples(seed, stream, n, iters, k):
    """iters x k: k distinct indices below n per iteration, splitmix64(seed ^ stream << 48 ^ iteration << 16 ^ attempt) mod n (draw_distinct, csrc/geom_device.hpp)"""
    out = np.full((iters, k), -1, dtype=np.int32)
    for it in range(iters):
        att = 0
        idx = []
        while len(idx) < k:
            h = _splitmix64((int(seed) ^ (int(stream) << 48) ^ (it << 16) ^ att) & 0xFFFFFFFFFFFFFFFF)
            att += 1
            c = int(h % n)
            if c not in idx:
                idx.append(c)
        out[it] = idx
    return out


def pose_samples(seed, stream, n, iters):
    """The triples slam_kpset_compute_pose draws for stream `stream` with `n` 3-D keypoints (csrc/pose.hip, k_kpose_samples); -1 when n < 5."""
    return np.full((iters, 3), -1, dtype=np.int32) if n < 5 else _samples(seed, stream, n, iters, 3)


def pose_samples5(seed, stream, n, iters):
    """The 5-tuples slam_kpset_compute_pose_5pt draws (csrc/fivepoint.hip, k_kfive_samples): as pose_samples, five distinct indices."""
    return _samples(seed, stream, n, iters, 5)


def pose_5pt_inputs(cam, dist, yx, kyx):
    """front_end.jl:263-272 for the keypoints both frames observe: (px1, px2, pd1, pd2), (x, y) order -- undistorted pixels and
    normalised coordinates of the key-frame (1) and the frame (2); the arithmetic of k_kfive_gather."""
    fx, fy, cx, cy = cam
    z = np.zeros((len(np.atleast_2d(yx)), 3))
    _, p2, _ = pose_inputs(cam, dist, yx, z)
    _, p1, _ = pose_inputs(cam, dist, kyx, z)
    pd = lambda p: np.stack([(p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy], axis=1)
    return p1, p2, pd(p1), pd(p2)


def pose_5pt_compose(Rt, prev_cw, cur_wc):
    """front_end.jl:320-330: translation scaled to the motion model's key-frame -> frame distance, composed with the key-frame pose."""
    scale = np.linalg.norm((prev_cw @ cur_wc)[:3, 3])
    R, t = Rt[:, :3], Rt[:, 3]
    t = scale * (t / np.linalg.norm(t))
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    return T @ prev_cw


def pose_inputs(cam, dist, yx, xyz):
    """front_end.jl:139-160 for one stream's 3-D keypoints: (pts3d, px_xy, pdn) as p3p_ransac takes them -- undistort_point
    (camera.jl:98-125), backproject (:138-140), normalize; the arithmetic of k_kpose_gather term by term."""
    fx, fy, cx, cy = cam
    k1, k2, p1, p2 = dist
    yx = np.asarray(yx, dtype=np.float64).reshape(-1, 2)
    ny = (yx[:, 0] - cy) / fy; nx = (yx[:, 1] - cx) / fx
    s0 = ny * ny; s1 = nx * nx; r2 = s0 + s1
    rd = (1.0 + k1 * r2) + k2 * (r2 * r2)
    pp = ny * nx
    dtx = 2 * p1 * pp + p2 * (r2 + 2 * s0); dty = p1 * (r2 + 2 * s1) + 2 * p2 * pp
    uy = (rd * ny + dty) * fy + cy; ux = (rd * nx + dtx) * fx + cx
    bx = (ux - cx) / fx; by = (uy - cy) / fy
    inv = 1.0 / np.sqrt((bx * bx + by * by) + 1.0)
    px_xy = np.stack([ux, uy], axis=1)
    pdn = np.stack([inv * bx, inv * by, inv * 1.0], axis=1)
    return np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3), px_xy, pdn
