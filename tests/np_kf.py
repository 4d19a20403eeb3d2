"""numpy model of the key-frame decision, written from the reference alone: check_new_kf_required (front_end.jl:361-393),
compute_parallax (:412-452), nb_occupied_cells (frame.jl:321-337 with to_cartesian, SLAM.jl:30-45) and the lens model (camera.jl:62-140).
Nothing of slam_jl_amd is imported: the tests compare the library with this file.

    frame_stats(...)  -> the 8 numbers slam_kpset_frame_stats returns for one stream
    decide(...)       -> (required, rule, margin) for one stream; margin = the smallest distance of a quantity that was compared as a
                         double from its threshold, over the comparisons the decision evaluated (inf if none)
"""
import warnings

import numpy as np


def undistort(cam, dist, yx):
    """undistort_point (camera.jl:98-125): (n, 2) pixels (y, x) -> undistorted pixels (y, x)"""
    fx, fy, cx, cy = cam
    k1, k2, p1, p2 = dist
    yx = np.asarray(yx, dtype=np.float64).reshape(-1, 2)
    ny = (yx[:, 0] - cy) / fy; nx = (yx[:, 1] - cx) / fx
    s0 = ny * ny; s1 = nx * nx; r2 = s0 + s1
    rd = 1.0 + k1 * r2 + k2 * r2 ** 2
    p = ny * nx
    dtx = 2 * p1 * p + p2 * (r2 + 2 * s0)
    dty = p1 * (r2 + 2 * s1) + 2 * p2 * p
    return np.stack([(rd * ny + dty) * fy + cy, (rd * nx + dtx) * fx + cx], axis=1)


def parallax_terms(cam, dist, yx, kyx, R=None):
    """|upx - undistort(kyx)| per keypoint (front_end.jl:434-438); R: the 3 x 3 compensation (None: not compensated)"""
    fx, fy, cx, cy = cam
    u = undistort(cam, dist, yx); v = undistort(cam, dist, kyx)
    if R is not None:
        R = np.asarray(R, dtype=np.float64)
        bx = (u[:, 1] - cx) / fx; by = (u[:, 0] - cy) / fy                                         # backproject (camera.jl:138-140), z = 1
        with np.errstate(all="ignore"):
            rx = (R[0, 0] * bx + R[0, 1] * by) + R[0, 2] * 1.0                                     # current_rotation * position, term by term
            ry = (R[1, 0] * bx + R[1, 1] * by) + R[1, 2] * 1.0
            rz = (R[2, 0] * bx + R[2, 1] * by) + R[2, 2] * 1.0
            u = np.stack([fy * ry / rz + cy, fx * rx / rz + cx], axis=1)                           # project (camera.jl:62-67)
    d = u - v
    with np.errstate(all="ignore"):
        return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])


def occupied_cells(yx, cell_size, height, width):
    """number of distinct to_cartesian(pixel, cell_size) = round.(pixel) .÷ cell_size .+ 1 (round half to even, ÷ truncating) that lie in the
    ceil(height / cell_size) x ceil(width / cell_size) grid; a keypoint outside it is skipped (the reference would throw)"""
    yx = np.asarray(yx, dtype=np.float64).reshape(-1, 2)
    gr, gc = -(-height // cell_size), -(-width // cell_size)
    ok = np.isfinite(yx).all(axis=1)
    r = np.clip(np.round(yx[ok]), -2.0 ** 62, 2.0 ** 62).astype(np.int64)                                                      # half to even
    q = np.sign(r) * (np.abs(r) // cell_size)                                                  # truncating division
    q = q[(q[:, 0] >= 0) & (q[:, 0] < gr) & (q[:, 1] >= 0) & (q[:, 1] < gc)]
    return len(np.unique(q[:, 0] * gc + q[:, 1]))


def frame_stats(cam, dist, yx, is3d, stereo, kyx, haskf, flags, cell_size, height, width, R=None):
    """[n, nb_3d, nb_stereo, nb_haskf, nb_occupied_cells, n_parallax, mean, median]; flags bit 0: compensate with R, bit 1: only_2d"""
    yx = np.asarray(yx, dtype=np.float64).reshape(-1, 2); kyx = np.asarray(kyx, dtype=np.float64).reshape(-1, 2)
    is3d = np.asarray(is3d, dtype=bool); stereo = np.asarray(stereo, dtype=bool); haskf = np.asarray(haskf, dtype=bool)
    take = haskf & ~is3d if flags & 2 else haskf.copy()
    t = parallax_terms(cam, dist, yx[take], kyx[take], R if flags & 1 else None)
    m = len(t)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        mean = float(np.sum(t) / m) if m else 0.0                                          # (the order of the sum is the implementation's)
        median = float(np.median(t)) if m else 0.0
    return np.array([len(yx), is3d.sum(), stereo.sum(), haskf.sum(), occupied_cells(yx, cell_size, height, width), m, mean, median], dtype=np.float64)


def decide(stats, frames_delta, prev_kf_nb_3d, has_prev_kf, max_nb_keypoints, initial_parallax=20.0, local_ba_on=False):
    """front_end.jl:361-393.  rule: 0 no previous key-frame, 1 sparse cells, 2 few 3-D keypoints, 3 enough 3-D keypoints, 4 parallax rule."""
    margin = [np.inf]

    def lt(a, b):                                                # a < b on doubles, recording |a - b|
        margin[0] = min(margin[0], abs(float(a) - float(b))) if np.isfinite(a) and np.isfinite(b) else margin[0]
        return float(a) < float(b)

    def ge(a, b):
        margin[0] = min(margin[0], abs(float(a) - float(b))) if np.isfinite(a) and np.isfinite(b) else margin[0]
        return float(a) >= float(b)                              # False for NaN

    if not has_prev_kf:
        return False, 0, margin[0]
    cells, nb_3d, median = float(stats[4]), float(stats[1]), float(stats[7])
    if lt(cells, 0.33 * max_nb_keypoints) and frames_delta >= 5 and not local_ba_on:
        return True, 1, margin[0]
    if nb_3d < 20 and frames_delta >= 2:
        return True, 2, margin[0]
    if nb_3d > 0.5 * max_nb_keypoints and (local_ba_on or frames_delta < 2):
        return False, 3, margin[0]
    cx = ge(median, initial_parallax / 2.0)
    c0 = ge(median, initial_parallax)
    c1 = lt(nb_3d, 0.75 * prev_kf_nb_3d)
    c2 = lt(cells, 0.5 * max_nb_keypoints) and lt(nb_3d, 0.85 * prev_kf_nb_3d) and not local_ba_on
    return bool(cx and (c0 or c1 or c2)), 4, margin[0]
