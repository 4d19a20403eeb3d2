"""CPU: known-answer cases for the Python model of the local-map match (tests/np_local_map.py: src/mapper.jl:318-462 restated), one per rule of
the seam -- hand-built scenes of at most 4 keypoints, an identity pose and a pinhole camera whose projections can be read off the numbers:
a world point (x, y, z) lands on the pixel (100 y / z + 60, 100 x / z + 80).  Plus the CSR packing of the host mirror and the synthetic
generator's deliberate ties."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_local_map as npl  # noqa: E402

CAM = (100.0, 100.0, 80.0, 60.0, 0.0, 0.0, 0.0, 0.0, 120, 160)
DESC_A = np.array([[0x0123456789ABCDEF, 0xFFFF0000FFFF0000, 0x0F0F0F0F0F0F0F0F, 0x1]], dtype=np.uint64)
DESC_B = DESC_A ^ np.array([[0xFF, 0, 0, 0]], dtype=np.uint64)                  # 8 bits away from DESC_A
K2 = np.stack([np.eye(4), np.eye(4)])
K2[0, 0, 3] = 0.5                                                               # key-frame 0: shifted half a metre sideways


class P:
    def __init__(self, proj=2.0, desc=0.35):
        self.max_projection_distance, self.max_descriptor_distance = proj, desc


def frame(cam=CAM, cell=35, nb_3d=100):
    return {"Tcw": np.eye(4), "cam": cam, "cell_size": cell, "nb_3d_kpts": nb_3d}


def at(pixel, z=5.0):
    """the world point that projects to `pixel` (y, x) at depth z"""
    return ((pixel[1] - 80.0) / 100.0 * z, (pixel[0] - 60.0) / 100.0 * z, z)


def kp(pixel, desc=DESC_A, observers=()):
    return {"pixel": pixel, "descriptors": desc, "observers": list(observers)}


def mp(position, desc=DESC_A, observers=()):
    return {"position": position, "descriptors": desc, "observers": list(observers)}


def run(kps, mps, fr=None, params=None, keyframes=K2):
    return npl.do_local_map_matching(fr or frame(), kps, keyframes, mps, params or P())


def test_depth_gate():
    r = run([kp((60.0, 80.0))], [mp((0.0, 0.0, 0.05)), mp((0.0, 0.0, 0.2))])
    assert list(r["best_kp"]) == [-1, 0] and list(r["match"]) == [1]
    assert np.isnan(r["proj_yx"][0]).all() and r["best_dist"][0] == -1.0
    assert np.array_equal(r["proj_yx"][1], [60.0, 80.0]) and r["best_dist"][1] == 0.0


def test_view_angle_gate():
    # threshold cos(atan(max(0.6, 0.8))) = 0.7809: (0.75, 0.5, 1) is inside the image at (110, 155) but 42 degrees off the axis (cos = 0.743)
    r = run([kp((110.0, 155.0)), kp((60.0, 150.0))], [mp((0.75, 0.5, 1.0)), mp((0.7, 0.0, 1.0))])
    assert list(r["best_kp"]) == [-1, 1] and np.isnan(r["proj_yx"][0]).all()
    assert np.allclose(r["proj_yx"][1], [60.0, 150.0], atol=1e-12)


def test_project_undistort_radial_and_tangential():
    cam = (100.0, 100.0, 80.0, 60.0, -0.2, 0.0, 0.01, 0.02, 120, 160)
    r = run([kp((60.0, 80.0))], [mp((0.5, 0.0, 1.0))], fr=frame(cam))
    # r2 = 0.25: rd = 0.95; dty = p1 (r2 + 2 nx^2) = 0.0075; dtx = p2 (r2 + 2 ny^2) = 0.005  ->  y = 60.75, x = (0.475 + 0.005) 100 + 80
    assert np.allclose(r["proj_yx"][0], [60.75, 128.0], atol=1e-12)
    r = run([kp((60.0, 80.0))], [mp((0.5, 0.0, 1.0))], fr=frame((100.0, 100.0, 80.0, 60.0, 0.0, 0.5, 0.0, 0.0, 120, 160)))
    assert np.allclose(r["proj_yx"][0], [60.0, 80.0 + 50.0 * (1.0 + 0.5 * 0.0625)], atol=1e-12)      # k2 r2^2


def test_image_gate():
    pts = [at((60.0, 160.4)), at((60.0, 159.9)), at((0.9, 80.0)), at((119.9, 80.0))]
    r = run([kp((60.0, 159.5)), kp((119.5, 80.0))], [mp(p) for p in pts])
    assert [bool(np.isnan(p).any()) for p in r["proj_yx"]] == [True, False, True, False]
    assert list(r["best_kp"]) == [-1, 0, -1, 1]


def test_projection_distance_doubles_below_30_points():
    kps, mps = [kp((60.0, 83.0))], [mp(at((60.0, 80.0)))]
    assert list(run(kps, mps)["match"]) == [-1]
    assert list(run(kps, mps, fr=frame(nb_3d=29))["match"]) == [0]
    assert list(run(kps, mps, fr=frame(nb_3d=30))["match"]) == [-1]


def test_centre_cell_outside_the_grid_is_skipped_not_clamped():
    cam = (100.0, 100.0, 87.0, 70.0, 0.0, 0.0, 0.0, 0.0, 140, 175)              # 4 x 5 cells of 35: y = 139.7 rounds to 140 -> row 5
    pos = ((80.0 - 87.0) / 100.0 * 5.0, (139.7 - 70.0) / 100.0 * 5.0, 5.0)
    near, far = kp((139.2, 80.0)), kp((104.0, 80.0))                            # rows 4 and 3
    r = run([far, near], [mp(pos)], fr=frame(cam), params=P(proj=40.0))
    assert npl.to_cartesian(r["proj_yx"][0], 35) == (5, 3)
    assert list(r["best_kp"]) == [1]                                            # the last candidate wins: `far` would be it if row 3 were visited
    r = run([far], [mp(pos)], fr=frame(cam), params=P(proj=40.0))
    assert list(r["best_kp"]) == [-1]                                           # rows 4 .. 6 only: a clamped centre (row 4) would reach row 3
    # a centre one row further up does reach it
    up = ((80.0 - 87.0) / 100.0 * 5.0, (139.2 - 70.0) / 100.0 * 5.0, 5.0)
    assert list(run([far], [mp(up)], fr=frame(cam), params=P(proj=40.0))["best_kp"]) == [0]


def test_rounding_is_to_nearest_even():
    assert npl.to_cartesian((34.5, 35.5), 35) == (1, 2)                         # 34, 36
    assert npl.to_cartesian((69.5, 70.5), 35) == (3, 3)                         # 70, 70


def test_equal_distances_last_candidate_wins():
    # keypoint 1 lies in column 2 (x rounds to 69), keypoint 0 in column 3: the cells are visited c inner, so keypoint 0 comes LAST
    kps = [kp((60.0, 71.0)), kp((60.0, 69.4))]
    r = run(kps, [mp(at((60.0, 70.2)))])
    assert r["count"]["ties_forward"] == 1 and list(r["best_kp"]) == [0]
    # inside one cell: ascending list index
    r = run([kp((60.0, 80.0)), kp((60.5, 80.0)), kp((61.0, 80.0), DESC_B)], [mp(at((60.2, 80.0)))])
    assert list(r["best_kp"]) == [1] and r["best_dist"][0] == 0.0
    # a strictly smaller distance beats a later candidate
    r = run([kp((60.0, 80.0)), kp((60.5, 80.0), DESC_B)], [mp(at((60.2, 80.0)))])
    assert list(r["best_kp"]) == [0]


def test_reverse_selection_smallest_distance_then_last():
    kps = [kp((60.0, 80.0))]
    r = run(kps, [mp(at((60.2, 80.0))), mp(at((60.0, 80.3)), DESC_B), mp(at((59.9, 80.0)))])
    assert list(r["best_kp"]) == [0, 0, 0] and list(r["best_dist"]) == [0.0, 8.0, 0.0]
    assert list(r["match"]) == [2] and r["count"]["ties_reverse"] == 1 and r["count"]["contested"] == 1
    r = run(kps, [mp(at((60.2, 80.0))), mp(at((60.0, 80.3)), DESC_B)])
    assert list(r["match"]) == [0]


def test_descriptor_threshold_and_minimum_over_pairs():
    far = DESC_A ^ np.array([[0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0, 0]], dtype=np.uint64)     # 96 bits > 0.35 * 256 = 89.6
    r = run([kp((60.0, 80.0), far)], [mp(at((60.0, 80.0)))])
    assert list(r["best_kp"]) == [-1] and r["best_dist"][0] == 256.0 * 0.35
    both = np.concatenate([far, DESC_B])
    r = run([kp((60.0, 80.0), both)], [mp(at((60.0, 80.0)), np.concatenate([far ^ np.array([[1, 0, 0, 0]], dtype=np.uint64), DESC_A]))])
    assert list(r["best_kp"]) == [0] and r["best_dist"][0] == 1.0                # far vs far ^ 1


def test_no_listed_observer_passes_as_nan():
    target = at((60.0, 80.0), z=20.0)                                           # the keypoint's own point is at 5 m
    true_in_kf0 = (60.0, 100.0 * (0.0 + 0.5) / 5.0 + 80.0)
    assert list(run([kp((60.0, 80.0), observers=[(0, true_in_kf0)])], [mp(target)])["match"]) == [-1]     # 7.5 px off in key-frame 0
    r = run([kp((60.0, 80.0), observers=[(0, true_in_kf0)])], [mp(target)])
    assert r["count"]["average"] == 1
    assert list(run([kp((60.0, 80.0))], [mp(target)])["match"]) == [0]          # 0 / 0 = NaN > d is false
    assert list(run([kp((60.0, 80.0), observers=[(0, true_in_kf0)])], [mp(at((60.0, 80.0)))])["match"]) == [0]


def test_observer_overlap_rejects():
    obs = [(1, (60.0, 80.0))]
    assert list(run([kp((60.0, 80.0), observers=obs)], [mp(at((60.0, 80.0)), observers=[0])])["match"]) == [0]
    r = run([kp((60.0, 80.0), observers=obs)], [mp(at((60.0, 80.0)), observers=[0, 1])])
    assert list(r["match"]) == [-1] and r["count"]["overlap"] == 1


def test_keypoint_without_descriptors_is_skipped():
    none = np.zeros((0, 4), dtype=np.uint64)
    r = run([kp((60.0, 80.0), none), kp((60.5, 80.0), DESC_B)], [mp(at((60.0, 80.0)))])
    assert list(r["best_kp"]) == [1] and list(r["match"]) == [-1, 0]
    r = run([kp((60.0, 80.0), none)], [mp(at((60.0, 80.0)))])
    assert list(r["best_kp"]) == [-1] and np.array_equal(r["proj_yx"][0], [60.0, 80.0])


def test_margin_reports_the_closest_gate():
    r = run([kp((60.0, 81.875))], [mp(at((60.0, 80.0)))])
    assert math.isclose(r["margin"], 0.125, abs_tol=1e-9)                       # pixel distance 1.875 against 2.0 (the view gate is 0.22 away)
    r = run([kp((60.0, 80.0))], [mp((0.0, 0.0, 0.1 + 1e-12)), mp(at((60.0, 80.0)))])
    assert r["margin"] < 1e-11


def test_pack_round_trips_ragged_inputs(slam_host):
    none = np.zeros((0, 4), dtype=np.uint64)
    kps = [kp((1.0, 2.0), none), kp((3.0, 4.0), np.concatenate([DESC_A, DESC_B]), [(1, (5.0, 6.0)), (0, (7.0, 8.0))]), kp((9.0, 10.0), DESC_B)]
    mps = [mp((1.0, 2.0, 3.0), DESC_A, [1]), mp((4.0, 5.0, 6.0), none), mp((7.0, 8.0, 9.0), np.concatenate([DESC_B, DESC_A, DESC_B]), [0, 1])]
    fr = frame()
    fr["Tcw"] = np.arange(16.0).reshape(4, 4)
    p = slam_host.pack_local_map(fr, kps, K2, mps, P(3.0, 0.25))
    assert (p["N"], p["K"], p["M"]) == (3, 2, 3)
    assert list(p["Tcw"][0][:5]) == [0.0, 4.0, 8.0, 12.0, 1.0]                  # column-major
    assert p["kf_Tcw"].shape == (2, 16) and p["kf_Tcw"][0][12] == 0.5
    assert list(p["kp_desc_off"]) == [0, 0, 2, 3] and list(p["kp_obs_off"]) == [0, 0, 2, 2]
    assert list(p["mp_desc_off"]) == [0, 1, 1, 4] and list(p["mp_obs_off"]) == [0, 1, 1, 3]
    for j, k in enumerate(kps):
        assert np.array_equal(p["kp_desc"][p["kp_desc_off"][j]:p["kp_desc_off"][j + 1]], k["descriptors"])
        o = slice(p["kp_obs_off"][j], p["kp_obs_off"][j + 1])
        assert [(int(a), tuple(b)) for a, b in zip(p["kp_obs_kf"][o], p["kp_obs_yx"][o])] == k["observers"]
        assert tuple(p["kp_yx"][j]) == k["pixel"]
    for m, q in enumerate(mps):
        assert np.array_equal(p["mp_desc"][p["mp_desc_off"][m]:p["mp_desc_off"][m + 1]], q["descriptors"])
        assert list(p["mp_obs_kf"][p["mp_obs_off"][m]:p["mp_obs_off"][m + 1]]) == q["observers"]
    assert p["max_projection_distance"][0] == 3.0 and p["max_descriptor_distance"][0] == 0.25 and p["cell_size"].dtype == np.int32
    for name in ("kp_desc", "mp_desc"):
        assert p[name].dtype == np.uint64 and p[name].flags.c_contiguous
    # nothing at all
    e = slam_host.pack_local_map(fr, [], np.zeros((0, 4, 4)), [], P())
    assert (e["N"], e["K"], e["M"]) == (0, 0, 0) and list(e["kp_desc_off"]) == [0] and e["kp_desc"].shape == (0, 4) and e["mp_xyz"].shape == (0, 3)
    # a batch with an empty stream in the middle
    c, kp_off, kf_off, mp_off = slam_host.concat_packs([p, e, p])
    assert list(kp_off) == [0, 3, 3, 6] and list(kf_off) == [0, 2, 2, 4] and list(mp_off) == [0, 3, 3, 6]
    assert list(c["kp_desc_off"]) == [0, 0, 2, 3, 3, 5, 6] and list(c["mp_obs_off"]) == [0, 1, 1, 3, 4, 4, 6]
    assert np.array_equal(c["mp_desc"][4:], p["mp_desc"]) and list(c["kp_obs_kf"]) == [1, 0, 1, 0]


@pytest.mark.parametrize("seed", [0, 1])
def test_generator_makes_the_deliberate_ties(syn, seed):
    s = syn.local_map_scene(seed=seed)
    assert len(s["keypoints"]) == 150 and len(s["local_map"]) == 397 and s["keyframes"].shape == (6, 4, 4)
    r = npl.do_local_map_matching(s["frame"], s["keypoints"], s["keyframes"], s["local_map"], s["params"])
    c = r["count"]
    assert c["ties_forward"] > 0 and c["ties_reverse"] > 0 and c["contested"] > 0
    assert c["overlap"] > 0 and c["average"] > 0 and c["gated"] > 0 and (r["match"] >= 0).sum() > 20
    assert r["margin"] >= 1e-9
    assert sum(len(k["descriptors"]) == 0 for k in s["keypoints"]) > 0 and sum(len(k["observers"]) == 0 for k in s["keypoints"]) > 0
    t = syn.local_map_scene(seed=seed)
    assert all(np.array_equal(a["position"], b["position"]) for a, b in zip(s["local_map"], t["local_map"]))      # seeded
