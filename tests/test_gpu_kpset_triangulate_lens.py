"""GPU: slam_kpset_triangulate_lens (k_kpset_triangulate_lens, csrc/kpset.hip) -- triangulate_stereo! on the device-resident lists of a rig with two
different lenses -- against the model of tests/kpset_lens_cases.py (the C oracle's stereo triangulation fed with orc.undistort_point of both pixels) on
that module's case list: S = 3, cap 64, lists of 40, 0 and 64 keypoints uploaded with upload + upload_stereo; every gate fires, keypoints that are 3-D
already and keypoints without a stereo match are left alone.  tests/test_kpset_triangulate_lens_host.py shows that every gate quantity of the list is
1e-6 clear of its threshold, so the flags are array_equal; xyz within 1e-9 max(1, |world|), the bar of tests/test_gpu_kpset.py (the device's lens
model and DLT may contract multiply-adds).  Every test fails without slam_kpset_triangulate_lens / slam_kpset_upload_stereo."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kpset_lens_cases as kc  # noqa: E402

pytestmark = pytest.mark.gpu
FIELDS = ("yx", "is_3d", "xyz", "ids", "stereo_yx", "has_stereo")


@pytest.fixture(scope="module")
def lists(orc):
    return kc.build(orc)


def make_set(slam, lists):
    ks = slam.KeypointSet(kc.S, kc.CAP)
    for s, lst in enumerate(lists):
        ks.upload(s, lst["yx"], lst["is_3d"], lst["xyz"])
        ks.upload_stereo(s, lst["stereo_yx"], lst["has_stereo"])
    return ks


def as_bytes(d):
    return {k: np.ascontiguousarray(d[k]).tobytes() for k in FIELDS}


def check(got, lst, want):
    is3, has, xyz, acted = want
    assert np.array_equal(got["is_3d"], is3) and np.array_equal(got["has_stereo"], has)
    assert np.array_equal(got["yx"], lst["yx"]) and np.array_equal(got["stereo_yx"], lst["stereo_yx"])          # the lists keep the raw pixels
    new = acted & is3
    if new.any():
        assert np.abs(got["xyz"][new] - xyz[new]).max() <= 1e-9 * max(1.0, np.abs(xyz[new]).max())
    assert np.array_equal(got["xyz"][~new], lst["xyz"][~new])


def test_upload_stereo_round_trip(slam, lists):
    ks = make_set(slam, lists)
    try:
        assert list(ks.counts()) == list(kc.SIZES)
        for s, lst in enumerate(lists):
            got = ks.download(s)
            assert np.array_equal(got["stereo_yx"], lst["stereo_yx"]) and np.array_equal(got["has_stereo"], lst["has_stereo"])
            assert np.array_equal(got["yx"], lst["yx"]) and np.array_equal(got["is_3d"], lst["is_3d"])
        with pytest.raises(ValueError, match="flags"):           # pixels and flags of different lengths: refused before anything is copied
            ks.upload_stereo(0, lists[0]["stereo_yx"][:3], lists[0]["has_stereo"][:5])
    finally:
        ks.close()


def test_lens_triangulation_equals_the_model(slam, orc, lists):
    T21, Twc = kc.rig()
    ks = make_set(slam, lists)
    try:
        want = [kc.model(orc, lst, Twc[s]) for s, lst in enumerate(lists)]
        before = as_bytes(ks.download(2))
        with ks.selected((1, 1, 0)):                             # stream 2 is not selected: not a byte of it moves
            ks.triangulate(kc.CAM1, kc.CAM2, T21, Twc, kc.MAX_ERROR, kc.MIN_DEPTH, dist1=kc.DIST1, dist2=kc.DIST2)
        assert as_bytes(ks.download(2)) == before
        check(ks.download(0), lists[0], want[0])
        assert list(ks.counts()) == list(kc.SIZES)               # nothing is compacted away
        ks.triangulate(kc.CAM1, kc.CAM2, T21, Twc, kc.MAX_ERROR, kc.MIN_DEPTH, dist1=kc.DIST1, dist2=kc.DIST2)
        for s in (0, 2):                                         # (stream 0 has no candidate left: the second call finds nothing to do there)
            check(ks.download(s), lists[s], want[s])
        assert len(ks.download(1)["yx"]) == 0
        assert sum(int((w[3] & w[0]).sum()) for w in want) >= 20 and sum(int((w[3] & ~w[1]).sum()) for w in want) >= 8
    finally:
        ks.close()


def test_zero_distortion_is_the_pinhole_call_byte_for_byte(slam, orc, lists):
    T21, Twc = kc.rig()
    a, b = make_set(slam, lists), make_set(slam, lists)
    try:
        zero = np.zeros(4)
        a.triangulate(kc.CAM1, kc.CAM2, T21, Twc, kc.MAX_ERROR, kc.MIN_DEPTH)
        b.triangulate(kc.CAM1, kc.CAM2, T21, Twc, kc.MAX_ERROR, kc.MIN_DEPTH, dist1=zero, dist2=zero)
        changed = 0
        for s, lst in enumerate(lists):
            da, db = a.download(s), b.download(s)
            assert as_bytes(da) == as_bytes(db), s
            changed += int((da["is_3d"] & ~lst["is_3d"]).sum())
        assert changed >= 10                                     # the pinhole call did accept keypoints: the comparison is not of two idle calls
    finally:
        a.close(); b.close()


def _projections(T21):
    from slam_jl_amd.triangulation import projection_matrices
    return projection_matrices(kc.CAM1, kc.CAM2, T21)


def test_one_lens_is_enough_to_take_the_lens_path(slam, orc, lists):
    """dist2 = None stands for a right camera without a lens: its pixel is used as stored, the left one is undistorted"""
    T21, Twc = kc.rig()
    ks = make_set(slam, lists)
    try:
        ks.triangulate(kc.CAM1, kc.CAM2, T21, Twc, kc.MAX_ERROR, kc.MIN_DEPTH, dist1=kc.DIST1)
        for s, lst in enumerate(lists):
            if len(lst["yx"]) == 0:
                continue
            cand = lst["has_stereo"] & ~lst["is_3d"]
            P1, P2 = _projections(T21)
            X, ok = orc.triangulate(P1, P2, T21, kc.CAM1, kc.CAM2, kc.undistorted(orc, kc.CAM1, kc.DIST1, lst["yx"][cand]), lst["stereo_yx"][cand],
                                    kc.MAX_ERROR, kc.MIN_DEPTH)
            z1, z2, d1, d2, _ = kc.gates(orc, T21, kc.undistorted(orc, kc.CAM1, kc.DIST1, lst["yx"][cand]), lst["stereo_yx"][cand])
            clear = kc.margin_of(z1, z2, d1, d2) >= kc.MARGIN     # (the case list was chosen clear of the thresholds for two lenses, not for one)
            got = ks.download(s)
            idx = np.flatnonzero(cand)[clear]
            assert np.array_equal(got["is_3d"][idx], ok[clear]) and np.array_equal(got["has_stereo"][idx], ok[clear]) and len(idx) >= 20, s
    finally:
        ks.close()
