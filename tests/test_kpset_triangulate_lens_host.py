"""CPU: the case list of tests/kpset_lens_cases.py, which tests/test_gpu_kpset_triangulate_lens.py runs on the device, is a fair one -- under the model
(the C oracle's stereo triangulation fed with orc.undistort_point of both pixels), for every keypoint the call acts on (a stereo match, not 3-D yet):
  * the four gate quantities -- the depth in either camera against min_depth = 0.1, the reprojection distance in either image against max_error = 3 --
    lie at least 1e-6 from their thresholds, so no verdict hangs on the last bits of the lens model or the DLT;
  * each of the four gates rejects at least one keypoint and at least ten pass, on every stream that has keypoints;
and the lists hold keypoints that are 3-D already and keypoints without a stereo match.  The lens matters: with the lenses left out of the call the
verdicts differ."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kpset_lens_cases as kc  # noqa: E402

GATES = ("depth1", "depth2", "left", "right")


def test_every_gate_quantity_is_clear_of_its_threshold(orc):
    T21, _ = kc.rig()
    for s, lst in enumerate(kc.build(orc)):
        z1, z2, d1, d2, cls = kc.gates(orc, T21, kc.undistorted(orc, kc.CAM1, kc.DIST1, lst["yx"]), kc.undistorted(orc, kc.CAM2, kc.DIST2, lst["stereo_yx"]))
        margin = kc.margin_of(z1, z2, d1, d2)
        print(f"stream {s}: {len(cls)} keypoints, smallest margin {margin.min() if len(margin) else float('inf'):.3g}")
        assert np.all(np.isfinite(margin)) and np.all(margin >= kc.MARGIN), s
        assert np.array_equal(cls, lst["cls"])


def test_every_gate_rejects_and_ten_pass_per_stream(orc):
    _, Twc = kc.rig()
    lists = kc.build(orc)
    assert [len(l["yx"]) for l in lists] == list(kc.SIZES) and 0 in kc.SIZES and kc.CAP in kc.SIZES
    for s, lst in enumerate(lists):
        if len(lst["yx"]) == 0:
            continue
        is3, has, xyz, acted = kc.model(orc, lst, Twc[s])
        counts = {c: int(np.sum(acted & (lst["cls"] == c))) for c in kc.CLASSES}
        print(f"stream {s}: of the keypoints acted on {counts}; 3-D already {int(lst['is_3d'].sum())}, without a stereo match {int((~lst['has_stereo']).sum())}")
        assert all(counts[g] >= 1 for g in GATES) and counts["pass"] >= 10, (s, counts)
        assert lst["is_3d"].sum() >= 2 and (~lst["has_stereo"]).sum() >= 2
        # the model's verdicts are the classes: a passing keypoint becomes 3-D, a rejected one loses its stereo observation, the others are untouched
        assert np.array_equal(is3, lst["is_3d"] | (acted & (lst["cls"] == "pass")))
        assert np.array_equal(has, lst["has_stereo"] & ~(acted & (lst["cls"] != "pass")))
        assert np.array_equal(xyz[~(acted & (lst["cls"] == "pass"))], lst["xyz"][~(acted & (lst["cls"] == "pass"))])


def test_without_the_lenses_the_verdicts_differ(orc):
    _, Twc = kc.rig()
    zero = ((0.0,) * 4, (0.0,) * 4)
    for s, lst in enumerate(kc.build(orc)):
        if len(lst["yx"]) == 0:
            continue
        a, b = kc.model(orc, lst, Twc[s]), kc.model(orc, lst, Twc[s], dists=zero)
        assert not np.array_equal(a[0], b[0]) or not np.array_equal(a[1], b[1]), s
        both = a[0] & b[0] & a[3]                                # where both accept, the map points are far apart: the lens is no rounding matter
        assert both.any() and np.abs(a[2][both] - b[2][both]).max() > 1e-3, s
