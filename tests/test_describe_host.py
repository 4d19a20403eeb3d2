"""CPU: the precondition of tests/test_gpu_describe_dev.py -- on its frames describe() (extractor.jl:103-105) drops detected keypoints at the
border, for every stream and window, so a device path that forgot the drop cannot pass there -- and the three device-pyramid describe entry
points have no CPU fallback."""
import numpy as np
import pytest

import describe_cases as dc


@pytest.mark.parametrize("window", dc.WINDOWS)
def test_oracle_describe_drops_detected_keypoints(orc, syn, slam_host, window):
    pat = slam_host.brief_pattern(64, window)
    cases = [(dc.as_f64(dc.frames(syn, H, W, seed=0)[0][0][1]), 150, None) for H, W in dc.SINGLE_SHAPES]
    cases += [(dc.as_f64(dc.set_stream(syn, s)[0][0][1]), dc.SET_MAX_POINTS, dc.SET_GRID) for s in range(dc.SET_S)]
    cases += [(dc.as_f64(dc.wide_frame(syn, s)), dc.WIDE_MAX_POINTS, dc.WIDE_GRID) for s in (0, 35, 71)]
    for img, max_points, grid in cases:
        kp = orc.detect(img, np.zeros((0, 2)), max_points=max_points, grid=grid)
        bits, rc = orc.describe(img, kp, pat, window=window)
        assert 0 < len(rc) < len(kp), (img.shape, window, len(kp), len(rc))
        lim = (window + 1) // 2
        H, W = img.shape
        inside = (kp[:, 0] - lim >= 1) & (kp[:, 0] + lim <= H) & (kp[:, 1] - lim >= 1) & (kp[:, 1] + lim <= W)
        assert np.array_equal(rc, kp[inside])                       # order kept


def test_hand_placed_keypoints_sit_on_the_drop_boundary(orc, syn, slam_host):
    for H, W in dc.SINGLE_SHAPES:
        img = dc.as_f64(dc.frames(syn, H, W, seed=0)[0][0][1])
        for window in dc.WINDOWS:
            kept, dropped = dc.hand_placed(H, W, window)
            _, rc = orc.describe(img, np.concatenate([kept, dropped]), dc.edge_pattern(64, window), window=window)
            assert np.array_equal(rc, kept), (H, W, window)


def test_device_describe_has_no_cpu_fallback(slam_host):
    """without a HIP device nothing describes: the single form raises at its context, and neither a PyramidBatch (describe_batch) nor a
    KeypointSet (detect_describe) can come to exist -- as test_abi.test_no_cpu_fallback_without_device shows for the other seams"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    for name in ("slam_describe_pyr", "slam_describe_batch", "slam_kpset_detect_describe"):
        assert hasattr(slam_host.load(), name)                      # bound and exported: what fails below is the device, not a missing symbol
    raises = pytest.raises(slam_host.SlamHipError, match="no HIP device|slam_ctx_create")
    pyr = slam_host.LKPyramid.__new__(slam_host.LKPyramid)          # (no handle: construction itself needs a context)
    with raises:
        slam_host.describe(slam_host.Extractor(150, 17, (4, 5), 35), pyr, np.array([[20, 20]]))
    with raises:
        slam_host.PyramidBatch((64, 80), levels=2, S=2)
    with raises:
        slam_host.KeypointSet(2, 200)
