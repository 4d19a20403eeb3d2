"""CPU: the host-side restatements that accompany the device-resident pose seams (slam.jl_amd/keypoint_set.py): the tuple
generator the kernels share with the tests, the gather arithmetic against the oracle's camera model, the pose composition."""
import numpy as np


def test_pose_samples_are_distinct_deterministic_and_in_range(slam_host):
    a = slam_host.pose_samples(77, 3, 41, 200)
    b = slam_host.pose_samples(77, 3, 41, 200)
    assert np.array_equal(a, b) and a.dtype == np.int32 and a.shape == (200, 3)
    assert a.min() >= 0 and a.max() < 41
    assert all(len(set(r)) == 3 for r in a.tolist())
    assert not np.array_equal(a, slam_host.pose_samples(78, 3, 41, 200)) and not np.array_equal(a, slam_host.pose_samples(77, 4, 41, 200))
    assert (slam_host.pose_samples(1, 0, 4, 8) == -1).all()                    # fewer than five 3-D keypoints: no P3P (front_end.jl:133)
    f = slam_host.pose_samples5(5, 1, 9, 64)
    assert f.shape == (64, 5) and f.min() >= 0 and f.max() < 9 and all(len(set(r)) == 5 for r in f.tolist())
    # the first draw of a stream is the plain generator value: splitmix64(seed ^ stream << 48 ^ it << 16 ^ attempt) mod n
    from slam_jl_amd.keypoint_set import _splitmix64
    assert a[0, 0] == _splitmix64(77 ^ (3 << 48)) % 41
    assert _splitmix64(0) == 0xE220A8397B1DCDAF                            # reference value of the published generator


def test_pose_inputs_follow_the_camera_model(slam_host, orc, syn):
    cam = syn.KITTI_CAM
    dist = (-0.28, 0.07, 2e-4, -1e-4)
    rng = np.random.default_rng(2)
    yx = np.stack([rng.uniform(1, 370, 50), rng.uniform(1, 1226, 50)], axis=1)
    xyz = rng.normal(0, 5, (50, 3))
    pts, px, pdn = slam_host.pose_inputs(cam, dist, yx, xyz)
    assert np.array_equal(pts, xyz)
    for i in range(50):
        u = orc.undistort_point(cam, dist, yx[i])                          # camera.jl:98-125, (y, x)
        assert np.allclose(px[i], u[::-1], rtol=0, atol=1e-12)             # P3P takes (x, y): front_end.jl:151
        b = np.array([(u[1] - cam[2]) / cam[0], (u[0] - cam[3]) / cam[1], 1.0])     # backproject, camera.jl:138-140
        assert np.allclose(pdn[i], b / np.linalg.norm(b), rtol=0, atol=1e-15)
    p1, p2, d1, d2 = slam_host.pose_5pt_inputs(cam, dist, yx, yx + 3.0)
    assert np.allclose(p2, px) and np.allclose(d2[:, 0], (px[:, 0] - cam[2]) / cam[0]) and p1.shape == p2.shape == d1.shape == (50, 2)


def test_pose_5pt_compose_scales_and_chains(slam_host):
    th = 0.1
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
    Rt = np.concatenate([R, np.array([[0.6], [0.0], [0.8]])], axis=1)      # |t| = 1
    prev_cw = np.eye(4); prev_cw[:3, 3] = [1.0, 2.0, 3.0]
    cur_wc = np.eye(4); cur_wc[:3, 3] = [-1.0, -2.0, -0.5]                 # motion model: 2.5 m from the key-frame (front_end.jl:322-324)
    T = slam_host.pose_5pt_compose(Rt, prev_cw, cur_wc)
    rel = T @ np.linalg.inv(prev_cw)
    assert np.allclose(rel[:3, :3], R) and np.allclose(rel[:3, 3], 2.5 * np.array([0.6, 0.0, 0.8]))


def test_parameter_slot_constants_match_the_header(slam_host):
    """KP_PAR* of csrc/kpset.hpp (read from the header text) are keypoint_set.py's module constants, and stream_params puts camera,
    distortion and shift at exactly those columns."""
    import os
    import re
    from slam_jl_amd import keypoint_set as K
    text = open(os.path.join(os.path.dirname(K.__file__), "csrc", "kpset.hpp")).read()
    line = re.search(r"^constexpr int (KP_PAR\b.*);$", text, re.M).group(1)
    hdr = {m.group(1): int(m.group(2)) for m in re.finditer(r"(KP_PAR\w*) = (\d+)", line)}
    assert hdr == {"KP_PAR": K.KP_PAR, "KP_PAR_CAM": K.KP_PAR_CAM, "KP_PAR_DIST": K.KP_PAR_DIST, "KP_PAR_SHIFT": K.KP_PAR_SHIFT}
    T = np.arange(16.0).reshape(4, 4) + 100
    p = K.stream_params(3, Tcw=T, cam=(1.5, 2.5, 3.5, 4.5), dist=(5.5, 6.5, 7.5, 8.5), shift_yx=[[9.5, 10.5], [11.5, 12.5], [13.5, 14.5]])
    assert p.shape == (3, hdr["KP_PAR"]) and p.flags["C_CONTIGUOUS"]
    want = np.zeros((3, hdr["KP_PAR"]))
    want[:, :16] = T.T.reshape(16)                                             # column-major
    want[:, hdr["KP_PAR_CAM"]:hdr["KP_PAR_CAM"] + 4] = (1.5, 2.5, 3.5, 4.5)
    want[:, hdr["KP_PAR_DIST"]:hdr["KP_PAR_DIST"] + 4] = (5.5, 6.5, 7.5, 8.5)
    want[:, hdr["KP_PAR_SHIFT"]:hdr["KP_PAR_SHIFT"] + 2] = [[9.5, 10.5], [11.5, 12.5], [13.5, 14.5]]
    assert np.array_equal(p, want)
    d = K.stream_params(2)                                                     # the defaults: fx = fy = 1, everything else 0
    want = np.zeros((2, hdr["KP_PAR"])); want[:, hdr["KP_PAR_CAM"]:hdr["KP_PAR_CAM"] + 2] = 1.0
    assert np.array_equal(d, want)


def test_pose_samples_equal_the_recorded_arrays(slam_host):
    """tests/golden/pose_samples_v1.npz: pose_samples / pose_samples5 over a small grid of (seed, stream, n, iters), recorded from the two
    spelled-out loops before they became one (_samples); the n = 4 entry is pose_samples' all -1 exit."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_samples_v1.npz"))
    assert len(g["grid"]) == 5
    for i, (seed, stream, n, iters) in enumerate(g["grid"].tolist()):
        a = slam_host.pose_samples(seed, stream, n, iters)
        assert a.dtype == np.int32 and np.array_equal(a, g[f"s3_{i}"]), i
        if n >= 5:
            b = slam_host.pose_samples5(seed, stream, n, iters)
            assert b.dtype == np.int32 and np.array_equal(b, g[f"s5_{i}"]), i
        else:
            assert (a == -1).all() and a.shape == (iters, 3)
