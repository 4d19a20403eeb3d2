"""GPU: the boundaries owned by the routines of csrc/geom_device.hpp that several kernels share -- the RANSAC select body at the
LDS / global-memory edge of its error staging (4096 elements) in the keypoint-set layout, the 1024-thread cell scan at its chunk
edge, and the 256-thread ordered compactions at theirs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [4096, 4097, 4]                  # eligible keypoints per stream: staged in LDS, in global memory, below both estimators' minimum
CAP = 4352


def _interleave(rng, n_el, n_extra):
    order = rng.permutation(n_el + n_extra)
    return order[:n_el], order[n_el:]


def test_p3p_select_in_set_layout_across_the_error_staging_edge(slam, syn):
    """slam_kpset_compute_pose, S = 3, cap = 4352, 16 iterations, 4096 / 4097 / 4 three-dimensional keypoints, against
    slam_p3p_ransac_batch fed the gathered arrays and the same triples (the route of
    test_compute_pose_on_the_set_equals_the_host_seams).  The set seam hands back the inlier count, the status and the lists
    (exact) and the pose after its PnP refinement (compared as in that test: the refinement's start angles are formed by the
    device's atan2 there and by the host's here).  The winning iteration and the summed error stay in device scratch in the set
    seam; they are compared, exactly, between the S = 3 call and single-problem calls of the host seam on the same arrays."""
    S, cam, dist = 3, syn.KITTI_CAM, (0.0, 0.0, 0.0, 0.0)
    ks = slam.KeypointSet(S, CAP)
    rng = np.random.default_rng(41)
    for s, n3 in enumerate(SIZES):
        sc = syn.p3p_scene(n=n3, seed=30 + s, noise_px=0.3, outlier_frac=0.2, iters=4)
        n2 = 100
        e3, e2 = _interleave(rng, n3, n2)
        yx = np.zeros((n3 + n2, 2)); is3 = np.zeros(n3 + n2, bool); xyz = np.zeros((n3 + n2, 3))
        yx[e3] = sc["px_xy"][:, ::-1]; is3[e3] = True; xyz[e3] = sc["pts3d"]
        yx[e2] = rng.uniform(5, 300, (n2, 2))
        ks.upload(s, yx, is3, xyz)
    sp = slam.stream_params(S, cam=cam, dist=dist)
    before = [ks.download(s) for s in range(S)]
    iters, seed, thr = 16, 9, 3.0
    poses, status, ninl, counts = ks.compute_pose(sp, threshold=thr, iters=iters, seed=seed)
    after = [ks.download(s) for s in range(S)]
    K = np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1.0]])
    P, X, B, SM, idx3 = [], [], [], [], []
    for s in range(S):
        m = before[s]["is_3d"].astype(bool)
        assert m.sum() == SIZES[s]
        pts, px, pdn = slam.pose_inputs(cam, dist, before[s]["yx"][m], before[s]["xyz"][m])
        P.append(px); X.append(pts); B.append(pdn); idx3.append(np.flatnonzero(m))
        SM.append(slam.pose_samples(seed, s, int(m.sum()), iters))
    r3 = slam.p3p_ransac_batch(X, P, B, K, threshold=thr, samples=SM)
    for s in range(2):                                           # batch of three == one problem at a time: every output of the select body
        r1 = slam.p3p_ransac(X[s], P[s], B[s], K, threshold=thr, samples=SM[s], return_pose=True)
        assert r1[0] == r3[s][0] and np.array_equal(r1[1][0], r3[s][1][0]) and np.array_equal(r1[1][1], r3[s][1][1])
        assert r1[1][2] == r3[s][1][2] and np.array_equal(r1[1][3], r3[s][1][3]) and r1[1][4] == r3[s][1][4]
    assert r3[2] is None
    T0 = [np.eye(4) for _ in range(S)]; bp = [np.zeros((0, 2))] * S; bx = [np.zeros((0, 3))] * S
    for s in range(2):
        assert r3[s][0] >= 5
        inl = r3[s][1][1]
        T0[s][:3] = r3[s][1][3]; bp[s] = P[s][inl][:, ::-1]; bx[s] = X[s][inl]
    rb = slam.pnp_bundle_adjustment_batch(cam, T0, bp, bx, repr_eps=thr)
    for s in range(2):
        inl = r3[s][1][1]
        newT, e0, e1, outl, no = rb[s]
        assert not (int(inl.sum()) - no < 5 or e1 > e0)
        keep = np.ones(len(before[s]["yx"]), bool)
        keep[idx3[s][~inl]] = False
        keep[idx3[s][inl][outl]] = False
        assert status[s] == 1 and ninl[s] == r3[s][0] == int(inl.sum()), s
        assert np.allclose(poses[s], newT, rtol=0, atol=1e-9), (s, np.abs(poses[s] - newT).max())
        assert counts[s] == keep.sum() == len(after[s]["yx"]), (s, counts[s], keep.sum())
        for k in ("yx", "ids", "is_3d", "xyz"):
            assert np.array_equal(after[s][k], before[s][k][keep]), (s, k)
    assert status[2] == 0 and ninl[2] == 0 and np.array_equal(poses[2], np.eye(4)) and counts[2] == len(before[2]["yx"])
    for k in ("yx", "ids", "is_3d", "xyz"):
        assert np.array_equal(after[2][k], before[2][k]), k
    ks.close()


def test_5pt_select_in_set_layout_across_the_error_staging_edge(slam, syn):
    """slam_kpset_compute_pose_5pt, S = 3, cap = 4352, 16 iterations, 4096 / 4097 / 4 keypoints the key-frame observes, against
    slam_five_point_ransac_batch fed the gathered pairs and the same 5-tuples: [R | t], inlier count, status and the surviving
    lists, exactly.  Winning iteration and summed error: as in the P3P test above."""
    S, cam, dist = 3, syn.KITTI_CAM, (0.0, 0.0, 0.0, 0.0)
    ks = slam.KeypointSet(S, CAP)
    rng = np.random.default_rng(43)
    for s, n5 in enumerate(SIZES):
        fs = syn.five_point_scene(n=n5, seed=70 + s, noise_px=0.3, outlier_frac=0.2, iters=4)
        extra = 100
        e5, ex = _interleave(rng, n5, extra)
        yx = rng.uniform(5, 300, (n5 + extra, 2)); kyx = np.zeros((n5 + extra, 2)); hk = np.zeros(n5 + extra, bool)
        yx[e5] = fs["px2"][:, ::-1]; kyx[e5] = fs["px1"][:, ::-1]; hk[e5] = True
        ks.upload(s, yx, np.zeros(n5 + extra, bool))
        ks.upload_keyframe(s, kyx, hk)
    sp = slam.stream_params(S, Tcw=np.eye(4), cam=cam, dist=dist)
    before = [ks.download(s) for s in range(S)]
    kf = [ks.download_keyframe(s) for s in range(S)]
    iters, seed, thr = 16, 5, 3.0
    Rt, status, ninl, par, counts = ks.compute_pose_5pt(sp, min_parallax=5.0, max_repr_error=thr, iters=iters, seed=seed)
    after = [ks.download(s) for s in range(S)]
    K = np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1.0]])
    A1, A2, D1, D2, SM, idx = [], [], [], [], [], []
    for s in range(S):
        m = kf[s][1]
        assert m.sum() == SIZES[s]
        p1, p2, d1, d2 = slam.pose_5pt_inputs(cam, dist, before[s]["yx"][m], kf[s][0][m])
        A1.append(p1); A2.append(p2); D1.append(d1); D2.append(d2); idx.append(np.flatnonzero(m))
        SM.append(slam.pose_samples5(seed, s, int(m.sum()), iters) if s < 2 else np.full((iters, 5), -1, np.int32))
        if s < 2:
            assert np.linalg.norm(p2 - p1, axis=1).mean() >= 5.0
    r5 = slam.five_point_ransac_batch(A1, A2, D1, D2, K, K, max_repr_error=thr, samples=SM)
    for s in range(2):
        r1 = slam.five_point_ransac(A1[s], A2[s], D1[s], D2[s], K, K, max_repr_error=thr, samples=SM[s], return_extra=True)
        assert r1[0] == r5[s][0] and all(np.array_equal(r1[1][k], r5[s][1][k]) for k in range(3))
        assert r1[1][3] == r5[s][1][3] and r1[1][4] == r5[s][1][4]
        n_in, inl = r5[s][0], r5[s][1][2]
        assert 5 <= n_in < len(inl)
        keep = np.ones(len(before[s]["yx"]), bool)
        keep[idx[s][~inl]] = False
        assert status[s] == 1 and ninl[s] == n_in, s
        assert np.array_equal(Rt[s], r5[s][1][1]), (s, np.abs(Rt[s] - r5[s][1][1]).max())
        assert counts[s] == keep.sum() == len(after[s]["yx"]), (s, counts[s], keep.sum())
        assert np.array_equal(after[s]["ids"], before[s]["ids"][keep]) and np.array_equal(after[s]["yx"], before[s]["yx"][keep]), s
        k2, h2 = ks.download_keyframe(s)
        assert np.array_equal(h2, kf[s][1][keep]) and np.array_equal(k2[h2], kf[s][0][keep][h2]), s
    assert status[2] == 0 and ninl[2] == 0 and not Rt[2].any() and counts[2] == len(before[2]["yx"])
    assert np.array_equal(after[2]["ids"], before[2]["ids"]) and np.array_equal(after[2]["yx"], before[2]["yx"])
    ks.close()


def test_cell_scan_across_its_1024_cell_chunk(slam, syn, orc):
    """cell_size 8 on a 200 x 328 image: 25 x 41 = 1025 cells, the second chunk of the scan holds the last cell alone (the oracle puts two
    keypoints there for this texture).  slam_detect_pyr, slam_detect_batch (S = 2) and slam_kpset_detect (S = 2) with a non-empty
    avoidance list and sigma_mask = 1: index for index the oracle's list."""
    import torch
    H, W, S = 200, 328, 2
    imgs = [np.asfortranarray(syn.texture_canvas(H, W, seed=70 + s, margin=0)) for s in range(S)]
    e = slam.Extractor(2100, 5, (25, 41), 8)
    rng = np.random.default_rng(5)
    cur = [np.stack([rng.uniform(1, H - 20, 60), rng.uniform(1, W - 20, 60)], axis=1) for s in range(S)]
    ref = [orc.detect(imgs[s], cur[s], max_points=2100, radius=5, cell_size=8, sigma_mask=1.0) for s in range(S)]
    for s in range(S):
        assert orc.grid_resolution(H, W, 8) == (25, 41) and ((ref[s][:, 0] > 192) & (ref[s][:, 1] > 320)).sum() >= 1, s
    dev = [torch.from_numpy(np.ascontiguousarray(im.T)).cuda() for im in imgs]
    torch.cuda.synchronize()
    batch = slam.PyramidBatch((H, W), levels=1, S=S)
    batch.update_([d.data_ptr() for d in dev])
    for s in range(S):
        assert np.array_equal(slam.detect(e, batch.pyramids[s], cur[s], sigma_mask=1.0), ref[s]), s
    kp, ksid = slam.detect_batch(e, batch, np.concatenate(cur), np.repeat(np.arange(S, dtype=np.int32), 60), sigma_mask=1.0)
    ks = slam.KeypointSet(S, 2100 + 1025 + 8)
    for s in range(S):
        assert np.array_equal(kp[ksid == s], ref[s]), s
        ks.upload(s, cur[s], np.zeros(60, bool))
    ks.detect(e, batch, sigma_mask=1.0)
    for s in range(S):
        d = ks.download(s)
        assert np.array_equal(d["yx"][:60], cur[s]) and np.array_equal(d["yx"][60:], ref[s].astype(float)), s
        assert np.array_equal(d["ids"], np.arange(60 + len(ref[s]))), s
    ks.close()


def test_ordered_compactions_at_their_256_slot_chunk(slam, syn):
    """Lists of 255, 256, 257 and 513 keypoints (S = 4, cap = 640): slam_kpset_remove with every third flag set, then
    slam_kpset_compute_pose_5pt with the key-frame observing every second keypoint -- every field of the surviving lists against
    numpy's stable compaction (boolean indexing), the five-point route restated as in test_compute_pose_5pt_on_the_set_equals_the_host_seam."""
    import torch
    S, cap, sizes = 4, 640, [255, 256, 257, 513]
    cam, dist = syn.KITTI_CAM, (0.0, 0.0, 0.0, 0.0)
    ks = slam.KeypointSet(S, cap)
    rng = np.random.default_rng(17)
    flags = np.zeros((S, cap), np.uint8)
    host = []
    for s, n in enumerate(sizes):
        fs = syn.five_point_scene(n=n, seed=90 + s, noise_px=0.3, outlier_frac=0.25, iters=4)
        yx = fs["px2"][:, ::-1].copy(); kyx = fs["px1"][:, ::-1].copy()
        is3 = rng.uniform(size=n) < 0.5; xyz = rng.normal(size=(n, 3)); hk = np.arange(n) % 2 == 0
        ids = 1000 * s + 3 * np.arange(n, dtype=np.int64)
        ks.upload(s, yx, is3, xyz, ids=ids)
        ks.upload_keyframe(s, kyx, hk)
        flags[s, :n:3] = 1
        host.append(dict(yx=yx, is_3d=is3, xyz=xyz, ids=ids, kyx=kyx, hk=hk))
    fl = torch.from_numpy(flags).cuda()
    torch.cuda.synchronize()
    ks.remove(fl.data_ptr())
    before, kf = [], []
    for s, n in enumerate(sizes):
        keep = flags[s, :n] == 0
        d = ks.download(s); k2, h2 = ks.download_keyframe(s)
        assert len(d["yx"]) == keep.sum() == n - (n + 2) // 3, s
        for k in ("yx", "is_3d", "xyz", "ids"):
            assert np.array_equal(d[k], host[s][k][keep]), (s, k)
        assert not d["has_stereo"].any() and np.array_equal(h2, host[s]["hk"][keep]) and np.array_equal(k2[h2], host[s]["kyx"][keep][h2]), s
        before.append(d); kf.append((k2, h2))
    del fl
    iters, seed, thr = 32, 21, 3.0
    sp = slam.stream_params(S, Tcw=np.eye(4), cam=cam, dist=dist)
    Rt, status, ninl, par, counts = ks.compute_pose_5pt(sp, min_parallax=5.0, max_repr_error=thr, iters=iters, seed=seed)
    K = np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1.0]])
    A1, A2, D1, D2, SM, idx = [], [], [], [], [], []
    for s in range(S):
        m = kf[s][1]
        p1, p2, d1, d2 = slam.pose_5pt_inputs(cam, dist, before[s]["yx"][m], kf[s][0][m])
        assert np.linalg.norm(p2 - p1, axis=1).mean() >= 5.0
        A1.append(p1); A2.append(p2); D1.append(d1); D2.append(d2); idx.append(np.flatnonzero(m))
        SM.append(slam.pose_samples5(seed, s, int(m.sum()), iters))
    r5 = slam.five_point_ransac_batch(A1, A2, D1, D2, K, K, max_repr_error=thr, samples=SM)
    for s in range(S):
        n_in, inl = r5[s][0], r5[s][1][2]
        assert 5 <= n_in < len(inl), (s, n_in)
        keep = np.ones(len(before[s]["yx"]), bool)
        keep[idx[s][~inl]] = False
        assert status[s] == 1 and ninl[s] == n_in and np.array_equal(Rt[s], r5[s][1][1]), s
        d = ks.download(s); k2, h2 = ks.download_keyframe(s)
        assert counts[s] == keep.sum() == len(d["yx"]), (s, counts[s], keep.sum())
        for k in ("yx", "is_3d", "xyz", "ids"):
            assert np.array_equal(d[k], before[s][k][keep]), (s, k)
        assert np.array_equal(h2, kf[s][1][keep]) and np.array_equal(k2[h2], kf[s][0][keep][h2]), s
    ks.close()
