"""Byte comparison of the device-resident keypoint lists between two builds of the library: one scripted sequence through every slam_kpset_*
seam at S = 3 and at S = 70 (96 x 128 synthetic stereo streams), every downloadable field of every stream dumped after every call, with the
poses, statuses, inlier counts, parallaxes, frame statistics and descriptors the calls return.
    python scripts/probes/kpset_dump.py dump OUT.npz           the library is the package's, or the one SLAMHIP_LIB names
    python scripts/probes/kpset_dump.py compare A.npz B.npz    every array byte for byte; exit status 1 if any differs"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
H, W = 96, 128


def sequence(slam, syn, S, out):
    import torch
    params = slam.Params(stereo=True, max_nb_keypoints=80)
    cam = syn.KITTI_CAM
    e = slam.Extractor.from_params(params, slam.Camera(*cam, height=H, width=W))
    ncell = e.grid_resolution[0] * e.grid_resolution[1]
    cap = params.max_nb_keypoints + ncell + 8
    streams = [syn.stereo_stream((H, W), 3, 30 + s, (1.0 + 0.02 * s, -1.4), 6.3) for s in range(S)]
    keep = []

    def batch(side, k):
        b = slam.PyramidBatch((H, W), levels=3, S=S)
        d = [torch.from_numpy(np.ascontiguousarray(st[side][k].T)).cuda() for st in streams]
        torch.cuda.synchronize()
        b.update_([x.data_ptr() for x in d]); keep.append(d)
        return b
    l0, l1, l2, r1 = batch(0, 0), batch(0, 1), batch(0, 2), batch(1, 1)
    ks = slam.KeypointSet(S, cap)
    step = [0]

    def dump(tag, **extra):
        pre = f"S{S}/{step[0]:02d}_{tag}/"; step[0] += 1
        out[pre + "counts"] = ks.counts()
        for s in range(S):
            d = ks.download(s); k, hk = ks.download_keyframe(s); f, fk, kc = ks.download_first(s)
            for key, v in list(d.items()) + [("kyx", k), ("has_kf", hk), ("first_yx", f), ("first_kf", fk), ("kf_count", np.array([kc]))]:
                out[pre + f"{s}/{key}"] = np.asarray(v)
        for key, v in extra.items():
            out[pre + key] = np.asarray(v)

    rng = np.random.default_rng(S)
    for s in range(S):                                           # ragged lists on a grid, half of them 3-D; stream 1 starts empty
        n = 0 if s == 1 else 20 + (s * 7) % 40
        yx = np.stack([rng.uniform(8, H - 8, n), rng.uniform(8, W - 8, n)], axis=1)
        is3 = np.arange(n) % 2 == 0
        ks.upload(s, yx, is3, np.where(is3[:, None], rng.normal(0, 1, (n, 3)) + [0, 0, 8.0], 0.0), ids=5 + np.arange(n) if s % 2 else None)
        ks.upload_keyframe(s, yx + rng.normal(0, 1.5, (n, 2)), rng.random(n) < 0.7)
        ks.upload_first(s, yx + rng.normal(0, 3.0, (n, 2)), rng.integers(0, 3, n).astype(np.int32), 3)
    dump("upload")
    flow = np.array([st[2][1] for st in streams], dtype=np.float64)
    sp = slam.stream_params(S, Tcw=np.eye(4), cam=cam, dist=(-0.01, 0.001, 1e-4, -1e-4), shift_yx=flow)
    ks.detect(e, l0); dump("detect")
    ks.keyframe(); dump("keyframe")
    ks.flow_match(l0, l1, params, sp, prior=2); dump("flow_match_shift")
    ks.stereo_match(l1, r1, params, slam.stream_params(S, cam=cam, shift_yx=np.tile([0.0, -6.3], (S, 1))), prior=2); dump("stereo_match")
    T21 = np.eye(4); T21[0, 3] = -0.54
    Twc = np.eye(4); Twc[:3, 3] = [1.0, 2.0, 3.0]
    ks.triangulate(cam, cam, T21, Twc, max_error=3.0); dump("triangulate")
    st = ks.frame_stats(sp, 1, e.cell_size, (H, W)); dump("frame_stats_1", stats=st)
    st = ks.frame_stats(sp, 2, e.cell_size, (H, W)); dump("frame_stats_2", stats=st)
    Rt, status, ninl, par, cnt = ks.compute_pose_5pt(sp, min_parallax=0.5, max_repr_error=3.0, iters=32, seed=7)
    dump("compute_pose_5pt", Rt=Rt, status=status, ninl=ninl, parallax=par, counts_ret=cnt)
    poses, status, ninl, cnt = ks.compute_pose(sp, threshold=3.0, iters=32, seed=9)
    dump("compute_pose", poses=poses, status=status, ninl=ninl, counts_ret=cnt)
    flags = np.zeros((S, cap), np.uint8)
    for s in range(S):
        flags[s, ::5] = 1
    fd = torch.from_numpy(flags).cuda(); torch.cuda.synchronize()
    ks.remove(fd.data_ptr()); dump("remove")
    words = 4
    desc = torch.zeros((S, ncell * -(-params.max_nb_keypoints // ncell), words), dtype=torch.int64, device="cuda")
    info = torch.zeros((S, 2), dtype=torch.int64, device="cuda")
    ks.detect_describe(e, l1, desc.data_ptr(), info.data_ptr(), desc.shape[1], pattern=slam.brief_pattern(256, 9), window=9)
    torch.cuda.synchronize()
    dump("detect_describe", info=info.cpu().numpy(), desc=desc.cpu().numpy())
    ks.keyframe(); dump("keyframe_2")
    ks.flow_match(l1, l2, params, slam.stream_params(S, Tcw=np.eye(4), cam=cam), prior=1); dump("flow_match_pose")
    kf_cw = np.tile(np.eye(4), (S, 4, 1, 1))
    for k in range(4):
        kf_cw[:, k, 0, 3] = 0.3 * k
    ks.triangulate_temporal(sp, kf_cw, np.eye(4), np.full(S, 5, np.int32), kf_lo=np.full(S, 2, np.int32), max_error=3.0, min_parallax=2.0)
    dump("triangulate_temporal")
    r = ks.compute_pose_5pt(sp, iters=16, seed=1, fetch=False); dump("compute_pose_5pt_enqueue")
    assert r is None
    ks.close()


def main():
    if sys.argv[1] == "compare":
        a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
        diff = [k for k in sorted(set(a.files) | set(b.files)) if k not in a.files or k not in b.files or a[k].dtype != b[k].dtype or a[k].tobytes() != b[k].tobytes()]
        print(f"kpset_dump: {len(a.files)} arrays, {len(diff)} differing" + "".join("\n  " + k for k in diff[:40]))
        sys.exit(1 if diff else 0)
    sys.path.insert(0, ROOT)
    import slam_jl_amd as slam
    from slam_jl_amd import synthetic as syn
    slam.default_context(0)
    out = {}
    for S in (3, 70):
        sequence(slam, syn, S, out)
    np.savez(sys.argv[2], **out)
    print(f"kpset_dump: {len(out)} arrays -> {sys.argv[2]} ({os.environ.get('SLAMHIP_LIB', 'the package library')})")


if __name__ == "__main__":
    main()
