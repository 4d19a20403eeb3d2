"""GPU: every field of a keypoint's record travels with it through both modes of the lists' compaction (k_kpset_compact, csrc/kpset.hip),
across the edges of its 256-slot chunks.  S = 3 streams, cap = 600, 120 x 160 images; list lengths 255 / 256 / 257 and 513 / 257 / 0.

Every downloadable field is filled with values that differ from slot to slot and from field to field: upload (yx, is_3d mixed, xyz, ids
not starting at 0), upload_keyframe (kyx, has_kf mixed), upload_first (first_yx, first_kf, a key-frame counter per stream), and a
stereo_match of the batch against itself sets stereo_yx / has_stereo.  The three downloads are the snapshot, keyed by id.

The scene (texture seeds 50 + stream; positions from a fixed seed: three in five inside the image, two in five within a pixel of its
border, where most tracks fail; stream 2's prior shift is 40 px off, so the rightmost of its 3-D keypoints are skipped) was picked with the
CPU oracle (oracle/orc_lk.c through oracle.py: pyr_build + optical_flow_matching, window 9, 3 levels) so that the conditions the tests
assert hold.  The oracle's counts per stream, of the list length:
    lengths 255 / 256 / 257:  is_3d 125 / 136 / 133, has_kf 157 / 144 / 153, has_stereo 185 / 212 / 212;
                              mode 0 keeps (tracked or skipped) 182 / 206 / 194, per 256-slot chunk [182] / [206] / [193, 1]
    lengths 513 / 257 / 0:    is_3d 260 / 131 / -, has_kf 332 / 158 / -, has_stereo 407 / 215 / -;
                              mode 0 keeps 413 / 209 / -, per chunk [216, 197, 0] / [208, 1]
(a chunk of one slot cannot both lose and keep a keypoint: the chunk condition is asserted for the chunks of two slots or more)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S, CAP, H, W = 3, 600, 120, 160
CASES = {"255-256-257": ((255, 256, 257), 1), "513-257-0": ((513, 257, 0), 2)}          # list lengths, seed of the lists


def lists(lengths, seed):
    """per stream: dict of the uploadable fields, every value its own"""
    out = []
    for s, n in enumerate(lengths):
        r = np.random.default_rng(1000 * seed + s)
        yx = np.stack([r.uniform(8, H - 7, n), r.uniform(8, W - 7, n)], axis=1)
        edge = np.flatnonzero(r.random(n) < 0.4)
        side = r.integers(0, 4, len(edge))
        yx[edge[side == 0], 0] = r.uniform(1, 2, (side == 0).sum()); yx[edge[side == 1], 0] = r.uniform(H - 1, H, (side == 1).sum())
        yx[edge[side == 2], 1] = r.uniform(1, 2, (side == 2).sum()); yx[edge[side == 3], 1] = r.uniform(W - 1, W, (side == 3).sum())
        is3 = r.random(n) < 0.5
        xyz = np.where(is3[:, None], r.normal(0, 5, (n, 3)), np.nan)
        out.append(dict(yx=yx, is_3d=is3, xyz=xyz, ids=1000 * (s + 1) + 17 + 2 * np.arange(n, dtype=np.int64),
                        kyx=np.stack([r.uniform(1, H, n), r.uniform(1, W, n)], axis=1) + 1000.0, has_kf=r.random(n) < 0.6,
                        first_yx=np.stack([r.uniform(1, H, n), r.uniform(1, W, n)], axis=1) + 2000.0,
                        first_kf=r.integers(0, 7, n).astype(np.int32), kf_count=7 + s))
    return out


def shifts(streams):
    """the prior shift of the temporal match: the true flow; stream 2's pushed 40 px to the right, so its 3-D keypoints fail the prior attempt
    and the rightmost of them are skipped (projected outside the image)"""
    sh = np.array([st[2][1] for st in streams], dtype=np.float64)
    sh[2] += (0.0, 40.0)
    return sh


@pytest.fixture(scope="module")
def images(slam, texture):
    import torch
    streams = [texture(H, W, seed=50 + s, step=(1.0 + 0.2 * s, -1.4), disparity=6.3) for s in range(S)]
    a = slam.PyramidBatch((H, W), levels=3, S=S); b = slam.PyramidBatch((H, W), levels=3, S=S)
    d0 = [torch.from_numpy(np.ascontiguousarray(st[0][0].T)).cuda() for st in streams]
    d1 = [torch.from_numpy(np.ascontiguousarray(st[0][1].T)).cuda() for st in streams]
    torch.cuda.synchronize()
    a.update_([d.data_ptr() for d in d0]); b.update_([d.data_ptr() for d in d1])
    return dict(a=a, b=b, shift=shifts(streams), keep=(d0, d1))


FIELDS = ("yx", "is_3d", "xyz", "ids", "stereo_yx", "has_stereo", "kyx", "has_kf", "first_yx", "first_kf")


def download_all(ks):
    out = []
    for s in range(S):
        d = ks.download(s)
        d["kyx"], d["has_kf"] = ks.download_keyframe(s)
        d["first_yx"], d["first_kf"], d["kf_count"] = ks.download_first(s)
        out.append(d)
    return out


def fill(slam, syn, ks, images, L):
    """the lists of L in the set, stereo observations by a match of the batch against itself; returns the snapshot"""
    for s, f in enumerate(L):
        ks.upload(s, f["yx"], f["is_3d"], f["xyz"], f["ids"])
        ks.upload_keyframe(s, f["kyx"], f["has_kf"])
        ks.upload_first(s, f["first_yx"], f["first_kf"], f["kf_count"])
    ks.stereo_match(images["a"], images["a"], slam.Params(stereo=True, max_nb_keypoints=600), slam.stream_params(S, cam=syn.KITTI_CAM))
    snap = download_all(ks)
    for s, f in enumerate(L):                                    # nothing left the lists, the uploaded fields are as uploaded
        for key in ("yx", "is_3d", "xyz", "ids", "kyx", "has_kf", "first_yx", "first_kf"):
            assert np.array_equal(snap[s][key], f[key], equal_nan=True), (s, key)
        assert snap[s]["kf_count"] == f["kf_count"]
    return snap


def check_survivors(ks, snap, keep, moved=None):
    """stream by stream: the lists hold exactly the snapshot's rows flagged in keep[s], in order, every field (positions from `moved`
    where given); counts() agrees and the key-frame counters are unchanged"""
    got = download_all(ks)
    assert list(ks.counts()) == [int(k.sum()) for k in keep]
    for s in range(S):
        idx = np.flatnonzero(keep[s])
        assert np.array_equal(got[s]["ids"], snap[s]["ids"][idx]), s
        for key in FIELDS:
            want = snap[s][key][idx] if not (key == "yx" and moved is not None) else moved[s][idx]
            assert got[s][key].dtype == snap[s][key].dtype and np.array_equal(got[s][key], want, equal_nan=key == "xyz"), (s, key)
        assert got[s]["kf_count"] == snap[s]["kf_count"]


def chunks(n):
    return [(c0, min(c0 + 256, n)) for c0 in range(0, n, 256)]


def both_sides(flag, what):
    assert len(flag) == 0 or (flag.sum() >= 0.1 * len(flag) and (~flag).sum() >= 0.1 * len(flag)), (what, int(flag.sum()), len(flag))


@pytest.mark.parametrize("case", list(CASES))
def test_mode_1_removal_by_flags(slam, syn, images, case):
    import torch
    lengths, seed = CASES[case]
    L = lists(lengths, seed)
    ks = slam.KeypointSet(S, CAP)
    rng = np.random.default_rng(11)
    quarter = []
    for n in lengths:                                            # between a quarter and three quarters of every chunk, from a fixed seed
        f = np.zeros(n, bool)
        for c0, c1 in chunks(n):
            m = int(round((c1 - c0) * rng.uniform(0.3, 0.7)))
            f[c0 + rng.choice(c1 - c0, m, replace=False)] = True
            assert c1 - c0 < 4 or 0.25 <= f[c0:c1].mean() <= 0.75
        quarter.append(f)
    at = lambda slots: [np.isin(np.arange(n), slots) for n in lengths]
    patterns = {"quarter to three quarters": quarter, "last slot of a chunk": at([255, 511]), "first slot of the next": at([256, 512]),
                "everything": [np.ones(n, bool) for n in lengths]}
    assert any(f.any() for f in patterns["last slot of a chunk"]) and any(f.any() for f in patterns["first slot of the next"])
    for name, flags in patterns.items():
        snap = fill(slam, syn, ks, images, L)
        for s in range(S):
            both_sides(snap[s]["has_stereo"], (s, "has_stereo")); both_sides(snap[s]["is_3d"], (s, "is_3d")); both_sides(snap[s]["has_kf"], (s, "has_kf"))
        dev = np.zeros((S, CAP), np.uint8)
        for s, f in enumerate(flags):
            dev[s, :len(f)] = f
        dev[:, max(lengths):] = 1                                # (slots past the lists: never read)
        t = torch.from_numpy(dev).cuda(); torch.cuda.synchronize()
        ks.remove(t.data_ptr())
        check_survivors(ks, snap, [~f for f in flags])
    ks.close()


@pytest.mark.parametrize("case", list(CASES))
def test_mode_0_after_a_match(slam, syn, images, case):
    lengths, seed = CASES[case]
    L = lists(lengths, seed)
    ks = slam.KeypointSet(S, CAP)
    snap = fill(slam, syn, ks, images, L)
    for s in range(S):                                           # the scene's own conditions, so that this test cannot pass vacuously on its own
        both_sides(snap[s]["has_stereo"], (s, "has_stereo")); both_sides(snap[s]["is_3d"], (s, "is_3d")); both_sides(snap[s]["has_kf"], (s, "has_kf"))
    a, b, shift = images["a"], images["b"], images["shift"]
    params = slam.Params(stereo=True, max_nb_keypoints=600)
    P = np.concatenate([f["yx"] for f in L]); T = np.concatenate([f["is_3d"] for f in L])
    I = np.concatenate([np.full(n, s, np.int32) for s, n in enumerate(lengths)])
    proj = P + shift[I]
    skip = T & ~((proj[:, 0] >= 1) & (proj[:, 0] <= H) & (proj[:, 1] >= 1) & (proj[:, 1] <= W))
    ns = np.flatnonzero(~skip)
    hk, h3, hs, hsrc = slam.optical_flow_matching_batch_kept(a, b, I[~skip], P[~skip], T[~skip], proj[~skip], params)
    keep_all = skip.copy(); keep_all[ns[hsrc]] = True            # kept indices: tracked or skipped
    moved_all = P.copy(); moved_all[ns[hsrc]] = hk
    ks.flow_match(a, b, params, slam.stream_params(S, cam=syn.KITTI_CAM, shift_yx=shift), prior=2)
    off = np.concatenate([[0], np.cumsum(lengths)])
    keep = [keep_all[off[s]:off[s + 1]] for s in range(S)]; moved = [moved_all[off[s]:off[s + 1]] for s in range(S)]
    print(case, "kept", [int(k.sum()) for k in keep], "per chunk", [[int(k[c0:c1].sum()) for c0, c1 in chunks(len(k))] for k in keep], "skipped", int(skip.sum()))
    for s in range(S):                                           # the step removes and keeps something in every chunk (of two slots or more)
        for c0, c1 in chunks(lengths[s]):
            assert c1 - c0 < 2 or 0 < keep[s][c0:c1].sum() < c1 - c0, (s, c0)
    assert (keep_all & ~skip).any() and skip.any()
    check_survivors(ks, snap, keep, moved)
    ks.close()
