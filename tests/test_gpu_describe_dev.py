"""GPU: describe() on device-resident pyramids -- slam_describe_pyr, slam_describe_batch, slam_kpset_detect_describe (csrc/brief.hip
k_brief_patch; extractor.jl:103-105 as map_manager.jl:105-113 calls it) -- against the CPU oracle and the host-image slam_describe.
Everything is compared with array_equal: the smoothed neighbourhood is formed with the arithmetic of the two full-frame passes."""
import numpy as np
import pytest

import describe_cases as dc

pytestmark = pytest.mark.gpu


def _pyramid(slam, img, levels=2):
    pyr = slam.LKPyramid(shape=img.shape, levels=levels)
    slam.update_(pyr, img)
    return pyr


def _u8_batch(slam, u8s, levels, **kw):
    """PyramidBatch of the given 8-bit frames (column-major bytes in HBM)"""
    import torch
    H, W = u8s[0].shape
    dev = torch.from_numpy(np.stack([np.ascontiguousarray(u.T) for u in u8s])).cuda()
    torch.cuda.synchronize()
    b = slam.PyramidBatch((H, W), levels=levels, S=len(u8s))
    b.update_([dev.data_ptr() + s * H * W for s in range(len(u8s))], u8=True, **kw)
    return b, dev


# ---- 1. pyramid form, single image ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ingest", ["f64", "u8"])
@pytest.mark.parametrize("shape", dc.SINGLE_SHAPES)
def test_describe_pyr_equals_oracle_and_host_image_form(slam, orc, syn, shape, ingest):
    H, W = shape
    f64, u8 = dc.frames(syn, H, W, seed=0)[0][0]
    img = f64 if ingest == "f64" else dc.as_f64(u8)
    pyr = _pyramid(slam, f64 if ingest == "f64" else u8)
    assert np.array_equal(pyr.plane("layers", 0), img)              # the resident layer 0 IS the oracle's image (u8: raw / 255), bit for bit
    e = slam.Extractor(150, 17, (-(-H // 35), -(-W // 35)), 35)
    det = orc.detect(img, np.zeros((0, 2)), max_points=150)
    for window in dc.WINDOWS:
        kept, dropped = dc.hand_placed(H, W, window)
        kp = np.concatenate([det, kept, dropped])
        for n_bits in (64, 256, 512):
            for pat in (slam.brief_pattern(n_bits, window), dc.edge_pattern(n_bits, window)):
                where = (shape, ingest, window, n_bits)
                bits, rc = slam.describe(e, pyr, kp, pattern=pat, window=window)
                rbits, rrc = orc.describe(img, kp, pat, window=window)
                hbits, hrc = slam.describe(e, img, kp, pattern=pat, window=window)
                assert bits.shape == (len(rrc), n_bits // 64), where
                assert np.array_equal(rc, rrc) and np.array_equal(bits, rbits), where
                assert np.array_equal(rc, hrc) and np.array_equal(bits, hbits), where
                got = {tuple(p) for p in rc}
                assert all(tuple(p) in got for p in kept) and not any(tuple(p) in got for p in dropped), where
                assert len(rc) < len(det) + len(kept), where       # detected keypoints were dropped too


def test_describe_pyr_errors_and_empty_lists(slam, syn):
    H, W = 93, 131
    pyr = _pyramid(slam, dc.frames(syn, H, W, seed=0)[0][0][1])
    e = slam.Extractor(150, 17, (3, 4), 35)
    kp = np.array([[40, 50], [20, 100]])
    with pytest.raises(slam.SlamHipError, match="15"):              # the limit is named
        slam.describe(e, pyr, kp, pattern=slam.brief_pattern(64, 17), window=17)
    bad = slam.brief_pattern(64, 9); bad[10, 2] = 6                  # lim + 1
    with pytest.raises(slam.SlamHipError, match="pattern offset"):
        slam.describe(e, pyr, kp, pattern=bad, window=9)
    bits, rc = slam.describe(e, pyr, np.zeros((0, 2)), window=9)
    assert bits.shape == (0, 4) and rc.shape == (0, 2)
    bits, rc = slam.describe(e, pyr, np.array([[1, 1], [5, 60], [H, W], [50, W - 4]]), window=9)
    assert bits.shape == (0, 4) and rc.shape == (0, 2)             # every keypoint dropped
    bits, rc = slam.describe(e, pyr, kp, window=9)                  # the pyramid still describes after the refused calls
    assert len(rc) == 2


# ---- 2. batch form ----------------------------------------------------------------------------------------------------------------
def _batch_lists(orc, imgs, window):
    """ragged lists: detected keypoints + border ones, stream 2 empty"""
    H, W = imgs[0].shape
    _, dropped = dc.hand_placed(H, W, window)
    kps = [np.zeros((0, 2), np.int64) if s == 2 else
           np.concatenate([orc.detect(im, np.zeros((0, 2)), max_points=40 + 25 * s), dropped[s % 3:]]) for s, im in enumerate(imgs)]
    return kps, np.concatenate([np.full(len(k), s, np.int32) for s, k in enumerate(kps)])


def _check_batch(slam, orc, batch, imgs, kps, sid, pat, window, tag):
    bits, rc, osid = slam.describe_batch(None, batch, np.concatenate(kps), sid, pattern=pat, window=window)
    for s, im in enumerate(imgs):
        rbits, rrc = orc.describe(im, kps[s], pat, window=window)
        m = osid == s
        assert np.array_equal(rc[m], rrc) and np.array_equal(bits[m], rbits), (tag, s)
        assert len(rrc) < len(kps[s]) or len(kps[s]) == 0, (tag, s)
    assert (osid == 2).sum() == 0 and len(osid) > 0


def test_describe_batch_mode1_and_target_only(slam, orc, syn):
    S, (H, W), window = 5, (93, 131), 9
    u8s = [dc.frames(syn, H, W, seed=40 + s)[0][0][1] for s in range(S)]
    imgs = [dc.as_f64(u) for u in u8s]
    kps, sid = _batch_lists(orc, imgs, window)
    pat = slam.brief_pattern(256, window)
    b, keep = _u8_batch(slam, u8s, 2)
    _check_batch(slam, orc, b, imgs, kps, sid, pat, window, "mode 1")
    t, keep_t = _u8_batch(slam, u8s, 2, target_only=True)           # SLAM_PYR_TARGET_ONLY: level 0 is complete there as well
    _check_batch(slam, orc, t, imgs, kps, sid, dc.edge_pattern(256, window), window, "target only")


def test_describe_batch_tolerance_mode(slam, orc, syn, monkeypatch):
    """mode 3 (tolerance build, its kernels forced at this size): the oracle describes each member's DOWNLOADED layer 0.
    On the MI355X run that layer equalled u8 / 255 bit for bit for every member (the ingest does not depend on the mode); the test asserts it."""
    monkeypatch.setenv("SLAMHIP_CK_MIN_MB", "0")
    S, (H, W), window = 5, (120, 160), 9
    u8s = [dc.frames(syn, H, W, seed=50 + s)[0][0][1] for s in range(S)]
    b, keep = _u8_batch(slam, u8s, 2, fast=True)
    layers = [b.pyramids[s].plane("layers", 0) for s in range(S)]
    same = [bool(np.array_equal(layers[s], dc.as_f64(u8s[s]))) for s in range(S)]
    print("mode 3: layer 0 == u8 / 255 per member:", same)
    kps, sid = _batch_lists(orc, layers, window)
    _check_batch(slam, orc, b, layers, kps, sid, slam.brief_pattern(256, window), window, "mode 3")
    assert all(same)


# ---- 3. / 4. set form -------------------------------------------------------------------------------------------------------------
class _HostLists:
    """the host protocol of map_manager.jl:98-113 on the oracle: detect with the stream's list as avoidance list, describe, append the
    survivors with consecutive ids"""

    def __init__(self, S):
        self.yx = [np.zeros((0, 2)) for _ in range(S)]
        self.ids = [np.zeros(0, np.int64) for _ in range(S)]
        self.next_id = [0] * S

    def keyframe(self, orc, s, img, max_points, grid, pat, window):
        cand = orc.detect(img, self.yx[s], max_points=max_points, grid=grid) if len(self.yx[s]) < max_points else np.zeros((0, 2), np.int64)
        bits, kept = orc.describe(img, cand, pat, window=window)
        first = self.next_id[s]
        self.yx[s] = np.concatenate([self.yx[s], kept.astype(float)])
        self.ids[s] = np.concatenate([self.ids[s], first + np.arange(len(kept))])
        self.next_id[s] = first + len(kept)
        return first, bits, len(cand)


def _dev_buffers(S, dcap, words):
    import torch
    desc = torch.zeros((S, dcap, words), dtype=torch.int64, device="cuda")
    info = torch.full((S, 2), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return desc, info


def _check_keyframe(ks, host, desc, info, expect, tag):
    """expect[s] = (first id, oracle bits) of this key-frame"""
    import torch
    cnt = ks.counts()
    torch.cuda.synchronize()
    d = desc.cpu().numpy().view(np.uint64); inf = info.cpu().numpy()
    for s, (first, bits) in enumerate(expect):
        got = ks.download(s)
        assert cnt[s] == len(host.yx[s]) == len(got["yx"]), (tag, s)
        assert np.array_equal(got["yx"], host.yx[s]) and np.array_equal(got["ids"], host.ids[s]), (tag, s)
        assert tuple(inf[s]) == (first, len(bits)), (tag, s, inf[s])
        assert np.array_equal(d[s, :len(bits)], bits), (tag, s)
        assert not got["is_3d"][len(got["yx"]) - len(bits):].any(), (tag, s)


def test_kpset_detect_describe_two_keyframes(slam, orc, syn):
    S, (H, W), mp, grid, cell, window = dc.SET_S, dc.SET_SHAPE, dc.SET_MAX_POINTS, dc.SET_GRID, dc.SET_CELL, 9
    streams = [dc.set_stream(syn, s) for s in range(S)]
    u8 = lambda k: [streams[s][0][k][1] for s in range(S)]
    img = lambda k: [dc.as_f64(u) for u in u8(k)]
    a, keep_a = _u8_batch(slam, u8(0), 3)
    b, keep_b = _u8_batch(slam, u8(1), 3)
    e = slam.Extractor(mp, 17, grid, cell)
    ncell = grid[0] * grid[1]
    dcap = ncell * -(-mp // ncell)
    pat = slam.brief_pattern(256, window)
    words = 4
    ks = slam.KeypointSet(S, mp + ncell + 8)
    old = slam.KeypointSet(S, mp + ncell + 8)                       # the old entry on identical (empty) lists
    host = _HostLists(S)
    desc, info = _dev_buffers(S, dcap, words)
    with pytest.raises(slam.SlamHipError, match="dcap"):
        ks.detect_describe(e, a, desc.data_ptr(), info.data_ptr(), dcap - 1, pattern=pat, window=window)
    assert not ks.counts().any()                                    # the refused call left the lists alone
    # ---- first key-frame, empty lists ----
    ks.detect_describe(e, a, desc.data_ptr(), info.data_ptr(), dcap, pattern=pat, window=window)
    expect = []
    for s in range(S):
        first, bits, ncand = host.keyframe(orc, s, img(0)[s], mp, grid, pat, window)
        assert 0 < len(bits) < ncand, s                             # the oracle dropped a candidate: the case is not slam_kpset_detect's
        expect.append((first, bits))
    _check_keyframe(ks, host, desc, info, expect, "key-frame 1")
    old.detect(e, a)
    for s in range(S):
        full = orc.detect(img(0)[s], np.zeros((0, 2)), max_points=mp, grid=grid)
        assert np.array_equal(old.download(s)["yx"], full.astype(float)) and len(full) > len(expect[s][1]), s
    ks.keyframe()
    # ---- track to the next frame (lost keypoints leave the lists), second key-frame ----
    params = slam.Params(stereo=True, max_nb_keypoints=mp)
    shift = np.array([streams[s][1][1] for s in range(S)])
    ks.flow_match(a, b, params, slam.stream_params(S, cam=syn.KITTI_CAM, shift_yx=shift), prior=2)
    # map culling on top (flags in HBM), so that the second key-frame has room: ids in the lists are no longer consecutive
    import torch
    cnt = ks.counts()
    rng = np.random.default_rng(5)
    flags = np.zeros((S, ks.cap), np.uint8)
    for s in range(S):
        flags[s, :cnt[s]] = rng.random(cnt[s]) < 0.4
    fdev = torch.from_numpy(flags).cuda(); torch.cuda.synchronize()
    ks.remove(fdev.data_ptr())
    for s in range(S):                                              # (tracking and removal are test_gpu_kpset's subject: the host takes their result)
        got = ks.download(s)
        assert 0 < len(got["yx"]) < len(host.yx[s]) and np.array_equal(got["ids"], np.sort(got["ids"])), s
        host.yx[s], host.ids[s] = got["yx"], got["ids"]
    ks.keyframe()
    desc2, info2 = _dev_buffers(S, dcap, words)
    ks.detect_describe(e, b, desc2.data_ptr(), info2.data_ptr(), dcap, pattern=pat, window=window)
    expect = []
    for s in range(S):
        first, bits, ncand = host.keyframe(orc, s, img(1)[s], mp, grid, pat, window)
        assert 0 < len(bits) < ncand, s
        expect.append((first, bits))
    _check_keyframe(ks, host, desc2, info2, expect, "key-frame 2")
    # ---- a stream at max_points gets nothing: info = (next id, 0), list untouched ----
    rng = np.random.default_rng(3)
    full_yx = np.stack([rng.uniform(10, H - 10, mp), rng.uniform(10, W - 10, mp)], 1)
    ks.upload(1, full_yx, np.zeros(mp, bool))
    host.yx[1], host.ids[1], host.next_id[1] = full_yx, np.arange(mp), mp
    desc3, info3 = _dev_buffers(S, dcap, words)
    ks.detect_describe(e, b, desc3.data_ptr(), info3.data_ptr(), dcap, pattern=pat, window=window)
    expect = []
    for s in range(S):
        first, bits, ncand = host.keyframe(orc, s, img(1)[s], mp, grid, pat, window)
        expect.append((first, bits))
    assert len(expect[1][1]) == 0 and expect[1][0] == mp
    _check_keyframe(ks, host, desc3, info3, expect, "full stream")
    assert not desc3[1].any()


def test_kpset_detect_describe_72_streams(slam, orc, syn):
    """more than 64 streams (the set once advanced only the first 64): every stream against the oracle"""
    S, (H, W), mp, grid, window = dc.WIDE_S, dc.WIDE_SHAPE, dc.WIDE_MAX_POINTS, dc.WIDE_GRID, 9
    u8s = [dc.wide_frame(syn, s) for s in range(S)]
    b, keep = _u8_batch(slam, u8s, 2)
    e = slam.Extractor(mp, 17, grid, 35)
    ncell = grid[0] * grid[1]
    dcap = ncell * -(-mp // ncell)
    pat = slam.brief_pattern(256, window)
    ks = slam.KeypointSet(S, mp + ncell + 8)
    host = _HostLists(S)
    desc, info = _dev_buffers(S, dcap, 4)
    ks.detect_describe(e, b, desc.data_ptr(), info.data_ptr(), dcap, pattern=pat, window=window)
    expect = []
    dropped = 0
    for s in range(S):
        first, bits, ncand = host.keyframe(orc, s, dc.as_f64(u8s[s]), mp, grid, pat, window)
        dropped += ncand - len(bits)
        expect.append((first, bits))
    assert dropped >= S
    _check_keyframe(ks, host, desc, info, expect, "72 streams")
