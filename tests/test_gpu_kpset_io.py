"""GPU: the six host seams of the device-resident keypoint lists (slam_kpset_upload / _upload_keyframe / _upload_first and the three
downloads, csrc/kpset.hip) at S = 2, cap = 8: round trips at n = 0, 1 and cap, null outputs and null inputs, and every refusal -- a
refused call leaves both streams' lists as they were, a download into too small arrays still reports the list length and names itself."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S, CAP = 2, 8
ERR_ARG, ERR_CAPACITY = -1, -4


def _fields(n, seed):
    """n keypoints, every field different from slot to slot and from field to field"""
    r = np.random.default_rng(seed)
    return dict(yx=r.uniform(1, 100, (n, 2)), is_3d=(np.arange(n) + seed) % 2 == 0, xyz=r.normal(0, 5, (n, 3)), ids=100 * seed + 7 + 3 * np.arange(n, dtype=np.int64),
                kyx=r.uniform(101, 200, (n, 2)), has_kf=(np.arange(n) + seed) % 3 != 0, first_yx=r.uniform(201, 300, (n, 2)),
                first_kf=(seed + np.arange(n, dtype=np.int32)) % 5, kf_count=11 + seed)


def _fill(ks, s, f):
    ks.upload(s, f["yx"], f["is_3d"], f["xyz"], f["ids"])
    ks.upload_keyframe(s, f["kyx"], f["has_kf"])
    ks.upload_first(s, f["first_yx"], f["first_kf"], f["kf_count"])


def _snapshot(ks):
    """every downloadable field of both streams, as bytes"""
    out = []
    for s in range(S):
        d = ks.download(s); k, hk = ks.download_keyframe(s); f, fk, kc = ks.download_first(s)
        out.append([d[key].tobytes() for key in ("yx", "is_3d", "xyz", "ids", "stereo_yx", "has_stereo")] + [k.tobytes(), hk.tobytes(), f.tobytes(), fk.tobytes(), kc])
    return out


@pytest.fixture()
def ks(slam):
    k = slam.KeypointSet(S, CAP)
    yield k
    k.close()


@pytest.mark.parametrize("n", [0, 1, CAP])
def test_round_trips(slam, ks, n):
    other = _fields(3, 9)
    _fill(ks, 1, other)
    f = _fields(n, 1)
    _fill(ks, 0, f)
    assert list(ks.counts()) == [n, 3]
    for s, g in ((0, f), (1, other)):
        d = ks.download(s)
        for key in ("yx", "is_3d", "xyz", "ids"):
            assert d[key].shape == np.asarray(g[key]).shape and np.array_equal(d[key], g[key]), (s, key)
        assert not d["has_stereo"].any() and d["stereo_yx"].shape == (len(g["yx"]), 2)      # upload clears the stereo observations
        k, hk = ks.download_keyframe(s)
        assert np.array_equal(k, g["kyx"]) and np.array_equal(hk, g["has_kf"])
        fy, fk, kc = ks.download_first(s)
        assert np.array_equal(fy, g["first_yx"]) and np.array_equal(fk, g["first_kf"]) and fk.dtype == np.int32 and kc == g["kf_count"]
    # upload replaces the list and clears has_kf; the first observations and the key-frame counter are not its business
    ks.upload(0, f["yx"], f["is_3d"], f["xyz"], f["ids"])
    assert not ks.download_keyframe(0)[1].any() and ks.download_first(0)[2] == f["kf_count"]


def _download_args(n):
    return [np.full((n, 2), -1.0), np.full(n, 7, np.uint8), np.full((n, 3), -1.0), np.full(n, -1, np.int64), np.full((n, 2), -1.0), np.full(n, 7, np.uint8)]


def test_null_outputs_are_skipped_and_the_others_filled(slam, ks):
    from slam_jl_amd import _lib as L
    c = ks.ctx
    f = _fields(5, 2)
    _fill(ks, 1, f)
    types = (L.f64p, L.u8p, L.f64p, L.i64p, L.f64p, L.u8p)
    full = _download_args(5)
    n = C.c_int(-1)
    assert c.lib.slam_kpset_download(c.h, ks.h, 1, *[L.ptr(a, t) for a, t in zip(full, types)], 5, C.byref(n)) == 0 and n.value == 5
    assert np.array_equal(full[0], f["yx"]) and np.array_equal(full[3], f["ids"]) and not full[5].any()
    for skip in list(range(6)) + [None]:                       # one output null at a time, then all of them
        out = _download_args(5)
        ptrs = [None if (skip is None or i == skip) else L.ptr(a, t) for i, (a, t) in enumerate(zip(out, types))]
        n = C.c_int(-1)
        assert c.lib.slam_kpset_download(c.h, ks.h, 1, *ptrs, 5, C.byref(n)) == 0 and n.value == 5
        for i in range(6):
            if skip is None or i == skip:
                assert np.array_equal(out[i], _download_args(5)[i]), (skip, i)            # untouched
            else:
                assert np.array_equal(out[i], full[i]), (skip, i)
    for skip in (0, 1, None):
        k = np.full((5, 2), -1.0); h = np.full(5, 7, np.uint8); n = C.c_int(-1)
        ptrs = [None if (skip is None or skip == 0) else L.ptr(k), None if (skip is None or skip == 1) else L.ptr(h, L.u8p)]
        assert c.lib.slam_kpset_download_keyframe(c.h, ks.h, 1, *ptrs, 5, C.byref(n)) == 0 and n.value == 5
        assert np.array_equal(k, f["kyx"]) == (ptrs[0] is not None) and (k == -1).all() == (ptrs[0] is None)
        assert np.array_equal(h, f["has_kf"].astype(np.uint8)) == (ptrs[1] is not None) and (h == 7).all() == (ptrs[1] is None)
        y = np.full((5, 2), -1.0); fk = np.full(5, -9, np.int32); n = C.c_int(-1); kc = C.c_int(-1)
        ptrs = [None if (skip is None or skip == 0) else L.ptr(y), None if (skip is None or skip == 1) else L.ptr(fk, L.i32p)]
        assert c.lib.slam_kpset_download_first(c.h, ks.h, 1, *ptrs, 5, C.byref(n), C.byref(kc) if skip != 1 else None) == 0 and n.value == 5
        assert kc.value == (f["kf_count"] if skip != 1 else -1)
        assert np.array_equal(y, f["first_yx"]) == (ptrs[0] is not None) and (y == -1).all() == (ptrs[0] is None)
        assert np.array_equal(fk, f["first_kf"]) == (ptrs[1] is not None) and (fk == -9).all() == (ptrs[1] is None)


def test_null_inputs(slam, ks):
    """ids = None numbers the list 0 .. n-1 and xyz = None stores zeros.  The stream's id counter (next_id) moves past the uploaded ids, but no
    download returns it and an upload never reads it (a second ids = None upload numbers its list from 0 again, here as at the parent): it
    is observable only through the ids a detect appends, which tests/test_gpu_describe_dev.py compares with its host lists after uploads."""
    f = _fields(4, 3)
    _fill(ks, 1, _fields(2, 8))
    before1 = _snapshot(ks)[1]
    ks.upload(0, f["yx"], f["is_3d"], f["xyz"])                  # ids = None: 0 .. n-1
    assert np.array_equal(ks.download(0)["ids"], np.arange(4)) and np.array_equal(ks.download(0)["xyz"], f["xyz"])
    g = _fields(6, 4)
    ks.upload(0, g["yx"], g["is_3d"])                            # the next upload numbers its list the same way; xyz = None: zeros
    d = ks.download(0)
    assert np.array_equal(d["ids"], np.arange(6)) and d["ids"].dtype == np.int64
    assert d["xyz"].shape == (6, 3) and not d["xyz"].any() and d["xyz"].tobytes() == bytes(6 * 24)
    assert np.array_equal(d["yx"], g["yx"]) and np.array_equal(d["is_3d"], g["is_3d"])
    assert _snapshot(ks)[1] == before1


def test_refusals_leave_the_lists_alone(slam, ks):
    from slam_jl_amd import _lib as L
    c = ks.ctx
    for s in range(S):
        _fill(ks, s, _fields(5 + s, 5 + s))
    before = _snapshot(ks)
    g = _fields(CAP + 1, 7)
    yx, f3, xyz, ids = L.ptr(g["yx"]), L.ptr(g["is_3d"].astype(np.uint8), L.u8p), L.ptr(g["xyz"]), L.ptr(g["ids"], L.i64p)
    kyx, hk = L.ptr(g["kyx"]), L.ptr(g["has_kf"].astype(np.uint8), L.u8p)
    fyx, fkf = L.ptr(g["first_yx"]), L.ptr(g["first_kf"], L.i32p)
    lib = c.lib
    calls = []
    for s, n in ((-1, 3), (S, 3), (0, CAP + 1), (1, -1)):
        calls += [lambda s=s, n=n: lib.slam_kpset_upload(c.h, ks.h, s, yx, f3, xyz, ids, n),
                  lambda s=s, n=n: lib.slam_kpset_upload_keyframe(c.h, ks.h, s, kyx, hk, n),
                  lambda s=s, n=n: lib.slam_kpset_upload_first(c.h, ks.h, s, fyx, fkf, n, 99)]
    # a null required pointer with n > 0
    calls += [lambda: lib.slam_kpset_upload(c.h, ks.h, 0, None, f3, xyz, ids, 3), lambda: lib.slam_kpset_upload(c.h, ks.h, 0, yx, None, xyz, ids, 3),
              lambda: lib.slam_kpset_upload_keyframe(c.h, ks.h, 0, None, hk, 3), lambda: lib.slam_kpset_upload_keyframe(c.h, ks.h, 0, kyx, None, 3),
              lambda: lib.slam_kpset_upload_first(c.h, ks.h, 0, None, fkf, 3, 99), lambda: lib.slam_kpset_upload_first(c.h, ks.h, 0, fyx, None, 3, 99)]
    out = _download_args(CAP)
    po = [L.ptr(a, t) for a, t in zip(out, (L.f64p, L.u8p, L.f64p, L.i64p, L.f64p, L.u8p))]
    n = C.c_int(-5)
    for s in (-1, S):
        calls += [lambda s=s: lib.slam_kpset_download(c.h, ks.h, s, *po, CAP, C.byref(n)),
                  lambda s=s: lib.slam_kpset_download_keyframe(c.h, ks.h, s, po[0], po[1], CAP, C.byref(n)),
                  lambda s=s: lib.slam_kpset_download_first(c.h, ks.h, s, po[0], L.ptr(np.zeros(CAP, np.int32), L.i32p), CAP, C.byref(n), None)]
    calls += [lambda: lib.slam_kpset_download(c.h, ks.h, 0, *po, CAP, None), lambda: lib.slam_kpset_download_keyframe(c.h, ks.h, 0, po[0], po[1], CAP, None),
              lambda: lib.slam_kpset_download_first(c.h, ks.h, 0, po[0], None, CAP, None, None)]
    for i, call in enumerate(calls):
        assert call() == ERR_ARG, i
        assert "argument check failed" in lib.slam_last_error(c.h).decode(), i
    assert n.value == -5 and all((a == b).all() for a, b in zip(out, _download_args(CAP)))
    assert _snapshot(ks) == before
    # n == 0 needs no arrays
    assert lib.slam_kpset_upload_keyframe(c.h, ks.h, 0, None, None, 0) == 0 and lib.slam_kpset_upload_first(c.h, ks.h, 0, None, None, 0, before[0][-1]) == 0
    assert _snapshot(ks) == before


def test_a_download_into_too_small_arrays_reports_the_length_and_names_itself(slam, ks):
    from slam_jl_amd import _lib as L
    c, lib = ks.ctx, ks.ctx.lib
    nk = 6
    for s in range(S):
        _fill(ks, s, _fields(nk if s == 1 else 2, s))
    before = _snapshot(ks)
    out = _download_args(CAP)
    po = [L.ptr(a, t) for a, t in zip(out, (L.f64p, L.u8p, L.f64p, L.i64p, L.f64p, L.u8p))]
    fk = np.full(CAP, -9, np.int32)
    seams = {"slam_kpset_download": lambda n, kc: lib.slam_kpset_download(c.h, ks.h, 1, *po, nk - 1, C.byref(n)),
             "slam_kpset_download_keyframe": lambda n, kc: lib.slam_kpset_download_keyframe(c.h, ks.h, 1, po[0], po[1], nk - 1, C.byref(n)),
             "slam_kpset_download_first": lambda n, kc: lib.slam_kpset_download_first(c.h, ks.h, 1, po[0], L.ptr(fk, L.i32p), nk - 1, C.byref(n), C.byref(kc))}
    for name, call in seams.items():
        n, kc = C.c_int(-1), C.c_int(-1)
        assert call(n, kc) == ERR_CAPACITY, name
        assert n.value == nk, name
        msg = lib.slam_last_error(c.h).decode()
        assert (name + ":") in msg and f"{nk} keypoints" in msg and f"cap = {nk - 1}" in msg, msg
        if name == "slam_kpset_download_first":
            assert kc.value == 11 + 1                            # the key-frame counter is reported with the length
    assert all((a == b).all() for a, b in zip(out, _download_args(CAP))) and (fk == -9).all()          # nothing was copied
    assert _snapshot(ks) == before
