"""GPU: the descriptor rows of the key-frame map (slam_kfmap_enable_descriptor_rows: a point keeps one row per key-frame, csrc/kfmap.hpp) against the
model (tests/np_kfmap_rows.py) on the sequences of tests/kfmap_rows_scripts.py: S = 3, cap 64, R = 4, mcap = 128, eight key-frames, both list modes of
tests/kfmap_merge_scripts.py, D = 2 and D = 4 -- add_keyframe + add_descriptors -> local_map_match -> merge at every key-frame, the hand-picked
merge, gather + update behind key-frames 3 and 4, then a filter that removes every covisible key-frame it may (a point whose only observers are two
removed key-frames is decided between concurrent slabs) and once more match and merge.

After EVERY step descriptor_rows of every stream, every key-frame of the ring, download_points and the live lists are array_equal to the model; after
every match the status, pairs, distances and the staged lists (debug_local_map) are.  Hamming distances are integers: no tolerance anywhere.  (A
key-frame's angles are computed on the device in its own arithmetic; add() -- tests/kfmap_device.py's -- holds them to 1e-12 once and hands
the device's bits to the model.)  tests/test_kfmap_rows_host.py holds the model to the reference and shows what the scenes hold.

A hand-built stream at cap 300 (R = 4, mcap = 1024, D = 3) puts more than 256 points into the local map and more than 256 described keypoints into
the newest slab, with 0, 1, 2 and D rows on both sides of record 256 of both lists: the scans of the row counts cross a chunk edge."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_device as kd  # noqa: E402
import kfmap_lmm_scripts as ls  # noqa: E402
import kfmap_merge_scripts as ms  # noqa: E402
import kfmap_rows_scripts as rs  # noqa: E402
import kfmap_scripts as scr  # noqa: E402
import np_kfmap as npk  # noqa: E402
import np_kfmap_rows as nr  # noqa: E402
from kfmap_device import check_map, check_staged, upload_descriptors  # noqa: E402

pytestmark = pytest.mark.gpu
S = ls.S
EMPTY = np.zeros((0, 2), dtype=np.int64)


class Dev(kd.DeviceSide, rs.RowsRun):
    """the device map with its keypoint set beside the models, driven by the same scripted key-frames and descriptors; max_rows = None: a map that
    never enables the rows, beside the one-row models"""

    def __init__(self, slam, mode, max_rows, **kw):
        super().__init__(slam, mode, max_rows, descriptor_rows=max_rows, **kw)

    def filter(self, ratio, minc, first_kfid=0):
        logs = super().filter(ratio, minc, first_kfid)
        removed = self.km.filter(ratio, np.array(minc, dtype=np.int32), first_kfid=first_kfid)
        assert [sorted(k for k, ex, _, _ in log if ex in ("few", "ratio")) for log in logs] == removed
        return logs


dev = kd.device_fixture(Dev, "dev")


def _sequence(p):
    """the scripted sequence with the device beside the model, everything compared after every step; the sequence's merges take the pairs where the
    match left them on the device, the hand-picked ones are host pairs -> what the run met"""
    seen = dict(applied=0, hand=[], removed=0, orphaned=0, rows=set())
    for k in range(ls.N_KF):
        p.add(ls.LAST_MASK if k == ls.N_KF - 1 else None); p.check()
        res = p.match()
        p.merge([r["pairs"] if r["status"] == 0 else EMPTY for r in res], device_pairs=True); p.check()
        seen["applied"] += int(p.dev_counts[:, 0].sum())
        if k == ms.HAND_AT:
            hp, kinds = p.hand()
            p.merge(hp); p.check()
            seen["hand"] += [k2 for ks_ in kinds for k2 in ks_]
        if k in ls.BA_AT:
            p.ba(); p.check()
        if p.max_rows is not None:
            seen["rows"] |= {len(ks_) for s in range(S) for ks_ in p.rows(s)["keys"]}
    before = [copy.deepcopy(m) for m in p.m]                     # (for the count of points the filter leaves without an observer)
    logs = p.filter(0.5, [1000] * S); p.check()
    for s, log in enumerate(logs):
        gone = [kf for kf, ex, _, _ in log if ex in ("few", "ratio")]
        seen["removed"] += len(gone); seen["orphaned"] += len(rs.orphaned_by_filter(before[s], gone))
    res = p.match()
    p.merge([r["pairs"] if r["status"] == 0 else EMPTY for r in res], device_pairs=True); p.check()
    return seen


@pytest.mark.parametrize("max_rows", (2, 4))
@pytest.mark.parametrize("mode", ms.MODES)
def test_device_equals_model_after_every_step(dev, mode, max_rows):
    p = dev(mode, max_rows)
    seen = _sequence(p)
    assert seen["applied"] >= 9 and {"has_new", "tombstone"} <= set(seen["hand"])
    assert seen["removed"] >= 3 and seen["orphaned"] >= 1          # the last-observer clear was decided between concurrent slabs
    assert {0, 1, 2} <= seen["rows"] and (max_rows == 2 or 3 in seen["rows"])
    dropped = [p.km.descriptor_rows(s)["dropped"] for s in range(S)]
    assert (sum(dropped) > 0) == (max_rows == 2)                   # (tests/test_kfmap_rows_host.py: the bound acts at D = 2, never at D = 4)
    # reset: the stream's rows and its counter go, the other streams keep theirs
    p.km.reset(1)
    got = p.km.descriptor_rows(1)
    assert len(got["ids"]) == 0 and got["dropped"] == 0
    assert nr.same_rows(p.km.descriptor_rows(0), p.rows(0)) and nr.same_rows(p.km.descriptor_rows(2), p.rows(2))


@pytest.mark.parametrize("mode", ms.MODES)
def test_a_map_without_rows_is_the_map_it_was(dev, slam, mode):
    p = dev(mode, None)
    with pytest.raises(slam.SlamHipError, match="descriptor rows are not enabled"):
        p.km.descriptor_rows(0)
    seen = _sequence(p)                                          # the one-row models, on the same script
    assert seen["applied"] >= 9
    with pytest.raises(slam.SlamHipError, match="descriptor rows are not enabled"):
        p.km.descriptor_rows(0)


def test_enable_and_download_arguments(dev, slam):
    import ctypes as C
    from slam_jl_amd import _lib as L
    km = slam.KeyframeMap(S, ls.CAP, R=ls.R, mcap=ls.MCAP)
    try:
        with pytest.raises(slam.SlamHipError, match="descriptors are not enabled"):
            km.enable_descriptor_rows(4)
        km.enable_descriptors()
        for bad in (1, 9, 0, -3):
            with pytest.raises(slam.SlamHipError, match="max_rows"):
                km.enable_descriptor_rows(bad)
        km.enable_descriptor_rows(4)
        km.enable_descriptor_rows(4)                             # the same D: a no-op
        with pytest.raises(slam.SlamHipError, match="keeps 4 rows"):
            km.enable_descriptor_rows(3)
        with pytest.raises(slam.SlamHipError):
            km.descriptor_rows(S)                                # no such stream
        got = km.descriptor_rows(0)
        assert len(got["ids"]) == 0 and got["dropped"] == 0
    finally:
        km.close()
    # the capacities, on a map that holds points
    p = dev("follow", 4)
    for _ in range(3):
        p.add(); p.merge([r["pairs"] if r["status"] == 0 else EMPTY for r in p.match()], device_pairs=True)
    want = p.rows(0)
    n_pts, n_rows = len(want["ids"]), sum(len(k) for k in want["keys"])
    assert n_pts >= 2 and n_rows >= 2
    c, n = p.km.ctx, C.c_int32(0)
    ids = np.zeros(n_pts, dtype=np.int64); keys = np.zeros(n_rows, dtype=np.int32); off = np.zeros(n_pts + 1, dtype=np.int32)
    call = lambda cp, cr, k: c.lib.slam_kfmap_download_descriptor_rows(c.h, p.km.h, 0, L.ptr(ids, L.i64p), None, L.ptr(off, L.i32p), k, None, cp, cr, C.byref(n), None)
    assert call(n_pts - 1, n_rows, L.ptr(keys, L.i32p)) != 0 and n.value == n_pts and b"caps" in c.lib.slam_last_error(c.h)
    assert call(n_pts, n_rows - 1, L.ptr(keys, L.i32p)) != 0 and n.value == n_pts
    assert call(n_pts, 0, None) == 0 and np.array_equal(ids, want["ids"]) and off[n_pts] == n_rows      # without keys and rows the row capacity is not needed
    assert call(n_pts, n_rows, L.ptr(keys, L.i32p)) == 0 and np.array_equal(keys, np.concatenate(want["keys"]))


def test_status_2_with_rows(dev):
    p = dev("stale", 4)
    for k in range(4):
        p.add()
        res = p.match()
        p.merge([r["pairs"] if r["status"] == 0 else EMPTY for r in res], device_pairs=True)
    p.check()
    sizes = [len(r["lm_ids"]) for r in p.match()]                # (the local maps as the merges left them)
    assert max(sizes) >= 2
    res = p.match(max_local=max(sizes) - 1)                      # the largest local map no longer fits: status 2, nothing staged or paired for it
    assert 2 in [r["status"] for r in res]
    p.check()                                                    # the match changes nothing in the map


# ---- the hand-built stream at cap 300: the row-offset scans cross a chunk edge ------------------------------------------------------------------------------
HCAP, HR, HMCAP, HD, HDCAP = 300, 4, 1024, 3, 512
L0A, L1, L0B = range(100, 230), range(230, 370), range(370, 380)          # the local map: born at key-frame 0 / 1 / 0, seen up to key-frame 3
K0, K3, K4, LINK = (10, 11, 990, 991), (420, 421, 980, 981), range(500, 772), range(400, 410)
H_LISTS = [sorted([*L0A, *L0B, *K0]), sorted([*L0A, *L1, *L0B, *K0, 810, 811]), sorted([*L0A, *L1, *L0B, *range(800, 804), *range(820, 824)]),
           sorted([*L0A, *L1, *L0B, *LINK, *K3, 830, 831]), sorted([*K4, *K0, *K3, *LINK])]
H_RUNS = [[(10, 2), (100, 130), (370, 10), (990, 2)], [(230, 140), (810, 2)], [(800, 4), (820, 4)], [(400, 10), (420, 2), (830, 2), (980, 2)], [(500, 272)]]
# (prev, new): the donors 8xx, born at key-frames 1, 2 and 3 and seen by no other, hand their rows to keypoints of the newest key-frame (420, 421, 980,
# 981) and to local-map points (231, 232, 360, 361); a new id occurs once per call, hence two calls
H_MERGES = [[(800, 420), (801, 421), (802, 980), (803, 981), (820, 231), (821, 360), (822, 232), (823, 361)], [(810, 421), (811, 981), (830, 232), (831, 361)]]


def test_row_offsets_cross_a_chunk_edge(slam):
    import torch
    seed = 51
    m = npk.Map(HCAP, HR, HMCAP, ls.CAM10[:4], None, 4)
    D = nr.new_descriptors(m, HD)
    ks, km = slam.KeypointSet(1, HCAP), slam.KeyframeMap(1, HCAP, R=HR, mcap=HMCAP)
    try:
        km.enable_descriptors(); km.enable_descriptor_rows(HD)
        for k, ids in enumerate(H_LISTS):
            assert len(ids) <= HCAP
            T = np.eye(4); T[0, 3] = 0.01 * k
            yx = np.array([[1.5 + (ls.H - 2.0) * scr._u(seed, 1, i, k), 1.5 + (ls.W - 2.0) * scr._u(seed, 2, i, k)] for i in ids])
            xyz = np.array([[2.0 * scr._u(seed, 3, i) - 1.0, 1.4 * scr._u(seed, 4, i) - 0.7, 2.0 + scr._u(seed, 5, i)] for i in ids])
            f = dict(Tcw=T, ids=np.array(ids, dtype=np.int64), yx=yx, is_3d=np.ones(len(ids), dtype=bool), xyz=xyz)
            nr.add_keyframe(m, D, k, T, f)
            ks.upload(0, f["yx"], f["is_3d"], f["xyz"], f["ids"])
            ks.keyframe()
            km.add_keyframe(ks, slam.stream_params(1, Tcw=T[None], cam=ls.CAM10[:4], dist=np.zeros((1, 4))))
            for first, n in H_RUNS[k]:
                rows = np.array([ls.random_row(seed, i) for i in range(first, first + n)], dtype=np.uint64)
                nr.add_descriptors(m, D, first, rows)
                upload_descriptors(torch, km, 1, HDCAP, {0: (first, rows)})
            kd.hand_over_theta(km, m, 0, k)
        for pairs in H_MERGES:                                   # the rows come from host-pair merges (a new id once per call: two calls)
            want = nr.merge(m, D, np.array(pairs, dtype=np.int64), None, with_list=False)
            got = km.merge(None, [np.array(pairs, dtype=np.int64)])
            assert want["applied"] == len(pairs) and tuple(got[0]) == (want["applied"], want["skipped"], want["renamed"], want["status"])
        assert nr.same_rows(km.descriptor_rows(0), nr.descriptor_rows(m, D))
        want = nr.local_map_match(m, D, ls.CAM10, ls.CELL, ls.PARAMS)
        assert want["status"] == 0 and len(want["lm_ids"]) > 256 and len(want["kp_ids"]) > 256
        for counts in (want["lm_rows"], want["kp_rows"]):        # 0, 1, 2 and D rows on both sides of record 256 of both lists
            assert {0, 1, 2, HD} <= set(int(c) for c in counts[:256]) and {0, 1, 2, HD} <= set(int(c) for c in counts[256:])
        status, pairs, dist = km.local_map_match(ls.CAM10, ls.CELL, ls.PARAMS.max_projection_distance, ls.PARAMS.max_descriptor_distance, max_local=HMCAP)
        assert status[0] == 0 and np.array_equal(pairs[0], want["pairs"]) and np.array_equal(dist[0], want["dist"])
        check_staged(km, [want], [0])
        check_map(km, None, [m])
    finally:
        km.close(); ks.close()
