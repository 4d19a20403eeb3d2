"""CPU: slam_keyframe_required (csrc/kf_host.hpp: check_new_kf_required, front_end.jl:361-393) against the numpy model of tests/np_kf.py over the
full grid of values around every threshold of the rule -- through ctypes (the exported symbol and the Python wrapper), and as a stand-alone
host program (tests/c_host/kf_decide_check.cpp) that replays the same table, built plain and with -fsanitize=address,undefined (the program
alone; nothing loaded into Python runs under a sanitizer)."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_kf  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "kf_decide_check.cpp")
INC = os.path.join(ROOT, "slam.jl_amd", "csrc")

CELLS = (329, 330, 331, 499, 500)
NB_3D = (0, 19, 20, 500, 501)
FRAMES_D = (0, 1, 2, 4, 5)
LOCAL_BA = (0, 1)
PREV_3D = (0, 24, 27, 1000)
MEDIAN = (9.99, 10.0, 19.99, 20.0, float("nan"))
HAS_PREV = (0, 1)
MAX_KP, INITIAL_PARALLAX = 1000, 20.0


def _grid():
    """rows (cells, nb_3d, frames_delta, local_ba_on, prev_kf_nb_3d, median, has_prev_kf) + the model's (required, rule)"""
    rows = list(itertools.product(CELLS, NB_3D, FRAMES_D, LOCAL_BA, PREV_3D, MEDIAN, HAS_PREV))
    want = []
    for cells, n3, fd, ba, p3, med, has in rows:
        st = np.array([1000, n3, 0, 900, cells, 900, med, med], dtype=np.float64)
        req, rule, _ = np_kf.decide(st, fd, p3, bool(has), MAX_KP, INITIAL_PARALLAX, bool(ba))
        want.append((int(req), rule))
    return rows, want


GRID = _grid()


def test_model_covers_every_exit_both_ways():
    """the grid is worth its rows: every rule code occurs, the parallax rule and the two `true` exits with both outcomes where they have two"""
    rows, want = GRID
    assert len(rows) == 5 * 5 * 5 * 2 * 4 * 5 * 2
    seen = set(want)
    assert {(0, 0), (1, 1), (1, 2), (0, 3), (0, 4), (1, 4)} == seen, seen
    # at 1000 keypoints 0.33 * 1000 rounds to 330.0 in doubles: 329 cells are sparse, 330 are not
    st = lambda c: np.array([1000, 100, 0, 900, c, 900, 0.0, 0.0])
    assert np_kf.decide(st(329), 5, 100, True, 1000)[:2] == (True, 1) and np_kf.decide(st(330), 5, 100, True, 1000)[:2] == (False, 4)


def test_keyframe_required_equals_the_model_on_the_grid(slam_host):
    from slam_jl_amd import _lib as L
    from slam_jl_amd.keypoint_set import keyframe_required
    lib = L.load()
    rows, want = GRID
    a = np.array(rows, dtype=np.float64)
    wreq = np.array([w[0] for w in want], dtype=np.uint8); wrule = np.array([w[1] for w in want], dtype=np.uint8)
    P = slam_host.Params(max_nb_keypoints=MAX_KP)
    assert P.initial_parallax == INITIAL_PARALLAX                                   # params.jl:66
    for ba in LOCAL_BA:
        sel = np.nonzero(a[:, 3] == ba)[0]
        S = len(sel)
        st = np.zeros((S, 8)); st[:, 0] = 1000; st[:, 1] = a[sel, 1]; st[:, 3] = 900; st[:, 4] = a[sel, 0]; st[:, 5] = 900; st[:, 6] = a[sel, 5]; st[:, 7] = a[sel, 5]
        fd = np.ascontiguousarray(a[sel, 2].astype(np.int32)); p3 = np.ascontiguousarray(a[sel, 4].astype(np.int32)); has = np.ascontiguousarray(a[sel, 6].astype(np.uint8))
        req = np.full(S, 9, np.uint8); rule = np.full(S, 9, np.uint8)
        rc = lib.slam_keyframe_required(S, L.ptr(st), L.ptr(fd, L.i32p), L.ptr(p3, L.i32p), L.ptr(has, L.u8p), MAX_KP, INITIAL_PARALLAX, ba,
                                        L.ptr(req, L.u8p), L.ptr(rule, L.u8p))
        assert rc == 0
        assert np.array_equal(req, wreq[sel]) and np.array_equal(rule, wrule[sel]), np.nonzero((req != wreq[sel]) | (rule != wrule[sel]))[0][:10]
        req2 = np.full(S, 9, np.uint8)                                              # rule == NULL
        assert lib.slam_keyframe_required(S, L.ptr(st), L.ptr(fd, L.i32p), L.ptr(p3, L.i32p), L.ptr(has, L.u8p), MAX_KP, INITIAL_PARALLAX, ba,
                                          L.ptr(req2, L.u8p), None) == 0 and np.array_equal(req2, req)
        r3, u3 = keyframe_required(st, fd, p3, has, P, local_ba_on=bool(ba))        # the wrapper
        assert np.array_equal(r3, wreq[sel].astype(bool)) and np.array_equal(u3, wrule[sel])
    # refusals: SLAM_ERR_ARG (-1), nothing written
    req = np.full(1, 7, np.uint8); z = np.zeros(1, np.int32); h = np.ones(1, np.uint8); st = np.zeros((1, 8))
    for args in ((0, L.ptr(st), L.ptr(z, L.i32p), L.ptr(z, L.i32p), L.ptr(h, L.u8p)), (1, None, L.ptr(z, L.i32p), L.ptr(z, L.i32p), L.ptr(h, L.u8p)),
                 (1, L.ptr(st), None, L.ptr(z, L.i32p), L.ptr(h, L.u8p)), (1, L.ptr(st), L.ptr(z, L.i32p), L.ptr(z, L.i32p), None)):
        assert lib.slam_keyframe_required(*args, MAX_KP, INITIAL_PARALLAX, 0, L.ptr(req, L.u8p), None) == -1 and req[0] == 7
    assert b"slam_keyframe_required" in lib.slam_last_error(None)


BUILDS = pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])


@BUILDS
def test_kf_decide_host_program(tmp_path, flags):
    rows, want = GRID
    table = tmp_path / "kf_table.txt"
    with open(table, "w") as f:
        for (cells, n3, fd, ba, p3, med, has), (req, rule) in zip(rows, want):
            m = "nan" if med != med else float(med).hex()
            f.write(f"{cells} {n3} {fd} {ba} {p3} {m} {has} {MAX_KP} {INITIAL_PARALLAX!r} {req} {rule}\n")
    exe = str(tmp_path / "kf_decide_check")
    cxx = os.environ.get("CXX", "c++")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", INC] + flags + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe, str(table)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("kf_decide OK") and f"{len(rows)} rows" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
