"""CPU: the pose seams' shared records and conversions (csrc/pose_records.hpp) and the typed regions of csrc/layout.hpp, replayed by a stand-alone
host program (tests/c_host/pose_records_check.cpp, which includes the two headers alone) and compared with a transcription in numpy float64 scalars
in the association the header documents -- every double with ==.  sin / cos / atan2 / sqrt are libm's on both sides (math.*).  Built twice: plain,
and with -fsanitize=address,undefined (the program alone; nothing loaded into Python runs under a sanitizer)."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "pose_records_check.cpp")
INC = os.path.join(ROOT, "slam.jl_amd", "csrc")
F = np.float64

# the offsets the kernels and the host code of the parent agreed on by hand
OFFSETS = {"P3POut": [0, 96, 192, 200, 204, 256], "FPOut": [0, 96, 168, 176, 180, 256], "PnPResult": [0, 48, 56, 64, 72, 80, 88, 128]}

COUNTS = [0, 1, 31, 32, 33, 255, 256, 257]
SIZES = [1, 4, 8, 16, 24]


# ---- the routines, transcribed (np.float64 scalars: one IEEE operation per Python operation, nothing fused) ---------------------------
def angles_to_pose(X):
    s1, c1, s2, c2, s3, c3 = (F(f(float(X[k]))) for k in range(3) for f in (math.sin, math.cos))
    R = [c1 * c2, c1 * s2 * s3 - s1 * c3, c1 * s2 * c3 + s1 * s3, s1 * c2, s1 * s2 * s3 + c1 * c3, s1 * s2 * c3 - c1 * s3, -s2, c2 * s3, c2 * c3]
    T = [F(1.0) if k % 5 == 0 else F(0.0) for k in range(16)]
    for i in range(3):
        for j in range(3):
            T[i + 4 * j] = R[3 * i + j]
    T[12], T[13], T[14] = F(X[3]), F(X[4]), F(X[5])
    return T


def pose_to_angles(M, t, ld):
    M = [F(x) for x in M]
    R11, R21, R31, R12, R22, R13, R23 = M[0], M[1], M[2], M[ld], M[ld + 1], M[2 * ld], M[2 * ld + 1]
    t1 = F(math.atan2(R21, R11)); s1 = F(math.sin(t1)); c1 = F(math.cos(t1))
    return [t1, F(math.atan2(-R31, math.sqrt(R11 * R11 + R21 * R21))), F(math.atan2(R13 * s1 - R23 * c1, R22 * c1 - R12 * s1)), F(t[0]), F(t[1]), F(t[2])]


def _angle_cases():
    rng = np.random.default_rng(2301)
    cases = {}
    for k in range(64):                                    # theta1, theta3 anywhere, theta2 inside its range: the round trip is well conditioned
        cases[("random", k)] = np.concatenate([rng.uniform(-3.1, 3.1, 1), rng.uniform(-1.4, 1.4, 1), rng.uniform(-3.1, 3.1, 1), rng.standard_normal(3) * 5.0])
    cases[("gimbal", "+")] = np.array([0.3, math.pi / 2, -0.7, 1.0, -2.0, 3.0])
    cases[("gimbal", "-")] = np.array([0.3, -math.pi / 2, -0.7, 1.0, -2.0, 3.0])
    cases[("zeros", 0)] = np.zeros(6)
    return cases


ANGLES = _angle_cases()
FLAGS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def _hex(v):
    return " ".join(float(x).hex() for x in np.asarray(v, dtype=np.float64).ravel())


def _rt(T):
    """column-major 3 x 4 [R | t] of a column-major 4 x 4 pose"""
    return [T[i + 4 * j] for j in range(4) for i in range(3)]


@pytest.fixture(scope="module", params=list(FLAGS), ids=list(FLAGS))
def replay(request, tmp_path_factory):
    """One build and one run per flag set: {case: the program's line}."""
    exe = str(tmp_path_factory.mktemp("pose_records_" + request.param) / "pose_records_check")
    cxx = os.environ.get("CXX", "c++")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", INC] + FLAGS[request.param] + [SRC, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    keys, lines = [], []
    for key, X in ANGLES.items():
        T = angles_to_pose(X)
        keys.append(("a2p",) + key); lines.append("a2p " + _hex(X))
        keys.append(("p2a4",) + key); lines.append("p2a4 " + _hex(T))
        keys.append(("p2a3",) + key); lines.append("p2a3 " + _hex(_rt(T)))
    keys.append(("take", "by_size")); lines.append("take " + " ".join("%d %d" % (s, c) for s in SIZES for c in COUNTS))
    keys.append(("take", "by_count")); lines.append("take " + " ".join("%d %d" % (s, c) for c in COUNTS for s in SIZES))
    keys.append(("offsets",)); lines.append("offsets")
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.strip("\n").split("\n")
    assert len(out) == len(keys), r.stdout[-2000:]
    return dict(zip(keys, (ln.split() for ln in out)))


def _doubles(tokens):
    return np.array([float.fromhex(t) for t in tokens])


def _same(got, want):
    want = np.asarray([float(x) for x in want], dtype=np.float64)
    return got.shape == want.shape and bool(np.all(got == want))


@pytest.mark.parametrize("key", list(ANGLES), ids=lambda k: "%s_%s" % k)
def test_conversions_bits(replay, key):
    X = ANGLES[key]
    T = angles_to_pose(X)
    got_T = _doubles(replay[("a2p",) + key])
    assert _same(got_T, T)
    assert _same(got_T[[3, 7, 11, 15]], [0.0, 0.0, 0.0, 1.0])      # the bottom row is the caller's: the routine leaves it alone
    got4, got3 = _doubles(replay[("p2a4",) + key]), _doubles(replay[("p2a3",) + key])
    assert _same(got4, pose_to_angles(T, T[12:15], 4))
    assert _same(got3, pose_to_angles(_rt(T), T[12:15], 3))
    assert _same(got3, got4)                                        # the two pitches read the same seven entries
    if key[0] == "random":                                          # |theta2| <= 1.4: cos(theta2) >= 0.17, the angles come back
        assert np.max(np.abs(got4 - X)) < 1e-12
    if key[0] == "zeros":
        assert _same(got_T, np.eye(4).ravel()) and _same(got4, np.zeros(6))


@pytest.mark.parametrize("order", ["by_size", "by_count"])
def test_typed_take_equals_untyped(replay, order):
    """take<T>(n) returns the offset and advances the end exactly as take(n * sizeof(T)) does, region after region."""
    pairs = [(s, c) for s in SIZES for c in COUNTS] if order == "by_size" else [(s, c) for c in COUNTS for s in SIZES]
    v = [int(t) for t in replay[("take", order)]]
    assert len(v) == 5 * len(pairs)
    end = 0
    for k, (size, count) in enumerate(pairs):
        off, nbytes, typed_end, raw_off, raw_end = v[5 * k: 5 * k + 5]
        assert (off, typed_end) == (raw_off, raw_end), (size, count)
        assert off == end and off % 256 == 0 and nbytes == size * count, (size, count)
        end += (size * count + 255) // 256 * 256                    # the rule stated once more from the outside
        assert typed_end == end, (size, count)


def test_record_offsets(replay):
    v = [int(t) for t in replay[("offsets",)]]
    assert v[:6] == OFFSETS["P3POut"] and v[6:12] == OFFSETS["FPOut"] and v[12:] == OFFSETS["PnPResult"]
