"""CPU: the pyramid filters' shared arithmetic (csrc/pyr_iir.hpp) replayed by a stand-alone host program and compared with the oracle,
every bit of every double.  The program (tests/c_host/pyr_iir_check.cpp) filters each line twice -- plainly, and through the
checkpointed pass A / pass B split with a host array as the checkpoint buffer -- and resizes with resize_coord on both axes.
Built twice: plain, and with -fsanitize=address,undefined (the program alone; nothing loaded into Python runs under a sanitizer)."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "pyr_iir_check.cpp")
INC = os.path.join(ROOT, "slam.jl_amd", "csrc")

# line lengths: 4 .. 7 (4 is the smallest a pyramid accepts; up to 6 the checkpointed sweep has no block at all), the 3 + 32 j block
# edges with and without a remainder block and with `have_last` true and false, and three full blocks (one checkpoint read twice)
LINES = [4, 5, 6, 7, 34, 35, 36, 38, 67, 99]
SIGMAS = [1.0, 4.0]
BORDERS = [0, 1]                                     # replicate, Fill(0)
RESIZES = [(4, 2), (5, 3), (7, 4), (8, 4), (65, 33), (2049, 1025)]
UPSIZES = [(2, 4), (3, 7), (4, 5)]                   # enlargements: the s < 1 clamp of resize_coord, which only k_resize's callers can reach
ROWS = 4                                             # the other axis of every case: the shortest line


def _hex(v):
    return " ".join(float(x).hex() for x in np.asarray(v, dtype=np.float64).ravel(order="F"))


def _coef(sigma):
    a, scale, M, asum = oracle.iir_coeffs(sigma)
    return _hex(list(a) + [scale] + list(M.ravel()) + [1 - asum, 1 - asum])


def _image(H, W, seed):
    return np.asfortranarray(np.random.default_rng(seed).random((H, W)))


def _iir_cases():
    return [(n, s, b) for n in LINES for s in SIGMAS for b in BORDERS]


def _rz_cases():
    return [(ns, nd, axis) for ns, nd in RESIZES for axis in (0, 1)]


def _rz_shape(ns, nd, axis):
    return ((ns, ROWS), (nd, ROWS // 2)) if axis == 0 else ((ROWS, ns), (ROWS // 2, nd))


FLAGS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(FLAGS), ids=list(FLAGS))
def replay(request, tmp_path_factory):
    """One build and one run per flag set: {case: flat array of the program's doubles}."""
    exe = str(tmp_path_factory.mktemp("pyr_iir_" + request.param) / "pyr_iir_check")
    cxx = os.environ.get("CXX", "c++")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", INC] + FLAGS[request.param] + [SRC, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    keys, lines = [], []
    for i, (n, sigma, border) in enumerate(_iir_cases()):
        keys.append(("iir", n, sigma, border))
        lines.append(f"iir {_coef(sigma)} {float(border).hex()} {float(ROWS).hex()} {float(n).hex()} {_hex(_image(ROWS, n, 100 + i))}")
    for i, (ns, nd, axis) in enumerate(_rz_cases()):
        (Hs, Ws), (Hd, Wd) = _rz_shape(ns, nd, axis)
        for me in (1, 0):                                # k_resize's form, and the fused kernels' (may_enlarge = false)
            keys.append(("rz", ns, nd, axis, me))
            lines.append("rz " + " ".join(float(v).hex() for v in (me, Hs, Ws, Hd, Wd)) + " " + _hex(_image(Hs, Ws, 500 + i)))
    for i, (ns, nd) in enumerate(UPSIZES):
        keys.append(("up", ns, nd))
        lines.append("rz " + " ".join(float(v).hex() for v in (1, ns, ROWS, nd, ROWS // 2)) + " " + _hex(_image(ns, ROWS, 700 + i)))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.strip().split("\n")
    assert len(out) == len(keys), r.stdout[-2000:]
    return {k: np.array([float.fromhex(t) for t in ln.split()]) for k, ln in zip(keys, out)}


def _same_bits(got, want):
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(np.asarray(want, dtype=np.float64).ravel(order="F"))
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("n,sigma,border", _iir_cases())
def test_iir_line_bits(replay, n, sigma, border):
    i = _iir_cases().index((n, sigma, border))
    want = oracle.iir_gaussian(_image(ROWS, n, 100 + i), sigma, border)
    got = replay[("iir", n, sigma, border)]
    assert got.size == 2 * ROWS * n
    assert _same_bits(got[:ROWS * n], want), "plain sweep"
    assert _same_bits(got[ROWS * n:], want), "checkpointed pass A / pass B"


@pytest.mark.parametrize("ns,nd,axis", _rz_cases())
def test_resize_bits(replay, ns, nd, axis):
    i = _rz_cases().index((ns, nd, axis))
    (Hs, Ws), (Hd, Wd) = _rz_shape(ns, nd, axis)
    want = oracle.imresize(_image(Hs, Ws, 500 + i), Hd, Wd)
    assert _same_bits(replay[("rz", ns, nd, axis, 1)], want), "may_enlarge = true"
    assert _same_bits(replay[("rz", ns, nd, axis, 0)], want), "may_enlarge = false"


def _imresize_clamped(img, Hd, Wd):
    """imresize! in Float64 with the source coordinate clamped to the image first when an axis grows (ImageTransformations' s < 1 branch);
    the C oracle has no such branch (the pyramid only shrinks), so the enlargements are checked against these lines."""
    Hs, Ws = img.shape
    def coord(ns, nd, k):
        s = float(ns) / float(nd); c = s * k + (1 - 0.5 - s * (1 - 0.5))
        if s < 1:
            c = 1.0 if c < 1 else (float(ns) if c > ns else c)
        i = min(max(int(np.floor(c)), 1), ns - 1)
        return i, c - i
    out = np.empty((Hd, Wd), order="F")
    for x in range(1, Wd + 1):
        for y in range(1, Hd + 1):
            (iy, fy), (ix, fx) = coord(Hs, Hd, y), coord(Ws, Wd, x)
            r0 = (1 - fx) * img[iy - 1, ix - 1] + fx * img[iy - 1, ix]
            r1 = (1 - fx) * img[iy, ix - 1] + fx * img[iy, ix]
            out[y - 1, x - 1] = (1 - fy) * r0 + fy * r1
    return out


@pytest.mark.parametrize("ns,nd", UPSIZES)
def test_resize_enlarging_clamps_to_the_source(replay, ns, nd):
    i = UPSIZES.index((ns, nd))
    img = _image(ns, ROWS, 700 + i)
    want = _imresize_clamped(img, nd, ROWS // 2)
    assert _same_bits(replay[("up", ns, nd)], want)
    assert want.min() >= img.min() and want.max() <= img.max()      # clamped: an interpolation, never an extrapolation
