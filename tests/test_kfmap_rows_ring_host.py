"""CPU: the row-set routines of csrc/kfmap_ring.hpp (kfm_rows_find / _drop / _clear / _count / _next / _put / _union: what the kernels of the key-frame
map call for a point's descriptor rows) as a stand-alone host program (tests/c_host/kfmap_rows_check.cpp), built plain and with
-fsanitize=address,undefined (the program alone; nothing is loaded into Python).  The expected values come from the numpy model
(tests/np_kfmap_rows.py: put, union, a dict per point), not from the header.

Scripts at D = 2, 3, 8: a union with equal keys (the survivor's row stays), a union that overflows (the D largest keys stay, whatever the slots'
order; the excess is counted), sets with holes (drops in the middle, then puts that take the holes), the drop of an absent key, a put of a key below
a full set's smallest (the arriving row is the one that goes), and 200 random scripts per D."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_kfmap_rows as nr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "kfmap_rows_check.cpp")
INC = os.path.join(ROOT, "slam.jl_amd", "csrc")
FLAGS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
DS = (2, 3, 8)


def scripts(D):
    """-> [(name, [op tuples])]"""
    out = []
    full = [("p", k, 100 + k) for k in range(D)]
    out.append(("equal_keys", [("p", 3, 10), ("p", 5, 11), ("P", 5, 20), ("P", 4, 21), ("u",)]))
    out.append(("overflow", full + [("P", D + k, 200 + k) for k in range(D)] + [("u",)]))
    out.append(("overflow_interleaved", [("p", 2 * k, 100 + k) for k in range(D)] + [("P", 2 * k + 1, 200 + k) for k in range(D)] + [("u",)]))
    out.append(("overflow_reversed_slots", [("p", D - 1 - k, 100 + k) for k in range(D)] + [("P", 2 * D - k, 200 + k) for k in range(D)] + [("u",)]))
    out.append(("holes", full + [("d", 0)] + ([("d", D // 2)] if D > 2 else []) + [("p", 50, 7), ("p", 51, 8), ("p", 52, 9)]))
    out.append(("holes_in_prev", [("P", k, 300 + k) for k in range(D)] + [("D", 1), ("p", 1, 5), ("u",)]))
    out.append(("absent_drop", [("p", 4, 1), ("d", 9), ("d", 0), ("p", 6, 2), ("d", 5)]))
    out.append(("below_smallest", [("p", 10 + k, k) for k in range(D)] + [("p", 3, 99)]))
    out.append(("put_twice", [("p", 7, 1), ("p", 7, 2)]))
    out.append(("clear", full + [("c",), ("p", 1, 1)]))
    out.append(("empty_union", [("p", 1, 1), ("u",)]))
    rng = np.random.default_rng(500 + D)
    for t in range(200):
        ops = []
        for _ in range(int(rng.integers(1, 30))):
            kind = rng.choice(["p", "p", "P", "P", "d", "D", "u", "c"], p=[0.25, 0.15, 0.2, 0.1, 0.1, 0.05, 0.13, 0.02])
            if kind in ("p", "P"):
                ops.append((str(kind), int(rng.integers(0, 2 * D + 3)), int(rng.integers(0, 1 << 40))))
            elif kind in ("d", "D"):
                ops.append((str(kind), int(rng.integers(0, 2 * D + 3))))
            else:
                ops.append((str(kind),))
        out.append(("random%d" % t, ops))
    return out


def expected(D, ops):
    """the model's run of a script -> (dropped, [(key, w)] ascending); also what the script met"""
    A, B, dropped, met = {}, {}, 0, set()
    row = lambda w: np.array([w, w + 1, w + 2, w + 3], dtype=np.uint64)
    for op in ops:
        if op[0] in ("p", "P"):
            tgt = A if op[0] == "p" else B
            met.add("equal_put" if op[1] in tgt else "full_put" if len(tgt) == D else "put")
            dropped += nr.put(tgt, op[1], row(op[2]), D)
        elif op[0] in ("d", "D"):
            tgt = A if op[0] == "d" else B
            met.add("drop" if op[1] in tgt else "absent_drop")
            tgt.pop(op[1], None)
        elif op[0] == "c":
            A.clear()
        else:
            if set(A) & set(B):
                met.add("equal_union")
            if len(set(A) | set(B)) > D:
                met.add("overflow_union")
            dropped += nr.union(A, B, D)
            B.clear()
    return dropped, [(k, int(A[k][0])) for k in sorted(A)], met


SCRIPTS = {D: scripts(D) for D in DS}


@pytest.fixture(scope="module", params=sorted(FLAGS))
def replay(request, tmp_path_factory):
    """One build and one run per flag set: {(D, name): the program's line}."""
    exe = str(tmp_path_factory.mktemp("kfmap_rows_" + request.param) / "kfmap_rows_check")
    cxx = os.environ.get("CXX", "c++")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", INC] + FLAGS[request.param] + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    keys, lines = [], []
    for D in DS:
        for name, ops in SCRIPTS[D]:
            keys.append((D, name)); lines.append(" ".join([str(D)] + [str(t) for op in ops for t in op]))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.strip("\n").split("\n")
    assert len(out) == len(keys)
    return dict(zip(keys, out))


def test_the_scripts_cover_what_they_claim():
    for D in DS:
        met = set()
        for _, ops in SCRIPTS[D]:
            met |= expected(D, ops)[2]
        assert {"equal_put", "full_put", "put", "drop", "absent_drop", "equal_union", "overflow_union"} <= met, (D, met)
        by = dict(SCRIPTS[D])
        assert expected(D, by["overflow"])[:2] == (D, [(D + k, 200 + k) for k in range(D)])                 # the D largest keys stay, D rows counted
        assert expected(D, by["below_smallest"])[:2] == (1, [(10 + k, k) for k in range(D)])                 # the arriving row is the one that goes
        assert expected(D, by["equal_keys"])[1][-1] == (5, 11)                                                # the survivor's row under the equal key


@pytest.mark.parametrize("D", DS)
def test_row_sets_equal_the_model(replay, D):
    for name, ops in SCRIPTS[D]:
        v = [int(t) for t in replay[(D, name)].split()]
        dropped, rows, _ = expected(D, ops)
        assert v[0] == dropped and v[1] == len(rows) and list(zip(v[2::2], v[3::2])) == rows, (D, name)
