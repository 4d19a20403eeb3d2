"""CPU: the host arithmetic of the compact right batch (csrc/kpset_select.hpp: kpset_select_rank, the member of a compact batch that holds a
stream's build -- the inverse of the ascending table -- and kpset_select_same, the stale-build check of slam_kpset_stereo_match_compact) as a
stand-alone host program (tests/c_host/compact_rank_check.cpp) at S in {1, 64, 65, 128} under null, none, all, first, last, alternating and random
masks -- built plain and with -fsanitize=address,undefined (the program alone; nothing loaded into Python runs under a sanitizer)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "compact_rank_check.cpp")
INC = os.path.join(ROOT, "slam.jl_amd", "csrc")

BUILDS = pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])


@BUILDS
def test_compact_rank_host_program(tmp_path, flags):
    exe = str(tmp_path / "compact_rank_check")
    cxx = os.environ.get("CXX", "c++")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", INC] + flags + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    n_cases = 4 * (3 + 2 + 2 + 8)                 # 4 sizes x (null, none, all, first, last, 2 alternating, 8 random)
    assert r.returncode == 0 and r.stdout.strip().endswith("compact_rank OK") and f"{n_cases} cases" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_the_library_uses_this_arithmetic():
    """the header under test is the one the library includes: slam_kpset_select stages its rank table, the compact build compacts with its plan,
    and the compact match's stale-build check is its mask comparison"""
    src = {f: open(os.path.join(INC, f)).read() for f in ("kpset.hpp", "kpset.hip", "pyramid.hip", "lk.hip")}
    assert '#include "kpset_select.hpp"' in src["kpset.hpp"] and '#include "kpset_select.hpp"' in src["pyramid.hip"]
    assert "kpset_select_rank(S, idx, n_sel, rank)" in src["kpset.hip"]
    assert "kpset_select_plan(S, selected, idx, norm)" in src["pyramid.hip"]
    assert "kpset_select_same(al->sel_S, al->sel_mask, ks->S, cur)" in src["lk.hip"]
