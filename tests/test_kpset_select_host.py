"""CPU: the selection plan of slam_kpset_select (csrc/kpset_select.hpp: mask -> ascending table of the selected streams, normalised mask, launch
sizes) as a stand-alone host program (tests/c_host/kpset_select_check.cpp) over S in {1, 3, 64, 65, 128} with empty, full, single and alternating
masks -- built plain and with -fsanitize=address,undefined (the program alone; nothing loaded into Python runs under a sanitizer)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "kpset_select_check.cpp")
INC = os.path.join(ROOT, "slam.jl_amd", "csrc")

BUILDS = pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])


@BUILDS
def test_kpset_select_host_program(tmp_path, flags):
    exe = str(tmp_path / "kpset_select_check")
    cxx = os.environ.get("CXX", "c++")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", INC] + flags + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    # 5 sizes x (null, empty, full, S singles, 2 alternating) + "all but the last" for S > 1
    n_cases = sum(3 + S + 2 + (S > 1) for S in (1, 3, 64, 65, 128))
    assert r.returncode == 0 and r.stdout.strip().endswith("kpset_select OK") and f"{n_cases} cases" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_the_library_uses_this_plan():
    """the header under test is the one kpset.hpp includes, and slam_kpset_select calls it"""
    hpp = open(os.path.join(INC, "kpset.hpp")).read()
    hip = open(os.path.join(INC, "kpset.hip")).read()
    assert '#include "kpset_select.hpp"' in hpp and "kpset_select_plan(S, selected, idx, norm)" in hip
