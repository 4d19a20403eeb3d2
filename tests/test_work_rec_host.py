"""CPU: where the work records of a match live (csrc/work_order.hpp: work_rec_slot and its inverse work_rec_entry) as a stand-alone host
program -- for ntot in {0, 1, 7, 8, 9, 63, 64, 65, S cap - 1, S cap} and strides from capacities that are no multiple of 8, every entry gets a
distinct slot inside the 8 x stride records, and the walk of k_kpset_match (launches smaller than, equal to and larger than the list) visits
exactly the ntot entries once each, XCD x its contiguous eighth in order.  Built twice: plain, and with -fsanitize=address,undefined (the
program alone; nothing loaded into Python runs under a sanitizer).  The record's size and alignment are a static_assert next to its
definition (csrc/kpset.hpp); there is no Python mirror of it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "work_rec_check.cpp")
INC = os.path.join(ROOT, "slam.jl_amd", "csrc")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "ubsan"])
def test_work_rec_host_program(tmp_path, flags):
    exe = str(tmp_path / "work_rec_check")
    cxx = os.environ.get("CXX", "c++")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", INC] + flags + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("work_rec OK"), r.stdout[-2000:] + r.stderr[-2000:]


def test_the_kernels_use_the_header():
    """the mapping under test is the one both kernels call, and the record keeps the layout the match's fetch restates"""
    inc = open(os.path.join(INC, "kpset.hip")).read()
    lk = open(os.path.join(INC, "lk.hip")).read()
    hpp = open(os.path.join(INC, "kpset.hpp")).read()
    assert "work_rec_slot(idx, per, R.stride)" in inc and "work_rec_stride((long long)n)" in inc
    assert "LK_XCDS 8" in lk and "WORK_XCDS 8" in open(os.path.join(INC, "work_order.hpp")).read()
    assert re.search(r"static_assert\(sizeof\(KpWorkRec\) == 48 && alignof\(KpWorkRec\) == 16", hpp)
    assert "kp_match_prior(" in inc and "kp_match_prior(" in lk        # ONE routine for the prior, called by the work list and by the record-less prologue
