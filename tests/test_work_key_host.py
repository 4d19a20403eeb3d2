"""CPU: the work list's sort key (csrc/work_order.hpp) as a stand-alone host program -- monotone in band and row, clamped at 0, W and
H, defined for NaN / +-inf / huge positions.  Built twice: plain, and with -fsanitize=undefined,float-cast-overflow (the program
alone; nothing loaded into Python runs under a sanitizer)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "work_key_check.cpp")
INC = os.path.join(ROOT, "slam.jl_amd", "csrc")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all"]], ids=["plain", "ubsan"])
def test_work_key_host_program(tmp_path, flags):
    exe = str(tmp_path / "work_key_check")
    cxx = os.environ.get("CXX", "c++")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", INC] + flags + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("work_key OK"), r.stdout[-2000:] + r.stderr[-2000:]
