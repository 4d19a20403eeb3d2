"""CPU: the work list's sort key (csrc/work_order.hpp) as a stand-alone host program -- monotone in band and row, clamped at 0, W and
H, defined for NaN / +-inf / huge positions -- and the rule that picks the tracking kernels' instantiation for a window_size
(lk_slots / lk_window_elems, the same header).  Built twice: plain, and with -fsanitize=address,undefined,float-cast-overflow (the program
alone; nothing loaded into Python runs under a sanitizer)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "work_key_check.cpp")
INC = os.path.join(ROOT, "slam.jl_amd", "csrc")


BUILDS = pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"]], ids=["plain", "ubsan"])


def _build(tmp_path, flags):
    exe = str(tmp_path / "work_key_check")
    cxx = os.environ.get("CXX", "c++")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", INC] + flags + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    return exe


@BUILDS
def test_work_key_host_program(tmp_path, flags):
    exe = _build(tmp_path, flags)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("work_key OK"), r.stdout[-2000:] + r.stderr[-2000:]


# window_size -> template slots per lane of the instantiation the host launches (csrc/lk.hip: lk_launch)
LK_SLOTS = {0: 3, 1: 3, 2: 3, 3: 3, 4: 3, 5: 3, 6: 3, 7: 6, 8: 6, 9: 6, 10: 9, 11: 9, 12: 9, 13: 9, 14: 9, 15: 9, 16: 9}


@BUILDS
def test_lk_slots_table(tmp_path, flags):
    """lk_slots for windows 0..16 equals the table above, and the kernel's `cached` (elements <= 64 * slots) holds exactly for w <= 11."""
    r = subprocess.run([_build(tmp_path, flags), "slots"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [tuple(int(v) for v in ln.split()) for ln in r.stdout.strip().splitlines()]
    assert [w for w, _, _ in rows] == list(range(17))
    for w, slots, elems in rows:
        assert slots == LK_SLOTS[w] and elems == (2 * w + 1) ** 2, (w, slots, elems)
        assert (elems <= 64 * slots) == (w <= 11), (w, slots, elems)
