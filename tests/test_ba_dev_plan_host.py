"""CPU: csrc/ba_dev_plan.hpp -- which windows the one-workgroup BA kernel takes, the relabelling of poses, the cost split -- as a stand-alone host
program (tests/c_host/ba_dev_plan_check.cpp), built plain and with -fsanitize=address,undefined (the program alone; nothing is loaded into Python),
held to the numpy model tests/np_ba_dev_stage.py on the window set the GPU test solves, on the windows it must refuse and on small structural cases
(one pose, one free pose among several, no constant pose, 128 / 129 poses, 168 / 169 observations of a point).  The model itself is held to the
input: its staged arrays reconstruct the window (the permutations invert), and four mutants of it fail the same assertions."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_ba_dev_stage as npd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRC = os.path.join(ROOT, "tests", "c_host", "ba_dev_plan_check.cpp")
INC = os.path.join(ROOT, "slam.jl_amd", "csrc")
FLAGS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def _structural(P, free, counts):
    """a window given by its free poses and per-point lists of observing poses (structure only)"""
    tc = np.ones(P, dtype=np.uint8); tc[list(free)] = 0
    pi = np.array([p + 1 for obs in counts for p in obs], dtype=np.int64)
    li = np.array([j + 1 for j, obs in enumerate(counts) for _ in obs], dtype=np.int64)
    return dict(P=P, M=len(counts), O=len(pi), theta_const=tc, pose_ids=pi, point_ids=li)


def structural_cases():
    out = [
        _structural(1, (0,), [[0], [0]]),                                     # one pose, free: the rule admits it, the batch does not take it
        _structural(4, (2,), [[0, 2], [1, 2, 3]]),                            # one free pose among several
        _structural(3, (0, 1, 2), [[0, 1], [1, 2], [0, 2]]),                  # no constant pose
        _structural(7, (0, 2, 3, 5, 6), [[0, 1, 2], [], [3, 4, 5, 6], [1]]),  # five free, scattered; a point nobody observes; one seen by a constant pose only
        _structural(7, (0, 1, 2, 4, 5, 6), [[0, 1, 2], [3, 4]]),              # six free
        _structural(128, (126, 127), [[0, 126, 127], [5, 127]]),
        _structural(129, (127, 128), [[0, 127, 128]]),
        _structural(170, (168, 169), [list(range(128)) + list(range(130, 170))]),      # 168 observations of one point, but 170 poses
        _structural(3, (1, 2), [[0] * 166 + [1, 2], [0, 1]]),                 # 168 of one point
        _structural(3, (1, 2), [[0] * 167 + [1, 2], [0, 1]]),                 # 169
        _structural(2, (1,), []),                                             # no points, no observations
    ]
    rng = np.random.default_rng(5)
    for _ in range(40):
        P = int(rng.integers(1, 12)); M = int(rng.integers(1, 30))
        free = [p for p in range(P) if rng.random() < 0.4]
        out.append(_structural(P, free, [sorted(rng.choice(P, int(rng.integers(0, P + 1)), replace=False).tolist()) for _ in range(M)]))
    return out


@pytest.fixture(scope="module")
def windows():
    from slam_jl_amd import synthetic as syn
    return npd.window_set(syn) + npd.ineligible_set(syn)


@pytest.fixture(scope="module", params=list(FLAGS), ids=list(FLAGS))
def replay(request, tmp_path_factory, windows):
    exe = str(tmp_path_factory.mktemp("ba_dev_plan_" + request.param) / "ba_dev_plan_check")
    cxx = os.environ.get("CXX", "c++")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", INC] + FLAGS[request.param] + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    cases = list(windows) + structural_cases()
    lines = [str(len(cases))]
    for w in cases:
        lines += ["%d %d %d" % (w["P"], w["M"], w["O"]), " ".join(map(str, w["theta_const"])), " ".join(map(str, w["pose_ids"])), " ".join(map(str, w["point_ids"]))]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:] + r.stderr[-2000:])
    out = r.stdout.strip("\n").split("\n")
    assert len(out) == len(cases)
    return list(zip(cases, [[int(t) for t in ln.split()] for ln in out]))


def test_the_cases_cover_what_they_claim(windows):
    cases = list(windows) + structural_cases()
    el = [npd.eligible(npd.probe(w["P"], w["M"], w["O"], w["theta_const"], w["pose_ids"], w["point_ids"]), w["P"], w["M"], w["O"]) for w in cases]
    assert all(el[:6]) and el[6:10] == [False, False, True, False]
    assert any(w["M"] == 1 for w in windows) and any(256 < w["M"] <= 300 for w in windows)
    assert any((w["theta_const"] == 0).sum() == 5 and w["P"] == 25 for w in windows)
    # free poses that relabelling has to move, and points no free pose observes
    assert any(np.diff(np.flatnonzero(w["theta_const"] == 0)).max(initial=1) > 1 for w in windows[:6])
    for w in windows[:6]:
        assert w["O"] and (np.diff(w["point_ids"]) >= 0).all()
    w = windows[2]
    free_obs = w["theta_const"][w["pose_ids"] - 1] == 0
    assert len(np.unique(w["point_ids"][free_obs])) < len(np.unique(w["point_ids"]))


def test_header_equals_the_model(replay):
    for w, v in replay:
        P, M, O = w["P"], w["M"], w["O"]
        tc = np.asarray(w["theta_const"])
        pr = npd.probe(P, M, O, tc, w["pose_ids"], w["point_ids"])
        order, label = npd.relabel(tc)
        free = np.flatnonzero(tc == 0)
        nfree, cmax, p0u, su, p0, sp, rule = v[:7]
        assert (nfree, cmax) == (pr["nfree"], pr["cmax"]), (P, M, O)
        want_u = (int(free[0]), int(free[-1] - free[0] + 1)) if len(free) >= 2 else (0, P)
        assert (p0u, su) == want_u and (p0, sp) == npd.free_span_relabelled(P, nfree)
        assert bool(rule) == npd.window_rule(pr, P, M, O), (P, M, O, pr)
        assert v[7:7 + P] == order.tolist() and v[7 + P:7 + 2 * P] == label.tolist()
        assert v[7 + 2 * P:7 + 3 * P] == np.concatenate([np.flatnonzero(tc != 0), free[::-1]]).tolist()
        st = npd.stage(P, M, O, np.zeros(6 * P + 3 * M), tc, np.zeros((O, 2)), w["pose_ids"], w["point_ids"])
        kc, ko = v[7 + 3 * P:]
        if M > 1:
            assert kc == st["ksplit"], (P, M, O, kc, st["ksplit"])
        assert ko == min(int(np.searchsorted(st["pt_start"], (O + 1) // 2)), M)


def test_the_model_reconstructs_its_input(windows):
    for w in windows[:6]:
        npd.check_staged(w, npd.stage(w["P"], w["M"], w["O"], w["theta0"], w["theta_const"], w["pixels_yx"], w["pose_ids"], w["point_ids"]))


@pytest.mark.parametrize("mutant", ["not_consecutive", "pfs_off_by_one", "ksplit_obs_only"])
def test_a_mutant_of_the_stager_is_rejected(windows, mutant):
    bad = 0
    for w in windows[:6]:
        try:
            npd.check_staged(w, npd.stage(w["P"], w["M"], w["O"], w["theta0"], w["theta_const"], w["pixels_yx"], w["pose_ids"], w["point_ids"], mutant=mutant))
        except AssertionError:
            bad += 1
    assert bad >= 1, mutant


def test_a_rule_that_admits_one_free_pose_among_several_is_rejected(replay):
    """the fourth mutant: the header's answers differ from the mutated model's on the windows with one free pose among several"""
    differs = 0
    for w, v in replay:
        pr = npd.probe(w["P"], w["M"], w["O"], w["theta_const"], w["pose_ids"], w["point_ids"])
        if bool(v[6]) != npd.window_rule(pr, w["P"], w["M"], w["O"], mutant="admit_one_free"):
            differs += 1
            assert pr["nfree"] == 1 and w["P"] > 1
    assert differs >= 2
