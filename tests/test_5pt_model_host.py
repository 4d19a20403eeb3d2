"""CPU: orc_five_point_solve against an independent model of the minimal problem (tests/np_5pt.py: SVD null space, the ten
cubics by dictionary polynomial arithmetic in extended precision, action matrix + eigenvectors, every solution polished by Newton in
complex extended precision).  The device kernel k_5pt_solve is held to the oracle bit for bit (tests/test_gpu_5pt_hypotheses.py), so
this is the one place where the ARITHMETIC both share is judged by something that does not share it.

Case list (np_5pt.groups): five_point_scene(n = 60), seeds 0-5 x noise 0 / 0.5 px x 64 tuples (768); noise-free seeds 0-7 x 100
tuples (800); three searched tuples with eight real solutions (four more occur among the 768).  Real-solution counts over the list:
2: 147, 4: 783, 6: 634, 8: 7 tuples.

Assertions
  admission   a property of the inputs, read from the model alone: every solution clearly real (relative imaginary part <= 1e-9) or
              clearly complex (>= 1e-4), the real solutions' unit-norm Es pairwise >= 1e-6 apart, model residual <= 1e-12.  At most
              5 % of the list may be refused.  Measured: 1571 of 1571 admitted; the model's worst residual is 2e-19.
  soundness   every E the oracle returns is within 1e-6 (max-abs of the Frobenius-normalised Es, sign-free) of a model solution: an
              epipolar line moves by ~1e-3 px across a 1241 px frame, three orders under the 3 px inlier gate.  No exceptions.
  completeness  fewer Es than the model has real solutions on <= 1 % of the tuples, never more; on the noise-free tuples the true
              motion is within 1e-6 of a returned E on >= 99 %.
  mutants     the same assertions reject: last root dropped, one root moved by 1e-5 relative, E transposed, x and y exchanged in the
              back-substitution (each applied to the model's own solutions, which pass).

Measured (this commit: two Gauss-Newton steps on the ten constraints after the back-substitution, gate 1e-9 on the unit-norm E):
  worst distance 5.1e-08; 7279 hypotheses, 1 above 1e-9; fewer Es on 5 of 1571 tuples (0.32 %), never more; truth found on 797 of
  800 (99.6 %; the model alone: 800 of 800).  The gate dropped 5 of 7284 polished hypotheses, at distances 2.6e-6, 5.8e-4, 2.2e-3,
  8.8e-3 and 3.4e-2 from the nearest solution (residuals 7.6e-9 ... 3.0e-3): nothing within 1e-6 of a solution was lost; the
  largest residual it kept is 3.1e-10, at distance 5.1e-8.  On 4352 tuples outside this list (seeds 6-39): worst 1.7e-9, fewer on 6.
The parent (no polish, no gate): soundness FAILED on 79 of 1571 tuples (17 of the 768), worst distance 0.447 (an E that misses
  the cubic constraints by 4e-2: not an essential matrix); 804 of 7284 hypotheses above 1e-9; fewer Es on 1 tuple; truth found on
  780 of 800 (97.5 %).  (The issue that asked for this test counted 31 of 768 on its own draw of the list.)  The comment "the rest:
  ill-conditioned 5-tuples" that tests/test_oracle_5pt.py carried was wrong: the model solves every one of them to 1e-15."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_5pt as m5  # noqa: E402

SOUND, MAX_REFUSED, MAX_FEWER, MIN_FOUND = 1e-6, 0.05, 0.01, 0.99


@pytest.fixture(scope="module")
def cases(syn):
    """the case list with the model's solutions, computed once: [(name, q1 (k, 5, 2), q2, model dict, true E or None)]"""
    out = []
    for name, sc, tuples, clean in m5.groups(syn):
        q1, q2 = m5.tuple_points(sc, tuples)
        out.append((name, q1, q2, m5.solve(q1, q2), m5.true_E(sc) if clean else None))
    return out


def judge(solver, cases):
    """Run solver(q1 (5, 2), q2 (5, 2), model, t) -> list of 3x3 E over the admitted tuples; return the figures the assertions are about."""
    f = dict(tuples=0, admitted=0, hyps=0, worst=0.0, unsound=0, above_1e9=0, fewer=0, more=0, clean=0, found=0, model_found=0)
    for name, q1, q2, mod, Et in cases:
        for t in range(len(q1)):
            f["tuples"] += 1
            if not mod["admitted"][t]:
                continue
            f["admitted"] += 1
            Em = mod["E"][t][mod["real"][t]]
            Es = solver(q1[t], q2[t], mod, t)
            d = np.array([m5.dist(E, Em).min() for E in Es]) if len(Es) else np.zeros(0)
            d = np.where(np.isfinite(d), d, np.inf)
            f["hyps"] += len(Es); f["above_1e9"] += int((d > 1e-9).sum())
            f["worst"] = max(f["worst"], float(d.max()) if len(d) else 0.0)
            f["unsound"] += bool((d > SOUND).any())
            f["fewer"] += len(Es) < len(Em); f["more"] += len(Es) > len(Em)
            if Et is not None:
                f["clean"] += 1
                f["found"] += bool(len(Es)) and min(m5.dist(E, Et) for E in Es) < SOUND
                f["model_found"] += m5.dist(Em, Et).min() < SOUND
    return f


def verdict(f):
    """the assertions, as a list of the ones that fail"""
    bad = []
    if f["admitted"] < (1 - MAX_REFUSED) * f["tuples"]:
        bad.append("admission")
    if f["unsound"] or not f["worst"] <= SOUND:
        bad.append("soundness")
    if f["more"] or f["fewer"] > MAX_FEWER * f["admitted"]:
        bad.append("count")
    if f["found"] < MIN_FOUND * f["clean"]:
        bad.append("truth")
    return bad


def test_model_is_its_own_reference(cases):
    """the model's solutions: ten per tuple, an even number of real ones, residual at the extended-precision floor, and the four real-solution
    counts the device root search needs all occur"""
    counts = {}
    for name, q1, q2, mod, Et in cases:
        assert mod["xyz"].shape == (len(q1), 10, 3)
        for t in range(len(q1)):
            if mod["admitted"][t]:
                k = int(mod["real"][t].sum())
                counts[k] = counts.get(k, 0) + 1
                assert k % 2 == 0 and mod["res"][t][mod["real"][t]].max() <= m5.MAX_RESIDUAL
                h1 = np.c_[q1[t], np.ones(5)]; h2 = np.c_[q2[t], np.ones(5)]
                assert np.abs(np.einsum("ij,ejk,ik->ei", h2, mod["E"][t][mod["real"][t]], h1)).max() < 1e-13
    print("real-solution counts:", dict(sorted(counts.items())))
    assert all(counts.get(k, 0) > 0 for k in (2, 4, 6)) and sum(v for k, v in counts.items() if k >= 8) >= 5


def test_oracle_solver_against_the_model(orc, cases):
    f = judge(lambda q1, q2, mod, t: orc.five_point_solve(q1, q2), cases)
    print("orc_five_point_solve vs model: admitted %d of %d (%.2f %%); worst distance %.3g; %d hypotheses, %d above 1e-9, unsound tuples %d; "
          "fewer Es on %d tuples (%.2f %%), more on %d; truth found on %d of %d noise-free tuples (%.2f %%; model %d)"
          % (f["admitted"], f["tuples"], 100.0 * f["admitted"] / f["tuples"], f["worst"], f["hyps"], f["above_1e9"], f["unsound"], f["fewer"],
             100.0 * f["fewer"] / f["admitted"], f["more"], f["found"], f["clean"], 100.0 * f["found"] / f["clean"], f["model_found"]))
    assert f["tuples"] >= 1568 and f["clean"] >= 0.95 * 800
    assert f["model_found"] == f["clean"]
    assert verdict(f) == [], (verdict(f), f)


def _model_E(mod, t, xyz):
    N = mod["N"][t]
    return [x * N[0] + y * N[1] + z * N[2] + N[3] for x, y, z in xyz]


def _mutants():
    def real_xyz(mod, t):
        return mod["xyz"][t][mod["real"][t]].real.astype(float)
    def exact(q1, q2, mod, t):
        return _model_E(mod, t, real_xyz(mod, t))
    def last_root_dropped(q1, q2, mod, t):
        return exact(q1, q2, mod, t)[:-1]
    def one_root_moved(q1, q2, mod, t):
        s = real_xyz(mod, t).copy()
        s[0, 2] *= 1.0 + 1e-5
        return _model_E(mod, t, s)
    def transposed(q1, q2, mod, t):
        return [E.T for E in exact(q1, q2, mod, t)]
    def xy_exchanged(q1, q2, mod, t):
        return _model_E(mod, t, real_xyz(mod, t)[:, [1, 0, 2]])
    return exact, [last_root_dropped, one_root_moved, transposed, xy_exchanged]


def test_assertions_reject_mutant_solvers(cases):
    """the model's own solutions pass; each mutant of them fails the assertion it should (on the noise-free groups: they carry the truth check)"""
    sub = [c for c in cases if c[4] is not None][:2]
    exact, mutants = _mutants()
    assert verdict(judge(exact, sub)) == []
    expect = {"last_root_dropped": "count", "one_root_moved": "soundness", "transposed": "soundness", "xy_exchanged": "soundness"}
    for mut in mutants:
        bad = verdict(judge(mut, sub))
        print(mut.__name__, "->", bad)
        assert expect[mut.__name__] in bad, (mut.__name__, bad)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])


@BUILDS
def test_oracle_routines_in_a_standalone_program(tmp_path, orc, syn, flags):
    """orc_five_point_solve (with its polish), orc_essential_pose_cheirality and orc_two_view_inliers in a plain C program of their own
    (tests/c_host/orc_5pt_check.c), built plain and with ASan + UBSan: it ends clean and writes what the library loaded here computes."""
    import subprocess
    sc = syn.five_point_scene(n=70, seed=41, noise_px=0.4, iters=48)
    n, thr = 70, 3.0
    q1, q2 = m5.tuple_points(sc, sc["samples"])
    degenerate = np.array([[0.1, 0.2], [0.1, 0.2], [0.3, -0.1], [0.0, 0.0], [-0.2, 0.1]])          # zero motion, a repeated point
    q1 = np.concatenate([q1, degenerate[None], np.zeros((1, 5, 2))]); q2 = np.concatenate([q2, degenerate[None], np.zeros((1, 5, 2))])
    T = len(q1)
    blob = np.concatenate([[T, n, thr], np.asfortranarray(sc["K"]).ravel(order="F"), sc["px1"].ravel(), sc["px2"].ravel(),
                           np.concatenate([q1.reshape(T, 10), q2.reshape(T, 10)], 1).ravel()]).astype(np.float64)
    fin, fout, exe = tmp_path / "in.bin", tmp_path / "out.bin", str(tmp_path / "orc_5pt_check")
    blob.tofile(fin)
    src = [os.path.join(ROOT, "tests", "c_host", "orc_5pt_check.c"), os.path.join(ROOT, "oracle", "orc_5pt.c"), os.path.join(ROOT, "oracle", "orc_tri.c")]
    b = subprocess.run([os.environ.get("CC", "cc"), "-std=gnu11", "-O1", "-g", "-ffp-contract=off", "-fopenmp", "-Wall", "-Werror", "-I", os.path.join(ROOT, "oracle")]
                       + flags + src + ["-o", exe, "-lm"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("orc_5pt OK"), r.stdout[-2000:] + r.stderr[-2000:]
    got = np.fromfile(fout)
    at = hyps = 0
    for t in range(T):
        Es = orc.five_point_solve(q1[t], q2[t])
        assert got[at] == len(Es), t
        at += 1
        for E in Es:
            row = got[at:at + 23 + n]; at += 23 + n; hyps += 1
            assert np.array_equal(row[:9].reshape(3, 3), E)
            P = orc.essential_pose_cheirality(E, q1[t], q2[t])
            assert row[9] == (P is not None)
            if P is not None:
                mask = orc.two_view_inliers(sc["px1"], sc["px2"], sc["K"], sc["K"], P, thr)
                assert np.array_equal(row[10:22], P.T.reshape(12)) and row[22] == mask.sum() and np.array_equal(row[23:] != 0, mask)
    assert at == len(got) and hyps > 4 * 48
