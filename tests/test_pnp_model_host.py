"""CPU: the long-double model of the single-pose refinement (hp_pnp.py) against the C oracle and np_pnp.py on every case of the GPU
test, the admission conditions of the case list, the trace properties the cases were chosen for, and the mutation test: every
fault of np_pnp.py is rejected by the assertion function of test_gpu_pnp_model.py (hp_pnp.check) at the asserted k.

Which case rejects which mutant at hp_pnp.K = parameters 12.3, costs 48.6 (the same table at ten times these k): named cases + how many
of the 130 small problems.  A fault that only acts on a branch is rejected only by the cases that reach the branch -- which is what
the case list is for:

  a   last observation dropped         57 + 130  every case with n >= 1 (all return a cost)
  b   unclamped damping                 1 +   0  far_n6 alone (the translation's diag(H) ~ 1e-7: the 1e-6 clamp IS its damping)
  c   |r| > repr_eps                   29 +  46  classify_*, it1_*, ...: flags differ wherever an r^2 lies between eps and eps^2
  d   n - no <= 5                       4 +   6  trip_n5, it5_10_n5, inliers_5, reject_accept_reject_pass2 (n - no = 5: the mutant exits)
  e   delta update without the cube     4 +   0  reject_both_passes, reject_accept_reject_pass2, reject_first_step, reject_then_identity
  f   decrease not reset                1 +   0  reject_accept_reject_pass2 (a rejection, an accepted step, a rejection)
  g   pass 2 keeps flagged points      33 +  96  every refined case with n_outliers > 0
  h   predicted = |J dx + r|^2         42 + 130  every case with an iteration whose pass has not converged to rounding
  i   Jacobian not rebuilt             26 + 130  every case with two accepted steps in a pass
  i2  Jacobian rebuilt after a reject   4 +   0  the four of e
  j   theta3 of the transposed R       57 + 130  every case with n >= 1

e, f and i2 are invisible on the scenes the suite had before: there rho ~ 1, so 1 - (2 rho - 1)^3 and 1 - (2 rho - 1) are both below the
1/3 floor, and nothing is ever rejected.  reject_pass1 / reject_twice_pass1 converge after their rejections and end within rounding
of the unmutated run: a converged run forgets how it got there, which is why the cases that stop early carry these rows."""
import numpy as np
import pytest

import hp_ba
import hp_pnp
import np_pnp


@pytest.fixture(scope="module")
def every_case(syn):
    cs = dict(hp_pnp.cases(syn))
    cs.update(hp_pnp.small_cases(syn))
    return cs


def _records(m):
    return m.trace1 + m.trace2


def test_model_oracle_and_numpy_take_the_same_decisions(orc, every_case):
    """decisions equal (flags, n_outliers, identity exit, and np_pnp's trace = the model's), errors printed"""
    bad = []
    worst = {}
    for name, q in every_case.items():
        y = hp_pnp.yardsticks(orc, q)
        for who, out in (("oracle", y.out_orc), ("np_pnp", y.out_np)):
            bad += [f"{name}: {who}: {c}" for c in hp_pnp.decisions(out, y.m)]
        a, kw = hp_pnp.call_args(q)
        tr = np_pnp.pnp_ba(*a, **kw, full=True)[5]
        if tr != hp_pnp.trace_string(y.m):
            bad.append(f"{name}: np_pnp's trace {tr} != the model's {hp_pnp.trace_string(y.m)}")
        if not name.startswith("small_"):
            print(f"{name:32s} n {q['n']:5d} no {y.m.n_outliers:4d} {'identity' if y.m.identity else '        '} {hp_pnp.trace_string(y.m):28s} "
                  + " ".join(f"{k} {y.e_orc.get(k, np.nan):.1e}/{y.e_np.get(k, np.nan):.1e}" for k in ("x", "R", "t", "initial", "final")))
        for k in y.e_orc:
            worst[k] = max(worst.get(k, 0.0), y.e_orc[k], y.e_np[k])
    print("largest E_orc / E_np per measure:", {k: f"{v:.2e}" for k, v in worst.items()})
    # how far the two f64 implementations are from EACH OTHER in the bound's own unit (one held to the other alone as its yardstick): the
    # final cost of a fitted scene is a sum of squares of 0.1-1 px differences of ~ 600 px coordinates, its rounding error a random draw
    spread = max(max(a["final"] / max(b["final"], hp_ba.F64_FLOOR) for a, b in ((y.e_orc, y.e_np), (y.e_np, y.e_orc)))
                 for y in (hp_pnp.yardsticks(orc, q) for q in every_case.values()))
    print(f"final cost: largest E_orc / max(E_np, floor) or E_np / max(E_orc, floor) over the list: {spread:.1f}")
    assert spread > hp_pnp.K["costs"] / 4                       # the r the k of the costs comes from lies inside this spread
    assert not bad, "\n".join(bad)
    # the f64 implementations are at rounding level on every case, so a bound of k * max(E_orc, E_np, floor) is a rounding-level bound.
    # (The cost of a run whose cost is ~ 0 -- one point, six parameters -- has no relative accuracy: it5_10_n1.)
    assert all(v < 1e-11 for k, v in worst.items() if k != "final"), worst


def test_every_case_is_admitted(orc, every_case):
    """classification margins >= 1e-6 (px^2, m), every |rho - 1e-3| >= 1e-3, no accepted step within 10 x the cost bound of the f_conv
    edge (|ssr - trial| / (|ssr| + ftol) moves by twice the costs' relative error), max|dx| not within 1e-3 of xtol (relative)"""
    bad = []
    for name, q in every_case.items():
        y = hp_pnp.yardsticks(orc, q)
        m = y.m
        if m.flag_margin.min(initial=np.inf) < 1e-6:
            bad.append(f"{name}: classification margin {m.flag_margin.min():.2e}")
        cost_bound = max(v for k, v in hp_pnp.bounds(y.e_orc, y.e_np).items() if hp_pnp.GROUP[k] == "costs")
        for i, t in enumerate(_records(m)):
            if t.rho_margin < 1e-3:
                bad.append(f"{name}: iteration {i}: rho = {t.rho}")
            if t.f_margin < 10 * 2 * min(cost_bound, 1e-9):
                bad.append(f"{name}: iteration {i}: f_conv margin {t.f_margin:.2e} against a cost bound of {cost_bound:.2e}")
            if t.x_margin < 1e-3:
                bad.append(f"{name}: iteration {i}: max|dx| = {t.maxdx}")
            if t.fired == "chol":
                bad.append(f"{name}: iteration {i}: the damped normal equations are not positive definite")
    assert not bad, "\n".join(bad)


def test_cases_have_the_properties_they_were_chosen_for(orc, syn):
    cs = hp_pnp.cases(syn)
    M = lambda name: hp_pnp.yardsticks(orc, cs[name]).m
    assert {q["n"] for q in cs.values()} >= set(hp_pnp.COUNTS)
    for name, q in cs.items():
        m, e = M(name), q.get("expect")
        tr = hp_pnp.trace_string(m)
        if name.startswith("trip_"):
            assert not m.identity and m.n_outliers == 0 and tr == "|" and float(m.final) == float(m.initial), name
        if e == "classify":
            assert 0.2 * q["n"] <= m.n_outliers <= 0.8 * q["n"] and tr == "|" and not m.by_depth.any(), name
        if e == "pass2_converges":
            assert 0 < len(m.trace2) < q["iterations"] and m.trace2[-1].fired != "" and len(m.trace1) < q["iters_fast"], (name, tr)
        if e == "trace":
            assert tr == q["trace"], (name, tr)
        if e == "depth_alone":
            only = m.by_depth & ~m.by_repr
            z = hp_pnp.Model(q["cam"], q["pixels_yx"], q["points"]).residuals(m.X1)[1]
            assert only.sum() == 7 and (z[only] < -1.0).all() and np.isfinite(z.astype(np.float64)).all(), name
        if e == "depth_in_front":
            only = m.by_depth & ~m.by_repr
            z = hp_pnp.Model(q["cam"], q["pixels_yx"], q["points"]).residuals(m.X1)[1]
            assert only.sum() >= 50 and (z[only] > 1.0).all() and (m.by_repr & ~m.by_depth).any(), name
        if e in ("inliers_4", "inliers_5"):
            assert q["n"] - m.n_outliers == int(e[-1]) and m.identity == (e == "inliers_4"), name
        if e == "clamp":
            st = hp_pnp.Model(q["cam"], q["pixels_yx"], q["points"]).step(m.X0, np.ones(q["n"], bool), 10.0)
            d = np.diag(st["H"]).astype(np.float64)
            assert (d[3:] < 1e-6).all() and (d[:3] > 1.0).all() and not m.identity, (name, d)
    # the rejection cases: a rejection in pass 1 that still ends in a pose; one in pass 2; two in a row (decrease reaches 4); a rejected FIRST
    # step; rejection - accepted step - rejection (decrease is back at 2); the far start that ends in the identity exit
    m = M("reject_pass1"); assert "R" in hp_pnp.trace_string(m).split("|")[0] and not m.identity
    m = M("reject_twice_pass1"); assert not m.identity and [t.decrease for t in m.trace1[1:3]] == [4.0, 8.0] and m.trace1[2].delta == m.trace1[1].delta / 2 and m.trace1[3].delta == m.trace1[2].delta / 4
    m = M("reject_both_passes"); assert "R" in hp_pnp.trace_string(m).split("|")[1] and not m.identity
    m = M("reject_accept_reject_pass2"); assert [t.accepted for t in m.trace2[4:8]] == [False, True, False, False] and [t.decrease for t in m.trace2[4:8]] == [4.0, 2.0, 4.0, 8.0]
    m = M("reject_first_step"); assert not m.trace1[0].accepted and np.array_equal(m.X1, m.X0) and float(m.pass1) == float(m.initial)
    m = M("reject_then_identity"); assert m.identity and m.n_outliers == 257
    # the gimbal starts are what they say: cos(theta2) of the start is below 1e-8 / exactly the rounded pi / 2
    for name in ("trip_theta2_plus_half_pi_n6", "trip_theta2_minus_half_pi_n65"):
        assert abs(abs(float(M(name).X0[1])) - np.pi / 2) < 1e-15, name
    assert abs(float(M("trip_theta2_below_half_pi_n6").X0[1]) - (np.pi / 2 - 1e-9)) < 1e-15


def test_every_mutant_is_rejected(orc, every_case):
    table = {}
    for f in np_pnp.FAULTS:
        hits = []
        for name, q in every_case.items():
            y = hp_pnp.yardsticks(orc, q)
            a, kw = hp_pnp.call_args(q)
            with np.errstate(all="ignore"):
                out = np_pnp.pnp_ba(*a, **kw, fault=f)
            if hp_pnp.rejected(f"{f}/{name}", out, y):
                hits.append(name)
        table[f] = hits
        print(f"mutant {f:2s}: rejected by {len(hits):3d} cases: {', '.join(hits[:6])}{' ...' if len(hits) > 6 else ''}")
    # and the unmutated restatement passes everywhere (it is one of the two yardsticks: by construction, at any k >= 1)
    for name, q in every_case.items():
        hp_pnp.check(name, hp_pnp.yardsticks(orc, q).out_np, hp_pnp.yardsticks(orc, q))
    assert all(table[f] for f in np_pnp.FAULTS), {f: len(v) for f, v in table.items()}
    named = lambda f: {c for c in table[f] if not c.startswith("small_")}
    assert named("b") == {"far_n6"}
    assert {"it5_10_n5", "inliers_5"} <= named("d")
    # ... and the same at ten times the asserted k: no mutant is anywhere near the bound
    k10 = {g: 10 * v for g, v in hp_pnp.K.items()}
    for f in np_pnp.FAULTS:
        a, kw = hp_pnp.call_args(every_case[table[f][0]])
        with np.errstate(all="ignore"):
            assert hp_pnp.rejected(f, np_pnp.pnp_ba(*a, **kw, fault=f), hp_pnp.yardsticks(orc, every_case[table[f][0]]), k10), f
    rej = {c for c in every_case if c.startswith("reject_")}
    # e, f, i2 act on the steps around a rejection (on the easy scenes rho ~ 1: 1 - (2 rho - 1)^3 and 1 - (2 rho - 1) are both below 1/3), and
    # a case that converges afterwards forgets them: reject_pass1 / reject_twice_pass1 end within rounding of the unmutated run
    assert named("f") == {"reject_accept_reject_pass2"}
    assert named("e") == named("i2") == rej - {"reject_pass1", "reject_twice_pass1"}


def test_model_sanity(syn):
    """the model's own pieces against independent arithmetic: the complex-step Jacobian against a central difference (1e-9 of the
    column's largest entry), one damped step against numpy.linalg.solve in f64 (1e-10 relative)"""
    q = hp_pnp.cases(syn)["it5_10_n65"]
    m = hp_pnp.Model(q["cam"], q["pixels_yx"], q["points"])
    X = hp_pnp.rotzyx_angles(q["pose0"])
    J = m.jacobian(X)
    h = hp_ba.LD(1e-7)
    for k in range(6):
        e = np.zeros(6, dtype=hp_ba.LD); e[k] = h
        fd = (m.residuals(X + e)[0] - m.residuals(X - e)[0]) / (2 * h)
        assert float(np.abs(fd - J[:, :, k]).max()) <= 1e-9 * float(np.abs(J[:, :, k]).max()), k
    st = m.step(X, np.ones(q["n"], bool), 10.0)
    Jf = J.reshape(-1, 6).astype(np.float64); r = m.residuals(X)[0].reshape(-1).astype(np.float64)
    H = Jf.T @ Jf
    dx = np.linalg.solve(H + np.diag(np.clip(np.diag(H), 1e-6, 1e32) / 10.0), Jf.T @ r)
    assert np.abs(dx - st["dx"].astype(np.float64)).max() <= 1e-10 * np.abs(dx).max()
    # the rotation the model returns is the rotation of the library's restatement, and the angles invert it
    R = hp_pnp.rotation(X)
    assert np.abs(R.astype(np.float64) - syn.rotzyx(*X[:3].astype(np.float64))).max() < 1e-15
    assert float(np.abs(hp_pnp.rotzyx_angles(hp_pnp.pose_of(X)) - X).max()) < 1e-17
