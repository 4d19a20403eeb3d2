"""CPU: the extended-precision model of one BA iteration (tests/hp_ba.py) against the two f64 implementations that exist on the host --
the C oracle (orc.ba_reduced_system, orc.bundle_adjustment with ONE iteration) and tests/np_ba.py -- on every window family of the GPU
stage tests (hp_ba.stage_windows).  Three things are established here, without a GPU, that make the GPU assertions trustworthy:

  * the model is right: both f64 implementations, written independently of it and of each other, agree with it to f64 rounding
    (bounds reasoned from the length of the sums and the conditioning of the damped system, below), and its shards add up;
  * the yardstick: E_orc and E_np, the error of honest f64 arithmetic on THIS window per quantity, from which the GPU bounds are
    taken (k * max(E_orc, E_np, 4 * 2^-52), k = hp_ba.K[stage]);
  * the sensitivity: deliberately damaged copies of the f64 outputs (never a kernel's) are REJECTED by the same assertion function
    (hp_ba.check) with the same bounds the GPU tests use.

Measures: hp_ba.build_errors / step_errors (scales come from the model only)."""
import numpy as np
import pytest

import hp_ba as hp

INV_DELTAS = (1.0 / hp.LM_DELTA0, 3.0, 1e-6)
NAMES = ("hb1", "hb9", "hb14", "hb15", "hb16", "hb17", "hb18", "hb20", "hb21_dense", "hb21_tiled", "p16", "p17", "p32", "loop",
         "const_first", "const_scattered", "const_most", "ragged")


@pytest.fixture(scope="module")
def windows(syn):
    w = hp.stage_windows(syn)
    assert tuple(w) == NAMES
    return w


_np_shard, build_yardsticks, step_yardsticks = hp.np_shard, hp.build_yardsticks, hp.step_yardsticks


# ---- the window families have the properties their names promise (not: trust the seed) ----
def test_window_properties(windows, syn):
    for hb in (1, 9, 14, 15, 16, 17, 18, 20):
        assert syn.ba_halfband(windows[f"hb{hb}"]) == hb
    for nm in ("hb21_dense", "hb21_tiled", "loop"):
        assert syn.ba_halfband(windows[nm]) > 20
    free_span = lambda s: np.ptp(np.flatnonzero(s["theta_const"] == 0)) + 1
    assert free_span(windows["hb21_dense"]) <= 30 < free_span(windows["hb21_tiled"])
    assert [6 * windows[f"p{P}"]["P"] for P in (16, 17, 32)] == [96, 102, 192]
    c = windows["const_scattered"]["theta_const"]
    assert c[0] and c[-1] and 0 < c[1:-1].sum() and (c[1:-1] == 0).any()
    assert (windows["const_most"]["theta_const"] == 1).sum() == 20 and windows["const_first"]["theta_const"][:6].all()
    s = windows["ragged"]; pr = s["props"]
    const = s["theta_const"].astype(bool)
    cnt = np.bincount(s["point_ids"] - 1, minlength=s["M"])
    assert cnt[pr["orphan"]] == 0 and all(cnt[j] == 1 for j in pr["singles"]) and len(pr["singles"]) == 3
    assert all(not const[s["pose_ids"][s["point_ids"] - 1 == j][0] - 1] for j in pr["singles"])
    assert len(pr["const_only"]) == 3 and all(cnt[j] >= 1 and const[s["pose_ids"][s["point_ids"] - 1 == j] - 1].all() for j in pr["const_only"])
    assert not const[pr["empty_pose"]] and not (s["pose_ids"] - 1 == pr["empty_pose"]).any()
    assert (np.diff(s["point_ids"]) < 0).any(), "observation order is not shuffled"
    assert const[0] and const[-1]


# ---- the model against the two f64 implementations: build ----
def _build_bound(s, inv_delta):
    """what an honest f64 build may differ from the model by (reasoning: test_model_build_vs_oracle_and_numpy)"""
    b = 8.0 * s["O"] * 2.0 ** -53
    return dict(S=b * (3 + inv_delta) / inv_delta, g=b * (3 + inv_delta) / inv_delta, ud=b, ssr=b)


@pytest.mark.parametrize("name", NAMES)
def test_model_build_vs_oracle_and_numpy(windows, orc, name):
    """Every accumulated quantity is a sum of at most O products of f64 numbers, formed in f64 by the oracle and by np_ba in their own
    orders: the error of such a sum is at most O * 2^-53 times the sum of the magnitudes, and the scales of the measures (ud for S,
    sqrt(ud ssr) for g: Cauchy-Schwarz) bound those magnitudes.  The inverse of the 3 x 3 point blocks and the residual's own rounding
    add a few units: 8 O 2^-53.  The Schur term goes through (V + D_l)^-1, whose error grows with the condition number of the damped
    point block: in Jacobi scaling its eigenvalues lie in [inv_delta, 3 + inv_delta] (a point with one observation has a singular V,
    so the lower end is reached: the `ragged` window at inv_delta = 1e-6), hence bound 8 O 2^-53 (3 + inv_delta) / inv_delta for S and
    g, 8 O 2^-53 for ud and ssr.  (Measured: 1e-15 .. 6e-15; `ragged` at inv_delta = 1e-6: 5e-12 in S.)"""
    s = windows[name]
    for inv_delta in INV_DELTAS:
        bound = _build_bound(s, inv_delta)
        _, e_orc, e_np, _, _ = build_yardsticks(orc, s, name, 0, inv_delta)
        print(f"yardstick build {name} inv_delta={inv_delta:g}: E_orc {e_orc}  E_np {e_np}")
        hp.check(f"oracle vs model, {name}, inv_delta {inv_delta}", e_orc, bound)
        hp.check(f"np_ba vs model, {name}, inv_delta {inv_delta}", e_np, bound)


def test_model_blocks_on_the_large_window(windows, orc, syn):
    """Model.build_blocks (the block-wise form used on the 50 key-frame / 1e5 observation window) equals Model.build on a small
    window to longdouble rounding, and the oracle agrees with it on the large window's sampled blocks (bound as above: a pose of that
    window has 2000 observations, the cost sums all 1e5)"""
    s = windows["ragged"]
    m = hp.Model(*hp.scene_args(s))
    mb = m.build_blocks(0, 0.1, [(1, 1), (1, 2), (2, 4), (9, 9), (3, 8), (0, 1), (7, 3)])
    hp.check("build_blocks vs build", hp.block_errors(m.build(0, 0.1), mb), dict.fromkeys(("S", "g", "ud", "ssr"), 64 * float(np.finfo(hp.LD).eps)))
    big, _, e_orc, _ = hp.big_yardsticks(orc, syn)
    print(f"yardstick build big: E_orc {e_orc}")
    assert big["O"] == 100000 and syn.ba_halfband(big) == 9
    hp.check("oracle vs model blocks, big", e_orc, _build_bound(big, 0.1))


@pytest.mark.parametrize("name", ("hb9", "ragged", "loop"))
def test_model_build_with_outlier_flags(windows, orc, name):
    """ignore_outliers = 1 with the model's own flags (repr_eps = 5 at theta0 flags a good part of the perturbed window)"""
    s = windows[name]
    m = hp.Model(*hp.scene_args(s))
    n_out = m.flag_outliers(5.0)
    ns = _np_shard(s)
    assert ns.flag_outliers(5.0) == n_out and np.array_equal(ns.outl, m.outl) and 0 < n_out < s["O"]
    _, e_orc, e_np, _, _ = build_yardsticks(orc, s, name, 1, 0.1, outl=m.outl)
    bound = _build_bound(s, 0.1)
    hp.check(f"oracle vs model, {name}, flagged", e_orc, bound)
    hp.check(f"np_ba vs model, {name}, flagged", e_np, bound)


@pytest.mark.parametrize("name", ("hb9", "ragged", "const_scattered", "loop"))
def test_model_shards_add_up(windows, orc, name):
    """the contributions of the point ranges [0, m) and [m, M) sum to the whole, in the model (to longdouble rounding) and each range
    agrees with the oracle's and np_ba's shard"""
    s = windows[name]
    m = hp.Model(*hp.scene_args(s))
    whole = m.build(0, 0.1)
    cut = s["M"] // 3
    parts = [m.build(0, 0.1, 0, cut), m.build(0, 0.1, cut, s["M"])]
    tot = {q: parts[0][q] + parts[1][q] for q in ("S", "g", "ud", "ssr")}
    e = hp.build_errors(tot, whole)
    hp.check(f"model shard additivity, {name}", e, dict.fromkeys(("S", "g", "ud", "ssr"), 64 * float(np.finfo(hp.LD).eps)))
    bound = _build_bound(s, 0.1)
    for lo, hi in ((0, cut), (cut, s["M"])):
        _, e_orc, e_np, _, _ = build_yardsticks(orc, s, name, 0, 0.1, None, lo, hi)
        hp.check(f"np_ba shard [{lo}, {hi}), {name}", e_np, bound)
        hp.check(f"oracle shard [{lo}, {hi}), {name}", e_orc, bound)


# ---- the model's full-system step against the two Schur-complement steps in f64 ----
@pytest.mark.parametrize("name", NAMES)
def test_model_step_vs_oracle_and_numpy(windows, orc, name):
    """The model solves the full damped normal equations (free poses and all points at once) by a dense Cholesky; the oracle and np_ba
    eliminate the points first.  In Jacobi scaling the damped matrix I + D^-1/2 J'J D^-1/2 / ... has its eigenvalues in
    [inv_delta / (1 + inv_delta), N]: condition number below 11 N at delta0 = 10 (N = 6 F + 3 M <= 700 here), so an f64 solve is
    good to about 11 N * N * 2^-53 ~ 5e-10 relative in the worst case: bound 1e-9 for the step, 1e-11 for the costs.
    (Measured: 1e-13 .. 5e-12.)"""
    s = windows[name]
    st, e_orc, e_np, _ = step_yardsticks(orc, s, name)
    print(f"yardstick step {name}: E_orc {e_orc}  E_np {e_np}")
    bound = dict(dp=1e-9, dl=1e-9, trial_ssr=1e-11, ssr=1e-11)
    hp.check(f"oracle one LM step vs model, {name}", e_orc, bound)
    hp.check(f"np_ba solve vs model, {name}", e_np, dict(bound, predicted_ssr=1e-11, maxdx=1e-9))


def test_model_two_lm_steps_vs_oracle_and_numpy(windows, orc):
    """the LM rule restated in the model (accept, delta update from rho) against two iterations of the oracle and of np_ba under the
    same rule; bound as for one step"""
    for name in ("hb9", "const_most"):
        ref, e_orc, e_np = hp.lm2_yardsticks(orc, windows[name], name)
        print(f"yardstick two LM steps {name}: E_orc {e_orc}  E_np {e_np}")
        hp.check(f"oracle, two LM steps, {name}", e_orc, dict(dp=1e-9, dl=1e-9, trial_ssr=1e-11, ssr=1e-11))
        hp.check(f"np_ba, two LM steps, {name}", e_np, dict(dp=1e-9, dl=1e-9, trial_ssr=1e-11))


# ---- sensitivity: damaged copies of the f64 outputs must be rejected by the assertion the GPU tests use ----
def _blocks_of_point(ns, j):
    """np_ba's f64 Schur terms of point j: observations a, b of the point contribute -T_a W_b' to block (pose a, pose b)"""
    obs = np.flatnonzero(ns.li == j)
    T = np.einsum("oab,obc->oac", ns.Wm[obs], ns.Vi[ns.li[obs]])
    return obs, T


def test_sensitivity_build(windows, orc):
    """a build that is subtly wrong in ONE block fails hp.check at k = hp.K['build']"""
    s = windows["hb1"]                                           # every point is seen by two consecutive poses
    b, e_orc, e_np, o, ns = build_yardsticks(orc, s, "hb1", 0, 0.1)
    bound = hp.bounds(hp.K["build"], e_orc, e_np)
    hp.check("undamaged oracle build", hp.build_errors(o, b), bound)
    free = ~s["theta_const"].astype(bool)
    j = next(j for j in range(s["M"]) if free[ns.pi[ns.li == j]].all() and (ns.li == j).sum() == 2)
    obs, T = _blocks_of_point(ns, j)
    p, q = ns.pi[obs[0]], ns.pi[obs[1]]
    term = T[0] @ ns.Wm[obs[1]].T                                # what point j subtracts from S_pq
    blk = lambda A, p, q: A[6 * p:6 * p + 6, 6 * q:6 * q + 6]
    # 1. one observation pair's contribution dropped from one off-diagonal block (both triangles: S stays symmetric)
    d = dict(o, S=o["S"].copy()); blk(d["S"], p, q)[:] += term; blk(d["S"], q, p)[:] += term.T
    with pytest.raises(AssertionError, match="S ="):
        hp.check("dropped contribution", hp.build_errors(d, b), bound)
    # 2. one off-diagonal block transposed (both triangles)
    d = dict(o, S=o["S"].copy()); blk(d["S"], p, q)[:] = blk(o["S"], p, q).T; blk(d["S"], q, p)[:] = blk(o["S"], q, p).T
    with pytest.raises(AssertionError, match="S ="):
        hp.check("transposed block", hp.build_errors(d, b), bound)
    # 3. the Schur term of g dropped for one point seen by two poses
    d = dict(o, g=o["g"].copy())
    for a in range(2):
        d["g"][6 * ns.pi[obs[a]]:6 * ns.pi[obs[a]] + 6] += T[a] @ ns.bl[j]
    with pytest.raises(AssertionError, match="g ="):
        hp.check("g without one point's Schur term", hp.build_errors(d, b), bound)
    # and the plain ones: one entry of ud, the cost
    d = dict(o, ud=o["ud"].copy()); d["ud"][6 * p] *= 1 + 1e-12
    with pytest.raises(AssertionError, match="ud ="):
        hp.check("ud off by 1e-12", hp.build_errors(d, b), bound)
    d = dict(o, S=o["S"].copy()); d["S"][0, 6 * int(np.flatnonzero(free)[0])] = 1e-300       # a constant pose's row must be exactly zero
    with pytest.raises(AssertionError, match="S ="):
        hp.check("non-zero in a constant pose's row", hp.build_errors(d, b), bound)


def test_sensitivity_solve(windows, orc):
    """a step that is subtly wrong in ONE pose's damping, ONE point's back-substitution or in the predicted cost fails hp.check at
    k = hp.K['solve'] and k = hp.K['step']"""
    s = windows["ragged"]
    st, e_orc, e_np, xn = step_yardsticks(orc, s, "ragged")
    P, n = s["P"], 6 * s["P"]
    for stage in ("solve", "step"):
        bound = hp.bounds(hp.K[stage], e_orc, e_np)
        hp.check("undamaged np_ba step", hp.step_errors(xn, st, P), bound)
        # 4. the damping of one pose scaled by 1 + 1e-6: the diagonal handed to np_ba's solve
        ns = _np_shard(s)
        red = ns.build(0, 0.1).clone()
        p = int(np.flatnonzero(s["theta_const"] == 0)[2])
        red[n * n + n + 6 * p:n * n + n + 6 * p + 6] *= 1 + 1e-6
        tr = ns.solve(red, 0.1).numpy().copy(); ns.commit(1)
        d = dict(dx=s["theta0"] - ns.download()[0], trial_ssr=tr[0], predicted_ssr=tr[1], maxdx=tr[2])
        with pytest.raises(AssertionError, match="dp ="):
            hp.check("one pose's damping scaled", hp.step_errors(d, st, P), bound)
        # 5. dl of one single-observation point left at zero
        j = s["props"]["singles"][0]
        d = dict(xn, dx=xn["dx"].copy()); d["dx"][n + 3 * j:n + 3 * j + 3] = 0
        with pytest.raises(AssertionError, match="dl ="):
            hp.check("one point not back-substituted", hp.step_errors(d, st, P), bound)
        # 6. predicted_ssr replaced by trial_ssr
        d = dict(xn, predicted_ssr=xn["trial_ssr"])
        with pytest.raises(AssertionError, match="predicted_ssr ="):
            hp.check("predicted cost = trial cost", hp.step_errors(d, st, P), bound)
