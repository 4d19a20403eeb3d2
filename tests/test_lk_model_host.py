"""CPU: the long-double model of the tracking path (tests/hp_lk.py) against the C oracle (oracle/orc_lk.c), point for point, on the
oracle's own planes -- every case, window and prior mode of the GPU point tests (test_gpu_lk_model.py).  Established here, without a
GPU:

  * the oracle is right where it can be told: fate equal on every point that is not excused (decision margin > 1e-6), in both
    summation orders, at most 1 % of a case's points excused, positions within 1e-12 px of the model (measured: E_seq / E_wave are
    printed per case; run with -s);
  * the yardsticks E_seq / E_wave from which the GPU bounds are taken: K * max(E_seq, E_wave, ulp(max(H, W)));
  * the sensitivity: damaged oracle runs and damaged copies of its output are REJECTED by hp_lk.check, the assertion function the GPU
    tests use, at the same K."""
import numpy as np
import pytest

import hp_lk as hp

_WORLD = {}


def world(orc, syn, shape):
    """frames, points, oracle pyramids and their planes of one shape; models per (stream, window) are added on demand"""
    if shape not in _WORLD:
        frs = hp.frames(syn, shape)
        w = dict(frs=frs, pts=hp.points(orc, shape, frs), models={})
        w["pa"] = [orc.pyr_build(hp.as_f64(f["a"]), 3, 1.0, 1) for f in frs]
        w["pb"] = [orc.pyr_build(hp.as_f64(f["b"]), 3, 1.0, 1) for f in frs]
        w["A"] = [hp.planes_of(p) for p in w["pa"]]
        w["B"] = [hp.planes_of(p) for p in w["pb"]]
        _WORLD[shape] = w
    return _WORLD[shape]


def model_of(w, s, window, key="B"):
    k = (s, window, key)
    if k not in w["models"]:
        w["models"][k] = hp.Model(w["A"][s], w[key][s], window, 1.0)
    return w["models"][k]


def test_planes_round_trip(orc, syn):
    """Planes.to_oracle gives the oracle the model's planes bit for bit (the GPU tests feed both from downloaded planes this way)"""
    w = world(orc, syn, "odd")
    p = w["A"][1].to_oracle(orc)
    assert [w["pa"][1].plane("layers", l).shape for l in range(4)] == [(93, 131), (47, 66), (24, 33), (12, 17)]
    for n in hp.PLANES:
        assert np.array_equal(getattr(p, n), getattr(w["pa"][1], n))


@pytest.mark.parametrize("mode", hp.MODES)
@pytest.mark.parametrize("window", hp.WINDOWS)
@pytest.mark.parametrize("shape", list(hp.SHAPES))
def test_oracle_vs_model(orc, syn, shape, window, mode):
    w = world(orc, syn, shape)
    HW = hp.SHAPES[shape]
    levels3d = hp.mode_levels(mode)[0]
    pr = hp.priors(shape, w["frs"], w["pts"], window, mode)
    mod = hp.concat([model_of(w, s, window).matching(w["pts"][s], pr[s][0], pr[s][1], HW, 3, levels3d) for s in range(hp.S)])
    E = []
    for order in (0, 1):
        got = hp.concat([hp.oracle_matching(orc, w["pa"][s], w["pb"][s], w["pts"][s], pr[s][0], pr[s][1], HW, window, 3, levels3d, order)
                         for s in range(hp.S)])
        e, nex = hp.check(mod, got, 0.0, 0.0, HW, hp.E_ORACLE_MAX, (shape, window, mode, order))
        assert e <= hp.E_ORACLE_MAX
        E.append(e)
    n = len(mod["fate"])
    print(f"\n{shape} w{window} {mode}: n={n} excused={nex} min margin={mod['margin'].min():.2e} tracked={(mod['fate'] == 1).sum()} "
          f"kept as is={(mod['fate'] == 2).sum()} E_seq={E[0]:.2e} E_wave={E[1]:.2e}")
    assert (mod["fate"] == 2).sum() >= 1                               # the in_image gate is exercised
    if mode != "l0x3":
        assert (mod["fate"] == 1).mean() > 0.3
    # the per-point-displacement form (fb_tracking! with `displacement`) on streams 0 and 3
    disp = {s: (1.0 / 2.0 ** levels3d) * (pr[s][1] - w["pts"][s]) for s in (0, 3)}
    m = hp.concat([model_of(w, s, window).fb_tracking(w["pts"][s], disp[s], levels3d) for s in (0, 3)])
    for order in (0, 1):
        got = hp.concat([hp.oracle_fb(orc, w["pa"][s], w["pb"][s], w["pts"][s], disp[s], window, levels3d, order) for s in (0, 3)])
        hp.check(m, got, 0.0, 0.0, HW, hp.E_ORACLE_MAX, (shape, window, mode, "fb", order))
    # the oracle's own protocol restatement (pyramid_levels_3d = 1 is built into it)
    if mode == "l1":
        refs = [orc.optical_flow_matching(w["pa"][s], w["pb"][s], w["pts"][s], pr[s][0], pr[s][1], HW, window_size=window, sum_order=1)
                for s in range(hp.S)]
        got = hp.concat([hp.result(np.where(r["updated"], 1, np.where(r["removed"], 0, 2)), r["new_pixels"]) for r in refs])
        hp.check(mod, got, 0.0, 0.0, HW, hp.E_ORACLE_MAX, (shape, window, "protocol"))


def test_stereo_case(orc, syn):
    """even, window 9, disparity 6.3, epipolar_error 2.0, undistortion the identity"""
    shape, window = "even", 9
    w = world(orc, syn, shape)
    HW = hp.SHAPES[shape]
    if "R" not in w:
        w["pr"] = [orc.pyr_build(hp.as_f64(f["r"]), 3, 1.0, 1) for f in w["frs"]]
        w["R"] = [hp.planes_of(p) for p in w["pr"]]
    pr = hp.priors(shape, w["frs"], w["pts"], window, "l1", seed=1, shift=(0.0, -hp.DISPARITY))
    models = [hp.Model(w["B"][s], w["R"][s], window, 1.0) for s in range(hp.S)]
    mod = hp.concat([models[s].matching(w["pts"][s], pr[s][0], pr[s][1], HW, 3, 1, stereo=True, undistorted_left=w["pts"][s]) for s in range(hp.S)])
    for order in (0, 1):
        got = hp.concat([hp.oracle_matching(orc, w["pb"][s], w["pr"][s], w["pts"][s], pr[s][0], pr[s][1], HW, window, 3, 1, order, stereo=True)
                         for s in range(hp.S)])
        e, nex = hp.check(mod, got, 0.0, 0.0, HW, hp.E_ORACLE_MAX, ("stereo", order))
        print(f"\nstereo order {order}: n={len(mod['fate'])} excused={nex} matched={(mod['fate'] == 1).sum()} removed={(mod['fate'] == 0).sum()} E={e:.2e}")
    assert (mod["fate"] == 1).mean() > 0.3 and (mod["fate"] == 0).sum() >= 1 and (mod["fate"] == 2).sum() >= 1


# ---- sensitivity: every damaged run must be rejected by the assertion the GPU tests use ----
@pytest.fixture(scope="module")
def victim(orc, syn):
    """even, window 9, priors at level 1, stream 0: the model, the honest yardsticks, and a tracked point that is not excused"""
    shape, window, s = "even", 9, 0
    w = world(orc, syn, shape)
    pr = hp.priors(shape, w["frs"], w["pts"], window, "l1")[s]
    mod = model_of(w, s, window).matching(w["pts"][s], pr[0], pr[1], hp.SHAPES[shape], 3, 1)
    run = lambda pa, pb, win=window, order=1: hp.oracle_matching(orc, pa, pb, w["pts"][s], pr[0], pr[1], hp.SHAPES[shape], win, 3, 1, order)
    honest = run(w["pa"][s], w["pb"][s])
    E_seq, E_wave = hp.measure(mod, run(w["pa"][s], w["pb"][s], order=0)), hp.measure(mod, honest)
    ok = np.flatnonzero((mod["fate"] == 1) & ~hp.excused(mod) & (w["pts"][s][:, 0] > 30) & (w["pts"][s][:, 0] < 90))
    hp.check(mod, honest, E_seq, E_wave, hp.SHAPES[shape], hp.CAP_TOL)          # the honest run passes
    return dict(w=w, s=s, mod=mod, run=run, honest=honest, E=(E_seq, E_wave), i=int(ok[0]), shape=hp.SHAPES[shape])


def _rejected(v, got):
    with pytest.raises(AssertionError):
        hp.check(v["mod"], got, v["E"][0], v["E"][1], v["shape"], hp.CAP_TOL)


def _copy_pyr(orc, p):
    q = orc.Pyramid(p.H0, p.W0, p.levels)
    for n in hp.PLANES:
        getattr(q, n)[...] = getattr(p, n)
    return q


def test_damage_one_target_pixel(orc, victim):
    v = victim; w, s = v["w"], v["s"]
    q = _copy_pyr(orc, w["pb"][s])
    y, x = np.rint(v["mod"]["pos"][v["i"]].astype(np.float64)).astype(int)
    q.plane("layers", 0)[y - 1, x - 1] += 2.0 ** -20
    _rejected(v, v["run"](w["pa"][s], q))


@pytest.mark.parametrize("level", [0, 1])
def test_damage_swapped_template_gradients(orc, victim, level):
    v = victim; w, s = v["w"], v["s"]
    q = _copy_pyr(orc, w["pa"][s])
    iy, ix = q.plane("Iy", level).copy(), q.plane("Ix", level).copy()
    q.plane("Iy", level)[...] = ix; q.plane("Ix", level)[...] = iy
    _rejected(v, v["run"](q, w["pb"][s]))


def test_damage_status_cleared(victim):
    v = victim
    got = {k: a.copy() for k, a in v["honest"].items()}
    got["fate"][v["i"]] = 0
    _rejected(v, got)


def test_damage_position_moved(victim):
    v = victim
    got = {k: a.copy() for k, a in v["honest"].items()}
    got["pos"][v["i"], 1] += 1e-9
    _rejected(v, got)


@pytest.mark.parametrize("dw", [-1, 1])
def test_damage_window_off_by_one(victim, dw):
    v = victim; w, s = v["w"], v["s"]
    _rejected(v, v["run"](w["pa"][s], w["pb"][s], win=9 + dw))


# ---- the model's 2 x 2 algebra against numpy ----
def test_svd_and_pinv_vs_numpy():
    rng = np.random.default_rng(4)
    tol = float(hp.SQRT_EPS)
    mats = [rng.normal(size=(2, 2)) * 10.0 ** rng.integers(-3, 4) for _ in range(40)]
    for u in rng.normal(size=(10, 2)):
        mats.append(np.outer(u, u) * 37.0)                               # rank 1, symmetric
        mats.append(np.outer(u, rng.normal(size=2)))                      # rank 1, general
    mats += [np.zeros((2, 2)), np.diag([3.0, 0.0]), np.diag([0.0, -2.0]), np.diag([5.0, 1e-9]), np.array([[2.0, -1.0], [-1.0, 0.5]])]
    for M in mats:
        U, S, V = hp.svd2x2(M)
        sn = np.linalg.svd(M, compute_uv=False)
        scale = max(sn[0], 1e-300)
        assert np.abs(np.asarray(U @ np.diag(S) @ V.T, dtype=np.float64) - M).max() <= 1e-15 * scale
        assert np.abs(np.asarray(S, dtype=np.float64) - sn).max() <= 1e-15 * scale
        # numpy's cutoff is relative to the largest singular value: hand it pinv2x2's absolute one
        ref = np.linalg.pinv(M, rcond=tol / scale) if sn[0] > tol else np.zeros((2, 2))
        near = sn[(sn > 0.5 * tol) & (sn < 2 * tol)]
        assert len(near) == 0
        pscale = max(np.abs(ref).max(), 1e-300)
        kappa = sn[0] / sn[sn > tol].min() if (sn > tol).any() else 1.0
        # utils.jl:44 multiplies U * D * V': the TRANSPOSE of the pseudo-inverse V * D * U' -- the same matrix for the symmetric G it
        # is applied to
        assert np.abs(np.asarray(hp.pinv2x2(M), dtype=np.float64) - ref.T).max() <= 1e-14 * kappa * pscale
        if np.array_equal(M, M.T):
            Gi, Ss = hp.pinv_sym2x2(M[0, 0], M[0, 1], M[1, 1])
            assert np.abs(np.asarray(Gi, dtype=np.float64) - ref).max() <= 1e-14 * kappa * pscale
            assert np.abs(np.array(Ss, dtype=np.float64) - sn).max() <= 1e-15 * scale
