"""GPU parity: slam_local_ba / slam_pnp_ba vs the CPU oracle's Schur-LM (same
algorithm: tolerances below) and vs the reference-style LM+LSMR restatement
(cross-algorithm: final cost within 1e-3 relative)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL_THETA = 1e-6
RTOL_SSR = 1e-8


def _run(slam, orc, s, iters_fast=5, iterations=10, repr_eps=5.0):
    cache = slam.LocalBACache(s["theta0"].copy(), s["theta_const"], s["pixels_yx"], s["pose_ids"], s["point_ids"])
    slam.bundle_adjustment_(cache, s["cam"], iterations=iterations, repr_eps=repr_eps, iters_fast=iters_fast)
    th, ol, st = orc.bundle_adjustment(s["cam"], s["theta0"], s["theta_const"], s["pixels_yx"], s["pose_ids"], s["point_ids"],
                                       iters_fast, iterations, repr_eps, solver=1)
    return cache, th, ol, st


def _check_recall(outliers, s):
    """The injected wrong associations (4-12 px off, synthetic.ba_scene) are flagged by pass 1 (bundle_adjustment.jl:90-111)."""
    go = s["gross_outliers"]
    assert len(go) > 0
    assert outliers[go].mean() >= 0.95, outliers[go].mean()    # small windows can absorb a 4-px error of a 2-view point
    clean = np.ones(len(outliers), bool); clean[go] = False
    assert outliers[clean].mean() < 0.03                          # 0.5-px noise: squared error > 5 is a > 3-sigma event


@pytest.mark.parametrize("P,M,seed", [(5, 300, 0), (8, 600, 1), (20, 2000, 2)])
def test_local_ba_matches_oracle_schur(slam, orc, syn, P, M, seed):
    s = syn.ba_scene(P=P, M=M, seed=seed)
    cache, th, ol, st = _run(slam, orc, s)
    assert np.array_equal(cache.outliers, ol)
    assert cache.stats["n_outliers"] == st["n_outliers"]
    assert cache.stats["iters_pass1"] == st["iters_pass1"] and cache.stats["iters_pass2"] == st["iters_pass2"]
    for k in ("ssr_init", "ssr_pass1", "ssr_final"):
        assert abs(cache.stats[k] - st[k]) <= RTOL_SSR * st[k], k
    assert np.abs(cache.theta - th).max() <= RTOL_THETA * max(1.0, np.abs(th).max())
    # constant poses never move (bundle_adjustment.jl:77)
    c = s["theta_const"].astype(bool)
    assert np.array_equal(cache.theta[:6 * P].reshape(P, 6)[c], s["theta0"][:6 * P].reshape(P, 6)[c])
    # recovers ground truth within noise, flags the injected gross outliers
    assert np.abs(cache.theta[:6 * P] - s["theta_gt"][:6 * P]).max() < 0.05
    _check_recall(cache.outliers, s)


@pytest.mark.parametrize("P,M,opp,n_const", [(26, 1500, 24, 1), (30, 1200, 28, 2), (24, 900, 23, 1), (27, 700, 25, 5)])
def test_windows_no_pose_order_makes_banded_take_the_dense_solver(slam, orc, syn, P, M, opp, n_const):
    """every map point seen by (almost) every key-frame: half-bandwidth > 20 in any order -> point groups over the whole block triangle +
    k_dense_solve (one workgroup, lower triangle in LDS) instead of pair lists + the tiled Cholesky; same answers as the oracle's Schur-LM"""
    s = syn.ba_scene(P=P, M=M, seed=40 + P, obs_per_point=opp, n_const=n_const)
    cache, th, ol, st = _run(slam, orc, s)
    assert np.array_equal(cache.outliers, ol)
    assert cache.stats["iters_pass1"] == st["iters_pass1"] and cache.stats["iters_pass2"] == st["iters_pass2"]
    for k in ("ssr_init", "ssr_pass1", "ssr_final"):
        assert abs(cache.stats[k] - st[k]) <= RTOL_SSR * st[k], k
    assert np.abs(cache.theta - th).max() <= RTOL_THETA * max(1.0, np.abs(th).max())
    c = s["theta_const"].astype(bool)
    assert np.array_equal(cache.theta[:6 * P].reshape(P, 6)[c], s["theta0"][:6 * P].reshape(P, 6)[c])


def test_local_ba_vs_reference_style_lsmr(slam, orc, syn):
    s = syn.ba_scene(P=6, M=500, seed=3)
    cache, th, ol, st = _run(slam, orc, s)
    th0, ol0, st0 = orc.bundle_adjustment(s["cam"], s["theta0"], s["theta_const"], s["pixels_yx"], s["pose_ids"], s["point_ids"], solver=0)
    assert abs(cache.stats["ssr_final"] - st0["ssr_final"]) <= 1e-3 * st0["ssr_final"]
    assert (cache.outliers != ol0).mean() < 0.01
    assert np.abs(cache.theta[:36] - th0[:36]).max() < 1e-3


def test_local_ba_edge_cases(slam, orc, syn):
    # all poses constant -> only points move; zero iterations -> theta unchanged, outliers flagged at theta0
    s = syn.ba_scene(P=4, M=100, seed=4, n_const=4)
    cache, th, ol, st = _run(slam, orc, s)
    assert np.array_equal(cache.theta[:24], s["theta0"][:24])
    assert np.abs(cache.theta - th).max() <= 1e-6
    s = syn.ba_scene(P=4, M=100, seed=5)
    cache, th, ol, st = _run(slam, orc, s, iters_fast=0, iterations=0)
    assert np.array_equal(cache.theta, s["theta0"]) and np.array_equal(cache.outliers, ol)
    # shuffled observation order gives the same answer (device re-orders by point internally)
    s = syn.ba_scene(P=5, M=200, seed=6)
    perm = np.random.default_rng(0).permutation(s["O"])
    s2 = dict(s); s2["pixels_yx"] = s["pixels_yx"][perm]; s2["pose_ids"] = s["pose_ids"][perm]; s2["point_ids"] = s["point_ids"][perm]
    c1, *_ = _run(slam, orc, s); c2, th2, ol2, _ = _run(slam, orc, s2)
    assert np.array_equal(c2.outliers, ol2)
    assert np.abs(c1.theta - c2.theta).max() < 1e-7
    with pytest.raises(slam.SlamHipError):
        bad = dict(s); bad["pose_ids"] = s["pose_ids"].copy(); bad["pose_ids"][0] = 99
        _run(slam, orc, bad)


def test_pnp_ba_matches_oracle(slam, orc, syn):
    """the END of a converged run on an easy scene (every LM step accepted) against the oracle: a parity smoke test.  Its 1e-8 / 1e-9 bars are
    ~ 1e7 times the f64 error; the accuracy test of the refinement, stage by stage and at rounding level, is test_gpu_pnp_model.py."""
    for seed in range(3):
        s = syn.pnp_scene(n=300, seed=seed)
        pose, e0, e1, ol, no = slam.pnp_bundle_adjustment(s["cam"], s["pose0"], s["pixels_yx"], s["points"], repr_eps=3.0)
        rp, r0, r1, rol, rno = orc.pnp_ba(s["cam"], s["pose0"], s["pixels_yx"], s["points"], repr_eps=3.0)
        assert np.array_equal(ol, rol) and no == rno
        assert abs(e0 - r0) <= 1e-9 * r0 and abs(e1 - r1) <= 1e-8 * r1
        assert np.abs(pose - rp).max() <= 1e-8
        assert np.abs(pose - s["pose_gt"]).max() < 0.02 and e1 < e0


def test_pnp_ba_identity_sentinel(slam, orc, syn):
    s = syn.pnp_scene(n=6, seed=1, outlier_frac=0.0)
    px = s["pixels_yx"].copy(); px[:4] += 300.0                                # only 2 inliers can remain
    pose, e0, e1, ol, no = slam.pnp_bundle_adjustment(s["cam"], s["pose0"], px, s["points"], repr_eps=3.0)
    rp, r0, r1, rol, rno = orc.pnp_ba(s["cam"], s["pose0"], px, s["points"], repr_eps=3.0)
    assert no == rno and np.array_equal(ol, rol)
    assert len(px) - rno < 5                                                    # the identity exit IS taken
    assert np.array_equal(pose, np.eye(4)) and np.array_equal(rp, np.eye(4))   # bundle_adjustment.jl:157-161
    # the mirror: one inlier above the exit (7 points, 2 displaced: exactly five remain) is refined
    s = syn.pnp_scene(n=7, seed=1, outlier_frac=0.0)
    px = s["pixels_yx"].copy(); px[:2] += 300.0
    pose, e0, e1, ol, no = slam.pnp_bundle_adjustment(s["cam"], s["pose_gt"], px, s["points"], repr_eps=9.0, iters_fast=0)
    rp, r0, r1, rol, rno = orc.pnp_ba(s["cam"], s["pose_gt"], px, s["points"], repr_eps=9.0, iters_fast=0)
    assert no == rno == 2 and np.array_equal(ol, rol) and len(px) - rno == 5
    assert not np.array_equal(pose, np.eye(4)) and np.abs(pose - rp).max() <= 1e-8


@pytest.mark.parametrize("P,M", [(50, 10000), (100, 40000)])
def test_local_ba_at_baseline_window_sizes(slam, orc, syn, P, M):
    """BASELINE.json's own BA sizes: the metric's 50-KF window (O = 1e5, configs[3]) and the 100-KF / O = 4e5 window of
    configs[4], against the oracle's Schur-LM with the bars of the small windows."""
    s = syn.ba_scene(P=P, M=M, seed=P)
    assert s["O"] == 10 * M
    cache, th, ol, st = _run(slam, orc, s)
    assert np.array_equal(cache.outliers, ol)
    assert cache.stats["n_outliers"] == st["n_outliers"]
    assert cache.stats["iters_pass1"] == st["iters_pass1"] and cache.stats["iters_pass2"] == st["iters_pass2"]
    for k in ("ssr_init", "ssr_pass1", "ssr_final"):
        assert abs(cache.stats[k] - st[k]) <= RTOL_SSR * st[k], k
    assert np.abs(cache.theta - th).max() <= RTOL_THETA * max(1.0, np.abs(th).max())
    _check_recall(cache.outliers, s)


def test_local_ba_vs_reference_style_lsmr_20kf(slam, orc, syn):
    """configs[2]'s 20-KF window against the reference-style solver (LM + LSMR on the full Jacobian, inexact steps)."""
    s = syn.ba_scene(P=20, M=2000, seed=20)
    cache, th, ol, st = _run(slam, orc, s)
    th0, ol0, st0 = orc.bundle_adjustment(s["cam"], s["theta0"], s["theta_const"], s["pixels_yx"], s["pose_ids"], s["point_ids"], solver=0)
    assert abs(cache.stats["ssr_final"] - st0["ssr_final"]) <= 1e-3 * st0["ssr_final"]
    assert (cache.outliers != ol0).mean() < 0.01
    assert np.abs(cache.theta[:120] - th0[:120]).max() < 1e-3
    _check_recall(cache.outliers, s)


@pytest.mark.parametrize("P,M", [(50, 10000), (100, 40000)])
def test_local_ba_vs_reference_style_lsmr_at_the_baseline_windows(slam, orc, syn, P, M):
    """The metric's 50-KF window and configs[4]'s 100-KF window against the reference-style solver -- LM + LSMR on the full Jacobian with
    the reference's 5 + 10 iterations (bundle_adjustment.jl:35-54) -- at the cross-algorithm bar of the small windows: final cost within
    1e-3 relative (the Schur-LM takes exact steps, LSMR with btol = 0.5 inexact ones), outlier sets within 1 %."""
    s = syn.ba_scene(P=P, M=M, seed=P)
    cache = slam.LocalBACache(s["theta0"].copy(), s["theta_const"], s["pixels_yx"], s["pose_ids"], s["point_ids"])
    slam.bundle_adjustment_(cache, s["cam"], iterations=10, iters_fast=5)
    th0, ol0, st0 = orc.bundle_adjustment(s["cam"], s["theta0"], s["theta_const"], s["pixels_yx"], s["pose_ids"], s["point_ids"], 5, 10, 5.0, solver=0)
    rel = abs(cache.stats["ssr_final"] - st0["ssr_final"]) / st0["ssr_final"]
    assert rel <= 1e-3, rel
    assert cache.stats["ssr_final"] <= st0["ssr_final"] * (1 + 1e-3)
    assert (cache.outliers != ol0).mean() < 0.01
    _check_recall(cache.outliers, s)


def test_twisted_solve_with_the_sides_on_different_xcds():
    """The banded solve's two workgroups normally share an XCD (launch of nine, sides = workgroups 0 and 8) and hand data to each
    other through the common L2 without agent-scope fences; each side checks the other's XCC_ID and falls back to the agent-scope
    path otherwise.  SLAMHIP_TWIST_SPREAD=1 launches the two sides as neighbouring workgroups (different XCDs): the fallback must give
    bit-identical parameters (the env is read once per process: a child process each)."""
    import os, subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import sys, hashlib, numpy as np
        sys.path.insert(0, %r)
        import slam_jl_amd as slam
        from slam_jl_amd import synthetic as syn
        out = []
        for P, M in ((50, 10000), (31, 1500)):
            s = syn.ba_scene(P=P, M=M, seed=3)
            for _ in range(3):
                c = slam.LocalBACache(s["theta0"].copy(), s["theta_const"], s["pixels_yx"], s["pose_ids"], s["point_ids"])
                slam.bundle_adjustment_(c, s["cam"])
                out.append(hashlib.sha256(c.theta.tobytes() + c.outliers.tobytes()).hexdigest() + repr(c.stats["ssr_final"]))
        print("RESULT", *out)
    """ % root)
    res = {}
    for spread in (False, True):
        env = dict(os.environ)
        env.pop("SLAMHIP_TWIST_SPREAD", None)
        if spread: env["SLAMHIP_TWIST_SPREAD"] = "1"
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        res[spread] = [l for l in p.stdout.splitlines() if l.startswith("RESULT")][0]
    assert res[False] == res[True]
    toks = res[False].split()[1:]
    assert toks[0] == toks[1] == toks[2] and toks[3] == toks[4] == toks[5]      # and each repeat gives the same bits
