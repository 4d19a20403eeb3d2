"""GPU: what ONE iteration of the bundle adjustment computes, stage by stage, against the extended-precision model (tests/hp_ba.py).

Every other GPU test of the BA looks at the end of a converged LM run, which forgives its own linear algebra.  Here:

  (a) build   HipShard.build -> the buffer [S ; g ; diag(Jp'Jp) ; ssr] against the model's S = U - W (V + D_l)^-1 W', g, ud, ssr.
              The buffer's pose order is the CALLER's: slam_ba_create calls ba_setup with may_reorder = false (only slam_local_ba and
              the batch relabel poses), so no mapping is needed; the loop-closure window is ALSO run relabelled by the test itself
              through slam_ba_plan_order ("loop_planned").  S must be symmetric, exactly zero outside the band slam_ba_halfband
              reports and in the rows / columns of constant poses.
  (b) solve   HipShard.solve + commit(1) + download: the new theta (poses AND points) against the model's step from the FULL damped
              normal equations, the trial block (trial_ssr, predicted_ssr, max|dx|) against the model's.  The same solve fed with the
              MODEL's reduced system rounded to f64 tells a solve error from a build error in the failure message.
  (c) step    slam_local_ba and slam_local_ba_batch with iters_fast = 1 (and 2), iterations = 0: theta, ssr_init, ssr_pass1 and the
              outlier flags against the model's accepted step(s).

Bounds: k * max(E_orc, E_np, 4 * 2^-52) per measure (hp_ba.build_errors / step_errors; scales from the model only), E_orc / E_np the
same measure of the C oracle and of np_ba.py on the same window, computed inside the test; k = hp_ba.K[stage] = 4 x the largest
measured r = E_hip / max(E_orc, E_np, 4 * 2^-52) of the stage.  Every case prints its r (lines "STAGE_R ..."; run with -s).
With outlier flags (ignore_outliers = 1) the oracle has no one-iteration entry point: the step's yardstick is np_ba's alone.

Paths and the windows that reach them (hp_ba.stage_windows; P poses, hb = block half-bandwidth; `ba_plan` / `ba_enqueue_solve`):
  k_schur_groups + k_schur_reduce (grouped build)       every window with hb <= BS_MAXHB = 20, and hb21_dense / loop (hb 21 / 22 with
                                                        <= DS_MAXF = 30 free poses in a row: `dense_ok`)
  ungrouped build (k_linearize / k_points /             hb21_tiled (hb 21, 33 free poses: neither banded nor dense), and every window
    k_obs_factors / k_blocks; k_backsub / k_trial)      of the child process with SLAMHIP_NO_GROUPS=1
  k_band_solve on one workgroup                         hb14 .. hb20 (6 hb > 58: no twist), p16 / p17 / const_most / ragged (fewer
                                                        free poses in a row than max(2 hb + 1, hb + 8)); hb1 / hb9 with SLAMHIP_NO_TWIST=1
  k_band_solve twisted on two workgroups                hb1 (11 free poses, hb 1), hb9 (29, hb 9), p32 (31, hb 4), const_first (14, hb 7),
                                                        const_scattered (18 in the span, hb 7: pspan < P at both ends); the same with
                                                        SLAMHIP_TWIST_SPREAD=1 (the two sides on different XCDs)
  k_dense_solve                                         hb21_dense (29 free poses), loop in caller order (hb 22, 23 free poses)
  tiled chain k_chol_prepare / _first / _step / _backsolve   hb21_tiled (too wide for the band, too long for the dense solver), and
                                                        hb9 / p16 / p17 / p32 / const_scattered with SLAMHIP_NO_BAND=1
  k_ba_window (batch, <= 5 free poses in a row)         const_most (P 25, 5 free), small (P 12, 4 free); also SLAMHIP_BA_WINDOW_ONE=1
  k_schur_groups_m (batch, MFMA build)                  hb9, p16, hb16, ragged, const_first: pad2 = 1 (sgm_lds_bytes <= 64 KB)
  k_schur_groups_b (batch, vector build)                wide_sparse (hb 18, 3 observations per point: the matrix Y of a group of
                                                        256 / 3 points x 19 slots is far beyond 64 KB: pad2 = 0), and every window
                                                        with SLAMHIP_BA_NO_MFMA=1
The library reports hb (slam_ba_halfband), the pose order (slam_ba_plan_order) and per-window status / iteration counts: asserted.
Which solver / build kernel ran is not reported: the rules above are those of the dispatch code, and the batch test shows the MFMA /
vector split by difference (a window whose result changes bit-wise under SLAMHIP_BA_NO_MFMA=1 ran on the matrix cores).

Measured on an MI355X, r = E_hip / max(E_orc, E_np, 4 * 2^-52), largest over the cases and measures of the row (full table per measure:
DESIGN.md 3.4.1, "stage tests"):
  build   grouped (default, rebuilds, flags) 1.78 (g, ragged at inv_delta 1e-6) | ungrouped 1.01 | two shards 1.33 | 50 KF / 1e5
          observations: sampled blocks 1.08, whole buffer against the oracle 1.32
  solve   default 3.94 (predicted_ssr, p32, model-fed) | one workgroup forced 2.42 | twist spread 3.94 | tiled chain 4.13 (predicted_ssr,
          p32, model-fed) | ungrouped + k_backsub / k_trial 2.36;  dp <= 1.32, dl <= 1.51 everywhere
  step    slam_local_ba 2.14 (ssr_init, const_most) | batch 2.14 | batch, vector build 2.14 | batch, k_ba_window on one workgroup 2.14;
          dp <= 1.02, dl <= 1.00 everywhere
  k = 4 x the largest r of the stage: build 7.2, solve 16.6, step 8.6 (hp_ba.K).  The ratios above 2 are costs a few ulps off a yardstick
  that sits on its floor of 4 ulps; no path is ten times another on the same window; no defect found.
Symmetry: S_qp is S_pq' bit for bit; inside a diagonal block the two triangles are summed separately and differ in the last bits (the
solvers read one triangle): asserted within twice the bound of S (check_build)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hp_ba as hp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV_DELTAS = (1.0 / hp.LM_DELTA0, 3.0, 1e-6)
REPR_EPS = 5.0
_WIN = {}


def windows():
    if not _WIN:
        from slam_jl_amd import synthetic as syn
        import slam_jl_amd as slam
        _WIN.update(hp.stage_windows(syn)); _WIN.update(hp.batch_windows(syn))
        s = _WIN["loop"]
        order, hb, reordered = slam.ba_plan_order(_cache(s))
        assert reordered and hb <= 20 < syn.ba_halfband(s), "the loop-closure window should be banded only after relabelling"
        _WIN["loop_planned"] = hp.relabel(s, order)
        assert syn.ba_halfband(_WIN["loop_planned"]) == hb
    return _WIN


def _cache(s):
    import slam_jl_amd as slam
    return slam.LocalBACache(s["theta0"].copy(), s["theta_const"], s["pixels_yx"], s["pose_ids"], s["point_ids"])


def _hip_shard(s, lo=0, hi=None):
    from slam_jl_amd import sharded_ba
    hi = s["M"] if hi is None else hi
    n = 6 * s["P"]
    sel = np.flatnonzero((s["point_ids"] - 1 >= lo) & (s["point_ids"] - 1 < hi))
    th = np.concatenate([s["theta0"][:n], s["theta0"][n + 3 * lo:n + 3 * hi]])
    return sharded_ba.HipShard(s["cam"], s["P"], th, s["theta_const"], s["pixels_yx"][sel], s["pose_ids"][sel], s["point_ids"][sel] - lo)


def _host(t):
    return t.detach().cpu().numpy().copy()


# ---------------------------------------------------------------------------------------------------------------------------------
# the product calls of one case: arrays only (the same function runs in the child processes of the env-knob variants)
# ---------------------------------------------------------------------------------------------------------------------------------
def run_shard(s, flags=False, rebuild=False, model_fed=True):
    import torch
    out = {}
    sh = _hip_shard(s)
    out["hb"] = np.int64(sh.halfband())
    ignore = 0
    if flags:
        out["n_out"] = np.int64(sh.flag_outliers(REPR_EPS)); out["outl"] = sh.download()[1]; ignore = 1
    for k in (2, 1, 0):                                          # every build into the SAME caller-owned buffer; inv_delta = 0.1 last
        out[f"red_{k}"] = _host(sh.build(ignore, INV_DELTAS[k]))
    out["trial"] = _host(sh.solve(sh.red, INV_DELTAS[0])); sh.commit(1)
    out["theta1"] = sh.download()[0]
    if rebuild:
        out["red_b1"] = _host(sh.build(ignore, INV_DELTAS[0]))   # linearised at the committed step
        sh.solve(sh.red, INV_DELTAS[0]); sh.commit(0)            # a rejected step: the linearisation point stays
        out["theta_rej"] = sh.download()[0]
        out["red_b2"] = _host(sh.build(ignore, INV_DELTAS[0]))
    sh.close()
    if model_fed:
        sh = _hip_shard(s)
        m = hp.Model(*hp.scene_args(s))
        if flags:
            sh.flag_outliers(REPR_EPS); m.outl = out["outl"].copy()
        sh.build(ignore, INV_DELTAS[0])                           # (the back-substitution reads the point blocks of the shard's own build)
        red_m = torch.from_numpy(hp.pack_reduce(m.build(ignore, INV_DELTAS[0]), s["P"])).to(sh.red.device)
        assert red_m.numel() == sh.red.numel()
        torch.cuda.synchronize()
        out["trial_m"] = _host(sh.solve(red_m, INV_DELTAS[0])); sh.commit(1)
        out["theta_m"] = sh.download()[0]
        sh.close()
    return out


def run_two_shards(s, cut):
    out = {}
    for k, (lo, hi) in enumerate(((0, cut), (cut, s["M"]))):
        sh = _hip_shard(s, lo, hi)
        out[f"hb_{k}"] = np.int64(sh.halfband()); out[f"red_{k}"] = _host(sh.build(0, INV_DELTAS[0]))
        sh.close()
    return out


def run_big():
    from slam_jl_amd import synthetic as syn
    sh = _hip_shard(hp.big_window(syn)[0])
    out = dict(hb=np.int64(sh.halfband()), red=_host(sh.build(0, INV_DELTAS[0])))
    sh.close()
    return out


def run_local_ba(s, iters_fast):
    import slam_jl_amd as slam
    c = slam.bundle_adjustment_(_cache(s), s["cam"], iterations=0, iters_fast=iters_fast)
    st = c.stats
    return dict(theta=c.theta, outl=c.outliers, stats=np.array([st["ssr_init"], st["ssr_pass1"], st["iters_pass1"], st["iters_pass2"], st["n_outliers"], 0.0]))


BATCH = ("const_most", "small", "hb9", "p16", "hb16", "ragged", "wide_sparse", "const_first")


def run_batch(names, iters_fast):
    import slam_jl_amd as slam
    W = windows()
    b = slam.BABatch([_cache(W[nm]) for nm in names], W[names[0]]["cam"])
    status = b.solve(iterations=0, iters_fast=iters_fast)
    out = {}
    for z, nm in enumerate(names):
        th, ol, st = b.window(z)
        out[nm + "/theta"] = th; out[nm + "/outl"] = ol
        out[nm + "/stats"] = np.array([st["ssr_init"], st["ssr_pass1"], st["iters_pass1"], st["iters_pass2"], st["n_outliers"], float(status[z])])
    return out


_CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import slam_jl_amd as slam
slam.default_context(0)
import test_gpu_ba_stages as T
out = {}
kind, names = %(kind)r, %(names)r
if kind == "big":
    out = T.run_big()
elif kind == "shard":
    for nm in names:
        for k, v in T.run_shard(T.windows()[nm]).items():
            out[nm + "/" + k] = v
else:
    out = T.run_batch(names, %(iters)d)
np.savez(%(path)r, **out)
print("OK")
'''


def _child(tmp_path, tag, env, kind, names, iters=1):
    """a fresh process per env-knob variant (the knobs are read once per process), one at a time; results through an .npz"""
    path = str(tmp_path / (tag + ".npz"))
    code = _CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), kind=kind, names=tuple(names), iters=iters, path=path)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-800:] + r.stderr[-2500:]
    z = np.load(path)
    if kind != "shard":
        return {k: z[k] for k in z.files}
    return {nm: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(nm + "/")} for nm in names}


# ---------------------------------------------------------------------------------------------------------------------------------
# the assertions
# ---------------------------------------------------------------------------------------------------------------------------------
def _report(stage, case, path, e, *yard):
    r = hp.ratios(e, *yard)
    b = hp.bounds(1.0, *yard)
    print("STAGE_R %-6s %-16s %-14s " % (stage, case, path) + "  ".join(f"{q}: r={r[q]:.2f} (E={e[q]:.2e} ref={b[q]:.2e})" for q in sorted(r)))
    return r


def check_build(orc, s, key, path, red, hb, ignore=0, inv_delta=INV_DELTAS[0], outl=None, lo=0, hi=None, label=""):
    b, e_orc, e_np, _, _ = hp.build_yardsticks(orc, s, key, ignore, inv_delta, outl, lo, hi)
    x = hp.unpack_reduce(red, s["P"])
    bad = hp.structure_errors(x["S"], hb, s["theta_const"])
    assert not bad, f"{key} [{path}] {label}: " + "; ".join(bad)
    e = hp.build_errors(x, b, b["scale"])
    case = f"{key or ''}{label}@{inv_delta:g}"
    _report("build", case, path, e, e_orc, e_np)
    bound = hp.bounds(hp.K["build"], e_orc, e_np)
    hp.check(f"build {case} [{path}]", e, bound)
    # symmetry: S_qp is S_pq' bit for bit; inside a DIAGONAL block the kernels sum the two triangles separately (the Schur term
    # (W V^-1) W' is not symmetric in floating point, and the solvers read one triangle): both lie within the bound of S from the
    # model's symmetric block, so they differ by at most twice that
    asym_diag, asym_off = hp.asymmetry(x["S"], b)
    assert asym_off == 0.0, f"build {case} [{path}]: S_qp is not the exact transpose of S_pq ({asym_off:.3e})"
    assert asym_diag <= 2 * bound["S"], f"build {case} [{path}]: a diagonal block of S is asymmetric by {asym_diag:.3e} > {2 * bound['S']:.3e}"
    return e, e_orc, e_np


def check_shard(orc, name, s, out, path):
    """build at three inv_delta, then the solve stage at 1 / delta0 (kernel-built and model-fed)"""
    from slam_jl_amd import synthetic as syn
    P = s["P"]
    assert int(out["hb"]) == syn.ba_halfband(s), f"{name} [{path}]: slam_ba_halfband is not the window's half-bandwidth in the caller's pose order"
    outl = out.get("outl")
    ignore = int(outl is not None)
    if outl is not None:
        m = hp.Model(*hp.scene_args(s))
        n_out = m.flag_outliers(REPR_EPS)
        assert m.flag_margin > 1e-6, f"{name}: an observation lies within {m.flag_margin} of a flag threshold: pick another seed"
        assert np.array_equal(outl, m.outl) and int(out["n_out"]) == n_out and 0 < n_out < s["O"], f"{name} [{path}]: outlier flags differ from the model's"
    for k, d in enumerate(INV_DELTAS):
        check_build(orc, s, name, path, out[f"red_{k}"], int(out["hb"]), ignore, d, outl, label="+flags" if ignore else "")
    st, e_orc, e_np, _ = hp.step_yardsticks(orc, s, name, outl)
    bound = hp.bounds(hp.K["solve"], e_orc, e_np)
    ssr = hp.unpack_reduce(out["red_0"], P)["ssr"]
    res = {}
    for tag in ("", "_m"):
        if "trial" + tag not in out:
            continue
        tr = out["trial" + tag]
        assert tr[3] == 0.0, f"{name} [{path}]: the solver reports a failed factorisation"
        x = dict(dx=s["theta0"] - out["theta1" if tag == "" else "theta_m"], trial_ssr=tr[0], predicted_ssr=tr[1], maxdx=tr[2], ssr=ssr)
        res[tag] = hp.step_errors(x, st, P)
        _report("solve", name + ("+flags" if ignore else "") + ("/model-fed" if tag else ""), path, res[tag], e_orc, e_np)
    why = ""
    if "_m" in res:
        fed_ok = all(res["_m"][q] <= bound[q] for q in bound)
        why = " -- the same solve fed with the MODEL's system is " + ("within its bounds: look at the BUILD" if fed_ok else "out of bounds too: look at the SOLVE / back-substitution")
    hp.check(f"solve {name} [{path}]{why}", res[""], bound)
    if "_m" in res:
        hp.check(f"solve of the model's reduced system, {name} [{path}]", res["_m"], bound)
    if "red_b1" in out:
        s1 = dict(s, theta0=out["theta1"])
        assert np.array_equal(out["theta_rej"], out["theta1"]), f"{name} [{path}]: commit(0) moved theta"
        check_build(orc, s1, None, path, out["red_b1"], int(out["hb"]), ignore, INV_DELTAS[0], outl, label=name + "/after-commit(1)")
        check_build(orc, s1, None, path, out["red_b2"], int(out["hb"]), ignore, INV_DELTAS[0], outl, label=name + "/after-commit(0)")


def check_step(orc, name, s, theta, outl, stats, path, steps=1):
    """one (two) LM iteration(s) through an entry point that does not expose S: theta, ssr_init, ssr_pass1, outlier flags"""
    assert stats[2] == steps and stats[3] == 0 and stats[5] == 0, f"{name} [{path}]: iterations / status {stats}"
    if steps == 1:
        st, e_orc, e_np, _ = hp.step_yardsticks(orc, s, name)
        theta_ref = st["theta_new"]
    else:
        st, e_orc, e_np = hp.lm2_yardsticks(orc, s, name)
        theta_ref = s["theta0"].astype(hp.LD) - st["dx"]
    e = hp.step_errors(dict(dx=s["theta0"] - theta, trial_ssr=stats[1], ssr=stats[0]), st, s["P"])
    only = ("dp", "dl", "trial_ssr", "ssr")
    _report("step", name + (f"/{steps} steps" if steps > 1 else ""), path, e, e_orc, e_np)
    hp.check(f"LM step {name} [{path}]", e, hp.bounds(hp.K["step"], e_orc, e_np), only=only)
    m = hp.Model(*hp.scene_args(s)); m.theta = theta_ref
    n_out = m.flag_outliers(REPR_EPS)
    assert m.flag_margin > 1e-6, f"{name}: an observation lies within {m.flag_margin} of a flag threshold after the step: pick another seed"
    assert np.array_equal(outl, m.outl) and stats[4] == n_out, f"{name} [{path}]: outlier flags after the step differ from the model's"


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) + (b): build and solve, single / sharded path
# ---------------------------------------------------------------------------------------------------------------------------------
SHARD_CASES = ("hb1", "hb9", "hb14", "hb15", "hb16", "hb17", "hb18", "hb20", "hb21_dense", "hb21_tiled", "p16", "p17", "p32", "loop",
               "loop_planned", "const_first", "const_scattered", "const_most", "ragged")


@pytest.mark.parametrize("name", SHARD_CASES)
def test_build_and_solve_default_paths(slam, orc, name):
    """the planner's own choice per window (module docstring): k_schur_groups + k_schur_reduce, except hb21_tiled (ungrouped build);
    k_band_solve on one workgroup (hb14 .. hb20, p16, p17, const_most, ragged, loop_planned if its band allows no twist), twisted on two
    (hb1, hb9, p32, const_first, const_scattered), k_dense_solve (hb21_dense, loop), tiled k_chol_* chain (hb21_tiled).  Includes the
    round-3 half-bandwidths 15-18, BS_MAXHB and BS_MAXHB + 1, 6P = 96 / 102 / 192, and the constant-pose / ragged families."""
    s = windows()[name]
    check_shard(orc, name, s, run_shard(s), "default")


@pytest.mark.parametrize("name", ("hb9", "hb16", "ragged", "loop"))
def test_rebuild_into_the_same_buffer(slam, orc, name):
    """a second and a third build into the SAME buffer: after solve + commit(1) the system is the model's at the new theta, after a
    further solve + commit(0) it is again that one (a rejected step must not move the linearisation point, and theta stays bit-identical)"""
    s = windows()[name]
    check_shard(orc, name, s, run_shard(s, rebuild=True, model_fed=False), "rebuild")


@pytest.mark.parametrize("name", ("hb9", "hb17", "ragged", "const_scattered", "loop"))
def test_build_and_solve_ignoring_flagged_outliers(slam, orc, name):
    """slam_ba_flag_outliers at theta0 (repr_eps = 5 flags a few per cent of the perturbed window): the flags equal the model's, and
    build(ignore_outliers = 1) / solve equal the model's given the same flags"""
    s = windows()[name]
    check_shard(orc, name, s, run_shard(s, flags=True), "default")


@pytest.mark.parametrize("name", ("hb9", "hb18", "ragged", "const_scattered", "loop"))
def test_two_shards_by_point_range(slam, orc, name):
    """two shards by point range on one GPU: each buffer equals the model's contribution of that range (S and g on the scale of the
    whole window), and their sum equals the whole"""
    s = windows()[name]
    cut = s["M"] // 3
    out = run_two_shards(s, cut)
    tot = out["red_0"] + out["red_1"]
    errs = [check_build(orc, s, name, "shard", out[f"red_{k}"], int(out[f"hb_{k}"]), lo=lo, hi=hi, label=f"[{lo},{hi})")
            for k, (lo, hi) in enumerate(((0, cut), (cut, s["M"])))]
    b, e_orc, e_np, _, _ = hp.build_yardsticks(orc, s, name, 0, INV_DELTAS[0])
    e = hp.build_errors(hp.unpack_reduce(tot, s["P"]), b)
    _report("build", name + "/sum of 2", "shard", e, e_orc, e_np)
    # the sum carries both shards' rounding: the sum of their bounds
    bound = {q: sum(hp.bounds(hp.K["build"], eo, en)[q] for _, eo, en in errs) for q in e}
    hp.check(f"sum of two shards, {name}", e, bound)
    assert not hp.structure_errors(hp.unpack_reduce(tot, s["P"])["S"], max(int(out["hb_0"]), int(out["hb_1"])), s["theta_const"])


VARIANTS = {
    # tag: (environment, windows) -- what each selects is in the module docstring
    "no_groups": ({"SLAMHIP_NO_GROUPS": "1"}, ("hb9", "hb16", "hb20", "p17", "const_scattered", "ragged")),
    "no_band": ({"SLAMHIP_NO_BAND": "1"}, ("hb9", "p16", "p17", "p32", "const_scattered")),
    "twist_spread": ({"SLAMHIP_TWIST_SPREAD": "1"}, ("hb1", "hb9", "p32", "const_scattered")),
    "no_twist": ({"SLAMHIP_NO_TWIST": "1"}, ("hb1", "hb9", "const_scattered")),
}


@pytest.mark.parametrize("tag", sorted(VARIANTS))
def test_build_and_solve_forced_paths(slam, orc, tmp_path, tag):
    """the other implementation of a stage on windows the default run covers too (one child process per knob):
    no_groups     SLAMHIP_NO_GROUPS=1: the ungrouped build k_linearize / k_points / k_obs_factors / k_blocks with k_backsub / k_trial
                  (hb9, hb16, hb20, p17, const_scattered, ragged) in place of k_schur_groups / k_update_groups
    no_band       SLAMHIP_NO_BAND=1: the tiled chain k_chol_prepare / k_chol_first / k_chol_step / k_chol_backsolve on hb9, p16, p17,
                  p32 (6P = 96 / 102 / 192: on and around its 32-wide tiles) and const_scattered
    twist_spread  SLAMHIP_TWIST_SPREAD=1: k_band_solve twisted, its two workgroups on different XCDs (hb1, hb9, p32, const_scattered)
    no_twist      SLAMHIP_NO_TWIST=1: k_band_solve on ONE workgroup where the default twists (hb1, hb9, const_scattered)"""
    env, names = VARIANTS[tag]
    res = _child(tmp_path, tag, env, "shard", names)
    for nm in names:
        check_shard(orc, nm, windows()[nm], res[nm], tag)


@pytest.mark.parametrize("path", ("default", "no_groups"))
def test_build_of_the_large_window(slam, orc, syn, tmp_path, path):
    """the 50 key-frame / 1e5 observation window of the benchmarks, build stage only: k_schur_groups over hundreds of point groups with
    k_schur_reduce folding their partial blocks (default), and the ungrouped k_linearize / k_points / k_obs_factors / k_blocks with its
    passes split into chunks (SLAMHIP_NO_GROUPS=1, child process).  The model forms a sub-sample of the blocks (hp_ba.big_window);
    on those the bound is k * max(E_orc, 4 * 2^-52) (np_ba is out of reach at this size).  The WHOLE buffer is then compared with the
    oracle's on the oracle's own scales: |hip - orc| <= |hip - model| + |orc - model|, so (k + 1) times the same yardstick, taking
    the sampled blocks' E_orc as representative of the others."""
    s, mb, e_orc, o = hp.big_yardsticks(orc, syn)
    out = run_big() if path == "default" else _child(tmp_path, "big_" + path, {"SLAMHIP_NO_GROUPS": "1"}, "big", ())
    x = hp.unpack_reduce(out["red"], s["P"])
    assert int(out["hb"]) == 9
    bad = hp.structure_errors(x["S"], 9, s["theta_const"])
    assert not bad, "; ".join(bad)
    e = hp.block_errors(x, mb)
    _report("build", "big/blocks", path, e, e_orc)
    hp.check(f"build of the large window, sampled blocks [{path}]", e, hp.bounds(hp.K["build"], e_orc))
    e_all = hp.build_errors(x, o)
    _report("build", "big/vs-oracle", path, e_all, e_orc)
    hp.check(f"build of the large window, whole buffer against the oracle [{path}]", e_all, hp.bounds(hp.K["build"] + 1.0, e_orc))


# ---------------------------------------------------------------------------------------------------------------------------------
# (c): one LM step through slam_local_ba / slam_local_ba_batch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("hb9", "hb16", "hb21_dense", "hb21_tiled", "loop", "const_most", "ragged", "p17"))
def test_local_ba_one_step(slam, orc, name):
    """slam_local_ba(iters_fast = 1, iterations = 0): the device-paced LM (use_state = 1) with the library's private reduce buffer.
    hb9: grouped build + twisted k_band_solve; hb16, const_most, ragged, p17: one workgroup; hb21_dense: k_dense_solve; hb21_tiled:
    ungrouped build + tiled chain; loop: relabelled by ba_pose_order (slam_ba_plan_order reports it: asserted in windows()), banded,
    theta back in the caller's order.  Every step is an accepted one (asserted by the yardstick helper)."""
    s = windows()[name]
    r = run_local_ba(s, 1)
    check_step(orc, name, s, r["theta"], r["outl"], r["stats"], "local_ba")


@pytest.mark.parametrize("name", ("hb9", "const_most", "loop"))
def test_local_ba_two_steps(slam, orc, name):
    """two iterations: the second step's damping delta0 / max(1/3, 1 - (2 rho - 1)^3) carries predicted_ssr of the first, which this
    entry point does not return; the second build is the band-only rewrite into the library's private buffer (red == ba->reduce)"""
    s = windows()[name]
    r = run_local_ba(s, 2)
    check_step(orc, name, s, r["theta"], r["outl"], r["stats"], "local_ba", steps=2)


def _check_batch(orc, out, names, path, steps=1):
    W = windows()
    for nm in names:
        check_step(orc, nm, W[nm], out[nm + "/theta"], out[nm + "/outl"].astype(bool), out[nm + "/stats"], path, steps)


def test_batch_one_step_on_every_batch_path(slam, orc, tmp_path):
    """slam_local_ba_batch(iters_fast = 1, iterations = 0) on a mixed batch (BATCH), three times: default, SLAMHIP_BA_NO_MFMA=1,
    SLAMHIP_BA_WINDOW_ONE=1.
      const_most (P 25, 5 free poses in a row), small (P 12, 4 free)   -> k_ba_window (nfree <= 5 == pspan, P <= 128): two workgroups
                                                                          per window by default, one with SLAMHIP_BA_WINDOW_ONE=1
      hb9, p16, hb16, ragged, const_first                              -> k_schur_groups_m: TT == 256 (every group <= 256 observations,
                                                                          (max hb + 1)(max hb + 2) / 2 <= 256) and sgm_lds_bytes <= 64 KB
      wide_sparse (hb 18, 3 observations per point)                    -> k_schur_groups_b<256> in the SAME launch set (pad2 = 0: groups of
                                                                          256 / 3 points x 19 window slots, Y far beyond 64 KB)
      everything but k_ba_window's windows with SLAMHIP_BA_NO_MFMA=1   -> k_schur_groups_b
    pad2 differs between windows of one call; that it does is shown by difference: under SLAMHIP_BA_NO_MFMA=1 the results of the MFMA
    windows change bit-wise, those of wide_sparse and of k_ba_window's windows do not."""
    out = run_batch(BATCH, 1)
    _check_batch(orc, out, BATCH, "batch")
    vec = _child(tmp_path, "no_mfma", {"SLAMHIP_BA_NO_MFMA": "1"}, "batch", BATCH)
    _check_batch(orc, vec, BATCH, "batch/no_mfma")
    one = _child(tmp_path, "window_one", {"SLAMHIP_BA_WINDOW_ONE": "1"}, "batch", BATCH)
    _check_batch(orc, one, BATCH, "batch/window_one")
    same = {nm: np.array_equal(out[nm + "/theta"], vec[nm + "/theta"]) for nm in BATCH}
    assert same["wide_sparse"] and same["const_most"] and same["small"], f"windows outside the matrix-core build changed under SLAMHIP_BA_NO_MFMA=1: {same}"
    assert not any(same[nm] for nm in ("hb9", "p16", "hb16", "ragged", "const_first")), f"windows expected on the matrix cores did not change under SLAMHIP_BA_NO_MFMA=1: {same}"


def test_batch_two_steps(slam, orc):
    """two iterations per window of the mixed batch: k_control_b's delta update from rho (predicted_ssr of the first step) per window,
    and k_ba_window's in-kernel LM loop"""
    names = ("const_most", "hb9", "wide_sparse")
    _check_batch(orc, run_batch(names, 2), names, "batch", steps=2)
