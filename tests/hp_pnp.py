"""Extended-precision model of the single-pose refinement, pnp_bundle_adjustment (bundle_adjustment.jl:113-171) (test helper, CPU only).

A plain, slow restatement in numpy.longdouble (80-bit x87) of the WHOLE call, stage by stage, used as the common reference of
test_pnp_model_host.py and test_gpu_pnp_model.py:

  start         X0 = (RotZYX(pose[1:3,1:3]).theta1..3, pose[1:3,4]):  theta1 = atan(R21, R11), theta2 = atan(-R31, sqrt(R11^2 + R21^2)),
                theta3 = atan(R13 s1 - R23 c1, R22 c1 - R12 s1)  (Rotations.jl; defined at theta2 = +-pi/2 as well)
  residual      hp_ba._residual: X = Rz(t1) Ry(t2) Rx(t3) p + t, r = (py - (fy X_y / X_z + cy), px - (fx X_x / X_z + cx)), and the depth X_z
  Jacobian      2n x 6 by complex step (hp_ba's width 1e-40)
  step          H = J'J, g = J'r, D = clamp(diag H, 1e-6, 1e32) / delta, dx = (H + D)^-1 g by hp_ba.cholesky_solve, trial = |r(X - dx)|^2,
                predicted = |J dx - r|^2
  LM rule       the one hp_ba's header states, with LeastSquaresOptim's reject branch and convergence tests: rho = (trial - ssr) /
                (predicted - ssr) > 1e-3 accepts (delta <- min(delta / max(1/3, 1 - (2 rho - 1)^3), 1e16), decrease <- 2, new Jacobian,
                converged = max|dx| <= 1e-8 or |ssr - trial| / (|ssr| + 1e-8) <= 1e-8); otherwise delta <- max(delta / decrease, 1e-16),
                decrease <- 2 decrease, the SAME H and g again, converged = max|dx| <= 1e-8
  the call      initial_error at X0; pass 1 (iters_fast, all points); flags = depth < depth_eps or r^2 > repr_eps at the end of pass 1;
                n - n_outliers < 5: identity pose, final_error = the cost of pass 1; else pass 2 (iterations, flagged points left out)

The model returns more than the ABI does (Result): the trace (one record per iteration), the parameters after each pass, the decision
margins of every point / iteration, |n - no - 5|.  Nothing here is shared with the oracle, ba_math.hpp or np_pnp.py.  The second half
holds the error measures (every scale is the model's), the assertion function of both test files, and the case list."""
import numpy as np

import hp_ba
from hp_ba import CLD, LD, LM_DELTA0, LM_MAX_DELTA, LM_MAX_DIAGONAL, LM_MIN_DIAGONAL, LM_MIN_STEP_QUALITY, LM_XTOL, _H, _residual, cholesky_solve

LM_FTOL, LM_MIN_DELTA = 1e-8, 1e-16
# the asserted k per measure group: 4 x the largest measured r = E_hip / max(E_orc, E_np, 4 * 2^-52) of the group over the three launch
# forms: parameters 4 x 3.06, costs 4 x 12.15 (table and what the 12.15 is: DESIGN.md 3.5.1 and the docstring of test_gpu_pnp_model.py);
# test_pnp_model_host.py proves every mutant of np_pnp.py is rejected at these k, and still at ten times these k
K = dict(parameters=12.3, costs=48.6)
GROUP = dict(x="parameters", R="parameters", t="parameters", initial="costs", final="costs")


def rotzyx_angles(pose):
    """RotZYX(pose[1:3,1:3]) -> (theta1, theta2, theta3), then the translation: X0 (6,) longdouble"""
    R = np.asarray(pose).astype(LD)
    t1 = np.arctan2(R[1, 0], R[0, 0])
    s1, c1 = np.sin(t1), np.cos(t1)
    t2 = np.arctan2(-R[2, 0], np.sqrt(R[0, 0] * R[0, 0] + R[1, 0] * R[1, 0]))
    t3 = np.arctan2(R[0, 2] * s1 - R[1, 2] * c1, R[1, 1] * c1 - R[0, 1] * s1)
    return np.array([t1, t2, t3, R[0, 3], R[1, 3], R[2, 3]], dtype=LD)


def rotation(x):
    """Rz(x0) Ry(x1) Rx(x2), factor by factor (longdouble)"""
    a, b, c = (LD(v) for v in x[:3])
    one, zero = LD(1), LD(0)
    Rz = np.array([[np.cos(a), -np.sin(a), zero], [np.sin(a), np.cos(a), zero], [zero, zero, one]], dtype=LD)
    Ry = np.array([[np.cos(b), zero, np.sin(b)], [zero, one, zero], [-np.sin(b), zero, np.cos(b)]], dtype=LD)
    Rx = np.array([[one, zero, zero], [zero, np.cos(c), -np.sin(c)], [zero, np.sin(c), np.cos(c)]], dtype=LD)
    return Rz @ (Ry @ Rx)


def pose_of(x):
    T = np.eye(4, dtype=LD)
    T[:3, :3] = rotation(x); T[:3, 3] = x[3:]
    return T


class Result(dict):
    __getattr__ = dict.__getitem__


class Model:
    def __init__(self, cam, pixels_yx, points):
        self.cam = tuple(float(c) for c in cam)
        self.px = np.asarray(pixels_yx, dtype=np.float64).reshape(-1, 2).astype(LD)
        self.pts = np.asarray(points, dtype=np.float64).reshape(-1, 3).astype(LD)
        self.n = len(self.px)

    def residuals(self, X):
        """r (n,2) and the camera depth (n,) at the parameters X (longdouble or clongdouble)"""
        X = np.asarray(X)
        t = CLD if np.iscomplexobj(X) else LD
        return _residual(self.cam, np.broadcast_to(X.astype(t), (self.n, 6)), self.pts.astype(t), self.px.astype(t))

    def jacobian(self, X):
        """(n,2,6) by complex step"""
        J = np.zeros((self.n, 2, 6), dtype=LD)
        for k in range(6):
            q = np.asarray(X, dtype=LD).astype(CLD); q[k] += 1j * _H
            J[:, :, k] = self.residuals(q)[0].imag / _H
        return J

    def step(self, X, act, delta, J=None):
        """one damped step at X over the active points: dict dx, Xt, ssr, trial, predicted, maxdx, H, g (no decision)"""
        r = self.residuals(X)[0] * act[:, None]
        J = (self.jacobian(X) if J is None else J) * act[:, None, None]
        Jf, rf = J.reshape(-1, 6), r.reshape(-1)
        H, g = Jf.T @ Jf, Jf.T @ rf
        D = np.clip(np.diag(H), LM_MIN_DIAGONAL, LM_MAX_DIAGONAL) / LD(delta)
        dx = cholesky_solve(H + np.diag(D), g)
        Xt = np.asarray(X, dtype=LD) - dx
        rt = self.residuals(Xt)[0] * act[:, None]
        p = Jf @ dx - rf
        return dict(dx=dx, Xt=Xt, ssr=(rf * rf).sum(dtype=LD), trial=(rt * rt).sum(dtype=LD), predicted=(p * p).sum(dtype=LD),
                    maxdx=np.abs(dx).max(), H=H, g=g, D=D, J=J)

    def lm(self, X, act, iterations):
        """LeastSquaresOptim's loop -> (X, ssr, trace).  A trace record: accepted, rho, delta (the one the step used), maxdx, fired
        ('' / 'x' / 'f' / 'xf': which convergence test ended the pass), rho_margin = |rho - 1e-3|, f_margin = | |ssr - trial| /
        (|ssr| + ftol) - ftol | (accepted steps), x_margin = |max|dx| - xtol| / xtol."""
        X = np.asarray(X, dtype=LD).copy()
        ssr = self.step_cost(X, act)
        delta, decrease = LD(LM_DELTA0), LD(2)
        J, conv, it, trace = None, False, 0, []
        while not conv and it < iterations:
            it += 1
            if J is None:
                J = self.jacobian(X)
            try:
                st = self.step(X, act, delta, J)
            except ArithmeticError:
                trace.append(Result(accepted=False, rho=np.nan, delta=float(delta), maxdx=0.0, fired="chol", rho_margin=np.inf, f_margin=np.inf, x_margin=np.inf))
                break
            trial, pred, mx = st["trial"], st["predicted"], st["maxdx"]
            with np.errstate(invalid="ignore", divide="ignore"):
                rho = (trial - ssr) / (pred - ssr)
            rec = Result(rho=float(rho), delta=float(delta), maxdx=float(mx), f_margin=np.inf, x_margin=float(abs(mx - LD(LM_XTOL)) / LD(LM_XTOL)),
                         rho_margin=np.inf if np.isnan(rho) else float(abs(rho - LD(LM_MIN_STEP_QUALITY))))      # (0 / 0: n = 0, the same NaN everywhere)
            x_conv = bool(mx <= LD(LM_XTOL))
            if rho > LD(LM_MIN_STEP_QUALITY):
                fq = abs(ssr - trial) / (abs(ssr) + LD(LM_FTOL))
                f_conv = bool(fq <= LD(LM_FTOL))
                rec.update(accepted=True, f_margin=float(abs(fq - LD(LM_FTOL))), fired=("x" if x_conv else "") + ("f" if f_conv else ""))
                ssr, X, J = trial, st["Xt"], None
                u = LD(2) * rho - LD(1)
                delta = min(delta / max(LD(1) / LD(3), LD(1) - u * u * u), LD(LM_MAX_DELTA)); decrease = LD(2)
                conv = x_conv or f_conv
            else:
                rec.update(accepted=False, fired="x" if x_conv else "")
                delta = max(delta / decrease, LD(LM_MIN_DELTA)); decrease = decrease * LD(2)
                conv = x_conv
            rec["decrease"] = float(decrease)
            trace.append(rec)
        return X, ssr, trace

    def step_cost(self, X, act):
        r = self.residuals(X)[0] * act[:, None]
        return (r * r).sum(dtype=LD)

    def classify(self, X, repr_eps, depth_eps):
        """flags and, per point, the distance to the nearest threshold whose crossing would flip the flag"""
        r, z = self.residuals(X)
        r2 = (r * r).sum(1)
        a, b = z < LD(depth_eps), r2 > LD(repr_eps)
        ma, mb = np.abs(z - LD(depth_eps)), np.abs(r2 - LD(repr_eps))
        margin = np.where(a & b, np.maximum(ma, mb), np.where(a, ma, np.where(b, mb, np.minimum(ma, mb))))
        return np.asarray(a | b), margin.astype(np.float64), np.asarray(a), np.asarray(b)

    def run(self, pose0, iters_fast, iterations, repr_eps, depth_eps):
        n = self.n
        X0 = rotzyx_angles(pose0)
        everything = np.ones(n, dtype=bool)
        initial = self.step_cost(X0, everything)
        X1, ssr1, tr1 = self.lm(X0, everything, iters_fast)
        flags, margin, by_depth, by_repr = self.classify(X1, repr_eps, depth_eps)
        no = int(flags.sum())
        identity = n - no < 5
        inlier1 = self.step_cost(X1, ~flags)
        if identity:
            X2, final, tr2 = X1, ssr1, []
        else:
            X2, final, tr2 = self.lm(X1, ~flags, iterations)
        return Result(X0=X0, X1=X1, X2=X2, pose=np.eye(4, dtype=LD) if identity else pose_of(X2), initial=initial, pass1=ssr1, inlier1=inlier1,
                      final=final, flags=flags, n_outliers=no, identity=identity, trace1=tr1, trace2=tr2, flag_margin=margin,
                      by_depth=by_depth, by_repr=by_repr, inlier_margin=abs(n - no - 5))


def trace_string(m):
    """'AARRA|AAA': accepted / rejected steps of pass 1 | pass 2"""
    return "|".join("".join("A" if t.accepted else "R" for t in tr) for tr in (m.trace1, m.trace2))


# ---------------------------------------------------------------------------------------------------------------------------
# error measures (scaled by the model only), decisions, and the assertion function of both test files
# ---------------------------------------------------------------------------------------------------------------------------
def errors(out, m, gimbal=False):
    """out = (pose, initial_error, final_error, flags, n_outliers) of an implementation, m = Model.run's.  x: the six parameters read back
    from the returned pose (RotZYX in longdouble), per entry relative to max(|x*|, 1e-8) -- not at theta2 = +-pi/2 (gimbal), where the
    angles of a rounded rotation are not defined to rounding; R: the rotation's entries (absolute: a rotation's scale is 1); t: relative
    to max(|t*|, 1e-8); the costs relative (a zero cost must be returned as zero).  The identity exit has no parameters: decisions() holds it."""
    pose = np.asarray(out[0])
    e = dict(initial=hp_ba._rel(out[1], m.initial), final=hp_ba._rel(out[2], m.final))
    if not m.identity:
        T = pose.astype(LD)
        e["R"] = float(np.abs(T[:3, :3] - m.pose[:3, :3]).max())
        e["t"] = float((np.abs(T[:3, 3] - m.pose[:3, 3]) / np.maximum(np.abs(m.pose[:3, 3]), LD(1e-8))).max())
        if not gimbal:
            e["x"] = float((np.abs(rotzyx_angles(pose) - m.X2) / np.maximum(np.abs(m.X2), LD(1e-8))).max())
    return e


def decisions(out, m):
    """the exact part: a list of complaints (empty = every decision is the model's)"""
    pose, _, _, flags, no = out
    bad = []
    if not np.array_equal(np.asarray(flags, dtype=bool), m.flags):
        bad.append(f"outlier flags differ at {np.flatnonzero(np.asarray(flags, dtype=bool) != m.flags)[:8]}")
    if int(no) != m.n_outliers:
        bad.append(f"n_outliers {no} != {m.n_outliers}")
    is_id = np.array_equal(np.asarray(pose), np.eye(4))
    if is_id != m.identity:
        bad.append(f"identity exit {'taken' if is_id else 'not taken'}, the model: {'taken' if m.identity else 'not taken'} (n - no = {len(m.flags) - m.n_outliers})")
    if not m.identity and not np.array_equal(np.asarray(pose)[3], [0.0, 0.0, 0.0, 1.0]):
        bad.append("last row of the pose is not (0, 0, 0, 1)")
    return bad


def bounds(e_orc, e_np, k=None):
    """k(group) * max(E_orc, E_np, 4 * 2^-52) per measure -- hp_ba.bounds' convention with one k per measure group"""
    k = K if k is None else k
    b = hp_ba.bounds(1.0, e_orc, e_np)
    return {q: k[GROUP[q]] * v for q, v in b.items()}


def ratios(e, e_orc, e_np):
    return hp_ba.ratios(e, e_orc, e_np)


def check(label, out, y, k=None, only=None):
    """THE assertion: decisions exact, every measure within k * max(E_orc, E_np, 4 * 2^-52).  y: yardsticks(case); only: the measure
    group to hold (KeypointSet.compute_pose returns no costs)."""
    bad = decisions(out, y.m)
    assert not bad, f"{label}: " + "; ".join(bad)
    b = bounds(y.e_orc, y.e_np, k)
    hp_ba.check(label, errors(out, y.m, y.case.get("gimbal", False)), b, None if only is None else [q for q in b if GROUP[q] == only])


def rejected(label, out, y, k=None):
    """True when check() fails (the mutation test)"""
    try:
        check(label, out, y, k)
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------------------------------------------------------------------
# the case list
# ---------------------------------------------------------------------------------------------------------------------------
COUNTS = (0, 1, 4, 5, 6, 63, 64, 65, 255, 256, 257, 300, 1200)      # around the 64-lane butterflies and the stride PNP_T = 256
OFF, BIG = dict(repr_eps=1e30, depth_eps=-1e30), 1e30


def _pose(syn, ang, t):
    T = np.eye(4); T[:3, :3] = syn.rotzyx(*ang); T[:3, 3] = t
    return T


def rebase(s, pose):
    """the scene with its world points moved so that `pose` sees what pose_gt saw (camera-frame points unchanged): pose_gt := pose"""
    Xc = s["points"] @ s["pose_gt"][:3, :3].T + s["pose_gt"][:3, 3]
    t = dict(s)
    t["points"] = np.ascontiguousarray((Xc - pose[:3, 3]) @ pose[:3, :3]); t["pose_gt"] = pose.copy(); t["pose0"] = pose.copy()
    return t


def _case(name, s, iters_fast, iterations, repr_eps=3.0, depth_eps=1e-6, pose0=None, **tags):
    return dict(name=name, cam=s["cam"], pose0=np.array(s["pose0"] if pose0 is None else pose0, dtype=np.float64), pixels_yx=np.ascontiguousarray(s["pixels_yx"]),
                points=np.ascontiguousarray(s["points"]), n=len(s["points"]), iters_fast=iters_fast, iterations=iterations,
                repr_eps=float(repr_eps), depth_eps=float(depth_eps), **tags)


# start poses that reject steps, found by a seeded search with np_pnp.py over `pnp_scene` (angles + da, t + dt of the scene's own
# (0.03, -0.05, 0.02) / (0.3, -0.1, 0.5), 7000 starts up to 1.3 rad / 9 m away); the search is not part of the suite, the model's trace
# of every entry is asserted in test_pnp_model_host.py.  Pass 2 starts where pass 1 converged, so no start rejects a step THERE at
# the reference's counts: those cases stop pass 1 after 2-3 iterations and classify with repr_eps = 1e5.
# (name, n, scene seed, da, dt, iters_fast, iterations, repr_eps, the trace the model must produce)
REJECTION_STARTS = (
    ("reject_pass1", 257, 264, (1.21, 0.54, -0.59), (3.1, -2.7, 4.8), 12, 20, 3.0, "AARAAAAAAA|AAAAA"),
    ("reject_twice_pass1", 65, 8, (0.82, 0.23, -0.34), (8.0, 8.2, 8.4), 12, 20, 3.0, "ARRAAAAAAA|AAAAA"),
    ("reject_both_passes", 65, 8, (1.11, -1.26, 0.14), (-7.7, 0.1, 4.6), 2, 14, 1e5, "AR|AAARRAAAAAAAAA"),
    ("reject_accept_reject_pass2", 40, 7, (-1.21, 1.13, -0.1), (-3.9, 5.9, 6.4), 2, 14, 1e5, "AA|AAAARARRAAAAAA"),
    ("reject_first_step", 257, 264, (-0.53, -0.74, -0.11), (4.6, -2.3, -5.1), 3, 14, 1e5, "RRR|AAAAAAAAAA"),
    ("reject_then_identity", 257, 264, (1.2, 0.9, -1.0), (3.0, -4.0, 8.0), 5, 10, 3.0, "AARRA|"),
)


def far_start(syn, da, dt):
    return _pose(syn, np.add((0.03, -0.05, 0.02), da), np.add((0.3, -0.1, 0.5), dt))


_CASES = {}


def cases(syn):
    """name -> case: n, the scene, the start pose, iters_fast, iterations, repr_eps, depth_eps (+ tags: gimbal, expect).  Fixed: no
    case is chosen or dropped at run time; test_pnp_model_host.py holds every entry to the admission conditions."""
    if _CASES:
        return _CASES
    c = []
    sc = lambda n, seed=None, **kw: syn.pnp_scene(n=n, seed=n if seed is None else seed, **kw)
    # ---- (0, 0): the pose round trip pose_to_angles<4> -> angles_to_pose, initial_error and the inlier cost at X0 (nothing flagged) ----
    for n in (5, 64, 257):
        c.append(_case(f"trip_n{n}", sc(n), 0, 0, **OFF))
    for tag, t2 in (("1.2", 1.2), ("below_half_pi", np.pi / 2 - 1e-9), ("plus_half_pi", np.pi / 2), ("minus_half_pi", -np.pi / 2)):
        for n in (6, 65):
            s = rebase(sc(n, seed=100 + n), _pose(syn, (0.4, t2, -0.3), (0.3, -0.1, 0.5)))
            c.append(_case(f"trip_theta2_{tag}_n{n}", s, 0, 0, gimbal=abs(abs(t2) - np.pi / 2) < 1e-6, **OFF))
    # ---- (0, 0): classification at X0; repr_eps = half way between the model's two middle r^2 at X0 (half of the points flagged) ----
    for n in (6, 65, 300):
        s = sc(n, seed=200 + n)
        m = Model(s["cam"], s["pixels_yx"], s["points"])
        r = m.residuals(rotzyx_angles(s["pose0"]))[0]
        r2 = np.sort((r * r).sum(1).astype(np.float64))
        c.append(_case(f"classify_n{n}", s, 0, 0, repr_eps=float(0.5 * (r2[n // 2 - 1] + r2[n // 2])), expect="classify"))
    # ---- one iteration, the reference's counts, longer runs ----
    for n in (5, 64, 256, 1200):
        c.append(_case(f"it1_0_n{n}", sc(n), 1, 0))
    for n in COUNTS:
        c.append(_case(f"it1_1_n{n}", sc(n), 1, 1))
    for n in COUNTS:
        c.append(_case(f"it5_10_n{n}", sc(n, seed=300 + n), 5, 10))
    for n in (64, 256, 300, 1200):
        c.append(_case(f"it12_20_n{n}", sc(n, seed=400 + n), 12, 20, expect="pass2_converges"))
    # ---- rejected steps ----
    for name, n, seed, da, dt, itf, it, eps, trace in REJECTION_STARTS:
        c.append(_case(name, sc(n, seed=seed), itf, it, repr_eps=eps, pose0=far_start(syn, da, dt), expect="trace", trace=trace))
    # ---- thresholds ----
    s = sc(65, seed=501)                                     # 7 points BEHIND the camera whose pixel is their own (finite) projection: depth alone flags them
    Xc = s["points"] @ s["pose_gt"][:3, :3].T + s["pose_gt"][:3, 3]
    Xc[3:65:9, 2] = -Xc[3:65:9, 2]
    fx, fy, cx, cy = s["cam"]
    s["pixels_yx"][3:65:9] = np.stack([fy * Xc[3:65:9, 1] / Xc[3:65:9, 2] + cy, fx * Xc[3:65:9, 0] / Xc[3:65:9, 2] + cx], 1)
    s["points"] = (Xc - s["pose_gt"][:3, 3]) @ s["pose_gt"][:3, :3]
    c.append(_case("behind_n65", s, 5, 10, expect="depth_alone"))
    c.append(_case("depth_eps_20_n257", sc(257, seed=502), 5, 10, depth_eps=20.0, expect="depth_in_front"))
    for keep, nbad in ((4, 5), (5, 4)):                      # n - no exactly 4 (identity exit) and exactly 5 (refined): displaced pixels of a 9-point scene
        s = sc(9, seed=503, outlier_frac=0.0)
        s["pixels_yx"][:nbad] += 40.0
        c.append(_case(f"inliers_{keep}", s, 0, 10, repr_eps=9.0, pose0=s["pose_gt"], expect=f"inliers_{keep}"))
    # ---- points 5e6 m away: diag(H) of the translation is below 1e-6, the lower clamp of the damping decides the step ----
    s = sc(6, seed=504, outlier_frac=0.0)
    Xc = (s["points"] @ s["pose_gt"][:3, :3].T + s["pose_gt"][:3, 3]) * 1e6
    s["points"] = (Xc - s["pose_gt"][:3, 3]) @ s["pose_gt"][:3, :3]
    c.append(_case("far_n6", s, 5, 10, expect="clamp"))
    for q in c:
        assert q["name"] not in _CASES
        _CASES[q["name"]] = q
    return _CASES


_SMALL = {}


def small_cases(syn, S=130):
    """S small problems of one setting (5, 10, repr_eps 3) for ONE batch call: more workgroups than any other test launches; 5 <= n <= 27"""
    if not _SMALL:
        for z in range(S):
            # (seed 707 would be the rule's: its pass 1 stops 2.9e-11 from the f_conv edge, inside 10 x the cost bound -- not admitted)
            q = _case(f"small_{z}", syn.pnp_scene(n=5 + (7 * z) % 23, seed=1107 if z == 107 else 600 + z), 5, 10)
            _SMALL[q["name"]] = q
    return _SMALL


def stage_of(name):
    """the row of the tables in DESIGN.md 3.5.1 a case belongs to"""
    for prefix, stage in (("trip_", "round trip (0,0)"), ("classify_", "classification (0,0)"), ("it1_", "one iteration"), ("it5_10_", "(5,10)"),
                          ("it12_20_", "(12,20)"), ("reject_", "rejections"), ("small_", "130 small")):
        if name.startswith(prefix):
            return stage
    return "thresholds"


def settings(cs):
    """the cases grouped by (iters_fast, iterations, repr_eps, depth_eps), in list order: one batch call each"""
    g = {}
    for q in cs.values():
        g.setdefault((q["iters_fast"], q["iterations"], q["repr_eps"], q["depth_eps"]), []).append(q)
    return g


def call_args(q):
    return (q["cam"], q["pose0"], q["pixels_yx"], q["points"]), dict(iters_fast=q["iters_fast"], iterations=q["iterations"], repr_eps=q["repr_eps"], depth_eps=q["depth_eps"])


# ---------------------------------------------------------------------------------------------------------------------------
# the yardsticks: the model's run of a case, and what the C oracle and np_pnp.py achieve against it
# ---------------------------------------------------------------------------------------------------------------------------
_YARD = {}


def yardsticks(orc, q):
    """Result(case, m, out_orc, out_np, e_orc, e_np) of a case (cached by name; unnamed cases are not cached)"""
    key = q.get("name")
    if key is None or key not in _YARD:
        import np_pnp
        a, kw = call_args(q)
        m = Model(q["cam"], q["pixels_yx"], q["points"]).run(q["pose0"], q["iters_fast"], q["iterations"], q["repr_eps"], q["depth_eps"])
        o = orc.pnp_ba(*a, **kw)
        p = np_pnp.pnp_ba(*a, **kw)
        g = q.get("gimbal", False)
        y = Result(case=q, m=m, out_orc=o, out_np=p, e_orc=errors(o, m, g), e_np=errors(p, m, g))
        if key is None:
            return y
        _YARD[key] = y
    return _YARD[key]
