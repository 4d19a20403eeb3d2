"""pnp_bundle_adjustment (bundle_adjustment.jl:113-171) in plain Float64 numpy (test helper, CPU only): the counterpart of np_ba.py.

Two uses.  (1) The second yardstick of the pose-refinement tests: what a straightforward f64 implementation with ANALYTIC Jacobians and
numpy's own Cholesky achieves against the long-double model (hp_pnp.py), next to the C oracle.  (2) The mutation carrier: `fault=`
switches on ONE wrong formula, and test_pnp_model_host.py proves that the assertion of the GPU test rejects each of them:

  a   the last observation is left out of every reduction          f   `decrease` is not reset to 2 after an accepted step
  b   the damping uses the unclamped diagonal                       g   pass 2 does not skip the flagged points
  c   the outlier test is on |r| instead of r^2                     h   predicted is formed with J dx + r
  d   n - no <= 5 instead of < 5                                    i   the Jacobian is not rebuilt after an accepted step
  e   the delta update without the cube                             i2  the Jacobian is rebuilt after a REJECTED step, at the trial point
                                                                    j   theta3 is taken from the transposed rotation

Nothing here is shared with hp_pnp.py, the oracle or the kernels."""
import numpy as np

FAULTS = ("a", "b", "c", "d", "e", "f", "g", "h", "i", "i2", "j")
DELTA0, MIN_QUALITY, XTOL, FTOL, MIN_DIAG, MAX_DIAG, MAX_DELTA, MIN_DELTA = 10.0, 1e-3, 1e-8, 1e-8, 1e-6, 1e32, 1e16, 1e-16


def angles(pose, fault=None):
    R = np.asarray(pose, dtype=np.float64)
    t1 = np.arctan2(R[1, 0], R[0, 0])
    s1, c1 = np.sin(t1), np.cos(t1)
    t2 = np.arctan2(-R[2, 0], np.hypot(R[0, 0], R[1, 0]))
    if fault == "j":
        R = R[:3, :3].T
    t3 = np.arctan2(R[0, 2] * s1 - R[1, 2] * c1, R[1, 1] * c1 - R[0, 1] * s1)
    return np.array([t1, t2, t3, pose[0][3], pose[1][3], pose[2][3]], dtype=np.float64)


def _rot3(x):
    s1, c1, s2, c2, s3, c3 = np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]), np.sin(x[2]), np.cos(x[2])
    Rz = np.array([[c1, -s1, 0], [s1, c1, 0], [0, 0, 1.0]]); dRz = np.array([[-s1, -c1, 0], [c1, -s1, 0], [0, 0, 0.0]])
    Ry = np.array([[c2, 0, s2], [0, 1.0, 0], [-s2, 0, c2]]); dRy = np.array([[-s2, 0, c2], [0, 0.0, 0], [-c2, 0, -s2]])
    Rx = np.array([[1.0, 0, 0], [0, c3, -s3], [0, s3, c3]]); dRx = np.array([[0.0, 0, 0], [0, -s3, -c3], [0, c3, -s3]])
    return Rz @ Ry @ Rx, (dRz @ Ry @ Rx, Rz @ dRy @ Rx, Rz @ Ry @ dRx)


def residuals(cam, x, px, pts, jac=False):
    """r (n,2) (y, x), depth (n,), and with jac the analytic (n,2,6) Jacobian of r"""
    fx, fy, cx, cy = cam
    R, dR = _rot3(x)
    Xc = pts @ R.T + x[3:]
    X, Y, Z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    r = np.stack([px[:, 0] - (fy * Y / Z + cy), px[:, 1] - (fx * X / Z + cx)], 1)
    if not jac:
        return r, Z
    # d proj / d Xc, rows (y, x); r = px - proj
    P = np.zeros((len(pts), 2, 3))
    P[:, 0, 1] = fy / Z; P[:, 0, 2] = -fy * Y / (Z * Z)
    P[:, 1, 0] = fx / Z; P[:, 1, 2] = -fx * X / (Z * Z)
    dX = np.zeros((len(pts), 3, 6))
    for k in range(3):
        dX[:, :, k] = pts @ dR[k].T
        dX[:, k, 3 + k] = 1.0
    return r, Z, -np.einsum("nij,njk->nik", P, dX)


def _solve(A, g):
    L = np.linalg.cholesky(A)
    return np.linalg.solve(L.T, np.linalg.solve(L, g))


def lm(cam, x, px, pts, act, iterations, fault=None):
    """-> (x, ssr, trace string)"""
    w = act.copy()
    if fault == "a" and len(w):
        w[-1] = False
    x = x.copy()
    r = residuals(cam, x, px, pts)[0] * w[:, None]
    ssr = float((r * r).sum())
    delta, decrease, need_jac, conv, it, trace = DELTA0, 2.0, True, False, 0, ""
    H = g = Jf = None
    jac_at = x
    while not conv and it < iterations:
        it += 1
        if need_jac:
            J = residuals(cam, jac_at, px, pts, jac=True)[2] * w[:, None, None]
            Jf = J.reshape(-1, 6)
            H, g = Jf.T @ Jf, Jf.T @ r.reshape(-1)
            need_jac = False
        d = np.diag(H) if fault == "b" else np.clip(np.diag(H), MIN_DIAG, MAX_DIAG)
        try:
            dx = _solve(H + np.diag(d / delta), g)
        except np.linalg.LinAlgError:
            break
        xt = x - dx
        rt = residuals(cam, xt, px, pts)[0] * w[:, None]
        trial = float((rt * rt).sum())
        p = Jf @ dx + r.reshape(-1) if fault == "h" else Jf @ dx - r.reshape(-1)
        pred = float((p * p).sum())
        mx = float(np.abs(dx).max())
        with np.errstate(invalid="ignore", divide="ignore"):
            rho = np.float64(trial - ssr) / np.float64(pred - ssr)
        if rho > MIN_QUALITY:
            x_conv = mx <= XTOL
            f_conv = abs(ssr - trial) / (abs(ssr) + FTOL) <= FTOL
            ssr, x, r = trial, xt, rt
            u = 2.0 * rho - 1.0
            delta = min(delta / max(1.0 / 3.0, 1.0 - (u if fault == "e" else u * u * u)), MAX_DELTA)
            if fault != "f":
                decrease = 2.0
            need_jac = fault != "i"
            jac_at = x
            conv = x_conv or f_conv
            trace += "A"
        else:
            delta = max(delta / decrease, MIN_DELTA)
            decrease *= 2.0
            conv = mx <= XTOL
            if fault == "i2":
                need_jac, jac_at = True, xt
            trace += "R"
    return x, ssr, trace


def pnp_ba(cam, pose_cw, pixels_yx, points_xyz, iters_fast=5, iterations=10, depth_eps=1e-6, repr_eps=5.0, fault=None, full=False):
    """-> (new_pose 4x4, initial_error, final_error, outliers, n_outliers), the ABI's tuple; full: + the trace string"""
    assert fault is None or fault in FAULTS
    px = np.asarray(pixels_yx, dtype=np.float64).reshape(-1, 2)
    pts = np.asarray(points_xyz, dtype=np.float64).reshape(-1, 3)
    n = len(px)
    x0 = angles(np.asarray(pose_cw, dtype=np.float64), fault)
    every = np.ones(n, dtype=bool)
    r0 = residuals(cam, x0, px, pts)[0]
    if fault == "a":
        r0 = r0[:-1]
    e0 = float((r0 * r0).sum())
    x1, ssr1, tr1 = lm(cam, x0, px, pts, every, iters_fast, fault)
    r, z = residuals(cam, x1, px, pts)
    r2 = (r * r).sum(1)
    outl = (z < depth_eps) | ((np.sqrt(r2) if fault == "c" else r2) > repr_eps)
    no = int(outl.sum())
    if (n - no <= 5) if fault == "d" else (n - no < 5):
        res = (np.eye(4), e0, ssr1, outl, no)
        return res + (tr1 + "|",) if full else res
    x2, ssr2, tr2 = lm(cam, x1, px, pts, every if fault == "g" else ~outl, iterations, fault)
    T = np.eye(4)
    T[:3, :3] = _rot3(x2)[0]; T[:3, 3] = x2[3:]
    res = (T, e0, ssr2, outl, no)
    return res + (tr1 + "|" + tr2,) if full else res
