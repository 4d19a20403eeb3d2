"""Extended-precision model of ONE linearisation and ONE damped step of the local bundle adjustment (test helper, CPU only).

A plain, slow restatement in numpy.longdouble (80-bit x87: eps 1.08e-19) of what one LM iteration computes, used as the common
reference of the stage tests (test_ba_stages_host.py, test_gpu_ba_stages.py):

  residual (bundle_adjustment.jl:23-30, RotZYX):  X = Rz(t1) Ry(t2) Rx(t3) l + t,   r = (py - (fy X_y / X_z + cy), px - (fx X_x / X_z + cx))
  Jacobians     complex step in clongdouble (h = 1e-40: the truncation term h^2 is far below the type's eps)
  build         U, V, W, S = U - W (V + D_l)^-1 W', g = Jp'f - W (V + D_l)^-1 Jl'f, ud = diag(U), ssr  -- for an outlier mask,
                constant poses and a point range [lo, hi) (a shard); D = clamp(diag, 1e-6, 1e32) * inv_delta (the LM damping rule)
  step          the FULL damped normal equations (J'J + D) [dp ; dl] = J'f over the free poses and all points, solved densely by a
                hand-written Cholesky: no Schur complement, no banding, no pose order enters the step
  LM rule       rho = (trial - ssr) / (predicted - ssr) > 1e-3 accepts; delta <- delta / max(1/3, 1 - (2 rho - 1)^3) (orc_ba.c lm_optimize)

Nothing here is shared with the oracle, np_ba.py or the kernels.  The second half of the module holds the error measures and the
assertion functions of the stage tests: every scale comes from the model, never from the quantity under test."""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble
LM_MIN_DIAGONAL, LM_MAX_DIAGONAL = LD(1e-6), LD(1e32)
LM_DELTA0, LM_MIN_STEP_QUALITY, LM_XTOL = 10.0, 1e-3, 1e-8
LM_MAX_DELTA = 1e16
F64_FLOOR = 4.0 * 2.0 ** -52
# the asserted k per stage: 4 x the largest measured r = E_hip / max(E_orc, E_np, 4 * 2^-52) of that stage (tables: DESIGN.md, "stage tests",
# and the docstring of test_gpu_ba_stages.py); test_ba_stages_host.py proves that every sensitivity case is still rejected at these k
K = dict(build=7.2, solve=16.6, step=8.6)
_H = LD(1e-40)


def _residual(cam, pose, pt, px):
    """pose (O,6), pt (O,3), px (O,2) as (y,x), any of longdouble / clongdouble -> (O,2), and the camera-frame depth"""
    fx, fy, cx, cy = (LD(c) for c in cam)
    a, b, c = pose[:, 0], pose[:, 1], pose[:, 2]
    x, y, z = pt[:, 0], pt[:, 1], pt[:, 2]
    # Rx(c) first, then Ry(b), then Rz(a): the product Rz Ry Rx applied factor by factor
    y1, z1 = np.cos(c) * y - np.sin(c) * z, np.sin(c) * y + np.cos(c) * z
    x2, z2 = np.cos(b) * x + np.sin(b) * z1, -np.sin(b) * x + np.cos(b) * z1
    x3, y3 = np.cos(a) * x2 - np.sin(a) * y1, np.sin(a) * x2 + np.cos(a) * y1
    X, Y, Z = x3 + pose[:, 3], y3 + pose[:, 4], z2 + pose[:, 5]
    return np.stack([px[:, 0] - (fy * Y / Z + cy), px[:, 1] - (fx * X / Z + cx)], 1), Z


def _inv3(A):
    """closed-form inverse of (M,3,3) symmetric positive definite blocks (adjugate / determinant)"""
    a, b, c = A[:, 0, 0], A[:, 0, 1], A[:, 0, 2]
    d, e, f = A[:, 1, 0], A[:, 1, 1], A[:, 1, 2]
    g, h, i = A[:, 2, 0], A[:, 2, 1], A[:, 2, 2]
    C = np.empty_like(A)
    C[:, 0, 0] = e * i - f * h; C[:, 0, 1] = c * h - b * i; C[:, 0, 2] = b * f - c * e
    C[:, 1, 0] = f * g - d * i; C[:, 1, 1] = a * i - c * g; C[:, 1, 2] = c * d - a * f
    C[:, 2, 0] = d * h - e * g; C[:, 2, 1] = b * g - a * h; C[:, 2, 2] = a * e - b * d
    det = a * C[:, 0, 0] + b * C[:, 1, 0] + c * C[:, 2, 0]
    return C / det[:, None, None]


def cholesky_solve(A, b):
    """x with A x = b, A symmetric positive definite (longdouble): right-looking Cholesky by numpy row operations, two triangular sweeps"""
    n = len(b)
    L = np.array(A, dtype=LD, copy=True)
    for k in range(n):
        if not L[k, k] > 0:
            raise ArithmeticError(f"hp_ba.cholesky_solve: pivot {k} is not positive")
        L[k, k] = np.sqrt(L[k, k])
        L[k + 1:, k] /= L[k, k]
        L[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k + 1:, k])
    y = np.array(b, dtype=LD, copy=True)
    for k in range(n):
        y[k] /= L[k, k]
        y[k + 1:] -= L[k + 1:, k] * y[k]
    for k in range(n - 1, -1, -1):
        y[k] /= L[k, k]
        y[:k] -= L[k, :k] * y[k]
    return y


def _damping(diag, inv_delta):
    return np.clip(diag, LM_MIN_DIAGONAL, LM_MAX_DIAGONAL) * LD(inv_delta)


class Model:
    """One BA window in the flat layout of the entry points: theta = [6P ; 3M], pixels (O,2) (y,x), 1-based ids."""

    def __init__(self, cam, theta, theta_const, pixels_yx, pose_ids, point_ids):
        self.cam = tuple(float(c) for c in cam)
        self.const = np.asarray(theta_const).astype(bool)
        self.P = len(self.const)
        self.theta = np.asarray(theta, dtype=np.float64).astype(LD)
        self.M = (len(self.theta) - 6 * self.P) // 3
        self.px = np.asarray(pixels_yx, dtype=np.float64).reshape(-1, 2).astype(LD)
        self.pi = np.asarray(pose_ids, dtype=np.int64) - 1
        self.li = np.asarray(point_ids, dtype=np.int64) - 1
        self.O = len(self.pi)
        self.outl = np.zeros(self.O, dtype=bool)

    # ---- linearisation ----
    def _split(self, theta):
        return theta[:6 * self.P].reshape(self.P, 6), theta[6 * self.P:].reshape(self.M, 3)

    def residuals(self, theta=None):
        poses, pts = self._split(self.theta if theta is None else theta)
        return _residual(self.cam, poses[self.pi], pts[self.li], self.px)

    def linearise(self, ignore):
        """f (O,2), Jp (O,2,6), Jl (O,2,3): rows of ignored outliers zeroed, Jp of constant poses zeroed"""
        poses, pts = self._split(self.theta)
        po, lo = poses[self.pi].astype(CLD), pts[self.li].astype(CLD)
        pxc = self.px.astype(CLD)
        f = _residual(self.cam, poses[self.pi], pts[self.li], self.px)[0]
        Jp = np.zeros((self.O, 2, 6), dtype=LD); Jl = np.zeros((self.O, 2, 3), dtype=LD)
        for k in range(6):
            q = po.copy(); q[:, k] += 1j * _H
            Jp[:, :, k] = _residual(self.cam, q, lo, pxc)[0].imag / _H
        for k in range(3):
            q = lo.copy(); q[:, k] += 1j * _H
            Jl[:, :, k] = _residual(self.cam, po, q, pxc)[0].imag / _H
        act = ~(self.outl & bool(ignore))
        f = f * act[:, None]; Jl = Jl * act[:, None, None]
        Jp = Jp * (act & ~self.const[self.pi])[:, None, None]
        return f, Jp, Jl

    def flag_outliers(self, repr_eps, depth_eps=1e-6):
        f, z = self.residuals()
        self.outl = np.asarray((z < LD(depth_eps)) | ((f * f).sum(1) > LD(repr_eps)))
        # distance of the closest observation to either threshold: a test may only compare flags that rounding cannot flip
        self.flag_margin = float(min(np.abs((f * f).sum(1) - LD(repr_eps)).min(initial=np.inf), np.abs(z - LD(depth_eps)).min(initial=np.inf)))
        return int(self.outl.sum())

    # ---- build stage ----
    def build(self, ignore, inv_delta, lo=0, hi=None):
        """the contribution of the points [lo, hi) to the reduced camera system: dict S (6P,6P), g, ud, ssr in longdouble"""
        hi = self.M if hi is None else hi
        P, M, n = self.P, self.M, 6 * self.P
        f, Jp, Jl = self.linearise(ignore)
        sel = np.flatnonzero((self.li >= lo) & (self.li < hi))
        U = np.zeros((n, n), dtype=LD); W = np.zeros((n, 3 * M), dtype=LD)
        V = np.zeros((M, 3, 3), dtype=LD); bl = np.zeros((M, 3), dtype=LD); bp = np.zeros(n, dtype=LD)
        for o in sel:
            p, j = self.pi[o], self.li[o]
            U[6 * p:6 * p + 6, 6 * p:6 * p + 6] += Jp[o].T @ Jp[o]
            W[6 * p:6 * p + 6, 3 * j:3 * j + 3] += Jp[o].T @ Jl[o]
            V[j] += Jl[o].T @ Jl[o]
            bl[j] += Jl[o].T @ f[o]; bp[6 * p:6 * p + 6] += Jp[o].T @ f[o]
        d = _damping(np.einsum("mii->mi", V), inv_delta)
        Vd = V.copy()
        for a in range(3):
            Vd[:, a, a] += d[:, a]
        Vi = _inv3(Vd)
        Vi[:lo] = 0; Vi[hi:] = 0
        WV = np.einsum("amk,mkl->aml", W.reshape(n, M, 3), Vi).reshape(n, 3 * M)
        S = U - WV @ W.T
        g = bp - WV @ bl.reshape(-1)
        return dict(S=S, g=g, ud=np.diag(U).copy(), ssr=(f[sel] * f[sel]).sum(dtype=LD))

    def build_blocks(self, ignore, inv_delta, pairs):
        """the same reduced system block by block, for windows too large for build()'s dense W: S_pq for the listed pose pairs, g_p and
        ud_p for every pose named in them, ssr.  Per pose and point the sums T_pj = sum_o W_o (V_j + D_j)^-1 and W_pj, then
        S_pq = [p = q] U_p - sum_j T_pj W_qj'."""
        f, Jp, Jl = self.linearise(ignore)
        M = self.M
        V = np.zeros((M, 3, 3), dtype=LD); bl = np.zeros((M, 3), dtype=LD)
        np.add.at(V, self.li, np.einsum("oka,okb->oab", Jl, Jl)); np.add.at(bl, self.li, np.einsum("oka,ok->oa", Jl, f))
        d = _damping(np.einsum("mii->mi", V), inv_delta)
        for a in range(3):
            V[:, a, a] += d[:, a]
        Vi = _inv3(V)
        per_pose = {}
        for p in sorted({p for pq in pairs for p in pq}):
            o = np.flatnonzero(self.pi == p)
            Wo = np.einsum("oka,okb->oab", Jp[o], Jl[o])
            Wp = np.zeros((M, 6, 3), dtype=LD); np.add.at(Wp, self.li[o], Wo)
            Tp = np.einsum("mab,mbc->mac", Wp, Vi)
            U = np.einsum("oka,okb->ab", Jp[o], Jp[o])
            per_pose[p] = (Wp, Tp, U, np.einsum("oka,ok->a", Jp[o], f[o]) - np.einsum("mab,mb->a", Tp, bl))
        S = {(p, q): (per_pose[p][2] if p == q else 0) - np.einsum("mac,mbc->ab", per_pose[p][1], per_pose[q][0]) for p, q in pairs}
        return dict(S=S, g={p: v[3] for p, v in per_pose.items()}, ud={p: np.diag(v[2]).copy() for p, v in per_pose.items()}, ssr=(f * f).sum(dtype=LD))

    # ---- one damped step from the full normal equations ----
    def step(self, ignore, inv_delta):
        """dx (6P + 3M; zero for constant poses), theta_new = theta - dx, trial_ssr, predicted_ssr, maxdx, ssr"""
        P, M = self.P, self.M
        f, Jp, Jl = self.linearise(ignore)
        free = np.flatnonzero(~self.const)
        slot = np.full(P, -1); slot[free] = np.arange(len(free))
        nf = 6 * len(free); N = nf + 3 * M
        A = np.zeros((N, N), dtype=LD); b = np.zeros(N, dtype=LD)
        for o in range(self.O):
            j = nf + 3 * self.li[o]
            A[j:j + 3, j:j + 3] += Jl[o].T @ Jl[o]; b[j:j + 3] += Jl[o].T @ f[o]
            s = slot[self.pi[o]]
            if s >= 0:
                A[6 * s:6 * s + 6, 6 * s:6 * s + 6] += Jp[o].T @ Jp[o]; b[6 * s:6 * s + 6] += Jp[o].T @ f[o]
                A[6 * s:6 * s + 6, j:j + 3] += Jp[o].T @ Jl[o]; A[j:j + 3, 6 * s:6 * s + 6] += Jl[o].T @ Jp[o]
        A[np.diag_indices(N)] += _damping(np.diag(A), inv_delta)
        x = cholesky_solve(A, b)
        dx = np.zeros(6 * P + 3 * M, dtype=LD)
        dpm = dx[:6 * P].reshape(P, 6); dpm[free] = x[:nf].reshape(-1, 6)
        dx[6 * P:] = x[nf:]
        dlm = dx[6 * P:].reshape(M, 3)
        theta_new = self.theta - dx
        act = ~(self.outl & bool(ignore))
        ft = self.residuals(theta_new)[0] * act[:, None]
        pred = np.einsum("oka,oa->ok", Jp, dpm[self.pi]) + np.einsum("oka,oa->ok", Jl, dlm[self.li]) - f
        return dict(dx=dx, theta_new=theta_new, trial_ssr=(ft * ft).sum(dtype=LD), predicted_ssr=(pred * pred).sum(dtype=LD),
                    maxdx=np.abs(dx).max(initial=LD(0)), ssr=(f * f).sum(dtype=LD))

    def lm_steps(self, steps, ignore=0):
        """`steps` iterations of the LM outer loop from delta0 (orc_ba.c lm_optimize, without the convergence tests: the stage
        tests use windows whose steps are far from converged).  Returns the list of (accepted, rho, delta used, step dict)."""
        delta, decrease, log = LM_DELTA0, 2.0, []
        for _ in range(steps):
            st = self.step(ignore, 1.0 / delta)
            rho = float((st["trial_ssr"] - st["ssr"]) / (st["predicted_ssr"] - st["ssr"]))
            ok = rho > LM_MIN_STEP_QUALITY
            log.append((ok, rho, delta, st))
            if ok:
                self.theta = st["theta_new"]
                u = 2.0 * rho - 1.0
                delta = min(delta / max(1.0 / 3.0, 1.0 - u * u * u), LM_MAX_DELTA); decrease = 2.0
            else:
                delta = max(delta / decrease, 1e-16); decrease *= 2.0
        return log


# ---------------------------------------------------------------------------------------------------------------------------
# error measures (the scale always comes from the model) and the assertion functions shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------
def unpack_reduce(buf, P):
    """[S (6P x 6P, column-major) ; g ; ud ; ssr ; pad] -> dict"""
    n = 6 * P
    buf = np.asarray(buf)
    return dict(S=buf[:n * n].reshape(n, n, order="F"), g=buf[n * n:n * n + n], ud=buf[n * n + n:n * n + 2 * n], ssr=buf[n * n + 2 * n])


def pack_reduce(m, P):
    """a build dict (model or f64) rounded to the f64 reduce buffer of slam_ba_build"""
    n = 6 * P
    out = np.zeros(n * n + 2 * n + 8)
    out[:n * n] = np.asarray(m["S"], dtype=np.float64).reshape(-1, order="F")
    out[n * n:n * n + n] = m["g"]; out[n * n + n:n * n + 2 * n] = m["ud"]; out[n * n + 2 * n] = m["ssr"]
    return out


def _rel(x, ref):
    x, ref = np.asarray(x, dtype=LD), np.asarray(ref, dtype=LD)
    nz = ref != 0
    if (x[~nz] != 0).any():
        return np.inf
    return float((np.abs(x[nz] - ref[nz]) / np.abs(ref[nz])).max(initial=LD(0)))


def build_errors(x, m, scale=None):
    """x: S / g / ud / ssr under test, m: the model's.  S scaled by sqrt(ud*_i ud*_j), g by sqrt(ud*_i ssr*), ud and ssr relative;
    where the scale is zero the entry must be exactly zero (inf otherwise).  scale: the model's build of the WHOLE window when x and m
    are one shard's contribution (a shard's own ud can vanish where its S does not: the scale of S and g is the window's)."""
    sc_m = m if scale is None else scale
    ud = np.asarray(sc_m["ud"], dtype=LD)
    sc = np.sqrt(np.outer(ud, ud))
    dS = np.abs(np.asarray(x["S"], dtype=LD) - m["S"])
    e = {}
    e["S"] = np.inf if (np.asarray(x["S"])[sc == 0] != 0).any() else float((dS[sc > 0] / sc[sc > 0]).max(initial=LD(0)))
    sg = np.sqrt(ud * sc_m["ssr"])
    dg = np.abs(np.asarray(x["g"], dtype=LD) - m["g"])
    e["g"] = np.inf if (np.asarray(x["g"])[sg == 0] != 0).any() else float((dg[sg > 0] / sg[sg > 0]).max(initial=LD(0)))
    e["ud"] = _rel(x["ud"], m["ud"])
    e["ssr"] = _rel(x["ssr"], m["ssr"])
    return e


def block_errors(x, mb):
    """build_errors on the sub-sampled blocks of Model.build_blocks: x a full f64 build (S, g, ud, ssr), mb the model's blocks"""
    blk = lambda A, p, q: np.asarray(A, dtype=LD)[6 * p:6 * p + 6, 6 * q:6 * q + 6]
    vec = lambda a, p: np.asarray(a, dtype=LD)[6 * p:6 * p + 6]
    e = dict(S=0.0, g=0.0, ud=0.0)
    for (p, q), Sm in mb["S"].items():
        sc = np.sqrt(np.outer(mb["ud"][p], mb["ud"][q]))
        d = np.abs(blk(x["S"], p, q) - Sm)
        e["S"] = np.inf if (blk(x["S"], p, q)[sc == 0] != 0).any() else max(e["S"], float((d[sc > 0] / sc[sc > 0]).max(initial=LD(0))))
    for p, gm in mb["g"].items():
        sg = np.sqrt(mb["ud"][p] * mb["ssr"])
        d = np.abs(vec(x["g"], p) - gm)
        e["g"] = np.inf if (vec(x["g"], p)[sg == 0] != 0).any() else max(e["g"], float((d[sg > 0] / sg[sg > 0]).max(initial=LD(0))))
        e["ud"] = max(e["ud"], _rel(vec(x["ud"], p), mb["ud"][p]))
    e["ssr"] = _rel(x["ssr"], mb["ssr"])
    return e


def step_errors(x, m, P):
    """x: dict with dx (6P + 3M) and optionally trial_ssr / predicted_ssr / maxdx, m: Model.step's.  The step per 6-block (pose) and
    3-block (point), max-norm, relative to max(|dx*| of that block, LM_XTOL); the scalars relative."""
    dxm = np.asarray(m["dx"], dtype=LD)
    d = np.abs(np.asarray(x["dx"], dtype=LD) - dxm)
    e = {}
    for name, sl, w in (("dp", slice(0, 6 * P), 6), ("dl", slice(6 * P, None), 3)):
        err, ref = d[sl].reshape(-1, w).max(1, initial=LD(0)), np.abs(dxm[sl]).reshape(-1, w).max(1, initial=LD(0))
        e[name] = float((err / np.maximum(ref, LD(LM_XTOL))).max(initial=LD(0)))
    for name in ("trial_ssr", "predicted_ssr", "maxdx", "ssr"):
        if name in x:
            e[name] = _rel(x[name], m[name])
    return e


def bounds(k, *yardsticks):
    """k * max(E_orc, E_np, 4 * 2^-52) per measure (over the yardsticks that have the measure).  max|dx| is ONE entry of the step, and
    whether a reference happens to hit that entry to the last bit is chance: its yardstick is the larger of the references' maxdx, dp
    and dl errors (the entry's relative error is bounded by the step error of its block)."""
    keys = set().union(*yardsticks)
    ref = {q: max(max(y[q] for y in yardsticks if q in y), F64_FLOOR) for q in keys}
    if "maxdx" in ref:
        ref["maxdx"] = max(ref[q] for q in ("maxdx", "dp", "dl") if q in ref)
    return {q: k * ref[q] for q in keys}


def ratios(e, *yardsticks):
    """r = E / max(E_orc, E_np, 4 * 2^-52) per measure: what the tables in DESIGN.md record"""
    b = bounds(1.0, *yardsticks)
    return {q: e[q] / b[q] for q in b if q in e}


def asymmetry(S, m):
    """(max |S_ij - S_ji| / sqrt(ud*_i ud*_j) over the DIAGONAL 6 x 6 blocks, the same over the off-diagonal blocks), scales from the model"""
    S = np.asarray(S, dtype=LD)
    ud = np.asarray(m["scale"]["ud"] if "scale" in m else m["ud"], dtype=LD)
    sc = np.sqrt(np.outer(ud, ud))
    D = np.abs(S - S.T)
    if (D[sc == 0] != 0).any():
        return np.inf, np.inf
    R = np.zeros_like(D); R[sc > 0] = D[sc > 0] / sc[sc > 0]
    P = len(ud) // 6
    B = R.reshape(P, 6, P, 6).max((1, 3))
    return float(np.diag(B).max(initial=LD(0))), float((B - np.diag(np.diag(B))).max(initial=LD(0)))


def structure_errors(S, hb, const):
    """zeros outside the block band `hb`, zeros in rows / columns of constant poses: a list of complaints (empty = fine)"""
    S = np.asarray(S)
    P = len(const)
    out = []
    B = np.abs(S).reshape(P, 6, P, 6).max((1, 3))
    pp, qq = np.nonzero(B)
    if len(pp) and (np.abs(pp - qq) > hb).any():
        w = np.argmax(np.abs(pp - qq))
        out.append(f"S has a non-zero block ({pp[w]}, {qq[w]}) outside the half-bandwidth {hb}")
    c = np.asarray(const).astype(bool)
    if B[c].any() or B[:, c].any():
        out.append("S is non-zero in a row / column of a constant pose")
    return out


def check(label, e, bound, only=None):
    """the one assertion of the stage tests: every measure in `bound` (or: every measure named in `only`) is present in `e` and within
    its bound"""
    if only is not None:
        bound = {q: bound[q] for q in only}
    bad = {q: (e.get(q, np.nan), bound[q]) for q in bound if not (e.get(q, np.nan) <= bound[q])}          # (a missing measure fails)
    assert not bad, f"{label}: " + ", ".join(f"{q} = {v[0]:.3e} > bound {v[1]:.3e}" for q, v in sorted(bad.items()))


# ---------------------------------------------------------------------------------------------------------------------------
# the window families of the stage tests (small: the full-system step of the model is O(n^3) in Python)
# ---------------------------------------------------------------------------------------------------------------------------
def relabel(s, order):
    """the scene with its poses relabelled: position k of the new window is the caller's pose order[k]"""
    order = np.asarray(order, dtype=np.int64)
    P = s["P"]
    new_of = np.empty(P, dtype=np.int64); new_of[order] = np.arange(P)
    t = dict(s)
    t["theta0"] = np.concatenate([s["theta0"][:6 * P].reshape(P, 6)[order].ravel(), s["theta0"][6 * P:]])
    t["theta_const"] = np.asarray(s["theta_const"])[order].copy()
    t["pose_ids"] = new_of[s["pose_ids"] - 1] + 1
    return t


def with_const(s, const_poses):
    t = dict(s)
    c = np.zeros(s["P"], dtype=np.uint8); c[list(const_poses)] = 1
    t["theta_const"] = c
    return t


def ragged_window(syn, seed=31):
    """P = 14, constant poses scattered (0, 5, 6, 13: the free span is shorter than the window at both ends); observations removed so that
    the window holds points with ONE observation, points seen ONLY by constant poses, an orphan point (no observation), a free pose with
    no observation; observation order shuffled.  `props` names the points / the pose: the tests assert each property."""
    s = with_const(syn.ba_scene(P=14, M=90, obs_per_point=5, seed=seed), (0, 5, 6, 13))
    rng = np.random.default_rng(seed)
    pose, pt = s["pose_ids"] - 1, s["point_ids"] - 1
    keep = np.ones(s["O"], dtype=bool)
    empty_pose = 9
    keep &= pose != empty_pose
    const = s["theta_const"].astype(bool)
    pts_in = lambda f: [j for j in range(s["M"]) if f(pose[(pt == j) & keep])]
    orphan = pts_in(lambda q: len(q) >= 3)[0]
    keep &= pt != orphan
    singles = [j for j in pts_in(lambda q: len(q) >= 3 and not const[q[0]]) if j != orphan][:3]
    for j in singles:
        idx = np.flatnonzero((pt == j) & keep); keep[idx[1:]] = False
    const_only = [j for j in pts_in(lambda q: const[q].sum() >= 1 and len(q) >= 2) if j not in singles and j != orphan][:3]
    for j in const_only:
        idx = np.flatnonzero((pt == j) & keep); keep[idx[~const[pose[idx]]]] = False
    order = rng.permutation(np.flatnonzero(keep))
    s["pose_ids"], s["point_ids"] = s["pose_ids"][order], s["point_ids"][order]
    s["pixels_yx"] = np.ascontiguousarray(s["pixels_yx"][order]); s["O"] = len(order)
    s["props"] = dict(orphan=orphan, singles=singles, const_only=const_only, empty_pose=empty_pose)
    return s


def stage_windows(syn):
    """name -> scene.  ba_scene's points are seen by `obs_per_point` consecutive key-frames: block half-bandwidth obs_per_point - 1."""
    w = {}
    for hb, P in ((1, 12), (9, 30), (14, 24), (15, 26), (16, 26), (17, 26), (18, 26), (20, 28)):
        w[f"hb{hb}"] = syn.ba_scene(P=P, M=120 if hb > 1 else 160, obs_per_point=hb + 1, seed=20 + hb)
    w["hb21_dense"] = syn.ba_scene(P=30, M=120, obs_per_point=22, seed=41)        # 29 free poses in a row: <= DS_MAXF = 30
    w["hb21_tiled"] = syn.ba_scene(P=34, M=120, obs_per_point=22, seed=42)        # 33 free poses: beyond the dense solver, beyond the band
    for P in (16, 17, 32):                                                         # 6P = 96 / 102 / 192: on and around the 32-wide tiles
        w[f"p{P}"] = syn.ba_scene(P=P, M=5 * P, obs_per_point=5, seed=50 + P)
    w["loop"] = syn.ba_scene_loop(P=24, M=100, seed=61, n_loop=12, k_loop=3, obs_per_point=6)
    w["const_first"] = syn.ba_scene(P=20, M=100, obs_per_point=8, seed=62, n_const=6)
    w["const_scattered"] = with_const(syn.ba_scene(P=20, M=100, obs_per_point=8, seed=63), (0, 3, 4, 9, 15, 19))
    w["const_most"] = syn.ba_scene(P=25, M=120, obs_per_point=10, seed=64, n_const=20)
    w["ragged"] = ragged_window(syn)
    return w


def batch_windows(syn):
    """the extra windows of the batch tests: a second window of <= 5 free poses in a row (k_ba_window's shape), and a wide band with
    three observations per point (first, last and one observer between of 19 consecutive key-frames): half-bandwidth 18"""
    w = {"small": syn.ba_scene(P=12, M=60, obs_per_point=5, seed=71, n_const=8)}
    s = syn.ba_scene(P=26, M=150, obs_per_point=19, seed=72)
    rng = np.random.default_rng(72)
    keep = np.zeros(s["O"], dtype=bool)
    for j in range(s["M"]):
        idx = np.flatnonzero(s["point_ids"] - 1 == j)
        keep[[idx[0], idx[-1], idx[rng.integers(1, len(idx) - 1)]]] = True
    for key in ("pose_ids", "point_ids"):
        s[key] = s[key][keep]
    s["pixels_yx"] = np.ascontiguousarray(s["pixels_yx"][keep]); s["O"] = int(keep.sum())
    w["wide_sparse"] = s
    return w


def big_window(syn):
    """the 50 key-frame / 1e5 observation window of the benchmarks (build stage only), and the sub-sample of blocks the model forms:
    diagonal, first off-diagonal, mid-band and edge-of-band (hb = 9) blocks at the start, in the middle and at the end of the window"""
    pairs = [(p, p + d) for p in (1, 7, 24, 40) for d in (0, 1, 5, 9)] + [(49, 49), (40, 49)]
    return syn.ba_scene(P=50, M=10000, seed=3), pairs


def scene_args(s):
    return s["cam"], s["theta0"], s["theta_const"], s["pixels_yx"], s["pose_ids"], s["point_ids"]


# ---------------------------------------------------------------------------------------------------------------------------
# the yardsticks: what the two f64 implementations of the host (the C oracle, np_ba.py) achieve against the model on a window
# ---------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def np_shard(s, lo=0, hi=None):
    hi = s["M"] if hi is None else hi
    P = s["P"]
    sel = np.flatnonzero((s["point_ids"] - 1 >= lo) & (s["point_ids"] - 1 < hi))
    th = np.concatenate([s["theta0"][:6 * P], s["theta0"][6 * P + 3 * lo:6 * P + 3 * hi]])
    import np_ba
    return np_ba.NumpyShard(s["cam"], P, th, s["theta_const"], s["pixels_yx"][sel], s["pose_ids"][sel], s["point_ids"][sel] - lo)


def orc_build(orc, s, outl, ignore, inv_delta, lo=0, hi=None):
    S, g, ud, ssr = orc.ba_reduced_system(*scene_args(s), np.asarray(outl, dtype=np.uint8), ignore, inv_delta, lo, s["M"] if hi is None else hi)
    return dict(S=S, g=g, ud=ud, ssr=ssr)


def build_yardsticks(orc, s, key, ignore=0, inv_delta=0.1, outl=None, lo=0, hi=None):
    """(model build, E_orc, E_np, the oracle's f64 build, the NumpyShard after build) of the points [lo, hi) of a window; key: the
    cache key of the window (None: not cached).  A shard's S and g are measured on the scale of the whole window."""
    key = None if key is None else ("build", key, ignore, inv_delta, lo, hi)
    if key not in _CACHE:
        m = Model(*scene_args(s))
        ns = np_shard(s, lo, hi)
        if outl is not None:
            m.outl = np.asarray(outl, dtype=bool).copy()
            ns.outl = m.outl[(s["point_ids"] - 1 >= lo) & (s["point_ids"] - 1 < (s["M"] if hi is None else hi))]
        b = m.build(ignore, inv_delta, lo, hi)
        whole = b if (lo == 0 and hi in (None, s["M"])) else m.build(ignore, inv_delta)
        b["scale"] = dict(ud=whole["ud"], ssr=whole["ssr"])
        o = orc_build(orc, s, m.outl, ignore, inv_delta, lo, hi)
        n = unpack_reduce(ns.build(ignore, inv_delta).numpy().copy(), s["P"])
        res = (b, build_errors(o, b, b["scale"]), build_errors(n, b, b["scale"]), o, ns)
        if key is None:
            return res
        _CACHE[key] = res
    return _CACHE[key]


def big_yardsticks(orc, syn):
    """(scene, model blocks, E_orc on them, the oracle's whole f64 build) of big_window; np_ba's Python loops are out of reach at this
    size, so the yardstick is the oracle's alone"""
    if "big" not in _CACHE:
        s, pairs = big_window(syn)
        mb = Model(*scene_args(s)).build_blocks(0, 1.0 / LM_DELTA0, pairs)
        o = orc_build(orc, s, np.zeros(s["O"]), 0, 1.0 / LM_DELTA0)
        _CACHE["big"] = (s, mb, block_errors(o, mb), o)
    return _CACHE["big"]


def step_yardsticks(orc, s, key, outl=None):
    """(model step at delta0, E_orc, E_np, np_ba's f64 step dict).  The oracle's step is its one-iteration run (first pass: all
    observations), so with outlier flags (ignore_outliers = 1) only np_ba's is available and E_orc is empty.  The step must be an
    accepted one (asserted)."""
    key = None if key is None else ("step", key, outl is not None)
    if key not in _CACHE:
        ignore = int(outl is not None)
        m = Model(*scene_args(s))
        ns = np_shard(s)
        if outl is not None:
            m.outl = np.asarray(outl, dtype=bool).copy(); ns.outl = m.outl.copy()
        st = m.step(ignore, 1.0 / LM_DELTA0)
        st["rho"] = float((st["trial_ssr"] - st["ssr"]) / (st["predicted_ssr"] - st["ssr"]))
        assert st["rho"] > LM_MIN_STEP_QUALITY, f"{key}: the model rejects the first step (rho = {st['rho']}): pick another seed"
        tr = ns.solve(ns.build(ignore, 0.1), 0.1).numpy().copy(); ns.commit(1)
        xn = dict(dx=s["theta0"] - ns.download()[0], trial_ssr=tr[0], predicted_ssr=tr[1], maxdx=tr[2], ssr=float(ns.red[-8]))
        e_orc = {}
        if outl is None:
            th, _, so = orc.bundle_adjustment(*scene_args(s), iters_fast=1, iterations=0)
            assert so["iters_pass1"] == 1 and not np.array_equal(th, s["theta0"]), f"{key}: the oracle rejected the step the model accepts"
            e_orc = step_errors(dict(dx=s["theta0"] - th, trial_ssr=so["ssr_pass1"], ssr=so["ssr_init"]), st, s["P"])
        res = (st, e_orc, step_errors(xn, st, s["P"]), xn)
        if key is None:
            return res
        _CACHE[key] = res
    return _CACHE[key]


def lm2_yardsticks(orc, s, key):
    """TWO LM iterations from delta0: (model's last step dict with dx = theta0 - theta after both, E_orc, E_np).  The second step's
    damping is delta0 / max(1/3, 1 - (2 rho - 1)^3): it carries the first step's predicted cost."""
    key = ("lm2", key)
    if key not in _CACHE:
        m = Model(*scene_args(s))
        log = m.lm_steps(2)
        assert all(ok for ok, *_ in log), f"{key}: a step of the two is rejected: pick another seed"
        ref = dict(log[1][3], dx=s["theta0"].astype(LD) - m.theta, ssr=log[0][3]["ssr"])
        th, _, so = orc.bundle_adjustment(*scene_args(s), iters_fast=2, iterations=0)
        assert so["iters_pass1"] == 2
        e_orc = step_errors(dict(dx=s["theta0"] - th, trial_ssr=so["ssr_pass1"], ssr=so["ssr_init"]), ref, s["P"])
        ns = np_shard(s)
        delta = LM_DELTA0
        for _ in range(2):
            red = ns.build(0, 1.0 / delta); ssr = float(red[-8])
            tr = ns.solve(red, 1.0 / delta).numpy().copy(); ns.commit(1)
            u = 2.0 * (tr[0] - ssr) / (tr[1] - ssr) - 1.0
            delta = min(delta / max(1.0 / 3.0, 1.0 - u * u * u), LM_MAX_DELTA)
        e_np = step_errors(dict(dx=s["theta0"] - ns.download()[0], trial_ssr=tr[0]), ref, s["P"])
        _CACHE[key] = (ref, e_orc, e_np)
    return _CACHE[key]
