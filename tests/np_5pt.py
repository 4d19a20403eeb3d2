"""Independent model of the five-point minimal problem (test infrastructure, plain numpy).

It shares nothing with oracle/orc_5pt.c beyond the definition of the problem: five correspondences q2' E q1 = 0, E in the
null space of the 5x9 epipolar system, det E = 0 and 2 E E'E - tr(E E')E = 0.

  - null space by SVD (orc_5pt.c: Gauss-Jordan + Gram-Schmidt);
  - the ten cubics by generic polynomial arithmetic on monomial dictionaries {(i, j, k): coefficient of x^i y^j z^k}, the
    coefficients accumulated in np.longdouble (orc_5pt.c: index tables in Nister's order, double);
  - degree-ordered monomials  x3 x2y x2z xy2 xyz xz2 y3 y2z yz2 z3 | x2 xy xz y2 yz z2 x y z 1,  reduction to [I | B], the
    action matrix of multiplication by x on the ten low monomials (rows 0-5 = -B[0:6], rows 6-9 the unit rows x.x -> x2,
    x.y -> xy, x.z -> xz, x.1 -> x), its eigenvectors v give (x, y, z) = v[6:9] / v[9]  (orc_5pt.c: the 3x3 polynomial matrix
    B(z), its degree-10 determinant, roots bracketed between the derivative's roots);
  - every solution, complex ones included, is polished by Newton (Gauss-Newton on the ten cubics evaluated from E itself, analytic
    Jacobian, complex extended precision) until its residual stops falling, so the model's own error (<= 1e-15) is negligible
    beside the 1e-6 it judges and the imaginary parts it reports separate real from complex solutions crisply.

Every routine is vectorised over T tuples (leading axis)."""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble
MONO3 = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)]
MONO2 = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
REAL_IMAG, COMPLEX_IMAG, MIN_SEP, MAX_RESIDUAL = 1e-9, 1e-4, 1e-6, 1e-12


# ---- polynomials in (x, y, z): {exponent triple: coefficient array of shape (T,)} ------------------------------------------
def p_add(a, b, sb=1):
    o = dict(a)
    for m, c in b.items():
        o[m] = o[m] + sb * c if m in o else sb * c
    return o


def p_mul(a, b):
    o = {}
    for ma, ca in a.items():
        for mb, cb in b.items():
            m = (ma[0] + mb[0], ma[1] + mb[1], ma[2] + mb[2])
            o[m] = o[m] + ca * cb if m in o else ca * cb
    return o


def p_scale(a, s):
    return {m: s * c for m, c in a.items()}


def nullspace(q1, q2):
    """(T, 5, 2) normalised points of both views -> (T, 4, 3, 3): E = x N[0] + y N[1] + z N[2] + N[3]."""
    q1 = np.asarray(q1, float).reshape(-1, 5, 2); q2 = np.asarray(q2, float).reshape(-1, 5, 2)
    x, y, u, v = q1[..., 0], q1[..., 1], q2[..., 0], q2[..., 1]
    A = np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], -1)
    return np.linalg.svd(A)[2][:, 5:9].reshape(-1, 4, 3, 3)


def cubics(N):
    """The ten cubics as a (T, 10, 20) coefficient matrix in the order MONO3 | MONO2."""
    N = np.asarray(N, LD)
    var = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
    E = [[{var[m]: N[:, m, r, c] for m in range(4)} for c in range(3)] for r in range(3)]
    EEt = [[None] * 3 for _ in range(3)]
    for r in range(3):
        for c in range(3):
            s = {}
            for k in range(3):
                s = p_add(s, p_mul(E[r][k], E[c][k]))
            EEt[r][c] = s
    tr = p_add(p_add(EEt[0][0], EEt[1][1]), EEt[2][2])
    polys = []
    for r in range(3):
        for c in range(3):
            s = {}
            for k in range(3):
                s = p_add(s, p_mul(EEt[r][k], E[k][c]))
            polys.append(p_add(p_scale(s, LD(2)), p_mul(tr, E[r][c]), -1))
    det = {}
    for (a, b, c), sg in (((0, 1, 2), 1), ((1, 2, 0), 1), ((2, 0, 1), 1), ((0, 2, 1), -1), ((1, 0, 2), -1), ((2, 1, 0), -1)):
        det = p_add(det, p_mul(p_mul(E[0][a], E[1][b]), E[2][c]), sg)
    polys.append(det)
    zero = np.zeros(N.shape[0], LD)
    return np.stack([np.stack([p.get(m, zero) for m in MONO3 + MONO2], -1) for p in polys], 1)


def _E(N, s):
    return s[..., 0, None, None] * N[:, None, 0] + s[..., 1, None, None] * N[:, None, 1] + s[..., 2, None, None] * N[:, None, 2] + N[:, None, 3]


def _res(E):
    """the ten constraint values of E (..., 3, 3), any dtype: (..., 10)"""
    Et = np.swapaxes(E, -1, -2)
    EEt = E @ Et
    tr = np.trace(EEt, axis1=-2, axis2=-1)[..., None, None]
    c = 2 * (EEt @ E) - tr * E
    det = (E[..., 0, 0] * (E[..., 1, 1] * E[..., 2, 2] - E[..., 1, 2] * E[..., 2, 1])
           - E[..., 0, 1] * (E[..., 1, 0] * E[..., 2, 2] - E[..., 1, 2] * E[..., 2, 0])
           + E[..., 0, 2] * (E[..., 1, 0] * E[..., 2, 1] - E[..., 1, 1] * E[..., 2, 0]))
    return np.concatenate([c.reshape(c.shape[:-2] + (9,)), det[..., None]], -1)


def _dres(E, dE):
    """directional derivative of _res at E along dE"""
    Et, dEt = np.swapaxes(E, -1, -2), np.swapaxes(dE, -1, -2)
    EEt = E @ Et
    c = (2 * (dE @ Et @ E + E @ dEt @ E + EEt @ dE) - 2 * np.trace(E @ dEt, axis1=-2, axis2=-1)[..., None, None] * E
         - np.trace(EEt, axis1=-2, axis2=-1)[..., None, None] * dE)
    adjT = np.stack([np.cross(E[..., 1, :], E[..., 2, :]), np.cross(E[..., 2, :], E[..., 0, :]), np.cross(E[..., 0, :], E[..., 1, :])], -2)
    return np.concatenate([c.reshape(c.shape[:-2] + (9,)), (adjT * dE).sum((-1, -2))[..., None]], -1)


def residual(E):
    """max-abs of the ten constraints on the Frobenius-normalised E (real or complex, any leading shape)"""
    E = np.asarray(E)
    nrm = np.sqrt((np.abs(E) ** 2).sum((-1, -2)))[..., None, None]
    return np.abs(_res(E / nrm)).max(-1)


def _solve3(A, b):
    """Cramer on (..., 3, 3) systems of any dtype"""
    def det(M):
        return (M[..., 0, 0] * (M[..., 1, 1] * M[..., 2, 2] - M[..., 1, 2] * M[..., 2, 1])
                - M[..., 0, 1] * (M[..., 1, 0] * M[..., 2, 2] - M[..., 1, 2] * M[..., 2, 0])
                + M[..., 0, 2] * (M[..., 1, 0] * M[..., 2, 1] - M[..., 1, 1] * M[..., 2, 0]))
    d = det(A)
    out = []
    for k in range(3):
        M = A.copy(); M[..., :, k] = b
        out.append(det(M) / d)
    return np.stack(out, -1)


def polish(N, s, steps=25):
    """Newton in complex extended precision; s (T, 10, 3) complex.  Each solution keeps its best iterate."""
    Nc = np.asarray(N, CLD)
    s = np.asarray(s, CLD).copy()
    best = residual(_E(Nc, s))
    live = np.ones(best.shape, bool)
    with np.errstate(all="ignore"):
        for _ in range(steps):
            E = _E(Nc, s)
            r = _res(E)
            J = np.stack([_dres(E, np.broadcast_to(Nc[:, None, k], E.shape)) for k in range(3)], -1)          # (T, 10, 10, 3)
            JH = np.conj(np.swapaxes(J, -1, -2))
            d = _solve3(JH @ J, (JH @ r[..., None])[..., 0])
            cand = s - d
            rc = residual(_E(Nc, cand))
            better = live & np.isfinite(rc) & (rc < best)
            s[better] = cand[better]; best[better] = rc[better]
            live = better
            if not live.any():
                break
    return s, best


def solve(q1, q2):
    """All ten solutions of T tuples.  Returns a dict:
      N (T, 4, 3, 3); xyz (T, 10, 3) complex; imag (T, 10) relative imaginary part |Im (x, y, z)| / |(x, y, z, 1)|;
      real (T, 10) bool (imag <= REAL_IMAG); E (T, 10, 3, 3) float64, Frobenius-normalised, of the real parts;
      res (T, 10) the residual of E; admitted (T,) bool and why (T,) (0 admitted, 1 ambiguous real/complex, 2 close pair, 3 residual)."""
    N = nullspace(q1, q2)
    M = cubics(N).astype(float)
    T = len(N)
    with np.errstate(all="ignore"):
        B = np.linalg.solve(M[:, :, :10], M[:, :, 10:])
        A = np.zeros((T, 10, 10))
        A[:, :6] = -B[:, :6]
        A[:, 6, 0] = A[:, 7, 1] = A[:, 8, 2] = A[:, 9, 6] = 1.0
        A = np.where(np.isfinite(A).all((1, 2), keepdims=True), A, 0.0)
        v = np.linalg.eig(A)[1]
        s0 = np.swapaxes(v[:, 6:9, :] / v[:, 9:10, :], 1, 2)
        s0 = np.where(np.isfinite(s0), s0, 1.0)
    s, _ = polish(N, s0)
    sr, si = s.real.astype(float), s.imag.astype(float)
    imag = np.sqrt((si ** 2).sum(-1)) / np.sqrt((np.abs(s) ** 2).sum(-1).astype(float) + 1.0)
    real = imag <= REAL_IMAG
    E = _E(np.asarray(N, LD), np.asarray(s.real, LD))
    E = E / np.sqrt((E ** 2).sum((-1, -2)))[..., None, None]
    res = np.abs(_res(E)).max(-1).astype(float)
    E = E.astype(float)
    why = np.zeros(T, int)
    for t in range(T):
        if ((imag[t] > REAL_IMAG) & (imag[t] < COMPLEX_IMAG)).any():
            why[t] = 1
        elif not np.all(np.isfinite(res[t][real[t]])) or (res[t][real[t]] > MAX_RESIDUAL).any():
            why[t] = 3
        else:
            Er = E[t][real[t]]
            for i in range(len(Er)):
                for j in range(i):
                    if dist(Er[i], Er[j]) < MIN_SEP:
                        why[t] = 2
    return dict(N=N, xyz=s, imag=imag, real=real, E=E, res=res, admitted=why == 0, why=why)


def dist(Ea, Eb):
    """max-abs difference of the Frobenius-normalised matrices, sign-free; broadcasts over leading axes"""
    Ea = np.asarray(Ea, float); Eb = np.asarray(Eb, float)
    Ea = Ea / np.sqrt((Ea ** 2).sum((-1, -2)))[..., None, None]; Eb = Eb / np.sqrt((Eb ** 2).sum((-1, -2)))[..., None, None]
    return np.minimum(np.abs(Ea - Eb).max((-1, -2)), np.abs(Ea + Eb).max((-1, -2)))


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0.0]])


# ---- the case list ---------------------------------------------------------------------------------------------------------
# groups of tuples over one n = 60 scene each: (name, five_point_scene keywords, tuples (k, 5) or None for the scene's own samples)
N_POINTS = 60
# found by a CPU search over seeds 0-39 (noise 0 and 0.5, the scene's first 64 samples) for tuples with many real solutions: the
# interval lanes l <= nc of the device root search are only all live then.  (seed, noise_px, sample rows)
MANY_REAL = [(7, 0.0, (52,)), (14, 0.0, (31,)), (38, 0.5, (15,))]        # eight real solutions each (four more occur among the 768)


def groups(syn):
    """[(name, scene, tuples (k, 5) int32, noise_free)]: the 768 noisy-and-clean tuples, the 800 noise-free ones, the searched ones"""
    out = []
    for seed in range(6):
        for noise in (0.0, 0.5):
            sc = syn.five_point_scene(n=N_POINTS, seed=seed, noise_px=noise, iters=64)
            out.append(("mixed s%d n%.1f" % (seed, noise), sc, sc["samples"], False))
    for seed in range(8):
        sc = syn.five_point_scene(n=N_POINTS, seed=seed, noise_px=0.0, outlier_frac=0.0, iters=100)
        out.append(("clean s%d" % seed, sc, sc["samples"], True))
    for seed, noise, rows in MANY_REAL:
        sc = syn.five_point_scene(n=N_POINTS, seed=seed, noise_px=noise, iters=64)
        out.append(("many-real s%d n%.1f" % (seed, noise), sc, sc["samples"][list(rows)], False))
    return out


def tuple_points(sc, tuples):
    return sc["pd1"][tuples], sc["pd2"][tuples]                     # (k, 5, 2) each


def true_E(sc):
    E = skew(sc["Rt_gt"][:, 3]) @ sc["Rt_gt"][:, :3]
    return E / np.linalg.norm(E)
