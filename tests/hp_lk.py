"""Extended-precision model of the tracking path, one point at a time (test helper, CPU only).

A plain, slow restatement in numpy.longdouble (80-bit x87: eps 1.08e-19) of what the reference does with ONE keypoint, written from
the reference's sources and from nothing else of this repository:

  optflow!                 optical_flow/lucas_kanade.jl:9-100 -- the levels of one point: get_pyramid_coordinate, get_offsets, get_grid,
                           compute_spatial_gradient (boxdiff of the three integral images, :140-157), the iteration with its two lies_in
                           tests, the offsets re-evaluation, prepare_linear_system / compute_flow_vector (:159-187, BSpline(Linear())
                           sampling of the target layer), the epsilon break
  svd2x2 / pinv2x2         optical_flow/utils.jl: singular values Q +- R; the pseudo-inverse of the symmetric matrix from its
                           eigen-decomposition (projectors), singular values <= sqrt(eps(Float64)) dropped
  fb_tracking!             tracker.jl:17-66: forward pass, level-1 backward pass with the default epsilon 1e-2 from -displacement,
                           norm(keypoint - back) >= max_distance fails
  optical_flow_matching!   map_manager.jl:451-564 with maybe_stereo_update! (:579-590): a 3-D keypoint runs `pyramid_levels_3d` levels
                           from (projection - pixel) / 2^levels3d, on failure the 2-D attempt from zero; in_image gates; the epipolar test

Window sums are plain long-double sums: no summation order is modelled.  Inputs are Float64 (points, priors, planes); every
intermediate is long double.  Beside fate and position every point gets a DECISION MARGIN: the smallest distance of a computed
quantity from the threshold it was compared with, over everything the point executed (Margin, below).  A point whose margin is
<= TAU is *excused*: a Float64 implementation may legitimately decide it the other way.

The second half holds the seeded cases, the measure E(x) = max |x - model| over the points that are not excused and that both sides
track, and `check`, the ONE assertion function of test_lk_model_host.py (where damaged runs must be rejected by it) and
test_gpu_lk_model.py."""
import numpy as np

LD = np.longdouble
PLANES = ("layers", "Iy", "Ix", "Iyy", "Ixx", "Iyx")
SQRT_EPS = LD(2.0) ** -26                    # sqrt(eps(Float64)), pinv2x2's threshold
EIG_THR, EPS, ITERATIONS = 1e-4, 1e-2, 30    # LucasKanade defaults (lucas_kanade.jl:1-7; fb_tracking!'s keyword form passes no others)
TAU = 1e-6                                   # a margin at or below this excuses the point: the documented position bar of tolerance mode
K = 64                                       # bound of a case = K * max(E_seq, E_wave, ulp(max(H, W))), fixed in advance
MAX_EXCUSED = 0.01                           # share of a case's points that may be excused
CAP_EXACT, CAP_TOL = 1e-9, 1e-6              # px: the bound never exceeds these (exact kernels / tolerance instantiation)
E_ORACLE_MAX = 1e-12                         # px: the C oracle against the model, either summation order


# ---------------------------------------------------------------------------------------------------------------- the model
class Margin:
    """running minimum of |quantity - threshold| over the comparisons a point executed"""
    __slots__ = ("v",)

    def __init__(self):
        self.v = np.inf

    def note(self, d):
        d = float(abs(d))
        if d < self.v:
            self.v = d


def svd2x2(M):
    """utils.jl:5-27 in long double: U, (sx, |sy|), V with M == U * diag(S) * V'"""
    M = np.asarray(M, dtype=LD)
    E, F = (M[0, 0] + M[1, 1]) / 2, (M[0, 0] - M[1, 1]) / 2
    G, H = (M[1, 0] + M[0, 1]) / 2, (M[1, 0] - M[0, 1]) / 2
    Q, R = np.sqrt(E * E + H * H), np.sqrt(F * F + G * G)
    sx, sy = Q + R, Q - R
    a1, a2 = np.arctan2(G, F), np.arctan2(H, E)
    th, ph = (a2 - a1) / 2, (a2 + a1) / 2
    s = np.sign(sy)
    U = np.array([[np.cos(ph), -s * np.sin(ph)], [np.sin(ph), s * np.cos(ph)]], dtype=LD)
    V = np.array([[np.cos(th), np.sin(th)], [-np.sin(th), np.cos(th)]], dtype=LD)
    return U, np.array([sx, abs(sy)], dtype=LD), V


def pinv2x2(M):
    """utils.jl:31-45 through svd2x2: U * D * V', singular values <= sqrt(eps) dropped"""
    U, S, V = svd2x2(M)
    D = np.diag([1 / S[0] if S[0] > SQRT_EPS else LD(0), 1 / S[1] if S[1] > SQRT_EPS else LD(0)]).astype(LD)
    return U @ D @ V.T


def pinv_sym2x2(a, b, d, margin=None):
    """pseudo-inverse of the SYMMETRIC [[a, b], [b, d]] from its eigen-decomposition: eigenvalues E +- R with projectors
    (I +- [[F, b], [b, -F]] / R) / 2; |eigenvalue| are the singular values svd2x2 returns (Q + R, |Q - R| with Q = |E|).
    Returns (pinv, singular values (large, small))."""
    a, b, d = LD(a), LD(b), LD(d)
    E, F = (a + d) / 2, (a - d) / 2
    R = np.sqrt(F * F + b * b)
    lam = (E + R, E - R)
    if margin is not None:
        for l in lam:
            margin.note((abs(l) - SQRT_EPS) / SQRT_EPS)
    c = [1 / l if abs(l) > SQRT_EPS else LD(0) for l in lam]
    I2 = np.eye(2, dtype=LD)
    if R == 0:
        Gi = c[0] * I2
    else:
        N = np.array([[F, b], [b, -F]], dtype=LD) / R
        Gi = c[0] * (I2 + N) / 2 + c[1] * (I2 - N) / 2
    s = sorted((abs(lam[0]), abs(lam[1])), reverse=True)
    return Gi, (s[0], s[1])


class Planes:
    """the six planes of every level of one pyramid as long-double H x W arrays (index [row - 1, column - 1])"""

    def __init__(self, get, levels):
        """get(name, level0) -> H x W Float64 array; levels = number of layers"""
        self.f64 = [{n: np.array(get(n, l), dtype=np.float64, order="F") for n in PLANES} for l in range(levels)]
        self.lv = [{n: a.astype(LD) for n, a in d.items()} for d in self.f64]
        self.levels = levels

    def to_oracle(self, orc):
        """an oracle.Pyramid holding exactly these planes"""
        H, W = self.f64[0]["layers"].shape
        p = orc.Pyramid(H, W, self.levels)
        for l in range(self.levels):
            for n in PLANES:
                p.plane(n, l)[...] = self.f64[l][n]
        return p


def planes_of(pyr, levels=4):
    """from anything with .plane(name, level0): an oracle.Pyramid or a device LKPyramid (downloads)"""
    return Planes(pyr.plane, levels)


def _boxdiff(I, y1, y2, x1, x2):
    """Images.boxdiff over the 1-based inclusive ranges y1:y2, x1:x2 of an integral image"""
    s = I[y2 - 1, x2 - 1]
    if x1 > 1:
        s = s - I[y2 - 1, x1 - 2]
    if y1 > 1:
        s = s - I[y1 - 2, x2 - 1]
    if y1 > 1 and x1 > 1:
        s = s + I[y1 - 2, x1 - 2]
    return s


def _lies_in(H, W, p, exact, m):
    """lucas_kanade.jl:189-191; `exact`: the operands are integers held exactly (no margin: the comparison cannot flip)"""
    if not exact:
        for d in (p[0] - 1, H - p[0], p[1] - 1, W - p[1]):
            m.note(d)
    return 1 <= p[0] <= H and 1 <= p[1] <= W


def _get_offsets(point, newp, exact, window, H, W, m):
    """lucas_kanade.jl:199-208 over the axes 1:H, 1:W.  Each floor takes min(window, a_point, a_new) with a_point an exact integer:
    as a function of the inexact a_new it steps at the integers k <= min(window, a_point) (k = window included) and nowhere else."""
    def one(a_int, a_new):
        cap = min(window, a_int)
        if not exact:
            k = np.rint(a_new)
            if k <= cap:
                m.note(a_new - k)
        return int(np.floor(min(LD(cap), a_new)))
    return (one(point[0] - 1, newp[0] - 1), one(H - point[0], H - newp[0]),
            one(point[1] - 1, newp[1] - 1), one(W - point[1], W - newp[1]))


def _spatial_gradient(F, point, offs, m):
    """compute_spatial_gradient (:149-157): G from the integral images over grid = point + offsets, its pseudo-inverse, min singular
    value / number of grid cells"""
    y1, y2, x1, x2 = point[0] - offs[0], point[0] + offs[1], point[1] - offs[2], point[1] + offs[3]
    # (a level coordinate can be 0 -- floor(y / 2^l) of y < 2^l -- with offsets -1:down; an EMPTY grid would need a prior as long as the
    #  level is high on top of that: outside what the reference defines, and outside every case here)
    assert y2 >= y1 >= 1 and x2 >= x1 >= 1, "empty window"
    syy, sxx, syx = (_boxdiff(F[n], y1, y2, x1, x2) for n in ("Iyy", "Ixx", "Iyx"))
    Gi, S = pinv_sym2x2(syy, syx, sxx, m)
    return Gi, S[1] / LD((y2 - y1 + 1) * (x2 - x1 + 1))


def _sample(B, r, c):
    """BSpline(Linear()) interpolation of B at the rows r x columns c (1-based, inside the image): outer grid of values"""
    H, W = B.shape
    iy = np.clip(np.floor(r), 1, max(H - 1, 1)).astype(np.int64); fy = r - iy
    ix = np.clip(np.floor(c), 1, max(W - 1, 1)).astype(np.int64); fx = c - ix
    iy1 = np.minimum(iy, H - 1); ix1 = np.minimum(ix, W - 1)           # 0-based index of the second sample (H == 1: the same row)
    top = (1 - fx)[None, :] * B[np.ix_(iy - 1, ix - 1)] + fx[None, :] * B[np.ix_(iy - 1, ix1)]
    bot = (1 - fx)[None, :] * B[np.ix_(iy1, ix - 1)] + fx[None, :] * B[np.ix_(iy1, ix1)]
    return (1 - fy)[:, None] * top + fy[:, None] * bot


def _flow_vector(F, S, point, corr, offs, Gi):
    """prepare_linear_system + compute_flow_vector (:159-187)"""
    up, down, left, right = offs
    ys = slice(point[0] - up - 1, point[0] + down); xs = slice(point[1] - left - 1, point[1] + right)
    r = corr[0] + np.arange(-up, down + 1).astype(LD)
    c = corr[1] + np.arange(-left, right + 1).astype(LD)
    dI = F["layers"][ys, xs] - _sample(S["layers"], r, c)
    b = np.array([(dI * F["Iy"][ys, xs]).sum(), (dI * F["Ix"][ys, xs]).sum()], dtype=LD)
    return Gi @ b


def optflow_point(first, second, pt, disp, pyramid_levels, window, m, eps=EPS, eig_thr=EIG_THR, iterations=ITERATIONS):
    """optflow! (:9-100) for one point: (status, displacement).  pt, disp: 2-vectors (y, x), any float type."""
    pt = np.asarray(pt, dtype=LD); d = np.array(disp, dtype=LD)
    assert first.levels > pyramid_levels and second.levels > pyramid_levels, "Not enough layers in pyramids."
    for level in range(pyramid_levels + 1, 0, -1):
        F, S = first.lv[level - 1], second.lv[level - 1]
        H, W = F["layers"].shape
        scaled = pt / LD(2) ** (level - 1)
        if level == 1:                                      # Float64 points divided by a power of two are exact; a long-double point
            for v in scaled:                                # (the backward pass starts from pt + displacement) is not
                if v != np.float64(v):
                    m.note(v - np.rint(v))
        point = (int(np.floor(scaled[0])), int(np.floor(scaled[1])))
        pf = np.array(point, dtype=LD)
        offs = _get_offsets(point, pf, True, window, H, W, m)
        Gi, min_eig = _spatial_gradient(F, point, offs, m)
        m.note((min_eig - eig_thr) / eig_thr)
        if min_eig < eig_thr:
            return False, d
        contrib = np.zeros(2, dtype=LD)
        for _ in range(iterations):
            flow = d + contrib
            exact = bool(flow[0] == 0 and flow[1] == 0)
            corr = pf + flow
            if not _lies_in(H, W, corr, exact, m):
                return False, d
            noffs = _get_offsets(point, corr, exact, window, H, W, m)
            if noffs != offs:
                offs = noffs
                Gi, min_eig = _spatial_gradient(F, point, offs, m)
                m.note((min_eig - eig_thr) / eig_thr)
                if min_eig < eig_thr:
                    return False, d
            est = _flow_vector(F, S, point, corr, offs, Gi)
            big = max(abs(est[0]), abs(est[1]))
            m.note(big - eps)
            if big < eps:
                break
            contrib = contrib + est
            if not _lies_in(H, W, corr + est, False, m):
                return False, d
        d = d + contrib
        if level > 1:
            d = d * 2
    return True, d


def fb_point(prev, cur, pt, disp, pyramid_levels, window, max_distance, m):
    """fb_tracking! (tracker.jl:17-66) for one point: (status, new position (long double) or None)"""
    pt = np.asarray(pt, dtype=LD)
    ok, d = optflow_point(prev, cur, pt, disp, pyramid_levels, window, m)
    if not ok:
        return False, None
    new = pt + d
    ok, bd = optflow_point(cur, prev, new, -d, 0, window, m, eps=1e-2)
    if not ok:
        return False, None
    diff = pt - (new + bd)
    dist = np.sqrt(diff[0] * diff[0] + diff[1] * diff[1])
    m.note(dist - max_distance)
    if dist >= max_distance:
        return False, None
    return True, new


class Model:
    """fb_point over lists, memoised per (point, prior, levels): the tests of one case share every run"""

    def __init__(self, prev, cur, window, max_distance):
        self.prev, self.cur, self.window, self.maxd = prev, cur, window, max_distance
        self._memo = {}

    def one(self, pt, disp, levels):
        key = (float(pt[0]), float(pt[1]), float(disp[0]), float(disp[1]), levels)
        if key not in self._memo:
            m = Margin()
            ok, new = fb_point(self.prev, self.cur, pt, disp, levels, self.window, self.maxd, m)
            self._memo[key] = (ok, new, m.v)
        return self._memo[key]

    def fb_tracking(self, pts, disp, levels):
        """-> dict(fate (n,) 0 / 1, pos (n, 2) long double (nan where lost), margin (n,))"""
        n = len(pts)
        disp = np.zeros((n, 2)) if disp is None else disp
        fate = np.zeros(n, np.int64); pos = np.full((n, 2), np.nan, dtype=LD); mar = np.full(n, np.inf)
        for i in range(n):
            ok, new, mv = self.one(pts[i], disp[i], levels)
            fate[i] = ok; mar[i] = mv
            if ok:
                pos[i] = new
        return dict(fate=fate, pos=pos, margin=mar)

    def matching(self, pts, is_3d, proj, image_size, pyramid_levels, levels3d, stereo=False, undistorted_left=None, epipolar=2.0):
        """optical_flow_matching! on arrays.  Fate: 0 lost (temporal: observation removed; stereo: 3-D keypoint projected outside the
        right image), 1 updated, 2 kept as it is (temporal: projection outside the image; stereo: no match).  pos: the updated
        position (stereo: (left row, matched column)), the input pixel for fate 2, nan for fate 0.  The right camera of the stereo
        mode undistorts with the identity."""
        n = len(pts)
        Himg, Wimg = image_size
        scale = 1.0 / 2.0 ** levels3d
        fate = np.zeros(n, np.int64); pos = np.full((n, 2), np.nan, dtype=LD); mar = np.full(n, np.inf)
        for i in range(n):
            ok, new = False, None
            if is_3d[i]:
                if not (1 <= proj[i, 0] <= Himg and 1 <= proj[i, 1] <= Wimg):      # in_image on Float64 inputs: exact
                    fate[i] = 0 if stereo else 2
                    if not stereo:
                        pos[i] = pts[i]
                    continue
                ok, new, mv = self.one(pts[i], scale * (proj[i] - pts[i]), levels3d)
                mar[i] = min(mar[i], mv)
            if not ok:
                ok, new, mv = self.one(pts[i], (0.0, 0.0), pyramid_levels)
                mar[i] = min(mar[i], mv)
            if stereo:
                fate[i] = 2; pos[i] = pts[i]
                if ok:
                    gap = abs(LD(undistorted_left[i, 0]) - new[0])
                    mar[i] = min(mar[i], float(abs(gap - epipolar)))
                    if not gap > epipolar:
                        fate[i] = 1; pos[i] = (LD(pts[i, 0]), new[1])
            elif ok:
                fate[i] = 1; pos[i] = new
        return dict(fate=fate, pos=pos, margin=mar)


# ------------------------------------------------------------------------------------------------- measure, bound, assertion
def result(fate, pos):
    """an implementation's answer in the model's terms: fate (n,) ints, pos (n, 2) Float64 (ignored where the fate has no position)"""
    return dict(fate=np.asarray(fate).astype(np.int64), pos=np.asarray(pos, dtype=np.float64))


def excused(model):
    return model["margin"] <= TAU


def measure(model, got):
    """E = max |x - model| (px, infinity norm) over the points that are not excused and that both sides give a position"""
    both = ~excused(model) & (model["fate"] > 0) & (got["fate"] > 0)
    if not both.any():
        return 0.0
    return float(np.abs(got["pos"][both].astype(LD) - model["pos"][both]).max())


def ulp(x):
    return float(np.spacing(np.float64(x)))


def bound(E_seq, E_wave, shape, cap):
    return min(K * max(E_seq, E_wave, ulp(max(shape))), cap)


def check(model, got, E_seq, E_wave, shape, cap, tag=""):
    """THE assertion of the point tests: at most 1 % excused; fate equal on every other point; E within the case's bound.
    Returns (E, number of excused points)."""
    ex = excused(model)
    n = len(ex)
    assert ex.sum() <= MAX_EXCUSED * n, (tag, "excused", int(ex.sum()), n)
    diff = np.flatnonzero(~ex & (model["fate"] != got["fate"]))
    assert len(diff) == 0, (tag, "fate differs at points", diff[:8].tolist(), model["fate"][diff[:8]].tolist(), got["fate"][diff[:8]].tolist(),
                            "margins", model["margin"][diff[:8]].tolist())
    E = measure(model, got)
    b = bound(E_seq, E_wave, shape, cap)
    assert E <= b, (tag, "E", E, "bound", b, "E_seq", E_seq, "E_wave", E_wave)
    return E, int(ex.sum())


# ------------------------------------------------------------------------------------------------------------------ the cases
S = 4                                         # streams of a case (different frames per stream)
SHAPES = {"odd": (93, 131), "even": (120, 160)}     # odd: levels 47 x 66, 24 x 33, 12 x 17 -- odd heights (pitch padding rows), every
STEPS = {"odd": (2.2, -3.1), "even": (1.3, -2.1)}   # coarse level smaller than the 22 / 28 / 32 LDS patch; even: level 3 is 15 x 20
WINDOWS = (5, 9, 11, 12)                      # kernel instantiations 3 / 6 / 9 slots, and 12 on the 9-slot kernel's uncached path
MODES = ("zero", "l1", "l0", "l0x3")          # prior modes, below
DISPARITY = 6.3
N_DETECTED, N_BORDER, BORDER_PX = 38, 30, 24.0


def mode_levels(mode):
    """(pyramid_levels of the prior attempt, multiple of the prior's offset from the true flow)"""
    return {"zero": (3, 0.0), "l1": (1, 1.0), "l0": (0, 1.0), "l0x3": (0, 3.0)}[mode]


def frames(syn, shape_name):
    """per stream: (left frame 0, left frame 1, right frame 1) as u8 Fortran arrays, and the stream's true flow (dy, dx)"""
    H, W = SHAPES[shape_name]
    out = []
    for s in range(S):
        step = (STEPS[shape_name][0] + 0.1 * s, STEPS[shape_name][1] - 0.15 * s)
        L, R, flows = syn.stereo_stream((H, W), 2, seed=70 + s, step=step, disparity=DISPARITY)
        u8 = lambda im: np.asfortranarray(np.round(np.asarray(im) * 255).astype(np.uint8))
        out.append(dict(a=u8(L[0]), b=u8(L[1]), r=u8(R[1]), flow=np.array(flows[1], dtype=np.float64)))
    return out


def as_f64(u8):
    return np.asfortranarray(u8.astype(np.float64) / 255.0)


def points(orc, shape_name, frs, seed=2):
    """per stream: ~38 detected keypoints of frame 0 with uniform sub-pixel jitter + 30 sub-pixel points within 24 px of one of the four
    borders, clipped to the image, none on integer coordinates"""
    H, W = SHAPES[shape_name]
    out = []
    for s in range(S):
        rng = np.random.default_rng([seed, s, H])
        kp = orc.detect(as_f64(frs[s]["a"]), np.zeros((0, 2)), max_points=N_DETECTED).astype(np.float64)
        kp = kp[rng.permutation(len(kp))[:N_DETECTED]]
        kp = kp + rng.uniform(0.01, 0.99, kp.shape)
        side = np.arange(N_BORDER) % 4
        d = rng.uniform(0.0, BORDER_PX, N_BORDER)
        y = rng.uniform(1, H, N_BORDER); x = rng.uniform(1, W, N_BORDER)
        y = np.where(side == 0, 1 + d, np.where(side == 1, H - d, y))
        x = np.where(side == 2, 1 + d, np.where(side == 3, W - d, x))
        p = np.concatenate([kp, np.stack([y, x], 1)])
        p = np.clip(p, 1.0 + 1e-3, [H - 1e-3, W - 1e-3])
        assert not (p == np.rint(p)).any()
        out.append(np.ascontiguousarray(p))
    return out


def priors(shape_name, frs, pts, window, mode, seed=0, shift=None):
    """per stream: (is_3d, projection) of the prior mode.  The projection is pixel + (true flow + mult * offset), offset 3-7 px in a
    random direction ("zero": the pixel itself); ~60 % of the points are 3-D; a 3-D flag is dropped where the projection leaves the
    image, except on the first two such points of the stream (temporal: kept as they are; stereo: observation removed)."""
    H, W = SHAPES[shape_name]
    mult = mode_levels(mode)[1]
    out = []
    for s in range(S):
        n = len(pts[s])
        rng = np.random.default_rng([seed, s, window, MODES.index(mode), H])
        is3 = rng.random(n) < 0.6
        ang = rng.uniform(0, 2 * np.pi, n); mag = rng.uniform(3.0, 7.0, n)
        off = np.stack([mag * np.sin(ang), mag * np.cos(ang)], 1)
        base = frs[s]["flow"] if shift is None else np.asarray(shift, dtype=np.float64)
        proj = pts[s].copy() if mode == "zero" else pts[s] + (base + mult * off)
        if mode == "zero":
            far = np.flatnonzero(is3)[:2]                       # two 3-D points sent far outside: the in_image gate
            proj[far] = proj[far] + np.array([2.0 * H, 5.0])
        outside = ~((proj[:, 0] >= 1) & (proj[:, 0] <= H) & (proj[:, 1] >= 1) & (proj[:, 1] <= W))
        drop = np.flatnonzero(is3 & outside)[2:]
        is3[drop] = False
        out.append((is3, np.ascontiguousarray(proj)))
    return out


def xyz_of(proj):
    """map points that project EXACTLY onto proj (y, x) through Tcw = I and the camera (fx, fy, cx, cy) = (1, 1, 0, 0): (x, y, 1)"""
    return np.ascontiguousarray(np.stack([proj[:, 1], proj[:, 0], np.ones(len(proj))], 1))


IDENTITY_CAM = (1.0, 1.0, 0.0, 0.0)


def oracle_matching(orc, prev, cur, pts, is3, proj, shape, window, levels, levels3d, sum_order, stereo=False):
    """the C oracle's fb_tracking under the protocol of optical_flow_matching! (the protocol itself restated here from
    map_manager.jl:451-564, so that `pyramid_levels_3d` is a parameter), in the model's fate coding"""
    n = len(pts)
    H, W = shape
    fate = np.zeros(n, np.int64); pos = np.full((n, 2), np.nan)
    inside = (proj[:, 0] >= 1) & (proj[:, 0] <= H) & (proj[:, 1] >= 1) & (proj[:, 1] <= W)
    skipped = is3 & ~inside
    if not stereo:
        fate[skipped] = 2; pos[skipped] = pts[skipped]
    ids3 = np.flatnonzero(is3 & inside); ids2 = list(np.flatnonzero(~is3))
    new = {}
    if len(ids3):
        o, st = orc.fb_tracking(prev, cur, pts[ids3], (1.0 / 2.0 ** levels3d) * (proj[ids3] - pts[ids3]), 30, window, levels3d,
                                EIG_THR, EPS, 1.0, sum_order=sum_order)
        for k, j in enumerate(ids3):
            if st[k]:
                new[j] = o[k]
            else:
                ids2.append(j)
    if len(ids2):
        ids2 = np.asarray(ids2)
        o, st = orc.fb_tracking(prev, cur, pts[ids2], None, 30, window, levels, EIG_THR, EPS, 1.0, sum_order=sum_order)
        for k, j in enumerate(ids2):
            if st[k]:
                new[j] = o[k]
    for j in range(n):
        if skipped[j]:
            continue
        if stereo:
            fate[j] = 2; pos[j] = pts[j]
            if j in new and not abs(pts[j, 0] - new[j][0]) > 2.0:
                fate[j] = 1; pos[j] = (pts[j, 0], new[j][1])
        elif j in new:
            fate[j] = 1; pos[j] = new[j]
    return result(fate, pos)


def oracle_fb(orc, prev, cur, pts, disp, window, levels, sum_order, max_distance=1.0):
    o, st = orc.fb_tracking(prev, cur, pts, disp, 30, window, levels, EIG_THR, EPS, max_distance, sum_order=sum_order)
    return result(st, o)


def concat(results):
    """the per-stream dicts of a case as one"""
    return {k: np.concatenate([r[k] for r in results]) for k in results[0]}
