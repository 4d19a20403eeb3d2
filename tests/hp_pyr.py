"""Extended-precision model of the pyramid build, plane by plane (test helper, CPU only).

A plain, slow restatement in numpy.longdouble (80-bit x87: eps 1.08e-19) of what the reference computes for ONE image, written from
the reference's sources and SURVEY Appendix A.4 / A.6 / A.7 and from nothing else of this repository (neither the C oracle nor the kernels):

  LKPyramid(image, levels)      optical_flow/pyramid.jl:40-79 -- gaussian_pyramid (IIR Gaussian with NA(): the Fill(0)-filtered image over
                                the Fill(0)-filtered indicator, then imresize to ceil.(size / 2)), Scharr gradients with Fill(0)    [mode 0]
  update!(lk, img)              pyramid.jl:81-137 -- the same chain with the default (replicate) border everywhere            [modes 1, 3]
  compute_partial_derivatives!  lucas_kanade.jl:102-138 -- Iy Iy, Ix Ix, Iy Ix, each filtered with IIRGaussian(4.0) and integrated
                                (cumsum along dim 1, then dim 2)

The IIR Gaussian carries NO boundary algebra here: the causal and anticausal recurrences of A.4 run over the line extended explicitly by
`pad` samples on both sides (replicated samples, or zeros for Fill(0)), started from the steady state of the constant continuation;
`pad` is chosen from the largest pole modulus so that |p|^pad < 2^-70 (asserted).  That checks the constant-signal left start and the
Triggs-Sdika right start of the reference independently instead of restating them.

COEFFICIENT PRECISION: inputs are Float64 images and every intermediate is long double, with ONE exception -- the Young-van Vliet
coefficients a1, a2, a3, B are evaluated in Float64 by the A.4 formulas and then promoted.  The reference computes them in Float64, so
their rounding is part of the specification: with long-double coefficients a model sits a systematic 1.8-2.8e-14 (relative to the
plane's largest magnitude) away from any Float64 implementation on every sigma = 4 plane.

The second half holds the seeded cases, the measure E = max |x - model| / max |model| per plane and level, `check` -- the ONE assertion
function of test_pyr_model_host.py (where damaged planes must be rejected by it) and test_gpu_pyr_model.py -- and a pure-Python
restatement of the build's segment geometry, from which the GPU tests predict the kernel route they then assert."""
import numpy as np

LD = np.longdouble
PLANES = ("layers", "Iy", "Ix", "Iyy", "Ixx", "Iyx")
BAR = 1e-11                      # (a) the documented bar of tolerance mode, relative to the plane's largest magnitude
K = 64                           # (b) E_dev <= K * max(E_oracle, 2^-52): the project's margin (hp_lk.K), fixed before any device run
EPS64 = 2.0 ** -52
# The C oracle against the model: 4 x the worst measured over every case below, both border modes, sigma 1.0 and 1.7
# (test_pyr_model_host.py): 6.15e-14, Ix of level 1 of 64 x 2049.  Typical planes sit at 1-8e-15; the worst ones follow an ODD-size
# imresize! of a wide level, where the Float64 source coordinate (n_src / n_dst)(dst - 0.5) + 0.5 carries ulp(1800) = 2e-13 of a pixel
# into the interpolation weight (layer 2.0e-14) and the gradients of that layer double it relative to their smaller range.
E_ORACLE_MAX = 2.5e-13


# ---------------------------------------------------------------------------------------------------------------- the model
def yvv_coeffs(sigma):
    """A.4: Young-van Vliet a1, a2, a3, B -- in Float64 (Python floats), see COEFFICIENT PRECISION above"""
    m0, m1, m2 = 1.16680, 1.10783, 1.40586
    sigma = float(sigma)
    q = 1.31564 * (float(np.sqrt(1 + 0.490811 * sigma * sigma)) - 1)
    scale = (m0 + q) * (m1 * m1 + m2 * m2 + 2 * m1 * q + q * q)
    a1 = q * (2 * m0 * m1 + m1 * m1 + m2 * m2 + (2 * m0 + 4 * m1) * q + 3 * q * q) / scale
    a2 = -q * q * (m0 + 2 * m1 + 3 * q) / scale
    a3 = q * q * q / scale
    b = m0 * (m1 * m1 + m2 * m2) / scale
    return a1, a2, a3, b * b


def pole_modulus(sigma):
    a1, a2, a3, _ = yvv_coeffs(sigma)
    return float(np.abs(np.roots([1.0, -a1, -a2, -a3])).max())


def pad_for(sigma):
    """samples of explicit extension: |p|^pad < 2^-70 for the slowest pole"""
    p = pole_modulus(sigma)
    assert 0 < p < 1
    pad = int(np.ceil(70 * np.log(2.0) / -np.log(p))) + 1
    assert p ** pad < 2.0 ** -70
    return pad


def iir_axis(X, sigma, axis, zero_ext=False, pad=None):
    """the A.4 recurrences along `axis` of X on the explicitly extended line: w[n] = x[n] + a1 w[n-1] + a2 w[n-2] + a3 w[n-3], then
    y[n] = B w[n] + a1 y[n+1] + a2 y[n+2] + a3 y[n+3]"""
    a1, a2, a3, B = (LD(c) for c in yvv_coeffs(sigma))
    pad = pad_for(sigma) if pad is None else pad
    assert pole_modulus(sigma) ** pad < 2.0 ** -70
    X = np.moveaxis(np.asarray(X, dtype=LD), axis, 0)
    n = X.shape[0]
    E = np.zeros((n + 2 * pad,) + X.shape[1:], dtype=LD)
    E[pad:pad + n] = X
    if not zero_ext:
        E[:pad] = X[0]; E[pad + n:] = X[-1]
    g = 1 / (1 - (a1 + a2 + a3))
    w1 = w2 = w3 = E[0] * g                                   # steady state of the constant continuation to the left
    W = np.empty_like(E)
    for i in range(n + 2 * pad):
        w = E[i] + a1 * w1 + a2 * w2 + a3 * w3
        W[i] = w; w3 = w2; w2 = w1; w1 = w
    y1 = y2 = y3 = B * E[-1] * g * g                          # ... and to the right
    Y = np.empty_like(X)
    for i in range(n + 2 * pad - 1, pad - 1, -1):
        y = B * W[i] + a1 * y1 + a2 * y2 + a3 * y3
        if i < pad + n:
            Y[i - pad] = y
        y3 = y2; y2 = y1; y1 = y
    return np.moveaxis(Y, 0, axis)


def iir2(X, sigma, zero_ext=False, pad=None):
    """imfilter(X, (IIRGaussian(sigma), IIRGaussian(sigma))): dim 1, then dim 2, over the last two axes"""
    return iir_axis(iir_axis(X, sigma, -2, zero_ext, pad), sigma, -1, zero_ext, pad)


def scharr(L, zero_border=False):
    """imgradients with KernelFactors.scharr as correlation: (-1, 0, 1) / 2 along the derivative axis, (3, 10, 3) / 16 across"""
    L = np.asarray(L, dtype=LD)
    spec = [(0, 0)] * (L.ndim - 2) + [(1, 1), (1, 1)]
    P = np.pad(L, spec, mode="constant") if zero_border else np.pad(L, spec, mode="edge")
    dy = (P[..., 2:, :] - P[..., :-2, :]) / 2
    dx = (P[..., :, 2:] - P[..., :, :-2]) / 2
    Iy = (3 * dy[..., :, :-2] + 10 * dy[..., :, 1:-1] + 3 * dy[..., :, 2:]) / 16
    Ix = (3 * dx[..., :-2, :] + 10 * dx[..., 1:-1, :] + 3 * dx[..., 2:, :]) / 16
    return Iy, Ix


def resize_axis(X, nd, axis):
    """imresize! along one axis (A.6): src = (n_src / n_dst)(dst - 0.5) + 0.5 (1-based), clamped to [1, n_src], linear"""
    X = np.moveaxis(np.asarray(X, dtype=LD), axis, 0)
    ns = X.shape[0]
    src = LD(ns) / LD(nd) * (np.arange(1, nd + 1, dtype=LD) - LD(0.5)) + LD(0.5)
    src = np.clip(src, LD(1), LD(ns))
    i0 = np.floor(src).astype(np.int64)
    f = (src - i0).reshape((nd,) + (1,) * (X.ndim - 1))
    i1 = np.minimum(i0 + 1, ns)
    return np.moveaxis((1 - f) * X[i0 - 1] + f * X[i1 - 1], 0, axis)


def resize_half(X):
    H, W = X.shape[-2:]
    return resize_axis(resize_axis(X, (H + 1) // 2, -2), (W + 1) // 2, -1)


def level_shapes(H, W, levels):
    out = [(H, W)]
    for _ in range(levels):
        H, W = (H + 1) // 2, (W + 1) // 2
        out.append((H, W))
    return out


def model(img, levels, mode, sigma=1.0, layer_sigma=None):
    """The six planes of every level: [{name: long-double array}] for level 0 .. levels.  img: Float64, H x W or S x H x W (S images
    at once).  mode 0: the constructor (Fill(0) + NA()); 1 and 3: update!.  layer_sigma: the Gaussian of the layer chain if it is to
    differ from `sigma` (damage tests)."""
    assert mode in (0, 1, 3)
    img = np.asarray(img)
    assert img.dtype == np.float64
    L = img.astype(LD)
    s_layer = sigma if layer_sigma is None else layer_sigma
    out = []
    for l in range(levels + 1):
        Iy, Ix = scharr(L, zero_border=(mode == 0))
        F = iir2(np.stack([Iy * Iy, Ix * Ix, Iy * Ix]), 4.0)
        I = np.cumsum(np.cumsum(F, axis=-2), axis=-1)
        out.append(dict(layers=L, Iy=Iy, Ix=Ix, Iyy=I[0], Ixx=I[1], Iyx=I[2]))
        if l < levels:
            if mode == 0:
                T = iir2(L, s_layer, zero_ext=True) / iir2(np.ones(L.shape[-2:], dtype=LD), s_layer, zero_ext=True)
            else:
                T = iir2(L, s_layer)
            L = resize_half(T)
    return out


def member(mdl, s):
    """image s of a model built from S x H x W"""
    return [{k: v[s] for k, v in lv.items()} for lv in mdl]


# ---------------------------------------------------------------------------------------------------------------- measure and bound
def _plane(planes, name, l):
    return planes.plane(name, l) if hasattr(planes, "plane") else planes[l][name]


class Planes:
    """six planes per level held in host memory (a downloaded device pyramid, a damaged copy of the oracle's)"""

    def __init__(self, src, levels):
        self.levels = levels
        self.d = {(n, l): np.array(_plane(src, n, l), dtype=np.float64) for l in range(levels + 1) for n in PLANES}

    def plane(self, name, l):
        return self.d[(name, l)]


def E(planes, mdl, which=None):
    """{(name, level): max |x - model| / max |model|}"""
    out = {}
    for l in range(len(mdl)):
        for n in PLANES:
            if which is not None and (n, l) not in which:
                continue
            m = mdl[l][n]
            x = np.asarray(_plane(planes, n, l), dtype=np.float64)
            assert x.shape == m.shape, (n, l, x.shape, m.shape)
            out[(n, l)] = float(np.abs(x.astype(LD) - m).max() / max(np.abs(m).max(), LD(1e-300)))
    return out


def check(dev, orc, mdl, tag="", which=None, report=None):
    """THE assertion on tolerance-mode planes.  dev, orc, mdl: one entry per batch member (device planes, the C oracle's planes of the
    same image, the model's).  For every member, plane and level (or those of `which`):
      (a) E_dev <= BAR                              the documented bar, against the model
      (b) E_dev <= K * max(E_oracle, 2^-52)         within K of what the reference arithmetic itself leaves
    `report`: a list that receives (tag, member, name, level, E_dev, E_oracle, ratio) for every figure, before anything is asserted.
    Returns the worst ratio."""
    assert len(dev) == len(orc) == len(mdl)
    bad, worst = [], 0.0
    for s in range(len(dev)):
        Ed, Eo = E(dev[s], mdl[s], which), E(orc[s], mdl[s], which)
        for (n, l), ed in Ed.items():
            floor = max(Eo[(n, l)], EPS64)
            ratio = ed / floor
            worst = max(worst, ratio)
            if report is not None:
                report.append((tag, s, n, l, ed, Eo[(n, l)], ratio))
            if not ed <= BAR:
                bad.append(f"(a) {tag} member {s} {n} level {l}: E_dev {ed:.3e} > {BAR:.0e}")
            elif not ed <= K * floor:
                bad.append(f"(b) {tag} member {s} {n} level {l}: E_dev {ed:.3e} > {K} x {floor:.3e} (ratio {ratio:.1f})")
    assert not bad, "\n".join(bad[:12]) + (f"\n... {len(bad)} in all" if len(bad) > 12 else "")
    return worst


def ratio_table(report):
    """worst ratio per (plane kind, level) of a report: the lines the GPU tests print"""
    kind = lambda n: "layer" if n == "layers" else "gradient" if n in ("Iy", "Ix") else "integral"
    t = {}
    for tag, s, n, l, ed, eo, r in report:
        k = (kind(n), l)
        if k not in t or r > t[k][0]:
            t[k] = (r, ed, eo)
    return "  ".join(f"{k[0]}@{k[1]}: {v[0]:.2f} (E_dev {v[1]:.1e}, E_orc {v[2]:.1e})" for k, v in sorted(t.items()))


# ---------------------------------------------------------------------------------------------------------------- seeded cases
def _box5(a):
    """5 x 5 box mean (valid part) through running sums"""
    c = np.cumsum(np.cumsum(np.pad(a, ((1, 0), (1, 0))), axis=0), axis=1)
    return (c[5:, 5:] - c[:-5, 5:] - c[5:, :-5] + c[:-5, :-5]) / 25.0


def texture_u8(H, W, seed):
    """a smoothed random texture quantised to 8 bits"""
    rng = np.random.default_rng(seed)
    t = _box5(rng.random((H + 4, W + 4)))
    t = (t - t.min()) / max(t.max() - t.min(), 1e-12)
    return np.asfortranarray(np.round(t * 255).astype(np.uint8))


def saturated_u8(H, W, seed):
    """the texture with saturated regions (flat areas: gradients and products exactly 0) and a one-pixel checkerboard patch (the
    largest gradients an 8-bit image has)"""
    im = np.array(texture_u8(H, W, seed))
    rng = np.random.default_rng(seed + 1000)
    h, w = max(H // 3, 2), max(W // 3, 2)
    y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
    im[y:y + h, x:x + w] = 255
    y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
    im[y:y + h, x:x + w] = 0
    h, w = max(H // 4, 2), max(W // 4, 2)
    y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
    yy, xx = np.mgrid[y:y + h, x:x + w]
    im[y:y + h, x:x + w] = np.where((yy + xx) & 1, 255, 0)
    return np.asfortranarray(im.astype(np.uint8))


def frames_u8(H, W, S, seed):
    """S different 8-bit frames: textures and saturated / checkerboard images in turn"""
    return [texture_u8(H, W, seed + 7 * s) if s % 2 == 0 else saturated_u8(H, W, seed + 7 * s) for s in range(S)]


def as_f64(u8):
    """Gray{Float64} of an 8-bit frame: raw / 255"""
    return np.asfortranarray(u8.astype(np.float64) / 255.0)


# ---------------------------------------------------------------------------------------------------------------- segment geometry
# What the build derives its kernel choice from, restated: the row kernel of the tolerance build takes its samples per segment from a
# fixed menu -- the smallest entry that covers a row with 32 segments and leaves at least two of them; rows past 40 x 32 samples take 64
# segments of 24 / 32 samples; nothing fits rows under 8 or over 2048 samples.  The single-image kernels cut a line into at most
# `nseg` segments of at least 4 samples.
RT_MENU = (4, 6, 8, 10, 12, 16, 20, 24, 32, 40)
RT_MENU_WIDE = (24, 32)
RT_NS = 32
SEG_MAX, SEG_SLMAX = 128, 16     # single image: segments per line, samples per segment


def rt_seg_len(n):
    """(samples per segment, segments) of the tolerance row kernel for rows of n samples; (0, 64): no variant fits"""
    for m in RT_MENU:
        if -(-n // m) <= RT_NS and n >= 2 * m:
            return m, RT_NS
    for m in RT_MENU_WIDE:
        if -(-n // m) <= 2 * RT_NS and n >= 2 * m:
            return m, 2 * RT_NS
    return 0, 2 * RT_NS


def seg_len(n, nseg):
    return max(4, -(-n // nseg))


def single_is_fast(H0, W0):
    """a single image's mode-3 build takes the segmented kernels when both level-0 dimensions fit 128 segments of 16 samples"""
    return seg_len(H0, SEG_MAX) <= SEG_SLMAX and seg_len(W0, SEG_MAX) <= SEG_SLMAX


def expect_tol_batch(H, W, has_next):
    """route fields of one level on the batch tolerance kernels (H >= 64, rt_seg_len(W) fits)"""
    sl, ns = rt_seg_len(W)
    P = (H + 15) & ~15
    even = H % 2 == 0
    return dict(family="FAM_TOLB", cols="COLS_FUSED", rows="ROWS_TOL", rt_sl=sl, rt_ns=ns, dec=int(has_next and even and P % 32 == 0),
                resize="RZ_NONE" if not has_next else "RZ_EVEN" if even else "RZ_PLAIN")


def expect_seg(H, W, has_next, rows_tol_single=True, seg_wide=False):
    """route fields of one level on the single-image tolerance kernels"""
    sl, ns = rt_seg_len(W)
    rt1 = sl > 0 and ns == RT_NS and rows_tol_single
    s32 = seg_len(H, 32)
    return dict(family="FAM_SEG", cols="COLS_SEG", rows="ROWS_TOL" if rt1 else "ROWS_SEG", rt_sl=sl, rt_ns=ns,
                slc=seg_len(H, SEG_MAX), slr=seg_len(W, SEG_MAX), slc32=s32 if s32 <= SEG_SLMAX and not seg_wide else 0,
                resize="RZ_NONE" if not has_next else "RZ_EVEN" if rt1 and H % 2 == 0 else "RZ_PLAIN")


# the level-0 sizes of test_gpu_pyr_model.py's batch cases: both ends of every k_rows_tol instantiation's width range, round-robin over
# heights with an even height at a pitch that is a multiple of 32 (64), an odd one (65), an even one at pitch 80, and 96 / 129
BATCH_WIDTHS = (8, 127, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 512, 513, 640, 641, 768, 769, 1024, 1025, 1280, 1281, 1536, 1537, 2048)
BATCH_HEIGHTS = (64, 65, 80, 96, 129)
BATCH_CASES = tuple((BATCH_HEIGHTS[i % len(BATCH_HEIGHTS)], w) for i, w in enumerate(BATCH_WIDTHS))
FALLBACK_WIDTHS = (7, 2049)
STRIP_CASES = tuple((64, w) for w in (62, 63, 124, 125, 187)) + tuple((h, 70) for h in (64, 95, 96, 97, 128))
CHAIN_CASES = ((256, 1531, 2), (259, 640, 3))
SINGLE_CASES = ((16, 16, 1), (65, 97, 2), (131, 163, 2), (512, 64, 1), (513, 64, 1), (64, 1281, 1), (64, 2048, 1), (64, 2049, 1))


def all_cases():
    """every (H, W, levels) the GPU tests build"""
    return ([(h, w, 1) for h, w in BATCH_CASES] + [(64, w, 1) for w in FALLBACK_WIDTHS] + [(h, w, 1) for h, w in STRIP_CASES]
            + list(CHAIN_CASES) + list(SINGLE_CASES))
