"""CPU: the long-double model of the pyramid build (tests/hp_pyr.py) -- the C oracle against it on every shape the GPU tests build,
the model's own sanity independent of the oracle, what `check` rejects, and the Python restatement of the segment geometry."""
import numpy as np
import pytest

import hp_pyr as hp

LD = hp.LD


# ---------------------------------------------------------------------------------------------------------------- oracle against model
@pytest.mark.parametrize("mode,sigma", [(1, 1.0), (1, 1.7), (0, 1.0), (0, 1.7)])
def test_oracle_within_e_oracle_max_of_the_model(orc, mode, sigma):
    """every (H, W, levels) of test_gpu_pyr_model.py, textures and saturated / checkerboard images in turn: the oracle's six planes of
    every level within E_ORACLE_MAX of the model.  MEASURED worst over the four (border mode, sigma) runs: see E_ORACLE_MAX's comment in
    DESIGN 3.2.1; E_ORACLE_MAX = 4 x that."""
    worst, at = 0.0, None
    for i, (H, W, lv) in enumerate(hp.all_cases()):
        img = hp.as_f64((hp.texture_u8, hp.saturated_u8)[i % 2](H, W, seed=100 + i))
        e = hp.E(orc.pyr_build(img, lv, sigma, mode), hp.model(img, lv, mode, sigma))
        k = max(e, key=e.get)
        if e[k] > worst:
            worst, at = e[k], (H, W, lv) + k
    print(f"worst E_oracle, mode {mode}, sigma {sigma}: {worst:.3e} at {at}")
    assert worst <= hp.E_ORACLE_MAX, (worst, at)


# ---------------------------------------------------------------------------------------------------------------- model sanity
def test_constant_image_stays_constant():
    """to 1e-18 through every level -- up to the filter's DC gain G = B / (1 - a1 - a2 - a3)^2 per dimension, which the Float64
    rounding of the four coefficients (part of the specification, see hp_pyr) leaves within a few eps(Float64) of 1 instead of at 1:
    with long-double coefficients G = 1 and the layers stay at the constant itself"""
    a1, a2, a3, B = (LD(c) for c in hp.yvv_coeffs(1.0))
    G = B / ((1 - (a1 + a2 + a3)) * (1 - (a1 + a2 + a3)))
    assert abs(G - 1) <= 4 * hp.EPS64
    m = hp.model(np.full((37, 50), 0.37), 3, 1)
    for l, lv in enumerate(m):
        assert np.abs(lv["layers"] - LD(0.37) * G ** (2 * l)).max() <= 1e-18, l
        assert np.abs(lv["layers"] - lv["layers"][0, 0]).max() <= 1e-18, l
        for n in hp.PLANES[1:]:
            assert np.abs(lv[n]).max() <= 1e-18, (n, l)


@pytest.mark.parametrize("sigma,zero_ext", [(1.0, False), (1.7, True), (4.0, False), (4.0, True)])
def test_pad_and_twice_pad_agree(sigma, zero_ext):
    """on what each sigma filters in the build: the image (layer chain), the gradient products (sigma = 4)"""
    X = hp.as_f64(hp.saturated_u8(40, 53, seed=2)).astype(LD)
    if sigma == 4.0:
        Iy, Ix = hp.scharr(X)
        X = np.stack([Iy * Iy, Ix * Ix, Iy * Ix])
    p = hp.pad_for(sigma)
    a, b = hp.iir2(X, sigma, zero_ext, pad=p), hp.iir2(X, sigma, zero_ext, pad=2 * p)
    assert np.abs(a - b).max() <= 1e-18


def test_pad_covers_the_slowest_pole():
    for sigma in (1.0, 1.7, 4.0):
        assert hp.pole_modulus(sigma) ** hp.pad_for(sigma) < 2.0 ** -70
    assert 0.68 < hp.pole_modulus(4.0) < 0.70 and 125 <= hp.pad_for(4.0) <= 145


def test_resize_of_even_sizes_is_the_box_mean():
    X = np.random.default_rng(1).random((3, 20, 34)).astype(LD)
    box = (X[:, 0::2, 0::2] + X[:, 1::2, 0::2] + X[:, 0::2, 1::2] + X[:, 1::2, 1::2]) / 4
    assert np.abs(hp.resize_half(X) - box).max() <= 1e-18


def test_resize_of_odd_sizes_interpolates_a_ramp_exactly():
    y, x = np.mgrid[1:8, 1:12].astype(LD)
    R = hp.resize_half(3 * y - 2 * x)                              # 7 x 11 -> 4 x 6
    sy = LD(7) / 4 * (np.arange(1, 5, dtype=LD) - LD(0.5)) + LD(0.5)
    sx = LD(11) / 6 * (np.arange(1, 7, dtype=LD) - LD(0.5)) + LD(0.5)
    assert np.abs(R - (3 * sy[:, None] - 2 * sx[None, :])).max() <= 1e-17


def test_scharr_of_a_ramp_is_its_slope():
    y, x = np.mgrid[0:9, 0:13].astype(LD)
    Iy, Ix = hp.scharr(LD(0.25) * y - LD(0.125) * x)
    assert np.abs(Iy[1:-1, 1:-1] - LD(0.25)).max() <= 1e-18 and np.abs(Ix[1:-1, 1:-1] + LD(0.125)).max() <= 1e-18
    Iy0, _ = hp.scharr(np.ones((5, 5)), zero_border=True)          # Fill(0): the border rows see the step to zero
    assert Iy0[0, 2] == LD(0.5) and Iy0[-1, 2] == LD(-0.5) and Iy0[2, 2] == 0


# ---------------------------------------------------------------------------------------------------------------- what check rejects
@pytest.fixture(scope="module")
def base(orc):
    """two members of a batch (64 x 97, one coarser level): images, model, oracle planes"""
    H, W, lv = 64, 97, 1
    fr = [hp.as_f64(f) for f in hp.frames_u8(H, W, 2, seed=11)]
    mdl = hp.model(np.stack(fr), lv, 1)
    return dict(fr=fr, lv=lv, mdl=[hp.member(mdl, s) for s in range(2)], orc=[hp.Planes(orc.pyr_build(f, lv, 1.0, 1), lv) for f in fr])


def _copy(base):
    return [hp.Planes(p, base["lv"]) for p in base["orc"]]


def _rejected(base, dev, bound):
    with pytest.raises(AssertionError, match=r"\(%s\)" % bound):
        hp.check(dev, base["orc"], base["mdl"], "damaged")


def test_check_passes_the_undamaged_planes(base):
    rep = []
    assert hp.check(_copy(base), base["orc"], base["mdl"], "oracle", report=rep) == pytest.approx(1.0, abs=0.5)   # ratio 1 (or E_orc / 2^-52 below it)
    assert len(rep) == 2 * 2 * 6


def test_check_rejects_a_perturbed_segment_entry_state(base):
    """what a wrong entry state of the segment that starts at column 24 leaves in one row of the filtered Ixx: a transient
    1e-12 * max|Ixx| * 0.69^k, then the running sums.  BELOW 1e-11 (about 3.2e-12: the sum of the transient): only bound (b) sees it."""
    dev = _copy(base)
    P = dev[0].plane("Ixx", 0)
    H, W = P.shape
    d = np.zeros((H, W))
    d[20, 24:] = 1e-12 * np.abs(P).max() * 0.69 ** np.arange(W - 24)
    P += np.cumsum(np.cumsum(d, axis=0), axis=1)
    e = hp.E(dev[0], base["mdl"][0])[("Ixx", 0)]
    assert 64 * max(hp.E(base["orc"][0], base["mdl"][0])[("Ixx", 0)], hp.EPS64) < e < hp.BAR, e
    _rejected(base, dev, "b")


def test_check_rejects_a_column_total_off_by_256_ulp(base):
    """total - suffix running sums along y: a column total that is off by 256 ulp of the plane's maximum moves that column of the
    y-summed plane, and with it every later column of the integral image.  BELOW 1e-11 (2.8 - 5.7e-14, by where the maximum lies
    in its binade) and only a little above 64 x E_oracle, which is 1.4 - 5e-14 on the integral planes of this case: applied where
    the oracle is closest to the model (member 0, level 1: 3.3e-16)."""
    dev = _copy(base)
    P = dev[0].plane("Iyy", 1)
    P[:, 20:] += 256 * np.spacing(np.abs(P).max())
    e = hp.E(dev[0], base["mdl"][0])[("Iyy", 1)]
    assert 64 * max(hp.E(base["orc"][0], base["mdl"][0])[("Iyy", 1)], hp.EPS64) < e < hp.BAR, e
    _rejected(base, dev, "b")


def test_check_rejects_a_copied_last_column(base):
    """ABOVE 1e-11 (a wrong sample, not a rounding)"""
    dev = _copy(base)
    P = dev[0].plane("layers", 1)
    P[:, -1] = P[:, -2]
    _rejected(base, dev, "a")


def test_check_rejects_swapped_batch_members(base):
    """ABOVE 1e-11"""
    dev = _copy(base)
    _rejected(base, dev[::-1], "a")


def test_check_rejects_swapped_gradients(base):
    """ABOVE 1e-11"""
    dev = _copy(base)
    dev[1].d[("Iy", 1)], dev[1].d[("Ix", 1)] = dev[1].d[("Ix", 1)], dev[1].d[("Iy", 1)]
    _rejected(base, dev, "a")


def test_check_rejects_a_layer_of_a_slightly_different_sigma(base, orc):
    """level 1's layer blurred with sigma = 1 + 1e-9: about 1e-10 of the layer's range, ABOVE 1e-11"""
    dev = _copy(base)
    dev[0].d[("layers", 1)] = np.array(orc.pyr_build(base["fr"][0], 1, 1.0 + 1e-9, 1).plane("layers", 1))
    e = hp.E(dev[0], base["mdl"][0])[("layers", 1)]
    assert hp.BAR < e < 1e-8, e
    _rejected(base, dev, "a")


def test_check_takes_a_subset_of_planes(base):
    """target-only builds: layers of every level + level 0's planes; damage outside the subset is not looked at"""
    dev = _copy(base)
    dev[0].plane("Ixx", 1)[:] = 0
    which = {("layers", 0), ("layers", 1)} | {(n, 0) for n in hp.PLANES}
    hp.check(dev, base["orc"], base["mdl"], "subset", which=which)
    _rejected(base, dev, "a")


# ---------------------------------------------------------------------------------------------------------------- segment geometry
def test_every_row_kernel_variant_and_both_fallbacks_have_a_case():
    got = {hp.rt_seg_len(w) for _, w in hp.BATCH_CASES}
    assert got == {(m, 32) for m in hp.RT_MENU} | {(m, 64) for m in hp.RT_MENU_WIDE}
    assert [hp.rt_seg_len(w)[0] for w in hp.FALLBACK_WIDTHS] == [0, 0] and hp.FALLBACK_WIDTHS == (7, 2049)
    for m, ns in sorted(got):                                      # both ends of each variant's width range
        ws = [w for _, w in hp.BATCH_CASES if hp.rt_seg_len(w) == (m, ns)]
        assert hp.rt_seg_len(min(ws) - 1) != (m, ns) and hp.rt_seg_len(max(ws) + 1) != (m, ns), (m, ns, ws)
    # left padding of 0 and of SL - 1 samples, a row of exactly two segments
    pads = {(m, (-w) % m) for _, w in hp.BATCH_CASES for m in [hp.rt_seg_len(w)[0]]}
    assert (4, 0) in pads and (16, 15) in pads and hp.rt_seg_len(8) == (4, 32)
    # batch in the single-image role: 12 and 24 samples at 32 segments, and the 64-segment rows that fall to k_iir_seg
    assert hp.rt_seg_len(752)[0] == 24 and hp.rt_seg_len(1392) == (24, 64)
    assert {h for h, _ in hp.BATCH_CASES} == set(hp.BATCH_HEIGHTS)


def test_segment_lengths_of_the_single_image_cases():
    assert hp.seg_len(16, 128) == 4 and hp.seg_len(2048, 128) == 16 and hp.seg_len(2049, 128) == 17
    assert hp.single_is_fast(64, 2048) and not hp.single_is_fast(64, 2049) and not hp.single_is_fast(2049, 64)
    assert hp.expect_seg(512, 64, True)["slc32"] == 16 and hp.expect_seg(513, 64, True)["slc32"] == 0
    assert hp.expect_seg(64, 1281, True)["rows"] == "ROWS_SEG" and hp.expect_seg(64, 1280, True)["rows"] == "ROWS_TOL"
    assert hp.expect_tol_batch(64, 128, True)["dec"] == 1 and hp.expect_tol_batch(80, 128, True)["dec"] == 0
    assert hp.expect_tol_batch(65, 128, True)["resize"] == "RZ_PLAIN" and hp.expect_tol_batch(64, 128, False)["resize"] == "RZ_NONE"
