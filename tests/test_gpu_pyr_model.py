"""GPU: the tolerance-mode pyramid build (mode 3) plane by plane against the long-double model of tests/hp_pyr.py, at the geometry edges
of its kernels: every k_rows_tol instantiation in the batch role at both ends of its width range, the widths no variant fits, the
62-column strips and 32-row blocks of k_cols_fused<TOL>, chained levels, and the single-image segment kernels.

Every case builds 8-bit frames (different per batch member), runs the build twice (the second run is the cached graph replay), asserts
the ROUTE the build took through slam.pyr_route -- so a changed threshold cannot silently turn a case into one more test of the exact
kernels -- and then calls hp_pyr.check: (a) E_dev <= 1e-11 against the model, (b) E_dev <= 64 x max(E_oracle, 2^-52) with the C oracle's
own distance from the model on the same image.  Each case prints its worst ratio E_dev / max(E_oracle, 2^-52) per plane kind and level."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hp_pyr as hp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 4                                    # the smallest batch that takes the batch kernels (SLAMHIP_TOL_BATCH_MIN_S default)


def _route(slam, p, mode, n, level, **want):
    r = slam.pyr_route(p, mode, n, level, target_only=want.pop("target_only", False))
    got = {k: r[k] for k in want}
    assert got == want, (level, got, want, r)
    return r


def _refs(orc, fr, levels):
    """the model (all members in one pass) and the oracle's planes of every frame"""
    f64 = [hp.as_f64(f) for f in fr]
    mdl = hp.model(np.stack(f64), levels, 1)
    return [hp.member(mdl, s) for s in range(len(fr))], [orc.pyr_build(f, levels, 1.0, 1) for f in f64]


def _batch(slam, fr, levels, u8=True, fast=True, target_only=False, pb=None):
    """PyramidBatch of the frames, built twice; returns (batch, the tensor that keeps the frames alive)"""
    import torch
    H, W = fr[0].shape
    if u8:
        dev = torch.from_numpy(np.stack([np.ascontiguousarray(f.T) for f in fr])).cuda(); step = H * W
    else:
        dev = torch.from_numpy(np.stack([np.ascontiguousarray(hp.as_f64(f).T) for f in fr])).cuda(); step = H * W * 8
    torch.cuda.synchronize()
    ptrs = [dev.data_ptr() + s * step for s in range(len(fr))]
    pb = pb or slam.PyramidBatch((H, W), levels=levels, S=len(fr))
    pb.update_(ptrs, u8=u8, fast=fast, target_only=target_only)
    pb.update_(ptrs, u8=u8, fast=fast, target_only=target_only)
    return pb, dev


def _assert_batch_routes(slam, pb, H, W, levels, n):
    """levels of >= 64 rows whose width a k_rows_tol variant fits are on the batch tolerance kernels, the rest on the exact ones"""
    for l, (h, w) in enumerate(hp.level_shapes(H, W, levels)):
        if h >= 64 and hp.rt_seg_len(w)[0]:
            _route(slam, pb, 3, n, l, **hp.expect_tol_batch(h, w, l < levels))
        else:
            _route(slam, pb, 3, n, l, family="FAM_EXACT")


def _check(pb_or_list, ref_orc, mdl, levels, tag, which=None):
    pyrs = pb_or_list.pyramids if hasattr(pb_or_list, "pyramids") else pb_or_list
    dev = [hp.Planes(p, levels) if which is None else p for p in pyrs]
    rep = []
    try:
        hp.check(dev, ref_orc, mdl, tag, which=which, report=rep)
    finally:
        print(f"RATIO {tag}: {hp.ratio_table(rep)}")
    return dev


# ---------------------------------------------------------------------------------------------------------------- batch tolerance family
@pytest.mark.parametrize("H,W", hp.BATCH_CASES)
def test_batch_every_row_variant_at_both_ends_of_its_widths(slam, orc, monkeypatch, H, W):
    monkeypatch.setenv("SLAMHIP_CK_MIN_MB", "0")
    fr = hp.frames_u8(H, W, S, seed=H + W)
    pb, _keep = _batch(slam, fr, 1)
    r = _route(slam, pb, 3, S, 0, **hp.expect_tol_batch(H, W, True))
    assert (r["rt_sl"], r["rt_ns"]) == hp.rt_seg_len(W) and r["rt_sl"] > 0
    _assert_batch_routes(slam, pb, H, W, 1, S)                    # level 1: under 64 rows (or 4 columns) the exact kernels on the device's layer; 65 rows: k_rows_tol again
    mdl, ref = _refs(orc, fr, 1)
    _check(pb, ref, mdl, 1, f"batch {H}x{W} SL{r['rt_sl']}/NS{r['rt_ns']} dec{r['dec']}")


@pytest.mark.parametrize("W", hp.FALLBACK_WIDTHS)
def test_batch_widths_no_row_variant_fits_take_the_exact_kernels(slam, orc, monkeypatch, W):
    monkeypatch.setenv("SLAMHIP_CK_MIN_MB", "0")
    H = 64
    fr = hp.frames_u8(H, W, S, seed=W)
    pb, _keep = _batch(slam, fr, 1)
    for l in (0, 1):
        r = _route(slam, pb, 3, S, l, family="FAM_EXACT")
        assert r["rt_sl"] == 0 or l == 1
    for s in range(S):
        ref = orc.pyr_build(hp.as_f64(fr[s]), 1, 1.0, 1)
        for l in (0, 1):
            for n in hp.PLANES:
                assert np.array_equal(pb.pyramids[s].plane(n, l), ref.plane(n, l)), (s, n, l)


@pytest.mark.parametrize("H,W,u8", [(h, w, True) for h, w in hp.STRIP_CASES] + [(97, 125, False)])
def test_batch_column_strips_and_row_blocks(slam, orc, monkeypatch, H, W, u8):
    """k_cols_fused<TOL>: widths around its 62-column strips, heights around its 32-row blocks; one case ingests Float64 frames (8-bit
    ingest is fused into the kernel, Float64 ingest too but through its other source path)"""
    monkeypatch.setenv("SLAMHIP_CK_MIN_MB", "0")
    fr = hp.frames_u8(H, W, S, seed=3 * H + W)
    pb, _keep = _batch(slam, fr, 1, u8=u8)
    _assert_batch_routes(slam, pb, H, W, 1, S)
    _route(slam, pb, 3, S, 0, family="FAM_TOLB", cols="COLS_FUSED")
    mdl, ref = _refs(orc, fr, 1)
    _check(pb, ref, mdl, 1, f"strips {H}x{W} {'u8' if u8 else 'f64'}")


@pytest.fixture(scope="module")
def chain_1531(orc):
    H, W, lv = hp.CHAIN_CASES[0]
    fr = hp.frames_u8(H, W, S, seed=1531)
    return (fr,) + _refs(orc, fr, lv)


def test_batch_levels_chained_all_on_the_tolerance_kernels(slam, monkeypatch, chain_1531):
    """256 x 1531, 3 levels: widths 1531 / 766 / 383 (k_rows_tol<24, 64>, <24, 32>, <12, 32>), heights 256 / 128 / 64"""
    monkeypatch.setenv("SLAMHIP_CK_MIN_MB", "0")
    H, W, lv = hp.CHAIN_CASES[0]
    fr, mdl, ref = chain_1531
    pb, _keep = _batch(slam, fr, lv)
    for l, (h, w) in enumerate(hp.level_shapes(H, W, lv)):
        _route(slam, pb, 3, S, l, **hp.expect_tol_batch(h, w, l < lv))
    _check(pb, ref, mdl, lv, f"chain {H}x{W}")


def test_batch_target_only_layers_and_level_0(slam, monkeypatch, chain_1531):
    """target_only: the layer of every level + the finest level's planes"""
    monkeypatch.setenv("SLAMHIP_CK_MIN_MB", "0")
    H, W, lv = hp.CHAIN_CASES[0]
    fr, mdl, ref = chain_1531
    pb, _keep = _batch(slam, fr, lv, target_only=True)
    _route(slam, pb, 3, S, 0, target_only=True, **hp.expect_tol_batch(H, W, True))
    _route(slam, pb, 3, S, 1, target_only=True, family="FAM_TARGET")
    _route(slam, pb, 3, S, lv, target_only=True, family="FAM_NONE")
    which = {("layers", l) for l in range(lv + 1)} | {(n, 0) for n in hp.PLANES}
    _check(pb, ref, mdl, lv, f"target-only {H}x{W}", which=which)


def test_batch_last_level_falls_to_the_exact_family(slam, orc, monkeypatch):
    """259 x 640, 4 levels of 259 / 130 / 65 / 33 rows: the last one is under 64 rows, takes the exact kernels, and equals the oracle's
    planes of the DEVICE's level-3 layer bit for bit; through the model it meets the same bound as the levels above it"""
    monkeypatch.setenv("SLAMHIP_CK_MIN_MB", "0")
    H, W, lv = hp.CHAIN_CASES[1]
    fr = hp.frames_u8(H, W, S, seed=259)
    pb, _keep = _batch(slam, fr, lv)
    _assert_batch_routes(slam, pb, H, W, lv, S)
    _route(slam, pb, 3, S, 2, family="FAM_TOLB"); _route(slam, pb, 3, S, 3, family="FAM_EXACT")
    mdl, ref = _refs(orc, fr, lv)
    dev = _check(pb, ref, mdl, lv, f"chain {H}x{W}")
    for s in range(S):
        top = orc.pyr_build(dev[s].plane("layers", lv), 0, 1.0, 1)
        for n in hp.PLANES:
            assert np.array_equal(dev[s].plane(n, lv), top.plane(n, 0)), (s, n)


def test_exact_mode_afterwards_on_the_same_batch_is_bit_exact(slam, orc, monkeypatch):
    monkeypatch.setenv("SLAMHIP_CK_MIN_MB", "0")
    H, W = 80, 193
    fr = hp.frames_u8(H, W, S, seed=80)
    pb, _keep = _batch(slam, fr, 1)
    _route(slam, pb, 3, S, 0, family="FAM_TOLB")
    _batch(slam, fr, 1, fast=False, pb=pb)
    _route(slam, pb, 1, S, 0, family="FAM_EXACT")
    for s in range(S):
        ref = orc.pyr_build(hp.as_f64(fr[s]), 1, 1.0, 1)
        for l in (0, 1):
            for n in hp.PLANES:
                assert np.array_equal(pb.pyramids[s].plane(n, l), ref.plane(n, l)), (s, n, l)


# ---------------------------------------------------------------------------------------------------------------- single-image family
@pytest.mark.parametrize("H,W,lv", hp.SINGLE_CASES)
def test_single_image_segment_kernels(slam, orc, H, W, lv):
    fr = hp.frames_u8(H, W, 2, seed=H * 3 + W)[1:]                # the saturated / checkerboard kind
    p = slam.LKPyramid(shape=(H, W), levels=lv)
    slam.update_(p, fr[0], fast=True); slam.update_(p, fr[0], fast=True)
    if not hp.single_is_fast(H, W):                               # a line of more than 2048 samples: the exact route, bit for bit
        ref = orc.pyr_build(hp.as_f64(fr[0]), lv, 1.0, 1)
        for l in range(lv + 1):
            _route(slam, p, 3, 1, l, family="FAM_EXACT")
            for n in hp.PLANES:
                assert np.array_equal(p.plane(n, l), ref.plane(n, l)), (n, l)
        return
    for l, (h, w) in enumerate(hp.level_shapes(H, W, lv)):
        _route(slam, p, 3, 1, l, **hp.expect_seg(h, w, l < lv))
    mdl, ref = _refs(orc, fr, lv)
    _check([p], ref, mdl, lv, f"single {H}x{W}")


# ---------------------------------------------------------------------------------------------------------------- knobs read once per process
CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import hp_pyr as hp, test_gpu_pyr_model as t
import slam_jl_amd as slam
from oracle import oracle as orc
slam.default_context(0)
H, W, n = %(H)d, %(W)d, %(n)d
fr = hp.frames_u8(H, W, max(n, 2), seed=H + W)[-n:]
mdl, ref = t._refs(orc, fr, 1)
if n > 1:
    pb, keep = t._batch(slam, fr, 1)
    t._route(slam, pb, 3, n, 0, **dict(hp.expect_tol_batch(H, W, True), %(want)s))
    t._check(pb, ref, mdl, 1, %(tag)r)
else:
    p = slam.LKPyramid(shape=(H, W), levels=1)
    slam.update_(p, fr[0], fast=True); slam.update_(p, fr[0], fast=True)
    t._route(slam, p, 3, 1, 0, **hp.expect_seg(H, W, True, %(want)s))
    t._check([p], ref, mdl, 1, %(tag)r)
print("OK")
'''


def _child(env, H, W, n, want, tag):
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), H=H, W=W, n=n, want=want, tag=tag)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-800:] + r.stderr[-1500:]


def test_knob_no_tol_dec_in_a_process_of_its_own():
    """SLAMHIP_NO_TOL_DEC=1: the blurred layer leaves k_cols_fused at full height where the default halves it (even height, pitch % 32 == 0)"""
    _child({"SLAMHIP_NO_TOL_DEC": "1", "SLAMHIP_CK_MIN_MB": "0"}, 64, 321, S, "dec=0", "batch 64x321 NO_TOL_DEC")


def test_knob_no_rows_tol_single_in_a_process_of_its_own():
    """SLAMHIP_NO_ROWS_TOL_SINGLE=1: the rows of a single image through k_iir_seg<false> + k_cum_seg instead of k_rows_tol"""
    _child({"SLAMHIP_NO_ROWS_TOL_SINGLE": "1"}, 65, 97, 1, "rows_tol_single=False", "single 65x97 NO_ROWS_TOL_SINGLE")
