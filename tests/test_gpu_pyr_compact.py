"""GPU: the COMPACT batch builds (slam_pyr_update_batch_sel_dev / _u8_dev; PyramidBatch.update_selected_): member r of the batch receives the
build of the r-th selected stream, members at index n_sel or above keep their bytes.  A batch of 12 members at 96 x 128 and 97 x 131 (odd heights
take the other resize route), pyramid_levels = 3, 8-bit frames of synthetic.stereo_stream, one frame per stream; masks with
n_sel in {0, 1, 2, 7, 8, 9, 12} -- one image (the single-image routes on a batch's scratch), both sides of the tolerance batch threshold (4) and of
the batch integral-image threshold (8), the whole batch.  Each case runs with the library's default kernel selection (at these sizes: the line
kernels) and with SLAMHIP_CK_MIN_MB=0 (the checkpointed / fused kernels the throughput shape takes: k_cols_fused with its fused ingest through
srctab, k_iir_rows_ck, k_rows_cum, k_cols_fused<TOL> + k_rows_tol with the column totals `tot`), and asserts the route of the compact build
(slam.pyr_route of an n_sel-member build) before it looks at a plane.  The reference is an ordinary 12-member build of the same frames, made once
per shape, switch and kind.  Sub-batches (SLAMHIP_PYR_CHUNK_MB, read once per process) run in a child process: `python test_gpu_pyr_compact.py`.

Every build starts from a SENTINEL: an ordinary 12-member build of ONE other frame in every member, so that what a build does not write (a
member at index n_sel or above; the gradient planes a target-only build leaves alone at levels >= 1) is known and the same in every member."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NB, LEVELS = 12, 3
SHAPES = ((96, 128), (97, 131))
PLANES = ("layers", "Iy", "Ix", "Iyy", "Ixx", "Iyx")
COUNTS = (0, 1, 2, 7, 8, 9, 12)
KINDS = {"exact": dict(fast=False, target_only=False), "exact_target": dict(fast=False, target_only=True), "tolerance": dict(fast=True, target_only=False)}
TOL_PLANE = 1e-11            # the tolerance mode's stated plane bound, relative to the plane's largest magnitude (README, slamhip.h)


def masks():
    """one mask per count, the selected streams spread irregularly over the 12 (first and last stream in some, not in others)"""
    rng = np.random.default_rng(7)
    out = []
    for k in COUNTS:
        m = np.zeros(NB, np.uint8)
        m[rng.choice(NB, k, replace=False)] = 1
        out.append(m)
    return out


@contextlib.contextmanager
def ck_min(mb):
    """SLAMHIP_CK_MIN_MB as the library reads it at every build (None: the default threshold)"""
    old = os.environ.get("SLAMHIP_CK_MIN_MB")
    if mb is not None:
        os.environ["SLAMHIP_CK_MIN_MB"] = str(mb)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SLAMHIP_CK_MIN_MB", None)
        else:
            os.environ["SLAMHIP_CK_MIN_MB"] = old


def planes_of(batch, members):
    return {(r, nm, l): batch.pyramids[r].plane(nm, l) for r in members for nm in PLANES for l in range(LEVELS + 1)}


class Scene:
    """the 12 streams' frames (u8 and Float64, resident), the sentinel frame, and the ordinary builds the compact ones are held against"""

    def __init__(self, slam, syn, shape):
        import torch
        self.slam, self.shape = slam, shape
        H, W = shape
        left, right, _ = syn.stereo_stream(shape, NB, seed=41, step=(1.7, -2.3), disparity=5.0)
        f8 = [np.ascontiguousarray((np.clip(im, 0, 1) * 255).round().astype(np.uint8).T) for im in right]          # column-major H x W bytes
        s8 = np.ascontiguousarray((np.clip(left[3], 0, 1) * 255).round().astype(np.uint8).T)
        self.d8 = [torch.from_numpy(f).cuda() for f in f8]
        self.d64 = [torch.from_numpy(f.astype(np.float64) / 255.0).cuda() for f in f8]
        self.sent8 = torch.from_numpy(s8).cuda()
        torch.cuda.synchronize()
        self.batch = slam.PyramidBatch(shape, levels=LEVELS, S=NB)
        self.ref_batch = slam.PyramidBatch(shape, levels=LEVELS, S=NB)
        self._ref, self._sent = {}, {}

    def sentinel(self, batch, kind="exact"):
        """an ordinary build of the sentinel frame in every member (it clears the batch's compact record, too)"""
        batch.update_([self.sent8.data_ptr()] * batch.S, u8=True, **KINDS[kind])

    def sentinel_planes(self, ck):
        """the planes of a member after sentinel() (the same in every member: one frame), per switch"""
        if ck not in self._sent:
            with ck_min(ck):
                self.sentinel(self.ref_batch)
            self._sent[ck] = {(nm, l): self.ref_batch.pyramids[5].plane(nm, l) for nm in PLANES for l in range(LEVELS + 1)}
            for r in (0, NB - 1):
                assert all(np.array_equal(self.ref_batch.pyramids[r].plane(nm, l), self._sent[ck][nm, l]) for nm in PLANES for l in range(LEVELS + 1))
        return self._sent[ck]

    def reference(self, kind, ck):
        """planes of the ordinary 12-member build of the 12 frames (from the sentinel), made once per kind and switch and left unchanged"""
        if (kind, ck) not in self._ref:
            with ck_min(ck):
                self.sentinel(self.ref_batch)
                self.ref_batch.update_([d.data_ptr() for d in self.d8], u8=True, **KINDS[kind])
            self._ref[kind, ck] = planes_of(self.ref_batch, range(NB))
        return self._ref[kind, ck]


_SCENES = {}


@pytest.fixture(scope="module")
def scene(slam, syn):
    def get(shape):
        if shape not in _SCENES:
            _SCENES[shape] = Scene(slam, syn, shape)
        return _SCENES[shape]
    return get


def expected_route(kind, ck, n_sel, shape):
    """level 0 and level 1 of an n_sel-member build on a batch of 12 at these shapes (csrc/pyramid.hip: level_route)"""
    big = ck == 0                                                    # every level of >= 64 samples per line counts as bandwidth-bound
    if kind == "tolerance" and n_sel < 4:
        l0 = dict(family="FAM_SEG", cols="COLS_SEG", rows="ROWS_TOL")
    elif kind == "tolerance" and big:
        l0 = dict(family="FAM_TOLB", cols="COLS_FUSED", rows="ROWS_TOL")
    else:
        l0 = dict(family="FAM_EXACT", cols="COLS_FUSED" if big else "COLS_LINE", rows="ROWS_CK" if big else "ROWS_LINE",
                  cum="CUM_ROWS_CUM" if n_sel >= 8 else "CUM_LINES")
    l1 = dict(family="FAM_TARGET") if kind == "exact_target" else dict(family=l0["family"] if l0["family"] != "FAM_TOLB" else "FAM_EXACT")
    return l0, l1


def assert_route(slam, batch, kind, ck, n_sel, shape):
    mode = 3 if KINDS[kind]["fast"] else 1
    l0, l1 = expected_route(kind, ck, n_sel, shape)
    for level, want in ((0, l0), (1, l1)):
        got = slam.pyr_route(batch, mode, n_sel, level, target_only=KINDS[kind]["target_only"])
        assert {k: got[k] for k in want} == want, (kind, ck, n_sel, level, got)


def check_compact(slam, sc, kind, ck, mask, u8=True):
    """sentinel -> compact build under `mask` -> members below n_sel against the reference, the others against the sentinel"""
    n_sel = int(mask.sum())
    sel = np.flatnonzero(mask)
    ref_kind = "exact" if kind == "tolerance" else kind                # tolerance planes are held against the mode-1 planes
    ref, sent = sc.reference(ref_kind, ck), sc.sentinel_planes(ck)
    with ck_min(ck):
        if n_sel:
            assert_route(slam, sc.batch, kind, ck, n_sel, sc.shape)
        sc.sentinel(sc.batch)
        ptrs = [(sc.d8 if u8 else sc.d64)[s].data_ptr() if mask[s] else 0 for s in range(NB)]      # unselected pointers: 0, never read
        n = sc.batch.update_selected_(ptrs, mask, u8=u8, **KINDS[kind])
    assert n == n_sel
    got = planes_of(sc.batch, range(NB))
    worst = 0.0
    for r in range(NB):
        for nm in PLANES:
            for l in range(LEVELS + 1):
                g = got[r, nm, l]
                if r >= n_sel:
                    assert np.array_equal(g, sent[nm, l]), (kind, ck, n_sel, "member at or above n_sel was written", r, nm, l)
                elif kind == "tolerance":
                    w = ref[sel[r], nm, l]
                    err = float(np.abs(g - w).max() / max(np.abs(w).max(), 1e-300))
                    worst = max(worst, err)
                    assert err <= TOL_PLANE, (ck, n_sel, r, nm, l, err)
                else:
                    assert np.array_equal(g, ref[sel[r], nm, l]), (kind, ck, n_sel, "member r differs from stream sel[r]", r, int(sel[r]), nm, l)
    return worst


@pytest.mark.parametrize("ck", [None, 0], ids=["default_routes", "ck_min_0"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_compact_build_equals_the_ordinary_build_member_for_member(slam, scene, shape, kind, ck):
    sc = scene(shape)
    worst = 0.0
    for mask in masks():
        worst = max(worst, check_compact(slam, sc, kind, ck, mask))
    if kind == "tolerance":
        print(f"tolerance-mode compact planes within {worst:.2e} of the mode-1 planes (bound {TOL_PLANE:.0e})")
        assert worst > 0.0                                           # the tolerance kernels ran: their planes are not the exact ones bit for bit


def test_float64_frames(slam, scene):
    """slam_pyr_update_batch_sel_dev: Float64 frames holding raw / 255 give the planes of the 8-bit entry"""
    sc = scene(SHAPES[1])
    for mask in (masks()[2], masks()[5]):
        check_compact(slam, sc, "exact", 0, mask, u8=False)


def test_same_mask_twice_and_another_mask_of_the_same_count(slam, scene):
    """the second build of a count replays the graph the first one made; its planes are the first's; another mask of that count lands in the same members"""
    sc = scene(SHAPES[0])
    mask = masks()[3]
    with ck_min(0):
        sc.sentinel(sc.batch)
        ptrs = [d.data_ptr() for d in sc.d8]
        assert sc.batch.update_selected_(ptrs, mask, u8=True) == 7
        first = planes_of(sc.batch, range(NB))
        assert sc.batch.update_selected_(ptrs, mask, u8=True) == 7
        second = planes_of(sc.batch, range(NB))
        other = np.roll(mask, 1)
        assert not np.array_equal(other, mask) and sc.batch.update_selected_(ptrs, other, u8=True) == 7
        third = planes_of(sc.batch, range(7))
    assert all(np.array_equal(first[k], second[k]) for k in first)
    ref = sc.reference("exact", 0)
    for r, s in enumerate(np.flatnonzero(other)):
        assert all(np.array_equal(third[r, nm, l], ref[s, nm, l]) for nm in PLANES for l in range(LEVELS + 1)), (r, s)


def test_marks_are_set_on_the_built_members_only(slam, scene):
    """target_only is set on the members a compact build wrote and nowhere else: a match refuses a target-only SOURCE, so fb_tracking_ shows the mark"""
    sc = scene(SHAPES[0])
    mask = masks()[2]                                                # two streams
    sc.sentinel(sc.batch)
    sc.batch.update_selected_([d.data_ptr() for d in sc.d8], mask, u8=True, target_only=True)
    pts = np.array([[40.0, 50.0]])
    for r in (0, 1):
        with pytest.raises(RuntimeError, match="TARGET_ONLY"):
            slam.fb_tracking_(sc.batch.pyramids[r], sc.batch.pyramids[5], pts, window_size=9, pyramid_levels=3, max_distance=1.0)
    slam.fb_tracking_(sc.batch.pyramids[2], sc.batch.pyramids[5], pts, window_size=9, pyramid_levels=3, max_distance=1.0)     # a full (sentinel) member still


def test_more_selected_streams_than_members(slam, scene):
    """a batch of 4 members under a mask of 5: SLAM_ERR_ARG, nothing enqueued, the planes untouched; under a mask of 4 of 12 streams it builds"""
    from slam_jl_amd import _lib as L
    sc = scene(SHAPES[0])
    small = slam.PyramidBatch(sc.shape, levels=LEVELS, S=4)
    sc.sentinel(small)
    before = planes_of(small, range(4))
    m5 = np.zeros(NB, np.uint8); m5[[0, 3, 4, 8, 11]] = 1
    c = small.ctx
    imgs = (C.c_void_p * NB)(*[C.c_void_p(d.data_ptr()) for d in sc.d8])
    n_built = C.c_int(-5)
    rc = c.lib.slam_pyr_update_batch_sel_u8_dev(c.h, small._handles, 4, imgs, NB, L.ptr(m5, L.u8p), 1, 1.0, 1, C.byref(n_built))
    assert rc == -1 and n_built.value == 0                           # SLAM_ERR_ARG
    with pytest.raises(RuntimeError, match="5 streams selected but the batch has 4 members"):
        small.update_selected_([d.data_ptr() for d in sc.d8], m5, u8=True)
    after = planes_of(small, range(4))
    assert all(np.array_equal(before[k], after[k]) for k in before)
    m4 = m5.copy(); m4[8] = 0
    assert small.update_selected_([d.data_ptr() if m4[s] else None for s, d in enumerate(sc.d8)], m4, u8=True) == 4
    ref = sc.reference("exact", None)
    got = planes_of(small, range(4))
    for r, s in enumerate(np.flatnonzero(m4)):
        assert all(np.array_equal(got[r, nm, l], ref[s, nm, l]) for nm in PLANES for l in range(LEVELS + 1)), (r, s)
    # argument refusals: a selected stream without a frame, a member list that is not the batch's, no out-parameter
    bad = (C.c_void_p * NB)(*[C.c_void_p(d.data_ptr()) for d in sc.d8]); bad[3] = None
    assert c.lib.slam_pyr_update_batch_sel_u8_dev(c.h, small._handles, 4, bad, NB, L.ptr(m4, L.u8p), 1, 1.0, 1, C.byref(n_built)) == -1
    assert c.lib.slam_pyr_update_batch_sel_u8_dev(c.h, small._handles, 3, imgs, NB, L.ptr(m4, L.u8p), 1, 1.0, 1, C.byref(n_built)) == -1
    assert c.lib.slam_pyr_update_batch_sel_u8_dev(c.h, small._handles, 4, imgs, NB, L.ptr(m4, L.u8p), 1, 1.0, 1, None) == -1
    again = planes_of(small, range(4))
    assert all(np.array_equal(got[k], again[k]) for k in got)


def test_sub_batches_in_a_child_process(slam):
    """SLAMHIP_PYR_CHUNK_MB=1 (read once per process): builds of >= 8 members run in sub-batches of 4 at level 0, so n_sel = 8, 9, 12 are chunked
    (9: a last chunk of one image) and 7 is not -- the same member-for-member checks, in a fresh process"""
    env = dict(os.environ, SLAMHIP_PYR_CHUNK_MB="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "compact sub-batches OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import slam_jl_amd
    from slam_jl_amd import synthetic
    assert os.environ.get("SLAMHIP_PYR_CHUNK_MB") == "1"
    slam_jl_amd.default_context(0)
    for shape_ in SHAPES:
        sc_ = Scene(slam_jl_amd, synthetic, shape_)
        for kind_ in ("exact", "tolerance"):
            for mask_ in masks()[3:]:
                check_compact(slam_jl_amd, sc_, kind_, 0, mask_)
    print("compact sub-batches OK")
