"""GPU: slam_kpset_stereo_match_compact (KeypointSet.stereo_match(..., compact=True)) -- the stereo match of a key-frame into a COMPACT right batch
(PyramidBatch.update_selected_: member r holds the build of the r-th selected stream), against a control set that goes through the ordinary
whole-batch right build + slam_kpset_stereo_match under the same selection: every field the three downloads show, the list lengths, the key-frame
counters and (through a detect that follows) the id counters, byte for byte; unselected streams byte for byte as before the call.  S = 5 and S = 70
(both sides of a wave of workgroup indices, as test_gpu_kpset_select.py), lists with 3-D and 2-D keypoints (that file's _Case, with map points so
that prior 1 projects where the match is), prior 2 and prior 1, masks none / one / all / alternating / random.  The compact batch has exactly
max(n_sel, 1) members -- fewer than S.  The record-less prologue (SLAMHIP_NO_MATCH_REC=1, read once per process) runs the same checks in a child
process: `python test_gpu_stereo_match_compact.py`."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_kpset_select import _Case, _diff, _snap  # noqa: E402

pytestmark = pytest.mark.gpu

DISP = 6.3                                                              # test_gpu_kpset._setup's stereo_stream disparity


def masks_for(S):
    rng = np.random.default_rng(S)
    one = np.zeros(S, np.uint8); one[S - 2] = 1
    alt = np.zeros(S, np.uint8); alt[1::2] = 1
    rnd = (rng.random(S) < 0.4).astype(np.uint8); rnd[0] = 1; rnd[S - 1] = 0
    return {"none": np.zeros(S, np.uint8), "one": one, "all": np.ones(S, np.uint8), "alternating": alt, "random": rnd}


class Stereo:
    """a _Case whose 3-D keypoints carry map points: the point at depth Z behind the pixel, so that prior 1 (projection into the right camera at
    baseline DISP Z / fx) lands DISP pixels to the left, where prior 2's shift puts it"""

    def __init__(self, slam, orc, syn, texture, S):
        self.slam, self.syn, self.S = slam, syn, S
        self.case = _Case(slam, orc, syn, texture, S, 96, 128, 80, lambda s: 30 + (s * 7) % 40)
        fx, fy, cx, cy = syn.KITTI_CAM
        Z = 20.0
        self.xyz = [np.stack([(k[:, 1] - cx) / fx * Z, (k[:, 0] - cy) / fy * Z, np.full(len(k), Z)], axis=1) for k in self.case.kps]
        Tcw = np.eye(4); Tcw[0, 3] = -DISP * Z / fx
        self.sp = {2: self.case.sps, 1: slam.stream_params(S, Tcw=Tcw, cam=syn.KITTI_CAM)}
        self.check = tuple(range(S)) if S <= 8 else (0, 1, 2, 31, 62, 63, 64, 65, 68, 69)
        self.before = None

    def new_set(self):
        c = self.case
        ks = self.slam.KeypointSet(c.S, c.cap)
        for s in range(c.S):
            ks.upload(s, c.kps[s], c.is3[s], xyz=self.xyz[s])
        ks.keyframe()
        ks.flow_match(c.a, c.b, c.params, c.sp, prior=2)
        if self.before is None:
            self.before = {s: _snap(ks, s) for s in self.check}
        return ks

    def right_ptrs(self, mask):
        """the right frames by stream; an unselected stream's pointer is 0 (never read)"""
        return [d.data_ptr() if mask[s] else 0 for s, d in enumerate(self.case.keep[2])]

    def compact_batch(self, mask, **kw):
        rb = self.slam.PyramidBatch((96, 128), levels=3, S=max(int(mask.sum()), 1))
        assert rb.update_selected_(self.right_ptrs(mask), mask, **kw) == int(mask.sum())
        return rb


def check_mask(st, mask, prior):
    """control (ordinary build + ordinary match) against compact build + compact match under `mask`; then the id counters through a detect"""
    c = st.case
    ctrl, A = st.new_set(), st.new_set()
    for ks in (ctrl, A):
        ks.select(mask)
    ctrl.stereo_match(c.b, c.r, c.params, st.sp[prior], prior=prior)
    rb = st.compact_batch(mask)
    assert rb.S <= st.S and (rb.S < st.S or mask.all())
    A.stereo_match(c.b, rb, c.params, st.sp[prior], prior=prior, compact=True)
    moved = 0
    for s in st.check:
        got, want = _snap(A, s), _snap(ctrl, s)
        assert _diff(got, want) == [], (st.S, prior, s, "compact differs from the control")
        if mask[s]:
            moved += int(got["has_stereo"].sum())
        else:
            assert _diff(got, st.before[s]) == [], (st.S, prior, s, "unselected stream changed")
    if any(mask[s] for s in st.check):
        assert moved > 3, (st.S, prior, moved)                         # the match matched: the comparison is not between two sets nothing happened to
    for ks in (ctrl, A):                                                # next_id: the ids a detect appends now
        ks.select(None)
        ks.detect(c.e, c.b)
    for s in st.check:
        assert _diff(_snap(A, s), _snap(ctrl, s)) == [], (st.S, prior, s, "after the detect")
    ctrl.close(); A.close()


_ST = {}


@pytest.fixture(scope="module")
def stereo(slam, orc, syn, texture):
    def get(S):
        if S not in _ST:
            _ST[S] = Stereo(slam, orc, syn, texture, S)
        return _ST[S]
    return get


@pytest.mark.parametrize("prior", [2, 1])
@pytest.mark.parametrize("name", ["none", "one", "all", "alternating", "random"])
@pytest.mark.parametrize("S", [5, 70])
def test_compact_match_equals_whole_batch_match(stereo, S, name, prior):
    st = stereo(S)
    check_mask(st, masks_for(S)[name], prior)


def test_prior_1_projects_where_the_match_is(stereo):
    """the prepared map points make prior 1 a real prior: 3-D keypoints get a stereo match through it, and some lie outside and are removed"""
    st = stereo(5)
    ks = st.new_set()
    n0 = ks.counts()
    ks.stereo_match(st.case.b, st.case.r, st.case.params, st.sp[1], prior=1)
    n1 = ks.counts()
    d = [ks.download(s) for s in range(5)]
    assert sum(int((x["is_3d"] & x["has_stereo"]).sum()) for x in d) > 5 and (n1 <= n0).all()
    ks.close()


def test_record_less_prologue_in_a_child_process(slam):
    """SLAMHIP_NO_MATCH_REC=1: k_kpset_match takes the target member from the set's rank table, not from a work record"""
    env = dict(os.environ, SLAMHIP_NO_MATCH_REC="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "compact match without records OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@contextlib.contextmanager
def ck_min_0():
    os.environ["SLAMHIP_CK_MIN_MB"] = "0"
    try:
        yield
    finally:
        os.environ.pop("SLAMHIP_CK_MIN_MB", None)


def test_tolerance_mode_compact_against_ordinary_tolerance_mode(stereo, slam):
    """Mode 3 on both sides (the contracted-arithmetic tracking kernels; SLAMHIP_CK_MIN_MB=0 so that the ordinary 70-member build takes
    k_cols_fused<TOL> + k_rows_tol, while a compact build of fewer than 4 streams takes the single-image segment kernels): the compact path against
    the ordinary mode-3 path -- lists and stereo flags equal, stereo pixels within 1e-6 px.  Admission first: on these inputs the ordinary mode-3
    path shows no flag flip against mode 1, so no keypoint sits on a threshold behind which a failure could hide."""
    S = 70
    st, c = stereo(S), stereo(S).case
    with ck_min_0():
        assert slam.pyr_route(c.r, 3, S, 0)["family"] == "FAM_TOLB" and slam.pyr_route(c.r, 3, 2, 0)["family"] == "FAM_SEG"
        b3 = slam.PyramidBatch((96, 128), levels=3, S=S); r3 = slam.PyramidBatch((96, 128), levels=3, S=S)
        b3.update_([d.data_ptr() for d in c.keep[1]], fast=True); r3.update_([d.data_ptr() for d in c.keep[2]], fast=True)
        worst = 0.0
        for name in ("one", "random", "all"):
            mask = masks_for(S)[name]
            m1, t3, A = st.new_set(), st.new_set(), st.new_set()
            for ks in (m1, t3, A):
                ks.select(mask)
            m1.stereo_match(c.b, c.r, c.params, st.sp[2], prior=2)
            t3.stereo_match(b3, r3, c.params, st.sp[2], prior=2)
            rb = st.compact_batch(mask, fast=True)
            assert slam.pyr_route(rb, 3, int(mask.sum()), 0)["family"] == ("FAM_SEG" if mask.sum() < 4 else "FAM_TOLB")
            A.stereo_match(b3, rb, c.params, st.sp[2], prior=2, compact=True)
            for s in st.check:
                exact, tol, got = _snap(m1, s), _snap(t3, s), _snap(A, s)
                # admission: mode 3 against mode 1, no flips
                admitted = np.array_equal(tol["ids"], exact["ids"]) and np.array_equal(tol["has_stereo"], exact["has_stereo"])
                assert admitted, (name, s, "not admitted: mode 3 flips a flag on these inputs")
                rest = [k for k in _diff(got, tol) if k != "stereo_yx"]
                assert rest == [], (name, s, rest)
                up = got["has_stereo"]
                if up.any():
                    err = float(np.abs(got["stereo_yx"][up] - tol["stereo_yx"][up]).max())
                    worst = max(worst, err)
                    assert err <= 1e-6, (name, s, err)
                if not mask[s]:
                    assert _diff(got, st.before[s]) == [], (name, s)
            for ks in (m1, t3, A):
                ks.close()
    print(f"compact against ordinary tolerance mode: stereo pixels within {worst:.2e} px (bound 1e-6)")


def test_stale_build_is_refused(stereo):
    st, c = stereo(5), stereo(5).case
    mA, mB = np.array([1, 0, 1, 1, 0], np.uint8), np.array([1, 1, 0, 1, 0], np.uint8)      # same count, other streams
    A = st.new_set()
    A.select(mA)
    rb = st.compact_batch(mA)
    A.select(mB)
    with pytest.raises(RuntimeError, match="stale build.*another selection"):
        A.stereo_match(c.b, rb, c.params, st.sp[2], prior=2, compact=True)
    for s in st.check:
        assert _diff(_snap(A, s), st.before[s]) == [], s                # the lists are untouched
    # the same selection, but an ordinary build since
    full = st.slam.PyramidBatch((96, 128), levels=3, S=5)
    full.update_selected_(st.right_ptrs(mB), mB)
    full.update_([d.data_ptr() for d in c.keep[2]])
    with pytest.raises(RuntimeError, match="stale build.*ordinary"):
        A.stereo_match(c.b, full, c.params, st.sp[2], prior=2, compact=True)
    with pytest.raises(RuntimeError, match="stale build.*ordinary"):
        A.stereo_match(c.b, c.r, c.params, st.sp[2], prior=2, compact=True)
    for s in st.check:
        assert _diff(_snap(A, s), st.before[s]) == [], s
    # a compact build of some streams and no selection on the set: refused as well; a batch too small for the selection never gets that far
    A.select(None)
    with pytest.raises(RuntimeError, match="stale build"):
        A.stereo_match(c.b, rb, c.params, st.sp[2], prior=2, compact=True)
    # and the right build under the right selection goes through
    A.select(mB)
    full.update_selected_(st.right_ptrs(mB), mB)
    A.stereo_match(c.b, full, c.params, st.sp[2], prior=2, compact=True)
    assert _diff(_snap(A, 1), st.before[1]) != [] and _diff(_snap(A, 2), st.before[2]) == []
    A.close()


def test_no_selection_compact_is_the_ordinary_call(stereo):
    st, c = stereo(5), stereo(5).case
    ctrl, A, B = st.new_set(), st.new_set(), st.new_set()
    ctrl.stereo_match(c.b, c.r, c.params, st.sp[2], prior=2)
    A.stereo_match(c.b, c.r, c.params, st.sp[2], prior=2, compact=True)            # an ordinary build, no selection
    rb = st.compact_batch(np.ones(5, np.uint8))                                    # a compact build of every stream: member s = stream s
    B.stereo_match(c.b, rb, c.params, st.sp[2], prior=2, compact=True)
    for s in st.check:
        assert _diff(_snap(A, s), _snap(ctrl, s)) == [] and _diff(_snap(B, s), _snap(ctrl, s)) == [], s
        assert _diff(_snap(ctrl, s), st.before[s]) != [], s
    for ks in (ctrl, A, B):
        ks.close()


if __name__ == "__main__":
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    import slam_jl_amd
    from slam_jl_amd import synthetic
    from oracle import oracle
    assert os.environ.get("SLAMHIP_NO_MATCH_REC") == "1"
    oracle.lib()
    slam_jl_amd.default_context(0)
    tex = lambda H, W, n=2, seed=0, step=(1.3, -2.1), disparity=12.4: synthetic.stereo_stream((H, W), n, seed, step, disparity)
    for S_ in (5, 70):
        st_ = Stereo(slam_jl_amd, oracle, synthetic, tex, S_)
        for name_, mask_ in masks_for(S_).items():
            for prior_ in (2, 1):
                check_mask(st_, mask_, prior_)
    print("compact match without records OK")
