"""GPU: EVERY hypothesis of the five-point RANSAC against the CPU oracle, not only the winner.

slam_five_point_ransac returns one hypothesis per call; each 5-tuple yields up to ten essential matrices and each call evaluates dozens
of tuples, so a defect confined to one team position of k_5pt_solve's wave, to the 7th-10th interval lane of its root search, to its
failure path or to an invalid tuple next to valid ones only changes losers.  The test seam slamhip_test_five_point_hypotheses (the same
staging and launches, the scratch filled with 0xFF bytes beforehand) reads out ne, every E, every pose, k_5pt_score's counts and the
incumbents; the oracle side is orc_five_point_solve + orc_essential_pose_cheirality + orc_two_view_inliers per tuple.  Everything is
array_equal: solver, polish, pose recovery and triangulation use only + - * / sqrt in the oracle's order.

Which losers k_5pt_score drops early depends on timing: loser counts are never compared between runs, only against the oracle's full
or prefix counts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_5pt as m5  # noqa: E402

pytestmark = pytest.mark.gpu
THR = 3.0
CALL = 67                                   # tuples per call: 17 solver workgroups, the last one with three teams


def _valid(t, n):
    return all(0 <= int(i) < n for i in t) and len(set(int(i) for i in t)) == 5


def _oracle_hyps(orc, sc, tuples, masks=False):
    """per tuple: (Es (k, 3, 3), poses (k, 12) column-major, masks (k, n) or None) -- what k_5pt_solve must leave for it"""
    n = len(sc["px1"])
    out = []
    for t in np.asarray(tuples):
        Es, Ps, Ms = [], [], []
        if _valid(t, n):
            q1, q2 = sc["pd1"][t], sc["pd2"][t]
            for E in orc.five_point_solve(q1, q2):
                P = orc.essential_pose_cheirality(E, q1, q2)
                if P is None:
                    continue
                Es.append(E); Ps.append(P.T.reshape(12))
                if masks:
                    Ms.append(orc.two_view_inliers(sc["px1"], sc["px2"], sc["K"], sc["K"], P, THR))
        out.append((np.array(Es).reshape(-1, 3, 3), np.array(Ps).reshape(-1, 12), np.array(Ms).reshape(len(Es), n) if masks else None))
    return out


def _run(slam, sc, tuples):
    res, hyp = slam.pose.five_point_hypotheses([sc["px1"]], [sc["px2"]], [sc["pd1"]], [sc["pd2"]], sc["K"], sc["K"], THR, [tuples])
    return res[0], {k: v[0] for k, v in hyp.items()}


def _all_ff(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


def _check_solve(hyp, ref, where):
    """ne, every E and every pose equal the oracle's; the slots behind them were never written"""
    for it, (Es, Ps, _) in enumerate(ref):
        k = len(Es)
        assert hyp["ne"][it] == k, (where, it, int(hyp["ne"][it]), k)
        assert np.array_equal(hyp["Es"][it, :k], Es, equal_nan=True), (where, it)
        assert np.array_equal(hyp["poses"][it, :k], Ps, equal_nan=True), (where, it)
        assert _all_ff(hyp["Es"][it, k:]) and _all_ff(hyp["poses"][it, k:]), (where, it)


def _check_winner(orc, sc, tuples, res):
    ref = orc.five_point_ransac(sc["px1"], sc["px2"], sc["pd1"], sc["pd2"], sc["K"], sc["K"], THR, tuples)
    cnt, (E, P, inl, err, bi) = res
    assert cnt == ref[0] and bi == ref[5], (cnt, ref[0], bi, ref[5])
    assert np.array_equal(E, ref[1]) and np.array_equal(P, ref[2]) and np.array_equal(inl, ref[3]) and err == ref[4]
    return ref


def test_every_hypothesis_in_every_team_position(slam, orc, syn):
    """The case list of the model test (tests/np_5pt.py: 768 mixed + 800 noise-free tuples + searched tuples with eight real solutions), n = 60,
    in calls of 67 tuples; the same calls rotated by 1, 2, 3 places, so that a tuple visits the four team positions of a solver wave."""
    n_tuples = n_hyp = 0
    for name, sc, tuples, _ in m5.groups(syn):
        reps = -(-len(tuples) // CALL) * CALL
        padded = np.ascontiguousarray(np.resize(tuples, (reps, 5)), dtype=np.int32)         # cyclic fill of the last call
        ref_all = _oracle_hyps(orc, sc, padded, masks=True)
        for c0 in range(0, reps, CALL):
            for rot in range(4):
                order = np.roll(np.arange(c0, c0 + CALL), rot)
                res, hyp = _run(slam, sc, padded[order])
                ref = [ref_all[i] for i in order]
                _check_solve(hyp, ref, (name, c0, rot))
                for it, (Es, _, Ms) in enumerate(ref):                                       # n <= 64: one chunk, no pose is dropped early
                    assert np.array_equal(hyp["counts"][it, :len(Es)], Ms.sum(1)), (name, c0, rot, it)
                    assert not hyp["counts"][it, len(Es):].any()
                if rot == 0:
                    _check_winner(orc, sc, padded[order], res)
                    n_tuples += CALL; n_hyp += int(hyp["ne"].sum())
    print(f"every hypothesis: {n_tuples} tuples, {n_hyp} hypotheses, x 4 team positions")
    assert n_tuples >= 1568 and n_hyp > 4 * n_tuples


def test_invalid_tuples_inside_a_wave(slam, orc, syn):
    """index -1, index >= n, a repeated index: one invalid tuple in each of the four positions of a wave of valid ones, waves with exactly one valid
    tuple in each position, a wave without any (the kernel's early exit), a partial last wave."""
    sc = syn.five_point_scene(n=60, seed=11, noise_px=0.3, iters=40)
    good = [t for t in sc["samples"]]
    bad = [np.array([-1, 2, 3, 4, 5]), np.array([5, 60, 2, 1, 0]), np.array([7, 8, 9, 8, 10]), np.array([3, 4, 5, 6, 1 << 30])]
    rows = []
    for p in range(4):                                           # three valid, one invalid at position p
        rows += [bad[p] if q == p else good.pop() for q in range(4)]
    for p in range(4):                                           # one valid at position p
        rows += [good.pop() if q == p else bad[(p + q) % 4] for q in range(4)]
    rows += bad                                                  # no valid tuple
    rows += [good.pop(), bad[0], good.pop()]                     # the last wave holds three teams
    tuples = np.ascontiguousarray(np.stack(rows), dtype=np.int32)
    res, hyp = _run(slam, sc, tuples)
    ref = _oracle_hyps(orc, sc, tuples, masks=True)
    _check_solve(hyp, ref, "mixed")
    n_valid = 0
    for it, (Es, _, Ms) in enumerate(ref):
        if _valid(tuples[it], 60):
            n_valid += 1
            assert len(Es) >= 1 and np.array_equal(hyp["counts"][it, :len(Es)], Ms.sum(1))
        else:
            assert hyp["ne"][it] == 0 and not hyp["counts"][it].any()
    assert n_valid == 12 + 4 + 2
    _check_winner(orc, sc, tuples, res)


def test_degenerate_tuples_next_to_valid_ones(slam, orc, syn):
    """Tuples on which the solver gives up at different stages -- zero motion, a repeated correspondence, an all-zero tuple, collinear points, NaN and
    infinite coordinates, coordinates of 1e200 and 1e120 -- each in a wave with valid tuples, in every team position: the failure paths of the
    elimination, of the root search and of the polish's gate change nothing for the neighbours, and give what the oracle gives."""
    sc = syn.five_point_scene(n=60, seed=12, noise_px=0.3, iters=40)
    pd1, pd2 = sc["pd1"], sc["pd2"]
    pd2[:10] = pd1[:10]
    pd1[11] = pd1[10]; pd2[11] = pd2[10]
    pd1[12] = [1e200, -1e200]; pd2[13] = [1e120, 3.0]; pd1[14] = [np.nan, 0.1]; pd1[15] = [np.inf, 0.1]
    pd1[16:21] = 0.0; pd2[16:21] = 0.0
    pd1[21:26, 1] = 0.0; pd2[21:26, 1] = 0.0
    odd = [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [0, 1, 2, 30, 31], [10, 11, 32, 33, 34], [12, 35, 36, 37, 38], [13, 35, 36, 37, 38], [14, 35, 36, 37, 38],
           [15, 35, 36, 37, 38], [16, 17, 18, 19, 20], [21, 22, 23, 24, 25], [12, 13, 14, 15, 16]]
    rng = np.random.default_rng(5)
    good = [26 + rng.permutation(34)[:5] for _ in range(8)]       # the untouched points
    rows = []
    for k, t in enumerate(odd):                                  # one odd tuple per wave, its position cycling; then waves of odd ones with one valid tuple
        w = [good[(k + q) % len(good)] for q in range(4)]
        w[k % 4] = np.array(t)
        rows += w
    for k in range(0, 9, 3):
        w = [np.array(t) for t in odd[k:k + 3]]
        w.insert(k % 4, good[k % len(good)])
        rows += w
    tuples = np.ascontiguousarray(np.stack(rows), dtype=np.int32)
    ref = _oracle_hyps(orc, sc, tuples, masks=True)
    assert sum(len(r[0]) == 0 for r in ref) >= 8 + 6              # the oracle gives up on eight of the eleven
    for rot in range(4):
        order = np.roll(np.arange(len(tuples)), rot)
        res, hyp = _run(slam, sc, tuples[order])
        _check_solve(hyp, [ref[i] for i in order], ("degenerate", rot))
        for it, i in enumerate(order):
            assert np.array_equal(hyp["counts"][it, :len(ref[i][0])], ref[i][2].sum(1)) and not hyp["counts"][it, len(ref[i][0]):].any()
        _check_winner(orc, sc, tuples[order], res)


def test_batch_streams_equal_their_single_calls(slam, orc, syn):
    """S = 3 with n = 60, 5, 200 and per-stream sample lists: every stream's hypotheses are those of its own single call"""
    iters = 23
    scs = [syn.five_point_scene(n=n, seed=20 + n, noise_px=0.3, outlier_frac=0.0 if n == 5 else 0.2, iters=iters) for n in (60, 5, 200)]
    for sc in scs:
        assert len(sc["samples"]) == iters
    args = [[sc[k] for sc in scs] for k in ("px1", "px2", "pd1", "pd2")]
    res, hyp = slam.pose.five_point_hypotheses(*args, [sc["K"] for sc in scs], [sc["K"] for sc in scs], THR, [sc["samples"] for sc in scs])
    for z, sc in enumerate(scs):
        r1, h1 = _run(slam, sc, sc["samples"])
        for k in ("ne", "Es", "poses"):
            assert np.array_equal(hyp[k][z].view(np.uint8), h1[k].view(np.uint8)), (z, k)        # bytes: the unwritten slots too
        if len(sc["px1"]) <= 64:
            assert np.array_equal(hyp["counts"][z], h1["counts"])
        assert hyp["best"][z] == h1["best"] == res[z][0]
        assert res[z][0] == r1[0] and res[z][1][4] == r1[1][4] and res[z][1][3] == r1[1][3]
        for a, b in zip(res[z][1][:3], r1[1][:3]):
            assert np.array_equal(a, b)
        _check_solve({k: v[z] for k, v in hyp.items()}, _oracle_hyps(orc, sc, sc["samples"]), ("batch", z))
        _check_winner(orc, sc, sc["samples"], res[z])
    assert res[0][0] >= 5 and res[2][0] >= 5


@pytest.mark.parametrize("n", [65, 128, 129, 256, 257, 320])
def test_scores_and_the_early_drop(slam, orc, syn, n):
    """k_5pt_score drops a pose once it cannot reach the incumbent any more ("only the counts of losers are partial").  For every hypothesis:
    the count is the oracle's full count, or it is the oracle's count over the first c correspondences, c a multiple of 64, and that prefix
    plus the n - c correspondences still to come is strictly below the final winner's count."""
    sc = syn.five_point_scene(n=n, seed=300 + n, noise_px=0.4, outlier_frac=0.25, iters=24)
    res, hyp = _run(slam, sc, sc["samples"])
    ref = _oracle_hyps(orc, sc, sc["samples"], masks=True)
    _check_solve(hyp, ref, n)
    win = _check_winner(orc, sc, sc["samples"], res)[0]
    assert hyp["best"] == win and win >= 0.5 * n
    full = partial = 0
    for it, (Es, _, Ms) in enumerate(ref):
        assert not hyp["counts"][it, len(Es):].any()
        for e in range(len(Es)):
            cnt = int(hyp["counts"][it, e])
            if cnt == int(Ms[e].sum()):
                full += 1
                continue
            cuts = [c for c in range(64, n, 64) if cnt == int(Ms[e, :c].sum()) and cnt + (n - c) < win]
            assert cuts, (n, it, e, cnt, int(Ms[e].sum()), win)
            partial += 1
    print(f"n = {n}: {full} full counts, {partial} dropped early, winner {win}")
    single = slam.five_point_ransac(sc["px1"], sc["px2"], sc["pd1"], sc["pd2"], sc["K"], sc["K"], max_repr_error=THR, samples=sc["samples"],
                                    return_extra=True)
    assert single[0] == res[0] and single[1][3] == res[1][3] and single[1][4] == res[1][4]
    for a, b in zip(single[1][:3], res[1][:3]):
        assert np.array_equal(a, b)


def test_ties_go_to_the_earliest_tuple(slam, orc, syn):
    """the winning tuple again later in the list; a noise-free scene (n = 130: three chunks) where many tuples score n"""
    sc = syn.five_point_scene(n=60, seed=31, noise_px=0.3, iters=20)
    first = orc.five_point_ransac(sc["px1"], sc["px2"], sc["pd1"], sc["pd2"], sc["K"], sc["K"], THR, sc["samples"])
    bi = first[5]
    assert 0 <= bi < 19
    tuples = np.concatenate([sc["samples"], sc["samples"][bi:bi + 1], sc["samples"][bi:bi + 1]]).astype(np.int32)
    res, hyp = _run(slam, sc, tuples)
    assert res[1][4] == bi and res[0] == first[0]
    assert np.array_equal(hyp["counts"][bi], hyp["counts"][20]) and hyp["counts"][20].max() == first[0]       # n <= 64: full counts, a real tie
    _check_winner(orc, sc, tuples, res)
    sc = syn.five_point_scene(n=130, seed=32, noise_px=0.0, outlier_frac=0.0, iters=24)
    res, hyp = _run(slam, sc, sc["samples"])
    ref = _oracle_hyps(orc, sc, sc["samples"], masks=True)
    winners = [it for it, (Es, _, Ms) in enumerate(ref) if len(Es) and Ms.sum(1).max() == 130]
    assert len(winners) >= 10 and res[0] == 130                  # a perfect scene: (nearly) every tuple holds the true motion
    assert res[1][4] == winners[0]
    _check_winner(orc, sc, sc["samples"], res)
