"""CPU: the lens scenes of tests/kfmap_lens_scripts.py and the model of a key-frame map that keeps raw pixels (slam_kfmap_enable_pixels) -- what
tests/test_gpu_kfmap_lens.py compares the device with.  Camera fx = fy = 60, (cx, cy) = (52, 35), a 70 x 105 image, dist = (-0.28, 0.07, 2e-4, 2e-5);
the sequence of tests/kfmap_lmm_scripts.py (8 key-frames, stream 1 not selected at the last, a local-BA update behind key-frames 3 and 4).

What the scenes hold, without merges (the figures the tests below assert or print):
  the model (raw pixels, lens camera in the match)   41, 30, 11 pairs on the three streams; smallest decision margin 4.6e-4; the lens moves a pixel
                                                     by up to 9.1 px in a coordinate, max_projection_distance is 2
  mutant A (raw pixels, pinhole camera)              35, 23, 9 pairs
  mutant B (pinhole pixels, lens camera)             36, 22, 9 pairs
  mutant U (undistorted pixels, lens camera)         37, 26, 10 pairs -- a stager that reads kupx where it should read kpx
With the merges applied the model still pairs on every stream (27, 19, 11; history 31, 21, 11; rows with D = 2: 23, 15, 9), margins as above.

With dist all zero the model is the model without the store, bit for bit, merges included."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfmap_lens_scripts as lz  # noqa: E402
import kfmap_lmm_scripts as ls  # noqa: E402
import kfmap_merge_scripts as ms  # noqa: E402
import np_kfmap as npk  # noqa: E402
import np_kfmap_merge as nm  # noqa: E402

S = ls.S
MARGIN = 1e-9                            # the project's rule: no decision of a parity scene closer than this to its threshold
MUTANTS = {"A": dict(lens=False), "B": dict(view="pinhole"), "U": dict(view="upx")}


def collect(run, merges=False, **kw):
    """-> per key-frame the match results of the sequence, the pair counts per stream, the smallest margin"""
    steps = []
    lz.run_sequence(run, merges=merges, on_step=lambda kind, k, data: steps.append(data) if kind == "match" else None, **kw)
    counts = [sum(len(r["pairs"]) for r in (st[s] for st in steps)) for s in range(S)]
    return steps, counts, min(r["margin"] for st in steps for r in st)


@pytest.fixture(scope="module")
def model():
    return collect(lz.LensRun())


def test_the_model_pairs_on_every_stream_with_margin(model):
    steps, counts, margin = model
    print(f"pairs per stream {counts}, smallest margin {margin:.3g}")
    assert min(counts) >= 5
    assert all(r["margin"] >= MARGIN for st in steps for r in st)


def test_the_lens_moves_pixels_further_than_the_projection_gate():
    frames, _ = ls.scenes()
    move = max(float(np.abs(lz.lens_pixel(lz.DIST, f["yx"]) - f["yx"]).max()) for fr in frames for f in fr if len(f["yx"]))
    print(f"largest raw-vs-pinhole displacement {move:.3g} px")
    assert move > ls.PARAMS.max_projection_distance
    raw = [lz.lens_pixel(lz.DIST, f["yx"]) for fr in frames for f in fr if len(f["yx"])]      # the raw pixels stay in the image: every keypoint has a cell
    assert all(np.all(p >= 1.0) and np.all(p[:, 0] <= ls.H) and np.all(p[:, 1] <= ls.W) for p in raw)


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_a_mutant_differs_from_the_model(model, name):
    steps, counts, _ = model
    msteps, mcounts, _ = collect(lz.LensRun(), **MUTANTS[name])
    print(f"mutant {name}: pairs per stream {mcounts} (the model: {counts})")
    differ = [s for s in range(S) if any(not np.array_equal(a[s]["pairs"], b[s]["pairs"]) for a, b in zip(steps, msteps))]
    assert differ == list(range(S))                              # on every stream


def test_upx_is_the_undistorted_raw_pixel_wherever_a_merge_moves_it():
    """the two arrays stay index-aligned through renames, re-ordering and dropped tombstones: upx == undistort(raw) record for record after every step"""
    run = lz.LensRun(mode="follow")
    seen = dict(merged=0, moved=0)

    def on_step(kind, k, data):
        for s, m in enumerate(run.m):
            for b in range(m.R):
                n = int(m.n[b])
                assert np.array_equal(m.upx[b, :n], npk.undistort(lz.CAM4, lz.DIST, m.views["raw"][b, :n])), (kind, k, s, b)
        if kind == "merge":
            seen["merged"] += int(run.counts[:, 0].sum()); seen["moved"] += int(run.counts[:, 2].sum())
    lz.run_sequence(run, merges=True, on_step=on_step)
    print(f"pairs applied {seen['merged']}, observations renamed {seen['moved']}")
    assert seen["merged"] >= 10 and seen["moved"] >= seen["merged"]


@pytest.mark.parametrize("kind", ("history", "rows"))
def test_the_history_and_row_forms_pair_on_every_stream(kind):
    _, counts, margin = collect(lz.LensRun(kind=kind, mode="follow"), merges=True)
    print(f"{kind}: pairs per stream {counts}, smallest margin {margin:.3g}")
    assert min(counts) >= 5 and margin >= MARGIN


@pytest.mark.parametrize("mode", ms.MODES)
def test_zero_distortion_is_the_model_without_the_store(mode):
    a, b = lz.LensRun(dist=lz.ZERO, mode=mode), ms.MergeRun(mode)
    log = {"a": [], "b": []}

    def rec(run, key):
        def on_step(kind, k, data):
            if kind == "match":
                log[key].append([(r["status"], r["pairs"].tobytes(), r["dist"].tobytes(), r["lm_ids"].tobytes(), r["kp_ids"].tobytes(),
                                  r["proj_yx"].tobytes(), r["best_kp"].tobytes(), r["best_dist"].tobytes()) for r in data])
            log[key].append([nm.snapshot(m) for m in run.m])
            log[key].append(repr([None if lst is None else sorted((n, v.tobytes()) for n, v in lst.items()) for lst in run.lists]))
        return on_step
    lz.run_sequence(a, merges=True, on_step=rec(a, "a"))
    for k in range(ls.N_KF):                                     # the same sequence on the model as it was
        b.add(ls.LAST_MASK if k == ls.N_KF - 1 else None); rec(b, "b")("add", k, None)
        res = b.match(); rec(b, "b")("match", k, res)
        b.merge(lz.pairs_of(res)); rec(b, "b")("merge", k, None)
        if k in ls.BA_AT:
            b.ba(); rec(b, "b")("ba", k, None)
    assert log["a"] == log["b"] and len(log["a"]) > 3 * ls.N_KF
    for ma in a.m:                                               # and the raw pixels are the slabs' own
        for s in range(ma.R):
            n = int(ma.n[s])
            assert np.array_equal(ma.views["raw"][s, :n], ma.upx[s, :n])
