#!/usr/bin/env python3
"""Regenerates tests/golden/tracked_ba_v1.npz: local-BA windows gathered from tracked key-frames (tests/tracked_ba.py) of the stereo
kitti05_1000 and the monocular euroc_mono workloads, their theta0 and the oracle's solutions.  The tracked run needs a GPU (the
front end's keypoint lists); the windows are then solved and chained by the CPU oracle alone (an oracle-only record).

    python tests/golden/make_golden_tracked_ba.py

Per workload it keeps one window: the smallest of those that show the most of the structure the tests are after."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import slam_jl_amd as slam  # noqa: E402
from slam_jl_amd import synthetic as syn  # noqa: E402
from oracle import oracle as orc  # noqa: E402
import tracked_ba as tb  # noqa: E402

OUT = os.path.join(HERE, "tracked_ba_v1.npz")


def windows(name, periods=6):
    """every window of the oracle-only chain of the four records of tracked_ba.STREAM_CFG"""
    rec, got = [], []

    def on_kf(kfid, Tcw, lists, camt):
        if not rec:
            rec.extend(tb.Record(camt, min_cov_score=c, mismatch=f) for c, f in tb.STREAM_CFG)
        for s, r in enumerate(rec):
            tb.add_keyframe(r, kfid, Tcw[s], lists[s])
            w = tb.gather(r)
            if w is None or len(w["poses_ids"]) == 0:
                continue
            th, ol, st = orc.bundle_adjustment(camt, w["theta"], w["theta_const"], w["pixels"], w["poses_ids"], w["points_ids"], 5, 10, 5.0, solver=1)
            got.append((f"{kfid} stream {s}", np.asarray(camt, dtype=np.float64), w, th, ol, st))
            tb.update(r, w, th, ol)

    slam.default_context(0)
    tb.run_tracked(slam, syn, name, len(tb.STREAM_CFG), periods, on_kf)
    return got


def pack(sel):
    out = {}
    for n, (tag, (kfid, cam, w, th, ol, st)) in enumerate(sel):
        p = f"w{n}_"
        out.update({p + "tag": np.array(f"{tag} kf {kfid}"), p + "cam": cam, p + "theta0": w["theta"], p + "theta_const": w["theta_const"],
                    p + "pixels": w["pixels"], p + "poses_ids": w["poses_ids"].astype(np.int32), p + "points_ids": w["points_ids"].astype(np.int32),
                    p + "theta": th, p + "outliers": ol.astype(np.uint8),
                    p + "stats": np.array([st["ssr_final"], st["ssr_init"], st["ssr_pass1"], st["iters_pass1"], st["iters_pass2"]])})
    out["n"] = np.array(len(sel))
    np.savez_compressed(OUT, **out)
    return os.path.getsize(OUT)


def main():
    sel = []
    for tag, name in (("stereo", "kitti05_1000"), ("mono", "euroc_mono")):
        got = windows(name)
        # the smallest of the windows that show most of: a single-observation point of a free pose, a point seen by constant poses only,
        # a constant pose other than key-frame 0, a flagged outlier
        cover = lambda g: sum(int(v > 0) for v in (tb.structure(g[2])["single_free"], tb.structure(g[2])["const_only"],
                                                   tb.structure(g[2])["const_not0"], int(g[4].sum())))
        best = max(cover(g) for g in got)
        g = min((g for g in got if cover(g) == best), key=lambda g: len(g[2]["poses_ids"]))
        print(tag, g[0], tb.structure(g[2]), "outliers", int(g[4].sum()))
        sel.append((tag, g))
    size = pack(sel)
    print(OUT, [t + " kf " + g[0] for t, g in sel], size, "bytes")
    assert size <= 512 * 1024, size


if __name__ == "__main__":
    main()
