"""Wall time of the whole estimator step per key-frame at the throughput shape of scripts/probes/prof_kfmap.py (S = 128, about 1 000 keypoints per
370 x 1226 list, cap 1 400, R 32; 8 warm-up key-frames, then 25 repeats, median (min - max)), both routes in one session on one device:
  (a) the host route   slam_kfmap_add_keyframe + slam_kfmap_ba_gather + slam_local_ba_batch + slam_kfmap_ba_update(ks)
  (b) the device route slam_kfmap_add_keyframe + slam_kfmap_local_ba(ks)
Both at the C seams (ctypes, the gathered arrays handed on as they are: none of the Python wrappers' slicing and re-packing), each step ended by a
wait for the context's stream; the two routes run on maps of their own fed the same lists, alternating per key-frame so that clocks and caches drift
alike.  Also recorded: the profiling spans of the device route's kernels (plan, emit, probe, stage, results, update) and of the host route's, the
solve's own device time (stats[6]), how many windows took the in-call host route, and the sizes of the device route's two small copies.

    python scripts/probes/prof_kfmap_local_ba.py [--streams 128] [--repeats 25] [--out profiles/kfmap_local_ba_s128.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from prof_kfmap import CAP, H, MCAP, NKP, RING, WARM, W, Stream, stat  # noqa: E402

MINC = 25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import slam_jl_amd as slam
    from slam_jl_amd import _lib as L, synthetic as syn
    from slam_jl_amd.keyframe_map import _Windows
    S, R = args.streams, args.repeats
    ctx = slam.default_context(0)
    lib = ctx.lib
    cam = syn.KITTI_CAM
    cams = np.ascontiguousarray(np.tile(np.asarray(cam, dtype=np.float64), (S, 1)))
    minc = np.full(S, MINC, dtype=np.int32)
    streams = [Stream(np.random.default_rng(100 + s), cam) for s in range(S)]
    side = {r: (slam.KeypointSet(S, CAP), slam.KeyframeMap(S, CAP, R=RING, mcap=MCAP)) for r in ("host", "dev")}
    # the host route's arrays, made once (what S windows can at most need, as KeyframeMap.gather sizes them)
    nW, nP = S, S * RING
    nM = S * min(MCAP, 5 * CAP); nO = min(nM * RING, 4_000_000)
    i32 = lambda n: np.zeros(max(n, 1), dtype=np.int32)
    i64 = lambda n: np.zeros(max(n, 1), dtype=np.int64)
    gst, ws, Pn, Mn, On = i32(S), i32(nW), i32(nW), i32(nW), i32(nW)
    theta, tc, px = np.zeros(6 * nP + 3 * nM), np.zeros(nP, dtype=np.uint8), np.zeros(2 * nO)
    pi, li, pr, lr, okf, okp, oc = i64(nO), i64(nO), i64(nP), i64(nM), i64(nO), i64(nO), np.zeros(nO, dtype=np.uint8)
    outl = np.zeros(nO, dtype=np.uint8); hstats = np.zeros((S, 8)); hstatus = i32(S)
    out = _Windows(nW, nP, nM, nO, L.ptr(gst, L.i32p), L.ptr(ws, L.i32p), L.ptr(Pn, L.i32p), L.ptr(Mn, L.i32p), L.ptr(On, L.i32p), L.ptr(theta), L.ptr(tc, L.u8p), L.ptr(px),
                   L.ptr(pi, L.i64p), L.ptr(li, L.i64p), L.ptr(pr, L.i64p), L.ptr(lr, L.i64p), L.ptr(okf, L.i64p), L.ptr(okp, L.i64p), L.ptr(oc, L.u8p))
    dstatus = i32(S); dstats = np.zeros((S, 8))
    spans_dev = ("kfmap_add", "kfmap_gather_plan", "kfmap_gather_emit", "ba_dev_probe", "ba_dev_stage", "ba_dev_results", "kfmap_update")
    spans_host = ("kfmap_add", "kfmap_gather_plan", "kfmap_gather_emit", "kfmap_update")
    m = {"host_wall": [], "dev_wall": [], "host_solve_dev": [], "dev_solve_dev": [], "windows": [], "dev_host_routed": [], "sizes": []}
    m.update({"dev_" + n: [] for n in spans_dev}); m.update({"host_" + n: [] for n in spans_host})
    ctx.prof_enable(True)
    for k in range(WARM + R):
        Tcw = np.tile(np.eye(4), (S, 1, 1))
        for s, st in enumerate(streams):
            Tcw[s], yx, f3, xyz, ids = st.keyframe(k)
            for ks, _ in side.values():
                ks.upload(s, yx, f3, xyz, ids)
        sp = np.ascontiguousarray(slam.stream_params(S, Tcw=Tcw, cam=cam), dtype=np.float64)
        for ks, _ in side.values():
            ks.keyframe()
        for route in (("host", "dev") if k % 2 == 0 else ("dev", "host")):
            ks, km = side[route]
            ctx.synchronize(); ctx.prof_reset()
            t0 = time.perf_counter()
            ctx.check(lib.slam_kfmap_add_keyframe(ctx.h, km.h, ks.h, L.ptr(sp)))
            if route == "host":
                n = C.c_int32(0)
                ctx.check(lib.slam_kfmap_ba_gather(ctx.h, km.h, L.ptr(minc, L.i32p), C.byref(out), C.byref(n)))
                nw = n.value
                if nw:
                    ctx.check(lib.slam_local_ba_batch(ctx.h, nw, L.ptr(cams), L.ptr(Pn, L.i32p), L.ptr(Mn, L.i32p), L.ptr(On, L.i32p), L.ptr(theta), L.ptr(tc, L.u8p), L.ptr(px),
                                                      L.ptr(pi, L.i64p), L.ptr(li, L.i64p), L.ptr(outl, L.u8p), 5, 10, 5.0, L.ptr(hstats), L.ptr(hstatus, L.i32p)))
                    ok = np.flatnonzero(hstatus[:nw] == 0)
                    assert len(ok) == nw, "a window failed on the host route: the update's arrays would need re-packing"
                    ctx.check(lib.slam_kfmap_ba_update(ctx.h, km.h, ks.h, nw, L.ptr(ws, L.i32p), L.ptr(theta), L.ptr(outl, L.u8p)))
            else:
                ctx.check(lib.slam_kfmap_local_ba(ctx.h, km.h, ks.h, L.ptr(minc, L.i32p), L.ptr(cams), 5, 10, 5.0, L.ptr(dstatus, L.i32p), L.ptr(dstats)))
            ctx.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            if k < WARM:
                continue
            if route == "host":
                m["host_wall"].append(wall); m["host_solve_dev"].append(float(hstats[0, 6])); m["windows"].append(nw)
                m["sizes"].append([float(Pn[:nw].mean()), float(Mn[:nw].mean()), float(On[:nw].mean())])
                for nme in spans_host:
                    m["host_" + nme].append(ctx.prof_get(nme)[0])
            else:
                m["dev_wall"].append(wall)
                solved = np.flatnonzero(dstatus == 0)
                assert len(solved), dstatus
                m["dev_solve_dev"].append(float(dstats[solved, 6].max()))
                m["dev_host_routed"].append(int(sum(1 for s in solved if dstats[s, 6] != dstats[solved, 6].max())))
                for nme in spans_dev:
                    m["dev_" + nme].append(ctx.prof_get(nme)[0])
    ctx.prof_enable(False)
    sz = np.mean(np.array(m["sizes"]), axis=0)
    a, b = stat(m["host_wall"]), stat(m["dev_wall"])
    nwin = int(np.median(m["windows"]))
    rec = {"lib": os.path.basename(slam.LIB_PATH), "S": S, "cap": CAP, "keypoints_per_stream": NKP, "shape": [H, W], "ring": RING, "table": MCAP, "repeats": R,
           "warmup_keyframes": WARM, "min_cov_score": MINC, "windows_per_step": nwin, "window_mean": {"poses": float(sz[0]), "points": float(sz[1]), "observations": float(sz[2])},
           "a_host_route_wall_ms": a, "b_device_route_wall_ms": b, "b_whole_range_below_a": bool(b["max"] < a["min"]),
           "a_solve_device_ms": stat(m["host_solve_dev"]), "b_solve_device_ms": stat(m["dev_solve_dev"]),
           "b_windows_through_the_in_call_host_route": stat(m["dev_host_routed"]),
           "b_kernel_ms": {n: stat(m["dev_" + n]) for n in spans_dev}, "a_kernel_ms": {n: stat(m["host_" + n]) for n in spans_host},
           "b_copy_bytes": {"probe_results_device_to_host": 16 * nwin, "lm_states_device_to_host": 256 * nwin, "plan_headers_device_to_host": 32 * S}}
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f_:
            f_.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
