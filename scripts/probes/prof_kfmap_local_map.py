"""slam_kfmap_local_map_match at the throughput shape against the only route there was before it -- download every stream's slabs and table, assemble
the local map, the observer lists and the descriptor sets in Python, slam_local_map_match_batch -- on the SAME map, in one session.

Shape: prof_kfmap.py's (S = 128 streams, 370 x 1226, lists of about 1 000 keypoints, cap 1 400, ring R = 32, table of 16 384 points, a rigid scene, a
fifth of a list replaced per key-frame), cell 35, max_local = 10 000, every new point with a random 256-bit descriptor (so hardly any pair: the cost of
staging and of the gates, not of merges).  Warm-up runs 8 key-frames; then per repeat one key-frame of all S streams:
  (a) device time of slam_kfmap_add_descriptors (span kfmap_add_descriptors);
  (b) slam_kfmap_local_map_match: device time of the whole call (span kfmap_local_map_match: upload, memset, staging, match, pairs, copy of results), of
      the staging kernel (kfmap_lm_stage) and of the match kernel (local_map_match_kernel), and the wall time of the synchronous call;
  (c) the host route on the same map, on the first --host-repeats of the steps (it takes seconds per step at S = 128): wall time of the downloads, of the
      Python assembly + packing, and of the slam_local_map_match_batch call; its pairs are compared with (b)'s.
Medians with the spread (min - max) over the repeats.

--history: a SECOND map with slam_kfmap_enable_local_map_history takes the same key-frames and descriptors, and per repeat both maps' match calls are
timed back to back (without history first): (b) for each, plus the local-map sizes each reaches and how many streams had status 2.  The host route (c)
is not run (it models the match without history).  --max-local sets the bound of both calls (16 384 = the table's size rules status 2 out).

--rows D: a SECOND map with slam_kfmap_enable_descriptor_rows(D) takes the same key-frames and descriptors; per repeat add_keyframe, add_descriptors and
the match of both maps are timed (rows off first).  With random descriptors no pair occurs: the figures are upkeep and staging, not merges.

--pixels: a SECOND map with slam_kfmap_enable_pixels takes the same key-frames and descriptors (a pinhole camera on both: what the store itself costs);
per repeat add_keyframe, add_descriptors and the match of both maps are timed, the plain map first, the two alternating through the session.

    python scripts/probes/prof_kfmap_local_map.py [--streams 128] [--repeats 25] [--host-repeats 25] [--out profiles/kfmap_local_map_s128.json]
    python scripts/probes/prof_kfmap_local_map.py --history [--max-local 16384] [--out profiles/kfmap_local_map_history_s128.json]
    python scripts/probes/prof_kfmap_local_map.py --rows 4 [--out profiles/kfmap_rows_s128.json]
    python scripts/probes/prof_kfmap_local_map.py --pixels [--out profiles/kfmap_lens_s128.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from prof_kfmap import CAP, H, MCAP, RING, W, WARM, NKP, Stream, stat  # noqa: E402

CELL, MAX_LOCAL, DCAP = 35, 10000, CAP


def tcw_of(theta):
    s1, c1, s2, c2, s3, c3 = np.sin(theta[0]), np.cos(theta[0]), np.sin(theta[1]), np.cos(theta[1]), np.sin(theta[2]), np.cos(theta[2])
    T = np.eye(4)
    T[:3, :3] = [[c1 * c2, c1 * s2 * s3 - s1 * c3, c1 * s2 * c3 + s1 * s3], [s1 * c2, s1 * s2 * s3 + c1 * c3, s1 * s2 * c3 - c1 * s3], [-s2, c2 * s3, c2 * c3]]
    T[:3, 3] = theta[3:6]
    return T


def download(km, s, cur):
    kfs = {k: d for k in range(max(cur - RING + 1, 0), cur + 1) for d in [km.download_keyframe(s, k)] if d is not None}
    return kfs, km.download_points(s)


def assemble(kfs, pts, cur, rows, cam10, params):
    """the host-array problem of one stream from its downloads (update_frame_covisibility! + the lists of do_local_map_matching) -> (problem, lm ids, keypoint ids)"""
    point = {int(i): j for j, i in enumerate(pts["ids"])}
    live = {k: {int(i): (float(p[0]), float(p[1])) for i, p, lv in zip(d["ids"], d["upx"], d["live"]) if lv} for k, d in kfs.items()}
    obs, is3 = pts["observers"], pts["is_3d"]
    cov = set()
    for i in live[cur]:
        if i in point:
            cov.update(o for o in obs[point[i]] if o != cur and o in kfs)
    lm = sorted({i for o in cov for i in live[o] if i in point and is3[point[i]] and i in rows and cur not in obs[point[i]]})
    order = sorted(kfs)
    row = {k: j for j, k in enumerate(order)}
    kp_ids = [i for i in live[cur] if i in point and i in rows]
    if not lm or not kp_ids:
        return None, lm, kp_ids
    keypoints = [{"pixel": live[cur][i], "descriptors": rows[i].reshape(1, 4), "observers": [(row[o], live[o][i]) for o in obs[point[i]] if o in kfs and i in live[o]]}
                 for i in kp_ids]
    local_map = [{"position": pts["xyz"][point[i]], "descriptors": rows[i].reshape(1, 4), "observers": [row[o] for o in obs[point[i]] if o in kfs]} for i in lm]
    frame = {"Tcw": tcw_of(kfs[cur]["theta"]), "cam": cam10, "cell_size": CELL, "nb_3d_kpts": sum(1 for i in live[cur] if i in point and is3[point[i]])}
    return (frame, keypoints, np.array([tcw_of(kfs[k]["theta"]) for k in order]), local_map, params), lm, kp_ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--host-repeats", type=int, default=25)
    ap.add_argument("--out", default=None)
    ap.add_argument("--history", action="store_true", help="time a second map with the local-map history beside the first, on the same steps (no host route)")
    ap.add_argument("--rows", type=int, default=0, metavar="D", help="time a second map with D descriptor rows per point beside the first, on the same steps (no host route)")
    ap.add_argument("--pixels", action="store_true", help="time a second map with the raw-pixel store beside the first, on the same steps (no host route)")
    ap.add_argument("--max-local", type=int, default=MAX_LOCAL)
    args = ap.parse_args()
    if bool(args.history) + bool(args.rows) + bool(args.pixels) > 1:
        ap.error("--history, --rows and --pixels each time ONE second map")
    if args.history or args.rows or args.pixels:
        args.host_repeats = 0
    import torch
    import slam_jl_amd as slam
    from slam_jl_amd import synthetic as syn
    S, R = args.streams, args.repeats
    ctx = slam.default_context(0)                                # no device: raises here, nothing is measured
    cam = syn.KITTI_CAM
    cam10 = tuple(cam) + (0.0, 0.0, 0.0, 0.0, float(H), float(W))
    params = slam.Params()
    rng = np.random.default_rng(7)
    streams = [Stream(np.random.default_rng(100 + s), cam) for s in range(S)]
    ks = slam.KeypointSet(S, CAP)
    km = slam.KeyframeMap(S, CAP, R=RING, mcap=MCAP)
    km.enable_descriptors()
    kmh = None
    if args.history:
        kmh = slam.KeyframeMap(S, CAP, R=RING, mcap=MCAP)
        kmh.enable_descriptors(); kmh.enable_local_map_history()
    if args.rows:
        kmh = slam.KeyframeMap(S, CAP, R=RING, mcap=MCAP)
        kmh.enable_descriptors(); kmh.enable_descriptor_rows(args.rows)
    if args.pixels:
        kmh = slam.KeyframeMap(S, CAP, R=RING, mcap=MCAP)
        kmh.enable_descriptors(); kmh.enable_pixels()
    rows = [dict() for _ in range(S)]
    m = {k: [] for k in ("desc", "call", "stage", "kernel", "wall", "h_down", "h_asm", "h_call", "h_total", "M", "N", "pairs",
                         "hist_call", "hist_stage", "hist_kernel", "hist_wall", "hist_M", "hist_pairs", "hist_status2", "status2", "add", "hist_add", "hist_desc")}
    agree, pairs_equal = [], []
    ctx.prof_enable(True)
    for k in range(WARM + R):
        Tcw = np.tile(np.eye(4), (S, 1, 1))
        desc = np.zeros((S, DCAP, 4), dtype=np.uint64); info = np.zeros((S, 2), dtype=np.int64)
        for s, st in enumerate(streams):
            first = st.next
            Tcw[s], yx, f3, xyz, ids = st.keyframe(k)
            ks.upload(s, yx, f3, xyz, ids)
            n_new = st.next - first
            assert n_new <= DCAP
            new = rng.integers(0, 2 ** 64, (n_new, 4), dtype=np.uint64)
            desc[s, :n_new] = new; info[s] = (first, n_new)
            rows[s].update({first + j: new[j] for j in range(n_new)})
        desc_dev = torch.from_numpy(desc.view(np.int64)).cuda(); info_dev = torch.from_numpy(info).cuda()
        torch.cuda.synchronize()
        ks.keyframe()
        ctx.synchronize()
        ctx.prof_reset()
        km.add_keyframe(ks, slam.stream_params(S, Tcw=Tcw, cam=cam))
        ctx.synchronize()
        if k >= WARM:
            m["add"].append(ctx.prof_get("kfmap_add")[0])
        if kmh is not None:
            ctx.prof_reset()
            kmh.add_keyframe(ks, slam.stream_params(S, Tcw=Tcw, cam=cam))
            kmh.add_descriptors(desc_dev.data_ptr(), info_dev.data_ptr(), DCAP)
            ctx.synchronize()
            if k >= WARM:
                m["hist_add"].append(ctx.prof_get("kfmap_add")[0]); m["hist_desc"].append(ctx.prof_get("kfmap_add_descriptors")[0])
        ctx.synchronize()
        ctx.prof_reset()
        km.add_descriptors(desc_dev.data_ptr(), info_dev.data_ptr(), DCAP)
        ctx.synchronize()
        t0 = time.perf_counter()
        status, pairs, dist = km.local_map_match(cam10, CELL, params.max_projection_distance, params.max_descriptor_distance, max_local=args.max_local)
        wall = (time.perf_counter() - t0) * 1e3
        assert args.history or args.rows or not (status == 2).any(), "a local map did not fit the probe's max_local"
        if k >= WARM:
            m["status2"].append(int((status == 2).sum()))
            m["desc"].append(ctx.prof_get("kfmap_add_descriptors")[0]); m["call"].append(ctx.prof_get("kfmap_local_map_match")[0])
            m["stage"].append(ctx.prof_get("kfmap_lm_stage")[0]); m["kernel"].append(ctx.prof_get("local_map_match_kernel")[0]); m["wall"].append(wall)
            dbg = [km.debug_local_map(s) for s in range(0, S, max(S // 8, 1))]
            m["M"].append(float(np.mean([len(d["lm_ids"]) for d in dbg]))); m["N"].append(float(np.mean([len(d["kp_ids"]) for d in dbg])))
            m["pairs"].append(int(sum(len(p) for p in pairs)))
        if kmh is not None:                                      # the same step on the map with history, right behind
            ctx.prof_reset()
            t0 = time.perf_counter()
            hstatus, hpairs, _ = kmh.local_map_match(cam10, CELL, params.max_projection_distance, params.max_descriptor_distance, max_local=args.max_local)
            hwall = (time.perf_counter() - t0) * 1e3
            if k >= WARM:
                m["hist_call"].append(ctx.prof_get("kfmap_local_map_match")[0]); m["hist_stage"].append(ctx.prof_get("kfmap_lm_stage")[0])
                m["hist_kernel"].append(ctx.prof_get("local_map_match_kernel")[0]); m["hist_wall"].append(hwall)
                dbg = [kmh.debug_local_map(s) for s in range(0, S, max(S // 8, 1))]
                m["hist_M"].append(float(np.mean([len(d["lm_ids"]) for d in dbg])))
                m["hist_pairs"].append(int(sum(len(p) for p in hpairs))); m["hist_status2"].append(int((hstatus == 2).sum()))
                if args.pixels:
                    pairs_equal.append(bool(np.array_equal(status, hstatus) and all(np.array_equal(a_, b_) for a_, b_ in zip(pairs, hpairs))))
        if k >= WARM and k - WARM < args.host_repeats:
            cur = km.newest()
            t0 = time.perf_counter()
            down = [download(km, s, int(cur[s])) for s in range(S)]
            t1 = time.perf_counter()
            made = [assemble(down[s][0], down[s][1], int(cur[s]), rows[s], cam10, params) for s in range(S)]
            live = [s for s in range(S) if made[s][0] is not None]
            from slam_jl_amd import _lib as L, local_map as lmod
            import ctypes as C
            packs = [lmod.pack_local_map(*made[s][0]) for s in live]
            p, kp_off, kf_off, mp_off = lmod.concat_packs(packs)
            a, out = lmod._args(p)
            t2 = time.perf_counter()
            ctx.check(ctx.lib.slam_local_map_match_batch(ctx.h, len(live), L.ptr(kp_off, L.i32p), L.ptr(kf_off, L.i32p), L.ptr(mp_off, L.i32p), C.byref(a)))
            t3 = time.perf_counter()
            m["h_down"].append((t1 - t0) * 1e3); m["h_asm"].append((t2 - t1) * 1e3); m["h_call"].append((t3 - t2) * 1e3); m["h_total"].append((t3 - t0) * 1e3)
            same = [status[s] == 0 for s in live] == [True] * len(live)
            for z, s in enumerate(live):
                mt = out["match"][kp_off[z]:kp_off[z + 1]]
                took = np.flatnonzero(mt >= 0)
                want = np.array([(made[s][2][j], made[s][1][mt[j]]) for j in took], dtype=np.int64).reshape(-1, 2)
                same = same and np.array_equal(want, pairs[s])
            agree.append(bool(same))
        del desc_dev, info_dev
    ctx.prof_enable(False)
    if kmh is not None:
        if args.history:
            newest = int(kmh.newest()[0])
            stored = [len(kmh.local_map_ids(s, newest)) for s in range(0, S, max(S // 8, 1))]
        elif args.rows:                                          # the rows the second map holds: per sampled stream the rows per live point, and what the bound dropped
            got = [kmh.descriptor_rows(s) for s in range(0, S, max(S // 8, 1))]
            rows_per_point = [float(np.mean([len(k_) for k_ in g["keys"]])) if len(g["keys"]) else 0.0 for g in got]
            rows_dropped = [g["dropped"] for g in got]
        kmh.close()
    km.close(); ks.close()
    rec = {"lib": os.path.basename(slam.LIB_PATH), "S": S, "cap": CAP, "keypoints_per_stream": NKP, "shape": [H, W], "cell": CELL, "ring": RING, "table": MCAP,
           "max_local": args.max_local, "repeats": R, "host_repeats": len(m["h_total"]), "warmup_keyframes": WARM,
           "local_map_points_per_stream": stat(m["M"]), "keypoints_with_descriptor_per_stream": stat(m["N"]), "pairs_all_streams": stat(m["pairs"]),
           "a_add_keyframe_device_ms": stat(m["add"]), "a_add_descriptors_device_ms": stat(m["desc"]),
           "b_local_map_match_device_ms": stat(m["call"]), "b_stage_kernel_ms": stat(m["stage"]), "b_match_kernel_ms": stat(m["kernel"]),
           "b_local_map_match_sync_wall_ms": stat(m["wall"]),
           "c_host_route_wall_ms": stat(m["h_total"]), "c_host_downloads_wall_ms": stat(m["h_down"]), "c_host_assembly_and_packing_wall_ms": stat(m["h_asm"]),
           "c_host_batch_call_wall_ms": stat(m["h_call"]), "c_host_route_pairs_equal_device": agree}
    if args.history:
        rec = {k: v for k, v in rec.items() if not k.startswith("c_")}
        rec.update({"streams_with_status_2": stat(m["status2"]),
                    "history_local_map_points_per_stream": stat(m["hist_M"]), "history_stored_set_of_newest_keyframe": stat(stored),
                    "history_pairs_all_streams": stat(m["hist_pairs"]), "history_streams_with_status_2": stat(m["hist_status2"]),
                    "history_local_map_match_device_ms": stat(m["hist_call"]), "history_stage_kernel_ms": stat(m["hist_stage"]),
                    "history_match_kernel_ms": stat(m["hist_kernel"]), "history_local_map_match_sync_wall_ms": stat(m["hist_wall"])})
    if args.rows:                                                # with random descriptors no pair occurs: upkeep and staging, not merges
        rec = {k: v for k, v in rec.items() if not k.startswith("c_")}
        rec.update({"rows_per_point_D": args.rows, "rows_per_live_point": stat(rows_per_point), "rows_dropped_by_the_bound": stat(rows_dropped),
                    "rows_pairs_all_streams": stat(m["hist_pairs"]), "rows_streams_with_status_2": stat(m["hist_status2"]),
                    "rows_add_keyframe_device_ms": stat(m["hist_add"]), "rows_add_descriptors_device_ms": stat(m["hist_desc"]),
                    "rows_local_map_match_device_ms": stat(m["hist_call"]), "rows_stage_kernel_ms": stat(m["hist_stage"]),
                    "rows_match_kernel_ms": stat(m["hist_kernel"]), "rows_local_map_match_sync_wall_ms": stat(m["hist_wall"]),
                    "note": "both maps take the same key-frames in one session; random descriptors pair nothing, so the figures are upkeep (add_keyframe's forgetting and "
                            "recording, add_descriptors) and staging, not merges; slam_kfmap_merge and slam_kfmap_filter are not timed here"})
    if args.pixels:                                              # the same answers from both maps: the store changes where the match reads, not what
        rec = {k: v for k, v in rec.items() if not k.startswith("c_")}
        rec.update({"pixels_store_bytes_per_stream": 16 * RING * CAP, "pixels_pairs_equal_plain": pairs_equal,
                    "pixels_pairs_all_streams": stat(m["hist_pairs"]), "pixels_streams_with_status_2": stat(m["hist_status2"]),
                    "pixels_add_keyframe_device_ms": stat(m["hist_add"]), "pixels_add_descriptors_device_ms": stat(m["hist_desc"]),
                    "pixels_local_map_match_device_ms": stat(m["hist_call"]), "pixels_stage_kernel_ms": stat(m["hist_stage"]),
                    "pixels_match_kernel_ms": stat(m["hist_kernel"]), "pixels_local_map_match_sync_wall_ms": stat(m["hist_wall"]),
                    "note": "both maps take the same key-frames in one session, the plain map first in every repeat; a pinhole camera on both, so the figures are "
                            "what the store costs (16 more bytes written per recorded observation, the stager reading kpx for kupx); slam_kfmap_merge is not timed here"})
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f_:
            f_.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
