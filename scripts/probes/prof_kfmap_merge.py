"""slam_kfmap_merge at the throughput shape, beside the slam_kfmap_local_map_match of the same step.  There is no earlier route to compare with: the map
has downloads and no upload, so before this call the pairs of a match could not be applied at all.  No ratio is stated.

Shape: prof_kfmap_local_map.py's (S = 128 streams, 370 x 1226, lists of about 1 000 keypoints, cap 1 400, ring R = 32, table of 16 384 points, cell 35,
max_local = 10 000, random 256-bit descriptors).  Random descriptors yield no pairs, so the probe builds host pairs from what the match staged
(debug_local_map): per stream k keypoints of the newest key-frame, spread evenly over its list, paired with k local-map ids spread evenly over the local
map -- valid, one-to-one pairs whose renames move records across the whole slab.  Warm-up runs 8 key-frames; then per repeat one key-frame of all S
streams -- add_keyframe, add_descriptors, local_map_match, merge(ks) -- cycling through k = 10 and k = 100 and through the two forms of the call:
  enqueue-only   want_counts=False: wall time of the call itself (it returns with the kernels enqueued), then a synchronise outside the measurement;
  synchronous    want_counts=True: wall time including the copy of the counts and the wait.
Per step: device time of the whole call (span kfmap_merge) and of each kernel (kfmap_merge_resolve, kfmap_merge_slabs, kfmap_merge_list), the renames
it made, and the device and wall time of the local_map_match before it.  Medians with the spread (min - max) over the repeats of each (k, form).

    python scripts/probes/prof_kfmap_merge.py [--streams 128] [--repeats 24] [--out profiles/kfmap_merge_s128.json]
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
KS = (10, 100)


def spread(a, k):
    """k entries of a, evenly spread, in order"""
    return a[np.linspace(0, len(a) - 1, k).astype(np.int64)] if k > 0 else a[:0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=24)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
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
    keys = ("call", "resolve", "slabs", "list", "wall", "pairs", "applied", "renamed", "lmm_call", "lmm_wall")
    m = {(k, form): {key: [] for key in keys} for k in KS for form in ("enqueue", "sync")}
    ctx.prof_enable(True)
    for step in range(WARM + R):
        Tcw = np.tile(np.eye(4), (S, 1, 1))
        desc = np.zeros((S, DCAP, 4), dtype=np.uint64); info = np.zeros((S, 2), dtype=np.int64)
        for s, st in enumerate(streams):
            first = st.next
            Tcw[s], yx, f3, xyz, ids = st.keyframe(step)
            ks.upload(s, yx, f3, xyz, ids)
            n_new = st.next - first
            assert n_new <= DCAP
            desc[s, :n_new] = rng.integers(0, 2 ** 64, (n_new, 4), dtype=np.uint64); info[s] = (first, n_new)
        desc_dev = torch.from_numpy(desc.view(np.int64)).cuda(); info_dev = torch.from_numpy(info).cuda()
        torch.cuda.synchronize()
        ks.keyframe()
        km.add_keyframe(ks, slam.stream_params(S, Tcw=Tcw, cam=cam))
        km.add_descriptors(desc_dev.data_ptr(), info_dev.data_ptr(), DCAP)
        ctx.synchronize()
        ctx.prof_reset()
        t0 = time.perf_counter()
        status, _, _ = km.local_map_match(cam10, CELL, params.max_projection_distance, params.max_descriptor_distance, max_local=MAX_LOCAL)
        lmm_wall = (time.perf_counter() - t0) * 1e3
        assert not (status == 2).any(), "a local map did not fit the probe's max_local"
        lmm_call = ctx.prof_get("kfmap_local_map_match")[0]
        del desc_dev, info_dev
        if step < WARM:
            continue
        k, form = KS[((step - WARM) // 2) % len(KS)], ("enqueue", "sync")[(step - WARM) % 2]
        pairs = []
        for s in range(S):
            d = km.debug_local_map(s)
            n = min(k, len(d["kp_ids"]), len(d["lm_ids"]))
            pairs.append(np.stack([spread(d["kp_ids"], n), spread(d["lm_ids"], n)], axis=1))
        ctx.synchronize()
        ctx.prof_reset()
        t0 = time.perf_counter()
        counts = km.merge(ks, pairs, want_counts=form == "sync")
        wall = (time.perf_counter() - t0) * 1e3
        ctx.synchronize()
        rec = m[(k, form)]
        rec["call"].append(ctx.prof_get("kfmap_merge")[0]); rec["resolve"].append(ctx.prof_get("kfmap_merge_resolve")[0])
        rec["slabs"].append(ctx.prof_get("kfmap_merge_slabs")[0]); rec["list"].append(ctx.prof_get("kfmap_merge_list")[0])
        rec["wall"].append(wall); rec["pairs"].append(int(sum(len(p) for p in pairs))); rec["lmm_call"].append(lmm_call); rec["lmm_wall"].append(lmm_wall)
        if counts is not None:
            assert not counts[:, 3].any()
            rec["applied"].append(int(counts[:, 0].sum())); rec["renamed"].append(int(counts[:, 2].sum()))
    ctx.prof_enable(False)
    km.close(); ks.close()
    out = {"lib": os.path.basename(slam.LIB_PATH), "S": S, "cap": CAP, "keypoints_per_stream": NKP, "shape": [H, W], "cell": CELL, "ring": RING, "table": MCAP,
           "max_local": MAX_LOCAL, "repeats": R, "warmup_keyframes": WARM, "cases": []}
    for (k, form), rec in m.items():
        out["cases"].append({"pairs_per_stream": k, "form": form, "steps": len(rec["wall"]), "pairs_all_streams": stat(rec["pairs"]),
                             "pairs_applied_all_streams": stat(rec["applied"]), "observations_renamed_all_streams": stat(rec["renamed"]),
                             "merge_device_ms": stat(rec["call"]), "resolve_kernel_ms": stat(rec["resolve"]), "slabs_kernel_ms": stat(rec["slabs"]),
                             "list_kernel_ms": stat(rec["list"]), "merge_call_wall_ms": stat(rec["wall"]),
                             "local_map_match_device_ms_same_step": stat(rec["lmm_call"]), "local_map_match_sync_wall_ms_same_step": stat(rec["lmm_wall"])})
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f_:
            f_.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
