#!/usr/bin/env python3
"""What k_kpset_match fetches per keypoint, on fresh and on steady-state (multi-generation) lists of the headline loop.

  run:      S_=128 WARM_=6 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d DIR -- python3 scripts/probes/prof_work_order.py run POINTS.json
            (the headline loop, WARM_ untimed + 2 timed key-frame periods; POINTS.json: keypoints that entered every match launch, in launch order)
  summary:  python3 scripts/probes/prof_work_order.py summary DIR POINTS.json [label]
            per counter: the launches of the FIRST period (lists of one detect generation) against those after WARM_ periods.
            FETCH_SIZE is in KB and reports half of coalesced 8-byte reads (profiles/r01_pmc_pyramid.json): bytes = KB x 1024 x 2.
env SLAMHIP_WORK_BAND selects the order of the work list (0: slot order).  Counters serialise the launches: the figures are of the kernel alone."""
import os, sys, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
KF = 5


def run(points_path):
    import torch
    import slam_jl_amd as slam
    from slam_jl_amd import synthetic as syn
    import bench
    S = int(os.environ.get("S_", "128")); warm = int(os.environ.get("WARM_", "6"))
    wl = bench.make_workload(slam, syn, "kitti05_1000", seed=0, streams=S)
    tot = {}

    def diag(i, kf, pst, ks, ctx, off):
        tot[i] = int(ks.counts(ctx=ctx).sum())
    r = bench.run_lockstep_kpset(slam, torch, 0, wl, 2, warm, 1, None, torch.device("cuda", 0), "host_u8", diag=diag)
    launches = []                                               # (frame step, kind, keypoints entering): temporal before stereo inside a step
    for i in sorted(tot):
        if tot.get(i - 1, 0) > 0:
            launches.append((i, "temporal", tot[i - 1]))
        if (i - 1) % KF == 0:
            launches.append((i, "stereo", tot[i]))              # the stereo match keeps every keypoint: the count after the step entered it
    json.dump({"S": S, "warm_periods": warm, "band": os.environ.get("SLAMHIP_WORK_BAND", "default"), "launches": launches,
               "frames_per_s": r["value"]}, open(points_path, "w"))
    print("launches", len(launches), "frames/s under the profiler", round(r["value"]))


def summary(d, points_path, label=""):
    import csv, glob, collections
    P = json.load(open(points_path)); L = P["launches"]
    per = collections.defaultdict(dict)
    for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
        for k, row in enumerate(csv.DictReader(open(f))):
            if "k_kpset_match" in row["Kernel_Name"]:
                per[row["Counter_Name"]][int(row.get("Dispatch_Id", k))] = float(row["Counter_Value"])
    for name, by_id in sorted(per.items()):
        vals = [by_id[k] for k in sorted(by_id)]
        assert len(vals) == len(L), (name, len(vals), len(L))
        fresh = [(v, n) for v, (i, kind, n) in zip(vals, L) if i <= KF]
        steady = [(v, n) for v, (i, kind, n) in zip(vals, L) if i > P["warm_periods"] * KF]
        for tag, grp in (("fresh (period 1)", fresh), ("steady (after %d periods)" % P["warm_periods"], steady)):
            per_pt = [v / n for v, n in grp]
            line = f"{label} band={P['band']} {name} {tag}: {len(grp)} launches, {sum(n for _, n in grp) / len(grp):.0f} keypoints per launch, per keypoint mean {sum(per_pt) / len(per_pt):.4g} min {min(per_pt):.4g} max {max(per_pt):.4g}"
            if name == "FETCH_SIZE":
                line += f"  = {sum(per_pt) / len(per_pt) * 2048 / 1e3:.2f} KB per keypoint, {sum(v for v, _ in grp) / len(grp) * 2048 / 1e9:.3f} GB per launch (x2 applied)"
            print(line)
    if "TCC_HIT_sum" in per and "TCC_MISS_sum" in per:
        for tag, sel in (("fresh", lambda i: i <= KF), ("steady", lambda i: i > P["warm_periods"] * KF)):
            h = sum(v for v, (i, _, _) in zip([per["TCC_HIT_sum"][k] for k in sorted(per["TCC_HIT_sum"])], L) if sel(i))
            m = sum(v for v, (i, _, _) in zip([per["TCC_MISS_sum"][k] for k in sorted(per["TCC_MISS_sum"])], L) if sel(i))
            print(f"{label} band={P['band']} L2 hit rate {tag}: {h / (h + m):.3f}")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        summary(*sys.argv[2:5])
