#!/usr/bin/env python3
"""Phase table of k_kpset_match on the headline loop's steady-state lists (needs slam.jl_amd/libslamhip_trace.so: make -C slam.jl_amd/csrc trace).

    S_=128 WARM_=3 python3 scripts/probes/lk_trace_kpset.py [label]

Runs the headline loop (WARM_ untimed + 2 timed key-frame periods) on the trace build, throws away the ticks of the first period (lists of
one detect generation) and prints, for the matches after it, every phase's share of the summed wave time.  Ticks are the 100 MHz wall clock,
summed over waves (lk.hip, LK_TRACE): a share says where a wave spends its slot, not what a launch costs.  The clocks and their atomics slow
the kernel itself; compare tables of two builds, not a table with a product build's timing.
Phases: 6 the prologue of k_kpset_match (wave start, or the previous keypoint's end, to the keypoint's position, prior and in-image decision
in registers), 7 the rest of the keypoint (level visits + stores); inside the level visits: 5 position + offsets, 1 set-up loads + gradient,
2 eig test, 3 LDS samples + accumulate, 4 reduce + solve."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault("SLAMHIP_LIB", os.path.join(ROOT, "slam.jl_amd", "libslamhip_trace.so"))
import ctypes as C
KF = 5


def main(label=""):
    import torch
    import slam_jl_amd as slam
    from slam_jl_amd import synthetic as syn
    import bench
    S = int(os.environ.get("S_", "128")); warm = int(os.environ.get("WARM_", "3"))
    lib = slam.load()
    lib.slam_debug_lk_ticks.restype = C.c_int
    buf = (C.c_ulonglong * 8)()
    wl = bench.make_workload(slam, syn, "kitti05_1000", seed=0, streams=S)
    tot, pts = {}, [0]

    def diag(i, kf, pst, ks, ctx, off):
        tot[i] = int(ks.counts(ctx=ctx).sum())                  # (synchronises the stream: every match enqueued so far has run)
        if i == KF:
            lib.slam_debug_lk_ticks(buf)                        # read and clear: the first period does not count
        elif i > KF:
            if tot.get(i - 1, 0) > 0:
                pts[0] += tot[i - 1]                            # the temporal match of this step
            if (i - 1) % KF == 0:
                pts[0] += tot[i]                                # its stereo match (keeps every keypoint)
    bench.run_lockstep_kpset(slam, torch, 0, wl, 2, warm, 1, None, torch.device("cuda", 0), "host_u8", diag=diag)
    lib.slam_debug_lk_ticks(buf)
    t = [int(b) for b in buf]
    total = t[6] + t[7]
    n = max(pts[0], 1)
    print(f"{label} k_kpset_match phases, S = {S}, periods 2..{warm + 2}, {pts[0]} keypoint visits, knob SLAMHIP_NO_MATCH_REC={os.environ.get('SLAMHIP_NO_MATCH_REC', 'unset')}")
    print(f"{'phase':<58}{'us per keypoint':>16}{'share of wave time':>20}")
    rows = (("6 prologue (to position, prior, decision in registers)", t[6]), ("7 level visits + stores", t[7]),
            ("  5 position + offsets", t[5]), ("  1 set-up loads (template, patch, corners) + gradient", t[1]), ("  2 eig test", t[2]),
            ("  3 LDS samples + accumulate", t[3]), ("  4 reduce + solve", t[4]))
    for name, v in rows:
        print(f"{name:<58}{v * 10.0 / n / 1e3:>16.3f}{100.0 * v / max(total, 1):>19.2f}%")
    print(f"{'total (6 + 7)':<58}{total * 10.0 / n / 1e3:>16.3f}{100.0:>19.2f}%")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "")
