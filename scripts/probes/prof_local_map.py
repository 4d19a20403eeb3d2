"""One slam_local_map_match_batch call at the mapper's size, timed with hipEvents (the library's profiling spans) after warm-up, median of repeats.

Shape: S = 128 streams, 370 x 1226, cell_size 35, N = 1 000 keypoints, M = 10 000 local-map points, K = 25 key-frames, 5 descriptors per point.
Four distinct scenes are generated and repeated over the streams.  Reports the whole call on the device (copy in, memset, kernel, copy out), the
kernel alone, the wall time of the C call and the call's share of a 28.9-ms key-frame period.

    python scripts/probes/prof_local_map.py [--streams 128] [--repeats 15] [--cache scenes.npz] [--out record.json]
    python scripts/probes/prof_local_map.py --widths        # the same in a child process per group width, on the libraries `make -C slam.jl_amd/csrc widths` built
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PERIOD_MS = 28.9


def packs(args):
    import slam_jl_amd as slam
    from slam_jl_amd import synthetic as syn
    if args.cache and os.path.exists(args.cache):
        z = np.load(args.cache)
        n = int(z["count"])
        return [{k[3:]: (int(z[k]) if z[k].ndim == 0 else z[k]) for k in z.files if k.startswith("%02d_" % i)} for i in range(n)]
    rng = np.random.default_rng(1)
    out = []
    for seed in range(args.distinct):
        s = syn.local_map_scene(seed=seed, H=370, W=1226, cell_size=35, N=args.N, M=args.M, K=25)
        for q in s["keypoints"] + s["local_map"]:              # 5 descriptors per point that has any
            d = q["descriptors"]
            if len(d):
                q["descriptors"] = np.concatenate([d, syn._lm_flip(rng, np.repeat(d[:1], 5, axis=0), 6)])[:5]
        out.append(slam.pack_local_map(s["frame"], s["keypoints"], s["keyframes"], s["local_map"], s["params"]))
    if args.cache:
        flat = {"count": np.int64(len(out))}
        for i, p in enumerate(out):
            flat.update({"%02d_%s" % (i, k): np.asarray(v) for k, v in p.items()})
        np.savez(args.cache, **flat)
    return out


def measure(args):
    import slam_jl_amd as slam
    from slam_jl_amd import _lib as L, local_map as lm
    distinct = packs(args)
    p, kp_off, kf_off, mp_off = slam.concat_packs([distinct[s % len(distinct)] for s in range(args.streams)])
    a, out = lm._args(p)
    ctx = slam.default_context(0)
    call = lambda: ctx.check(ctx.lib.slam_local_map_match_batch(ctx.h, args.streams, L.ptr(kp_off, L.i32p), L.ptr(kf_off, L.i32p), L.ptr(mp_off, L.i32p), C.byref(a)))
    for _ in range(3):
        call()
    ctx.prof_enable(True)
    dev, ker, wall = [], [], []
    for _ in range(args.repeats):
        ctx.prof_reset()
        t0 = time.perf_counter(); call(); wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(ctx.prof_get("local_map_match")[0]); ker.append(ctx.prof_get("local_map_match_kernel")[0])
    ctx.prof_enable(False)
    nb = sum(int(np.asarray(v).nbytes) for k, v in p.items() if k not in ("N", "K", "M"))
    return {"lib": os.path.basename(slam.LIB_PATH), "S": args.streams, "N": args.N, "M": args.M, "K": 25, "shape": [370, 1226], "repeats": args.repeats,
            "input_mb": round(nb / 1e6, 1), "matched_per_stream": round(float((out["match"] >= 0).sum()) / args.streams, 1),
            "chosen_per_stream": round(float((out["best_kp"] >= 0).sum()) / args.streams, 1),
            "device_ms": round(float(np.median(dev)), 3), "device_ms_min_max": [round(min(dev), 3), round(max(dev), 3)],
            "kernel_ms": round(float(np.median(ker)), 3), "kernel_ms_min_max": [round(min(ker), 3), round(max(ker), 3)],
            "wall_ms": round(float(np.median(wall)), 3), "share_of_keyframe_period": round(float(np.median(dev)) / PERIOD_MS, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--M", type=int, default=10000)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--widths", action="store_true")
    args = ap.parse_args()
    if args.widths:
        rec = {"widths": {}}
        for g in (16, 32, 64):
            lib = os.path.join(ROOT, "slam.jl_amd", "libslamhip_g%d.so" % g)
            if not os.path.exists(lib):
                sys.exit(f"{lib} is missing: make -C slam.jl_amd/csrc widths")
            cmd = [sys.executable, os.path.abspath(__file__), "--streams", str(args.streams), "--repeats", str(args.repeats), "--distinct", str(args.distinct),
                   "--N", str(args.N), "--M", str(args.M)] + (["--cache", args.cache] if args.cache else [])
            r = subprocess.run(cmd, env=dict(os.environ, SLAMHIP_LIB=lib), stdout=subprocess.PIPE, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"G = {g}: exit status {r.returncode}")
            rec["widths"]["G%d" % g] = json.loads(r.stdout.strip().splitlines()[-1])
    else:
        rec = measure(args)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
