"""Byte comparison of the local BA between two builds of the library: every window of hp_ba.stage_windows / batch_windows solved through
slam_local_ba (two passes, default iterations) and the batch test's mixed batch through slam_local_ba_batch, under the default environment and
under each switch that selects another kernel route -- one fresh process per environment, one at a time, each with a time limit.
    python scripts/probes/ba_dump.py dump OUT.npz           theta, outlier flags and the stats (without the device-milliseconds entry) of every solve;
                                                            the library is the package's, or the one SLAMHIP_LIB names
    python scripts/probes/ba_dump.py compare A.npz B.npz    every array byte for byte; exit status 1 if any differs"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ENVS = {"default": {}, "no_groups": {"SLAMHIP_NO_GROUPS": "1"}, "no_band": {"SLAMHIP_NO_BAND": "1"}, "no_twist": {"SLAMHIP_NO_TWIST": "1"},
        "no_mfma": {"SLAMHIP_BA_NO_MFMA": "1"}, "window_one": {"SLAMHIP_BA_WINDOW_ONE": "1"}}
STATS = ("ssr_init", "ssr_pass1", "ssr_final", "iters_pass1", "iters_pass2", "n_outliers")


def child(path):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hp_ba as hp
    from test_gpu_ba_stages import BATCH                  # the batch test's mixed batch: one list, the test's
    import slam_jl_amd as slam
    from slam_jl_amd import synthetic as syn
    slam.default_context(0)
    W = dict(hp.stage_windows(syn)); W.update(hp.batch_windows(syn))
    cache = lambda s: slam.LocalBACache(s["theta0"].copy(), s["theta_const"], s["pixels_yx"], s["pose_ids"], s["point_ids"])
    out = {}
    for nm, s in W.items():
        c = slam.bundle_adjustment_(cache(s), s["cam"])
        out[f"single/{nm}/theta"] = c.theta; out[f"single/{nm}/outl"] = c.outliers
        out[f"single/{nm}/stats"] = np.array([float(c.stats[k]) for k in STATS])
    b = slam.BABatch([cache(W[nm]) for nm in BATCH], W[BATCH[0]]["cam"])
    status = b.solve()
    for z, nm in enumerate(BATCH):
        th, ol, st = b.window(z)
        out[f"batch/{nm}/theta"] = th; out[f"batch/{nm}/outl"] = ol
        out[f"batch/{nm}/stats"] = np.array([float(st[k]) for k in STATS] + [float(status[z])])
    np.savez(path, **out)
    print("OK")


def dump(path):
    allv = {}
    with tempfile.TemporaryDirectory() as tmp:
        for tag, env in ENVS.items():
            part = os.path.join(tmp, tag + ".npz")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", part], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300, cwd=ROOT)
            if r.returncode != 0 or not r.stdout.strip().endswith("OK"):      # nothing more is started on the device after a failure
                print(f"{tag}: exit status {r.returncode}\n{r.stdout[-800:]}{r.stderr[-2500:]}")
                return 1
            z = np.load(part)
            allv.update({f"{tag}/{k}": z[k] for k in z.files})
            print(f"{tag}: {len(z.files)} arrays", flush=True)
    np.savez(path, **allv)
    print(f"{path}: {len(allv)} arrays, library {os.environ.get('SLAMHIP_LIB', '(the package default)')}")
    return 0


def compare(a, b):
    A, B = np.load(a), np.load(b)
    differing = [k for k in sorted(set(A.files) | set(B.files))
                 if k not in A.files or k not in B.files or A[k].dtype != B[k].dtype or A[k].shape != B[k].shape or A[k].tobytes() != B[k].tobytes()]
    print(f"{len(A.files)} / {len(B.files)} arrays, differing: {differing}")
    return 1 if differing else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "child": child(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "dump": sys.exit(dump(sys.argv[2]))
    elif len(sys.argv) == 4 and sys.argv[1] == "compare": sys.exit(compare(sys.argv[2], sys.argv[3]))
    else: sys.exit(__doc__)
