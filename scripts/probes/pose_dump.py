"""Byte comparison of the six array seams of the pose stage (slam_p3p_ransac(_batch), slam_five_point_ransac(_batch), slam_pnp_ba(_batch)) between
two builds of the library: the cases of tests/test_gpu_pose_records.py -- every problem size alone and in the S = 3 batches, iters 0 / 1 / 16, every
nullable output given and NULL in turn -- with every output of every call dumped.  One library per process; run it under a time limit.
    python scripts/probes/pose_dump.py dump OUT.npz           the library is the package's, or the one SLAMHIP_LIB names
    python scripts/probes/pose_dump.py compare A.npz B.npz    every array byte for byte; exit status 1 if any differs"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    if sys.argv[1] == "compare":
        a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
        diff = [k for k in sorted(set(a.files) | set(b.files)) if k not in a.files or k not in b.files or a[k].dtype != b[k].dtype or a[k].tobytes() != b[k].tobytes()]
        print(f"pose_dump: {len(a.files)} arrays, {len(diff)} differing" + "".join("\n  " + k for k in diff[:40]))
        sys.exit(1 if diff else 0)
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import slam_jl_amd as slam
    import test_gpu_pose_records as T
    slam.default_context(0)
    out = {}
    for seam, iters in T.CASES:
        for ns, batch in T.call_sets():
            for null in [()] + [(name,) for name in T.NULLABLE[seam]]:
                res = T.run(slam, seam, ns, iters, batch, null=null)
                pre = f"{seam}/iters{iters}/{'batch' if batch else 'single'}_{'_'.join(map(str, ns))}/null_{null[0] if null else 'none'}/"
                for name, rows in res.items():
                    for z, v in enumerate(rows):
                        out[pre + f"{name}/{z}"] = v
    np.savez(sys.argv[2], **out)
    print(f"pose_dump: {len(out)} arrays -> {sys.argv[2]} ({os.environ.get('SLAMHIP_LIB', 'the package library')})")


if __name__ == "__main__":
    main()
