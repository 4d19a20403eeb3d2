"""Byte comparison of the key-frame map (slam_kfmap_*) between two builds of the library.  `dump` replays the scripts of the key-frame map's GPU tests --
tests/test_gpu_kfmap.py (kfmap_scripts), _filter (np_kfmap_filter.frames), _local_map (kfmap_lmm_scripts), _merge (kfmap_merge_scripts) and
_local_map_history (kfmap_history_scripts) -- by running those test modules in this process with KeyframeMap's methods wrapped: after EVERY call that
acts on the map (add_keyframe, add_descriptors, gather, update, filter, remove_keyframe, local_map_match, merge, reset, the two enable_*) it records
every output of the call (gather arrays and statuses, removed key-frames, match statuses / pairs / distances, merge counts, an error's text without its
file:line) and the map's whole state: download_keyframe of every slot and download_points of every stream, debug_local_map where a match has staged,
local_map_ids where the history is on, the live lists where a keypoint set is attached.  One library per process; run it under a time limit.
    python scripts/probes/kfmap_dump.py dump OUT.npz           the library is the package's, or the one SLAMHIP_LIB names
    python scripts/probes/kfmap_dump.py compare A.npz B.npz    every array byte for byte; exit status 1 if any differs
An array is stored once per content (sha256); `names` / `digests` map every recorded name to its content."""
import dataclasses
import hashlib
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MODULES = ("test_gpu_kfmap.py", "test_gpu_kfmap_filter.py", "test_gpu_kfmap_local_map.py", "test_gpu_kfmap_merge.py", "test_gpu_kfmap_local_map_history.py")
WRAPPED = ("add_keyframe", "add_descriptors", "gather", "update", "filter", "remove_keyframe", "local_map_match", "merge", "reset", "enable_descriptors",
           "enable_local_map_history")


class Recorder:
    def __init__(self):
        self.names, self.digests, self.blobs, self.calls = [], [], {}, {}

    def put(self, name, v):
        """flattens v -- arrays, numbers, strings, None, lists / tuples / dicts / dataclasses of them -- into named arrays"""
        if v is None:
            v = np.zeros(0, dtype=np.uint8)
        if isinstance(v, str):
            v = np.frombuffer(v.encode(), dtype=np.uint8)
        if isinstance(v, dict):
            for k in sorted(v):
                self.put(f"{name}/{k}", v[k])
        elif dataclasses.is_dataclass(v) or (hasattr(v, "__dict__") and not isinstance(v, np.ndarray) and not callable(v)):
            self.put(name, {k: x for k, x in vars(v).items() if not k.startswith("_")})
        elif isinstance(v, (list, tuple)) and not all(isinstance(x, (int, float, bool, np.integer, np.floating)) for x in v):
            self.put(f"{name}/len", np.int64(len(v)))
            for i, x in enumerate(v):
                self.put(f"{name}/{i}", x)
        else:
            a = np.ascontiguousarray(np.asarray(v))
            d = hashlib.sha256(str((a.dtype, a.shape)).encode() + a.tobytes()).hexdigest()
            self.blobs.setdefault(d, a)
            self.names.append(name); self.digests.append(d)

    def state(self, pre, km, slam):
        newest = km.newest()
        self.put(pre + "newest", newest)
        for s in range(km.S):
            for k in range(max(int(newest[s]) - km.R + 1, 0), int(newest[s]) + 2):
                self.put(f"{pre}kf/{s}/{k}", km.download_keyframe(s, k))
                if getattr(km, "_dump_history", False):
                    try:
                        self.put(f"{pre}local_map_ids/{s}/{k}", km.local_map_ids(s, k))
                    except slam.SlamHipError as e:
                        self.put(f"{pre}local_map_ids/{s}/{k}", _text(e))
            self.put(f"{pre}points/{s}", km.download_points(s))
            if getattr(km, "_dump_staged", False):
                self.put(f"{pre}debug_local_map/{s}", km.debug_local_map(s))
            ks = getattr(km, "_dump_ks", None)
            if ks is not None and getattr(ks, "h", None):
                self.put(f"{pre}list/{s}", ks.download(s))


def _text(e):
    return re.sub(r"\s*\([^()]*:\d+\)", "", str(e))          # an argument check's message names its file and line, which move with the code


def install(slam, rec):
    KM = slam.KeyframeMap
    for name in WRAPPED:
        orig = getattr(KM, name)

        def wrapped(self, *a, _orig=orig, _name=name, **kw):
            test = os.environ.get("PYTEST_CURRENT_TEST", "-").split(" ")[0]
            n = rec.calls[test] = rec.calls.get(test, -1) + 1
            pre = f"{test}/{n:05d}/{_name}/"
            if _name in ("add_keyframe", "update", "merge"):
                ks = a[0] if _name != "update" and a else kw.get("ks")
                if ks is not None and hasattr(ks, "download"):
                    self._dump_ks = ks
            try:
                out = _orig(self, *a, **kw)
                rec.put(pre + "out", out)
                return out
            except slam.SlamHipError as e:
                rec.put(pre + "error", _text(e))
                raise
            finally:
                if _name == "enable_local_map_history":
                    self._dump_history = True
                if _name == "local_map_match" and "out" in locals():
                    self._dump_staged = True
                if getattr(self, "h", None):
                    rec.state(pre, self, slam)
        setattr(KM, name, wrapped)


def main():
    if sys.argv[1] == "compare":
        a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
        ia, ib = dict(zip(a["names"], a["digests"])), dict(zip(b["names"], b["digests"]))
        diff = [k for k in sorted(set(ia) | set(ib)) if ia.get(k) != ib.get(k)]
        print(f"kfmap_dump: {len(ia)} arrays against {len(ib)}, {len(diff)} differing" + "".join("\n  " + k for k in diff[:40]))
        sys.exit(1 if diff or not ia else 0)
    import pytest
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import slam_jl_amd as slam
    rec = Recorder()
    install(slam, rec)
    rc = pytest.main(["-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] + [os.path.join(ROOT, "tests", m) for m in MODULES])
    if rc != 0:
        sys.exit(f"kfmap_dump: the replayed tests ended with status {rc}: nothing written")
    np.savez_compressed(sys.argv[2], names=np.array(rec.names), digests=np.array(rec.digests), **{"blob_" + d: v for d, v in rec.blobs.items()})
    print(f"kfmap_dump: {len(rec.names)} arrays ({len(rec.blobs)} different) of {sum(n + 1 for n in rec.calls.values())} calls in {len(rec.calls)} tests -> {sys.argv[2]} "
          f"({os.environ.get('SLAMHIP_LIB', 'the package library')})")


if __name__ == "__main__":
    main()
