"""Host mirror of the mapper's local-map re-matching (reference: src/mapper.jl:318-462, src/map_point.jl:165-174).

`local_map_matching(...)` is the array-level body of do_local_map_matching: the local map is projected into the new key-frame and matched against
the keypoints of the surrounding grid cells by descriptor distance on the GPU (slam_local_map_match); the hash-map work around it (the union! of
local-map ids, merge_mappoints, the remove_mappoint_obs! clean-ups) is the caller's.  Inputs are plain Python / numpy structures:

  frame      {"Tcw": 4x4, "cam": (fx, fy, cx, cy, k1, k2, p1, p2, height, width), "cell_size": int, "nb_3d_kpts": int}
  keypoints  list of {"pixel": (y, x) 1-based, "descriptors": (D, 4) uint64 rows of slam.describe, "observers": [(key-frame row, (y, x)), ...]}
             in the order the candidates of a cell are to be met (a keypoint without descriptors is skipped)
  keyframes  (K, 4, 4) Tcw of every key-frame the observer lists name
  local_map  list of {"position": (x, y, z), "descriptors": (D, 4) uint64, "observers": [key-frame row, ...]} in iteration order
  params     anything with max_projection_distance / max_descriptor_distance (slam_jl_amd.Params)"""
import ctypes as C

import numpy as np

from . import _lib as L


class LocalMapArgs(C.Structure):
    """slam_local_map_args (include/slamhip.h)"""
    _fields_ = [("Tcw", L.f64p), ("cam", L.f64p), ("cell_size", L.i32p), ("nb_3d_kpts", L.i32p),
                ("max_projection_distance", L.f64p), ("max_descriptor_distance", L.f64p),
                ("kp_yx", L.f64p), ("kp_desc_off", L.i32p), ("kp_desc", L.u64p), ("kp_obs_off", L.i32p), ("kp_obs_kf", L.i32p), ("kp_obs_yx", L.f64p),
                ("kf_Tcw", L.f64p),
                ("mp_xyz", L.f64p), ("mp_desc_off", L.i32p), ("mp_desc", L.u64p), ("mp_obs_off", L.i32p), ("mp_obs_kf", L.i32p),
                ("match", L.i32p), ("best_kp", L.i32p), ("best_dist", L.f64p), ("proj_yx", L.f64p)]


_IN = ("Tcw", "cam", "cell_size", "nb_3d_kpts", "max_projection_distance", "max_descriptor_distance", "kp_yx", "kp_desc_off", "kp_desc",
       "kp_obs_off", "kp_obs_kf", "kp_obs_yx", "kf_Tcw", "mp_xyz", "mp_desc_off", "mp_desc", "mp_obs_off", "mp_obs_kf")
_PTR = {name: t for name, t in LocalMapArgs._fields_}


def _csr(lists, width, dtype):
    """ragged list of (n_i, width) arrays -> (offsets (len + 1,) int32, values (sum n_i, width))"""
    rows = [np.asarray(x, dtype=dtype).reshape(-1, width) for x in lists]
    off = np.zeros(len(rows) + 1, dtype=np.int32)
    if rows:
        off[1:] = np.cumsum([len(r) for r in rows])
    vals = np.concatenate(rows) if rows else np.zeros((0, width), dtype=dtype)
    return off, np.ascontiguousarray(vals.reshape(-1, width), dtype=dtype)


def pack_local_map(frame, keypoints, keyframes, local_map, params):
    """The arrays of slam_local_map_match for one stream, as a dict keyed by the fields of slam_local_map_args (+ N, K, M)."""
    p = {"Tcw": np.ascontiguousarray(np.asarray(frame["Tcw"], dtype=np.float64).reshape(4, 4).T).reshape(1, 16),      # column-major
         "cam": np.ascontiguousarray(frame["cam"], dtype=np.float64).reshape(1, 10),
         "cell_size": np.array([frame["cell_size"]], dtype=np.int32), "nb_3d_kpts": np.array([frame["nb_3d_kpts"]], dtype=np.int32),
         "max_projection_distance": np.array([params.max_projection_distance], dtype=np.float64),
         "max_descriptor_distance": np.array([params.max_descriptor_distance], dtype=np.float64)}
    p["kp_yx"] = np.ascontiguousarray([k["pixel"] for k in keypoints], dtype=np.float64).reshape(-1, 2)
    p["kp_desc_off"], p["kp_desc"] = _csr([k["descriptors"] for k in keypoints], 4, np.uint64)
    p["kp_obs_off"], kf = _csr([[o[0] for o in k["observers"]] for k in keypoints], 1, np.int32)
    p["kp_obs_kf"] = kf.reshape(-1)
    p["kp_obs_yx"] = _csr([[o[1] for o in k["observers"]] for k in keypoints], 2, np.float64)[1]
    kfs = np.asarray(keyframes, dtype=np.float64).reshape(-1, 4, 4)
    p["kf_Tcw"] = np.ascontiguousarray(kfs.transpose(0, 2, 1)).reshape(-1, 16)
    p["mp_xyz"] = np.ascontiguousarray([m["position"] for m in local_map], dtype=np.float64).reshape(-1, 3)
    p["mp_desc_off"], p["mp_desc"] = _csr([m["descriptors"] for m in local_map], 4, np.uint64)
    p["mp_obs_off"], kf = _csr([m["observers"] for m in local_map], 1, np.int32)
    p["mp_obs_kf"] = kf.reshape(-1)
    p["N"], p["K"], p["M"] = len(keypoints), len(kfs), len(local_map)
    return p


def concat_packs(packs):
    """S packs of pack_local_map -> (one pack of the concatenated arrays, kp_offsets, kf_offsets, mp_offsets) as slam_local_map_match_batch reads them"""
    out = {}
    for name in _IN:
        if name.endswith("_off"):
            base, parts = 0, [np.zeros(1, dtype=np.int32)]
            for q in packs:
                parts.append(q[name][1:] + base); base += int(q[name][-1])
            out[name] = np.concatenate(parts).astype(np.int32)
        else:
            out[name] = np.ascontiguousarray(np.concatenate([q[name] for q in packs]))
    offs = [np.concatenate([[0], np.cumsum([q[k] for q in packs])]).astype(np.int32) for k in ("N", "K", "M")]
    out["N"], out["K"], out["M"] = int(offs[0][-1]), int(offs[1][-1]), int(offs[2][-1])
    return out, offs[0], offs[1], offs[2]


def _args(p):
    """-> (LocalMapArgs over the pack's arrays with fresh outputs, the outputs)"""
    out = {"match": np.empty(p["N"], dtype=np.int32), "best_kp": np.empty(p["M"], dtype=np.int32),
           "best_dist": np.empty(p["M"], dtype=np.float64), "proj_yx": np.empty((p["M"], 2), dtype=np.float64)}
    a = LocalMapArgs()
    for name in _IN:
        setattr(a, name, p[name].ctypes.data_as(_PTR[name]))
    for name, arr in out.items():
        setattr(a, name, arr.ctypes.data_as(_PTR[name]))
    return a, out


def local_map_matching_packed(p, ctx=None):
    """slam_local_map_match on a pack of pack_local_map -> {"match", "best_kp", "best_dist", "proj_yx"}"""
    ctx = ctx or L.default_context()
    a, out = _args(p)
    ctx.check(ctx.lib.slam_local_map_match(ctx.h, C.byref(a), p["N"], p["K"], p["M"]))
    return out


def local_map_matching(frame, keypoints, keyframes, local_map, params, ctx=None):
    """do_local_map_matching(mapper, frame, local_map; max_projection_distance, max_descriptor_distance) on arrays.
    Returns {"match": (N,) int32 local-map index per keypoint or -1 (prev_new_map), "best_kp": (M,) int32, "best_dist": (M,), "proj_yx": (M, 2)}."""
    return local_map_matching_packed(pack_local_map(frame, keypoints, keyframes, local_map, params), ctx)


def local_map_matching_batch(problems, ctx=None):
    """S streams in one call: problems = [(frame, keypoints, keyframes, local_map, params), ...] -> list of S result dicts, equal to S single calls."""
    ctx = ctx or L.default_context()
    packs = [pack_local_map(*q) for q in problems]
    p, kp_off, kf_off, mp_off = concat_packs(packs)
    a, out = _args(p)
    ctx.check(ctx.lib.slam_local_map_match_batch(ctx.h, len(packs), L.ptr(kp_off, L.i32p), L.ptr(kf_off, L.i32p), L.ptr(mp_off, L.i32p), C.byref(a)))
    return [{"match": out["match"][kp_off[s]:kp_off[s + 1]].copy(), "best_kp": out["best_kp"][mp_off[s]:mp_off[s + 1]].copy(),
             "best_dist": out["best_dist"][mp_off[s]:mp_off[s + 1]].copy(), "proj_yx": out["proj_yx"][mp_off[s]:mp_off[s + 1]].copy()}
            for s in range(len(packs))]
