"""Python restatement of the mapper's local-map re-matching (test helper): do_local_map_matching + find_best_match (src/mapper.jl:318-462),
project_undistort / in_image (src/camera.jl:79-125), get_surrounding_keypoints (src/frame.jl:576-599), to_cartesian (src/SLAM.jl:30,42-45) and
mappoint_min_distance (src/map_point.jl:165-174), block by block on dicts and lists -- not on the packed arrays of the C ABI.

The structures are those slam_jl_amd.local_map_matching takes: frame {"Tcw", "cam", "cell_size", "nb_3d_kpts"}, keypoints [{"pixel",
"descriptors", "observers": [(key-frame row, pixel)]}], keyframes (K, 4, 4), local_map [{"position", "descriptors", "observers"}].  A keypoint's
list index is its id; a keypoint without descriptors stands for `kp.id < 0`, a vanished map point or an empty descriptor (mapper.jl:406, :411-415).

Besides the four outputs of the ABI the model returns `margin`: the smallest absolute distance of any gate quantity from its threshold (z - 0.1,
|view| - threshold, the four image bounds, every pixel distance and every observers' mean against max_projection_distance, every projection
coordinate from a .5 rounding boundary).  Exact equality with another implementation is only meaningful on inputs where no gate is decided by the
last bits (Julia's `norm` may or may not scale), so the parity tests assert margin >= 1e-9 on their scenes first: a condition on the inputs."""
import math

import numpy as np


def project_world_to_camera(Tcw, p):
    """frame.jl:458-462: f.cw * to_homogeneous(point), rows summed left to right"""
    return [((Tcw[r][0] * p[0] + Tcw[r][1] * p[1]) + Tcw[r][2] * p[2]) + Tcw[r][3] * 1.0 for r in range(4)]


def undistort_pdn_point(cam, point):
    """camera.jl:111-125; point (y, x) predivided"""
    fx, fy, cx, cy, k1, k2, p1, p2 = cam[:8]
    sq = (point[0] * point[0], point[1] * point[1])
    r2 = sq[0] + sq[1]
    rd = (1.0 + k1 * r2) + k2 * (r2 * r2)
    p = point[0] * point[1]
    dtx = (2 * p1) * p + p2 * (r2 + 2 * sq[0])
    dty = p1 * (r2 + 2 * sq[1]) + (2 * p2) * p
    dist = (rd * point[0] + dty, rd * point[1] + dtx)
    return (dist[0] * fy + cy, dist[1] * fx + cx)


def project_undistort(cam, point):
    """camera.jl:79-82: (x, y, z) -> (y, x)"""
    with np.errstate(all="ignore"):
        return undistort_pdn_point(cam, (np.float64(point[1]) / np.float64(point[2]), np.float64(point[0]) / np.float64(point[2])))


def in_image(cam, p):
    """camera.jl:90-92"""
    return 1 <= p[0] <= cam[8] and 1 <= p[1] <= cam[9]


def to_cartesian(pixel, cell_size):
    """SLAM.jl:30,42-45: round (to nearest even) .|> Int64, .÷ cell_size .+ 1"""
    r = [int(np.rint(pixel[0])), int(np.rint(pixel[1]))]
    return tuple((v // cell_size if v >= 0 else -(-v // cell_size)) + 1 for v in r)          # ÷ truncates


def hamming_distance(d1, d2):
    return float(sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(d1, d2)))


def mappoint_min_distance(desc1, desc2):
    """map_point.jl:165-174"""
    min_distance = 1e6
    for d1 in desc1:
        for d2 in desc2:
            distance = hamming_distance(d1, d2)
            if distance < min_distance:
                min_distance = distance
    return min_distance


class Margin:
    def __init__(self):
        self.value = math.inf

    def __call__(self, quantity, threshold):
        d = abs(quantity - threshold)
        if d == d and d < self.value:
            self.value = d


def build_grid(frame, keypoints):
    """frame.jl:321-327 (add_keypoint_to_grid!) for every keypoint in list order: cell -> keypoint ids, ascending inside a cell"""
    cam, cell = frame["cam"], frame["cell_size"]
    rows, cols = math.ceil(cam[8] / cell), math.ceil(cam[9] / cell)
    grid = {}
    for j, kp in enumerate(keypoints):
        grid.setdefault(to_cartesian(kp["pixel"], cell), []).append(j)
    return grid, rows, cols


def get_surrounding_keypoints(grid, rows, cols, pixel, cell_size):
    """frame.jl:576-599"""
    kpi = to_cartesian(pixel, cell_size)
    out = []
    for r in range(kpi[0] - 1, kpi[0] + 2):
        for c in range(kpi[1] - 1, kpi[1] + 2):
            if r < 1 or c < 1 or r > rows or c > cols:
                continue
            out.extend(grid.get((r, c), []))
    return out


def find_best_match(frame, keypoints, keyframes, target, projection, surrounding, max_projection_distance, max_descriptor_distance, margin, count):
    """mapper.jl:392-462"""
    cam = frame["cam"]
    target_observers = list(target["observers"])
    target_position = target["position"]
    min_distance = 256.0 * max_descriptor_distance
    best_distance, best_id = min_distance, -1
    for j in surrounding:
        kp = keypoints[j]
        if len(kp["descriptors"]) == 0:                                   # :406, :411-415
            continue
        distance = math.sqrt((projection[0] - kp["pixel"][0]) ** 2 + (projection[1] - kp["pixel"][1]) ** 2)       # :407
        margin(distance, max_projection_distance)
        if distance > max_projection_distance:
            continue
        if set(target_observers) & set(o[0] for o in kp["observers"]):   # :419-420
            count["overlap"] += 1
            continue
        avg_projection, n_projections = 0.0, 0                            # :422-442
        for kf_row, observer_pixel in kp["observers"]:
            op = project_undistort(cam, project_world_to_camera(keyframes[kf_row], target_position))
            avg_projection += math.sqrt((observer_pixel[0] - op[0]) ** 2 + (observer_pixel[1] - op[1]) ** 2)
            n_projections += 1
        avg_projection = avg_projection / n_projections if n_projections else math.nan      # 0.0 / 0 = NaN: the comparison below is false
        margin(avg_projection, max_projection_distance)
        if avg_projection > max_projection_distance:
            count["average"] += 1
            continue
        distance = mappoint_min_distance(target["descriptors"], kp["descriptors"])       # :444
        if distance <= best_distance:                                     # :445: the later candidate wins a tie
            if best_id != -1 and distance == best_distance:
                count["ties_forward"] += 1
            best_distance, best_id = distance, j
    return best_id, best_distance


def do_local_map_matching(frame, keypoints, keyframes, local_map, params):
    """mapper.jl:318-383 -> {"match" (N,), "best_kp" (M,), "best_dist" (M,), "proj_yx" (M, 2), "margin", "count"}.
    best_dist = -1 and proj_yx = NaN where find_best_match was not called, as the C ABI reports them; with no keypoint or no local-map point
    nothing is visited at all (the ABI launches nothing for such a stream)."""
    N, M = len(keypoints), len(local_map)
    out = {"match": np.full(N, -1, dtype=np.int32), "best_kp": np.full(M, -1, dtype=np.int32), "best_dist": np.full(M, -1.0),
           "proj_yx": np.full((M, 2), np.nan), "margin": math.inf,
           "count": {"overlap": 0, "average": 0, "ties_forward": 0, "ties_reverse": 0, "gated": 0, "contested": 0}}
    if M == 0 or N == 0:                                                  # :323
        return out
    cam = [float(v) for v in frame["cam"]]
    frame = dict(frame, cam=cam)
    keyframes = np.asarray(keyframes, dtype=np.float64).reshape(-1, 4, 4)
    margin, count = Margin(), out["count"]
    vfov = 0.5 * cam[8] / cam[1]                                          # :326-329
    hfov = 0.5 * cam[9] / cam[0]
    max_rad_fov = math.atan(vfov) if vfov > hfov else math.atan(hfov)
    view_threshold = math.cos(max_rad_fov)
    max_projection_distance = params.max_projection_distance
    if frame["nb_3d_kpts"] < 30:                                          # :332
        max_projection_distance *= 2.0
    grid, rows, cols = build_grid(frame, keypoints)
    matches = {}
    Tcw = np.asarray(frame["Tcw"], dtype=np.float64).reshape(4, 4)
    for m, mp in enumerate(local_map):                                    # :337
        camera_position = project_world_to_camera(Tcw, [float(v) for v in mp["position"]])[:3]       # :344-346
        margin(camera_position[2], 0.1)
        if camera_position[2] < 0.1:
            count["gated"] += 1
            continue
        view_angle = camera_position[2] / math.sqrt((camera_position[0] ** 2 + camera_position[1] ** 2) + camera_position[2] ** 2)    # :348-349
        margin(abs(view_angle), view_threshold)
        if abs(view_angle) < view_threshold:
            count["gated"] += 1
            continue
        projection = project_undistort(cam, camera_position)             # :351-352
        for q, hi in ((projection[0], cam[8]), (projection[1], cam[9])):
            margin(q, 1.0); margin(q, hi)
        if not in_image(cam, projection):
            count["gated"] += 1
            continue
        for q in projection:                                              # the cell of the projection: distance from a .5 boundary
            margin(q - math.floor(q), 0.5)
        surrounding = get_surrounding_keypoints(grid, rows, cols, projection, frame["cell_size"])    # :354
        best_id, best_distance = find_best_match(frame, keypoints, keyframes, mp, projection, surrounding, max_projection_distance,
                                                 params.max_descriptor_distance, margin, count)     # :357-360
        out["best_kp"][m], out["best_dist"][m], out["proj_yx"][m] = best_id, best_distance, projection
        if best_id == -1:
            continue
        matches.setdefault(best_id, []).append((m, best_distance))       # :362-367
    for kpid, match in matches.items():                                   # :370-381
        best_distance, best_id = 1e6, -1
        count["contested"] += len(match) > 1
        for local_kpid, distance in match:
            if distance <= best_distance:
                if best_id != -1 and distance == best_distance:
                    count["ties_reverse"] += 1
                best_distance, best_id = distance, local_kpid
            if best_id != -1:
                out["match"][kpid] = best_id
    out["margin"] = margin.value
    return out
