"""Scripted scenes for the local-map match on the key-frame map (test helper): kfmap_scripts.make_stream's key-frame lists (which ids live, which are
3-D) seen through a SMALL camera -- a 70 x 105 image with cell 35, a 2 x 3 grid -- plus a descriptor script.

Pixels: a keypoint's pixel is the projection of its world point plus a fraction of a pixel of hashed noise where that lies in the image, else a hashed
place in the image (the map only needs numbers; most world points of make_stream's volume fall outside so small an image).
Descriptors: every new point draws a random 256-bit row.  A seeded share of the new points are COPIES of an older 3-D point that the new key-frame
does not carry and whose map position projects into the image: the copy's row is the older point's with 0 .. 20 hashed bits flipped and its pixel lies
within 0.85 px of that projection (max_projection_distance is 2), so that real matches occur.  A share of the copies are TWINS: no bit flipped, 3-D at
birth, their world point 1 mm from the older point's -- once both have left the lists, a later copy of either is equally far from both, the tie that
tells `<=` from `<` in the reverse selection.  Every number is a function of (seed, id, key-frame)."""
from types import SimpleNamespace

import numpy as np

import kfmap_scripts as scr

H, W, CELL = 70, 105, 35
CAM10 = (60.0, 60.0, 52.0, 35.0, 0.0, 0.0, 0.0, 0.0, float(H), float(W))
PARAMS = SimpleNamespace(max_projection_distance=2.0, max_descriptor_distance=0.35)
CAP, R, MCAP, S = 64, 4, 128, 3
# S = 3 streams, 8 key-frames each, about 40 keypoints per list (cap 64: 0, 1, 63 and 64 occur)
SEEDS = (21, 22, 23)
SIZES = ((40, 42, 38, 44, 41, 64, 39, 43), (36, 40, 63, 41, 37, 42, 40, 38), (1, 40, 44, 0, 42, 39, 41, 40))
# the sequence both test files run: every stream at every key-frame but the last, where stream 1 is not selected; a local bundle adjustment's update
# (hashed outliers: tombstones, removed points) behind key-frames 3 and 4 only -- one at every key-frame would remove the points whose dead observation is
# what the `dead` mutant counts before the ring turns far enough to show it
N_KF, LAST_MASK, BA_AT = 8, (1, 0, 1), (3, 4)


def project(T, X):
    """pinhole projection (y, x) of world point X through Tcw = T with CAM10, or None behind the camera"""
    c = T[:3, :3] @ np.asarray(X, dtype=np.float64) + T[:3, 3]
    if c[2] < 0.1:
        return None
    return np.array([CAM10[1] * c[1] / c[2] + CAM10[3], CAM10[0] * c[0] / c[2] + CAM10[2]])


def random_row(seed, i):
    return np.array([int(scr._u(seed, 61, i, w) * 2.0 ** 32) << 32 | int(scr._u(seed, 62, i, w) * 2.0 ** 32) for w in range(4)], dtype=np.uint64)


def flipped(row, seed, i, nflip):
    out = [int(v) for v in row]
    bits = sorted({int(scr._u(seed, 63, i, t) * 256) for t in range(nflip)})      # (a repeated position flips once: at most nflip bits)
    for b in bits:
        out[b >> 6] ^= 1 << (b & 63)
    return np.array(out, dtype=np.uint64)


def make_scene(seed, sizes, p_copy=0.45, p_twin=0.3, window=3, **kw):
    """-> (frames, descs): frames as make_stream's with this module's pixels (and the twins' positions); descs[k] = (first new id, (n_new, 4) rows)"""
    kw = dict(dict(p_drop=0.4, p_long=0.15, p3=0.75, p_promote=0.5), **kw)
    frames = scr.make_stream(seed, sizes, **kw)
    world, rows, known, last_seen, seen, twins = {}, {}, {}, {}, set(), set()
    descs = []
    for k, f in enumerate(frames):
        T, ids = f["Tcw"], [int(i) for i in f["ids"]]
        err = {i: f["xyz"][j] - scr.world_point(seed, i) for j, i in enumerate(ids)}
        is3 = {i: bool(f["is_3d"][j]) or i in twins for j, i in enumerate(ids)}       # (is_3d stays monotone per id)
        yx = {}
        new = [i for i in ids if i not in seen]
        assert new == list(range(new[0], new[0] + len(new))) if new else True
        targets = []                                                            # older 3-D points the list does not carry, projecting well inside the image
        for t in sorted(known):
            if t in ids or k - last_seen[t] > window:
                continue
            p = project(T, known[t])
            if p is not None and 2.0 <= p[0] <= H - 1.0 and 2.0 <= p[1] <= W - 1.0:
                targets.append((t, p))
        for i in new:
            world[i] = scr.world_point(seed, i)
            rows[i] = random_row(seed, i)
            if k > 0 and targets and scr._u(seed, 64, i) < p_copy:
                t, p = targets[int(scr._u(seed, 65, i) * len(targets))]
                if scr._u(seed, 66, i) < p_twin:
                    world[i] = known[t] - err[i] + 1e-3 * np.array([scr._u(seed, 67, i), scr._u(seed, 68, i), scr._u(seed, 69, i)])
                    is3[i] = True; twins.add(i)
                    rows[i] = rows[t].copy()
                    yx[i] = project(T, world[i] + err[i])
                else:
                    rows[i] = flipped(rows[t], seed, i, int(scr._u(seed, 70, i) * 21))
                    yx[i] = p + 1.2 * np.array([scr._u(seed, 71, i) - 0.5, scr._u(seed, 72, i) - 0.5])
        for i in ids:
            if i in yx:
                continue
            p = project(T, world[i])
            if p is not None:
                p = p + 0.4 * np.array([scr._u(seed, 21, i, k) - 0.5, scr._u(seed, 22, i, k) - 0.5])
            if p is None or not (1.5 <= p[0] <= H - 0.5 and 1.5 <= p[1] <= W - 0.5):
                p = np.array([1.5 + (H - 2.0) * scr._u(seed, 73, i, k), 1.5 + (W - 2.0) * scr._u(seed, 74, i, k)])
            yx[i] = p
        xyz = np.array([world[i] + err[i] for i in ids]).reshape(-1, 3)
        out = dict(Tcw=T, ids=f["ids"].copy(), yx=np.ascontiguousarray(np.array([yx[i] for i in ids]).reshape(-1, 2)),
                   is_3d=np.array([is3[i] for i in ids], dtype=bool), xyz=np.ascontiguousarray(xyz))
        frames[k] = out
        for j, i in enumerate(ids):
            seen.add(i); last_seen[i] = k
            if is3[i]:
                known[i] = xyz[j].copy()
        descs.append((new[0] if new else (max(seen) + 1 if seen else 0), np.array([rows[i] for i in new], dtype=np.uint64).reshape(-1, 4)))
    return frames, descs


def scenes(seeds=SEEDS, sizes=SIZES, **kw):
    made = [make_scene(seed, sz, **kw) for seed, sz in zip(seeds, sizes)]
    return [m[0] for m in made], [m[1] for m in made]


class ModelRun:
    """The models of the S streams (np_kfmap.Map + descriptor dict each) driven through scenes(): add() consumes the next scripted key-frame of every
    selected stream, match() is the model's local-map match per stream, ba() a gather + update with the hashed stand-in solution (outliers, removed
    points).  replaced: how many entries changed owner while the old point had a descriptor."""

    def __init__(self, frames, descs, R=R, mcap=MCAP, cap=CAP, minc=4, seeds=SEEDS):
        import np_kfmap as npk
        import np_kfmap_local_map as nl
        self.npk, self.nl = npk, nl
        self.frames, self.descs, self.seeds = frames, descs, seeds
        self.n = len(frames)
        self.m = [npk.Map(cap, R, mcap, CAM10[:4], None, minc) for _ in range(self.n)]
        self.D = [nl.new_descriptors(m) for m in self.m]
        self.nkf = [0] * self.n
        self.sel = [True] * self.n
        self.replaced = 0

    def add(self, mask=None):
        self.sel = [True] * self.n if mask is None else [bool(v) for v in mask]
        took = {}
        for s in range(self.n):
            if self.sel[s]:
                f, d = self.frames[s][self.nkf[s]], self.descs[s][self.nkf[s]]
                before, had = self.m[s].ptag.copy(), self.D[s]["has"].copy()
                self.nl.add_keyframe(self.m[s], self.D[s], self.nkf[s], f["Tcw"], f)
                self.replaced += int(np.sum((before >= 0) & (before != self.m[s].ptag) & had))
                self.nl.add_descriptors(self.m[s], self.D[s], d[0], d[1])
                took[s] = (f, d)
                self.nkf[s] += 1
        return took

    def match(self, max_local=None, mutant=None):
        idle = self.nl.local_map_match(self.npk.Map(1, 2, 1), None, CAM10, CELL, PARAMS)         # an empty map: status 1, nothing staged
        return [self.nl.local_map_match(self.m[s], self.D[s], CAM10, CELL, PARAMS, max_local=max_local, mutant=mutant) if self.sel[s] else idle
                for s in range(self.n)]

    def ba(self):
        """-> {stream: (window, theta, outliers)} of the selected streams that have a window; applied to the models"""
        out = {}
        for s in range(self.n):
            if not self.sel[s]:
                continue
            win = self.npk.gather(self.m[s])
            if win is None:
                continue
            theta, outl = scr.refined(self.seeds[s], win), scr.outlier_pattern(self.seeds[s], win)
            self.npk.update(self.m[s], win, theta, outl)
            out[s] = (win, theta, outl)
        return out
