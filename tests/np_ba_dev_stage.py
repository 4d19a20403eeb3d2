"""numpy restatement of slam_local_ba_batch_dev's probe and stager, written from the layout description (include/slamhip.h), and the window
set the host-level test (test_ba_dev_plan_host.py) and the GPU test (test_gpu_ba_batch_dev.py) share.

A window: P poses, M points, O observations; theta = [6P ; 3M], theta_const (P), pixels (O, 2) as (y, x), pose_ids / point_ids (O, 1-based), the
observations grouped by point in ascending point id.

probe    free poses, the largest per-point observation count, the observations of free poses, the two checks (grouping, a point twice by one free pose)
eligible the one-workgroup kernel takes the window: 1 .. 5 free poses that are the whole free span AFTER relabelling (so a single free pose only where
         it is the only pose -- and such a window the batch does not take either: at least two poses in the span), P <= 128, 1 <= O <= 40000, M >= 1,
         at most 168 observations of one point
relabel  constant poses first, then the free ones, each in the caller's order: order[k] = caller's pose at solver position k
stage    pose / pconst in solver order; pts, pt_id = identity; opose = label of the pose, opoint = opk = point index; pix all y then all x;
         pt_start = first observation of a point (M + 1 entries); pfs = observations of free poses of the points before (M + 1); fobs = the
         observations of free poses, in order; fgrp = zeros (P + 1); ksplit = the cost split
ksplit   total = 2 O + 13 pfs[M]; the first point k with 2 (2 pt_start[k] + 13 pfs[k]) >= total, clamped to [1, M - 1]; a one-point window keeps the
         split by observation counts: the first k of pt_start[0 .. M] with pt_start[k] >= (O + 1) // 2
"""
import numpy as np

FMAX, PMAX, OMAX, CMAX = 5, 128, 40000, 168


def probe(P, M, O, tc, pose_ids, point_ids):
    tc = np.asarray(tc).astype(bool)
    pi, li = np.asarray(pose_ids, dtype=np.int64), np.asarray(point_ids, dtype=np.int64)
    out = dict(nfree=int((~tc).sum()), cmax=0, nfree_obs=0, ungrouped=False, twice=False)
    if O == 0:
        return out
    if (pi < 1).any() or (pi > P).any() or (li < 1).any() or (li > M).any() or (np.diff(li) < 0).any():
        out["ungrouped"] = True
        return out
    out["cmax"] = int(np.bincount(li, minlength=M + 1).max())
    free = ~tc[pi - 1]
    out["nfree_obs"] = int(free.sum())
    pairs = np.stack([li[free], pi[free]], 1)
    out["twice"] = len(np.unique(pairs, axis=0)) != len(pairs)
    return out


def free_span_relabelled(P, nfree, mutant=None):
    """(p0, span) of the free poses once they are the last labels; fewer than two free poses span every pose"""
    if nfree >= 2 or (mutant == "admit_one_free" and nfree >= 1):
        return P - nfree, nfree
    return 0, P


def window_rule(pr, P, M, O, mutant=None):
    """the planner's rule for the one-workgroup kernel (it admits a window of ONE pose, which the batch then does not take: eligible())"""
    p0, span = free_span_relabelled(P, pr["nfree"], mutant)
    return bool(M >= 1 and O >= 1 and 1 <= pr["nfree"] <= FMAX and pr["nfree"] == span and P <= PMAX and O <= OMAX and pr["cmax"] <= CMAX)


def eligible(pr, P, M, O, mutant=None):
    return window_rule(pr, P, M, O, mutant) and (free_span_relabelled(P, pr["nfree"], mutant)[1] >= 2 or mutant == "admit_one_free")


def relabel(tc, mutant=None):
    """-> (order, label): order[k] = caller's pose at solver position k, label[p] = solver position of caller's pose p"""
    tc = np.asarray(tc).astype(bool)
    P = len(tc)
    order = np.arange(P) if mutant == "not_consecutive" else np.concatenate([np.flatnonzero(tc), np.flatnonzero(~tc)])
    label = np.empty(P, dtype=np.int64); label[order] = np.arange(P)
    return order, label


def ksplit(M, O, pt_start, pfs, mutant=None):
    half = (O + 1) // 2
    by_obs = min(int(np.searchsorted(pt_start, half, side="left")), M)
    if M <= 1:
        return by_obs
    if mutant == "ksplit_obs_only":
        return min(max(by_obs, 1), M - 1)
    total = 2 * O + 13 * int(pfs[M])
    cost = 2 * (2 * pt_start[:M].astype(np.int64) + 13 * pfs[:M].astype(np.int64))
    kk = int(np.argmax(cost >= total)) if (cost >= total).any() else M
    return min(max(kk, 1), M - 1)


def stage(P, M, O, theta, tc, pixels, pose_ids, point_ids, mutant=None):
    theta = np.asarray(theta, dtype=np.float64); tc = np.asarray(tc, dtype=np.uint8)
    px = np.asarray(pixels, dtype=np.float64).reshape(-1, 2)
    pi, li = np.asarray(pose_ids, dtype=np.int64), np.asarray(point_ids, dtype=np.int64)
    order, label = relabel(tc, mutant)
    nfree = int((tc == 0).sum())
    opose = label[pi - 1].astype(np.int32)
    opoint = (li - 1).astype(np.int32)
    cnt = np.bincount(li - 1, minlength=M)
    pt_start = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    free_obs = tc[pi - 1] == 0
    fcnt = np.bincount(li[free_obs] - 1, minlength=M)
    pfs = np.concatenate([[0], np.cumsum(fcnt)]).astype(np.int32)
    if mutant == "pfs_off_by_one":
        pfs = np.concatenate([[0], pfs[:-1]]).astype(np.int32)
    p0, nb = free_span_relabelled(P, nfree)
    return dict(pose=theta[:6 * P].reshape(P, 6)[order].ravel().copy(), pts=theta[6 * P:].copy(), pconst=tc[order].copy(),
                pix=np.concatenate([px[:, 0], px[:, 1]]), opose=opose, opoint=opoint, pt_start=pt_start, pt_id=np.arange(M, dtype=np.int32),
                opk=opoint.copy(), pfs=pfs, fobs=np.flatnonzero(free_obs).astype(np.int32), fgrp=np.zeros(P + 1, dtype=np.int32),
                ksplit=ksplit(M, O, pt_start, pfs, mutant), p0=p0, nb=nb, order=order, label=label)


def unstage(st):
    """the window the staged arrays describe, in the caller's form: (theta, theta_const, pixels, pose_ids, point_ids) -- the permutations inverted"""
    P, M, O = len(st["pconst"]), len(st["pt_id"]), len(st["opose"])
    pose = np.empty((P, 6)); pose[st["order"]] = st["pose"].reshape(P, 6)
    tc = np.empty(P, dtype=np.uint8); tc[st["order"]] = st["pconst"]
    pts = np.empty((M, 3)); pts[st["pt_id"]] = st["pts"].reshape(M, 3)[np.arange(M)]
    theta = np.concatenate([pose.ravel(), pts.ravel()])
    px = np.stack([st["pix"][:O], st["pix"][O:]], 1)
    return theta, tc, px, st["order"][st["opose"]].astype(np.int64) + 1, st["opoint"].astype(np.int64) + 1


def check_staged(win, st):
    """the assertions both levels make of a set of staged arrays (a mutant of the model must fail one of them)"""
    P, M, O = win["P"], win["M"], win["O"]
    tc = np.asarray(win["theta_const"], dtype=np.uint8)
    nfree = int((tc == 0).sum())
    # the free poses are the last nfree labels: the kernel addresses free pose a as p0 + a
    assert st["p0"] == P - nfree and st["nb"] == nfree
    assert not st["pconst"][st["p0"]:].any() and st["pconst"][:st["p0"]].all()
    th, tc2, px, pi, li = unstage(st)
    assert np.array_equal(th, win["theta0"]) and np.array_equal(tc2, tc) and np.array_equal(px, win["pixels_yx"])
    assert np.array_equal(pi, win["pose_ids"]) and np.array_equal(li, win["point_ids"])
    # pt_start / pfs / fobs against a plain walk over the observations
    free = st["pconst"][st["opose"]] == 0
    assert st["pt_start"][0] == 0 and st["pt_start"][M] == O and st["pfs"][0] == 0
    for k in range(M):
        a, b = st["pt_start"][k], st["pt_start"][k + 1]
        assert (st["opk"][a:b] == k).all()
        assert st["pfs"][k + 1] - st["pfs"][k] == free[a:b].sum()
        assert np.array_equal(st["fobs"][st["pfs"][k]:st["pfs"][k + 1]], a + np.flatnonzero(free[a:b]))
    # ksplit: a plain walk of the costs
    if M > 1:
        total = 2 * O + 13 * int(free.sum())
        kk = 0
        while kk < M and 2 * (2 * int(st["pt_start"][kk]) + 13 * int(free[:st["pt_start"][kk]].sum())) < total:
            kk += 1
        assert st["ksplit"] == min(max(kk, 1), M - 1)
    assert not st["fgrp"].any()


def _scene(syn, P, M, seed, tc, k=10, drop_points=(), n_gross=None, noise=0.3, gross=(20.0, 35.0)):
    """a synthetic window (<= 0.5 px noise, no random outliers) with scripted gross outliers of >= 20 px; observations of `drop_points` removed.  A gross
    outlier of g px drags its point until the point's k - 1 other observations carry about g / k px each: g is chosen so that g / k stays clear of
    sqrt(repr_eps) = 2.2 px (k = 10: 60 .. 90 px)"""
    # (a start close enough for the five fast iterations to reach the noise floor: squared residuals of ~0.2 or of >= 400, none near repr_eps)
    s = syn.ba_scene(P=P, M=M, obs_per_point=k, seed=seed, noise_px=noise, outlier_frac=0.0, n_const=1, perturb=(2e-4, 2e-3, 5e-3))
    s["theta_const"] = np.asarray(tc, dtype=np.uint8)
    keep = ~np.isin(s["point_ids"], np.asarray(drop_points, dtype=np.int64) + 1)
    for key in ("pose_ids", "point_ids"):
        s[key] = s[key][keep]
    s["pixels_yx"] = np.ascontiguousarray(s["pixels_yx"][keep]); s["O"] = int(keep.sum())
    rng = np.random.default_rng(0xD0 + seed)
    n_gross = max(1, s["O"] // 60) if n_gross is None else n_gross
    idx = rng.choice(s["O"], min(n_gross, s["O"]), replace=False)
    ang = rng.uniform(0, 2 * np.pi, len(idx)); mag = rng.uniform(gross[0], gross[1], len(idx))
    s["pixels_yx"][idx, 0] += mag * np.sin(ang); s["pixels_yx"][idx, 1] += mag * np.cos(ang)
    s["gross_outliers"] = np.sort(idx)
    return s


def _const(P, free):
    tc = np.ones(P, dtype=np.uint8); tc[list(free)] = 0
    return tc


def window_set(syn):
    """six windows the one-workgroup kernel takes: one map point; 280 points (the scans cross a 256-point chunk) with the free poses scattered among the
    caller's pose ids; exactly five free poses of 25 with most points seen by constant poses only; points without any observation and two free poses;
    free poses consecutive in the MIDDLE of the caller's order; 300 points, three free poses of 25"""
    return [
        _scene(syn, 3, 1, 11, _const(3, (1, 2)), k=3, n_gross=0),
        _scene(syn, 8, 280, 12, _const(8, (1, 4, 6)), k=5),
        _scene(syn, 25, 200, 13, _const(25, range(20, 25)), gross=(60.0, 90.0)),
        _scene(syn, 6, 90, 14, _const(6, (4, 5)), k=4, drop_points=(0, 17, 18, 89)),
        _scene(syn, 10, 150, 15, _const(10, (3, 4, 5)), k=6),
        _scene(syn, 25, 300, 16, _const(25, (22, 23, 24)), gross=(60.0, 90.0)),
    ]


def ineligible_set(syn):
    """one free pose among several; six free poses; no observations -- and one window the kernel takes, alone in its list"""
    empty = _scene(syn, 2, 3, 23, _const(2, (1,)), k=2, n_gross=0)
    empty.update(pose_ids=np.zeros(0, dtype=np.int64), point_ids=np.zeros(0, dtype=np.int64), pixels_yx=np.zeros((0, 2)), O=0, gross_outliers=np.zeros(0, dtype=int))
    return [
        _scene(syn, 5, 60, 21, _const(5, (4,)), k=4),
        _scene(syn, 10, 120, 22, _const(10, range(4, 10)), k=6),
        _scene(syn, 8, 100, 24, _const(8, (5, 6, 7)), k=5),
        empty,
    ]
