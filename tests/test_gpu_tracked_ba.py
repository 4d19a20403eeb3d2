"""GPU: local BA on windows gathered from tracked key-frames (tests/tracked_ba.py: _get_ba_parameters / _update_ba_parameters!,
src/estimator.jl:143-335) instead of the synthetic generators' geometry -- points with one observer, constant poses chosen by the
covisibility rules, observers outside the window, tracking and triangulation error.

Two map records per stream follow the same tracked run (benchlib.lockstep, pose loop): at every key-frame each gathers its window; the
HIP record solves the windows of all streams in one slam_local_ba_batch, the oracle record with the oracle's Schur-LM; each applies its
own result.  Bars are those of the other BA tests: outlier sets equal, iteration counts equal, costs 1e-8, theta 1e-6 (relative)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tracked_ba as tb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 4
RUNS = {"stereo": ("kitti05_1000", 6), "mono": ("euroc_mono", 6)}     # 2 + 6 key-frame periods of 5 frames: 40 frames, 8 key-frames


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max(initial=0.0) / max(1.0, float(np.abs(np.asarray(b)).max(initial=0.0))))


def _bars(tag, got_th, got_ol, got_st, ref_th, ref_ol, ref_st, theta_tol=1e-6):
    """the BA tests' bars -> list of misses"""
    miss = []
    if not np.array_equal(got_ol, ref_ol):
        miss.append(f"{tag}: outliers differ at {np.flatnonzero(got_ol != ref_ol)[:8].tolist()}")
    for k in ("iters_pass1", "iters_pass2"):
        if int(got_st[k]) != int(ref_st[k]):
            miss.append(f"{tag}: {k} {got_st[k]} vs {ref_st[k]}")
    for k in ("ssr_init", "ssr_pass1", "ssr_final"):
        if abs(got_st[k] - ref_st[k]) > 1e-8 * ref_st[k]:
            miss.append(f"{tag}: {k} {got_st[k]!r} vs {ref_st[k]!r}")
    if _rel(got_th, ref_th) > theta_tol:
        miss.append(f"{tag}: theta off by {_rel(got_th, ref_th):.3g} relative")
    return miss


def _cache(slam, w):
    return slam.LocalBACache(w["theta"].copy(), w["theta_const"], w["pixels"], w["poses_ids"], w["points_ids"])


def _compare_records(tag, rh, ro):
    th_h, x_h, ob_h, gone_h = tb.snapshot(rh)
    th_o, x_o, ob_o, gone_o = tb.snapshot(ro)
    if ob_h != ob_o or gone_h != gone_o:
        return [f"{tag}: observation sets differ after update"]
    miss = []
    for k in th_h:
        if _rel(th_h[k], th_o[k]) > 1e-6:
            miss.append(f"{tag}: key-frame {k} pose off by {_rel(th_h[k], th_o[k]):.3g}")
    xs = [k for k in x_h if _rel(x_h[k], x_o[k]) > 1e-6]
    if xs:
        miss.append(f"{tag}: {len(xs)} landmarks off by > 1e-6 (worst {max(_rel(x_h[k], x_o[k]) for k in xs):.3g})")
    return miss


_RUNS = {}


@pytest.fixture(scope="module", params=sorted(RUNS))
def tracked(request, slam, orc, syn):
    """the estimator chain of one run: every window (its arrays as gathered by the HIP record, the batch's result) and every bar missed"""
    mode = request.param
    if mode in _RUNS:
        return _RUNS[mode]
    name, periods = RUNS[mode]
    rec_h, rec_o = [], []
    out = dict(mode=mode, windows=[], misses=[], steps=0)

    def on_kf(kfid, Tcw, lists, camt):
        if not rec_h:
            rec_h.extend(tb.Record(camt, min_cov_score=c, mismatch=f) for c, f in tb.STREAM_CFG)
            rec_o.extend(tb.Record(camt, min_cov_score=c, mismatch=f) for c, f in tb.STREAM_CFG)
        for s in range(S):
            tb.add_keyframe(rec_h[s], kfid, Tcw[s], lists[s]); tb.add_keyframe(rec_o[s], kfid, Tcw[s], lists[s])
        empty = lambda w: w is None or len(w["poses_ids"]) == 0                # (the first key-frame: its one pose is constant, nothing to solve)
        wh = [None if empty(w) else w for w in (tb.gather(r) for r in rec_h)]
        wo = [None if empty(w) else w for w in (tb.gather(r) for r in rec_o)]
        idx = [s for s in range(S) if wh[s] is not None]
        if [w is None for w in wo] != [w is None for w in wh]:
            out["misses"].append(f"kf {kfid}: the records disagree on which streams run a BA")
            return
        if not idx:
            return
        caches = [_cache(slam, wh[s]) for s in idx]
        status = slam.bundle_adjustment_batch_(caches, [camt] * len(idx))
        out["steps"] += 1
        for s, c, st in zip(idx, caches, status):
            w, v, tag = wh[s], wo[s], f"{mode} kf {kfid} stream {s}"
            if st:
                out["misses"].append(f"{tag}: status {st}"); continue
            args = (w["theta_const"], w["pixels"], w["poses_ids"], w["points_ids"], 5, 10, 5.0)
            th, ol, sto = orc.bundle_adjustment(camt, w["theta"], *args, solver=1)
            out["misses"] += _bars(tag + " (HIP vs oracle, same window)", c.theta, c.outliers, c.stats, th, ol, sto)
            if not all(np.array_equal(w[k], v[k]) for k in ("theta_const", "pixels", "poses_ids", "points_ids", "obs_kf", "obs_kp")):
                out["misses"].append(f"{tag}: the records gathered different windows"); continue
            tho, olo, stoo = orc.bundle_adjustment(camt, v["theta"], v["theta_const"], v["pixels"], v["poses_ids"], v["points_ids"], 5, 10, 5.0, solver=1)
            out["misses"] += _bars(tag + " (HIP record vs oracle record)", c.theta, c.outliers, c.stats, tho, olo, stoo)
            out["windows"].append(dict(tag=tag, kfid=kfid, s=s, covmap=dict(w["covmap"]), cam=np.asarray(camt, dtype=np.float64), win=w, theta=c.theta.copy(),
                                       outliers=c.outliers.copy(), stats=dict(c.stats), hb=slam.ba_plan_order(c)[1]))
            tb.update(rec_h[s], w, c.theta, c.outliers)
            tb.update(rec_o[s], v, tho, olo)
            out["misses"] += _compare_records(tag, rec_h[s], rec_o[s])

    tb.run_tracked(slam, syn, name, S, periods, on_kf)
    _RUNS[mode] = out
    for d in out["windows"]:
        st = tb.structure(d["win"])
        print(f"TRACKED {d['tag']}: P {st['P']} (free {st['free']}) M {st['M']} O {st['O']} single-observer {st['single_free']} "
              f"constant-only {st['const_only']} constant-not-0 {st['const_not0']} outliers {int(d['outliers'].sum())} hb {d['hb']} "
              f"iters {d['stats']['iters_pass1']}+{d['stats']['iters_pass2']} covisibility {d['covmap']}")
    return out


def test_tracked_windows_hip_chain_equals_oracle_chain(tracked):
    assert tracked["steps"] >= 7, tracked["steps"]
    assert not tracked["misses"], "\n".join(tracked["misses"][:40])


def test_tracked_windows_exercise_the_structure(tracked):
    """the run must produce what the generators never do -- else the chain above proves little"""
    st = [tb.structure(d["win"]) for d in tracked["windows"]]
    n_out = sum(int(d["outliers"].sum()) for d in tracked["windows"])
    print(f"TRACKED {tracked['mode']}: {len(st)} windows, P {min(s['P'] for s in st)}..{max(s['P'] for s in st)}, "
          f"M {min(s['M'] for s in st)}..{max(s['M'] for s in st)}, O {min(s['O'] for s in st)}..{max(s['O'] for s in st)}, "
          f"single-observer points {sum(s['single_free'] for s in st)}, constant-only points {sum(s['const_only'] for s in st)}, "
          f"outliers {n_out}")
    if tracked["mode"] == "stereo":              # (a monocular point is triangulated from two key-frames: it never has one observer)
        assert sum(s["single_free"] for s in st) > 0, "no single-observation point of a free pose"
    assert sum(s["const_only"] for s in st) > 0, "no point seen by constant poses only"
    assert sum(s["const_not0"] for s in st) > 0, "no constant pose other than key-frame 0"
    assert n_out > 0, "no flagged outlier"


def test_tracked_windows_batch_equals_single_calls(slam, tracked):
    misses = []
    for d in tracked["windows"]:
        c = _cache(slam, d["win"])
        slam.bundle_adjustment_(c, d["cam"])
        misses += _bars(d["tag"] + " (batch vs single)", d["theta"], d["outliers"], d["stats"], c.theta, c.outliers, c.stats)
    assert not misses, "\n".join(misses[:40])


_ALT = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r)
import slam_jl_amd as slam
z = np.load(%(src)r)
res = []
for g in range(int(z["ngroups"])):
    ks = [int(k) for k in z["group%%d" %% g]]
    caches = [slam.LocalBACache(z["theta%%d" %% k].copy(), z["tc%%d" %% k], z["px%%d" %% k], z["pi%%d" %% k], z["li%%d" %% k]) for k in ks]
    b = slam.BABatch(caches, [z["cam%%d" %% k] for k in ks]); b.solve()
    assert not b.status.any(), b.status
    res += [b.theta.ravel(), b.outl[:int(b.On.sum())].astype(np.float64), b.stats[:, :6].ravel()]
np.save(%(out)r, np.concatenate(res))
print("OK")
'''


def test_tracked_windows_library_alternatives_agree(tracked, tmp_path):
    """the same key-frame batches solved again in child processes: the default build, the vector Schur kernel (SLAMHIP_BA_NO_MFMA=1) and
    k_ba_window on one workgroup (SLAMHIP_BA_WINDOW_ONE=1) -- outliers equal, everything else to 1e-9 relative"""
    src = str(tmp_path / "windows.npz")
    arr, groups = {}, {}
    for k, d in enumerate(tracked["windows"]):
        w = d["win"]
        arr.update({f"theta{k}": w["theta"], f"tc{k}": w["theta_const"], f"px{k}": w["pixels"], f"pi{k}": w["poses_ids"],
                    f"li{k}": w["points_ids"], f"cam{k}": d["cam"]})
        groups.setdefault(d["kfid"], []).append(k)
    for g, kf in enumerate(sorted(groups)):
        arr[f"group{g}"] = np.array(groups[kf])
    np.savez(src, ngroups=len(groups), **arr)
    res = {}
    for tag, env in (("default", {}), ("vector", {"SLAMHIP_BA_NO_MFMA": "1"}), ("one", {"SLAMHIP_BA_WINDOW_ONE": "1"})):
        out = str(tmp_path / (tag + ".npy"))
        r = subprocess.run([sys.executable, "-c", _ALT % dict(root=ROOT, src=src, out=out)], env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), tag + ": " + r.stdout[-800:] + r.stderr[-1500:]
        res[tag] = np.load(out)
    # the outlier flags sit between theta and the stats of every group: compare them exactly, all of it to 1e-9
    a = res["default"]
    for tag in ("vector", "one"):
        b = res[tag]
        assert a.shape == b.shape, tag
        rel = np.abs(a - b) / np.maximum(1.0, np.abs(a))
        assert rel.max() <= 1e-9, (tag, rel.max())
    off = 0
    for g, kf in enumerate(sorted(groups)):
        ks = groups[kf]
        nth = sum(len(tracked["windows"][k]["win"]["theta"]) for k in ks)
        no = sum(len(tracked["windows"][k]["win"]["poses_ids"]) for k in ks)
        for tag in ("vector", "one"):
            assert np.array_equal(a[off + nth:off + nth + no], res[tag][off + nth:off + nth + no]), (tag, kf)
        off += nth + no + 6 * len(ks)
    assert off == len(a)
