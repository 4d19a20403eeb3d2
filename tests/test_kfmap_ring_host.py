"""CPU: csrc/kfmap_ring.hpp -- the key-frame map's integer logic, the serial sections one thread of k_kfm_plan, k_kfm_filter, the local-map stager and
k_kfm_merge_resolve runs -- and Layout::bind (csrc/layout.hpp) as a stand-alone host program (tests/c_host/kfmap_ring_check.cpp), built plain and with
-fsanitize=address,undefined (the program alone; nothing is loaded into Python).  The expected values come from the numpy models the GPU tests hold
the kernels to, not from the header: np_kfmap's covmap / ascending / meet / window_const (gather's co, asc, order, theta_const),
np_kfmap_filter's ascending_ids / walked / _decide, np_kfmap_local_map_history's oldest / rule, np_kfmap_merge.check_pairs.

Ring states: R in {2, 3, 32, 63, 64} (2: the smallest ring; 63 / 64: the last bits of the 64-bit masks), each with empty slots, key-frame 0 present and
absent, the newest key-frame in slot 0 and in slot R - 1, zero / one / five / more than five covisible slots as far as R - 1 other slots allow, scores
equal to, just below and just above min_cov_score, a tag above the newest id (passed over by the filter), and 64 random states."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_kfmap as npk  # noqa: E402
import np_kfmap_filter as npf  # noqa: E402
import np_kfmap_local_map_history as nph  # noqa: E402
import np_kfmap_merge as npm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "kfmap_ring_check.cpp")
INC = os.path.join(ROOT, "slam.jl_amd", "csrc")
FLAGS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
RS = (2, 3, 32, 63, 64)
MINC = 8
COUNTS = [0, 1, 31, 32, 33, 255, 256, 257]          # tests/test_pose_records_host.py's
SIZES = [1, 4, 8, 16, 24]


def _state(R, K, present, scores, nb3=MINC, minc=MINC):
    """a ring whose newest key-frame is K: `present` older (or, synthetic, newer) key-frame ids, scores: id -> shared points.  Model form: tag -1 = empty"""
    tag = np.full(R, -1, dtype=np.int64)
    for k in [K] + list(present):
        assert tag[k % R] == -1, (R, K, present)
        tag[k % R] = k
    cov = {k % R: int(v) for k, v in scores.items() if v > 0}
    assert all(tag[b] >= 0 for b in cov) and K % R not in cov
    return dict(R=R, K=K, tag=tag, cov=cov, nb3=nb3, minc=minc)


def ring_states(R):
    out = []
    older = lambda K: [k for k in range(max(K - R + 1, 0), K)]
    for K in (0, R - 1, R, 2 * R - 1, 5 * R, 5 * R + R - 1, 3 * R + 1):        # r0 = 0 and R - 1, with key-frame 0 (K < R) and without
        ks = older(K)
        for ncov in (0, 1, 5, 6, R - 1):                                        # zero, one, five, more than five covisible slots (as far as R allows)
            if ncov > len(ks):
                continue
            for pick in (ks[:ncov], ks[len(ks) - ncov:]):                       # the oldest (key-frame 0 among them when present) / the newest
                sc = {k: (MINC - 1, MINC, MINC + 1)[(j + len(out) // 2) % 3] for j, k in enumerate(pick)}       # just below, equal to, just above min_cov_score
                out.append(_state(R, K, ks, sc))
                out.append(_state(R, K, ks[1::2] + [k for k in pick if k not in ks[1::2]], sc, nb3=MINC + 3))      # with empty slots
        if R > 2 and K >= R:
            out.append(_state(R, K, ks[1:] + [K + 1], {K + 1: MINC, ks[1]: MINC + 1}))      # a tag above the newest id
    rng = np.random.default_rng(1000 + R)
    for _ in range(64):
        K = int(rng.integers(0, 4 * R))
        ks = [k for k in older(K) if rng.random() < 0.8]
        sc = {k: int(rng.integers(0, 2 * MINC)) for k in ks if rng.random() < (0.3 if rng.random() < 0.5 else 0.9)}
        out.append(_state(R, K, ks, sc, nb3=int(rng.integers(MINC, 3 * MINC)), minc=int(rng.integers(1, 2 * MINC))))
    return out


def ring_line(st):
    R, tag = st["R"], st["tag"]
    cov = [st["cov"].get(b, 0) for b in range(R)]
    cov[st["K"] % R] = st["nb3"]                                                # (as k_kfm_plan sets it before the pick)
    return "ring %d %d %d %d " % (R, st["K"] % R, st["K"], st["minc"]) + " ".join(str(int(t) + 1) for t in tag) + " " + " ".join(map(str, cov))


def ring_expected(st):
    """the program's line for a state, from the models"""
    R, K, tag, minc = st["R"], st["K"], st["tag"], st["minc"]
    r0 = K % R
    cov = dict(st["cov"]); cov[r0] = st["nb3"]                                  # np_kfmap.gather: cov[r0] = nb3
    co, asc = npk.covmap(tag, cov), npk.ascending(tag)
    rank = [-1] * R
    for k, b in enumerate(asc):
        rank[b] = k
    wconst = [int(npk.window_const(tag[b], b in co, cov.get(b, 0), minc)) if tag[b] >= 0 else None for b in range(R)]
    kfids, _ = npf.walked(npf.ascending_ids(tag, st["cov"].keys()), K)
    return dict(nv=len(asc), rank=rank, asc=asc, cl=co, mask=sum(1 << b for b in co), wconst=wconst, cand=[k % R for k in kfids],
                valid=sum(1 << b for b in range(R) if tag[b] >= 0))


def parse_ring(line, R):
    parts = [[int(t) for t in p.split()] for p in line.split("|")]
    nv = parts[0][0]
    return dict(nv=nv, rank=parts[0][1:1 + R], asc=parts[0][1 + R:], cl=parts[1][1:1 + parts[1][0]], mask=parts[1][-1], wconst=parts[2],
                cand=parts[3][1:1 + parts[3][0]], valid=parts[3][-1])


def poses_cases():
    """(R, P, order, first) + the model's result: np_kfmap.meet over the slots in the order of their first observation"""
    rng = np.random.default_rng(7)
    out = []
    for R in RS:
        for _ in range(16):
            have = [b for b in range(R) if rng.random() < 0.3]
            rng.shuffle(have)
            order = {int(b): k + 1 for k, b in enumerate(have)}
            met = [b for b in range(R) if b not in order and rng.random() < 0.5]
            first = dict(zip(met, rng.permutation(10 * R)[:len(met)]))
            want = dict(order)
            for b in sorted(met, key=lambda b: first[b]):
                npk.meet(want, b)
            out.append((R, len(order), [order.get(b, 0) for b in range(R)], [int(first.get(b, -1)) for b in range(R)], [want.get(b, 0) for b in range(R)]))
    return out


def decide_cases():
    out = [(0, 0, 0, 0.5), (0, 0, 1, 0.5), (0, 0, 3, 0.0)]                      # n_total = 0: 0 / 0 is NaN, kept unless `few` catches it
    for minc in (8, 9, 1, 0):
        few = minc // 2
        for n_total in (few - 1, few, few + 1):
            if n_total >= 0:
                out += [(n_total, 0, minc, 0.5), (n_total, n_total, minc, 0.5)]
    for n_total, n_good in ((2, 1), (10, 5), (3, 1), (7, 7), (64, 63)):
        q = float(np.float64(n_good) / np.float64(n_total))
        out += [(n_total, n_good, 2, r) for r in (q, math.nextafter(q, 0.0), math.nextafter(q, 2.0), 0.0, 0.999)]
    return out


def hist_cases():
    """(C, P, covmask, linked, max_local): 2 |C| = |P| and +- 1, |L| = max_local and max_local - 1, no covisible key-frame, unlinked"""
    out = []
    for nP in (0, 1, 6, 7):
        for nC in sorted({0, nP // 2, max((nP - 1) // 2, 0), (nP + 1) // 2, nP // 2 + 1, nP + 2}):
            for shared in sorted({0, min(nC, nP) // 2, min(nC, nP)}):
                C = set(range(nC)); P = set(range(nC - shared, nC - shared + nP))
                for size in {len(C), len(P | C)}:
                    for max_local in (size, size + 1, size - 1 if size else 1, 1 << 20):
                        for covmask, linked in ((0, 1), (0, 0), (1 << 63, 1), (1 << 63 | 5, 0), (2, 1)):
                            out.append((C, P, covmask, linked, max_local))
    return out


def pairs_cases():
    out = [[], [(3, 3)], [(3, 3), (4, 5)], [(1, 2), (3, 4)], [(1, 2), (1, 4)], [(1, 2), (3, 2)], [(1, 2), (2, 3)], [(1, 2), (3, 1)],
           [(3, 3), (3, 4)], [(3, 3), (4, 3)], [(3, 3), (3, 3)], [(1, 2), (2, 1)], [(2 ** 62, 5), (7, 2 ** 62)], [(0, 1), (2, 3), (4, 5), (6, 0)]]
    rng = np.random.default_rng(11)
    for _ in range(200):
        n = int(rng.integers(1, 7))
        out.append([(int(a), int(b)) for a, b in rng.integers(0, int(rng.choice([6, 12, 40])), size=(n, 2))])
    return out


def search_cases():
    out = []
    for n in (0, 1, 2, 63, 64, 65):
        ids = [10 + 10 * i for i in range(n)]
        qs = [0, 9, 10 * n + 11, 2 ** 62] + [v for i in (0, 1, n // 2, n - 2, n - 1) if 0 <= i < n for v in (ids[i] - 1, ids[i], ids[i] + 1)]
        out += [(q, ids) for q in qs]
    return out


ENTRY = [(i, m) for m in (1, 100, 128, 130) for i in (0, m - 1, m, 2 ** 62, -1)]
STATES = {R: ring_states(R) for R in RS}
POSES, DECIDE, HIST, PAIRS, SEARCH = poses_cases(), decide_cases(), hist_cases(), pairs_cases(), search_cases()
BIND = {"by_size": [(s, c) for s in SIZES for c in COUNTS], "by_count": [(s, c) for c in COUNTS for s in SIZES]}


@pytest.fixture(scope="module", params=list(FLAGS), ids=list(FLAGS))
def replay(request, tmp_path_factory):
    """One build and one run per flag set: {case: the program's line}."""
    exe = str(tmp_path_factory.mktemp("kfmap_ring_" + request.param) / "kfmap_ring_check")
    cxx = os.environ.get("CXX", "c++")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", INC] + FLAGS[request.param] + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    keys, lines = [], []

    def put(key, line):
        keys.append(key); lines.append(line)
    for R in RS:
        for k, st in enumerate(STATES[R]):
            put(("ring", R, k), ring_line(st))
    for k, (R, P, order, first, _) in enumerate(POSES):
        put(("poses", k), "poses %d %d " % (R, P) + " ".join(map(str, order)) + " " + " ".join(map(str, first)))
    for k, (nt, ng, minc, ratio) in enumerate(DECIDE):
        put(("decide", k), "decide %d %d %d %s" % (nt, ng, minc // 2, float(ratio).hex()))
    for k, (C, P, covmask, linked, max_local) in enumerate(HIST):
        put(("hist", k), "hist %d %d %d %d %d %d" % (len(C), len(P), len(P | C), covmask, linked, max_local))
    for R in RS:
        for k, st in enumerate(STATES[R]):
            if st["cov"]:
                put(("oldest", R, k), "oldest %d " % sum(1 << b for b in st["cov"]) + " ".join(str(int(st["tag"][b]) + 1 if b < R else 0) for b in range(64)))
    for k, pr in enumerate(PAIRS):
        put(("pairs", k), "pairs %d " % len(pr) + " ".join("%d %d" % p for p in pr))
    for k, (q, ids) in enumerate(SEARCH):
        put(("search", k), "search %d %d " % (q, len(ids)) + " ".join(map(str, ids)))
    for k, (i, m) in enumerate(ENTRY):
        put(("entry", k), "entry %d %d" % (i, m))
    for order, prs in BIND.items():
        put(("bind", order), "bind " + " ".join("%d %d" % p for p in prs))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.strip("\n").split("\n")
    assert len(out) == len(keys)
    return dict(zip(keys, out))


def test_the_states_cover_what_they_claim():
    """the generators are worth their rows (no program needed): per R every required kind of ring state occurs"""
    for R in RS:
        sts = STATES[R]
        ncov = {len(s["cov"]) for s in sts}
        assert {0, 1} <= ncov and (R < 7 or {5} <= ncov and max(ncov) > 5) and max(ncov) >= min(R - 1, 6)
        assert any((s["tag"] < 0).any() for s in sts) and any((s["tag"] == 0).any() for s in sts) and any(not (s["tag"] == 0).any() for s in sts)
        assert {s["K"] % R for s in sts} >= {0, R - 1}
        assert any((s["tag"] == 0).any() and s["tag"][0] == 0 and s["cov"].get(0) for s in sts)          # key-frame 0 covisible: the walk breaks
        sc = {v - s["minc"] for s in sts for v in s["cov"].values()}
        assert {-1, 0, 1} <= sc
        if R > 2:
            assert any(s["tag"].max() > s["K"] for s in sts)
        if R >= 63:
            assert any(s["K"] % R == R - 1 and s["cov"] for s in sts) and any(R - 1 in s["cov"] for s in sts)      # the top bit as newest and as covisible slot
        assert len(sts) >= 64 + 10
    assert any(broke for R in RS for s in STATES[R] for _, broke in [npf.walked(npf.ascending_ids(s["tag"], s["cov"].keys()), s["K"])])


@pytest.mark.parametrize("R", RS)
def test_ring_decisions_equal_the_models(replay, R):
    for k, st in enumerate(STATES[R]):
        got, want = parse_ring(replay[("ring", R, k)], R), ring_expected(st)
        for key in ("nv", "asc", "cl", "mask", "cand", "valid"):
            assert got[key] == want[key], (R, k, key, got[key], want[key], st)
        for b in range(R):
            if st["tag"][b] >= 0:
                assert got["rank"][b] == want["rank"][b] and got["wconst"][b] == want["wconst"][b], (R, k, b, st)
        if st["cov"]:
            assert int(replay[("oldest", R, k)]) == nph.oldest(st["cov"].keys(), st["tag"]), (R, k)


def test_pose_ids_in_first_encounter_order(replay):
    for k, (R, P, order, first, want) in enumerate(POSES):
        v = [int(t) for t in replay[("poses", k)].split()]
        assert v[0] == max(want) if any(want) else v[0] == 0
        assert v[1:] == want, (k, R, order, first)


def test_filter_decision(replay):
    seen = set()
    for k, (nt, ng, minc, ratio) in enumerate(DECIDE):
        want = npf._decide(nt, ng, ratio, minc)
        seen.add((want, nt == 0))
        assert int(replay[("decide", k)]) == (want != "keep"), (nt, ng, minc, ratio, want)
    assert {("keep", True), ("few", True), ("keep", False), ("few", False), ("ratio", False)} <= seen


def test_history_rule(replay):
    seen = set()
    for k, (C, P, covmask, linked, max_local) in enumerate(HIST):
        replace, L, chain = nph.rule(C, P, covmask != 0, linked, max_local)
        seen.add((replace, chain, 2 * len(C) - len(P) if abs(2 * len(C) - len(P)) <= 1 else None, max_local - len(L) if 0 <= max_local - len(L) <= 1 else None))
        assert [int(t) for t in replay[("hist", k)].split()] == [int(replace), int(chain), len(L)], (k, C, P, covmask, linked, max_local)
    assert {d for _, _, d, _ in seen} >= {-1, 0, 1} and {m for _, _, _, m in seen} >= {0, 1} and {(r, c) for r, c, _, _ in seen} == {(a, b) for a in (False, True) for b in (False, True)}


def test_pairs_one_to_one(replay):
    verdicts = set()
    for k, pr in enumerate(PAIRS):
        v = [int(t) for t in replay[("pairs", k)].split()]
        want = npm.check_pairs(np.array(pr, dtype=np.int64).reshape(-1, 2))
        verdicts.add(want)
        assert v[0] == int(want) and v[1] == int(want), (pr, v)                 # the device's form and the host's refuse exactly the same inputs
        assert len(v) == 2 + len(pr) and any(v[2:]) == (not want)
    assert verdicts == {True, False}
    for k, kind in ((4, "prev twice"), (5, "new twice"), (6, "an id on both sides"), (7, "an id on both sides")):
        assert replay[("pairs", k)].split()[:2] == ["0", "0"], kind
    assert replay[("pairs", 1)].split()[:2] == ["1", "1"] and replay[("pairs", 2)].split()[:2] == ["1", "1"]        # the pair of one id is not refused


def test_search_and_entry(replay):
    for k, (q, ids) in enumerate(SEARCH):
        lo = int(np.searchsorted(np.array(ids, dtype=np.int64), q))
        assert [int(t) for t in replay[("search", k)].split()] == [lo, lo if lo < len(ids) and ids[lo] == q else -1], (q, len(ids))
    for k, (i, m) in enumerate(ENTRY):
        e = int(replay[("entry", k)])
        assert 0 <= e < m and e == (i % m if i >= 0 else (i + 2 ** 64) % m), (i, m, e)


@pytest.mark.parametrize("order", list(BIND))
def test_bind_equals_take(replay, order):
    """Layout::bind places a region where take(bytes) does and advances the end the same, with a block and without; without, no pointer moves (the program checks)."""
    v = [int(t) for t in replay[("bind", order)].split()]
    assert len(v) == 5 * len(BIND[order])
    end = 0
    for k, (size, count) in enumerate(BIND[order]):
        at, raw_at, bound_end, null_end, raw_end = v[5 * k: 5 * k + 5]
        assert at == raw_at == end and at % 256 == 0
        end += (size * count + 255) // 256 * 256
        assert bound_end == null_end == raw_end == end
