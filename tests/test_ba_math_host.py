"""CPU: the local bundle adjustment's shared formulas (csrc/ba_math.hpp) replayed by a stand-alone host program and compared with a
transcription of each routine in numpy float64 scalars, in the operand order the routine documents -- every double with ==, two NaNs
counting as equal.  The program (tests/c_host/ba_math_check.cpp) includes ba_math.hpp alone.  Built twice: plain, and with
-fsanitize=address,undefined,float-cast-overflow (the program alone; nothing loaded into Python runs under a sanitizer)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "ba_math_check.cpp")
INC = os.path.join(ROOT, "slam.jl_amd", "csrc")

F = np.float64
LM_MAX_DELTA, LM_MIN_DELTA, LM_MIN_STEP_QUALITY = F(1e16), F(1e-16), F(1e-3)
LM_MIN_DIAGONAL, LM_MAX_DIAGONAL, LM_DELTA0, LM_XTOL, LM_FTOL = F(1e-6), F(1e32), F(10.0), F(1e-8), F(1e-8)
FIELDS = ["delta", "decrease_factor", "ssr", "trial_ssr", "pred_ssr", "maxdx", "ssr_init", "ssr_pass1", "ssr_final",
          "converged", "accept", "iters", "n_outliers", "chol_fail", "iters_pass1", "iters_pass2", "cur"]

DIAGS = [0.0, 1e-7, 1e-6, 1.0, 1e32, 1e33]             # below, at and above both clamps
INV_DELTAS = [0.1, 1e16, 1e-16]
NREC = 64


# ---- the routines, transcribed (np.float64 scalars: one IEEE operation per Python operation, nothing fused) ---------------------------
def lm_damp(diag, inv_delta):
    return np.fmin(np.fmax(F(diag), LM_MIN_DIAGONAL), LM_MAX_DIAGONAL) * F(inv_delta)


def jl_products(Jl, r):
    Jl = [F(x) for x in Jl]; r = [F(x) for x in r]
    v = [Jl[0] * Jl[0] + Jl[3] * Jl[3], Jl[0] * Jl[1] + Jl[3] * Jl[4], Jl[0] * Jl[2] + Jl[3] * Jl[5],
         Jl[1] * Jl[1] + Jl[4] * Jl[4], Jl[1] * Jl[2] + Jl[4] * Jl[5], Jl[2] * Jl[2] + Jl[5] * Jl[5]]
    return v + [Jl[k] * r[0] + Jl[3 + k] * r[1] for k in range(3)]


def inv3_sym(V):
    a, b, c, dd, e, f = V[:6]
    A, B, C = dd * f - e * e, c * e - b * f, b * e - c * dd
    det = a * A + b * B + c * C
    i = F(1.0) / det
    return [A * i, B * i, C * i, (a * f - c * c) * i, (b * c - a * e) * i, (a * dd - b * b) * i]


def point_solve(obs, inv_delta):
    V = [F(0.0)] * 9
    for Jl, r in obs:
        V = [V[k] + p for k, p in enumerate(jl_products(Jl, r))]
    for k in (0, 3, 5):
        V[k] = V[k] + lm_damp(V[k], inv_delta)
    return V, inv3_sym(V)


def w_rows(Jp, Jl):
    Jp = [F(x) for x in Jp]; Jl = [F(x) for x in Jl]
    return [Jp[a] * Jl[c] + Jp[6 + a] * Jl[3 + c] for a in range(6) for c in range(3)]


def sym3_mul(Vi, b):
    Vi = [F(x) for x in Vi]; b = [F(x) for x in b]
    return [Vi[0] * b[0] + Vi[1] * b[1] + Vi[2] * b[2], Vi[1] * b[0] + Vi[3] * b[1] + Vi[4] * b[2], Vi[2] * b[0] + Vi[4] * b[1] + Vi[5] * b[2]]


def jp_dot(jp, dp, a, b):
    a, b = F(a), F(b)
    for k in range(6):
        a = a + F(jp[k]) * F(dp[k]); b = b + F(jp[6 + k]) * F(dp[k])
    return [a, b]


def obs_is_outlier(z, r, depth_eps, repr_eps):
    return bool(F(z) < F(depth_eps) or (F(r[0]) * F(r[0]) + F(r[1]) * F(r[1])) > F(repr_eps))


class LM:
    """LMState and its four steps."""
    def __init__(self, vals):
        for k, v in zip(FIELDS, vals):
            setattr(self, k, F(v) if FIELDS.index(k) < 9 else int(v))

    def values(self):
        return [float(getattr(self, k)) for k in FIELDS]

    def first_pass(self, outliers):
        self.ssr_init = self.ssr; self.chol_fail = 0
        if outliers:
            self.n_outliers = 0

    def trust_reset(self):
        self.delta = LM_DELTA0; self.decrease_factor = F(2.0); self.converged = 0; self.accept = 0; self.iters = 0

    def record_pass(self, p):
        if p == 1:
            self.ssr_pass1 = self.ssr; self.iters_pass1 = self.iters
        else:
            self.ssr_final = self.ssr; self.iters_pass2 = self.iters

    def decide(self, t, p, mx):
        t, p, mx = F(t), F(p), F(mx)
        self.iters += 1
        if self.chol_fail:
            self.converged = 1; self.accept = 0
            return
        ssr = self.ssr
        rho = (t - ssr) / (p - ssr)
        if rho > LM_MIN_STEP_QUALITY:
            x_conv = mx <= LM_XTOL
            f_conv = np.abs(ssr - t) / (np.abs(ssr) + LM_FTOL) <= LM_FTOL
            self.ssr = t
            u = F(2.0) * rho - F(1.0)
            self.delta = np.fmin(self.delta / np.fmax(F(1.0) / F(3.0), F(1.0) - u * u * u), LM_MAX_DELTA)
            self.decrease_factor = F(2.0)
            self.accept = 1
            self.cur ^= 1
            self.converged = int(x_conv or f_conv)
        else:
            self.delta = np.fmax(self.delta / self.decrease_factor, LM_MIN_DELTA)
            self.decrease_factor = self.decrease_factor * F(2.0)
            self.accept = 0
            self.converged = int(mx <= LM_XTOL)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def _records(seed, n, width, scale=1.0):
    return np.random.default_rng(seed).standard_normal((n, width)) * scale


def _obs(seed, n):
    # Jacobian rows of a camera a few metres from its points (hundreds of pixels per metre), residuals of a few pixels
    rec = _records(seed, n, 8)
    return [(list(q[:6] * 300.0), list(q[6:] * 2.0)) for q in rec]


PSOLVE = [("obs1", _obs(11, 1), 0.1), ("obs2", _obs(12, 2), 0.1), ("obs7", _obs(13, 7), 0.1), ("obs7_tight", _obs(14, 7), 1e-16),
          ("rank_deficient", [([1.0, 2.0, 3.0, 4.0, 5.0, 6.0], [1.0, -1.0])], 0.0)]      # small integers: det is exactly 0
WELL = ["obs2", "obs7"]                                   # two or more observations and a damping of a tenth of the diagonal

SENTINEL = [3.0, 5.0, 100.0, -1.0, -2.0, -3.0, -4.0, -5.0, -6.0, 7, 8, 9, 10, 0, 11, 12, 0]      # every field something its routine does not write


def _lm_scripts():
    """name -> list of (command, arguments); the state starts from SENTINEL each time."""
    start = [("lm_first", [1]), ("lm_reset", [])]
    rej = ("lm_decide", [101.0, 99.0, 0.1])                # rho = 1 / -1 < 0
    return {
        "accept_plain": start + [("lm_decide", [60.0, 50.0, 0.1])],
        "accept_f_conv": start + [("lm_decide", [100.0 * (1 - 1e-10), 100.0 * (1 - 1.2e-10), 0.1])],
        "accept_x_conv": start + [("lm_decide", [50.0, 40.0, 1e-9])],
        "accept_x_conv_at_tolerance": start + [("lm_decide", [50.0, 40.0, 1e-8])],
        "three_rejections": start + [rej, rej, rej],
        "reject_then_accept": start + [rej, ("lm_decide", [60.0, 50.0, 0.1]), rej],
        "reject_x_conv": start + [("lm_decide", [101.0, 99.0, 1e-9])],
        "rho_at_threshold": start + [("lm_decide", [99.9, 0.0, 0.1])],
        "rho_nan": start + [("lm_decide", [100.0, 100.0, 0.1])],
        "delta_to_max": start + [("lm_decide", [100.0 - 0.5 ** k, 100.0 - 0.5 ** k, 0.1]) for k in range(1, 40)],
        "delta_to_min": start + [rej] * 12,
        "chol_fail": [("lm_set", SENTINEL[:13] + [1] + SENTINEL[14:]), ("lm_decide", [60.0, 50.0, 0.1])],
        "first_pass_keeps_outliers": [("lm_first", [0]), ("lm_reset", [])],
        "record_passes": start + [("lm_decide", [60.0, 50.0, 0.1]), ("lm_record", [1]), ("lm_reset", []), rej, ("lm_decide", [30.0, 20.0, 0.1]), ("lm_record", [2])],
    }


def _hex(v):
    return " ".join(float(x).hex() for x in np.asarray(v, dtype=np.float64).ravel())


FLAGS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(FLAGS), ids=list(FLAGS))
def replay(request, tmp_path_factory):
    """One build and one run per flag set: {case: array of the program's doubles}."""
    exe = str(tmp_path_factory.mktemp("ba_math_" + request.param) / "ba_math_check")
    cxx = os.environ.get("CXX", "c++")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", INC] + FLAGS[request.param] + [SRC, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    keys, lines = [], []
    def add(key, cmd, *args):
        keys.append(key); lines.append(cmd + " " + " ".join(_hex(a) for a in args))
    for d in DIAGS:
        for i in INV_DELTAS:
            add(("damp", d, i), "damp", [d, i])
    for name, obs, inv_delta in PSOLVE:
        add(("psolve", name), "psolve", [inv_delta, len(obs)], *[Jl + r for Jl, r in obs])
    jl, jp, vi, dp = _records(21, NREC, 8, 300.0), _records(22, NREC, 12, 300.0), _records(23, NREC, 9), _records(24, NREC, 8, 1e-2)
    for k in range(NREC):
        add(("jlp", k), "jlp", jl[k])
        add(("wrow", k), "wrow", jp[k], jl[k, :6])
        add(("sym3", k), "sym3", vi[k])
        add(("jpdot", k), "jpdot", jp[k], dp[k])
    add(("wrow", "zero_jp"), "wrow", np.zeros(12), jl[0, :6])
    add(("jpdot", "zero_jp"), "jpdot", np.zeros(12), dp[0])
    for k, (z, r, de, re) in enumerate(OUTLIER_CASES):
        add(("outl", k), "outl", [z], r, [de, re])
    for name, script in _lm_scripts().items():
        add(("lm", name, -1), "lm_set", SENTINEL)
        for q, (cmd, args) in enumerate(script):
            add(("lm", name, q), cmd, args)
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.strip().split("\n")
    assert len(out) == len(keys), r.stdout[-2000:]
    got = {k: np.array([float.fromhex(t) for t in ln.split()]) for k, ln in zip(keys, out)}
    got["records"] = (jl, jp, vi, dp)
    return got


def _same(got, want):
    got = np.asarray(got, dtype=np.float64); want = np.asarray([float(x) for x in want], dtype=np.float64)
    return got.shape == want.shape and bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))


# (z, r, depth_eps, repr_eps): both sides of both thresholds and equality on each; 3^2 + 4^2 = 25 exactly
OUTLIER_CASES = [(0.5, [3.0, 4.0], 0.1, 25.0), (0.1, [3.0, 4.0], 0.1, 25.0), (np.nextafter(0.1, 0.0), [3.0, 4.0], 0.1, 25.0), (-1.0, [0.0, 0.0], 0.1, 25.0),
                 (0.5, [3.0, 4.0], 0.1, np.nextafter(25.0, 0.0)), (0.5, [3.0, 4.0], 0.1, np.nextafter(25.0, 30.0)), (0.5, [0.0, 0.0], 0.1, 0.0),
                 (0.05, [30.0, 40.0], 0.1, 25.0)]
OUTLIER_WANT = [False, False, True, True, True, False, False, True]


@pytest.mark.parametrize("diag", DIAGS)
@pytest.mark.parametrize("inv_delta", INV_DELTAS)
def test_lm_damp_bits(replay, diag, inv_delta):
    assert _same(replay[("damp", diag, inv_delta)], [lm_damp(diag, inv_delta)])
    clamped = min(max(diag, 1e-6), 1e32)                   # the reference's rule: the clamped entry, scaled
    assert replay[("damp", diag, inv_delta)][0] == clamped * inv_delta


@pytest.mark.parametrize("name", [p[0] for p in PSOLVE])
def test_point_solve_bits(replay, name):
    _, obs, inv_delta = next(p for p in PSOLVE if p[0] == name)
    with np.errstate(all="ignore"):
        V, Vi = point_solve(obs, inv_delta)
    got = replay[("psolve", name)]
    assert _same(got, V + Vi)
    if name == "rank_deficient":
        assert not np.all(np.isfinite(got[9:]))            # nothing hides the singular block: the solve downstream reports it
    if name in WELL:
        v, i = got[:6], got[9:]
        sym = lambda q: np.array([[q[0], q[1], q[2]], [q[1], q[3], q[4]], [q[2], q[4], q[5]]])
        assert np.max(np.abs(sym(v) @ sym(i) - np.eye(3))) < 1e-9      # a sanity bound, not a parity claim


def test_observation_products_bits(replay):
    jl, jp, vi, dp = replay["records"]
    for k in range(NREC):
        assert _same(replay[("jlp", k)], jl_products(jl[k, :6], jl[k, 6:])), k
        assert _same(replay[("wrow", k)], w_rows(jp[k], jl[k, :6])), k
        assert _same(replay[("sym3", k)], sym3_mul(vi[k, :6], vi[k, 6:])), k
        assert _same(replay[("jpdot", k)], jp_dot(jp[k], dp[k, :6], dp[k, 6], dp[k, 7])), k


def test_constant_pose_observation(replay):
    """Jp = 0 (an observation of a constant pose): W is zero and the accumulators keep their values."""
    jl, jp, vi, dp = replay["records"]
    assert _same(replay[("wrow", "zero_jp")], w_rows(np.zeros(12), jl[0, :6])) and not replay[("wrow", "zero_jp")].any()
    assert _same(replay[("jpdot", "zero_jp")], jp_dot(np.zeros(12), dp[0, :6], dp[0, 6], dp[0, 7]))
    assert _same(replay[("jpdot", "zero_jp")], dp[0, 6:])


@pytest.mark.parametrize("k", range(len(OUTLIER_CASES)))
def test_obs_is_outlier(replay, k):
    z, r, de, re = OUTLIER_CASES[k]
    assert bool(replay[("outl", k)][0]) == obs_is_outlier(z, r, de, re) == OUTLIER_WANT[k]


@pytest.mark.parametrize("name", list(_lm_scripts()))
def test_lm_state_steps(replay, name):
    script = _lm_scripts()[name]
    s = LM(SENTINEL)
    assert _same(replay[("lm", name, -1)], s.values())
    seen = []
    for q, (cmd, args) in enumerate(script):
        before = s.values()
        with np.errstate(all="ignore"):
            if cmd == "lm_set": s = LM(args)
            elif cmd == "lm_first": s.first_pass(bool(args[0]))
            elif cmd == "lm_reset": s.trust_reset()
            elif cmd == "lm_record": s.record_pass(int(args[0]))
            else: s.decide(*args)
        assert _same(replay[("lm", name, q)], s.values()), (name, q, cmd, dict(zip(FIELDS, replay[("lm", name, q)])))
        seen.append((cmd, dict(zip(FIELDS, before)), dict(zip(FIELDS, s.values()))))
    # what each case is there for, stated on the transcription (which the program has just been shown to equal)
    last = seen[-1][2]
    decides = [(b, a) for c, b, a in seen if c == "lm_decide"]
    for b, a in decides:
        assert a["cur"] == (b["cur"] != a["accept"]) and a["iters"] == b["iters"] + 1      # cur toggles on accept only
    if name == "accept_plain": assert last["accept"] == 1 and last["converged"] == 0 and last["ssr"] == 60.0
    if name in ("accept_f_conv", "accept_x_conv", "accept_x_conv_at_tolerance"): assert last["accept"] == 1 and last["converged"] == 1
    if name == "three_rejections":
        assert [a["decrease_factor"] for _, a in decides] == [4.0, 8.0, 16.0] and [b["decrease_factor"] for b, _ in decides] == [2.0, 4.0, 8.0]
        assert [a["delta"] for _, a in decides] == [5.0, 1.25, 0.15625] and all(a["cur"] == 0 and a["accept"] == 0 and a["ssr"] == 100.0 for _, a in decides)
    if name == "rho_at_threshold": assert last["accept"] == 0                # rho = 0.001 exactly is not above the step quality
    if name == "rho_nan": assert last["accept"] == 0
    if name == "delta_to_max": assert last["delta"] == 1e16 and all(a["accept"] == 1 for _, a in decides)
    if name == "delta_to_min": assert last["delta"] == 1e-16
    if name == "chol_fail":
        b, a = decides[0]
        assert a["converged"] == 1 and a["accept"] == 0 and a["iters"] == b["iters"] + 1
        assert all(a[k] == b[k] for k in FIELDS if k not in ("converged", "accept", "iters"))
    if name == "first_pass_keeps_outliers": assert last["n_outliers"] == 10 and last["chol_fail"] == 0 and last["ssr_init"] == 100.0
    if name == "record_passes":
        assert last["ssr_pass1"] == 60.0 and last["iters_pass1"] == 1 and last["ssr_final"] == 30.0 and last["iters_pass2"] == 2
