"""Helpers shared by the tests of pushed rollouts (tests/test_push_rollout_host.py on the CPU,
tests/test_gpu_push_rollout.py on the device): the push of include/zmpc.h ("The push, stated
once") as a table of velocity steps, and the oracle loops that take it on both axes.  Not a test
module.

dvel [n, 2]: what the velocity of sample i + 1 is lowered by at history step i, on (x, y); row
n − 1 is never applied."""
import numpy as np

from oracle import herdt_oracle as HO
from oracle import zmp_oracle as O

import herdt_cases as hc
import push_shaped_cases as ps
import strict_cases as sc

N_WALK = 40                                  # samples of the strict cases
STRICT_HORIZONS = (8, 33, 64)
STRICT_WALKS = 3                             # walks of a case the host test rolls out
IMPULSE = (0.3, -0.2)                        # total velocity steps on (x, y), m/s
PUSHES = ((3, 0), (7, 20), (7, N_WALK - 4))  # (D, s); the last is truncated by the walk's end


def ramp(D):
    """D rising weights 1/D .. 1: not symmetric, so w_j and w_(D−1−j) differ (the half-sine the
    other cases use reads the same forwards and backwards)."""
    return (np.arange(D) + 1.0) / D


def window(n, s, D, w, amp):
    """dvel [n, 2] of one walk: amp (x, y) times w_j (None: ones, no product) at steps s + j,
    j < D; a start outside [0, n − 1) is no push, the part from step n − 1 on is dropped."""
    dv = np.zeros((n, 2))
    if not 0 <= s < n - 1:
        return dv
    for j in range(D):
        if s + j >= n - 1:
            break
        for a in range(2):
            dv[s + j, a] = amp[a] if w is None else amp[a] * w[j]
    return dv


def push_amp(D, w=None):
    """(x, y) amplitudes whose weights sum to the impulses IMPULSE."""
    tot = float(D) if w is None else float(np.sum(w))
    return np.array(IMPULSE) / tot


def strict_pushes(n=N_WALK):
    """The three half-sine pushes of the strict tests → list of (D, s, w [D], amp [2], dvel)."""
    out = []
    for D, s in PUSHES:
        w = ps.half_sine(D)
        amp = push_amp(D, w)
        out.append((D, s, w, amp, window(n, s, D, w, amp)))
    return out


RAMP_CASE = ("jitter", 33)  # the strict case that also takes the rising profile


def ramp_pushes(n=N_WALK):
    """The (7, 20) and the truncated (7, n − 4) push with the rising profile → as strict_pushes."""
    out = []
    for D, s in PUSHES[1:]:
        w = ramp(D)
        amp = push_amp(D, w)
        out.append((D, s, w, amp, window(n, s, D, w, amp)))
    return out


# ----------------------------------------------------------------------------- strict

def rollout_strict_pushed(x_init, y_init, zmax, zmin, N, dt, h, g, Q, R, dvel):
    """O.rollout_strict statement by statement, with the subtraction on both axes: after
    x⁺ = A x + B u0 of history step i the velocity of axis a drops by dvel[i, a].  With
    dvel[kick_step, 1] = kick alone it is O.rollout_strict bit for bit."""
    n = len(zmax)
    A, Bv, _ = O.lipm(dt, h, g)
    H, V, Px, Pu = O.strict_matrices(N, dt, h, g, Q, R)
    p0 = Pu[0, 0]
    zx, zn = O._extend(np.asarray(zmax), N), O._extend(np.asarray(zmin), N)
    hist = np.empty((n, 2, 3))
    st = [np.asarray(x_init, np.float64).reshape(3).copy(),
          np.asarray(y_init, np.float64).reshape(3).copy()]
    hist[0, 0], hist[0, 1] = st
    Ws = [None, None]
    for i in range(n - 1):
        for a in range(2):
            hi = zx[i + 1:i + 1 + N, a]
            lo = zn[i + 1:i + 1 + N, a]
            W0 = None if Ws[a] is None else np.concatenate([Ws[a][1:], Ws[a][-1:]])
            u0, W, z, q = O.strict_u0(st[a], hi, lo, H, Px, p0, Q, W0)
            Ws[a] = W
            st[a] = A @ st[a] + Bv[:, 0] * u0
        for a in range(2):
            if dvel[i, a] != 0.0:
                st[a] = st[a] - np.array([0.0, dvel[i, a], 0.0])
        hist[i + 1, 0], hist[i + 1, 1] = st
    return hist


def strict_walk(case, b, weights, dvel, dx0=0.0):
    Q, R, h = weights
    x0 = case["x0"][b] + dx0
    return rollout_strict_pushed(x0[0], x0[1], case["zmax"][b], case["zmin"][b], case["N"],
                                 case["dt"], h, sc.G, Q, R, dvel)


def kick_window(n, kick, kick_step):
    """The legacy one-sample y kick as dvel."""
    dv = np.zeros((n, 2))
    if 0 <= kick_step < n - 1:
        dv[kick_step, 1] = kick
    return dv


def strict_probe(job):
    """Pool worker: one (family, N, weights index, push index) — the anchor against
    O.rollout_strict on the case's own kicks and the oracle loop's response to x0 + 1e-12 under
    the push, over the first STRICT_WALKS walks → (anchor difference, response, max |state|)."""
    family, N, wi, pi = job
    case = sc.rollout_case(family, N, n=N_WALK)
    weights = sc.WEIGHTS[wi]
    # (push indices past the half-sine pushes: the rising profile)
    dvel = (strict_pushes() + ramp_pushes())[pi][4]
    anchor = resp = big = 0.0
    for b in range(STRICT_WALKS):
        if pi == 0:  # (the anchor does not depend on the push: once per case and weights)
            kv, ks = float(case["kick"][b]), int(case["kick_step"][b])
            ref = sc.oracle_walk(case, b, weights)
            mine = strict_walk(case, b, weights, kick_window(N_WALK, kv, ks))
            anchor = max(anchor, float(np.abs(mine - ref).max()))
        a = strict_walk(case, b, weights, dvel)
        c = strict_walk(case, b, weights, dvel, dx0=1e-12)
        resp = max(resp, float(np.abs(a - c).max()))
        big = max(big, float(np.abs(a).max()))
    return anchor, resp, big


# ----------------------------------------------------------------------------- Herdt

def herdt_rollout_pushed(cfg, x0, v_ref, states, dvel, step_fn=hc.oracle_step):
    """The loop of herdt_cases.rollout_ref with the subtraction on both axes over a window:
    after history step i the velocity of axis a drops by dvel[i, a].  → (com [n,2], y_hist [n,3],
    foot [n,2], x_hist [n,3])."""
    v_ref = np.asarray(v_ref, np.float64)
    states = np.asarray(states)
    n, N = len(v_ref), cfg.horizon
    x_fc, y_fc = 0.0, float(cfg.foot_spread)
    side = "left"
    x_air, y_air = x_fc, y_fc
    fxh, fyh = [x_fc], [y_fc]
    cur = states[0]
    vpad = np.vstack([v_ref, np.repeat(v_ref[-1:], N, axis=0)])
    spad = np.concatenate([states, np.repeat(states[-1:], N)])
    nb = HO.find_nb_steps(spad)
    xh = [np.asarray(x0[0], np.float64).reshape(3)]
    yh = [np.asarray(x0[1], np.float64).reshape(3)]
    for i in range(n - 1):
        xn, yn, fx, fy = step_fn(cfg, xh[-1], yh[-1], vpad[i + 1: i + 1 + N], fxh[-1], fyh[-1],
                                 cur, spad[i + 1: i + 1 + N], side, (x_air, y_air))
        xh.append(xn)
        yh.append(yn)
        if fx is not None:
            x_air += (1 / nb[i][0]) * (fx - x_air)
        if fy is not None:
            y_air += (1 / nb[i][0]) * (fy - y_air)
        if spad[i + 1] != cur and cur == hc.SS:
            side = "left" if side == "right" else "right"
            if fx is not None and fy is not None:
                fxh.append(float(fx))
                fyh.append(float(fy))
            else:
                fxh.append(x_air)
                fyh.append(y_air)
            x_air, y_air = fxh[-1], fyh[-1]
        else:
            fxh.append(fxh[-1])
            fyh.append(fyh[-1])
        if dvel[i, 0] != 0.0:
            xh[-1] = xh[-1] - np.array([0.0, dvel[i, 0], 0.0])
        if dvel[i, 1] != 0.0:
            yh[-1] = yh[-1] - np.array([0.0, dvel[i, 1], 0.0])
        if spad[i + 1] != cur:
            cur = spad[i + 1]
    xh, yh = np.array(xh), np.array(yh)
    return np.stack([xh[:, 0], yh[:, 0]], 1), yh, np.stack([fxh, fyh], 1), xh


HERDT_WALKS = ("n40_ssp9_kickmid", "seven", "n17_triangle", "n33_rect_16gon", "n17_n3")
HERDT_D = 5
HERDT_AMP = (0.012, 0.02)  # m/s per unit weight on (x, y): shoves of the size of the cases' kicks


def herdt_case(name):
    return {c["name"]: c for c in hc.rollout_cases()}[name]


HERDT_RAMP_WALK = "seven"   # the walk that also takes the rising profile
HERDT_BATCH_AMP = (0.004, 0.006)  # the same for the walks of rollout_batch()


def herdt_window(case, profile=ps.half_sine):
    """The D = 5 xy push (half-sine, or ramp) at the case's kick step → (w, amp, dvel)."""
    w = profile(HERDT_D)
    amp = np.array(HERDT_AMP)
    return w, amp, window(case["n"], case["kick_step"], HERDT_D, w, amp)


def herdt_batch_steps(n, B):
    """A start step per walk of rollout_batch() round n // 2: walk 5 outside the range, the last
    walk truncated by its end."""
    steps = n // 2 + (np.arange(B) % 7) - 3
    steps[5], steps[B - 1] = n - 1, n - 3
    return steps


def herdt_probe(key):
    """Pool worker: the pushed loop alone on one walk — a name of HERDT_WALKS, (name, "ramp"), or
    ("batch", b) for walk b of rollout_batch() under its push of the device test → the response
    of CoM and feet to x0 + 1e-12."""
    if key[0] == "batch":
        batch = hc.rollout_batch()
        cfg = hc.make_config(batch["cfg_kw"])
        b, n = key[1], batch["n"]
        x0, v, st = batch["x0"][b], batch["v"][b], batch["states"][b]
        s = int(herdt_batch_steps(n, len(batch["x0"]))[b])
        dvel = window(n, s, HERDT_D, ps.half_sine(HERDT_D), HERDT_BATCH_AMP)
    else:
        name, profile = (key, ps.half_sine) if isinstance(key, str) else (key[0], ramp)
        case = herdt_case(name)
        cfg = hc.make_config(case["cfg_kw"])
        x0, v, st = case["x0"], case["v"], case["states"]
        dvel = herdt_window(case, profile)[2]
    a = herdt_rollout_pushed(cfg, x0, v, st, dvel)
    c = herdt_rollout_pushed(cfg, x0 + 1e-12, v, st, dvel)
    return float(max(np.abs(a[0] - c[0]).max(), np.abs(a[2] - c[2]).max()))


# ----------------------------------------------------------------------------- unconstrained

def chained(zmax, zmin, par, dvel_steps):
    """push_shaped_cases.chained_histories for windows given by history step: dvel_steps
    [S, n, 2] as above (row i lowers sample i + 1) → hist [S, n, 2, 3]."""
    S, n = dvel_steps.shape[:2]
    by_sample = np.zeros((S, n, 2))
    by_sample[:, 1:] = dvel_steps[:, :n - 1]
    return ps.chained_histories(zmax, zmin, par, by_sample)
