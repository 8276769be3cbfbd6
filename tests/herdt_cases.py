"""Seeded inputs and CPU references shared by the Herdt shape tests (the host test of the inputs
and of the oracle, tests/test_herdt_cases_host.py; the device tests,
tests/test_gpu_herdt_shapes.py; the stored long-horizon answers,
tests/golden/make_herdt_shapes_golden.py).  Not a test module.

Everything here is plain arrays plus the MPCConfig keyword arguments of a case; the only solver
it calls is the CPU oracle (oracle/herdt_oracle.py).
"""
import functools

import numpy as np

from oracle import herdt_oracle as HO

ST, DS, SS = HO.STANDING, HO.DOUBLE_SUPPORT, HO.SINGLE_SUPPORT

STEP_HORIZONS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 33, 64)   # B = 40 each (N = 17: 75, 3 workgroups)
VARIANT_HORIZONS = (16, 17, 33)                          # polytope / geometry variants b, c, d
STEP_PARAMS = [(N, "a") for N in STEP_HORIZONS + (150,)] + \
              [(N, v) for N in VARIANT_HORIZONS for v in "bcd"]
LONG_HORIZONS = {300: 4, 702: 2}                         # stored answers (herdt_shapes.npz)


def step_dt(N):
    """Sampling time of the step cases: 0.07 s at the short horizons (the rollout cases' coarse
    step), else the class rule 1.5 / N (0.01 s at the default N = 150)."""
    return 0.07 if N <= 17 else 1.5 / N


def _ngon(k, cx, cy, r):
    a = 2 * np.pi * (np.arange(k) + 0.25) / k
    return tuple((float(cx + r * np.cos(t)), float(cy + r * np.sin(t))) for t in a)


TRIANGLE = ((-0.1, -0.38), (0.6, -0.3), (0.15, -0.1))
RECTANGLE = ((-0.1, -0.4), (0.6, -0.4), (0.6, -0.12), (-0.1, -0.12))
HEXADECAGON = _ngon(16, 0.25, 0.27, 0.16)
HEPTADECAGON = _ngon(17, 0.25, 0.27, 0.16)               # one facet too many for the device


def variant_kwargs(variant):
    """MPCConfig keyword arguments of the polytope / geometry variants a-d."""
    if variant == "a":
        return {}
    if variant == "b":
        return dict(left_foot_polytope=TRIANGLE,
                    right_foot_polytope=tuple((x, -y) for x, y in TRIANGLE),
                    foot_length=0.2, foot_width=0.1, foot_spread=0.12)
    if variant == "c":
        return dict(left_foot_polytope=RECTANGLE, right_foot_polytope=HEXADECAGON)
    if variant == "d":
        return dict(h=0.9, g=3.71)
    raise KeyError(variant)


def config_kwargs(N, dt, variant="a"):
    return dict(method="herdt", horizon=int(N), dt=float(dt), **variant_kwargs(variant))


# ----------------------------------------------------------------------------- schedules

def schedule(standing, dsp, ssp, tail, length):
    """A support schedule of `length` samples: `standing` STANDING samples, then steps of `dsp`
    DOUBLE_SUPPORT + `ssp` SINGLE_SUPPORT samples, the last `tail` samples STANDING."""
    walk = max(length - standing - tail, 0)
    step = [DS] * dsp + [SS] * ssp
    reps = walk // len(step) + 1
    seq = [ST] * standing + (step * reps)[:walk] + [ST] * tail
    return np.array(seq[:length], np.int8)


def window_of(seq, off, N):
    """(current, window [N]) at sample `off` of a schedule, padded with its last sample."""
    pad = np.concatenate([seq, np.repeat(seq[-1:], N + 1)])
    return int(pad[off]), pad[off + 1: off + 1 + N].astype(np.int8)


def footsteps(cur, win):
    """(m, M): footsteps in the window and those with rows inside the horizon."""
    seg = HO.support_segments(cur, win)
    m = len(seg) - 1
    return m, m - (1 if m > 0 and seg[-1] == 1 else 0)


def max_fit(N):
    """Most footsteps a horizon of N rows holds with dsp >= 1 and ssp >= 1 (a footstep every
    second row at the densest), capped at the device's 8."""
    return min(8, (N + 1) // 2)


def _walking(N, period, off):
    """Window of a walk of step period `period` (dsp = 1) seen from sample `off` of a step."""
    seq = schedule(0, 1, period - 1, 0, N + period + 2)
    return window_of(seq, off, N)


def _special_windows(N):
    """The named windows of a horizon, as (tag, current, window)."""
    out = [("stand0", ST, np.zeros(N, np.int8)),       # m = 0, standing hull
           ("stand1", DS, np.zeros(N, np.int8)),       # all standing, current DOUBLE_SUPPORT
           ("stand2", SS, np.zeros(N, np.int8))]       # all standing, current SINGLE_SUPPORT
    # m = 1 whose only break is on row N − 1 (M = 0), standing and walking
    w = np.zeros(N, np.int8)
    w[-1] = DS
    out.append(("m0stand", ST, w))
    # Not at N = 150: with 149 constrained rows this one window costs the oracle about 1.5 s
    # there and takes the batch's live-oracle work from 3.4 s to the 5 s a device test may
    # spend; m0stand above keeps the M = 0 shape at that horizon.
    if N != 150:
        w = np.full(N, SS, np.int8)
        w[-1] = DS
        out.append(("m0walk", SS, w))
    if N >= 3:
        # last transition on row N − 1 after an earlier footstep: empty last column, M = m − 1
        w = np.full(N, SS, np.int8)
        w[0] = w[-1] = DS
        out.append(("emptylast", SS, w))
        # current STANDING with walking rows ahead
        a, per = max(1, N // 3), max(2, N // 4)
        _, ww = _walking(N, per, per - 1)
        out.append(("standahead", ST, np.concatenate([np.zeros(a, np.int8), ww[: N - a]])))
        # a walking window that ends in standing rows
        t, per = max(1, N // 3), max(2, N // 5)
        c, ww = _walking(N, per, per - 1)
        out.append(("walktail", c, np.concatenate([ww[: N - t], np.zeros(t, np.int8)])))
    return out


def _find_walking(N, m):
    """A walking window with m footsteps: a periodic walk with every footstep's rows inside the
    horizon if there is one, else any periodic walk, else the densest walk cut short by a
    standing tail."""
    for full in (True, False):
        for per in range(2, N + 3):
            for off in range(per):
                c, w = _walking(N, per, off)
                mm, M = footsteps(c, w)
                if mm == m and (M == m or not full):
                    return (f"m{m}", c, w)
    for k in range(1, N):
        c, w = _walking(N, 2, 1)
        w = np.concatenate([w[:k], np.zeros(N - k, np.int8)])
        if footsteps(c, w)[0] == m:
            return (f"m{m}", c, w)
    return None


def _cover_windows(N, have):
    """Walking windows for every footstep count 0..max_fit(N) not in `have`."""
    out = []
    for m in range(max_fit(N) + 1):
        if m in have:
            continue
        found = _find_walking(N, m)
        assert found is not None, (N, m)
        out.append(found)
    return out


def _random_window(rng, N):
    per = int(rng.integers(2, max(3, N + 1)))
    dsp = 1 if per < 4 or rng.random() < 0.7 else 2
    standing = int(rng.integers(0, max(1, N // 2) + 1))
    tail = int(rng.integers(0, N + 1)) if rng.random() < 0.4 else 0
    length = standing + int(rng.integers(1, 2 * N + 2)) + tail
    seq = schedule(standing, dsp, per - dsp, tail, length)
    off = int(rng.integers(0, max(1, length - 1)))
    return window_of(seq, off, N)


def _random_states(rng, B, N, spread):
    """Sides, feet, states and constant reference velocities of B windows: the CoM within 1 cm
    of the foot, velocity ~N(0, 0.05), acceleration ~N(0, 0.1), foot x ~N(0, 0.3), foot y = ±spread
    (left: +), v_ref in [0, 0.4] × [−0.05, 0.05]."""
    side = rng.integers(0, 2, B).astype(np.int8)
    foot = np.stack([rng.normal(0.0, 0.3, B), np.where(side == 0, spread, -spread)], axis=1)
    x = np.empty((B, 2, 3))
    x[:, :, 0] = foot + rng.uniform(-0.01, 0.01, (B, 2))
    x[:, :, 1] = rng.normal(0.0, 0.05, (B, 2))
    x[:, :, 2] = rng.normal(0.0, 0.1, (B, 2))
    vc = np.stack([rng.uniform(0.0, 0.4, B), rng.uniform(-0.05, 0.05, B)], axis=1)
    return dict(x=x, v=np.repeat(vc[:, None, :], N, axis=1), foot=foot, side=side)


def step_batch_size(N, variant="a"):
    if N == 150:
        return 12
    return 75 if (N == 17 and variant == "a") else 40


def step_cases(N, variant="a", dt=None, B=None, seed=0):
    """A batch of independent windows for one horizon: dict of x [B,2,3], v [B,N,2],
    win [B,N] int8, cur [B] int8, foot [B,2], side [B] int8 (0 left), tags (list of str),
    cfg_kw (MPCConfig keyword arguments).  The named windows come first, then one walking
    window per footstep count they miss, then random schedules."""
    dt = step_dt(N) if dt is None else dt
    B = step_batch_size(N, variant) if B is None else B
    kw = config_kwargs(N, dt, variant)
    spread = kw.get("foot_spread", 0.1)
    rng = np.random.default_rng([20260301, N, ord(variant), seed])
    wins = _special_windows(N)
    wins += _cover_windows(N, {footsteps(c, w)[0] for _, c, w in wins})
    while len(wins) < B:
        c, w = _random_window(rng, N)
        if footsteps(c, w)[0] <= 8:      # the device solver's limit
            wins.append(("random", c, w))
    assert len(wins) == B, (N, len(wins), B)
    out = _random_states(rng, B, N, spread)
    out.update(N=N, win=np.stack([w for _, _, w in wins]).astype(np.int8),
               cur=np.array([c for _, c, _ in wins], np.int8),
               tags=[t for t, _, _ in wins], cfg_kw=kw)
    return out


def long_cases(N):
    """The walking windows of the long horizons whose oracle answers are stored in
    tests/golden/herdt_shapes.npz: N = 300 with m = 2, 5, 8 and an empty last column (m = 3),
    N = 702 with m = 3 and 6."""
    if N == 300:
        w_e = np.full(N, SS, np.int8)
        w_e[[0, 140, N - 1]] = DS
        picks = [_walking(N, 160, 30), _walking(N, 60, 5), _walking(N, 38, 37), (SS, w_e)]
    else:
        picks = [_walking(N, 260, 100), _walking(N, 120, 119)]
    k = len(picks)
    assert k == LONG_HORIZONS[N]
    out = _random_states(np.random.default_rng([20260303, N]), k, N, 0.1)
    out.update(N=N, cfg_kw=config_kwargs(N, 1.5 / N), tags=["long"] * k,
               cur=np.array([c for c, _ in picks], np.int8),
               win=np.stack([w for _, w in picks]).astype(np.int8))
    return out


def case_m(case):
    """Footstep counts (m, M) [B] of a batch."""
    mm = np.array([footsteps(int(c), w) for c, w in zip(case["cur"], case["win"])])
    return mm[:, 0], mm[:, 1]


def make_config(cfg_kw):
    from mpc_bipedal.config import MPCConfig
    return MPCConfig(**cfg_kw)


def window_qp(cfg, case, b):
    side = "left" if int(case["side"][b]) == 0 else "right"
    return HO.herdt_qp(cfg, case["x"][b, 0], case["x"][b, 1], case["v"][b],
                       float(case["foot"][b, 0]), float(case["foot"][b, 1]),
                       int(case["cur"][b]), case["win"][b], side)


def solve_case(case):
    """The oracle's answer for every window: (x_next [B,2,3], step [B,2] with NaN where the
    window holds no footstep)."""
    cfg = make_config(case["cfg_kw"])
    B = len(case["cur"])
    xn, step = np.empty((B, 2, 3)), np.full((B, 2), np.nan)
    for b in range(B):
        side = "left" if int(case["side"][b]) == 0 else "right"
        xs, ys, fx, fy = HO.herdt_step(cfg, case["x"][b, 0], case["x"][b, 1], case["v"][b],
                                       float(case["foot"][b, 0]), float(case["foot"][b, 1]),
                                       int(case["cur"][b]), case["win"][b], side)
        xn[b, 0], xn[b, 1] = xs, ys
        if fx is not None:
            step[b] = fx, fy
    return xn, step


@functools.lru_cache(maxsize=None)
def step_reference(N, variant="a"):
    """(case, x_next, step) of step_cases(N, variant), solved once per session; callers must
    not write into the arrays."""
    case = step_cases(N, variant)
    xn, step = solve_case(case)
    for a in (xn, step):
        a.setflags(write=False)
    return case, xn, step


def refined_kkt(Q, p, G, h, lam, iters=4):
    """Re-solve of the QP on a given active set (the rows with lam > 0): the KKT system
    [Q Gaᵀ; Ga 0][u; λ] = [−p; ha] by LU, iteratively refined with residuals accumulated in
    extended precision.  Returns u."""
    act = np.where(lam > 0)[0]
    n, q = len(p), len(act)
    K = np.zeros((n + q, n + q))
    K[:n, :n] = Q
    K[:n, n:] = G[act].T
    K[n:, :n] = G[act]
    rhs = np.concatenate([-p, h[act]])
    Kl, rl = K.astype(np.longdouble), rhs.astype(np.longdouble)

    def solve(r):
        try:
            return np.linalg.solve(K, r)
        except np.linalg.LinAlgError:           # dependent active rows: u is still unique
            return np.linalg.lstsq(K, r, rcond=None)[0]

    z = solve(rhs).astype(np.longdouble)
    for _ in range(iters):
        r = rl - Kl @ z
        z = z + solve(r.astype(np.float64)).astype(np.longdouble)
    return z[:n].astype(np.float64)


# ----------------------------------------------------------------------------- rollouts

def walk_schedule(n, standing, dsp, ssp, tail, offset=0, vx=0.2, vy=0.0):
    """(states [n] int8, v_ref [n,2]) of a walk: schedule() cut at `offset`, forward speed vx
    (and vy) on the non-standing samples."""
    st = schedule(standing, dsp, ssp, tail, n + offset)[offset:]
    v = np.zeros((n, 2))
    v[:, 0] = np.where(st == ST, 0.0, vx)
    v[:, 1] = np.where(st == ST, 0.0, vy)
    return st, v


def _walk(name, N, dt, n, standing, ssp, tail, offset=0, variant="a", kick_step=-1, F=0.0,
          x0=None, vx=0.2, dsp=1):
    st, v = walk_schedule(n, standing, dsp, ssp, tail, offset, vx)
    kw = config_kwargs(N, dt, variant)
    kw.update(add_force=kick_step >= 0, F_ext=float(F))
    return dict(name=name, cfg_kw=kw, n=n, states=st, v=v, kick_step=kick_step,
                x0=np.zeros((2, 3)) if x0 is None else np.asarray(x0, np.float64))


X0_A = ((0.004, 0.03, 0.0), (0.103, -0.02, 0.05))
X0_B = ((-0.006, 0.0, 0.1), (0.095, 0.04, 0.0))


def rollout_cases():
    """Short single walks for herdt_rollout (dicts: name, cfg_kw, n, states [n], v [n,2],
    x0 [2,3], kick_step (−1: none); the kick is cfg.dt·F_ext/m on the y velocity).  The first
    five reach max_footsteps 5, 6, 8, 4 and 2, `seven` reaches 7: one walk per kernel instance."""
    return [
        _walk("n40_ssp9_kickmid", 40, 0.03, 90, 12, 9, 15, kick_step=45, F=60.0),
        _walk("n40_ssp6_x0", 40, 0.03, 90, 12, 6, 15, x0=X0_A),
        _walk("n40_ssp5_kick0", 40, 0.03, 90, 12, 5, 15, kick_step=0, F=40.0),
        _walk("n40_midstep_ss_kicklast", 40, 0.03, 70, 0, 9, 0, offset=3, kick_step=68, F=60.0),
        _walk("n33_onestep", 33, 0.03, 50, 8, 9, 32, kick_step=25, F=40.0, x0=X0_B),
        _walk("seven", 33, 0.03, 80, 8, 4, 12, kick_step=40, F=40.0),
        _walk("n41_midstep_ds", 41, 0.03, 60, 0, 7, 10, x0=X0_A),
        _walk("n17_triangle", 17, 0.07, 50, 6, 4, 9, variant="b", kick_step=25, F=15.0),
        _walk("n33_rect_16gon", 33, 0.03, 70, 5, 7, 11, variant="c", kick_step=35, F=40.0,
              x0=X0_B),
        _walk("n17_n3", 17, 0.07, 3, 1, 1, 0, kick_step=1, F=20.0, x0=X0_A),
        _walk("n17_n2", 17, 0.07, 2, 1, 1, 0, kick_step=0, F=20.0, x0=X0_A),
    ]


INSTANCE_OF = {0: 2, 1: 2, 2: 2, 3: 4, 4: 4, 5: 6, 6: 6, 7: 7, 8: 8}  # max_footsteps → kernel


def rollout_batch(B=33, N=17, dt=0.07, n=40):
    """B different walks for one launch: schedules staggered so that the footstep count differs
    between the lanes of a wave, per-walk v_ref, states, x0 and kicks (one kick step, n // 2)."""
    rng = np.random.default_rng([20260304, B, N, n])
    st, v = [], []
    for b in range(B):
        s, vv = walk_schedule(n, (2, 3, 4, 6)[b % 4], 1, 3 + b % 3, 1 + b % 6, vx=0.1 + 0.0025 * b,
                              vy=0.01 * ((b % 3) - 1))
        st.append(s)
        v.append(vv)
    x0 = np.zeros((B, 2, 3))
    x0[:, :, 0] = rng.uniform(-0.005, 0.005, (B, 2))
    x0[:, 1, 0] += 0.1
    x0[:, :, 1] = rng.normal(0.0, 0.02, (B, 2))
    kw = config_kwargs(N, dt)
    kw.update(add_force=True, F_ext=0.0)
    return dict(cfg_kw=kw, n=n, states=np.stack(st), v=np.stack(v), x0=x0,
                kick=rng.uniform(0.0, 0.02, B), kick_step=n // 2)


def oracle_step(cfg, x, y, v, fx, fy, cur, win, side, air):
    return HO.herdt_step(cfg, x, y, v, fx, fy, cur, win, side)


def rollout_ref(cfg, x0, v_ref, states, kick=0.0, kick_step=-1, step_fn=oracle_step):
    """HO.herdt_rollout with the kick (an impulse on the y velocity, already dt·F/m) at any step
    and the single step replaceable: step_fn also receives the air foot (x_air, y_air).  With
    kick = cfg.dt·cfg.F_ext/cfg.m at n // 2 it is HO.herdt_rollout statement by statement (the
    host test holds the two equal).  → (com [n,2], y_hist [n,3], foot [n,2], x_hist [n,3])."""
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
        if spad[i + 1] != cur and cur == SS:
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
        if i == kick_step:
            yh[-1] = yh[-1] - np.array([0.0, kick, 0.0])
        if spad[i + 1] != cur:
            cur = spad[i + 1]
    xh, yh = np.array(xh), np.array(yh)
    return np.stack([xh[:, 0], yh[:, 0]], 1), yh, np.stack([fxh, fyh], 1), xh


def case_kick(case):
    """The y-velocity impulse of a single-walk case, as the oracle forms it."""
    cfg = make_config(case["cfg_kw"])
    return cfg.dt * cfg.F_ext / cfg.m if case["kick_step"] >= 0 else 0.0


def case_max_footsteps(states, N):
    """max_footsteps of a walk (brute force over its windows with HO.support_segments)."""
    n = len(states)
    pad = np.concatenate([states, np.repeat(states[-1:], N)])
    return max([len(HO.support_segments(pad[i], pad[i + 1: i + 1 + N])) - 1
                for i in range(max(n - 1, 1))])


@functools.lru_cache(maxsize=None)
def rollout_reference(name):
    """(com, y_hist, foot, x_hist) of the named single walk, computed once per session."""
    case = {c["name"]: c for c in rollout_cases()}[name]
    cfg = make_config(case["cfg_kw"])
    out = rollout_ref(cfg, case["x0"], case["v"], case["states"], case_kick(case),
                      case["kick_step"])
    for a in out:
        a.setflags(write=False)
    return out


def batch_walk(batch, b):
    """Walk b of rollout_batch() as a single-walk (x0, v, states, kick, kick_step)."""
    return batch["x0"][b], batch["v"][b], batch["states"][b], float(batch["kick"][b]), \
        batch["kick_step"]


def rollout_probe(key):
    """The oracle alone on one walk (a name of rollout_cases() or ("batch", b)): the largest
    |state| of its rollout, the response of CoM and feet to x0 + 1e-12, and whether
    HO.herdt_rollout gives the same arrays (None where its kick step, n // 2, is not the
    case's).  Module level so that a process pool can run it."""
    if isinstance(key, str):
        case = {c["name"]: c for c in rollout_cases()}[key]
        cfg = make_config(case["cfg_kw"])
        x0, v, st, kick, ks = case["x0"], case["v"], case["states"], case_kick(case), \
            case["kick_step"]
    else:
        batch = rollout_batch()
        cfg = make_config(batch["cfg_kw"])
        x0, v, st, kick, ks = batch_walk(batch, key[1])
    a = rollout_ref(cfg, x0, v, st, kick, ks)
    b = rollout_ref(cfg, x0 + 1e-12, v, st, kick, ks)
    same = None
    if isinstance(key, str) and ks in (-1, len(st) // 2):
        r = HO.herdt_rollout(cfg, x0[0], x0[1], v, st)
        same = all(np.array_equal(p, q) for p, q in zip(r, a))
    return dict(max_state=float(max(np.abs(a[1]).max(), np.abs(a[3]).max())),
                response=float(max(np.abs(a[0] - b[0]).max(), np.abs(a[2] - b[2]).max())),
                same=same)
