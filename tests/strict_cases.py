"""Seeded inputs and CPU references shared by the strict (ZMP box-QP) case tests: the host test of
the inputs and of the references alone, tests/test_strict_cases_host.py; the device tests,
tests/test_gpu_strict_cases.py; the stored long-horizon answers,
tests/golden/make_strict_cases_golden.py.  Not a test module.

Everything here is plain arrays.  The solvers it calls are the exact box-QP oracle
(oracle/zmp_oracle.py) and the C restatement of the device algorithm (oracle/strict_cpu.py).

Rollout cases: dict of zmax, zmin [B, n, 2], x0 [B, 2, 3], kick [B], kick_step [B] int64, kinds
(list of str), N, dt.  Window cases (cold steps): dict of x [B, 3], zmax, zmin [B, N], m [B],
N, dt.  Every case is drawn from np.random.default_rng with a seed derived from its name.
"""
import functools
import os
import zlib

import numpy as np

from oracle import zmp_oracle as O

G = 9.81
# (Q, R, h): the default weights first
WEIGHTS = ((1.0, 1e-6, 0.75), (1.0, 1e-9, 0.75), (0.1, 1e-3, 0.5), (1.0, 1e-2, 0.75))
FAMILIES = ("jitter", "narrow", "steps", "zigzag")
MIXED_KINDS = FAMILIES + ("pinned", "benign", "wide")
SMALL_HORIZONS = (1, 5, 8, 9, 33, 64, 65)
CHOL_M = {150: (0, 1, 16, 17, 32, 33, 48, 49, 64, 65, 128, 129, 150), 512: (129, 512, 128, 256)}
LQ_HORIZONS = (320, 321, 608, 609, 896, 897, 1600, 1601, 1888, 1889, 2176, 2177, 2464)
LQ_LIVE_MAX = 897            # cold solves beyond are stored (tests/golden/strict_cases.npz)
LQ_M = (20, 40, 60)          # pinned slots of the three windows of a long horizon
SCAN_HORIZONS = (512, 513, 960)
LQ_S = 8                     # csrc/dispatch.h: slots per LQ segment


def case_dt(N):
    """Sampling time of a case: 0.01 s at the small horizons (N <= 65) — the hostile walks start
    up to 0.5 m outside their boxes and a short horizon does not stabilise them, and 40 samples
    of 0.01 s keep the divergent mode's growth (time constant sqrt(h/g) = 0.23 .. 0.28 s) under
    e^1.8, so the oracle's own response to a 1e-12 change of x0 stays under 1e-10 (at
    dt = 1.5 / N it reached 2.9e-8 at N = 33 and 6.6e-10 at N = 64) — else the class rule
    1.5 / N."""
    return 0.01 if N <= 65 else 1.5 / N


def seed_of(name):
    return zlib.crc32(name.encode())


def _rng(name, *extra):
    return np.random.default_rng([seed_of(name), *extra])


# ----------------------------------------------------------------------------- bound families

def _walk(rng, n, step):
    return rng.uniform(-0.02, 0.02) + np.cumsum(rng.uniform(-step, step, n))


def _family_axis(rng, kind, n):
    """(centre [n], half-width [n]) of one axis."""
    if kind == "jitter":
        return _walk(rng, n, 0.02), rng.uniform(0.005, 0.06, n)
    if kind == "narrow":
        half = rng.uniform(0.0, 0.002, n)
        half[rng.permutation(n)[: (n + 1) // 2]] = 0.0
        return _walk(rng, n, 0.01), half
    if kind == "steps":
        c, hw = np.empty(n), np.empty(n)
        i, cc = 0, rng.uniform(-0.02, 0.02)
        while i < n:
            k = int(rng.integers(1, 12))
            c[i:i + k], hw[i:i + k] = cc, rng.uniform(0.0, 0.08)
            cc += rng.uniform(-0.3, 0.3)
            i += k
        return c, hw
    if kind == "zigzag":
        sign = 1.0 if rng.random() < 0.5 else -1.0
        return rng.uniform(-0.02, 0.02) + sign * (-1.0) ** np.arange(n) * \
            rng.uniform(0.1, 0.2, n), np.full(n, 0.01)
    if kind == "pinned":      # wide boxes, a zero-width (or 1e-4 m) sample every 5 to 9
        c, hw = _walk(rng, n, 0.001), np.full(n, 1.0)
        i = int(rng.integers(1, 6))
        while i < n:
            c[i] += 0.05 if rng.random() < 0.5 else -0.05
            hw[i] = 0.0 if rng.random() < 0.5 else 0.5e-4
            i += int(rng.integers(5, 10))
        return c, hw
    if kind == "wide":
        return _walk(rng, n, 0.02), np.full(n, 50.0)
    raise KeyError(kind)


_BENIGN = None


def _benign(rng, n):
    """n samples of the default walk's stepping phase (tests/golden/walk_n64.npz), rigidly
    shifted by up to 2 cm."""
    global _BENIGN
    if _BENIGN is None:
        d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                 "walk_n64.npz"))
        _BENIGN = d["zmax"].copy(), d["zmin"].copy()
    assert 45 + n <= len(_BENIGN[0])
    off = rng.uniform(-0.02, 0.02, 2)
    return _BENIGN[0][45:45 + n] + off, _BENIGN[1][45:45 + n] + off


def _one_walk(rng, kind, n):
    """(zmax [n,2], zmin [n,2], x0 [2,3], kick, kick_step) of one walk of a kind."""
    if kind == "benign":
        zx, zn = _benign(rng, n)
    else:
        ax = [_family_axis(rng, kind, n) for _ in range(2)]
        zx = np.stack([c + hw for c, hw in ax], axis=1)
        zn = np.stack([c - hw for c, hw in ax], axis=1)
    x0 = np.empty((2, 3))
    if kind in ("benign", "pinned"):
        x0[:, 0] = rng.uniform(-0.01, 0.01, 2) if kind == "benign" else rng.uniform(-0.05, 0.05, 2)
        x0[:, 1] = rng.uniform(-0.2, 0.2, 2)
        x0[:, 2] = 0.0
    else:
        x0[:, 0] = rng.uniform(-0.5, 0.5, 2)
        x0[:, 1] = rng.uniform(-1.0, 1.0, 2)
        x0[:, 2] = rng.uniform(-3.0, 3.0, 2)
    kick = rng.uniform(-0.3, 0.3)
    ks = int(rng.integers(n // 4, max(n // 4 + 1, 3 * n // 4)))
    return zx, zn, x0, kick, ks


def _stack(walks, kinds, N):
    zx, zn, x0, kick, ks = zip(*walks)
    return dict(zmax=np.stack(zx), zmin=np.stack(zn), x0=np.stack(x0), kick=np.array(kick),
                kick_step=np.array(ks, np.int64), kinds=list(kinds), N=N, dt=case_dt(N))


def rollout_case(family, N, B=6, n=40):
    """B walks of n samples of one family; the weights are not part of the case (the four
    weight points run the same inputs)."""
    name = f"{family}-N{N}-n{n}"
    return _stack([_one_walk(_rng(name, b), family, n) for b in range(B)], [family] * B, N)


def mixed_order():
    """The cycle of kinds of the mixed batch, fixed by seed."""
    return [MIXED_KINDS[i] for i in _rng("mixed-order").permutation(len(MIXED_KINDS))]


def mixed_case(B, N=64, n=40):
    """One batch whose consecutive walks cycle through the seven kinds (a cycle of 7: any two
    neighbours, the two 32-lane halves of a wave and any 64 consecutive walks differ in kind).
    Walk b depends on (N, n, b) alone, so a smaller batch is a prefix of a larger one."""
    order = mixed_order()
    kinds = [order[b % len(order)] for b in range(B)]
    name = f"mixed-N{N}-n{n}"
    return _stack([_one_walk(_rng(name, b), kinds[b], n) for b in range(B)], kinds, N)


# ----------------------------------------------------------------------------- pinned windows

def pinned_window(name, N, positions):
    """One cold window of N slots: boxes of ±1 m round a slow centre walk; the slots in
    `positions` are offset by ±5 cm and have width 0 or 1e-4 m.  x within ±5 cm, ±0.2 m/s."""
    rng = _rng(name)
    c, hw = _walk(rng, N, 0.0005), np.full(N, 1.0)
    pos = np.asarray(sorted(positions), np.int64)
    assert len(set(pos.tolist())) == len(pos) and (len(pos) == 0 or (0 <= pos[0] and pos[-1] < N))
    sign = np.where(rng.random(len(pos)) < 0.5, 1.0, -1.0)
    # runs of neighbours share a sign (a ±10 cm flip between adjacent slots every sample would
    # ask for jerks that throw the free slots past their ±1 m boxes)
    for i in range(1, len(pos)):
        if pos[i] - pos[i - 1] < 4:
            sign[i] = sign[i - 1]
    c[pos] += 0.05 * sign
    # width 1e-4 m only where neither neighbour is pinned: beside a pinned neighbour of the same
    # offset nothing pulls the slot to a bound and its optimum may lie inside the 1e-4 m
    narrow = (rng.random(len(pos)) < 0.5) & ~np.isin(pos - 1, pos) & ~np.isin(pos + 1, pos)
    hw[pos] = np.where(narrow, 0.5e-4, 0.0)
    x = np.array([c[0] + rng.uniform(-0.05, 0.05), rng.uniform(-0.2, 0.2), 0.0])
    return x, c + hw, c - hw


def _windows(wins, ms, N):
    x, zx, zn = zip(*wins)
    return dict(x=np.stack(x), zmax=np.stack(zx), zmin=np.stack(zn), m=np.array(ms), N=N,
                dt=1.5 / N)


def chol_positions(N, m, rng):
    """m positions for the reduced-Cholesky windows: slot 0 and slot N − 1 first, the rest drawn."""
    if m >= N:
        return np.arange(N)
    fixed = [p for p in (0, N - 1, 7, 8)][:m]
    rest = [p for p in rng.permutation(N) if p not in fixed]
    return np.array(sorted(fixed + rest[: m - len(fixed)]))


def chol_case(N):
    """The working-set sizes CHOL_M[N] in one launch (strict.hip reduced_solve: registers to
    m = 64 in four instantiations, packed LDS to 128, global scratch beyond)."""
    ms = CHOL_M[N]
    wins = []
    for i, m in enumerate(ms):
        name = f"pinned-chol-N{N}-m{m}-{i}"
        wins.append(pinned_window(name, N, chol_positions(N, m, _rng(name, 1))))
    return _windows(wins, ms, N)


def lq_positions(N, m, rng):
    """m positions at a long horizon: the first segment, across the first segment edge, the two
    segments before the last (the LDS checkpoints of a wave whose last pinned slot is in the last
    segment), segments in the middle (global checkpoints) and slot N − 1; the rest drawn."""
    NS = (N + LQ_S - 1) // LQ_S
    fixed = {1, 3, 7, 8, N - 1, (NS - 2) * LQ_S + 2, (NS - 3) * LQ_S + 5, (NS // 2) * LQ_S,
             (NS // 2) * LQ_S + 1, (NS // 3) * LQ_S + 6, (NS // 5) * LQ_S + 7}
    fixed = sorted(p for p in fixed if 0 <= p < N)
    rest = [p for p in rng.permutation(N) if p not in fixed]
    return np.array(sorted(fixed + rest[: m - len(fixed)]))


def lq_case(N, ms=LQ_M):
    wins = []
    for m in ms:
        name = f"pinned-lq-N{N}-m{m}"
        wins.append(pinned_window(name, N, lq_positions(N, m, _rng(name, 1))))
    return _windows(wins, ms, N)


def lq_rollout_case(N, n=6):
    """Three walks of n = 6 samples at a long horizon.  A rollout pads its bounds with the last
    sample, so only samples 1 .. n − 1 can differ: those carry pinned slots (first segment); the
    last sample, which fills the rest of every window, is wide on walks 0 and 2 and a box of
    ±4.5 cm, 5 cm off the centre, on walk 1, whose working set then reaches over the first 80 to
    150 slots of the horizon (N = 897; a box of ±1 cm pinned 600 slots and cost the exact oracle
    8 s)."""
    walks = []
    for b in range(3):
        rng = _rng(f"pinned-lq-rollout-N{N}-n{n}", b)
        zx, zn, x0, kick, _ = _one_walk(rng, "wide", n)
        c = _walk(rng, n, 0.0005)[:, None] + np.zeros((n, 2))
        hw = np.full((n, 2), 1.0)
        for a in range(2):
            for i in (1, 3, 4) if b != 1 else (2, 3):
                c[i, a] += 0.05 if rng.random() < 0.5 else -0.05
                hw[i, a] = 0.0 if (b != 2 and rng.random() < 0.5) else 0.5e-4
        if b == 1:
            c[-1] += np.array([0.05, -0.05])
            hw[-1] = 0.045
        x0 = np.zeros((2, 3))
        x0[:, 0] = c[0] + rng.uniform(-0.05, 0.05, 2)
        x0[:, 1] = rng.uniform(-0.2, 0.2, 2)
        walks.append((c + hw, c - hw, x0, kick, 2))
    out = _stack(walks, ["pinned"] * 3, N)
    out["dt"] = 1.5 / N
    return out


def nan_case(B=70, N=16, n=30, bad=37, since=12):
    """Benign boxes (the default walk's stepping phase, shifted); walk `bad` has NaN in zmax
    from sample `since` on.  → (case without the NaN, case with it)."""
    walks = [_one_walk(_rng(f"nan-N{N}-n{n}", b), "benign", n) for b in range(B)]
    good = _stack(walks, ["benign"] * B, N)
    poisoned = dict(good, zmax=good["zmax"].copy())
    poisoned["zmax"][bad, since:] = np.nan
    return good, poisoned


# ----------------------------------------------------------------------------- references

@functools.lru_cache(maxsize=None)
def matrices(N, dt, Q, R, h):
    H, V, Px, Pu = O.strict_matrices(N, dt, h, G, Q, R)
    A, Bv, _ = O.lipm(dt, h, G)
    for a in (H, Px, A, Bv):
        a.setflags(write=False)
    return H, Px, float(Pu[0, 0]), A, Bv


def solve_window(x, hi, lo, N, dt, weights=WEIGHTS[0]):
    """One cold strict solve by the exact oracle → (x_next [3], working set [N], KKT report)."""
    Q, R, h = weights
    H, Px, p0, A, Bv = matrices(N, dt, Q, R, h)
    u0, W, z, q = O.strict_u0(np.asarray(x, np.float64), hi, lo, H, Px, p0, Q)
    kkt = O.kkt_check(H, q, z, lo, hi, scale=max(1.0, float(np.abs(q).max())))
    return A @ x + Bv[:, 0] * u0, W, kkt


def solve_windows(case, weights=WEIGHTS[0]):
    """→ (x_next [B,3], working-set sizes [B], worst KKT residuals)."""
    out, m, worst = [], [], {}
    for x, hi, lo in zip(case["x"], case["zmax"], case["zmin"]):
        xn, W, kkt = solve_window(x, hi, lo, case["N"], case["dt"], weights)
        out.append(xn)
        m.append(int(np.count_nonzero(W)))
        for k, v in kkt.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return np.array(out), np.array(m), worst


def oracle_walk(case, b, weights=WEIGHTS[0], dx0=0.0, return_kkt=False):
    """The exact oracle's rollout of walk b → hist [n,2,3] (and the worst KKT residuals)."""
    Q, R, h = weights
    x0 = case["x0"][b] + dx0
    return O.rollout_strict(x0[0], x0[1], case["zmax"][b], case["zmin"][b], case["N"], case["dt"],
                            h, G, Q, R, kick=float(case["kick"][b]),
                            kick_step=int(case["kick_step"][b]), return_kkt=return_kkt)


def restatement(case, weights=WEIGHTS[0], threads=8):
    """The C restatement's rollout of the whole batch → (hist [B,n,2,3], status, passes).  It
    takes one kick step per call: the walks are grouped by theirs."""
    from oracle import strict_cpu
    Q, R, h = weights
    B, n = case["zmax"].shape[:2]
    hist = np.empty((B, n, 2, 3))
    status, passes = np.zeros(B, np.int32), np.zeros(B, np.uint64)
    for ks in np.unique(case["kick_step"]):
        idx = np.where(case["kick_step"] == ks)[0]
        hh, st, ps = strict_cpu.rollout_strict(case["zmax"][idx], case["zmin"][idx],
                                               case["x0"][idx], case["N"], case["dt"], h, G, Q, R,
                                               kick=case["kick"][idx], kick_step=int(ks),
                                               threads=threads)
        hist[idx], status[idx], passes[idx] = hh, st, ps
    return hist, status, passes


def walk_probe(job):
    """Pool worker: the exact oracle on one walk — its history, KKT report and, where asked, the
    response of the history to x0 + 1e-12."""
    case, b, weights, sens = job
    hist, kkt = oracle_walk(case, b, weights, return_kkt=True)
    resp = None
    if sens:
        resp = float(np.abs(oracle_walk(case, b, weights, dx0=1e-12) - hist).max())
    return hist, kkt, resp


def rel_err(a, ref):
    return float(np.abs(a - ref).max() / max(1.0, np.abs(ref).max()))
