"""Helpers shared by the tests of rollouts under per-walk traces (tests/test_trace_host.py and
tests/test_trace_emulation.py on the CPU, tests/test_gpu_trace.py on the device): the fixed inputs,
the oracle loops of tests/push_rollout_cases.py under them, and the extended-precision statement of
the unconstrained controller's response (include/zmpc.h, "The trace, stated once").  Not a test
module.

A trace here is (dv [L, C] in m/s, start step s): row j lowers the velocity of sample s + j + 1.
`table` spreads it into the dvel [n, 2] the oracle loops take (row i lowers sample i + 1, row
n − 1 is never applied)."""
import numpy as np

from oracle import zmp_oracle as O

import herdt_cases as hc
import push_rollout_cases as pr
import strict_cases as sc

SEED = 20261021
N_WALK = pr.N_WALK
STRICT_FAMILIES = ("jitter", "narrow")
STRICT_HORIZONS = pr.STRICT_HORIZONS
STRICT_WALKS = pr.STRICT_WALKS
STRICT_DENSE, HERDT_DENSE = 0.02, 0.004  # m/s, the standard deviation of a dense trace's entries
HERDT_BATCH = 0.012  # m/s, the same for the short traces of rollout_batch() (the sparse shoves' size)
HERDT_WALKS = ("n17_triangle", "seven")
BAR = 1e-9   # the oracle loops' response to x0 + 1e-12 stays below it on every case
MOVES = 1e-3  # m: every trace shifts the CoM by more than this


def rng_of(b):
    return np.random.default_rng([SEED, b])


def dense(n, b, scale):
    """dv [n − 1, 2] of walk b: scale·N(0, 1) on both axes at every step, from step 0."""
    return scale * rng_of(b).standard_normal((n - 1, 2))


def sparse(n, steps, shoves):
    """dv [n + 1, 2] from step 0: two-sample shoves of (x, y) m/s at the given history steps.  The
    rows n − 1 and n reach no sample: the trace runs past the walk's end and is truncated there;
    a shove at n − 3 fills the last two steps that are applied."""
    dv = np.zeros((n + 1, 2))
    for s, a in zip(steps, shoves):
        dv[s:s + 2] = a
    return dv


def strict_sparse(n=N_WALK):
    return sparse(n, (3, 17, n - 3), ((0.1, -0.05), (-0.08, 0.12), (0.05, 0.05)))


def herdt_sparse(n):
    return sparse(n, (2, n // 2, n - 3), ((0.012, -0.02), (-0.01, 0.02), (0.012, 0.012)))


def table(n, dv, s, axes="xy"):
    """dvel [n, 2] of one walk from its trace dv [L, C] at start step s (C columns of `axes`)."""
    out = np.zeros((n, 2))
    if not 0 <= s < n - 1:
        return out
    dv = np.asarray(dv, np.float64).reshape(len(dv), -1)
    k = min(len(dv), n - 1 - s)
    cols = {"x": (0,), "y": (1,), "xy": (0, 1)}[axes]
    for c, a in enumerate(cols):
        out[s:s + k, a] = dv[:k, c]
    return out


def strict_trace(kind, b, n=N_WALK):
    """(dv, start step) of walk b of a strict case."""
    return (dense(n, b, STRICT_DENSE), 0) if kind == "dense" else (strict_sparse(n), 0)


def strict_probe(job):
    """Pool worker: (family, N, kind) → over the first STRICT_WALKS walks, (the oracle loop's
    response to x0 + 1e-12 under the trace, the smallest CoM shift against the unpushed loop)."""
    family, N, kind = job
    case = sc.rollout_case(family, N, n=N_WALK)
    resp, shift = 0.0, np.inf
    for b in range(STRICT_WALKS):
        dv, s = strict_trace(kind, b)
        dvel = table(N_WALK, dv, s)
        a = pr.strict_walk(case, b, sc.WEIGHTS[0], dvel)
        c = pr.strict_walk(case, b, sc.WEIGHTS[0], dvel, dx0=1e-12)
        z = pr.strict_walk(case, b, sc.WEIGHTS[0], np.zeros((N_WALK, 2)))
        resp = max(resp, float(np.abs(a - c).max()))
        shift = min(shift, float(np.abs(a[..., 0] - z[..., 0]).max()))
    return resp, shift


def herdt_trace(kind, n, b=0):
    return (dense(n, b, HERDT_DENSE), 0) if kind == "dense" else (herdt_sparse(n), 0)


def herdt_batch_traces(n, B):
    """The traces of the walks of herdt_cases.rollout_batch(): dv [B, L, 2] with L = 12 — noise
    of HERDT_BATCH m/s of walk b over its first 4 + b % 9 rows, zeros after — and pr.herdt_batch_steps'
    start steps (walk 5 outside the range, the last walk truncated by its end)."""
    L = 12
    dv = np.zeros((B, L, 2))
    for b in range(B):
        k = 4 + b % 9
        dv[b, :k] = dense(L + 1, b, HERDT_BATCH)[:k]
    return dv, pr.herdt_batch_steps(n, B)


def herdt_probe(key):
    """Pool worker: (walk name, kind) or ("batch", b) → (response of CoM and feet of the pushed
    loop to x0 + 1e-12, CoM shift against the unpushed loop)."""
    if key[0] == "batch":
        batch = hc.rollout_batch()
        cfg = hc.make_config(batch["cfg_kw"])
        b, n = key[1], batch["n"]
        x0, v, st = batch["x0"][b], batch["v"][b], batch["states"][b]
        dv, steps = herdt_batch_traces(n, len(batch["x0"]))
        dvel = table(n, dv[b], int(steps[b]))
    else:
        case = pr.herdt_case(key[0])
        cfg = hc.make_config(case["cfg_kw"])
        x0, v, st, n = case["x0"], case["v"], case["states"], case["n"]
        dvel = table(n, *herdt_trace(key[1], n))
    a = pr.herdt_rollout_pushed(cfg, x0, v, st, dvel)
    c = pr.herdt_rollout_pushed(cfg, x0 + 1e-12, v, st, dvel)
    z = pr.herdt_rollout_pushed(cfg, x0, v, st, np.zeros_like(dvel))
    return (float(max(np.abs(a[0] - c[0]).max(), np.abs(a[2] - c[2]).max())),
            float(np.abs(a[0] - z[0]).max()))


# ----------------------------------------------------------------------------- unconstrained

def closed_loop(par, kx=None):
    """(T, T²/2, T³/6, kx [3]) of a plan's parameters par = (N, dt, h, g, Q, R), in double as the
    library evaluates them."""
    N, dt, h, g, Q, R = par
    if kx is None:
        kx = O.gain_row(N, dt, h, g, Q, R)[1]
    return dt, dt ** 2 / 2.0, dt ** 3 / 6.0, np.asarray(kx, np.float64)


def response(n, dv, s, consts, axes="xy"):
    """δ [n, 2, 3] in np.longdouble of one walk: δ_i = 0 for i <= s, δ_(i+1) = Ā·δ_i + e1·dv[i − s]
    with Ā = A − B·kxᵀ formed in extended precision from the double constants."""
    T, T2, T3, kx = (np.longdouble(c) if np.ndim(c) == 0 else np.asarray(c, np.longdouble)
                     for c in consts)
    A = np.array([[1, T, T2], [0, 1, T], [0, 0, 1]], np.longdouble)
    Bv = np.array([T3, T2, T], np.longdouble)
    Abar = A - np.outer(Bv, kx)
    dvel = table(n, dv, s, axes).astype(np.longdouble)
    d = np.zeros((n, 2, 3), np.longdouble)
    for i in range(n - 1):
        for a in range(2):
            d[i + 1, a] = Abar @ d[i, a]
            d[i + 1, a, 1] += dvel[i, a]
    return d


def traced_reference(h0, dv, steps, consts, axes="xy"):
    """h0 [B, n, 2, 3] minus the walks' responses, in np.longdouble; dv [B, L, C], steps [B]."""
    B, n = h0.shape[:2]
    return np.stack([np.asarray(h0[b], np.longdouble)
                     - response(n, dv[b], int(steps[b]), consts, axes) for b in range(B)])


def emu_steps(n):
    return np.array([0, 1, 62, 63, 64, n - 2, n - 1, -1], np.int64)


def emu_lengths(n):
    return sorted({1, 2, 64, 65, max(n - 1, 1), n + 5})


EMU_N = (2, 3, 64, 65, 129, 200)


def grid_dv(n, L, axes):
    """dv [8, L, C] of the eight start steps of emu_steps(n): dense noise of the strict scale."""
    C = 2 if axes == "xy" else 1
    return STRICT_DENSE * np.random.default_rng([SEED, n, L, C]).standard_normal((8, L, C))
