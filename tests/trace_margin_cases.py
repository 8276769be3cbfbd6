"""Helpers shared by the tests of the trace margin (zmpc_trace_margin): tests/test_trace_margin_host.py
and tests/test_trace_margin_emulation.py on the CPU, tests/test_gpu_trace_margin.py on the device.
The fixed inputs, and the extended-precision statement of include/zmpc.h "The trace margin, stated
once": ρ from trace_cases.response in np.longdouble, the margins in double in the header's order,
the quotient in extended precision.  Not a test module."""
import functools

import numpy as np

import push_map_cases as pm
import trace_cases as tc

PAR150 = (150, 0.01, 0.75, 9.81, 1.0, 1e-6)  # the default walk's plan
HG = 0.75 / 9.81
BAR = 1e-11        # forms that compute the same solution (include/zmpc.h)
FAIR = 1e-12       # the double-precision reference against extended precision; an index is compared
                   # where the runner-up lies further off than this
DRAWS = (1, 3, 5)  # K; with four rows per workgroup the draws of a walk straddle workgroups
WALKS = {1: 8, 3: 3, 5: 2}  # B of a grid case by K: at least the eight start steps in B·K rows
AXES = ("x", "y", "xy")


def closed_loop_matrix(consts):
    """Ā = A − B·kxᵀ in double, entry by entry as the kernels form it."""
    T, T2, T3, kx = consts
    A = np.array([[1.0, T, T2], [0.0, 1.0, T], [0.0, 0.0, 1.0]])
    return A - np.outer(np.array([T3, T2, T]), kx)


def grid_case(n, L, axes, K, shared, ragged=False):
    """One case of the grid: B = WALKS[K] synthetic walks (push_map_cases.synthetic_case: the
    nominal test passes at t = 0 by construction) with K draws each, row r from start step
    emu_steps(n)[r % 8], dense noise of the strict scale.  ragged: lengths n − 1 − 2b (at least
    1), the dead tails NaN and garbage."""
    B = WALKS[K]
    R = B * K
    C = 2 if axes == "xy" else 1
    lengths = None
    if ragged:
        lengths = np.array([max(n - 1 - 2 * b, 1) for b in range(B)], np.int64)
    hist, zmax, zmin = pm.synthetic_case(n, shared, B, seed=K, lengths=lengths)
    dv = tc.STRICT_DENSE * np.random.default_rng([tc.SEED, n, L, C, K]).standard_normal((R, L, C))
    steps = tc.emu_steps(n)[np.arange(R) % 8]
    return dict(hist=hist, zmax=zmax, zmin=zmin, lengths=lengths, dv=dv, steps=steps, axes=axes,
                K=K, n=n, L=L, t=0.0)


def grid(n):
    """The cases of one n: every length of emu_lengths(n), one axis and two, K = 1, 3, 5,
    per-walk and shared bounds."""
    for L in tc.emu_lengths(n):
        for axes in AXES:
            for K in DRAWS:
                for shared in (False, True):
                    yield grid_case(n, L, axes, K, shared)


def ragged_cases():
    """The ragged variant: n = 129, L = 65, K = 3, both axes, per-walk and shared bounds."""
    return [grid_case(129, 65, "xy", 3, shared, ragged=True) for shared in (False, True)]


@functools.lru_cache(maxsize=None)
def _rho(n, L, axes, K, nbs, consts_key):
    """ρ [R, n, 2] in np.longdouble of the rows of grid_case(n, L, axes, K, ·): it does not depend
    on the bounds.  nbs: the walks' live lengths."""
    case = grid_case(n, L, axes, K, False)
    consts = (consts_key[0], consts_key[1], consts_key[2], np.array(consts_key[3:]))
    return rho_rows(case["dv"], case["steps"], nbs, n, K, consts, axes)


def rho_rows(dv, steps, nbs, n, K, consts, axes):
    """ρ [R, n, 2] in np.longdouble: row r's ZMP response at scale 1 over the n_b live samples of
    its walk b = r // K (zero beyond, and at or before the start step)."""
    R = len(dv)
    hg = np.longdouble(HG)
    out = np.zeros((R, n, 2), np.longdouble)
    for r in range(R):
        nb = int(nbs[r // K])
        d = tc.response(nb, dv[r], int(steps[r]), consts, axes)          # [nb, 2, 3]
        out[r, :nb] = -(d[:, :, 0] - hg * d[:, :, 2])
    return out


def extended(case, consts, rho=None):
    """The extended-precision statement → (scale [B, K, 2] np.longdouble, limit [B, K, 2] int32,
    gap [B, K, 2]: the relative distance of the runner-up candidate, inf where there is none, NaN
    for NaN entries).  Margins in double in the header's order, quotients in np.longdouble."""
    hist, zmax, zmin = case["hist"], case["zmax"], case["zmin"]
    B, n = hist.shape[:2]
    K, t = case["K"], case["t"]
    lengths = case["lengths"]
    nbs = [n if lengths is None else min(max(int(lengths[b]), 1), n) for b in range(B)]
    if rho is None:
        rho = rho_rows(case["dv"], case["steps"], nbs, n, K, consts, case["axes"])
    scale = np.full((B, K, 2), np.inf, np.longdouble)
    limit = np.full((B, K, 2), -1, np.int32)
    gap = np.full((B, K, 2), np.inf)
    for b in range(B):
        nb = nbs[b]
        hi = (zmax if zmax.ndim == 2 else zmax[b])[:nb]
        lo = (zmin if zmin.ndim == 2 else zmin[b])[:nb]
        st = hist[b, :nb]
        z = st[:, :, 0] - HG * st[:, :, 2]
        v = np.fmax(np.fmax(z - hi, lo - z), 0.0)
        if not np.isfinite(st).all() or (v > t).any():
            scale[b], gap[b] = np.nan, np.nan
            continue
        up = ((hi - z) + t).astype(np.longdouble)
        dn = ((z - lo) + t).astype(np.longdouble)
        for k in range(K):
            p = rho[b * K + k, :nb]
            pos, neg = p > 0, p < 0
            for col, (a, c) in enumerate(((up, dn), (dn, up))):
                f = np.full((nb, 2), np.inf, np.longdouble)
                f[pos] = a[pos] / p[pos]
                f[neg] = c[neg] / -p[neg]
                f = f.reshape(-1)
                j = int(np.argmin(f))
                if not f[j] < np.inf:
                    continue
                scale[b, k, col], limit[b, k, col] = f[j], j
                rest = np.delete(f, j)
                nxt = rest.min() if len(rest) else np.inf
                if nxt < np.inf:
                    gap[b, k, col] = float((nxt - f[j]) / f[j]) if f[j] > 0 else \
                        (np.inf if nxt > 0 else 0.0)
    return scale, limit, gap


def grid_extended(case, consts):
    """extended() of a grid case, with ρ cached across the bounds variants."""
    B, n = case["hist"].shape[:2]
    lengths = case["lengths"]
    nbs = tuple(n if lengths is None else min(max(int(lengths[b]), 1), n) for b in range(B))
    rho = None
    if lengths is None:
        key = tuple(float(c) for c in consts[:3]) + tuple(float(c) for c in consts[3])
        rho = _rho(n, case["L"], case["axes"], case["K"], nbs, key)
    return extended(case, consts, rho)


def compare(scale, limit, ref):
    """(worst relative error of the finite entries, same inf/NaN pattern, indices equal where the
    runner-up gap allows the comparison) of a result [B, K, 2] against extended()'s triple."""
    rs, rl, gap = ref
    scale = np.asarray(scale)
    fin = np.isfinite(rs.astype(np.float64))
    same = bool(np.array_equal(np.isnan(scale), np.isnan(rs.astype(np.float64))) and
                np.array_equal(np.isposinf(scale), np.isposinf(rs.astype(np.float64))))
    err = 0.0
    if fin.any() and same:
        a, b = scale[fin].astype(np.longdouble), rs[fin]
        err = float(np.max(np.abs(a - b) / np.maximum(np.abs(b), np.longdouble(1e-300))))
    fair = ~fin | (gap > FAIR)
    idx = bool(np.array_equal(np.asarray(limit)[fair], rl[fair]))
    return err, same, idx


# ----------------------------------------------------------------------------- the N = 64 walk

@functools.lru_cache(maxsize=None)
def walk64():
    """The stored N = 64 walk at its own plan (dt = 1.5/64, MPCConfig(horizon=64)'s): (zmax, zmin
    [n, 2], the oracle's unpushed history [n, 2, 3], closed_loop constants)."""
    d, par, kx, _, hist, _ = pm.walk("walk_n64.npz")
    zmax, zmin = np.ascontiguousarray(d["zmax"]), np.ascontiguousarray(d["zmin"])
    h = np.ascontiguousarray(hist[0])
    for a in (zmax, zmin, h):
        a.setflags(write=False)
    return zmax, zmin, h, tc.closed_loop(par, kx)


def walk64_draws():
    """The K = 4 draws of the bracket tests on the N = 64 walk, dv [4, n + 1, 2] from step 0: two
    dense draws, the sparse shoves, and a dense draw on the y axis alone."""
    n = len(walk64()[0])
    dv = np.zeros((4, n + 1, 2))
    dv[0, :n - 1] = tc.dense(n, 0, tc.STRICT_DENSE)
    dv[1, :n - 1] = tc.dense(n, 1, tc.STRICT_DENSE)
    dv[2] = tc.strict_sparse(n)
    dv[3, :n - 1, 1] = tc.dense(n, 2, tc.STRICT_DENSE)[:, 1]
    return dv


def walk64_case(t=1e-9):
    """walk64 with walk64_draws as a case of extended(): B = 1, K = 4."""
    zmax, zmin, h, _ = walk64()
    dv = walk64_draws()
    return dict(hist=h[None], zmax=zmax, zmin=zmin, lengths=None, dv=dv,
                steps=np.zeros(4, np.int64), axes="xy", K=4, n=len(zmax), L=dv.shape[1], t=t)
