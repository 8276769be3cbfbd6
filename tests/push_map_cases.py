"""Seeded inputs and helpers shared by the push-map tests (tests/test_push_map_host.py on the CPU,
tests/test_gpu_push_map.py on the device).  Not a test module."""
import numpy as np

from conftest import golden
from oracle import zmp_oracle as O

HG = 0.75 / 9.81
WALKS = ("walk_n64.npz", "walk_n10.npz", "walk_n150.npz", "walk_n512.npz")


def walk(name):
    """A stored walk with its closed loop: (d, par, kx, r, hist, hg) — the file, its
    (N, dt, h, g, Q, R) at the weights stored in it, the oracle's state gain, the NumPy response
    table over the walk's n samples and the oracle's unpushed history [1, n, 2, 3]."""
    from mpc_bipedal.analysis import push_response
    d = golden(name)
    par = (int(d["horizon"]), float(d["dt"]), float(d["h"]), float(d["g"]), float(d["Q"]),
           float(d["R"]))
    N, dt, h, g, Q, R = par
    n = d["zmax"].shape[0]
    _, kx = O.gain_row(*par)
    A, B, C = O.lipm(dt, h, g)
    r = push_response(A, B, kx, C, dt, float(d["m"]), n)
    hist = O.rollout_gain(d["zmax"][None], d["zmin"][None], np.zeros((1, 2, 3)), *par)
    return d, par, kx, r, hist, h / g


def synthetic_case(n, shared, B, seed=0, lengths=None):
    """Random state histories (not rollouts) of O(0.1) magnitude with boxes placed round each
    uncontracted ZMP sample at margins between 0 and 5 cm on either side and axis, so that the
    nominal test passes by construction at max_violation = 0 (per-walk bounds), or with boxes
    that hold every walk's ZMP (shared bounds).  → hist [B,n,2,3], zmax, zmin [B,n,2] or [n,2].
    With `lengths` the dead tails hold NaN and garbage states that no box holds, and garbage
    per-walk bounds."""
    hg = HG
    rng = np.random.default_rng([20261020, n, int(shared), B, seed])
    hist = rng.uniform(-1.0, 1.0, (B, n, 2, 3)) * np.array([0.1, 0.5, 1.0])
    z = hist[..., 0] - hg * hist[..., 2]
    up = rng.uniform(0.0, 0.05, (B, n, 2))
    dn = rng.uniform(0.0, 0.05, (B, n, 2))
    zmax, zmin = z + up, z - dn
    # rounding of z + up may leave z − zmax a last bit above 0: push those boxes out by an ulp
    zmax = np.where(z - zmax > 0, np.nextafter(zmax, np.inf), zmax)
    zmin = np.where(zmin - z > 0, np.nextafter(zmin, -np.inf), zmin)
    if shared:
        live = np.ones((B, n), bool)
        if lengths is not None:
            live = np.arange(n)[None, :] < np.asarray(lengths)[:, None]
        zmax = np.where(live[..., None], zmax, -np.inf).max(axis=0)
        zmin = np.where(live[..., None], zmin, np.inf).min(axis=0)
        zmax = np.where(np.isfinite(zmax), zmax, 1.0)
        zmin = np.where(np.isfinite(zmin), zmin, -1.0)
    if lengths is not None:
        for b, nb in enumerate(lengths):
            hist[b, nb:] = rng.choice([np.nan, 1e300, -7.0], size=(n - nb, 2, 3))
            if not shared:
                zmax[b, nb:] = rng.choice([0.0, -1e9, 3.0], size=(n - nb, 2))
                zmin[b, nb:] = rng.choice([0.0, 1e9, -3.0], size=(n - nb, 2))
    return hist, zmax, zmin


def synthetic_response(n, seed=0):
    """A response table with both signs, exact zeros and a wide range: r_0 = r_1 = 0, then a
    decaying oscillation with every seventh entry zeroed."""
    rng = np.random.default_rng([20261021, n, seed])
    d = np.arange(n)
    r = 1e-3 * np.cos(0.37 * d + rng.uniform(0, 6)) * 0.995 ** d * rng.uniform(0.2, 1.0, n)
    r[::7] = 0.0
    r[:2] = 0.0
    return r


def quiet_walk(n):
    """One walk at rest at the origin in a ±0.1 box: z0 = 0 everywhere, margins 0.1.
    → hist [1,n,2,3], zmax, zmin [1,n,2] to plant samples in."""
    return np.zeros((1, n, 2, 3)), np.full((1, n, 2), 0.1), np.full((1, n, 2), -0.1)


def runner_up_gap(hist, zmax, zmin, r, hg, lengths=None, max_violation=0.0):
    """Per finite map entry the relative gap between the minimum and the runner-up candidate
    (inf where one sample alone constrains the push) → [B, n, 2], NaN elsewhere.  An index
    comparison is fair where the gap exceeds the rounding of the candidates."""
    hist = np.asarray(hist, np.float64)
    zmax, zmin = np.asarray(zmax, np.float64), np.asarray(zmin, np.float64)
    B, n = hist.shape[:2]
    gap = np.full((B, n, 2), np.nan)
    t = max_violation
    for b in range(B):
        nb = n if lengths is None else min(max(int(lengths[b]), 1), n)
        hi = (zmax if zmax.ndim == 2 else zmax[b])[:nb, 1]
        lo = (zmin if zmin.ndim == 2 else zmin[b])[:nb, 1]
        z = hist[b, :nb, 1, 0] - hg * hist[b, :nb, 1, 2]
        up, dn = (hi - z) + t, (z - lo) + t
        for s in range(nb - 2):
            rd = r[1:nb - s]
            for k, (a, c) in enumerate(((up[s + 1:], dn[s + 1:]), (dn[s + 1:], up[s + 1:]))):
                f = np.full(rd.shape, np.inf)
                with np.errstate(over="ignore"):
                    f[rd > 0] = a[rd > 0] / rd[rd > 0]
                    f[rd < 0] = c[rd < 0] / -rd[rd < 0]
                f = np.partition(f, 1)[:2] if len(f) > 1 else f  # the two smallest, in order
                if f[0] < np.inf:
                    if len(f) < 2 or f[1] == np.inf:
                        gap[b, s, k] = np.inf
                    elif f[0] == 0:
                        gap[b, s, k] = np.inf if f[1] > 0 else 0.0
                    else:
                        gap[b, s, k] = (f[1] - f[0]) / f[0]
    return gap


def residual(F, s, sign, z0, zmax, zmin, r, t):
    """g(F) = max_i max(z0_i + σF·r_d − zmax_i, zmin_i − z0_i − σF·r_d) − t over the samples
    behind step s of one walk's y axis: 0 at the critical push."""
    i = np.arange(s + 1, len(z0))
    z = z0[i] + sign * F * r[i - s]
    return np.max(np.maximum(z - zmax[i], zmin[i] - z)) - t
