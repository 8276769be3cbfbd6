"""Helpers shared by the tests of shaped and two-axis pushes (tests/test_push_shaped_host.py on
the CPU, tests/test_gpu_push_shaped.py on the device).  Not a test module."""
import numpy as np

from oracle import zmp_oracle as O

AXIS_LIMIT = 10112  # csrc/dispatch.h choose_push_shaped: the longest full map, one axis or two


def half_sine(D):
    """D weights of a half-sine bump sampled at the middle of each step, peak 1."""
    return np.sin(np.pi * (np.arange(D) + 0.5) / D)


def profile_of(kind, D):
    return None if kind == "ones" else half_sine(D)


def swap_axes(hist, zmax, zmin):
    """The same walks with x and y exchanged."""
    return (np.ascontiguousarray(hist[:, :, ::-1, :]), np.ascontiguousarray(zmax[..., ::-1]),
            np.ascontiguousarray(zmin[..., ::-1]))


def chained_histories(zmax, zmin, par, dvel):
    """Oracle histories of one walk under velocity kicks at many samples, by chained
    O.rollout_gain segments: scenario b restarts at every sample q that any scenario kicks, from
    the state of sample q lowered by dvel[b, q, axis] in its velocity, with the bounds sliced from
    q (a segment is rolled only as far as the next restart needs: its windows reach N samples
    ahead).  dvel [S, n, 2]; every scenario takes the same segments, so a scenario with no kick
    is the unpushed walk computed the same way.  → hist [S, n, 2, 3]."""
    N = par[0]
    S, n = dvel.shape[:2]
    stops = [int(q) for q in np.nonzero(np.any(dvel != 0, axis=(0, 2)))[0]]
    assert all(1 <= q <= n - 1 for q in stops)
    hist = np.empty((S, n, 2, 3))
    x0, start = np.zeros((S, 2, 3)), 0
    for q in stops + [None]:
        end = n if q is None else min(n, q + N)  # rows the windows of steps start … q − 1 read
        hi = np.broadcast_to(zmax[start:end], (S, end - start, 2))
        lo = np.broadcast_to(zmin[start:end], (S, end - start, 2))
        seg = O.rollout_gain(hi, lo, x0, *par)
        upto = n if q is None else q
        hist[:, start:upto] = seg[:, :upto - start]
        if q is None:
            break
        x0 = seg[:, q - start].copy()
        x0[:, :, 1] -= dvel[:, q, :]
        start = q
    return hist


def kicks_of(n, s, w, axis, dt, m):
    """dvel [n, 2] of a unit push with weights w_j during steps s + j on `axis`: the velocity of
    sample s + j + 1 drops by dt·w_j/m; the part past the walk's end is dropped."""
    dv = np.zeros((n, 2))
    for j, wj in enumerate(w):
        if s + j + 1 <= n - 1:
            dv[s + j + 1, axis] = dt * wj / m
    return dv


def summation_bound(r, D, w):
    """Per delay 2·(D + 1)·2⁻⁵³·Σ_j |w_j·r_(d−j)|: twice the standard bound of a D-term sum of
    rounded products, whatever the order."""
    n = len(r)
    tot = np.zeros(n)
    for j in range(min(D, n)):
        tot[j:] += np.abs((1.0 if w is None else w[j]) * r[:n - j])
    return 2.0 * (D + 1) * 2.0 ** -53 * tot
