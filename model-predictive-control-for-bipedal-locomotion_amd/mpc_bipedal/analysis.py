"""Per-walk robustness metrics of a rollout: did the ZMP stay inside the support box?

The reference answers that by plotting ``C·state`` (run_mpc.py:294) over the CoP bounds
(run_compare_resistance.py:173-197) and looking.  Here the state history stays on the device
and ``zmpc_walk_metrics`` (``include/zmpc.h``, ``csrc/metrics.hip``) reduces it to twelve numbers
per walk.  This module names those numbers (``SLOT_NAMES``, ``WalkMetrics``), states them once
more in plain NumPy (``walk_metrics_reference``: the checker of the kernel, not a fallback — the
library never calls it) and gives the closed form of the largest push an affine response
survives (``critical_force_affine``), the cross-check of ``ZMPController.critical_force``.

For the unconstrained controller that closed form is the product itself: the response depends
only on the delay between push and sample (``push_response``), and ``zmpc_push_map``
(``csrc/pushmap.hip``) evaluates it for every push step and both directions of an unpushed
history.  ``push_map_reference`` is that map in NumPy (again the checker, never a fallback) and
``PushMap`` names its outputs.
"""

import numpy as np

NMETRICS = 12  # include/zmpc.h ZMPC_NMETRICS
# quantity k of axis a (0: x, 1: y) is slot 2k + a
SLOT_NAMES = ("viol_max", "viol_argmax", "viol_count", "com_dev_max", "zmp_rms", "dcm_end")


class WalkMetrics:
    """Named [B, 2] columns (x, y) over a [B, 12] metrics tensor or array; views, no copies.

    viol_max     largest excursion of the ZMP beyond its sample's support box (0: none)
    viol_argmax  first sample that attains it (−1: none), as a float
    viol_count   samples outside the box
    com_dev_max  largest distance of the CoM from the box centre
    zmp_rms      RMS distance of the ZMP from the box centre
    dcm_end      divergent component of motion c + ċ·sqrt(h/g) at the last sample, relative to
                 the final box centre
    An axis that met a non-finite state reports viol_max = +inf, viol_argmax = the first such
    sample and NaN elsewhere."""

    __slots__ = ("data",)

    def __init__(self, data):
        if data.ndim != 2 or data.shape[1] != NMETRICS:
            raise ValueError(f"metrics must be [B, {NMETRICS}], got {tuple(data.shape)}")
        self.data = data

    def __getattr__(self, name):
        try:
            k = SLOT_NAMES.index(name)
        except ValueError:
            raise AttributeError(name) from None
        return self.data[:, 2 * k:2 * k + 2]

    def __len__(self):
        return int(self.data.shape[0])

    def __repr__(self):
        return f"WalkMetrics(B={len(self)}, slots={SLOT_NAMES})"


def walk_metrics_reference(hist, zmax, zmin, hg, lengths=None):
    """The table of include/zmpc.h zmpc_walk_metrics in NumPy, walk by walk → [B, 12].

    hist [B, n, 2, 3]; zmax, zmin [B, n, 2] or a shared [n, 2]; hg = h/g; lengths [B] or None."""
    hist = np.asarray(hist, np.float64)
    zmax = np.asarray(zmax, np.float64)
    zmin = np.asarray(zmin, np.float64)
    B, n = hist.shape[:2]
    out = np.empty((B, NMETRICS))
    root = np.sqrt(hg)
    for b in range(B):
        nb = n if lengths is None else int(lengths[b])
        hi = (zmax if zmax.ndim == 2 else zmax[b])[:nb]
        lo = (zmin if zmin.ndim == 2 else zmin[b])[:nb]
        for a in range(2):
            s = hist[b, :nb, a, :]
            bad = ~np.isfinite(s).all(axis=1)
            if bad.any():
                out[b, a::2] = np.nan
                out[b, a] = np.inf
                out[b, 2 + a] = float(np.argmax(bad))
                continue
            c, cd, cdd = s[:, 0], s[:, 1], s[:, 2]
            z = c - hg * cdd
            zr = (hi[:, a] + lo[:, a]) * 0.5
            v = np.maximum(np.maximum(z - hi[:, a], lo[:, a] - z), 0.0)
            vmax = v.max()
            out[b, a] = vmax
            out[b, 2 + a] = float(np.argmax(v)) if vmax > 0 else -1.0
            out[b, 4 + a] = float(np.count_nonzero(v > 0))
            out[b, 6 + a] = np.abs(c - zr).max()
            out[b, 8 + a] = np.sqrt(np.mean((z - zr) ** 2))
            out[b, 10 + a] = c[-1] + cd[-1] * root - zr[-1]
    return out


def push_response(A, B, kx, C, dt, m, n):
    """ZMP response of the unconstrained closed loop to a unit push, by delay → r [n].

    The closed loop is x⁺ = Ā x + B f with Ā = A − B·kxᵀ and f independent of the state, so a
    push of +1 N at history step s (the y velocity of sample s + 1 drops by dt/m,
    zmp_controller.py:105-106) moves the ZMP of sample i = s + d by
    r_d = −(dt/m)·C·Ā^(d−1)·e1 for d >= 1 and r_0 = 0, whatever s and whatever the walk.
    r_1 is exactly 0: a velocity kick moves neither c nor c̈ of the next sample."""
    A = np.asarray(A, np.float64).reshape(3, 3)
    Abar = A - np.outer(np.asarray(B, np.float64).reshape(3), np.asarray(kx, np.float64).reshape(3))
    C = np.asarray(C, np.float64).reshape(3)
    r = np.zeros(int(n))
    v = np.array([0.0, 1.0, 0.0])
    for d in range(1, int(n)):
        r[d] = -(dt / m) * (C @ v)
        v = Abar @ v
    return r


def push_map_reference(hist, zmax, zmin, r, hg, lengths=None, max_violation=0.0, push_steps=None):
    """The statement of include/zmpc.h zmpc_push_map in NumPy, with division: the checker of the
    kernels, never a fallback → (force, limit).

    hist [B, n, 2, 3] (unpushed, or already pushed: the entries are then the largest additional
    push); zmax, zmin [B, n, 2] or a shared [n, 2]; r [n] the response by delay (push_response,
    or the device's own table); hg = h/g; lengths [B] live samples or None.  push_steps None:
    force [B, n, 2] float64 and limit [B, n, 2] int32 — entry [b, s, 0] for a +y push at step s,
    [b, s, 1] for −y; push_steps [B]: the [B, 2] rows of those steps (a step outside
    [0, n_b − 2) gives +inf and −1)."""
    hist = np.asarray(hist, np.float64)
    zmax = np.asarray(zmax, np.float64)
    zmin = np.asarray(zmin, np.float64)
    r = np.asarray(r, np.float64)
    B, n = hist.shape[:2]
    t = float(max_violation)
    force = np.full((B, n, 2), np.inf)
    limit = np.full((B, n, 2), -1, np.int32)
    for b in range(B):
        nb = n if lengths is None else min(max(int(lengths[b]), 1), n)
        hi = (zmax if zmax.ndim == 2 else zmax[b])[:nb]
        lo = (zmin if zmin.ndim == 2 else zmin[b])[:nb]
        s = hist[b, :nb]
        z = s[:, :, 0] - hg * s[:, :, 2]                                 # [nb, 2]
        v = np.fmax(np.fmax(z - hi, lo - z), 0.0)
        if not np.isfinite(s).all() or (v > t).any():
            force[b] = np.nan
            continue
        up = (hi[:, 1] - z[:, 1]) + t
        dn = (z[:, 1] - lo[:, 1]) + t
        for st in range(nb - 2):
            rd = r[1:nb - st]                                            # delays of i = st+1 …
            u, d = up[st + 1:], dn[st + 1:]
            pos, neg = rd > 0, rd < 0
            for k, (a, c) in enumerate(((u, d), (d, u))):                # +y: up limits r > 0
                f = np.full(rd.shape, np.inf)
                with np.errstate(over="ignore"):  # (a denormal response: margin/r = +inf)
                    f[pos] = a[pos] / rd[pos]
                    f[neg] = c[neg] / -rd[neg]
                j = int(np.argmin(f))                                    # the first minimum
                if f[j] < np.inf:
                    force[b, st, k] = f[j]
                    limit[b, st, k] = st + 1 + j
    if push_steps is None:
        return force, limit
    f1 = np.full((B, 2), np.inf)
    l1 = np.full((B, 2), -1, np.int32)
    for b in range(B):
        nb = n if lengths is None else min(max(int(lengths[b]), 1), n)
        st = int(push_steps[b])
        if 0 <= st < nb - 2:
            f1[b], l1[b] = force[b, st], limit[b, st]
        elif np.isnan(force[b, 0, 0]):
            f1[b] = np.nan
    return f1, l1


class PushMap:
    """The push-robustness map of a batch of walks: ``force`` [B, n, 2] (N; [..., 0] a +y push,
    [..., 1] a −y push, at history step s) and ``limit`` [B, n, 2] (int32, the sample that leaves
    its box first, −1 where no sample does or the walk fails unpushed), tensors or arrays; views,
    no copies.  ``response`` [n] is the ZMP response by delay when it was asked for."""

    __slots__ = ("force", "limit", "response")

    def __init__(self, force, limit, response=None):
        if force.ndim != 3 or force.shape[2] != 2 or tuple(limit.shape) != tuple(force.shape):
            raise ValueError(f"force and limit must both be [B, n, 2], got {tuple(force.shape)} "
                             f"and {tuple(limit.shape)}")
        self.force, self.limit, self.response = force, limit, response

    def __len__(self):
        return int(self.force.shape[0])

    def __repr__(self):
        return f"PushMap(B={len(self)}, n={int(self.force.shape[1])})"

    def weakest(self):
        """Per walk the smallest critical push and where it acts → (force [B], step [B],
        direction [B]: +1 or −1).  A walk that fails unpushed gives NaN, and one that no push
        topples +inf, both with step −1 and direction 0."""
        f = self.force
        flat = f.reshape(f.shape[0], -1)
        if hasattr(flat, "detach"):  # torch
            import torch
            filled = torch.where(torch.isnan(flat), torch.full_like(flat, float("inf")), flat)
            val, idx = filled.min(dim=1)
            val = torch.where(torch.isnan(flat).any(dim=1), torch.full_like(val, float("nan")),
                              val)
            none = ~torch.isfinite(val)
            step = torch.where(none, torch.full_like(idx, -1), idx // 2)
            direction = torch.where(none, torch.zeros_like(idx), 1 - 2 * (idx % 2))
            return val, step, direction
        nan = np.isnan(flat)
        filled = np.where(nan, np.inf, flat)
        idx = filled.argmin(axis=1)
        val = np.where(nan.any(axis=1), np.nan, filled[np.arange(flat.shape[0]), idx])
        none = ~np.isfinite(val)
        return val, np.where(none, -1, idx // 2), np.where(none, 0, 1 - 2 * (idx % 2))


def critical_force_affine(z0, r, zmax, zmin, max_violation=0.0):
    """Largest F >= 0 with zmin − max_violation <= z0 + F·r <= zmax + max_violation at every
    sample: the push an affine ZMP response survives (the unconstrained controller is linear, so
    its ZMP is z0, the unpushed walk's, plus F times the response r to a unit push).

    z0, r, zmax, zmin: [..., n] arrays → [...]; NaN where the walk fails at F = 0, +inf where no
    sample ever leaves (r = 0 everywhere)."""
    z0, r, zmax, zmin = (np.asarray(x, np.float64) for x in (z0, r, zmax, zmin))
    up = zmax + max_violation - z0  # room towards the upper bound, >= 0 for a passing walk
    dn = z0 - (zmin - max_violation)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(r > 0, up / r, np.where(r < 0, dn / -r, np.inf))
    out = f.min(axis=-1)
    return np.where(((up < 0) | (dn < 0)).any(axis=-1), np.nan, out)
