"""Per-walk robustness metrics of a rollout: did the ZMP stay inside the support box?

The reference answers that by plotting ``C·state`` (run_mpc.py:294) over the CoP bounds
(run_compare_resistance.py:173-197) and looking.  Here the state history stays on the device
and ``zmpc_walk_metrics`` (``include/zmpc.h``, ``csrc/metrics.hip``) reduces it to twelve numbers
per walk.  This module names those numbers (``SLOT_NAMES``, ``WalkMetrics``), states them once
more in plain NumPy (``walk_metrics_reference``: the checker of the kernel, not a fallback — the
library never calls it) and gives the closed form of the largest push an affine response
survives (``critical_force_affine``), the cross-check of ``ZMPController.critical_force``.
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
