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

A push that lasts several samples, with or without a force profile, has the response
``shaped_response``; the x axis runs the same closed loop, and the axes decouple.
``zmpc_push_map_shaped`` (``csrc/pushmap.hip``) evaluates that on either axis or both,
``push_map_shaped_reference`` is its checker, and ``PushMap.weakest_push`` and ``PushMap.rose``
(``planar_push``) read the columns (+x, −x, +y, −y), the latter along any planar direction.

``Push`` describes the shove itself — force, direction, start step, duration, profile — for the
pushed rollouts of every controller (``zmpc_rollout_pushed``, ``zmpc_herdt_rollout_pushed``;
``Plan.rollout(push=)``, the batch methods of ``ZMPController``).  ``PushTrace`` is the general
disturbance: a force per walk, sample and axis (``zmpc_rollout_traced``,
``zmpc_herdt_rollout_traced``; ``Plan.rollout(trace=)``).

A Herdt walk has no fixed CoP bounds: ``zmpc_herdt_walk_metrics`` (``csrc/herdt_metrics.hip``)
rebuilds the support box from the feet the QP chose and adds the divergent component of motion
relative to the supporting foot, the quantity that tells whether the robot fell.
``HerdtWalkMetrics`` names its sixteen numbers and ``herdt_walk_metrics_reference`` states them in
NumPy (the checker, never a fallback).
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


NHERDT_METRICS = 16  # include/zmpc.h ZMPC_NHERDT_METRICS
# quantity k of axis a is slot 2k + a; slots 14 and 15 are per walk
HERDT_SLOT_NAMES = ("viol_max", "viol_argmax", "viol_count", "com_dev_max", "dcm_dev_max",
                    "dcm_end", "step_shift_max")
HERDT_WALK_SLOTS = {"reach_slack_min": 14, "steps_landed": 15}


class HerdtWalkMetrics:
    """Named columns over a [B, 16] tensor or array of zmpc_herdt_walk_metrics; views, no copies.
    [B, 2] (x, y) each, every one relative to the supporting foot fs_i = foot[max(i − 1, 0)]:

    viol_max        largest excursion of the ZMP beyond the support box the QP held it to (the
                    ZMP sits on the box edge by design: rounding noise, never the verdict)
    viol_argmax     first sample that attains it (−1: none), as a float
    viol_count      samples further out than count_tol
    com_dev_max     largest distance of the CoM from the supporting foot
    dcm_dev_max     largest distance of the divergent component of motion c + ċ·sqrt(h/g) from
                    the supporting foot: the survival quantity
    dcm_end         that component at the last sample, signed
    step_shift_max  largest distance of a foot from the nominal walk's (0 without foot_ref)
    and [B] each:
    reach_slack_min smallest slack a landed step left on its swing polytope (+inf: no landing
                    or no facets; 0: the step reached as far as it could)
    steps_landed    landings
    An axis that met a non-finite value reports viol_max = +inf, viol_argmax = the first such
    sample and NaN elsewhere; reach_slack_min is then NaN."""

    __slots__ = ("data",)

    def __init__(self, data):
        if data.ndim != 2 or data.shape[1] != NHERDT_METRICS:
            raise ValueError(f"metrics must be [B, {NHERDT_METRICS}], got {tuple(data.shape)}")
        self.data = data

    def __getattr__(self, name):
        if name in HERDT_WALK_SLOTS:
            return self.data[:, HERDT_WALK_SLOTS[name]]
        try:
            k = HERDT_SLOT_NAMES.index(name)
        except ValueError:
            raise AttributeError(name) from None
        return self.data[:, 2 * k:2 * k + 2]

    def __len__(self):
        return int(self.data.shape[0])

    def __repr__(self):
        return (f"HerdtWalkMetrics(B={len(self)}, slots={HERDT_SLOT_NAMES + tuple(HERDT_WALK_SLOTS)})")


def herdt_walk_metrics_reference(hist, foot, states, hg, foot_length, foot_width, foot_spread,
                                 facets=(None, None), lengths=None, foot_ref=None,
                                 count_tol=1e-9):
    """The statement of include/zmpc.h zmpc_herdt_walk_metrics in NumPy, walk by walk → [B, 16]:
    the checker of the kernel, never a fallback.

    hist [B, n, 2, 3]; foot [B, n, 2]; states [B, n] or a shared [n] int8 codes (0 STANDING,
    2 SINGLE_SUPPORT); hg = h/g; facets: per side (left, right) an [F, 3] array of rows
    (a_x, a_y, b) or None; lengths [B] or None; foot_ref [B, n, 2], a shared [n, 2] or None."""
    hist = np.asarray(hist, np.float64)
    foot = np.asarray(foot, np.float64)
    states = np.asarray(states)
    B, n = hist.shape[:2]
    out = np.empty((B, NHERDT_METRICS))
    root = np.sqrt(hg)
    half = (0.5 * foot_length, 0.5 * foot_width)
    fac = [np.zeros((0, 3)) if f is None else np.asarray(f, np.float64).reshape(-1, 3)
           for f in facets]
    for b in range(B):
        nb = n if lengths is None else min(max(int(lengths[b]), 1), n)
        st = (states if states.ndim == 1 else states[b])[:nb]
        ft = foot[b, :nb]
        ref = None if foot_ref is None else \
            (np.asarray(foot_ref, np.float64) if np.ndim(foot_ref) == 2
             else np.asarray(foot_ref[b], np.float64))[:nb]
        j = np.maximum(np.arange(nb) - 1, 0)
        fs = ft[j]                                                        # the supporting foot
        # landing[k]: a landing at step k; side[i]: parity of the landings at steps < j_i
        landing = np.zeros(nb, bool)
        landing[:nb - 1] = (st[:-1] == 2) & (st[1:] != 2)
        before = np.concatenate([[0], np.cumsum(landing)[:-1]])           # landings at steps < k
        side = before[j] % 2
        flagged = False
        for a in range(2):
            s = hist[b, :nb, a, :]
            bad = ~(np.isfinite(s).all(axis=1) & np.isfinite(ft[:, a]))
            if ref is not None:
                bad |= ~np.isfinite(ref[:, a])
            if bad.any():
                flagged = True
                out[b, a:14:2] = np.nan
                out[b, a] = np.inf
                out[b, 2 + a] = float(np.argmax(bad))
                continue
            c, cd, cdd = s[:, 0], s[:, 1], s[:, 2]
            z = c - hg * cdd
            lo, hi = fs[:, a] - half[a], fs[:, a] + half[a]
            if a == 1:
                other = np.where(side == 1, fs[:, 1] + 2.0 * foot_spread,
                                 fs[:, 1] - 2.0 * foot_spread)
                stand = st == 0
                lo = np.where(stand, np.minimum(fs[:, 1], other) - half[1], lo)
                hi = np.where(stand, np.maximum(fs[:, 1], other) + half[1], hi)
            v = np.maximum(np.maximum(z - hi, lo - z), 0.0)
            v[0] = 0.0                                                    # sample 0 has no box
            vmax = v.max()
            dcm = (c + cd * root) - fs[:, a]
            out[b, a] = vmax
            out[b, 2 + a] = float(np.argmax(v)) if vmax > 0 else -1.0
            out[b, 4 + a] = float(np.count_nonzero(v > count_tol))
            out[b, 6 + a] = np.abs(c - fs[:, a]).max()
            out[b, 8 + a] = np.abs(dcm).max()
            out[b, 10 + a] = dcm[-1]
            out[b, 12 + a] = 0.0 if ref is None else np.abs(ft[:, a] - ref[:, a]).max()
        slack = np.inf
        for k in np.nonzero(landing)[0]:
            f = fac[int(before[k] % 2)]
            d = ft[k + 1] - ft[k]
            if len(f):
                slack = min(slack, float((f[:, 2] - (f[:, 0] * d[0] + f[:, 1] * d[1])).min()))
        out[b, 14] = np.nan if flagged else slack
        out[b, 15] = float(np.count_nonzero(landing))
    return out


def herdt_params_facets(params):
    """The (left, right) facet arrays [F, 3] of a controllers.herdt.HerdtParams, as
    herdt_walk_metrics_reference takes them."""
    return tuple(np.array([[params.facets[sd][f][c] for c in range(3)]
                           for f in range(params.nfacets[sd])], np.float64).reshape(-1, 3)
                 for sd in range(2))


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


AXES = {"x": 1, "y": 2, "xy": 3}  # include/zmpc.h ZMPC_PUSH_AXIS_X | ZMPC_PUSH_AXIS_Y


def check_profile(duration, profile):
    """The (duration, profile) pair of a shaped push as (D, w): D >= 1 an int, w None (all ones)
    or a finite float64 [D] array.  Raises ValueError otherwise."""
    if isinstance(duration, bool) or not isinstance(duration, (int, np.integer)) or duration < 1:
        raise ValueError(f"duration must be an integer >= 1 (samples), got {duration!r}")
    if profile is None:
        return int(duration), None
    w = np.asarray(profile, np.float64)
    if w.ndim != 1 or w.shape[0] != duration:
        raise ValueError(f"profile must hold duration = {duration} weights, got shape "
                         f"{tuple(w.shape)}")
    if not np.isfinite(w).all():
        raise ValueError("profile must be finite")
    return int(duration), w


def shaped_response(r, duration, profile=None):
    """Response by delay of a push that lasts `duration` samples with force profile F·w_j during
    history steps s + j → R [n], R_d = Σ_{j=0}^{min(D−1, d)} w_j·r_{d−j}, summed in ascending j.

    r [n] is the one-sample response (push_response, or the device's table); profile None: all
    ones, and the product is skipped, so duration 1 returns r bit for bit.  Weights at j >= n are
    never read.  R_0 = R_1 = 0 as r_0 = r_1 = 0."""
    D, w = check_profile(duration, profile)
    r = np.asarray(r, np.float64)
    n = r.shape[0]
    R = np.zeros(n)
    for j in range(min(D, n)):
        R[j:] += r[:n - j] if w is None else w[j] * r[:n - j]
    return R


def _axis_columns(up, dn, R, nb, force, limit, gap=None):
    """force[s, 0:2], limit[s, 0:2] (and gap[s, 0:2], the relative distance of the runner-up
    candidate) of one axis of one walk from its margins up, dn [nb] and the response R."""
    aR = np.abs(R)
    for st in range(nb - 2):
        rd, ad = R[1:nb - st], aR[1:nb - st]                             # delays of i = st+1 …
        pos, neg = rd > 0, rd < 0
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            cu, cd = up[st + 1:nb] / ad, dn[st + 1:nb] / ad               # (masked where r = 0)
        for k, (a, c) in enumerate(((cu, cd), (cd, cu))):                 # +: up limits r > 0
            f = np.where(pos, a, np.where(neg, c, np.inf))
            j = int(np.argmin(f))                                        # the first minimum
            if f[j] < np.inf:
                force[st, k] = f[j]
                limit[st, k] = st + 1 + j
                if gap is not None:
                    two = np.partition(f, 1)[:2] if len(f) > 1 else f
                    if len(two) < 2 or two[1] == np.inf:
                        gap[st, k] = np.inf
                    elif two[0] == 0:
                        gap[st, k] = np.inf if two[1] > 0 else 0.0
                    else:
                        gap[st, k] = (two[1] - two[0]) / two[0]


def push_map_shaped_reference(hist, zmax, zmin, r, hg, lengths=None, max_violation=0.0,
                              push_steps=None, duration=1, profile=None, axes="y",
                              return_gap=False):
    """The statement of include/zmpc.h zmpc_push_map_shaped in NumPy, with division: the checker
    of the kernels, never a fallback → (force, limit).

    Arguments as push_map_reference; r [n] is the one-sample response, shaped here by
    shaped_response(r, duration, profile) (hand in an already shaped table with duration = 1).
    axes "x", "y" or "xy": the columns are (+x, −x), (+y, −y) or (+x, −x, +y, −y), C of them;
    force float64 and limit int32 are [B, n, C], or [B, C] with push_steps.  return_gap: also the
    relative gap between each finite entry's minimum and its runner-up candidate (inf where one
    sample alone constrains the push, NaN elsewhere), shaped as force: an index comparison is
    fair where it exceeds the rounding of the candidates."""
    if axes not in AXES:
        raise ValueError(f"axes must be 'x', 'y' or 'xy', got {axes!r}")
    hist = np.asarray(hist, np.float64)
    zmax = np.asarray(zmax, np.float64)
    zmin = np.asarray(zmin, np.float64)
    B, n = hist.shape[:2]
    R = shaped_response(np.asarray(r, np.float64)[:n], duration, profile)
    t = float(max_violation)
    cols = [a for a in (0, 1) if AXES[axes] >> a & 1]
    C = 2 * len(cols)
    force = np.full((B, n, C), np.inf)
    limit = np.full((B, n, C), -1, np.int32)
    gap = np.full((B, n, C), np.nan) if return_gap else None
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
        for c, a in enumerate(cols):
            up = (hi[:, a] - z[:, a]) + t
            dn = (z[:, a] - lo[:, a]) + t
            _axis_columns(up, dn, R, nb, force[b, :, 2 * c:2 * c + 2],
                          limit[b, :, 2 * c:2 * c + 2],
                          None if gap is None else gap[b, :, 2 * c:2 * c + 2])
    if push_steps is not None:
        f1 = np.full((B, C), np.inf)
        l1 = np.full((B, C), -1, np.int32)
        g1 = np.full((B, C), np.nan)
        for b in range(B):
            nb = n if lengths is None else min(max(int(lengths[b]), 1), n)
            st = int(push_steps[b])
            if 0 <= st < nb - 2:
                f1[b], l1[b] = force[b, st], limit[b, st]
                if gap is not None:
                    g1[b] = gap[b, st]
            elif np.isnan(force[b, 0, 0]):
                f1[b] = np.nan
        force, limit, gap = f1, l1, (g1 if return_gap else None)
    return (force, limit, gap) if return_gap else (force, limit)


def planar_push(force, limit, direction):
    """Critical magnitude of a push along a planar direction from the four columns of an "xy"
    map → (magnitude, limiting sample).  force, limit [..., 4] (+x, −x, +y, −y), tensors or
    arrays; direction [..., 2] unit vectors (dx, dy), a NumPy array that broadcasts against the
    leading dimensions.  The axes decouple, so the push F·(dx, dy) survives while F·|dx| <=
    F_x(sign dx) and F·|dy| <= F_y(sign dy): the magnitude is min(F_x/|dx|, F_y/|dy|), an
    exactly-zero component gives no limit from its axis, NaN stays NaN."""
    d = np.asarray(direction, np.float64)
    cx = (d[..., 0] < 0).astype(np.int64)
    cy = 2 + (d[..., 1] < 0)
    ax, ay = np.abs(d[..., 0]), np.abs(d[..., 1])
    if hasattr(force, "detach"):  # torch
        import torch
        dev = force.device
        ax, ay = (torch.as_tensor(a, dtype=force.dtype, device=dev) for a in (ax, ay))
        shape = torch.broadcast_shapes(force.shape[:-1], ax.shape)
        cx, cy = (torch.as_tensor(np.asarray(c), device=dev).expand(shape).unsqueeze(-1)
                  for c in (cx, cy))
        fe, le = force.expand(*shape, 4), limit.expand(*shape, 4)
        fx, fy = fe.gather(-1, cx).squeeze(-1), fe.gather(-1, cy).squeeze(-1)
        lx, ly = le.gather(-1, cx).squeeze(-1), le.gather(-1, cy).squeeze(-1)
        inf = torch.full_like(fx, float("inf"))
        mx = torch.where(ax > 0, fx / ax, inf)
        my = torch.where(ay > 0, fy / ay, inf)
        return torch.minimum(mx, my), torch.where(mx <= my, lx, ly)
    shape = np.broadcast_shapes(force.shape[:-1], ax.shape)
    cx, cy = (np.broadcast_to(c, shape)[..., None] for c in (cx, cy))
    fe, le = np.broadcast_to(force, shape + (4,)), np.broadcast_to(limit, shape + (4,))
    fx, fy = (np.take_along_axis(fe, c, -1)[..., 0] for c in (cx, cy))
    lx, ly = (np.take_along_axis(le, c, -1)[..., 0] for c in (cx, cy))
    with np.errstate(divide="ignore", invalid="ignore"):
        mx = np.where(ax > 0, fx / ax, np.inf)
        my = np.where(ay > 0, fy / ay, np.inf)
    return np.minimum(mx, my), np.where(mx <= my, lx, ly)


def unit_directions(directions):
    """[K, 2] (or [..., 2]) finite non-zero planar vectors, normalised → float64 array."""
    d = np.asarray(directions, np.float64)
    if d.ndim < 1 or d.shape[-1] != 2 or not np.isfinite(d).all():
        raise ValueError(f"directions must be finite [..., 2] vectors, got shape {tuple(d.shape)}")
    norm = np.hypot(d[..., 0], d[..., 1])
    if (norm == 0).any():
        raise ValueError("a direction must not be the zero vector")
    return d / norm[..., None]


class Push:
    """A shove for a rollout (include/zmpc.h zmpc_push, "The push, stated once"): `force` newtons
    along `direction`, from history step `step` on, for `duration` samples with force
    F·profile[j] in its j-th sample.

    force      scalar or [B], in newtons
    direction  a sign (scalar): ±F on the y axis, as the reference pushes
               (zmp_controller.py:105-106); or a planar vector (dx, dy), or [B, 2] of them,
               normalised by unit_directions.  A component that is exactly zero in every
               direction leaves its axis out: (0, −1) is a y push, (1, 0) an x push
    step       an int, or [B] start steps (a step outside [0, n − 1): no push for that walk)
    duration   D >= 1, in samples;  profile  None (constant) or D finite weights (check_profile)

    +F on an axis lowers that axis' velocity.  ``axes`` is "x", "y" or "xy";
    ``amplitudes(dt, m, B)`` the [B, C] velocity steps dt·F·dir/m the kernels take."""

    __slots__ = ("force", "direction", "step", "duration", "profile", "axes")

    def __init__(self, force, direction, step, duration=1, profile=None):
        F = np.asarray(force, np.float64)
        if F.ndim > 1 or not np.isfinite(F).all():
            raise ValueError(f"force must be a finite scalar or [B], got shape {tuple(F.shape)}")
        d = np.asarray(direction, np.float64)
        if d.ndim == 0:
            if not np.isfinite(d) or d == 0:
                raise ValueError("a sign direction must be finite and non-zero")
            unit, axes = np.array([[0.0, float(np.sign(d))]]), "y"
        else:
            unit = unit_directions(d)
            if unit.ndim > 2:
                raise ValueError(f"direction must be a sign, (dx, dy) or [B, 2], got shape "
                                 f"{tuple(d.shape)}")
            unit = unit.reshape(-1, 2)
            axes = "y" if (unit[:, 0] == 0).all() else "x" if (unit[:, 1] == 0).all() else "xy"
        st = np.asarray(step)
        if st.ndim > 1 or st.dtype.kind not in "iu":
            raise ValueError("step must be an integer or a [B] integer array")
        self.duration, self.profile = check_profile(duration, profile)
        self.force, self.direction, self.axes = F, unit, axes
        self.step = int(st) if st.ndim == 0 else st.astype(np.int64)

    def __repr__(self):
        return (f"Push(axes={self.axes!r}, step={self.step!r}, duration={self.duration}"
                f"{'' if self.profile is None else ', shaped'})")

    def batch(self):
        """The batch size the push asks for (None: it fits any)."""
        sizes = {int(a.shape[0]) for a in (self.force, self.direction[:, 0],
                                          np.asarray(self.step)) if a.ndim == 1 and a.shape[0] != 1}
        if len(sizes) > 1:
            raise ValueError(f"force, direction and step disagree on the batch size: {sorted(sizes)}")
        return sizes.pop() if sizes else None

    def amplitudes(self, dt, m, B):
        """amp [B, C] = dt·F_b·dir_(b, a)/m in m/s, C columns in the order of ``axes``."""
        nb = self.batch()
        if nb is not None and nb != B:
            raise ValueError(f"the push is for {nb} walks, the batch holds {B}")
        F = np.broadcast_to(self.force.reshape(-1), (B,))
        unit = np.broadcast_to(self.direction, (B, 2))
        cols = [a for a in (0, 1) if AXES[self.axes] >> a & 1]
        return np.ascontiguousarray(dt * (F[:, None] * unit[:, cols]) / m)

    def velocity_steps(self, dt, m, B, n):
        """dvel [B, n, 2]: what the velocity of sample i + 1 is lowered by at history step i, on
        (x, y) — the statement of include/zmpc.h in NumPy, for the checkers."""
        amp = self.amplitudes(dt, m, B)
        cols = [a for a in (0, 1) if AXES[self.axes] >> a & 1]
        steps = np.broadcast_to(np.asarray(self.step, np.int64).reshape(-1), (B,))
        dvel = np.zeros((B, n, 2))
        for b in range(B):
            s = int(steps[b])
            if not 0 <= s < n - 1:
                continue
            for j in range(self.duration):
                if s + j >= n - 1:
                    break
                for c, a in enumerate(cols):
                    dvel[b, s + j, a] = amp[b, c] if self.profile is None \
                        else amp[b, c] * self.profile[j]
        return dvel


class PushTrace:
    """A disturbance trace per walk for a rollout (include/zmpc.h zmpc_trace, "The trace, stated
    once"): walk b takes force[b, j] newtons during history step step_b + j, so two walks can be
    shoved for different lengths, with different shapes, more than once, or with noise of their own.

    force  [B, L, 2] newtons on (x, y), or [B, L]: the y axis, the reference's convention
           (zmp_controller.py:105-106).  NumPy, or a float64 tensor on the plan's device.  A
           column that is exactly zero everywhere leaves its axis out, as Push does
    step   an int, or [B] start steps (a step outside [0, n − 1): no disturbance for that walk)

    +F on an axis lowers that axis' velocity.  ``axes`` is "x", "y" or "xy", ``length`` is L.
    ``from_velocity_steps`` takes the velocity steps dv = dt·F/m themselves; a device tensor is
    then used as it is, without a copy.  ``scaled(k)`` is the trace with every entry times k."""

    __slots__ = ("values", "unit", "step", "axes", "length")

    def __init__(self, force, step=0):
        v = _trace_values(force, "force")
        if v.ndim == 2:
            axes = "y"
            v = v.reshape(v.shape[0], v.shape[1], 1)
        elif v.ndim == 3 and v.shape[2] == 2:
            zero = [bool((v[:, :, a] == 0).all()) for a in (0, 1)]
            if zero[0]:
                axes, v = "y", v[:, :, 1:2]  # (an all-zero trace is a y trace of zeros)
            elif zero[1]:
                axes, v = "x", v[:, :, 0:1]
            else:
                axes = "xy"
        else:
            raise ValueError(f"force must be [B, L, 2] or [B, L], got shape {tuple(v.shape)}")
        self._set(v, "N", step, axes)

    @classmethod
    def from_velocity_steps(cls, dv, step=0, axes="xy"):
        """The trace of the velocity steps dv [B, L, C] in m/s (C the columns of `axes`; [B, L]
        with one axis), what the kernels read: dv[b, j, c] lowers the velocity of sample
        step_b + j + 1."""
        if axes not in AXES:
            raise ValueError(f"axes must be 'x', 'y' or 'xy', got {axes!r}")
        v = _trace_values(dv, "dv")
        C = 2 if axes == "xy" else 1
        if v.ndim == 2 and C == 1:
            v = v.reshape(v.shape[0], v.shape[1], 1)
        if v.ndim != 3 or v.shape[2] != C:
            raise ValueError(f"dv must be [B, L, {C}] for axes {axes!r}"
                             f"{' or [B, L]' if C == 1 else ''}, got shape {tuple(v.shape)}")
        self = cls.__new__(cls)
        self._set(v, "m/s", step, axes)
        return self

    def _set(self, v, unit, step, axes):
        if v.shape[0] < 1 or v.shape[1] < 1:
            raise ValueError(f"a trace needs B >= 1 walks and L >= 1 samples, got shape "
                             f"{tuple(v.shape)}")
        st = np.asarray(step)
        if st.ndim > 1 or st.dtype.kind not in "iu":
            raise ValueError("step must be an integer or a [B] integer array")
        if st.ndim == 1 and st.shape[0] not in (1, v.shape[0]):
            raise ValueError(f"step is for {st.shape[0]} walks, the trace holds {v.shape[0]}")
        self.values, self.unit, self.axes, self.length = v, unit, axes, int(v.shape[1])
        self.step = int(st) if st.ndim == 0 else st.astype(np.int64)

    def __repr__(self):
        return (f"PushTrace(axes={self.axes!r}, walks={self.batch()}, length={self.length}, "
                f"step={self.step!r})")

    def batch(self):
        """The batch size the trace asks for: its B rows."""
        return int(self.values.shape[0])

    def scaled(self, k):
        """The same trace with every entry times k (a new array; self is unchanged)."""
        t = PushTrace.__new__(PushTrace)
        t._set(self.values * float(k), self.unit, self.step, self.axes)
        return t

    def dv(self, dt, m, B):
        """dv [B, L, C] = dt·F/m in m/s, C columns in the order of ``axes``: a NumPy array, or
        the device tensor itself when the trace holds velocity steps on the device."""
        if self.batch() != B:
            raise ValueError(f"the trace is for {self.batch()} walks, the batch holds {B}")
        if self.unit == "m/s":
            return self.values
        return dt * self.values / m

    def velocity_steps(self, dt, m, B, n):
        """dvel [B, n, 2]: what the velocity of sample i + 1 is lowered by at history step i, on
        (x, y) — the statement of include/zmpc.h in NumPy, for the checkers."""
        dv = self.dv(dt, m, B)
        if not isinstance(dv, np.ndarray):
            dv = dv.detach().cpu().numpy()
        cols = [a for a in (0, 1) if AXES[self.axes] >> a & 1]
        steps = np.broadcast_to(np.asarray(self.step, np.int64).reshape(-1), (B,))
        dvel = np.zeros((B, n, 2))
        for b in range(B):
            s = int(steps[b])
            if not 0 <= s < n - 1:
                continue
            k = min(self.length, n - 1 - s)
            for c, a in enumerate(cols):
                dvel[b, s:s + k, a] = dv[b, :k, c]
        return dvel


def _trace_values(a, name):
    """A trace's entries: a float64 device tensor as it is, anything else as a float64 array."""
    if hasattr(a, "data_ptr"):  # a torch tensor; analysis itself does not need torch
        if str(a.dtype) != "torch.float64":
            raise ValueError(f"a {name} tensor must be float64, got {a.dtype}")
        return a
    return np.asarray(a, np.float64)


class PushMap:
    """The push-robustness map of a batch of walks: ``force`` [B, n, C] (N, at history step s) and
    ``limit`` [B, n, C] (int32, the sample that leaves its box first, −1 where no sample does or
    the walk fails unpushed), tensors or arrays; views, no copies.  ``axes`` names the columns:
    "y" (the default) [..., 0] a +y push and [..., 1] a −y push, "x" the same on the x axis, "xy"
    (+x, −x, +y, −y).  ``response`` [n] is the ZMP response by delay when it was asked for."""

    __slots__ = ("force", "limit", "response", "axes")

    def __init__(self, force, limit, response=None, axes="y"):
        if axes not in AXES:
            raise ValueError(f"axes must be 'x', 'y' or 'xy', got {axes!r}")
        C = 4 if axes == "xy" else 2
        if force.ndim != 3 or force.shape[2] != C or tuple(limit.shape) != tuple(force.shape):
            raise ValueError(f"force and limit must both be [B, n, {C}], got {tuple(force.shape)} "
                             f"and {tuple(limit.shape)}")
        self.force, self.limit, self.response, self.axes = force, limit, response, axes

    def __len__(self):
        return int(self.force.shape[0])

    def __repr__(self):
        tail = "" if self.axes == "y" else f", axes={self.axes!r}"
        return f"PushMap(B={len(self)}, n={int(self.force.shape[1])}{tail})"

    def weakest_push(self):
        """Per walk the smallest critical push of any column and where it acts → (force [B],
        step [B], axis [B]: 0 x or 1 y, sign [B]: +1 or −1).  A walk that fails unpushed gives
        NaN, and one that no push topples +inf, both with step −1, axis −1 and sign 0."""
        f = self.force
        C = int(f.shape[2])
        first = 1 if self.axes == "y" else 0  # the axis of columns 0 and 1
        flat = f.reshape(f.shape[0], -1)
        if hasattr(flat, "detach"):  # torch
            import torch
            nan = torch.isnan(flat)
            filled = torch.where(nan, torch.full_like(flat, float("inf")), flat)
            val, idx = filled.min(dim=1)
            val = torch.where(nan.any(dim=1), torch.full_like(val, float("nan")), val)
            none = ~torch.isfinite(val)
            where, full = torch.where, torch.full_like
            return (val, where(none, full(idx, -1), idx // C),
                    where(none, full(idx, -1), first + (idx % C) // 2),
                    where(none, full(idx, 0), 1 - 2 * (idx % 2)))
        nan = np.isnan(flat)
        filled = np.where(nan, np.inf, flat)
        idx = filled.argmin(axis=1)
        val = np.where(nan.any(axis=1), np.nan, filled[np.arange(flat.shape[0]), idx])
        none = ~np.isfinite(val)
        return (val, np.where(none, -1, idx // C), np.where(none, -1, first + (idx % C) // 2),
                np.where(none, 0, 1 - 2 * (idx % 2)))

    def rose(self, directions):
        """Critical push magnitude along planar directions → (magnitude [B, n, K], limiting
        sample [B, n, K]); directions [K, 2] vectors (dx, dy), normalised here.  Needs an "xy"
        map; see planar_push."""
        if self.axes != "xy":
            raise ValueError(f"rose needs an 'xy' map, this one has axes = {self.axes!r}")
        d = unit_directions(directions)
        if d.ndim != 2:
            raise ValueError(f"directions must be [K, 2], got shape {tuple(d.shape)}")
        f, l = self.force, self.limit
        return planar_push(f[:, :, None, :], l[:, :, None, :], d)

    def weakest(self):
        """Per walk the smallest critical push and where it acts → (force [B], step [B],
        direction [B]: +1 or −1).  A walk that fails unpushed gives NaN, and one that no push
        topples +inf, both with step −1 and direction 0.  y-axis maps only (weakest_push takes
        every map)."""
        if self.axes != "y":
            raise ValueError("weakest() reads a y-axis map; use weakest_push() for maps with an "
                             "x axis")
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


def trace_margin_reference(hist, zmax, zmin, dv, steps, Abar, hg, draws=1, axes="xy", lengths=None,
                           max_violation=0.0):
    """The statement of include/zmpc.h zmpc_trace_margin in NumPy, with division: the checker of
    the kernel, never a fallback → (scale [B, K, 2] float64, limit [B, K, 2] int32).

    hist [B, n, 2, 3] unpushed; zmax, zmin [B, n, 2] or a shared [n, 2]; dv [B·K, L, C] velocity
    steps in m/s, C the columns of `axes`; steps an int or [B·K] start steps; Abar [3, 3] the closed
    loop A − B·kxᵀ; hg = h/g; lengths [B] live samples or None.  Row b·K + k is draw k of walk b."""
    hist = np.asarray(hist, np.float64)
    zmax, zmin = np.asarray(zmax, np.float64), np.asarray(zmin, np.float64)
    dv = np.asarray(dv, np.float64)
    dv = dv.reshape(dv.shape[0], dv.shape[1], -1)
    Abar = np.asarray(Abar, np.float64).reshape(3, 3)
    B, n = hist.shape[:2]
    K, t = int(draws), float(max_violation)
    cols = [a for a in (0, 1) if AXES[axes] >> a & 1]
    if dv.shape[0] != B * K or dv.shape[2] != len(cols):
        raise ValueError(f"dv must be [B·K, L, {len(cols)}] = [{B * K}, L, {len(cols)}], got "
                         f"{dv.shape}")
    steps = np.broadcast_to(np.asarray(steps, np.int64).reshape(-1), (B * K,))
    scale = np.full((B, K, 2), np.inf)
    limit = np.full((B, K, 2), -1, np.int32)
    for b in range(B):
        nb = n if lengths is None else min(max(int(lengths[b]), 1), n)
        hi = (zmax if zmax.ndim == 2 else zmax[b])[:nb]
        lo = (zmin if zmin.ndim == 2 else zmin[b])[:nb]
        st = hist[b, :nb]
        z = st[:, :, 0] - hg * st[:, :, 2]                               # [nb, 2]
        v = np.fmax(np.fmax(z - hi, lo - z), 0.0)
        if not np.isfinite(st).all() or (v > t).any():
            scale[b] = np.nan
            continue
        up, dn = (hi - z) + t, (z - lo) + t
        for k in range(K):
            r = b * K + k
            s = int(steps[r])
            if not 0 <= s < nb - 1:
                continue
            rho = np.zeros((nb, 2))                                      # [i, a], 0 up to s
            for c, a in enumerate(cols):
                d = np.zeros(3)
                for i in range(s, nb - 1):
                    d = Abar @ d
                    if i - s < dv.shape[1]:
                        d[1] += dv[r, i - s, c]
                    rho[i + 1, a] = -(d[0] - hg * d[2])
            pos, neg = rho > 0, rho < 0
            for col, (p, q) in enumerate(((up, dn), (dn, up))):
                f = np.full((nb, 2), np.inf)
                with np.errstate(over="ignore", invalid="ignore"):
                    f[pos] = p[pos] / rho[pos]
                    f[neg] = q[neg] / -rho[neg]
                j = int(np.argmin(f))                    # the first minimum in (i, a) order
                if f.flat[j] < np.inf:
                    scale[b, k, col] = f.flat[j]
                    limit[b, k, col] = j                 # = 2·i + a
    return scale, limit


class TraceMargin:
    """The trace margins of a batch of walks with K draws each (zmpc_trace_margin): ``scale``
    [B, K, 2] — [..., 0] the largest multiple of a draw's trace its walk survives, [..., 1] that of
    the negated trace; +inf where no sample limits it, NaN where the walk fails undisturbed — and
    ``limit`` [B, K, 2] int32, 2·sample + axis of what leaves its box first (−1: none).  Tensors or
    arrays; views, no copies."""

    __slots__ = ("scale", "limit")

    def __init__(self, scale, limit):
        if scale.ndim != 3 or scale.shape[2] != 2 or tuple(limit.shape) != tuple(scale.shape):
            raise ValueError(f"scale and limit must both be [B, K, 2], got {tuple(scale.shape)} "
                             f"and {tuple(limit.shape)}")
        self.scale, self.limit = scale, limit

    def __len__(self):
        return int(self.scale.shape[0])

    def __repr__(self):
        return f"TraceMargin(B={len(self)}, draws={int(self.scale.shape[1])})"

    @property
    def critical(self):
        """[B, K]: the largest multiple of each draw's trace its walk survives."""
        return self.scale[..., 0]

    @property
    def sample(self):
        """[B, K, 2]: the sample that leaves its box first, −1 where none does."""
        l = self.limit
        return (l >> 1) * (l >= 0) - (l < 0) * 1

    @property
    def axis(self):
        """[B, K, 2]: the axis on which it leaves (0 x, 1 y), −1 where none does."""
        l = self.limit
        return (l & 1) * (l >= 0) - (l < 0) * 1

    def survives(self, lam=1.0):
        """[B, K] bool: does the walk survive `lam` times the draw's trace?  A negative lam asks
        about |lam| times the negated trace (column 1).  NaN (a walk that fails undisturbed) is
        False."""
        lam = float(lam)
        return self.scale[..., 1 if lam < 0 else 0] >= abs(lam)

    def survival(self, lam=1.0):
        """[B]: the fraction of a walk's draws that survive (survives(lam))."""
        ok = self.survives(lam)
        if hasattr(ok, "detach"):  # torch
            return ok.to(self.scale.dtype).mean(dim=1)
        return ok.mean(axis=1)


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
