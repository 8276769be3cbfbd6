"""CPU ORACLE for the Wieber LIPM-ZMP MPC hot path — TEST INFRASTRUCTURE ONLY.

Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may
import this module, and only as the checker / the timed CPU baseline.  The product
(``model-predictive-control-for-bipedal-locomotion_amd/``) never imports it.

Restates the reference algorithm in NumPy (reference @ 2025-12-26,
``src/mpc_bipedal/controllers/zmp_controller.py``):

* ``predict_wieber_axis_ref`` / ``rollout_ref``: reference-faithful, per call the interpreted
  O(N²) ``Px``/``Pu`` build (:162-171) and ``np.linalg.inv`` (:196-198), then ``A x + B u``
  (:199); the rollout loops as :59-108 / :110-147 do (pad with the last row :81-88, kick
  at ``i == n//2`` :90,105-106).  This is the CPU baseline bench.py times (kind "port").
* ``gain_row`` / ``rollout_gain``: the same maths batched — ``u0 = k·(z_ref − Px x)`` with the
  gain row ``k = row 0 of inv(M) Puᵀ``; exact restatement, used to check the device results
  for whole batches.
* ``solve_box_qp`` / ``rollout_strict``: the strict branch (:173-195).  Its reference solver is
  cvxpy→OSQP, which is NOT installed here (third-party; cvxpy pinned only as ``>=1.2.0`` in
  requirements.txt:2, OSQP unpinned), so parity with OSQP itself is UNPINNED.  The oracle
  solves the same QP exactly — a primal active-set method on the z-space Hessian
  ``H = Q·I + R·Pu⁻ᵀPu⁻¹`` (independent of the device's dual/PDAS method on its inverse) —
  and certifies every answer with the KKT conditions (strictly convex, so the KKT point is
  the unique minimiser OSQP approximates).

Pinning: the unconstrained functions are checked against golden vectors produced by the
reference itself (``tests/golden/make_golden.py``); ``tests/test_oracle.py`` holds those checks.
"""

import numpy as np

# ----------------------------------------------------------------------------- model


def lipm(dt, h, g):
    """A, B, C of zmp_controller.py:18-20."""
    T = dt
    A = np.array([[1., T, T ** 2 / 2.], [0., 1., T], [0., 0., 1.]])
    B = np.array([T ** 3 / 6., T ** 2 / 2., T]).reshape((3, 1))
    C = np.array([1., 0., -h / g])
    return A, B, C


def prediction_matrices_loop(N, dt, h, g):
    """Px, Pu with the reference's interpreted double loop (zmp_controller.py:162-171)."""
    Px = np.zeros((N, 3))
    Pu = np.zeros((N, N))
    T = dt
    for i in range(N):
        Px[i, 0] = 1
        Px[i, 1] = T * (i + 1)
        Px[i, 2] = (T ** 2) / 2 * (i + 1) ** 2 - h / g
        for j in range(i + 1):
            Pu[i, j] = (T ** 3) / 6 * (1 + 3 * (i - j) + 3 * (i - j) ** 2) - T * h / g
    return Px, Pu


def prediction_matrices(N, dt, h, g):
    """Vectorised Px, Pu (same operations, bit-identical to the loop)."""
    T = dt
    i = np.arange(N)
    Px = np.empty((N, 3))
    Px[:, 0] = 1.0
    Px[:, 1] = T * (i + 1).astype(np.float64)
    Px[:, 2] = (T ** 2) / 2 * ((i + 1) ** 2).astype(np.float64) - h / g
    d = i[:, None] - i[None, :]
    Pu = np.where(d >= 0, (T ** 3) / 6 * (1 + 3 * d + 3 * d ** 2).astype(np.float64) - T * h / g,
                  0.0)
    return Px, Pu


# ----------------------------------------------------------------------------- reference-faithful


def predict_wieber_axis_ref(x, N, zmax, zmin, dt, h, g, Q, R):
    """zmp_controller.py:149-201 with strict=False, as written (loop build + inv)."""
    A, B, _ = lipm(dt, h, g)
    Px, Pu = prediction_matrices_loop(N, dt, h, g)
    z_ref = (zmax + zmin) / 2
    X = -np.linalg.inv(Pu.T @ Pu + R / Q * np.eye(N)) @ Pu.T @ (Px @ x - z_ref)
    return A @ x + B @ X[0:1, :]


def _extend(z, N):
    return np.vstack([z, np.tile(z[-1:, :], (N, 1))])


def rollout_ref(x_init, y_init, zmax, zmin, N, dt, h, g, Q, R, F_ext=None, m=40.0):
    """generate_com_trajectory_wieber (F_ext given) / generate_state_trajectory_wieber
    (F_ext None), per step with predict_wieber_axis_ref.  Returns (x_hist, y_hist) (n,3,1)."""
    n = len(zmin)
    zx, zn = _extend(zmax, N), _extend(zmin, N)
    xs, ys = [x_init], [y_init]
    for i in range(n - 1):
        xs.append(predict_wieber_axis_ref(xs[-1], N, zx[i + 1:i + 1 + N, 0:1],
                                          zn[i + 1:i + 1 + N, 0:1], dt, h, g, Q, R))
        ys.append(predict_wieber_axis_ref(ys[-1], N, zx[i + 1:i + 1 + N, 1:2],
                                          zn[i + 1:i + 1 + N, 1:2], dt, h, g, Q, R))
        if F_ext is not None and i == n // 2:
            ys[-1] = ys[-1] - np.array([[0., dt * F_ext / m, 0.]]).T
    return np.array(xs), np.array(ys)


# ----------------------------------------------------------------------------- gain form (batched)


def gain_row(N, dt, h, g, Q, R):
    """k = row 0 of inv(PuᵀPu + R/Q I) Puᵀ  and  kx = k·Px."""
    Px, Pu = prediction_matrices(N, dt, h, g)
    M = Pu.T @ Pu + R / Q * np.eye(N)
    y = np.linalg.solve(M, np.eye(N)[:, 0])
    k = Pu @ y
    return k, k @ Px


def rollout_gain(zmax, zmin, x0, N, dt, h, g, Q, R, kick=None, kick_step=-1, gain=None):
    """Batched unconstrained rollout.  zmax/zmin [B,n,2], x0 [B,2,3], kick [B] (or None),
    kick_step an int or a [B] array of per-walk steps; gain: (k, kx) to roll out with instead of
    gain_row's (a gain row known to higher precision).  Returns hist [B,n,2,3]."""
    zmax = np.asarray(zmax, np.float64)
    zmin = np.asarray(zmin, np.float64)
    Bn, n = zmax.shape[0], zmax.shape[1]
    A, Bv, _ = lipm(dt, h, g)
    k, kx = gain_row(N, dt, h, g, Q, R) if gain is None else gain
    zr = (zmax + zmin) / 2
    zr = np.concatenate([zr, np.repeat(zr[:, -1:, :], N, axis=1)], axis=1)   # [B, n+N, 2]
    # f_i = Σ_j k_j z_ref[i+1+j]  for all steps at once
    win = np.lib.stride_tricks.sliding_window_view(zr[:, 1:, :], N, axis=1)  # [B, n, 2, N]
    f = win[:, : n - 1] @ k                                                  # [B, n-1, 2]
    hist = np.empty((Bn, n, 2, 3))
    x = np.asarray(x0, np.float64).copy()
    hist[:, 0] = x
    kk = np.zeros(Bn) if kick is None else np.asarray(kick, np.float64)
    for i in range(n - 1):
        u = f[:, i, :] - x @ kx                                              # [B, 2]
        x = x @ A.T + u[..., None] * Bv[:, 0]
        if np.ndim(kick_step) == 0:
            if i == kick_step:
                x[:, 1, 1] -= kk
        else:
            hit = np.asarray(kick_step) == i
            x[hit, 1, 1] -= kk[hit]
        hist[:, i + 1] = x
    return hist


# ----------------------------------------------------------------------------- strict (exact box-QP)


def strict_matrices(N, dt, h, g, Q, R):
    """z-space Hessian H = Q I + R Pu⁻ᵀ Pu⁻¹ (built from Pu⁻¹ directly) and Px, p0."""
    Px, Pu = prediction_matrices(N, dt, h, g)
    V = np.linalg.solve(Pu, np.eye(N))
    H = Q * np.eye(N) + R * V.T @ V
    return H, V, Px, Pu


def kkt_check(H, q, z, lo, hi, scale=1.0):
    """KKT residuals of min ½zᵀHz + qᵀz, lo ≤ z ≤ hi.  Returns dict of maxima.

    A slot with hi − lo ≤ 0 is an equality: its multiplier is free in sign, so it enters
    `primal` only — neither dual term, nor `stationarity`."""
    gr = H @ z + q
    eq = hi - lo <= 0
    at_hi = (z >= hi - 1e-12) & ~eq
    at_lo = (z <= lo + 1e-12) & ~eq
    free = ~(at_hi | at_lo | eq)
    return dict(
        primal=max(0.0, float(np.max(z - hi)), float(np.max(lo - z))),
        stationarity=float(np.max(np.abs(gr[free]))) / scale if free.any() else 0.0,
        dual_hi=float(np.max(gr[at_hi])) / scale if at_hi.any() else 0.0,   # must be <= 0
        dual_lo=float(-np.min(gr[at_lo])) / scale if at_lo.any() else 0.0,  # must be <= 0
    )


def solve_box_qp(H, q, lo, hi, W0=None, maxit=1000):
    """Exact primal active-set solve of min ½zᵀHz + qᵀz s.t. lo ≤ z ≤ hi (H SPD).

    W0: optional warm-start working set (int8 array: 0 free, 1 at hi, 2 at lo).  Slots with
    hi − lo ≤ 0 are equalities: in the working set from the start and never dropped.
    Returns (z, working set).
    """
    n = len(q)
    Wset = np.zeros(n, np.int8) if W0 is None else np.asarray(W0, np.int8).copy()
    # a slot of zero width is an equality: always in the working set, never dropped (its
    # multiplier may take either sign)
    eq = hi - lo <= 0
    Wset[eq & (Wset == 0)] = 1
    # feasible start consistent with the working set: EQP for W0, then clip (clipped slots
    # join the working set)
    F = Wset == 0
    z = np.where(Wset == 1, hi, lo).astype(np.float64)
    if F.any():
        z[F] = np.linalg.solve(H[np.ix_(F, F)], -q[F] - H[np.ix_(F, ~F)] @ z[~F])
    up, dn = F & (z > hi), F & (z < lo)
    Wset[up], Wset[dn] = 1, 2
    z = np.clip(z, lo, hi)
    for _ in range(maxit):
        F = Wset == 0
        zf = z.copy()
        zf[Wset == 1] = hi[Wset == 1]
        zf[Wset == 2] = lo[Wset == 2]
        if F.any():
            rhs = -q[F] - H[np.ix_(F, ~F)] @ zf[~F]
            zf[F] = np.linalg.solve(H[np.ix_(F, F)], rhs)
        # ratio test towards zf
        d = zf - z
        alpha = 1.0
        block = -1
        for j in np.where(F)[0]:
            if d[j] > 0 and z[j] + d[j] > hi[j]:
                a = (hi[j] - z[j]) / d[j]
                if a < alpha:
                    alpha, block = a, j
            elif d[j] < 0 and z[j] + d[j] < lo[j]:
                a = (lo[j] - z[j]) / d[j]
                if a < alpha:
                    alpha, block = a, j
        if block >= 0:
            z = z + alpha * d
            Wset[block] = 1 if d[block] > 0 else 2
            z[block] = hi[block] if d[block] > 0 else lo[block]
            continue
        z = zf
        gr = H @ z + q
        # optimal if gr <= 0 at hi-active and gr >= 0 at lo-active
        viol = np.where(Wset == 1, gr, np.where(Wset == 2, -gr, 0.0))
        viol[eq] = 0.0
        j = int(np.argmax(viol))
        if viol[j] <= 1e-15 * max(1.0, float(np.abs(gr).max())):
            return z, Wset
        Wset[j] = 0
    raise RuntimeError("box-QP active set did not terminate")


def strict_u0(x, zmax_w, zmin_w, H, Px, p0, Q, W0=None):
    """One strict solve (zmp_controller.py:173-195).  x (3,), windows (N,) → (u0, W, z)."""
    c = Px @ x
    z_ref = (zmax_w + zmin_w) / 2
    # objective in z: ½Q‖z − z_ref‖² + ½R‖V(z − c)‖² = ½ zᵀHz + qᵀz + const,
    # q = −Q z_ref − (H − Q I) c
    q = -Q * z_ref - (H @ c - Q * c)
    z, W = solve_box_qp(H, q, zmin_w, zmax_w, W0)
    return (z[0] - c[0]) / p0, W, z, q


def rollout_strict(x_init, y_init, zmax, zmin, N, dt, h, g, Q, R, kick=0.0, kick_step=-1,
                   return_kkt=False):
    """Strict rollout of one walk: zmax/zmin [n,2], x_init/y_init (3,).  hist [n,2,3]."""
    n = len(zmax)
    A, Bv, _ = lipm(dt, h, g)
    H, V, Px, Pu = strict_matrices(N, dt, h, g, Q, R)
    p0 = Pu[0, 0]
    zx, zn = _extend(np.asarray(zmax), N), _extend(np.asarray(zmin), N)
    hist = np.empty((n, 2, 3))
    st = [np.asarray(x_init, np.float64).reshape(3).copy(),
          np.asarray(y_init, np.float64).reshape(3).copy()]
    hist[0, 0], hist[0, 1] = st
    Ws = [None, None]
    worst = dict(primal=0.0, stationarity=0.0, dual_hi=0.0, dual_lo=0.0)
    for i in range(n - 1):
        for a in range(2):
            hi = zx[i + 1:i + 1 + N, a]
            lo = zn[i + 1:i + 1 + N, a]
            W0 = None if Ws[a] is None else np.concatenate([Ws[a][1:], Ws[a][-1:]])
            u0, W, z, q = strict_u0(st[a], hi, lo, H, Px, p0, Q, W0)
            Ws[a] = W
            if return_kkt:
                r = kkt_check(H, q, z, lo, hi, scale=max(1.0, float(np.abs(q).max())))
                for key in worst:
                    worst[key] = max(worst[key], r[key])
            st[a] = A @ st[a] + Bv[:, 0] * u0
        if i == kick_step:
            st[1] = st[1] - np.array([0.0, kick, 0.0])
        hist[i + 1, 0], hist[i + 1, 1] = st
    return (hist, worst) if return_kkt else hist


def strict_step_batch(x, zmax_w, zmin_w, N, dt, h, g, Q, R):
    """Cold-start strict predict_wieber_axis for a batch: x [B,3], windows [B,N] → [B,3]."""
    A, Bv, _ = lipm(dt, h, g)
    H, V, Px, Pu = strict_matrices(N, dt, h, g, Q, R)
    out = np.empty((len(x), 3))
    for b in range(len(x)):
        u0, _, _, _ = strict_u0(np.asarray(x[b]), np.asarray(zmax_w[b]), np.asarray(zmin_w[b]),
                                H, Px, Pu[0, 0], Q)
        out[b] = A @ x[b] + Bv[:, 0] * u0
    return out
