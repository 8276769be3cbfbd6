"""Zero Moment Point (ZMP) controller using Model Predictive Control — HIP device path.

Drop-in for the reference ``ZMPController`` (``src/mpc_bipedal/controllers/zmp_controller.py``):
same constructor, same attributes (``config``, ``A``, ``B``, ``C``, ``external_force``), same
method names, argument meanings, shapes, return values and errors for the Wieber path.  Every
QP solve runs in hand-written HIP kernels (``csrc/``) reached through the C-ABI of
``include/zmpc.h``; NumPy inputs are staged to the device and results copied back, which is
the only host work.  There is no CPU solver behind this class.

The Herdt joint footstep QP (``method="herdt"``, :203-531) runs on the device as well
(``csrc/herdt.hip``); its host bookkeeping is in ``controllers/herdt.py``.

Additions (not in the reference): ``generate_com_trajectory_batch`` /
``generate_state_trajectory_batch`` / ``generate_com_trajectory_herdt_batch`` for many walks or
disturbance scenarios at once, taking and returning torch device tensors; ``walk_metrics`` (did
the ZMP stay inside the support box, per walk, reduced on the device), ``critical_force``
(the largest push each scenario survives, by bisection over batched rollouts), and for the
unconstrained controller ``push_map`` / ``critical_force_exact`` (that push in closed form, at
every step and in both directions, from one unpushed rollout).  The batch methods and
``critical_force`` also take a shove of any length, shape and planar direction
(``push=analysis.Push(...)``; ``duration=``, ``profile=``) on every controller, or a force trace
per walk, sample and axis (``trace=analysis.PushTrace(...)``).  For the
footstep-adapting controller the same two questions are ``herdt_walk_metrics`` (the support box
rebuilt from the feet the QP chose, and the divergent component of motion as the verdict) and
``critical_force_herdt``.
"""

import warnings
from typing import Optional, Tuple

import numpy as np
import torch

from ..analysis import (NHERDT_METRICS, NMETRICS, HerdtWalkMetrics, Push, PushMap, PushTrace,
                        TraceMargin, WalkMetrics, check_profile, planar_push, unit_directions)
from ..config import MPCConfig
from ..models.lipm_model import lipm_matrices
from ..solver import get_plan
from . import herdt

_FAILED = "QP solver did not find a solution (infeasible or other)."
_ST_MAXITER = 1  # include/zmpc.h ZMPC_ST_MAXITER
_ST_INFEASIBLE = 8  # include/zmpc.h ZMPC_ST_INFEASIBLE


def _default_force_step(n, lengths):
    """Where the push lands when no force_step is given: history step n // 2, or n_b // 2 of
    each ragged walk (lengths [B] tensor), as zmp_controller.py:90."""
    return n // 2 if lengths is None else lengths // 2


def _force_step(force_step, n, lengths):
    """The force_step argument of the critical-force searches: None gives the default above, a
    scalar an int, a [B] argument stays as given."""
    if force_step is None:
        return _default_force_step(n, lengths)
    return int(force_step) if np.ndim(force_step) == 0 else force_step


def _unit_push(direction, unit, B):
    """One newton along each scenario's direction, as analysis.Push takes it: (F1 [B], d1 [B,2])
    host arrays whose amplitudes a bisection scales.  unit: planar unit vectors [1, 2] or [B, 2],
    broadcast; else direction holds a sign or [B] signs on the host, pushed along y, and a sign
    of 0 is no push, through a zero force."""
    if unit is not None:
        return np.ones(B), np.broadcast_to(unit, (B, 2))
    sign = np.sign(np.broadcast_to(np.asarray(direction, np.float64), (B,)))
    return np.abs(sign), np.stack([np.zeros(B), np.where(sign == 0, 1.0, sign)], axis=1)


def _bisect(passes, B, F_hi, iters, f64, after_unpushed=None):
    """The bracket of critical_force and critical_force_herdt: passes(F [B]) -> [B] bool runs one
    evaluation; the unpushed one comes first (after_unpushed() is called behind it), then the top
    of the bracket, then iters halvings: iters + 2 evaluations.  Returns (F_lo, F_hi), NaN in both
    where the unpushed walk fails."""
    top = torch.full((B,), float(F_hi), **f64)
    lo = torch.zeros(B, **f64)
    hi = top.clone()
    never = ~passes(lo)
    if after_unpushed is not None:
        after_unpushed()
    lo = torch.where(passes(top), top, lo)
    for _ in range(int(iters)):
        mid = 0.5 * (lo + hi)
        ok = passes(mid)
        lo, hi = torch.where(ok, mid, lo), torch.where(ok, hi, mid)
    nan = torch.full_like(lo, float("nan"))
    return torch.where(never, nan, lo), torch.where(never, nan, hi)


def _direction_size(direction, unit):
    """direction as an argument that sizes the scenario batch (_scenario's `sized`): a sign or
    [B] signs as given; planar directions (unit [K, 2], else None) count as a [K] argument when
    K > 1, one scenario each."""
    if unit is None:
        return direction
    return unit[:, 0] if unit.shape[0] > 1 else None


def _batch_size(per_walk, sized, message):
    """B of a scenario batch: the rows of the first argument of `per_walk` — (argument, its rank
    when it holds one row per walk, None: whenever given) — that is per walk, else of the first
    [B] argument of `sized` (the arguments that may be scalars or [B]), else 1.  A [B'] argument
    of `sized` with B' != B raises ValueError(message.format(B=B))."""
    named = [int(np.shape(a)[0]) for a, rank in per_walk
             if a is not None and rank in (None, np.ndim(a))]
    sizes = [int(np.shape(a)[0]) for a in sized if a is not None and np.ndim(a) == 1]
    B = (named + sizes + [1])[0]
    if any(s != B for s in sizes):
        raise ValueError(message.format(B=B))
    return B


def _one_disturbance(F_ext, push, trace, force_step=None, walk_lengths=None):
    """The batch methods take F_ext, a push or a trace, one of them; a push and a trace carry their
    own start steps, so beside force_step or walk_lengths (where the method has them) they raise
    too."""
    if push is not None and F_ext is not None:
        raise ValueError("give either F_ext or push, not both")
    if trace is not None and (push is not None or F_ext is not None):
        raise ValueError("give either trace or F_ext or push, not both")
    for what, given in (("trace", trace), ("push", push)):
        if given is not None and (force_step is not None or walk_lengths is not None):
            raise ValueError(f"a {what} carries its own start step(s): force_step and "
                             "walk_lengths belong to F_ext")


def _trace_alone(trace, force_step, direction, D, w):
    """A trace in a critical-force search stands for force_step, direction, duration and profile
    (D, w: check_profile's answer): beside any of them it raises ValueError."""
    if not isinstance(trace, PushTrace):
        raise ValueError(f"trace must be an analysis.PushTrace, got {type(trace).__name__}")
    if force_step is not None or np.ndim(direction) != 0 or direction != +1 or D != 1 \
            or w is not None:
        raise ValueError("a trace carries its own start steps, directions and shape: "
                         "force_step, direction, duration and profile belong to a push")


class ZMPController:
    """ZMP Controller using Model Predictive Control for bipedal locomotion."""

    def __init__(self, config: MPCConfig):
        # zmp_controller.py:15-21
        self.config = config
        self.A, self.B, self.C = lipm_matrices(config.dt, config.h, config.g)
        self.external_force = True

    # ------------------------------------------------------------------ plans / helpers
    def _plan(self, horizon: Optional[int] = None):
        cfg = self.config
        if horizon is not None and int(horizon) != int(cfg.horizon):
            # predict_wieber_axis takes nb_steps explicitly (zmp_controller.py:149)
            from dataclasses import replace
            cfg = replace(cfg, horizon=int(horizon), dt=cfg.dt)
        return get_plan(cfg)

    def _raise_on_status(self, status):
        if int(status.max().item() if status.numel() else 0) != 0:
            raise RuntimeError(_FAILED)

    def _herdt_status(self, status):
        """Herdt drop-ins: the reference never raises on a failed joint QP — it prints a message,
        substitutes zero jerk and the air foot's centre and continues (zmp_controller.py:796-802).
        The kernel applies that same fallback to a solve whose swing polytope is infeasible
        (ZMPC_ST_INFEASIBLE, the analogue of OSQP returning no solution); a solve that reached the
        active-set pass cap (ZMPC_ST_MAXITER) keeps its last iterate, as OSQP returns its iterate
        at its own iteration limit.  Both warn; any other flag (non-finite state, footstep
        factorisation, more footsteps than the kernel was built for) raises RuntimeError."""
        st = status.cpu().numpy() if isinstance(status, torch.Tensor) else np.asarray(status)
        soft = _ST_MAXITER | _ST_INFEASIBLE
        if st.size and np.any(st & ~soft):
            raise RuntimeError(_FAILED)
        if st.size and np.any(st & soft):
            msg = (f"Joint QP solver failed in {int(np.count_nonzero(st & soft))} walk(s) "
                   f"(pass cap, last iterate kept: {int(np.count_nonzero(st & _ST_MAXITER))}; "
                   f"infeasible swing polytope, zero jerk and the air foot's centre used: "
                   f"{int(np.count_nonzero(st & _ST_INFEASIBLE))})")
            print(msg)
            warnings.warn(msg, RuntimeWarning, stacklevel=3)

    def _kick(self) -> float:
        # zmp_controller.py:106: dt * F_ext / m, subtracted from the y velocity
        return self.config.dt * self.config.F_ext / self.config.m

    # ------------------------------------------------------------------ reference API
    def generate_com_trajectory(self, x_init: np.ndarray, y_init: np.ndarray,
                                z_max: np.ndarray = None, z_min: np.ndarray = None,
                                v_ref: np.ndarray = None, state_ref: np.ndarray = None,
                                ) -> Tuple[np.ndarray, np.ndarray]:
        """Route on ``config.method`` (zmp_controller.py:23-57)."""
        method = self.config.method.lower()
        if method == "wieber":
            if z_max is None or z_min is None:
                raise ValueError("z_max and z_min are required for wieber method")
            return self.generate_com_trajectory_wieber(x_init, y_init, z_max, z_min)
        elif method == "herdt":
            if v_ref is None or state_ref is None:
                raise ValueError("v_ref and state_ref are required for herdt method")
            return self.generate_com_trajectory_herdt(x_init, y_init, v_ref, state_ref)
        else:
            raise ValueError(f"Unknown method: {method}. Must be 'wieber' or 'herdt'")

    def generate_com_trajectory_wieber(self, x_init: np.ndarray, y_init: np.ndarray,
                                       z_max: np.ndarray, z_min: np.ndarray
                                       ) -> Tuple[np.ndarray, np.ndarray]:
        """COM trajectory (n,2) and y state history (n,3,1) (zmp_controller.py:59-108)."""
        z_max = np.asarray(z_max, dtype=np.float64)
        z_min = np.asarray(z_min, dtype=np.float64)
        n_steps = len(z_min)
        force_time = n_steps // 2
        print(f"Time of the external force: {(force_time*self.config.dt):.2f}s")
        hist = self._rollout_host(x_init, y_init, z_max, z_min,
                                  self._kick() if self.config.add_force else None, force_time)
        com = hist[:, :, 0].copy()
        y_hist = hist[:, 1, :].reshape(n_steps, 3, 1).copy()
        return com, y_hist

    def generate_state_trajectory_wieber(self, x_init: np.ndarray, y_init: np.ndarray,
                                         z_max: np.ndarray, z_min: np.ndarray
                                         ) -> Tuple[np.ndarray, np.ndarray]:
        """Full x and y state histories (n,3,1) each, no force (zmp_controller.py:110-147)."""
        z_max = np.asarray(z_max, dtype=np.float64)
        z_min = np.asarray(z_min, dtype=np.float64)
        n_steps = len(z_min)
        hist = self._rollout_host(x_init, y_init, z_max, z_min, None, -1)
        return (hist[:, 0, :].reshape(n_steps, 3, 1).copy(),
                hist[:, 1, :].reshape(n_steps, 3, 1).copy())

    def predict_wieber_axis(self, x_init: np.ndarray, nb_steps: int, z_max: np.ndarray,
                            z_min: np.ndarray) -> np.ndarray:
        """One-axis next state (3,1) after the first optimal jerk (zmp_controller.py:149-201)."""
        plan = self._plan(nb_steps)
        x = np.asarray(x_init, dtype=np.float64).reshape(1, 3)
        zx = np.asarray(z_max, dtype=np.float64).reshape(1, -1)
        zn = np.asarray(z_min, dtype=np.float64).reshape(1, -1)
        if zx.shape[1] != nb_steps or zn.shape[1] != nb_steps:
            raise ValueError(f"z_max/z_min must hold nb_steps={nb_steps} rows")
        out, st = plan.step(x, zx, zn)
        if plan.strict:
            self._raise_on_status(st)
        return out.cpu().numpy().reshape(3, 1)

    # ------------------------------------------------------------------ Herdt
    def find_nb_steps(self, state_ref) -> list:
        """(steps to the next footstep change, steps of the current footstep phase) per index
        (zmp_controller.py:203-433)."""
        return herdt.find_nb_steps(state_ref)

    def _polytope_halfspace(self, vertices):
        """Convex polygon → (A, b) with A d <= b (zmp_controller.py:828-865)."""
        return herdt.polytope_halfspace(vertices)

    def generate_com_trajectory_herdt(self, x_init: np.ndarray, y_init: np.ndarray,
                                      v_ref: np.ndarray, state_ref: np.ndarray):
        """COM trajectory (n,2), y state history (n,3,1) and foot positions (n,2) of the Herdt
        joint footstep QP (zmp_controller.py:435-531), every QP on the device."""
        v_ref = np.asarray(v_ref, dtype=np.float64)
        n = len(v_ref)
        x0 = np.stack([np.asarray(x_init, np.float64).reshape(3),
                       np.asarray(y_init, np.float64).reshape(3)])[None]
        kick = np.array([self._kick()]) if self.config.add_force else None
        hist, foot, _ = self._herdt_rollout(x0, v_ref, herdt.encode_states(state_ref), kick,
                                            n // 2)
        hist, foot = hist[0].cpu().numpy(), foot[0].cpu().numpy()
        for i in np.nonzero(np.any(foot[1:] != foot[:-1], axis=1))[0]:
            # zmp_controller.py:510 (the footstep adopted when a single support ends)
            print(f"Je change : de ({foot[i, 0], foot[i, 1]}) à ({foot[i + 1, 0], foot[i + 1, 1]})")
        com = hist[:, :, 0].copy()
        return com, hist[:, 1, :].reshape(n, 3, 1).copy(), foot

    def predict_herdt_joint(self, x_init, y_init, v_ref, x_fc, y_fc, current_state, state_ref,
                            nb_steps, nb_steps_to_next_state, x_airc, y_airc, foot_side, idx):
        """One joint x/y step (zmp_controller.py:533-826): (next x state (3,1), next y state
        (3,1), first planned x footstep or None, first planned y footstep or None).  A solve whose
        swing polytope is infeasible takes the reference's fallback (:796-802): zero jerk (the
        kernel) and the air foot's centre x_airc / y_airc as the first footstep (here; the C-ABI
        step knows only the current foot); one at the pass cap keeps its last iterate."""
        plan = self._plan(nb_steps)
        v = np.asarray(v_ref, np.float64).reshape(1, nb_steps, 2)
        win = herdt.encode_states(state_ref).reshape(1, nb_steps)
        cur = herdt.encode_states([current_state])
        pad = herdt.pad_states(np.concatenate([cur, win[0]]), 0)[None]
        prm = herdt.make_params(self.config, herdt.max_footsteps(pad, nb_steps, 2))
        x = np.stack([np.asarray(x_init, np.float64).reshape(3),
                      np.asarray(y_init, np.float64).reshape(3)])[None]
        foot = np.array([[float(np.asarray(x_fc).reshape(-1)[0]),
                          float(np.asarray(y_fc).reshape(-1)[0])]])
        side = np.array([0 if foot_side == "left" else 1], np.int8)
        xn, step, st = plan.herdt_step(prm, x, v, win, cur, foot, side)
        self._herdt_status(st)
        failed = int(st[0]) & _ST_INFEASIBLE
        xn, step = xn[0].cpu().numpy(), step[0].cpu().numpy()
        fx = None if np.isnan(step[0]) else float(step[0])
        fy = None if np.isnan(step[1]) else float(step[1])
        if failed and fx is not None and x_airc is not None and y_airc is not None:
            fx = float(np.asarray(x_airc).reshape(-1)[0])
            fy = float(np.asarray(y_airc).reshape(-1)[0])
        return xn[0].reshape(3, 1), xn[1].reshape(3, 1), fx, fy

    def generate_com_trajectory_herdt_batch(self, x_init, v_ref, state_ref, F_ext=None,
                                            return_status: bool = False, push: Push = None,
                                            walk_lengths=None, trace: PushTrace = None):
        """Many Herdt walks at once (addition): x_init [B,2,3] or None; v_ref [B,n,2] or a
        shared [n,2]; state_ref [B,n] or a shared [n] (State enums or int8 codes, NumPy or a
        device tensor, which stays on the device); F_ext [B] or None.  Returns (com [B,n,2],
        hist [B,n,2,3], foot [B,n,2]) on the device; with return_status=True also the per-walk
        status [B] (ZMPC_ST_* flags) instead of raising or warning on a failed walk.  push: an
        analysis.Push — a shove of any length, shape and direction instead of F_ext
        (zmpc_herdt_rollout_pushed; not together with F_ext).  The footstep bookkeeping of the
        walks (nb_next, the footstep count that sizes the kernel) is made on the device
        (zmpc_herdt_prepare), whatever their gaits.

        walk_lengths : [B] sample counts of ragged walks padded to n
                (SpeedTrajectoryGenerator.generate_speed_and_state_batch): walk b is then rows
                [0, n_b) alone — its states and v_ref rows at or past n_b are replaced by row
                n_b − 1, which is what the walk alone sees through the rollout's last-row
                padding, and F_ext hits step n_b // 2 of each walk.  Output rows at or past n_b
                are unspecified but finite.
        trace : an analysis.PushTrace — a disturbance per walk, sample and axis instead of F_ext or
                push (zmpc_herdt_rollout_traced; together with either it raises ValueError)."""
        _one_disturbance(F_ext, push, trace)
        v = torch.as_tensor(v_ref, dtype=torch.float64)
        n = int(v.shape[-2])
        st = self._herdt_codes(state_ref)
        if x_init is not None:
            B = int(np.shape(x_init)[0])
        elif v.dim() == 3:
            B = int(v.shape[0])
        elif st.ndim == 2:
            B = int(st.shape[0])
        elif walk_lengths is not None:
            B = int(np.shape(walk_lengths)[0])
        elif push is not None:
            B = push.batch() or 1
        elif trace is not None:
            B = trace.batch()
        else:
            B = 1 if F_ext is None else int(np.size(F_ext))
        x0 = np.zeros((B, 2, 3)) if x_init is None else x_init
        kick = None
        if F_ext is not None and walk_lengths is None:
            kick = self.config.dt * np.asarray(F_ext, np.float64).reshape(B) / self.config.m
        elif F_ext is not None:
            # a kick step per walk: the legacy push of the pushed entry point, at n_b // 2
            steps = _default_force_step(n, self._lengths_host(walk_lengths, B, n))
            push = Push(np.asarray(F_ext, np.float64).reshape(B), +1, steps)
        hist, foot, status = self._herdt_rollout(x0, v_ref, st, kick, n // 2,
                                                 check=not return_status, push=push,
                                                 on_device=True, lengths=walk_lengths,
                                                 trace=trace)
        if return_status:
            return hist[..., 0], hist, foot, status
        return hist[..., 0], hist, foot

    @staticmethod
    def _herdt_codes(state_ref):
        """State enums, their names or int8 codes → int8 NumPy codes; a tensor stays where it
        is."""
        return state_ref if isinstance(state_ref, torch.Tensor) else herdt.encode_states(state_ref)

    @staticmethod
    def _lengths_host(walk_lengths, B, n):
        """walk_lengths as [B] int64 on the host, clamped to [1, n] as the kernels clamp them."""
        t = walk_lengths.cpu().numpy() if isinstance(walk_lengths, torch.Tensor) else walk_lengths
        return np.clip(np.asarray(t, np.int64).reshape(B), 1, n)

    def _herdt_device(self, plan, st, v_ref, lengths=None):
        """The preparation of a batched Herdt rollout on the device (Plan.herdt_prepare): (params
        sized by the most footsteps in a window of any walk, states, nb_next, v_ref).  With
        lengths [B] the states are walk b's own, continued by its last live state, and so are
        the rows of v_ref (a gather on the device)."""
        clean, nb, _, most = plan.herdt_prepare(st, lengths)
        prm = herdt.make_params(self.config, most)
        if lengths is None:
            return prm, clean, nb, v_ref
        dev = clean.device
        v = torch.as_tensor(v_ref, dtype=torch.float64, device=dev)
        B, n = clean.shape
        last = torch.as_tensor(lengths, dtype=torch.int64, device=dev).reshape(B).clamp(1, n) - 1
        rows = torch.minimum(torch.arange(n, device=dev)[None, :], last[:, None])
        if v.dim() == 2 and v.shape[0] == n:
            v = v[rows]
        elif v.dim() == 3 and tuple(v.shape) == (B, n, 2):
            v = torch.gather(v, 1, rows[:, :, None].expand(B, n, 2))
        return prm, clean, nb, v  # (any other shape: Plan.herdt_rollout names it)

    def _herdt_host(self, plan, st):
        """The host preparation of a Herdt rollout from the int8 states [B, n] or [n]: (params
        sized by the most footsteps in a window of the padded states, nb_next shaped as st)."""
        N = plan.N
        st2 = np.atleast_2d(st)
        pad = np.concatenate([st2, np.repeat(st2[:, -1:], N, axis=1)], axis=1)
        n = st2.shape[1]
        prm = herdt.make_params(self.config, herdt.max_footsteps(pad, N, n))
        nb = np.array([[t[0] for t in herdt.find_nb_steps(p)][:n] for p in pad], np.int32)
        return prm, (nb[0] if st.ndim == 1 else nb)

    def _herdt_rollout(self, x0, v_ref, st, kick, kick_step, check=True, push=None,
                       on_device=False, lengths=None, trace=None):
        plan = self._plan()
        if on_device:
            prm, st, nb, v_ref = self._herdt_device(plan, st, v_ref, lengths)
        else:
            prm, nb = self._herdt_host(plan, st)
        hist, foot, status = plan.herdt_rollout(prm, v_ref, st, nb, x0, kick=kick,
                                                kick_step=kick_step, push=push,
                                                mass=self.config.m, trace=trace)
        if check:
            self._herdt_status(status)
        return hist, foot, status

    # ------------------------------------------------------------------ batched additions
    def generate_state_trajectory_batch(self, x_init, z_max, z_min, F_ext=None,
                                        force_step: Optional[int] = None, walk_lengths=None,
                                        push: Push = None, trace: PushTrace = None):
        """Many walks at once; every input may be NumPy or a torch tensor.

        x_init : [B,2,3] initial (x-axis, y-axis) states, or None for zeros
        z_max, z_min : [B,n,2] per-walk CoP bounds, or [n,2] one CoP for every walk
        F_ext : None (no disturbance) or [B] forces in N; the y velocity at history index
                force_step+1 drops by dt·F_ext/m (default force_step = n//2, as
                zmp_controller.py:90,105-106)
        walk_lengths : [B] sample counts of ragged walks padded to n with their last row
                (CoPGenerator.generate_cop_batch); the force then hits step n_b//2 of each
                walk and hist[b, :n_b] is walk b's history
        push : an analysis.Push — a shove of any length, shape and direction instead of F_ext
                (zmpc_rollout_pushed).  It carries its own start step(s): together with F_ext,
                force_step or walk_lengths it raises ValueError (hist[b, :n_b] of a ragged walk
                is still walk b's history; give the steps n_b // 2 in the push)
        trace : an analysis.PushTrace — a disturbance per walk, sample and axis instead of F_ext
                or push (zmpc_rollout_traced).  It carries its own start step(s) too: together with
                F_ext, push, force_step or walk_lengths it raises ValueError
        Returns (hist [B,n,2,3], status [B]) on the plan's device.
        """
        _one_disturbance(F_ext, push, trace, force_step, walk_lengths)
        plan, zmax_t, zmin_t, x0, kick, step = self._batch_inputs(x_init, z_max, z_min, F_ext,
                                                                  force_step, walk_lengths)
        given = push if push is not None else trace
        if given is not None:
            if x_init is None and zmax_t.dim() == 2 and given.batch():
                x0 = x0.expand(given.batch(), 2, 3).contiguous()
            hist, st = plan.rollout(zmax_t, zmin_t, x0, push=push, trace=trace,
                                    mass=self.config.m)
        else:
            hist, st = plan.rollout(zmax_t, zmin_t, x0, kick=kick, kick_step=step)
        if plan.strict:
            self._raise_on_status(st)
        return hist, st

    def _scenario(self, plan, z_max, z_min, x_init, walk_lengths, sized=(), planar=False):
        """The scenario batch of the batch and robustness methods on plan's device:
        (z_max, z_min, x0 [B,2,3], B, n, lengths [B] or None).  B comes from x_init, else from
        per-walk bounds [B,n,2], else from the first [B] argument of `sized` (the arguments that
        may be scalars or [B]), else it is 1; x_init None gives zero states.  A [B'] argument of
        `sized` with B' != B raises ValueError, with planar=True in critical_force's wording."""
        f64 = dict(dtype=torch.float64, device=torch.device("cuda", plan.device))
        zmax_t = torch.as_tensor(z_max, **f64).contiguous()
        zmin_t = torch.as_tensor(z_min, **f64).contiguous()
        B = _batch_size(((x_init, None), (zmax_t, 3)), sized,
                        "force_step, direction and walk_lengths must be scalars or [B] = [{B}]"
                        + (" (planar directions [1, 2] or [B, 2])" if planar else ""))
        x0 = torch.zeros((B, 2, 3), **f64) if x_init is None else torch.as_tensor(x_init, **f64)
        lengths = None
        if walk_lengths is not None:
            lengths = torch.as_tensor(walk_lengths, dtype=torch.int64,
                                      device=f64["device"]).reshape(B)
        return zmax_t, zmin_t, x0, B, int(zmax_t.shape[-2]), lengths

    def _batch_inputs(self, x_init, z_max, z_min, F_ext, force_step, walk_lengths):
        """Device inputs of the batch methods: (plan, z_max, z_min, x0, kick, kick step(s)).
        Only x_init and per-walk bounds size the batch; with walk_lengths the kick hits n_b // 2
        whatever force_step says."""
        plan = self._plan()
        zmax_t, zmin_t, x0, B, n, lengths = self._scenario(plan, z_max, z_min, x_init,
                                                           walk_lengths)
        kick = None
        if F_ext is not None:
            F = torch.as_tensor(F_ext, dtype=torch.float64, device=x0.device).reshape(B)
            kick = self.config.dt * F / self.config.m
        if lengths is not None or force_step is None:
            step = _default_force_step(n, lengths)
        else:
            step = int(force_step)
        return plan, zmax_t, zmin_t, x0, kick, step

    def generate_walk_metrics_batch(self, x_init, z_max, z_min, F_ext=None,
                                    force_step: Optional[int] = None, walk_lengths=None):
        """The walks of generate_state_trajectory_batch (same arguments) reduced to their
        robustness metrics in one launch (addition; zmpc_rollout_metrics): what walk_metrics
        returns for that method's history, which is never written — 96 bytes per walk leave the
        device's registers instead of n·48.  With walk_lengths the metrics cover each walk's own
        n_b samples.  Returns (analysis.WalkMetrics, status [B]) on the plan's device.  Strict
        plans and walks of more than 513 samples run the two launches behind the same call."""
        plan, zmax_t, zmin_t, x0, kick, step = self._batch_inputs(x_init, z_max, z_min, F_ext,
                                                                  force_step, walk_lengths)
        m, st = plan.rollout_metrics(zmax_t, zmin_t, x0, kick=kick, kick_step=step,
                                     lengths=walk_lengths)
        if plan.strict:
            self._raise_on_status(st)
        return WalkMetrics(m), st

    def generate_com_trajectory_batch(self, x_init, z_max, z_min, F_ext=None,
                                      force_step: Optional[int] = None, walk_lengths=None,
                                      push: Push = None, trace: PushTrace = None):
        """Batched generate_com_trajectory_wieber: (com [B,n,2], hist [B,n,2,3]) on device;
        push and trace as generate_state_trajectory_batch."""
        hist, _ = self.generate_state_trajectory_batch(x_init, z_max, z_min, F_ext, force_step,
                                                       walk_lengths, push=push, trace=trace)
        return hist[..., 0], hist

    def zmp(self, hist):
        """ZMP estimate C·state (run_mpc.py:294) for a [..., 3] state tensor or array."""
        C = self.C
        if isinstance(hist, torch.Tensor):
            return hist @ torch.as_tensor(C, dtype=hist.dtype, device=hist.device)
        return np.asarray(hist) @ C

    # ------------------------------------------------------------------ robustness analysis
    def walk_metrics(self, hist, z_max, z_min, walk_lengths=None) -> WalkMetrics:
        """Per-walk robustness metrics of a state history (addition; zmpc_walk_metrics): the ZMP
        of run_mpc.py:294 against the support box of its sample, as
        run_compare_resistance.py:173-197 plots them, reduced on the device.

        hist [B,n,2,3] (a batch method's output; a NumPy array is staged to the device);
        z_max, z_min [B,n,2] or a shared [n,2]; walk_lengths [B] live samples of ragged walks.
        Returns analysis.WalkMetrics: named [B,2] (x, y) columns — viol_max, viol_argmax,
        viol_count, com_dev_max, zmp_rms, dcm_end — over one [B,12] device tensor."""
        plan = self._plan()
        dev = torch.device("cuda", plan.device)
        h = torch.as_tensor(hist, dtype=torch.float64, device=dev).contiguous()
        return WalkMetrics(plan.walk_metrics(h, z_max, z_min, lengths=walk_lengths))

    def critical_force(self, z_max, z_min, x_init=None, force_step=None, direction=+1,
                       F_hi: float = 1000.0, iters: int = 30, max_violation: float = 1e-9,
                       max_com_dev: Optional[float] = None,
                       max_dcm_end: Optional[float] = None, walk_lengths=None,
                       fused: bool = False, duration: int = 1, profile=None,
                       trace: PushTrace = None):
        """Largest push each scenario survives (addition): the question the F_ext sweep of
        run_compare_resistance.py:87-169 puts to the eye, answered by bisection on the device.

        B scenarios — from x_init [B,2,3], per-walk bounds [B,n,2], or a [B] force_step or
        direction.  Scenario b is pushed at history step force_step[b] (default n//2, or
        n_b//2 with walk_lengths) by direction[b]·F newtons on the y axis only, as the
        reference pushes (zmp_controller.py:105-106).  A push passes when, on both axes,
        viol_max <= max_violation and, where set, com_dev_max <= max_com_dev and
        |dcm_end| <= max_dcm_end (and, on a strict plan, the solver reported no failure).
        Bisection on F in [0, F_hi]: each of the iters + 2 evaluations is one batched rollout
        into one reused history buffer, one walk_metrics launch and a torch.where on the
        bracket; nothing is copied to the host.  With fused=True each evaluation is one
        zmpc_rollout_metrics launch into the reused [B,12] tensor and no history buffer exists
        (B·n·48 bytes less on the device: 20 GB against 96 MB of metrics for a million 420-sample
        scenarios); it needs a shape with a fused form (Plan.rollout_metrics) and raises
        otherwise.  Its value slots agree with the two launches to rounding, so a bracket can
        differ where a push lands a sample within rounding of max_violation.

        Returns (F_lo, F_hi), [B] device tensors: the final bracket, F_lo passes and F_hi fails,
        F_hi − F_lo = F_hi/2**iters.  NaN in both where the walk fails with no push at all;
        F_lo = F_hi = the search limit where it passes even there.

        Bisection assumes that pass/fail is monotone in F.  For the unconstrained controller
        with a passing unpushed walk that is exact: the closed loop is linear, every ZMP sample
        is affine in F, so the passing set is an interval that contains 0.  For strict plans
        it is an assumption (the clamped ZMP hides the push until the QP fails or the CoM
        criteria trip).

        duration, profile: a shove that lasts `duration` samples from force_step on, with force
        F·profile[j] in its j-th sample (None: constant).  direction may also hold planar vectors
        (dx, dy), as a two-dimensional [1, 2] or [B, 2] array (a bare pair stays two signs, as in
        critical_force_exact): F is then the magnitude of a push along that direction.  A scalar
        or [B] sign with duration 1 and no profile keeps the launches above; otherwise each
        evaluation is one pushed rollout (zmpc_rollout_pushed — on a strict plan the push window
        of the strict kernels) plus walk_metrics, and fused=True raises ValueError.

        trace: an analysis.PushTrace instead of force_step, direction, duration and profile (given
        together they raise ValueError).  The bisection then runs on the scale λ of each walk's
        own trace, dv = λ·dv₁ with λ in [0, F_hi]: the returned bracket holds the largest multiple
        of its trace that walk survives.  Everything else is as for a shove — one traced rollout
        (zmpc_rollout_traced) plus walk_metrics per evaluation, the [B, L, C] velocity steps
        scaled on the device — and fused=True raises ValueError."""
        D, w = check_profile(duration, profile)
        planar = np.ndim(direction) == 2
        traced = trace is not None
        if traced:
            _trace_alone(trace, force_step, direction, D, w)
            if fused:
                raise ValueError("fused=True has no traced form: a trace runs a traced rollout "
                                 "plus walk_metrics")
        shove = planar or D != 1 or w is not None
        if shove and fused:
            raise ValueError("fused=True has no pushed form: a shove (duration, profile or a "
                             "planar direction) runs a pushed rollout plus walk_metrics")
        unit = unit_directions(direction) if planar else None
        plan = self._plan()
        dev = torch.device("cuda", plan.device)
        f64 = dict(dtype=torch.float64, device=dev)
        zmax_t, zmin_t, x0, B, n, lengths = self._scenario(
            plan, z_max, z_min, x_init, walk_lengths,
            sized=(force_step, walk_lengths, _direction_size(direction, unit),
                   np.empty(trace.batch()) if traced else None), planar=True)
        if not (F_hi > 0) or iters < 0:
            raise ValueError("need F_hi > 0 and iters >= 0")
        sign = None if planar else \
            torch.sign(torch.as_tensor(direction, **f64)).expand(B).contiguous()
        step = _force_step(force_step, n, lengths)
        if not isinstance(step, int):
            step = torch.as_tensor(step, dtype=torch.int64, device=dev)
        kick = torch.zeros(B, **f64)
        metrics = torch.empty((B, NMETRICS), **f64)
        scaled = unit1 = None  # a shove's or trace's buffer the launch reads, and its copy for 1 N
        if traced:
            # (a copy of the trace at scale 1: the launch's buffer is rewritten per evaluation)
            launch = plan.rollout_launcher(zmax_t, zmin_t, x0, trace=trace.scaled(1.0),
                                           mass=self.config.m)
            scaled, unit1 = launch.trace_dv, launch.trace_dv.clone()  # [B, L, C] at λ = 1
        elif shove:
            F1, d1 = _unit_push(None if planar else sign.cpu().numpy(), unit, B)
            st = step.cpu().numpy() if isinstance(step, torch.Tensor) else step
            push = Push(F1, d1, st, duration=D, profile=w)
            launch = plan.rollout_launcher(zmax_t, zmin_t, x0, push=push, mass=self.config.m)
            scaled, unit1 = launch.push_amp, launch.push_amp.clone()  # [B, C] for 1 N
        elif fused:
            launch = plan.rollout_metrics_launcher(zmax_t, zmin_t, x0, kick=kick, kick_step=step,
                                                   lengths=lengths, out=metrics)
        else:
            launch = plan.rollout_launcher(zmax_t, zmin_t, x0, kick=kick, kick_step=step)
        m = WalkMetrics(metrics)
        dt, mass = self.config.dt, self.config.m

        def passes(F):
            if scaled is not None:
                scaled.copy_(unit1 * F.reshape((-1,) + (1,) * (unit1.dim() - 1)))
            else:
                kick.copy_(dt * (sign * F) / mass)  # zmp_controller.py:106
            launch()
            if not fused:
                plan.walk_metrics(launch.hist, zmax_t, zmin_t, lengths=lengths, out=metrics)
            ok = (m.viol_max <= max_violation).all(dim=1)  # (+inf and NaN fail)
            if max_com_dev is not None:
                ok &= (m.com_dev_max <= max_com_dev).all(dim=1)
            if max_dcm_end is not None:
                ok &= (m.dcm_end.abs() <= max_dcm_end).all(dim=1)
            if plan.strict:
                ok &= launch.status == 0
            return ok

        return _bisect(passes, B, F_hi, iters, f64)

    # ------------------------------------------------------------------ Herdt robustness
    def herdt_walk_metrics(self, hist, foot, state_ref, foot_ref=None,
                           walk_lengths=None) -> HerdtWalkMetrics:
        """Did a Herdt walk stay up (addition; zmpc_herdt_walk_metrics)?  The support box of a
        Herdt walk follows the footsteps its QP chose, so it is rebuilt from the walk's own feet:
        sample i against the box round foot[i − 1], reduced on the device.

        hist [B,n,2,3], foot [B,n,2]: generate_com_trajectory_herdt_batch's outputs (NumPy arrays
        are staged to the device); state_ref [B,n] or a shared [n], as that method took it;
        foot_ref [B,n,2] or [n,2]: the feet of the unpushed walk, for step_shift_max;
        walk_lengths [B] live samples.  Returns analysis.HerdtWalkMetrics over one [B,16] device
        tensor.  The QP is always feasible, so viol_max stays at rounding noise under any push:
        read dcm_dev_max to see whether the robot fell."""
        plan = self._plan()
        dev = torch.device("cuda", plan.device)
        h = torch.as_tensor(hist, dtype=torch.float64, device=dev).contiguous()
        f = torch.as_tensor(foot, dtype=torch.float64, device=dev).contiguous()
        prm = herdt.make_params(self.config, 0)
        return HerdtWalkMetrics(plan.herdt_walk_metrics(
            prm, h, f, self._herdt_codes(state_ref), lengths=walk_lengths, foot_ref=foot_ref))

    def critical_force_herdt(self, v_ref, state_ref, max_dcm_dev, x_init=None, force_step=None,
                             direction=+1, F_hi: float = 1000.0, iters: int = 30,
                             max_violation: float = 1e-9, max_com_dev: Optional[float] = None,
                             duration: int = 1, profile=None, walk_lengths=None,
                             trace: PushTrace = None):
        """Largest shove each scenario of the footstep-adapting controller survives (addition):
        critical_force for Herdt walks, with its bisection, bracket and NaN conventions.

        B scenarios — from x_init [B,2,3], per-walk v_ref [B,n,2] or state_ref [B,n], or a [B]
        force_step or direction.  Scenario b is pushed from history step force_step[b] on
        (default n//2) for `duration` samples with force F·profile[j] (None: constant), by
        direction[b]·F newtons on the y axis, or along planar vectors (dx, dy) given as a
        two-dimensional [1, 2] or [B, 2] array.  A push passes when the solver reported nothing
        (status == 0) and, on both axes, viol_max <= max_violation, dcm_dev_max <= max_dcm_dev
        and, where set, com_dev_max <= max_com_dev.

        max_dcm_dev has no default, because it is the verdict: the joint QP is always feasible
        (the jerk is unbounded), so under any push the ZMP stays on its box edge and viol_max at
        rounding noise while the CoM runs away.  The divergent component of motion relative to
        the supporting foot tells: it stays within a step length on a walk that recovers and grows
        exponentially on one that does not, so any bound of a step length or so (1 m, say) gives
        nearly the same force.

        walk_lengths: [B] sample counts of ragged walks padded to n, as
        generate_com_trajectory_herdt_batch takes them: scenario b is walk b alone (its states and
        v_ref rows continued by row n_b − 1), the default force_step is n_b // 2 of each walk and
        the metrics cover its own n_b samples.

        The preparation (padded states, nb_next, max_footsteps) is done once, on the device
        (zmpc_herdt_prepare), whatever the walks' gaits.  Each of the
        iters + 2 evaluations is one zmpc_herdt_rollout_pushed into reused buffers, its [B, C]
        amplitudes scaled on the device, and one zmpc_herdt_walk_metrics launch; nothing is
        copied to the host inside the loop.  The unpushed evaluation comes first and its feet are
        the foot_ref of the later ones.

        Returns (F_lo, F_hi), [B] device tensors: F_lo passes, F_hi fails, F_hi − F_lo =
        F_hi/2**iters; NaN in both where the walk fails unpushed; F_lo = F_hi = the search limit
        where it passes even there.  Bisection assumes that pass/fail is monotone in F.  That is
        an assumption here, as for strict plans in critical_force: the controller is piecewise
        linear; on the walks of the tests the passing set was one interval.

        trace: an analysis.PushTrace instead of force_step, direction, duration and profile (given
        together they raise ValueError): the bisection runs on the scale λ in [0, F_hi] of each
        walk's own trace, one zmpc_herdt_rollout_traced per evaluation."""
        D, w = check_profile(duration, profile)
        traced = trace is not None
        if traced:
            _trace_alone(trace, force_step, direction, D, w)
        if max_dcm_dev is None or not (float(max_dcm_dev) > 0):
            raise ValueError("max_dcm_dev must be a positive bound in metres: the ZMP of a Herdt "
                             "walk never tells whether the robot fell, the DCM does")
        if not (F_hi > 0) or iters < 0:
            raise ValueError("need F_hi > 0 and iters >= 0")
        planar = np.ndim(direction) == 2
        unit = unit_directions(direction) if planar else None
        plan = self._plan()
        dev = torch.device("cuda", plan.device)
        f64 = dict(dtype=torch.float64, device=dev)
        v = torch.as_tensor(v_ref, **f64).contiguous()
        n = int(v.shape[-2])
        st = self._herdt_codes(state_ref)
        sized = (force_step, _direction_size(direction, unit), walk_lengths,
                 np.empty(trace.batch()) if traced else None)
        B = _batch_size(((x_init, None), (v, 3), (st, 2)), sized,
                        "force_step and direction must be scalars or [B] = [{B}] (planar "
                        "directions [1, 2] or [B, 2])")
        x0 = torch.zeros((B, 2, 3), **f64) if x_init is None else torch.as_tensor(x_init, **f64)
        lengths = None
        if force_step is None and walk_lengths is not None:
            lengths = self._lengths_host(walk_lengths, B, n)
        step = _force_step(force_step, n, lengths)
        if not isinstance(step, int):
            step = np.asarray(torch.as_tensor(step).cpu(), np.int64)
        F1, d1 = _unit_push(direction, unit, B)
        prm, st, nb, v = self._herdt_device(plan, st, v, walk_lengths)
        if traced:
            # (a copy of the trace at scale 1: the launch's buffer is rewritten per evaluation)
            launch = plan.herdt_rollout_launcher(prm, v, st, nb, x0, mass=self.config.m,
                                                 trace=trace.scaled(1.0))
            scaled, amp1 = launch.trace_dv, launch.trace_dv.clone()  # [B, L, C] at λ = 1
        else:
            launch = plan.herdt_rollout_launcher(prm, v, st, nb, x0,
                                                 Push(F1, d1, step, duration=D, profile=w),
                                                 self.config.m)
            scaled, amp1 = launch.push_amp, launch.push_amp.clone()  # [B, C] for 1 N
        metrics = torch.empty((B, NHERDT_METRICS), **f64)
        foot_ref = torch.empty_like(launch.foot)
        measure, measure_ref = (plan.herdt_walk_metrics_launcher(
            prm, launch.hist, launch.foot, launch.states, lengths=walk_lengths, foot_ref=ref,
            count_tol=max_violation, out=metrics) for ref in (None, foot_ref))
        m = HerdtWalkMetrics(metrics)

        def passes(F):
            scaled.copy_(amp1 * F.reshape((-1,) + (1,) * (amp1.dim() - 1)))
            launch()
            measure()
            ok = (m.viol_max <= max_violation).all(dim=1)  # (+inf and NaN fail)
            ok &= (m.dcm_dev_max <= max_dcm_dev).all(dim=1)
            if max_com_dev is not None:
                ok &= (m.com_dev_max <= max_com_dev).all(dim=1)
            return ok & (launch.status == 0)

        def keep_unpushed_feet():
            # the unpushed walk's feet are the foot_ref of every later evaluation
            nonlocal measure
            foot_ref.copy_(launch.foot)
            measure = measure_ref

        return _bisect(passes, B, F_hi, iters, f64, after_unpushed=keep_unpushed_feet)

    def _unpushed(self, z_max, z_min, x_init, walk_lengths, extra=()):
        """One unpushed rollout for the push map: (plan, hist, zmax, zmin, lengths, B, n)."""
        plan = self._plan()
        if plan.strict:
            raise RuntimeError("the push map needs the unconstrained controller: the ZMP response "
                               "of a strict (clamped) plan is not affine in the push — use "
                               "critical_force")
        zmax_t, zmin_t, x0, B, n, lengths = self._scenario(plan, z_max, z_min, x_init,
                                                           walk_lengths, (*extra, walk_lengths))
        hist, _ = plan.rollout(zmax_t, zmin_t, x0)
        return plan, hist, zmax_t, zmin_t, lengths, B, n

    def push_map(self, z_max, z_min, x_init=None, walk_lengths=None,
                 max_violation: float = 1e-9, duration: int = 1, profile=None,
                 axes: str = "y") -> PushMap:
        """At which phase of the gait, and in which direction, is each walk weakest (addition;
        zmpc_push_map): one unpushed rollout, then the exact critical push of every (walk, push
        step, direction) in one launch — the F_ext sweep of run_compare_resistance.py:87-197 at
        every step at once.  x_init [B,2,3] or None; z_max, z_min [B,n,2] or a shared [n,2];
        walk_lengths [B] live samples of ragged walks.  Returns analysis.PushMap on the device:
        force [B,n,2] in newtons ([..., 0] a +y push at that history step, [..., 1] a −y push,
        as zmp_controller.py:105-106 applies it), +inf where no sample limits the push (steps
        from n_b − 2 on), NaN for a walk that fails with no push; limit [B,n,2] the sample that
        leaves its box first; weakest() the per-walk minimum.  Unconstrained plans only.

        duration, profile: a push that lasts `duration` samples from that history step on, with
        force F·profile[j] in its j-th sample (None: constant); the entries are then the critical
        F.  axes "x", "y" or "xy": the axis pushed — the columns are (+x, −x), (+y, −y) or
        (+x, −x, +y, −y) (zmpc_push_map_shaped); PushMap.rose gives any planar direction from an
        "xy" map, weakest_push() the per-walk minimum of every map."""
        plan, hist, zmax_t, zmin_t, lengths, _, _ = self._unpushed(z_max, z_min, x_init,
                                                                   walk_lengths)
        force, limit = plan.push_map(hist, zmax_t, zmin_t, lengths=lengths,
                                     max_violation=max_violation, mass=self.config.m,
                                     duration=duration, profile=profile, axes=axes)
        return PushMap(force, limit, axes=axes)

    def critical_force_exact(self, z_max, z_min, x_init=None, force_step=None, direction=+1,
                             max_violation: float = 1e-9, walk_lengths=None, duration: int = 1,
                             profile=None):
        """critical_force's scenarios (same conventions and defaults: force_step defaults to
        n//2, or n_b//2 with walk_lengths; direction[b]·F newtons on the y axis) answered in
        closed form (addition; the single-step form of zmpc_push_map): one unpushed rollout and
        one launch instead of 32 pushed rollouts, a number instead of a bracket.  Returns [B]
        forces on the device: NaN where the walk fails with no push, +inf where no push at that
        step ever fails (critical_force reports its search limit there).  Only the ZMP criterion
        (max_violation); raises on a strict plan.

        duration, profile: a sustained or shaped push as push_map.  direction may also hold
        planar vectors (dx, dy), as a two-dimensional [1, 2] or [B, 2] array (a bare pair stays
        two signs): the result is then the critical magnitude of a push along that direction,
        from the x and y tables of one launch (analysis.planar_push)."""
        planar = np.ndim(direction) == 2
        unit = unit_directions(direction) if planar else None
        plan, hist, zmax_t, zmin_t, lengths, B, n = self._unpushed(
            z_max, z_min, x_init, walk_lengths,
            extra=(force_step, _direction_size(direction, unit)))
        dev = hist.device
        if force_step is None:
            force_step = _default_force_step(n, lengths)
        step = torch.as_tensor(force_step, dtype=torch.int64, device=dev).expand(B)
        force, limit = plan.push_map(hist, zmax_t, zmin_t, lengths=lengths,
                                     push_steps=step.contiguous(), max_violation=max_violation,
                                     mass=self.config.m, duration=duration, profile=profile,
                                     axes="xy" if planar else "y")
        if planar:
            return planar_push(force, limit, unit)[0]
        sign = torch.as_tensor(direction, dtype=torch.float64, device=dev).expand(B)
        return torch.where(sign >= 0, force[:, 0], force[:, 1])

    def trace_margin(self, z_max, z_min, trace: PushTrace, x_init=None, walk_lengths=None,
                     max_violation: float = 1e-9, draws: int = 1) -> TraceMargin:
        """The largest multiple of its trace each (walk, draw) survives, in closed form (addition;
        zmpc_trace_margin): one unpushed rollout of the B walks, then one launch over the
        B·draws rows of `trace` — no rollout per evaluation and no history per draw.  Row
        b·draws + k of the trace is the k-th disturbance draw of walk b, so many random draws
        per nominal walk cost one rollout; TraceMargin.survival() is then the fraction of a walk's
        draws it survives.

        z_max, z_min [B,n,2] or a shared [n,2]; x_init [B,2,3] or None; walk_lengths [B] live
        samples of ragged walks; trace: an analysis.PushTrace with B·draws rows (ValueError
        otherwise).  Returns analysis.TraceMargin on the device: scale [B, draws, 2] ([..., 0]
        the trace, [..., 1] the negated trace; +inf where no sample limits it, NaN where the walk
        fails undisturbed) and limit [B, draws, 2].  Only the ZMP criterion (max_violation), and
        unconstrained plans only: a strict plan raises RuntimeError.  critical_force(trace=)
        remains for what this cannot answer — strict plans, whose clamped response is not affine
        in the scale, and the CoM and DCM criteria (max_com_dev, max_dcm_end)."""
        if not isinstance(trace, PushTrace):
            raise ValueError(f"trace must be an analysis.PushTrace, got {type(trace).__name__}")
        if isinstance(draws, bool) or not isinstance(draws, (int, np.integer)) or draws < 1:
            raise ValueError(f"draws must be an integer >= 1, got {draws!r}")
        if trace.batch() % int(draws):
            raise ValueError(f"the trace holds {trace.batch()} rows, not a multiple of draws = "
                             f"{draws} (row b·draws + k is draw k of walk b)")
        # the walks the other arguments name (as _scenario counts them), else the trace's own
        walks = trace.batch() // int(draws)
        named = np.shape(x_init)[0] if x_init is not None else \
            (np.shape(z_max)[0] if np.ndim(z_max) == 3 else walks)
        if named != walks:
            raise ValueError(f"the trace holds {trace.batch()} rows, B·draws = {named}·{draws} = "
                             f"{named * int(draws)} are needed (row b·draws + k is draw k of "
                             "walk b)")
        plan, hist, zmax_t, zmin_t, lengths, _, _ = self._unpushed(
            z_max, z_min, x_init, walk_lengths, extra=(np.empty(walks),))
        scale, limit = plan.trace_margin(hist, zmax_t, zmin_t, trace, draws=int(draws),
                                         lengths=lengths, max_violation=max_violation,
                                         mass=self.config.m)
        return TraceMargin(scale, limit)

    # ------------------------------------------------------------------ internals
    def _rollout_host(self, x_init, y_init, z_max, z_min, kick, kick_step) -> np.ndarray:
        if z_max.ndim != 2 or z_max.shape[1] != 2 or z_min.shape != z_max.shape:
            raise ValueError("z_max and z_min must both be [n_steps, 2]")
        plan = self._plan()
        x0 = np.stack([np.asarray(x_init, dtype=np.float64).reshape(3),
                       np.asarray(y_init, dtype=np.float64).reshape(3)])[None]
        kick_arr = None if kick is None else np.array([kick], dtype=np.float64)
        hist, st = plan.rollout(z_max[None], z_min[None], x0, kick=kick_arr, kick_step=kick_step)
        if plan.strict:
            self._raise_on_status(st)
        return hist[0].cpu().numpy()
