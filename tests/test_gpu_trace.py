"""Device tests of rollouts under per-walk traces (zmpc_rollout_traced, zmpc_herdt_rollout_traced):
a disturbance per walk, sample and axis on the strict kernels (csrc/strict_lq.hip,
strict_scan.hip), the Herdt kernel (csrc/herdt.hip) and, by the scan of csrc/trace.hip, on
unconstrained plans.

The references are the oracle loops of tests/push_rollout_cases.py under the fixed inputs of
tests/trace_cases.py (tests/test_trace_host.py proves them fair on the CPU) and, for the
unconstrained controller, the oracle's unpushed history minus the response in extended precision
(anchored there on chained oracle rollouts).  Bars, the project's existing ones: strict and Herdt
CoM RMSE and states 1e-9, Herdt histories 1e-8, unconstrained CoM RMSE 1e-9 and states 1e-7, forms
of the same solution 1e-11 (include/zmpc.h)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import herdt_cases as hc
import push_rollout_cases as pr
import push_shaped_cases as ps
import strict_cases as sc
import trace_cases as tc
from conftest import golden, rmse
from oracle import zmp_oracle as O

pytestmark = pytest.mark.gpu

from mpc_bipedal import _native  # noqa: E402
from mpc_bipedal.analysis import AXES, Push, PushTrace  # noqa: E402
from mpc_bipedal.config import MPCConfig  # noqa: E402
from mpc_bipedal.controllers import ZMPController  # noqa: E402
from mpc_bipedal.controllers import herdt as H  # noqa: E402
from mpc_bipedal.solver import Plan  # noqa: E402

BAR = 1e-9
PAIR = 1e-11
PAR150 = (150, 0.01, 0.75, 9.81, 1.0, 1e-6)  # the default walk's plan (walk_n150.npz)
PAR64 = (64, 0.01, 0.75, 9.81, 1.0, 1e-6)    # walk_n64.npz
MASS = 40.0
_PLANS = {}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    _native.load()
    yield
    for p in _PLANS.values():
        p.destroy()
    _PLANS.clear()


def strict_plan(N, dt, solver=0, kick_order=1):
    key = ("strict", N, dt)
    if key not in _PLANS:
        Q, R, h = sc.WEIGHTS[0]
        _PLANS[key] = Plan(torch.cuda.current_device(), N, dt, h, sc.G, Q, R, True)
    p = _PLANS[key]
    p.set_option("strict_solver", solver)
    p.set_option("kick_order", kick_order)
    return p


def unc_plan(par):
    key = ("unc",) + par
    if key not in _PLANS:
        _PLANS[key] = Plan(torch.cuda.current_device(), *par, False)
    return _PLANS[key]


def herdt_plan(cfg):
    key = ("herdt", cfg.horizon, cfg.dt)
    if key not in _PLANS:
        _PLANS[key] = Plan(torch.cuda.current_device(), cfg.horizon, cfg.dt, cfg.h, cfg.g, 1.0,
                           1e-6, False)
    return _PLANS[key]


def herdt_inputs(cfg, states, n):
    N = cfg.horizon
    st2 = np.atleast_2d(states)
    pad = np.concatenate([st2, np.repeat(st2[:, -1:], N, axis=1)], axis=1)
    nb = np.array([[t[0] for t in H.find_nb_steps(p)][:n] for p in pad], np.int32)
    return H.make_params(cfg, H.max_footsteps(pad, N, n)), nb


def dev(a, dtype=torch.float64):
    return torch.as_tensor(a, dtype=dtype, device="cuda").contiguous()


def vp(x):
    return None if x is None else ctypes.c_void_p(x.data_ptr())


def bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)) \
        .view(np.int64)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def trace_of(dv, steps, axes="xy"):
    """PushTrace of velocity steps dv [B, L, C]; steps an int or [B]."""
    return PushTrace.from_velocity_steps(np.ascontiguousarray(dv), steps, axes)


def assert_hist(h, st, ref, label):
    assert not st.any(), (label, st)
    r, e = rmse(h[..., 0], ref[..., 0]), sc.rel_err(h, ref)
    print(f"MEASURED {label}: CoM RMSE {r:.2e} state {e:.2e}")
    assert r <= BAR and e <= BAR, (label, r, e)


def walk_bounds(n):
    """n samples of the default walk's bounds (420 stored; beyond, its last row repeated)."""
    d = golden("walk_n150.npz")
    zx, zn = d["zmax"], d["zmin"]
    if n > len(zx):
        zx = np.concatenate([zx, np.repeat(zx[-1:], n - len(zx), axis=0)])
        zn = np.concatenate([zn, np.repeat(zn[-1:], n - len(zn), axis=0)])
    return np.ascontiguousarray(zx[:n]), np.ascontiguousarray(zn[:n])


# ------------------------------------------------------------- 1: a constant window as a trace

def _window_runs(n, B):
    """(D, step or steps [B]) of the windows: D = 3 at step 0, D = 7 at step 20, D = 7 at n − 4
    (truncated), and one run with a start step per walk, one of them outside the range."""
    per_walk = np.array([(3 * b) % (n - 1) for b in range(B)], np.int64)
    per_walk[B - 1] = n - 1
    per_walk[0] = -1 if B > 2 else per_walk[0]
    return ((3, 0), (7, min(20, n - 3)), (7, n - 4), (5, per_walk))


def _window_pair(B, D, steps, dt, w=None, amp_scale=1.0):
    """A Push of B walks with different forces and planar directions, and the same disturbance
    spelled as a trace: rows amp[b] (times w_j with a profile)."""
    rng = np.random.default_rng([tc.SEED, B, D])
    F = rng.uniform(20.0, 60.0, B) * amp_scale
    ang = rng.uniform(0.2, 1.3, B) + np.pi * rng.integers(0, 2, B)
    push = Push(F, np.stack([np.cos(ang), np.sin(ang)], 1), steps, duration=D, profile=w)
    amp = push.amplitudes(dt, MASS, B)
    rows = np.repeat(amp[:, None, :], D, axis=1)
    if w is not None:
        rows = rows * np.asarray(w)[None, :, None]
    return push, trace_of(rows, steps, push.axes)


@pytest.mark.parametrize("solver", (3, 4))
def test_constant_window_as_a_trace_is_the_window_bitwise_strict(solver):
    """hist and status of zmpc_rollout_pushed, bit for bit, on the LQ and the scan kernel; shaped
    windows (half-sine, ramp) to 1e-11: the kernels may fuse amp·w into the subtraction."""
    case = sc.rollout_case("jitter", 33, n=tc.N_WALK)
    B, n = len(case["kick"]), tc.N_WALK
    p = strict_plan(33, case["dt"], solver=solver)
    args = (case["zmax"], case["zmin"], case["x0"])
    h0, _ = p.rollout(*args)
    for D, steps in _window_runs(n, B):
        push, trace = _window_pair(B, D, steps, case["dt"], amp_scale=0.5)
        hw, sw = p.rollout(*args, push=push, mass=MASS)
        ht, st_ = p.rollout(*args, trace=trace)
        assert same_bits(ht, hw) and torch.equal(st_, sw), (D, steps)
        assert not torch.equal(ht, h0)
    for w in (ps.half_sine(7), pr.ramp(7)):
        push, trace = _window_pair(B, 7, 20, case["dt"], w=w, amp_scale=0.5)
        hw, sw = p.rollout(*args, push=push, mass=MASS)
        ht, st_ = p.rollout(*args, trace=trace)
        e = sc.rel_err(ht.cpu().numpy(), hw.cpu().numpy())
        print(f"MEASURED shaped window as a trace, solver {solver}: {e:.2e}")
        assert e <= PAIR and torch.equal(st_, sw)


def test_constant_window_as_a_trace_is_the_window_bitwise_herdt():
    """hist, foot and status of zmpc_herdt_rollout_pushed, bit for bit, on the batch of different
    walks; shaped windows to 1e-11."""
    batch = hc.rollout_batch()
    cfg = hc.make_config(batch["cfg_kw"])
    n, B = batch["n"], len(batch["x0"])
    prm, nb = herdt_inputs(cfg, batch["states"], n)
    plan = herdt_plan(cfg)
    args = (prm, batch["v"], batch["states"], nb, batch["x0"])
    for D, steps in _window_runs(n, B):
        push, trace = _window_pair(B, D, steps, cfg.dt, amp_scale=0.1 * cfg.m / MASS)
        ref = plan.herdt_rollout(*args, push=push, mass=MASS)
        got = plan.herdt_rollout(*args, trace=trace)
        assert same_bits(got[0], ref[0]) and same_bits(got[1], ref[1]), (D, steps)
        assert torch.equal(got[2], ref[2])
    for w in (ps.half_sine(5), pr.ramp(5)):
        push, trace = _window_pair(B, 5, n // 2, cfg.dt, w=w, amp_scale=0.1 * cfg.m / MASS)
        ref = plan.herdt_rollout(*args, push=push, mass=MASS)
        got = plan.herdt_rollout(*args, trace=trace)
        e = max(float((got[k] - ref[k]).abs().max()) for k in (0, 1))
        print(f"MEASURED shaped window as a trace, herdt: {e:.2e}")
        assert e <= PAIR and torch.equal(got[2], ref[2])


def test_constant_window_as_a_trace_unconstrained():
    """1e-11 against the window form (another order of the same sums)."""
    n, B = 179, 6
    d = golden("walk_n64.npz")
    p = unc_plan(PAR64)
    x0 = np.zeros((B, 2, 3))
    worst = 0.0
    for D, steps in _window_runs(n, B) + ((n + 5, 0),):
        for w in (None,) if D != 7 else (None, ps.half_sine(7), pr.ramp(7)):
            push, trace = _window_pair(B, D, steps, PAR64[1], w=w)
            hw, _ = p.rollout(d["zmax"], d["zmin"], x0, push=push, mass=MASS)
            ht, _ = p.rollout(d["zmax"], d["zmin"], x0, trace=trace)
            worst = max(worst, sc.rel_err(ht.cpu().numpy(), hw.cpu().numpy()))
    print(f"MEASURED window as a trace, unconstrained: {worst:.2e}")
    assert worst <= PAIR


# ------------------------------------------------------------- 2: per-walk traces, oracle loops

@functools.lru_cache(maxsize=None)
def strict_reference(family, N, kind):
    """The oracle loop's histories of the first walks of rollout_case(family, N) under their
    traces; not to be written into."""
    case = sc.rollout_case(family, N, n=tc.N_WALK)
    ref = np.stack([pr.strict_walk(case, b, sc.WEIGHTS[0],
                                   tc.table(tc.N_WALK, *tc.strict_trace(kind, b)))
                    for b in range(tc.STRICT_WALKS)])
    ref.setflags(write=False)
    return ref


def _strict_batch_trace(kind, B, n=tc.N_WALK):
    dvs = [tc.strict_trace(kind, b, n)[0] for b in range(B)]
    return trace_of(np.stack(dvs), 0)


@pytest.mark.parametrize("kind", ("dense", "sparse"))
@pytest.mark.parametrize("N", tc.STRICT_HORIZONS)
@pytest.mark.parametrize("family", tc.STRICT_FAMILIES)
def test_strict_traces_vs_oracle_loop(family, N, kind):
    """Solvers 0, 3 and 4: every status 0, the first 3 walks against the loop; LQ against scan on
    the whole batch."""
    case = sc.rollout_case(family, N, n=tc.N_WALK)
    B = len(case["kick"])
    trace = _strict_batch_trace(kind, B)
    ref = strict_reference(family, N, kind)
    out = {}
    for solver in (0, 3, 4):
        p = strict_plan(N, case["dt"], solver=solver)
        h, st = p.rollout(case["zmax"], case["zmin"], case["x0"], trace=trace)
        h, st = h.cpu().numpy(), st.cpu().numpy()
        assert not st.any(), (solver, st)
        assert_hist(h[:tc.STRICT_WALKS], st[:tc.STRICT_WALKS], ref,
                    f"{family} N={N} {kind} solver {solver}")
        out[solver] = h
    e = sc.rel_err(out[3], out[4])
    print(f"MEASURED {family} N={N} {kind}: LQ vs scan {e:.2e}")
    assert e <= PAIR


def test_strict_kick_order_on_and_off_agree_bitwise():
    """mixed_case(200) on the LQ kernel (three full waves and a partial one per axis), a dense
    trace and a start step per walk: the order changes the schedule alone."""
    case = sc.mixed_case(200)
    B, n = 200, case["zmax"].shape[1]
    dv = np.stack([tc.dense(n, b, tc.STRICT_DENSE * (1 + b % 5)) for b in range(B)])
    steps = np.array([(7 * b) % (n + 2) - 1 for b in range(B)], np.int64)
    trace = trace_of(dv, steps)
    outs = []
    for order in (1, 0):
        p = strict_plan(64, case["dt"], solver=3, kick_order=order)
        outs.append(p.rollout(case["zmax"], case["zmin"], case["x0"], trace=trace))
    assert same_bits(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    p = strict_plan(64, case["dt"], solver=4)
    h4, s4 = p.rollout(case["zmax"], case["zmin"], case["x0"], trace=trace)
    e = sc.rel_err(outs[0][0].cpu().numpy(), h4.cpu().numpy())
    print(f"MEASURED LQ vs scan, traced mixed B=200: {e:.2e}")
    assert e <= PAIR and torch.equal(outs[0][1], s4)


@pytest.mark.parametrize("kind", ("dense", "sparse"))
@pytest.mark.parametrize("name", tc.HERDT_WALKS)
def test_herdt_walks_vs_traced_loop(name, kind):
    case = pr.herdt_case(name)
    cfg = hc.make_config(case["cfg_kw"])
    n = case["n"]
    prm, nb = herdt_inputs(cfg, case["states"], n)
    dv, s = tc.herdt_trace(kind, n)
    dvel = tc.table(n, dv, s)
    com_o, y_o, foot_o, x_o = pr.herdt_rollout_pushed(cfg, case["x0"], case["v"], case["states"],
                                                      dvel)
    hist, foot, st = herdt_plan(cfg).herdt_rollout(prm, case["v"], case["states"], nb[0],
                                                   case["x0"][None], trace=trace_of(dv[None], s))
    hist, foot = hist[0].cpu().numpy(), foot[0].cpu().numpy()
    assert int(st[0]) == 0
    errs = (rmse(hist[:, :, 0], com_o), np.abs(foot - foot_o).max(),
            np.abs(hist[:, 1, :] - y_o).max(), np.abs(hist[:, 0, :] - x_o).max())
    print(f"MEASURED herdt {name} {kind}: CoM RMSE %.1e feet %.1e y %.1e x %.1e" % errs)
    assert errs[0] <= 1e-9 and errs[1] <= 1e-9 and errs[2] <= 1e-8 and errs[3] <= 1e-8


def test_herdt_batch_with_a_trace_and_a_start_step_per_walk():
    """rollout_batch(): 33 different walks in one launch, each under its own trace from its own
    start step (one outside the range, one truncated), against the traced loop of that walk."""
    batch = hc.rollout_batch()
    cfg = hc.make_config(batch["cfg_kw"])
    n, B = batch["n"], len(batch["x0"])
    prm, nb = herdt_inputs(cfg, batch["states"], n)
    dv, steps = tc.herdt_batch_traces(n, B)
    hist, foot, st = herdt_plan(cfg).herdt_rollout(prm, batch["v"], batch["states"], nb,
                                                   batch["x0"], trace=trace_of(dv, steps))
    hist, foot, st = hist.cpu().numpy(), foot.cpu().numpy(), st.cpu().numpy()
    errs = []
    for b in range(B):
        com_o, y_o, foot_o, x_o = pr.herdt_rollout_pushed(
            cfg, batch["x0"][b], batch["v"][b], batch["states"][b],
            tc.table(n, dv[b], int(steps[b])))
        errs.append((rmse(hist[b, :, :, 0], com_o), np.abs(foot[b] - foot_o).max(),
                     max(np.abs(hist[b, :, 1, :] - y_o).max(),
                         np.abs(hist[b, :, 0, :] - x_o).max())))
    errs = np.array(errs)
    print("MEASURED herdt traced batch: worst CoM RMSE %.1e feet %.1e history %.1e"
          % tuple(errs.max(axis=0)))
    assert np.all(st == 0), st
    assert errs[:, 0].max() <= 1e-9 and errs[:, 1].max() <= 1e-9 and errs[:, 2].max() <= 1e-8


# ------------------------------------------------------------- 3: unconstrained

@functools.lru_cache(maxsize=None)
def unpushed_oracle(n):
    zmax, zmin = walk_bounds(n)
    h = O.rollout_gain(zmax[None], zmin[None], np.zeros((1, 2, 3)), *PAR150)[0]
    h.setflags(write=False)
    return h


def _check_unconstrained(plan, par, zmax, zmin, h_oracle, dv, steps, axes, label):
    """One traced launch of B walks of the same bounds against the extended-precision reference;
    → the device history.  Rows up to the start step, walks without a disturbance and an axis not
    asked for hold the unpushed rollout's bits; a second launch repeats the first."""
    B, n = dv.shape[0], len(zmax)
    x0 = np.zeros((B, 2, 3))
    trace = trace_of(dv, steps, axes)
    h0, s0 = plan.rollout(zmax, zmin, x0)
    h, st = plan.rollout(zmax, zmin, x0, trace=trace)
    h2, _ = plan.rollout(zmax, zmin, x0, trace=trace)
    assert torch.equal(st, s0) and same_bits(h, h2)
    h, h0 = h.cpu().numpy(), h0.cpu().numpy()
    ref = tc.traced_reference(np.broadcast_to(h_oracle, (B, n, 2, 3)), dv, steps,
                              tc.closed_loop(par), axes).astype(np.float64)
    r, e = rmse(h[..., 0], ref[..., 0]), float(np.abs(h - ref).max())
    assert r <= 1e-9 and e <= 1e-7, (label, r, e)
    for b, s in enumerate(steps):
        upto = n if not 0 <= s < n - 1 else s + 1
        assert same_bits(h[b, :upto], h0[b, :upto]), (label, b)
    for a, name in enumerate("xy"):
        if name not in axes:
            assert same_bits(h[:, :, a], h0[:, :, a]), label
    return h, r, e


@pytest.mark.parametrize("n", tc.EMU_N)
def test_unconstrained_grid_vs_extended_precision(n):
    """The emulation's grid: every start step of emu_steps(n) with every length of
    emu_lengths(n), one axis and two."""
    plan = unc_plan(PAR150)
    zmax, zmin = walk_bounds(n)
    steps = tc.emu_steps(n)
    worst = (0.0, 0.0)
    for axes in ("x", "y", "xy"):
        for L in tc.emu_lengths(n):
            _, r, e = _check_unconstrained(plan, PAR150, zmax, zmin, unpushed_oracle(n),
                                           tc.grid_dv(n, L, axes), steps, axes, (n, L, axes))
            worst = (max(worst[0], r), max(worst[1], e))
    print(f"MEASURED unconstrained grid n={n}: CoM RMSE {worst[0]:.2e} state {worst[1]:.2e}")


@pytest.mark.parametrize("walk", ("walk_n64", "walk_n150", "long700"))
def test_unconstrained_walks_dense_sparse_and_batch_independence(walk):
    """n = 179 and 420 (the split kernels) and a walk of 700 samples (the long-walk route) under
    the dense and the sparse trace; the walk alone (B = 1) and inside B = 200 give the same bits;
    a zero trace gives the unpushed bits."""
    if walk == "long700":
        par, (zmax, zmin) = PAR150, walk_bounds(700)
    else:
        d = golden(walk + ".npz")
        par, zmax, zmin = (PAR64 if walk == "walk_n64" else PAR150), d["zmax"], d["zmin"]
    n = len(zmax)
    plan = unc_plan(par)
    h_oracle = O.rollout_gain(zmax[None], zmin[None], np.zeros((1, 2, 3)), *par)[0]
    dense = np.stack([tc.dense(n, b, tc.STRICT_DENSE) for b in range(3)])
    h, r, e = _check_unconstrained(plan, par, zmax, zmin, h_oracle, dense,
                                   np.array([0, 5, n // 2]), "xy", (walk, "dense"))
    print(f"MEASURED unconstrained {walk} dense: CoM RMSE {r:.2e} state {e:.2e}")
    sparse = np.stack([tc.strict_sparse(n), tc.herdt_sparse(n)])
    _, r, e = _check_unconstrained(plan, par, zmax, zmin, h_oracle, sparse, np.array([0, 0]),
                                   "xy", (walk, "sparse"))
    print(f"MEASURED unconstrained {walk} sparse: CoM RMSE {r:.2e} state {e:.2e}")
    # the second dense walk alone, and at place 137 of a batch of 200 other walks
    B = 200
    big = np.stack([tc.dense(n, 1000 + b, tc.STRICT_DENSE) for b in range(B)])
    steps = np.arange(B, dtype=np.int64) % (n - 1)
    big[137], steps[137] = dense[1], 5
    hb, _ = plan.rollout(zmax, zmin, np.zeros((B, 2, 3)), trace=trace_of(big, steps))
    h1, _ = plan.rollout(zmax, zmin, np.zeros((1, 2, 3)), trace=trace_of(dense[1:2], 5))
    assert same_bits(hb[137], h1[0]) and same_bits(h1[0], h[1])
    h0, _ = plan.rollout(zmax, zmin, np.zeros((3, 2, 3)))
    hz, _ = plan.rollout(zmax, zmin, np.zeros((3, 2, 3)), trace=trace_of(np.zeros_like(dense), 0))
    assert same_bits(hz, h0)


def test_device_velocity_steps_feed_a_launch_without_a_copy():
    """PushTrace.from_velocity_steps of a device tensor: the launcher's dv buffer is that tensor,
    and new values written into it reach the next launch."""
    d = golden("walk_n64.npz")
    plan = unc_plan(PAR64)
    n, B, L = len(d["zmax"]), 4, 30
    gen = torch.Generator(device="cuda").manual_seed(tc.SEED)
    dv = 0.02 * torch.randn((B, L, 2), dtype=torch.float64, device="cuda", generator=gen)
    launch = plan.rollout_launcher(d["zmax"], d["zmin"], np.zeros((B, 2, 3)),
                                   trace=PushTrace.from_velocity_steps(dv, 10, "xy"))
    assert launch.trace_dv.data_ptr() == dv.data_ptr() and launch.push_amp is None
    launch()
    a = launch.hist.clone()
    ref, _ = plan.rollout(d["zmax"], d["zmin"], np.zeros((B, 2, 3)),
                          trace=trace_of(dv.cpu().numpy(), 10))
    assert same_bits(a, ref)
    dv.mul_(2.0)
    launch()
    ref2, _ = plan.rollout(d["zmax"], d["zmin"], np.zeros((B, 2, 3)),
                           trace=trace_of(dv.cpu().numpy(), 10))
    assert same_bits(launch.hist, ref2) and not torch.equal(launch.hist, a)


# ------------------------------------------------------------- 4: bisection

def test_critical_force_of_a_trace_unconstrained():
    """walk_n64 under the sparse pattern: the final bracket holds λ* = min_i margin_i/|Δz_i(λ = 1)|
    computed on the host from the linear response, and traced rollouts at λ*(1 ∓ 1e-6) pass and
    fail."""
    d = golden("walk_n64.npz")
    zmax, zmin = d["zmax"], d["zmin"]
    n = len(zmax)
    c = ZMPController(MPCConfig(horizon=64, strict=False))
    dv = tc.strict_sparse(n)[None]
    trace = trace_of(dv, 0)
    t = 1e-9
    lo, hi = c.critical_force(zmax, zmin, trace=trace, max_violation=t)
    lo, hi = float(lo[0]), float(hi[0])
    plan = c._plan()
    h0 = plan.rollout(zmax, zmin, np.zeros((1, 2, 3)))[0][0].cpu().numpy()
    cfg = c.config
    consts = tc.closed_loop((64, cfg.dt, cfg.h, cfg.g, cfg.Q, cfg.R))
    delta = tc.response(n, dv[0], 0, consts)                     # hist −= λ·δ
    C = np.array([1.0, 0.0, -cfg.h / cfg.g], np.longdouble)
    z0 = np.asarray(h0, np.longdouble) @ C                       # [n, 2]
    dz = -(delta @ C)                                            # Δz at λ = 1
    with np.errstate(divide="ignore", invalid="ignore"):
        cand = np.where(dz > 0, (zmax - z0 + t) / dz, np.where(dz < 0, (z0 - zmin + t) / -dz,
                                                                np.inf))
    lam = float(cand.min())
    print(f"MEASURED critical trace scale: bracket [{lo:.9g}, {hi:.9g}], λ* {lam:.9g}")
    assert 0.0 < lo <= lam <= hi and hi - lo <= 1000.0 / 2 ** 30 * 1.0001

    def passes(k):
        hist, _ = plan.rollout(zmax, zmin, np.zeros((1, 2, 3)), trace=trace.scaled(k))
        return bool((c.walk_metrics(hist, zmax, zmin).viol_max <= t).all())

    assert passes(lam * (1 - 1e-6)) and not passes(lam * (1 + 1e-6))
    with pytest.raises(ValueError):
        c.critical_force(zmax, zmin, trace=trace, fused=True)


def test_critical_force_of_a_trace_strict():
    """On the strict plan the CoM criterion decides (the clamped ZMP hides the disturbance):
    rollouts at the returned F_lo pass and at F_hi fail."""
    d = golden("walk_n64.npz")
    zmax, zmin = d["zmax"], d["zmin"]
    n = len(zmax)
    s = ZMPController(MPCConfig(horizon=64, strict=True))
    plan = s._plan()
    x0 = np.zeros((1, 2, 3))
    h0, _ = plan.rollout(zmax, zmin, x0)
    dev_max = float(plan.walk_metrics(h0, zmax, zmin)[0, 6:8].max()) + 0.05
    trace = trace_of(tc.strict_sparse(n)[None], 0)
    lo, hi = s.critical_force(zmax, zmin, trace=trace, max_com_dev=dev_max, iters=20)
    lo, hi = float(lo[0]), float(hi[0])
    print(f"MEASURED strict critical trace scale: bracket [{lo:.9g}, {hi:.9g}]")
    assert 0.0 < lo < hi < 1000.0

    def alone(k):
        hist, st = plan.rollout(zmax, zmin, x0, trace=trace.scaled(k))
        m = s.walk_metrics(hist, zmax, zmin)
        return hist, bool((m.viol_max <= 1e-9).all() and (m.com_dev_max <= dev_max).all()
                          and int(st[0]) == 0)

    assert alone(lo)[1] and not alone(hi)[1]
    # the controller's batch methods are that rollout
    hist, st = s.generate_state_trajectory_batch(None, zmax, zmin, trace=trace.scaled(lo))
    assert torch.equal(hist, alone(lo)[0]) and int(st[0]) == 0
    com, hist2 = s.generate_com_trajectory_batch(None, zmax, zmin, trace=trace.scaled(lo))
    assert torch.equal(hist2, hist) and torch.equal(com, hist[..., 0])


def test_critical_force_herdt_of_a_trace():
    """n17_triangle: the half-sine shove of D = 5 at step 25 along two directions, spelled as the
    trace of one newton.  The scale's bracket is then the force's: it agrees with the shove form's
    bracket to one bracket width, and traced rollouts at F_lo pass and at F_hi fail."""
    import herdt_metrics_cases as mc
    case = pr.herdt_case(mc.SHOVE_WALK)
    cfg = hc.make_config(case["cfg_kw"])
    ctl = ZMPController(cfg)
    dirs = np.array([d for d, _ in mc.SHOVES[:2]], np.float64)
    w = ps.half_sine(mc.SHOVE_D)
    unit = Push(np.ones(2), dirs, mc.SHOVE_STEP, duration=mc.SHOVE_D, profile=w)
    n = case["n"]
    dvel = unit.velocity_steps(cfg.dt, cfg.m, 2, n)
    rows = np.ascontiguousarray(dvel[:, mc.SHOVE_STEP:mc.SHOVE_STEP + mc.SHOVE_D])
    trace = trace_of(rows, mc.SHOVE_STEP)
    iters = 24
    lo, hi = ctl.critical_force_herdt(case["v"], case["states"], mc.MAX_DCM_DEV, trace=trace,
                                      iters=iters)
    plo, phi = ctl.critical_force_herdt(case["v"], case["states"], mc.MAX_DCM_DEV, direction=dirs,
                                        force_step=mc.SHOVE_STEP, duration=mc.SHOVE_D, profile=w,
                                        iters=iters)
    lo, hi, plo = lo.cpu().numpy(), hi.cpu().numpy(), plo.cpu().numpy()
    width = 1000.0 / 2 ** iters
    print("MEASURED critical_force_herdt(trace=):", lo.tolist(), "shove form", plo.tolist())
    assert np.array_equal(hi - lo, np.full(2, width)) and (lo > 0).all()
    assert (np.abs(lo - plo) <= width).all()

    def passes(k):
        _, hist, foot, st = ctl.generate_com_trajectory_herdt_batch(
            None, case["v"], case["states"], trace=trace_of(rows * k[:, None, None],
                                                            mc.SHOVE_STEP), return_status=True)
        m = ctl.herdt_walk_metrics(hist, foot, case["states"])
        ok = (m.dcm_dev_max <= mc.MAX_DCM_DEV).all(dim=1) & (m.viol_max <= 1e-9).all(dim=1)
        return (ok & (st == 0)).cpu().numpy()

    assert passes(lo).all() and not passes(hi).any()


# ------------------------------------------------------------- 5: refusals

@pytest.mark.parametrize("solver", (1, 2))
def test_reduced_cholesky_solvers_refuse_a_trace(solver):
    """ZMPC_ESTATE with the reason, and the output buffers keep their prefill."""
    case = sc.rollout_case("jitter", 33)
    p = strict_plan(33, case["dt"], solver=solver)
    B, n = len(case["kick"]), case["zmax"].shape[1]
    zx, zn, x0 = dev(case["zmax"]), dev(case["zmin"]), dev(case["x0"])
    dv = dev(np.stack([tc.dense(n, b, tc.STRICT_DENSE) for b in range(B)]))
    hist = torch.full((B, n, 2, 3), -7.0, dtype=torch.float64, device="cuda")
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    c = _native.ZmpcTrace(dv.data_ptr(), AXES["xy"], None, 0, n - 1,
                          torch.cuda.current_stream().cuda_stream)
    rc = _native.load().zmpc_rollout_traced(p.handle, B, n, vp(zx), vp(zn), 2 * n, vp(x0),
                                            ctypes.addressof(c), vp(hist), vp(status))
    torch.cuda.synchronize()
    assert rc == _native.ZMPC_ESTATE
    assert b"reduced-Cholesky" in _native.load().zmpc_last_error()
    assert bool((hist == -7.0).all()) and bool((status == -7).all())
    p.set_option("strict_solver", 0)


# ------------------------------------------------------------- 6: the stream contract

def _busy(stream_tensor):
    """Work that keeps the current stream occupied for a while before what follows on it."""
    for _ in range(8):
        stream_tensor = stream_tensor @ stream_tensor
        stream_tensor = stream_tensor / stream_tensor.abs().max()
    return stream_tensor


def _stream_cases():
    """(label, run(dv_host, steps) → tuple of output tensors) for both new calls, each reading dv
    from a tensor a torch operation writes on the current stream immediately before the call."""
    case = sc.rollout_case("jitter", 33, n=tc.N_WALK)
    sp = strict_plan(33, case["dt"], solver=0)
    d = golden("walk_n64.npz")
    up = unc_plan(PAR64)
    batch = hc.rollout_batch()
    cfg = hc.make_config(batch["cfg_kw"])
    prm, nb = herdt_inputs(cfg, batch["states"], batch["n"])
    hp = herdt_plan(cfg)

    def written(dv_host):
        src = dev(dv_host)
        torch.cuda.current_stream().wait_stream(torch.cuda.default_stream())
        _busy(torch.rand((1024, 1024), dtype=torch.float32, device="cuda"))
        return src * 1.0  # a kernel on the current stream: the call must come after it

    def strict(dv_host, steps):
        t = PushTrace.from_velocity_steps(written(dv_host), steps, "xy")
        B = len(dv_host)
        return sp.rollout(case["zmax"][:B], case["zmin"][:B], case["x0"][:B], trace=t)

    def unc(dv_host, steps):
        t = PushTrace.from_velocity_steps(written(dv_host), steps, "xy")
        return up.rollout(d["zmax"], d["zmin"], np.zeros((len(dv_host), 2, 3)), trace=t)

    def herdt(dv_host, steps):
        B = len(dv_host)
        t = PushTrace.from_velocity_steps(written(dv_host), steps, "xy")
        return hp.herdt_rollout(prm, batch["v"][:B], batch["states"][:B], nb[:B],
                                batch["x0"][:B], trace=t)

    return (("strict", strict, tc.N_WALK, tc.STRICT_DENSE),
            ("unconstrained", unc, len(d["zmax"]), tc.STRICT_DENSE),
            ("herdt", herdt, batch["n"], tc.HERDT_DENSE))


def test_stream_contract_of_both_new_calls():
    """On a non-null stream, with dv written by a torch operation on that stream immediately
    before the call, the results equal the null-stream results bit for bit; two streams with
    different batches do not mix."""
    for label, run, n, scale in _stream_cases():
        dva = np.stack([tc.dense(n, b, scale) for b in range(6)])
        dvb = np.stack([tc.dense(n, 50 + b, scale) for b in range(4)])
        sa, sb = np.arange(6) % 3, np.arange(4) + 1
        ref_a, ref_b = run(dva, sa), run(dvb, sb)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            got_a = run(dva, sa)
        with torch.cuda.stream(s2):
            got_b = run(dvb, sb)
        s1.synchronize()
        s2.synchronize()
        for g, r in zip(got_a + got_b, ref_a + ref_b):
            assert torch.equal(g, r), label
        assert not torch.equal(got_a[0][:4], got_b[0])
