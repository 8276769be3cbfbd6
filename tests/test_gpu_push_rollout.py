"""Device tests of pushed rollouts (zmpc_rollout_pushed, zmpc_herdt_rollout_pushed): pushes of any
length, shape and direction on the strict kernels (csrc/strict_lq.hip, strict_scan.hip), the
Herdt kernel (csrc/herdt.hip) and, by the linear state response, on unconstrained plans
(csrc/pushmap.hip).

The references are the oracle loops of tests/push_rollout_cases.py (tests/test_push_rollout_host.py
holds them to the oracles they restate and proves every case used here on the CPU) and, for the
unconstrained controller, chained oracle rollouts.  Bars, the project's existing ones: strict
rollouts CoM RMSE <= 1e-9 and every state within 1e-9 x max(1, largest |reference state|), every
status asserted; Herdt CoM RMSE and feet 1e-9, histories 1e-8; unconstrained CoM RMSE 1e-9, state
1e-7; forms that compute the same solution agree to 1e-11 (include/zmpc.h)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import herdt_cases as hc
import push_rollout_cases as pr
import push_shaped_cases as ps
import strict_cases as sc
from conftest import golden, rmse

pytestmark = pytest.mark.gpu

from mpc_bipedal import _native  # noqa: E402
from mpc_bipedal.analysis import AXES, Push  # noqa: E402
from mpc_bipedal.config import MPCConfig  # noqa: E402
from mpc_bipedal.controllers import ZMPController  # noqa: E402
from mpc_bipedal.controllers import herdt as H  # noqa: E402
from mpc_bipedal.solver import Plan  # noqa: E402

BAR = 1e-9
PAIR = 1e-11
PAR150 = (150, 0.01, 0.75, 9.81, 1.0, 1e-6)  # the default walk's plan (walk_n150.npz)
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


def strict_plan(N, dt, weights=sc.WEIGHTS[0], solver=0, kick_order=1):
    key = (N, dt, weights)
    if key not in _PLANS:
        Q, R, h = weights
        _PLANS[key] = Plan(torch.cuda.current_device(), N, dt, h, sc.G, Q, R, True)
    p = _PLANS[key]
    p.set_option("strict_solver", solver)
    p.set_option("kick_order", kick_order)
    return p


def dev(a, dtype=torch.float64):
    return torch.as_tensor(a, dtype=dtype, device="cuda").contiguous()


def vp(x):
    return None if x is None else ctypes.c_void_p(x.data_ptr())


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def pushed(plan, zmax, zmin, x0, amp, axes, steps=None, step=-1, w=None, D=1, expect=0):
    """One zmpc_rollout_pushed call straight through ctypes, into prefilled buffers → (hist,
    status) on the host.  amp [B, C]; steps [B] or None (then `step`)."""
    B, n = x0.shape[0], zmax.shape[-2]
    zx, zn, x, a = dev(zmax), dev(zmin), dev(x0), dev(amp)
    assert a.shape == (B, 2 if axes == "xy" else 1)
    st_t = None if steps is None else dev(steps, torch.int64)
    w_t = None if w is None else dev(w)
    hist = torch.full((B, n, 2, 3), -7.0, dtype=torch.float64, device="cuda")
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    c = _native.ZmpcPush(a.data_ptr(), AXES[axes], None if st_t is None else st_t.data_ptr(),
                         int(step), None if w_t is None else w_t.data_ptr(), int(D))
    rc = _native.load().zmpc_rollout_pushed(
        plan.handle, B, n, vp(zx), vp(zn), 0 if np.ndim(zmax) == 2 else 2 * n, vp(x),
        ctypes.addressof(c), vp(hist), vp(status),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == expect, (rc, _native.load().zmpc_last_error())
    return hist.cpu().numpy(), status.cpu().numpy()


def assert_hist(h, st, ref, label):
    assert not st.any(), (label, st)
    r, e = rmse(h[..., 0], ref[..., 0]), sc.rel_err(h, ref)
    print(f"MEASURED {label}: CoM RMSE {r:.2e} state {e:.2e}")
    assert r <= BAR and e <= BAR, (label, r, e)


# ----------------------------------------------------------------------------- 1: legacy, bitwise

@pytest.mark.parametrize("kind", ("solver3", "solver4", "unconstrained"))
def test_legacy_push_is_rollout_kicks_bitwise(kind):
    """axes = y, D = 1, no profile: hist and status of zmpc_rollout_kicks (per-walk steps) and of
    zmpc_rollout (one step), bit for bit."""
    case = sc.mixed_case(70)
    if kind == "unconstrained":
        Q, R, h = sc.WEIGHTS[0]
        p = Plan(torch.cuda.current_device(), case["N"], case["dt"], h, sc.G, Q, R, False)
    else:
        p = strict_plan(case["N"], case["dt"], solver=int(kind[-1]))
    for ks in (case["kick_step"], 17):
        h0, s0 = p.rollout(case["zmax"], case["zmin"], case["x0"], kick=case["kick"], kick_step=ks)
        per_walk = np.ndim(ks) == 1
        h, s = pushed(p, case["zmax"], case["zmin"], case["x0"], case["kick"][:, None], "y",
                      steps=ks if per_walk else None, step=-1 if per_walk else ks)
        assert same_bits(h, h0.cpu().numpy()) and np.array_equal(s, s0.cpu().numpy())
    if kind == "unconstrained":
        p.destroy()


def _herdt_inputs(cfg, states, n):
    N = cfg.horizon
    st2 = np.atleast_2d(states)
    pad = np.concatenate([st2, np.repeat(st2[:, -1:], N, axis=1)], axis=1)
    nb = np.array([[t[0] for t in H.find_nb_steps(p)][:n] for p in pad], np.int32)
    return H.make_params(cfg, H.max_footsteps(pad, N, n)), nb


def _herdt_plan(cfg):
    key = ("herdt", cfg.horizon, cfg.dt)
    if key not in _PLANS:
        _PLANS[key] = Plan(torch.cuda.current_device(), cfg.horizon, cfg.dt, cfg.h, cfg.g, 1.0,
                           1e-6, False)
    return _PLANS[key]


def test_legacy_push_is_herdt_rollout_bitwise():
    """The same for zmpc_herdt_rollout (hist, foot, status), on a single walk and on the batch of
    different walks; Push(F, +1, step) is the kick dt·F/m."""
    case = pr.herdt_case("n40_ssp9_kickmid")
    batch = hc.rollout_batch()
    for cfg_kw, v, states, x0, kick, ks in (
            (case["cfg_kw"], case["v"], case["states"], case["x0"][None],
             np.array([hc.case_kick(case)]), case["kick_step"]),
            (batch["cfg_kw"], batch["v"], batch["states"], batch["x0"], batch["kick"],
             batch["kick_step"])):
        cfg = hc.make_config(cfg_kw)
        n = v.shape[-2]
        prm, nb = _herdt_inputs(cfg, states, n)
        nb = nb[0] if np.ndim(states) == 1 else nb
        plan = _herdt_plan(cfg)
        push = Push(kick * cfg.m / cfg.dt, +1, ks)
        amp = push.amplitudes(cfg.dt, cfg.m, len(kick))[:, 0]  # (the kick, to an ulp)
        assert np.allclose(amp, kick, rtol=1e-15, atol=0.0)
        ref = plan.herdt_rollout(prm, v, states, nb, x0, kick=amp, kick_step=ks)
        got = plan.herdt_rollout(prm, v, states, nb, x0, push=push, mass=cfg.m)
        for a, b in zip(got, ref):
            assert torch.equal(a, b)


# ----------------------------------------------------------------------------- 2: axis symmetry

def _mixed_push(case, D=7):
    """A half-sine push per walk of a strict case: the walk's own kick step, amplitudes from its
    kick (x: reversed)."""
    w = ps.half_sine(D)
    amp = np.stack([-case["kick"], case["kick"]], axis=1) / w.sum()
    return w, amp, case["kick_step"]


@pytest.mark.parametrize("solver", (3, 4))
def test_axis_symmetry_bitwise(solver):
    """An x push on axis-swapped bounds and x0 gives the y push's history with the axes swapped,
    and an xy launch equals the x rows of the x launch and the y rows of the y launch."""
    case = sc.mixed_case(70)
    p = strict_plan(64, case["dt"], solver=solver)
    D = 7
    w, amp, steps = _mixed_push(case, D)
    zx, zn, x0 = case["zmax"], case["zmin"], case["x0"]
    hy, sy = pushed(p, zx, zn, x0, amp[:, 1:], "y", steps=steps, w=w, D=D)
    hx, sx = pushed(p, zx, zn, x0, amp[:, :1], "x", steps=steps, w=w, D=D)
    hxy, sxy = pushed(p, zx, zn, x0, amp, "xy", steps=steps, w=w, D=D)
    assert not sy.any() and not sx.any() and not sxy.any()
    assert same_bits(hxy[:, :, 0], hx[:, :, 0]) and same_bits(hxy[:, :, 1], hy[:, :, 1])
    assert not np.array_equal(hy[:, :, 1], hx[:, :, 1])  # (the push does something)
    hs, ss = pushed(p, np.ascontiguousarray(zx[..., ::-1]), np.ascontiguousarray(zn[..., ::-1]),
                    np.ascontiguousarray(x0[:, ::-1]), amp[:, 1:], "x", steps=steps, w=w, D=D)
    assert not ss.any() and same_bits(np.ascontiguousarray(hs[:, :, ::-1]), hy)
    # an axis that was not asked for is the unpushed walk's, bit for bit
    h0, _ = p.rollout(zx, zn, x0)
    assert same_bits(hy[:, :, 0], np.ascontiguousarray(h0.cpu().numpy()[:, :, 0]))


# ----------------------------------------------------------------------------- 3: the oracle loop

def _family_steps(n, s, pi, B):
    """Per-walk start steps round s: one walk two steps later, one outside the range."""
    steps = np.full(B, s, np.int64)
    steps[3] = min(s + 2, n - 2)
    steps[B - 1] = (-1, n - 1, n + 7)[pi]
    return steps


@functools.lru_cache(maxsize=None)
def family_reference(family, N, wi, pi):
    """The oracle loop's histories of rollout_case(family, N) under push pi; not to be written
    into."""
    case = sc.rollout_case(family, N, n=pr.N_WALK)
    D, s, w, amp, _ = pr.strict_pushes()[pi]
    steps = _family_steps(pr.N_WALK, s, pi, len(case["kick"]))
    ref = np.stack([pr.strict_walk(case, b, sc.WEIGHTS[wi],
                                   pr.window(pr.N_WALK, int(steps[b]), D, w, amp))
                    for b in range(len(case["kick"]))])
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("N", pr.STRICT_HORIZONS)
@pytest.mark.parametrize("family", sc.FAMILIES)
def test_families_vs_oracle_loop(family, N):
    """Solvers 3 and 4 at the four weight points under the three half-sine pushes on both axes
    (0.3 m/s on x, −0.2 m/s on y in all), per-walk start steps."""
    case = sc.rollout_case(family, N, n=pr.N_WALK)
    B = len(case["kick"])
    for wi, weights in enumerate(sc.WEIGHTS):
        for pi, (D, s, w, amp, _) in enumerate(pr.strict_pushes()):
            ref = family_reference(family, N, wi, pi)
            steps = _family_steps(pr.N_WALK, s, pi, B)
            for solver in (3, 4):
                p = strict_plan(N, case["dt"], weights, solver)
                h, st = pushed(p, case["zmax"], case["zmin"], case["x0"], np.tile(amp, (B, 1)),
                               "xy", steps=steps, w=w, D=D)
                assert_hist(h, st, ref, f"{family} N={N} w{wi} push {pi} solver {solver}")


# ----------------------------------------------------------------------------- 4: kernel shapes

def test_lq_kernel_waves_and_kick_order():
    """mixed_case(200) on the LQ kernel, three full waves and a partial one per axis: kick order
    on and off agree bit for bit; against the scan kernel on the same pushed batch <= 1e-11."""
    case = sc.mixed_case(200)
    w, amp, steps = _mixed_push(case)
    outs = []
    for order in (1, 0):
        p = strict_plan(64, case["dt"], solver=3, kick_order=order)
        outs.append(pushed(p, case["zmax"], case["zmin"], case["x0"], amp, "xy", steps=steps, w=w,
                           D=7))
    assert not outs[0][1].any()
    assert same_bits(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    p = strict_plan(64, case["dt"], solver=4)
    h4, s4 = pushed(p, case["zmax"], case["zmin"], case["x0"], amp, "xy", steps=steps, w=w, D=7)
    e = sc.rel_err(outs[0][0], h4)
    print(f"MEASURED LQ vs scan, pushed mixed B=200: {e:.2e}")
    assert not s4.any() and e <= PAIR
    # one walk of each kind against the oracle loop
    ref = np.stack([pr.strict_walk(case, b, sc.WEIGHTS[0],
                                   pr.window(40, int(steps[b]), 7, w, amp[b])) for b in range(7)])
    assert_hist(outs[0][0][:7], outs[0][1][:7], ref, "mixed B=200 solver 3, oracle loop")


def test_scan_kernel_32_lane_instances():
    """mixed_case(1200) on the scan kernel (two 32-lane instances per wave): its first 200 walks
    agree with the B = 200 launch's to the pair bar 1e-11 (the launches may take instances of
    different lane widths), no walk is flagged, and the last seven walks meet the oracle loop."""
    case = sc.mixed_case(1200)
    w, amp, steps = _mixed_push(case)
    p = strict_plan(64, case["dt"], solver=4)
    h, st = pushed(p, case["zmax"], case["zmin"], case["x0"], amp, "xy", steps=steps, w=w, D=7)
    assert not st.any() and np.isfinite(h).all()
    small = sc.mixed_case(200)
    h2, _ = pushed(p, small["zmax"], small["zmin"], small["x0"], amp[:200], "xy",
                   steps=steps[:200], w=w, D=7)
    e = sc.rel_err(h[:200], h2)
    print(f"MEASURED scan kernel, B = 1200 vs B = 200 (its first walks alone): {e:.2e}")
    assert e <= PAIR
    ref = np.stack([pr.strict_walk(case, b, sc.WEIGHTS[0],
                                   pr.window(40, int(steps[b]), 7, w, amp[b]))
                    for b in range(1193, 1200)])
    assert_hist(h[1193:], st[1193:], ref, "mixed B=1200 solver 4, oracle loop")


def test_long_horizon_lq_shape():
    """lq_rollout_case(321), six samples, a D = 3 push at step 0 on both axes, against the oracle
    loop."""
    case = sc.lq_rollout_case(321)
    w = ps.half_sine(3)
    amp = pr.push_amp(3, w) * 0.1  # (walks that start within ±5 cm: a tenth of the impulse)
    p = strict_plan(321, case["dt"], solver=3)
    h, st = pushed(p, case["zmax"], case["zmin"], case["x0"], np.tile(amp, (3, 1)), "xy", step=0,
                   w=w, D=3)
    ref = np.stack([pr.strict_walk(case, b, sc.WEIGHTS[0], pr.window(6, 0, 3, w, amp))
                    for b in range(3)])
    assert_hist(h, st, ref, "lq_rollout_case(321) D=3")


@pytest.mark.parametrize("N", (897, 2177))
def test_lq_push_instances_of_short_workgroups(N):
    """The LQ kernel's push instances of 4 and 2 waves per workgroup (N = 897, 2177; csrc/dispatch.h
    lq_shape), in both bound forms: lq_rollout_case(N) with its kick given as a D = 1 push on y
    with the profile [1.0] (a profile, so not the legacy kick: the push instance runs).  That is
    the kick itself (include/zmpc.h, "The push, stated once"; amp·1.0 is exact), so the reference
    is the C restatement of the kicked rollout, as test_gpu_strict_cases.py test_lq_shapes."""
    case = sc.lq_rollout_case(N)
    ref, cst, _ = sc.restatement(case, threads=min(16, os.cpu_count() or 1))
    assert not cst.any()
    p = strict_plan(N, case["dt"], solver=3)
    outs = []
    try:
        for bounds in (1, 2):
            p.set_option("strict_bounds", bounds)
            h, st = pushed(p, case["zmax"], case["zmin"], case["x0"], case["kick"][:, None], "y",
                           steps=case["kick_step"], w=np.ones(1), D=1)
            assert_hist(h, st, ref, f"lq push instance N={N} bounds {bounds}")
            outs.append(h)
    finally:
        p.set_option("strict_bounds", 0)
    print(f"MEASURED lq push instance N={N}: bound forms bitwise equal {same_bits(*outs)}")


def test_asymmetric_profile_strict():
    """A rising profile (w_j != w_(D−1−j)) at (7, 20) and truncated at (7, n − 4): a kernel that
    read the profile backwards would miss the oracle loop.  Solvers 3 and 4, the four weights."""
    family, N = pr.RAMP_CASE
    case = sc.rollout_case(family, N, n=pr.N_WALK)
    B = len(case["kick"])
    for wi, weights in enumerate(sc.WEIGHTS):
        for pi, (D, s, w, amp, _) in enumerate(pr.ramp_pushes()):
            steps = _family_steps(pr.N_WALK, s, pi, B)
            ref = np.stack([pr.strict_walk(case, b, weights,
                                           pr.window(pr.N_WALK, int(steps[b]), D, w, amp))
                            for b in range(B)])
            back = pr.strict_walk(case, 0, weights,
                                  pr.window(pr.N_WALK, int(steps[0]), D, w[::-1].copy(), amp))
            assert sc.rel_err(back, ref[0]) > 1e-6  # (the reversed profile is another walk)
            for solver in (3, 4):
                p = strict_plan(N, case["dt"], weights, solver)
                h, st = pushed(p, case["zmax"], case["zmin"], case["x0"], np.tile(amp, (B, 1)),
                               "xy", steps=steps, w=w, D=D)
                assert_hist(h, st, ref, f"ramp {family} N={N} w{wi} push {pi} solver {solver}")


def test_lq_task_queue_instance():
    """More blocks than the chip holds at once: the LQ kernel's push instance with the task queue
    (one 8-wave block per compute unit is resident at 253+ VGPRs, so 72 000 walks = 282 blocks
    pass the 256 compute units).  The 200 mixed walks tiled 360 times under a rising D = 7 push
    on xy, each copy's amplitudes scaled differently; against the scan kernel on the same batch
    at the pair bar, and every copy of scale 1 against the B = 200 launch bit for bit."""
    base = sc.mixed_case(200)
    reps = 360
    w = pr.ramp(7)
    amp1 = np.stack([-base["kick"], base["kick"]], axis=1) / w.sum()
    scale = 1.0 - 0.002 * (np.arange(reps) % 5)
    amp = (amp1[None] * scale[:, None, None]).reshape(-1, 2)
    tile = lambda a: np.tile(a, (reps,) + (1,) * (a.ndim - 1))  # noqa: E731
    zx, zn, x0, steps = (tile(base[k]) for k in ("zmax", "zmin", "x0", "kick_step"))
    p = strict_plan(64, base["dt"], solver=3)
    h, st = pushed(p, zx, zn, x0, amp, "xy", steps=steps, w=w, D=7)
    assert not st.any()
    h200, _ = pushed(p, base["zmax"], base["zmin"], base["x0"], amp1, "xy",
                     steps=base["kick_step"], w=w, D=7)
    for r in np.nonzero(scale == 1.0)[0]:
        assert same_bits(h[200 * r:200 * (r + 1)], h200), r
    assert not np.array_equal(h[200:400], h200)
    p = strict_plan(64, base["dt"], solver=4)
    h4, s4 = pushed(p, zx, zn, x0, amp, "xy", steps=steps, w=w, D=7)
    e = sc.rel_err(h, h4)
    print(f"MEASURED LQ (task queue) vs scan, 72 000 pushed walks: {e:.2e}")
    assert not s4.any() and e <= PAIR


# ----------------------------------------------------------------------------- 5: Herdt

def _herdt_push(cfg, B, steps, amp=pr.HERDT_AMP, profile=ps.half_sine):
    """The D = 5 xy push (half-sine, or ramp) with velocity amplitudes `amp` per unit weight."""
    a = np.asarray(amp, np.float64)
    F = np.hypot(a[0], a[1]) * cfg.m / cfg.dt
    return Push(np.full(B, F), a[None], steps, duration=pr.HERDT_D, profile=profile(pr.HERDT_D))


@pytest.mark.parametrize("name", pr.HERDT_WALKS + ((pr.HERDT_RAMP_WALK, "ramp"),))
def test_herdt_walks_vs_pushed_loop(name):
    """A D = 5 half-sine push on xy at the case's kick step (n17_n3: truncated by the walk's end),
    on each kernel instance, against the pushed oracle loop; one walk also under the rising
    profile, which tells w_j from w_(D−1−j)."""
    name, profile = (name, ps.half_sine) if isinstance(name, str) else (name[0], pr.ramp)
    case = pr.herdt_case(name)
    cfg = hc.make_config(case["cfg_kw"])
    n = case["n"]
    prm, nb = _herdt_inputs(cfg, case["states"], n)
    push = _herdt_push(cfg, 1, int(case["kick_step"]), profile=profile)
    dvel = push.velocity_steps(cfg.dt, cfg.m, 1, n)[0]
    assert np.allclose(dvel, pr.herdt_window(case, profile)[2], rtol=1e-14, atol=0.0)
    assert np.count_nonzero(dvel[:, 1]) == min(pr.HERDT_D, n - 1 - case["kick_step"])
    com_o, y_o, foot_o, x_o = pr.herdt_rollout_pushed(cfg, case["x0"], case["v"], case["states"],
                                                      dvel)
    hist, foot, st = _herdt_plan(cfg).herdt_rollout(prm, case["v"], case["states"], nb[0],
                                                    case["x0"][None], push=push, mass=cfg.m)
    hist, foot = hist[0].cpu().numpy(), foot[0].cpu().numpy()
    assert int(st[0]) == 0
    errs = (rmse(hist[:, :, 0], com_o), np.abs(foot - foot_o).max(),
            np.abs(hist[:, 1, :] - y_o).max(), np.abs(hist[:, 0, :] - x_o).max())
    print(f"MEASURED herdt {name}: CoM RMSE %.1e feet %.1e y %.1e x %.1e" % errs)
    assert errs[0] <= 1e-9 and errs[1] <= 1e-9 and errs[2] <= 1e-8 and errs[3] <= 1e-8


def test_herdt_batch_with_per_walk_steps():
    """rollout_batch(): 33 different walks in one launch, a start step per walk (one outside the
    range), each against the pushed loop of that walk."""
    batch = hc.rollout_batch()
    cfg = hc.make_config(batch["cfg_kw"])
    n, B = batch["n"], len(batch["x0"])
    prm, nb = _herdt_inputs(cfg, batch["states"], n)
    steps = pr.herdt_batch_steps(n, B)
    push = _herdt_push(cfg, B, steps, amp=pr.HERDT_BATCH_AMP)
    dvel = push.velocity_steps(cfg.dt, cfg.m, B, n)
    assert not dvel[5].any() and np.count_nonzero(dvel[32, :, 0]) == 2
    hist, foot, st = _herdt_plan(cfg).herdt_rollout(prm, batch["v"], batch["states"], nb,
                                                    batch["x0"], push=push, mass=cfg.m)
    hist, foot, st = hist.cpu().numpy(), foot.cpu().numpy(), st.cpu().numpy()
    errs = []
    for b in range(B):
        com_o, y_o, foot_o, x_o = pr.herdt_rollout_pushed(cfg, batch["x0"][b], batch["v"][b],
                                                          batch["states"][b], dvel[b])
        errs.append((rmse(hist[b, :, :, 0], com_o), np.abs(foot[b] - foot_o).max(),
                     max(np.abs(hist[b, :, 1, :] - y_o).max(),
                         np.abs(hist[b, :, 0, :] - x_o).max())))
    errs = np.array(errs)
    print("MEASURED herdt batch: status", st.tolist(),
          "worst CoM RMSE %.1e feet %.1e history %.1e" % tuple(errs.max(axis=0)))
    assert np.all(st == 0), st
    assert errs[:, 0].max() <= 1e-9 and errs[:, 1].max() <= 1e-9 and errs[:, 2].max() <= 1e-8


# ----------------------------------------------------------------------------- 6: unconstrained

def _walk_bounds(n):
    """n samples of the default walk's bounds (420 stored; beyond, its last row repeated)."""
    d = golden("walk_n150.npz")
    zx, zn = d["zmax"], d["zmin"]
    if n > len(zx):
        zx = np.concatenate([zx, np.repeat(zx[-1:], n - len(zx), axis=0)])
        zn = np.concatenate([zn, np.repeat(zn[-1:], n - len(zn), axis=0)])
    return np.ascontiguousarray(zx[:n]), np.ascontiguousarray(zn[:n])


@pytest.mark.parametrize("n", (3, 66, 420, 600))
def test_unconstrained_vs_chained_rollouts(n):
    """The linear state response on top of the unpushed rollout, on the split kernels (n <= 513)
    and a long walk: ragged start steps (two outside the range), D = 1 with a one-weight profile,
    3, 20 and n + 5 (and 5 with a rising profile, which tells w_j from w_(D−1−j)), on x, y and
    xy, against chained oracle rollouts; two launches agree bit for
    bit."""
    key = ("unc",) + PAR150
    if key not in _PLANS:
        _PLANS[key] = Plan(torch.cuda.current_device(), *PAR150, False)
    plan = _PLANS[key]
    dt, m = PAR150[1], 40.0
    zmax, zmin = _walk_bounds(n)
    steps = np.array([0, n // 3, n - 2, n - 1, -1, max(n // 2 - 1, 0)], np.int64)
    S = len(steps)
    rng = np.random.default_rng([20261020, n])
    F = rng.uniform(20.0, 80.0, S) * np.where(rng.random(S) < 0.5, -1.0, 1.0)
    ang = rng.uniform(0.2, 1.3, S)
    x0 = np.zeros((S, 2, 3))
    h0 = plan.rollout(zmax, zmin, x0)[0].cpu().numpy()
    for D, w in ((1, np.array([0.7])), (3, None), (5, pr.ramp(5)), (20, ps.half_sine(20)),
                 (n + 5, None)):
        pushes = {"x": Push(F, (1, 0), steps, duration=D, profile=w),
                  "y": Push(F, (0, 1), steps, duration=D, profile=w),
                  "xy": Push(F, np.stack([np.cos(ang), np.sin(ang)], 1), steps, duration=D,
                             profile=w)}
        assert [p.axes for p in pushes.values()] == ["x", "y", "xy"]
        dvel = np.concatenate([p.velocity_steps(dt, m, S, n) for p in pushes.values()])
        ref = pr.chained(zmax, zmin, PAR150, dvel) if dvel.any() else \
            np.broadcast_to(h0[:1], (3 * S, n, 2, 3))
        for k, (axes, p) in enumerate(pushes.items()):
            h, st = plan.rollout(zmax, zmin, x0, push=p, mass=m)
            h2, _ = plan.rollout(zmax, zmin, x0, push=p, mass=m)
            assert torch.equal(h, h2)
            h = h.cpu().numpy()
            r, e = rmse(h[..., 0], ref[k * S:(k + 1) * S, ..., 0]), \
                float(np.abs(h - ref[k * S:(k + 1) * S]).max())
            print(f"MEASURED unconstrained n={n} D={D} {axes}: CoM RMSE {r:.2e} state {e:.2e}")
            assert r <= 1e-9 and e <= 1e-7, (n, D, axes, r, e)
            # walks without a push, rows up to the start step, and an axis not asked for: the
            # unpushed rollout's bits
            for b, s in enumerate(steps):
                upto = n if not 0 <= s < n - 1 else s + 1
                assert same_bits(h[b, :upto], h0[b, :upto]), (axes, b)
            if axes != "xy":
                other = 1 if axes == "x" else 0
                assert same_bits(np.ascontiguousarray(h[:, :, other]),
                                 np.ascontiguousarray(h0[:, :, other]))
            if n > 3:
                assert not np.array_equal(h[0], h0[0])


# ----------------------------------------------------------------------------- 7: critical_force

def test_critical_force_with_a_shove():
    """The N = 64 stored walk under a 20-sample shove at step 44: the bisection's final bracket
    holds critical_force_exact along (0, −1), (−1, 0) and (1, 1); along (0, −1) it holds the push
    map's 0.580999 N.  On the strict plan F_lo passes and F_hi fails when rolled out alone.  The
    scalar-sign, one-sample call keeps today's launches: bit-equal brackets."""
    d = golden("walk_n64.npz")
    c = ZMPController(MPCConfig(horizon=64, strict=False))
    for direction in ([[0.0, -1.0]], [[-1.0, 0.0]], [[1.0, 1.0]]):
        lo, hi = c.critical_force(d["zmax"], d["zmin"], force_step=44, direction=direction,
                                  duration=20)
        exact = c.critical_force_exact(d["zmax"], d["zmin"], force_step=44, direction=direction,
                                       duration=20)
        lo, hi, exact = float(lo[0]), float(hi[0]), float(exact[0])
        print(f"MEASURED shove along {direction[0]}: bracket [{lo:.9g}, {hi:.9g}] exact {exact:.9g}")
        assert lo <= exact <= hi and hi - lo <= 1000.0 / 2 ** 30 * 1.0001
        if direction == [[0.0, -1.0]]:
            assert lo <= 0.580999 + 5e-7 and hi >= 0.580999 - 5e-7  # (a six-digit figure)
    a = c.critical_force(d["zmax"], d["zmin"], force_step=44, direction=-1, iters=12)
    b = c.critical_force(d["zmax"], d["zmin"], force_step=44, direction=-1, iters=12, duration=1,
                         profile=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    s = ZMPController(MPCConfig(horizon=64, strict=True))
    plan = s._plan()
    zmax, zmin = dev(d["zmax"]), dev(d["zmin"])
    x0 = torch.zeros((1, 2, 3), dtype=torch.float64, device="cuda")
    h0, _ = plan.rollout(zmax, zmin, x0)
    # the clamped ZMP hides the push: the CoM criterion decides (5 cm beyond the unpushed walk's)
    dev_max = float(plan.walk_metrics(h0, zmax, zmin)[0, 6:8].max()) + 0.05
    lo, hi = s.critical_force(d["zmax"], d["zmin"], force_step=44, direction=[[0.0, -1.0]],
                              duration=20, max_com_dev=dev_max, iters=20)
    lo, hi = float(lo[0]), float(hi[0])
    print(f"MEASURED strict shove: bracket [{lo:.9g}, {hi:.9g}] at com_dev_max <= {dev_max:.4f}")
    assert 0.0 < lo < hi < 1000.0

    def alone(F):
        hist, st = plan.rollout(zmax, zmin, x0, push=Push(F, (0, -1), 44, duration=20),
                                mass=s.config.m)
        m = s.walk_metrics(hist, d["zmax"], d["zmin"])
        return hist, bool((m.viol_max <= 1e-9).all() and (m.com_dev_max <= dev_max).all()
                          and int(st[0]) == 0)

    assert alone(lo)[1] and not alone(hi)[1]
    # the controller's batch method is that rollout
    hist, st = s.generate_state_trajectory_batch(None, d["zmax"], d["zmin"],
                                                 push=Push(lo, (0, -1), 44, duration=20))
    assert torch.equal(hist, alone(lo)[0]) and int(st[0]) == 0
    com, hist2 = s.generate_com_trajectory_batch(None, d["zmax"], d["zmin"],
                                                 push=Push(lo, (0, -1), 44, duration=20))
    assert torch.equal(hist2, hist) and torch.equal(com, hist[..., 0])


# ----------------------------------------------------------------------------- 8: refusals

@pytest.mark.parametrize("solver", (1, 2))
def test_reduced_cholesky_solvers_refuse_a_shove(solver):
    """Solver 1 or 2 with D = 2: ZMPC_ESTATE, and the output buffers keep their prefill; the
    legacy push still runs there."""
    case = sc.rollout_case("jitter", 33)
    p = strict_plan(33, case["dt"], solver=solver)
    amp = case["kick"][:, None]
    h, st = pushed(p, case["zmax"], case["zmin"], case["x0"], amp, "y", steps=case["kick_step"],
                   D=2, expect=_native.ZMPC_ESTATE)
    assert b"reduced-Cholesky" in _native.load().zmpc_last_error()
    assert (h == -7.0).all() and (st == -7).all()
    h, st = pushed(p, case["zmax"], case["zmin"], case["x0"], amp, "y", steps=case["kick_step"])
    h0, s0 = p.rollout(case["zmax"], case["zmin"], case["x0"], kick=case["kick"],
                       kick_step=case["kick_step"])
    assert same_bits(h, h0.cpu().numpy()) and np.array_equal(st, s0.cpu().numpy())
