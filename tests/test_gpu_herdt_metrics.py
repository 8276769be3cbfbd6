"""Herdt walk metrics on the device (zmpc_herdt_walk_metrics, csrc/herdt_metrics.hip) and the
critical shove of the footstep-adapting controller (ZMPController.critical_force_herdt): the
emulation's seeded cases with the same assertions, bit-stable launches, the device's own Herdt
rollouts against the NumPy statement of the same arrays, and the bisection against the oracle
loop on n17_triangle."""
import numpy as np
import pytest
import torch

import herdt_cases as hc
import herdt_metrics_cases as mc
import push_rollout_cases as pr
import push_shaped_cases as ps

pytestmark = pytest.mark.gpu

from mpc_bipedal.analysis import (HerdtWalkMetrics, Push, herdt_params_facets,  # noqa: E402
                                  herdt_walk_metrics_reference)
from mpc_bipedal.controllers import ZMPController  # noqa: E402
from mpc_bipedal.controllers import herdt as H  # noqa: E402
from mpc_bipedal.solver import Plan  # noqa: E402

_PLANS = {}


def _plan(N=8, dt=0.07, h=0.75, g=9.81):
    key = (N, dt, h, g)
    if key not in _PLANS:
        _PLANS[key] = Plan(torch.cuda.current_device(), N, dt, h, g, 1.0, 1e-6, False)
    return _PLANS[key]


def _device(case, prm=None, count_tol=mc.COUNT_TOL, out=None):
    p = _plan()
    assert p.consts["hg"] == mc.HG
    dev = torch.device("cuda", p.device)
    hist = torch.as_tensor(case["hist"], device=dev)
    foot = torch.as_tensor(case["foot"], device=dev)
    m = p.herdt_walk_metrics(mc.make_params() if prm is None else prm, hist, foot,
                             case["states"], lengths=case["lengths"], foot_ref=case["foot_ref"],
                             count_tol=count_tol, out=out)
    return m.cpu().numpy()


# ----------------------------------------------------------------------------- the kernel

@pytest.mark.parametrize("shared,ref", ((False, "none"), (True, "shared"), (False, "walk")))
@pytest.mark.parametrize("n", mc.EMU_N)
def test_kernel_random(n, shared, ref):
    case = mc.emu_case(n, shared, ref)
    mc.assert_exact(_device(case), mc.reference(case))


def test_kernel_ragged_ties_and_non_finite():
    case = mc.hostile_case()
    got = _device(case)
    mc.assert_exact(got, mc.reference(case))
    assert got[4, 2:4].tolist() == [63.0, 63.0]
    assert got[5, 1] == np.inf and got[5, 3] == 70.0 and np.isnan(got[5, 14])
    assert got[6, 0] == np.inf and got[6, 2] == 33.0 and np.isnan(got[6, 14])
    assert np.isfinite(got[7]).all()


def test_kernel_without_facets():
    case = mc.emu_case(129, False, "none")
    none = (np.zeros((0, 3)), np.zeros((0, 3)))
    got = _device(case, prm=mc.make_params(nfacets=False))
    mc.assert_exact(got, mc.reference(case, facets=none))
    assert (got[:, 14] == np.inf).all()


def test_two_launches_agree_bit_for_bit_and_write_into_out():
    case = mc.emu_case(129, False, "walk", B=67)
    p = _plan()
    out = torch.full((67, 16), -7.0, dtype=torch.float64, device=torch.device("cuda", p.device))
    a = _device(case, out=out)
    assert np.array_equal(a, out.cpu().numpy(), equal_nan=True)
    b = _device(case)
    assert a.tobytes() == b.tobytes()
    mc.assert_exact(a, mc.reference(case))


def test_python_argument_errors():
    p = _plan()
    dev = torch.device("cuda", p.device)
    hist = torch.zeros((2, 5, 2, 3), dtype=torch.float64, device=dev)
    foot = torch.zeros((2, 5, 2), dtype=torch.float64, device=dev)
    st = np.zeros((2, 5), np.int8)
    prm = mc.make_params()
    with pytest.raises(ValueError, match="foot must be"):
        p.herdt_walk_metrics(prm, hist, foot[:, :4], st)
    with pytest.raises(ValueError, match="states must be"):
        p.herdt_walk_metrics(prm, hist, foot, st[:1])
    with pytest.raises(ValueError, match="foot_ref must be"):
        p.herdt_walk_metrics(prm, hist, foot, st, foot_ref=np.zeros((3, 5, 2)))
    with pytest.raises(ValueError, match="lengths must be"):
        p.herdt_walk_metrics(prm, hist, foot, st, lengths=[1, 2, 3])
    with pytest.raises(ValueError, match="count_tol"):
        p.herdt_walk_metrics(prm, hist, foot, st, count_tol=-1.0)
    with pytest.raises(ValueError, match="out must be"):
        p.herdt_walk_metrics(prm, hist, foot, st, out=torch.zeros((2, 12), dtype=torch.float64,
                                                                  device=dev))


# ----------------------------------------------------------------------------- device rollouts

def _herdt_inputs(cfg, states, n):
    N = cfg.horizon
    st2 = np.atleast_2d(states)
    pad = np.concatenate([st2, np.repeat(st2[:, -1:], N, axis=1)], axis=1)
    nb = np.array([[t[0] for t in H.find_nb_steps(p)][:n] for p in pad], np.int32)
    return H.make_params(cfg, H.max_footsteps(pad, N, n)), nb


def _against_statement(p, cfg, prm, hist, foot, states, foot_ref=None):
    got = p.herdt_walk_metrics(prm, hist, foot, states, foot_ref=foot_ref).cpu().numpy()
    want = herdt_walk_metrics_reference(
        hist.cpu().numpy(), foot.cpu().numpy(), states, p.consts["hg"], cfg.foot_length,
        cfg.foot_width, cfg.foot_spread, facets=herdt_params_facets(prm),
        foot_ref=None if foot_ref is None else foot_ref.cpu().numpy())
    mc.assert_close(got, want)
    return got


@pytest.mark.parametrize("name", [c["name"] for c in hc.rollout_cases()])
def test_device_rollout_cases(name):
    """The device's own walk, reduced on the device, equals the NumPy statement of the same
    arrays, and its ZMP stays in the box of foot[i − 1] to the project's bar."""
    case = pr.herdt_case(name)
    cfg = hc.make_config(case["cfg_kw"])
    n = case["n"]
    prm, nb = _herdt_inputs(cfg, case["states"], n)
    p = _plan(cfg.horizon, cfg.dt, cfg.h, cfg.g)
    hist, foot, st = p.herdt_rollout(prm, case["v"], case["states"], nb[0], case["x0"][None],
                                     kick=np.array([hc.case_kick(case)]),
                                     kick_step=case["kick_step"])
    assert int(st[0]) == 0
    got = _against_statement(p, cfg, prm, hist, foot, case["states"])
    m = HerdtWalkMetrics(got)
    print(f"MEASURED herdt metrics {name}: viol_max {m.viol_max.max():.3g} dcm_dev_max "
          f"{m.dcm_dev_max.max():.3g} reach_slack_min {m.reach_slack_min[0]:.3g}")
    assert m.viol_max.max() <= 1e-9
    assert m.steps_landed[0] == len(mc.landings_of(case["states"]))


def test_device_pushed_batch():
    """rollout_batch(): 33 different walks under a shove with a start step per walk; foot_ref is
    the unpushed launch's feet."""
    batch = hc.rollout_batch()
    cfg = hc.make_config(batch["cfg_kw"])
    n, B = batch["n"], len(batch["x0"])
    prm, nb = _herdt_inputs(cfg, batch["states"], n)
    a = np.asarray(pr.HERDT_BATCH_AMP, np.float64)
    push = Push(np.full(B, np.hypot(a[0], a[1]) * cfg.m / cfg.dt), a[None],
                pr.herdt_batch_steps(n, B), duration=pr.HERDT_D,
                profile=ps.half_sine(pr.HERDT_D))
    p = _plan(cfg.horizon, cfg.dt, cfg.h, cfg.g)
    _, foot0, st0 = p.herdt_rollout(prm, batch["v"], batch["states"], nb, batch["x0"])
    hist, foot, st = p.herdt_rollout(prm, batch["v"], batch["states"], nb, batch["x0"],
                                     push=push, mass=cfg.m)
    assert not st0.any() and not st.any()
    got = _against_statement(p, cfg, prm, hist, foot, batch["states"], foot_ref=foot0)
    m = HerdtWalkMetrics(got)
    print(f"MEASURED herdt metrics batch: viol_max {m.viol_max.max():.3g} dcm_dev_max "
          f"{m.dcm_dev_max.max():.3g} step_shift_max {m.step_shift_max.max():.3g} "
          f"reach_slack_min {m.reach_slack_min.min():.3g}")
    assert m.viol_max.max() <= 1e-9
    assert m.step_shift_max[5].max() == 0 and m.step_shift_max.max() > 0  # walk 5: no push


# ----------------------------------------------------------------------------- the critical shove

def _shove_controller():
    case = pr.herdt_case(mc.SHOVE_WALK)
    return ZMPController(hc.make_config(case["cfg_kw"])), case


def _shove_kwargs(**kw):
    return dict(force_step=mc.SHOVE_STEP, duration=mc.SHOVE_D,
                profile=ps.half_sine(mc.SHOVE_D), **kw)


def test_critical_force_herdt_vs_oracle():
    """n17_triangle, a half-sine of D = 5 at step 25, max_dcm_dev = 1 m, the four directions of
    the host test as one batch: the oracle loop passes at F_lo·(1 − 1e-6) and fails at
    F_hi·(1 + 1e-6), the margin of the push-map tests; the walk falls because it ran out of
    reach."""
    ctl, case = _shove_controller()
    dirs = np.array([d for d, _ in mc.SHOVES])
    lo, hi = ctl.critical_force_herdt(case["v"], case["states"], mc.MAX_DCM_DEV, direction=dirs,
                                      **_shove_kwargs())
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    print("MEASURED critical_force_herdt:", lo.tolist(), "oracle", [f for _, f in mc.SHOVES])
    assert np.array_equal(hi - lo, np.full(4, 1000.0 / 2 ** 30))
    for b, (d, fstar) in enumerate(mc.SHOVES):
        assert mc.shove_passes(lo[b] * (1 - 1e-6), d), (d, lo[b])
        assert not mc.shove_passes(hi[b] * (1 + 1e-6), d), (d, hi[b])
        assert abs(lo[b] - fstar) < 1e-3
    _, hist, foot = ctl.generate_com_trajectory_herdt_batch(
        None, case["v"], case["states"],
        push=Push(lo, dirs, mc.SHOVE_STEP, duration=mc.SHOVE_D,
                  profile=ps.half_sine(mc.SHOVE_D)))
    m = ctl.herdt_walk_metrics(hist, foot, case["states"])
    slack = m.reach_slack_min.cpu().numpy()
    print("MEASURED reach_slack_min at F_lo:", slack.tolist(),
          "dcm_dev_max", m.dcm_dev_max.max(dim=1).values.tolist())
    assert (slack <= 1e-9).all()
    assert (m.dcm_dev_max.max(dim=1).values <= mc.MAX_DCM_DEV).all()


def test_critical_force_herdt_conventions():
    ctl, case = _shove_controller()
    # the unpushed walk's DCM already reaches 0.36 m: a bound below it fails with no push at all
    lo, hi = ctl.critical_force_herdt(case["v"], case["states"], 0.2, direction=-1, iters=3,
                                      **_shove_kwargs())
    assert torch.isnan(lo).all() and torch.isnan(hi).all() and lo.shape == (1,)
    # a bound that nothing reaches at F_hi: the search limit in both
    lo, hi = ctl.critical_force_herdt(case["v"], case["states"], 1e300, direction=[-1.0, 1.0],
                                      iters=3, **_shove_kwargs())
    assert lo.tolist() == [1000.0, 1000.0] and hi.tolist() == [1000.0, 1000.0]
    # a sign of +1 is the planar direction (0, 1), and max_com_dev joins the criteria
    kw = _shove_kwargs(iters=12)
    a = ctl.critical_force_herdt(case["v"], case["states"], 1.0, direction=+1, **kw)
    b = ctl.critical_force_herdt(case["v"], case["states"], 1.0, direction=[[0.0, 2.0]], **kw)
    c = ctl.critical_force_herdt(case["v"], case["states"], 1.0, direction=+1, max_com_dev=0.3,
                                 **kw)
    assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()
    assert float(c[0]) < float(a[0])


def test_critical_force_herdt_argument_errors():
    ctl, case = _shove_controller()
    v, st = case["v"], case["states"]
    with pytest.raises(ValueError, match="duration"):
        ctl.critical_force_herdt(v, st, 1.0, duration=0)
    with pytest.raises(ValueError, match=r"\[B\]"):
        ctl.critical_force_herdt(v, st, 1.0, force_step=[20, 21, 22, 23], direction=[1, -1, 1])
    with pytest.raises(ValueError, match=r"\[B\]"):
        ctl.critical_force_herdt(v, st, 1.0, x_init=np.zeros((4, 2, 3)),
                                 direction=np.ones((3, 2)))
    with pytest.raises(TypeError):
        ctl.critical_force_herdt(v, st)
    with pytest.raises(ValueError, match="max_dcm_dev"):
        ctl.critical_force_herdt(v, st, None)
    with pytest.raises(ValueError, match="F_hi"):
        ctl.critical_force_herdt(v, st, 1.0, F_hi=0.0)
