"""The device Herdt joint footstep QP (csrc/herdt.hip) beyond its default shape: horizons from 1
to the longest the LDS layout takes, every footstep count up to 8 and every kernel instance,
waves of mixed windows, the window-shape branches, non-default polytopes and geometry, and the
ZMPC_ST_INFEASIBLE fallback — all through Plan.herdt_step / Plan.herdt_rollout and
controllers.herdt.make_params, against the CPU oracle (oracle/herdt_oracle.py) on the seeded
cases of tests/herdt_cases.py.

Bars: those of tests/test_gpu_herdt.py (x_next 1e-9 relative to max(1, |ref|), footsteps 1e-9,
CoM RMSE 1e-9, y history 1e-8); forms that compute the same solution agree to 1e-11
(include/zmpc.h).  The oracle's own error on these inputs is <= 1.9e-11
(tests/test_herdt_cases_host.py).
"""
import numpy as np
import pytest
import torch

import herdt_cases as HC
from conftest import golden, rmse
from oracle import herdt_oracle as HO
from oracle.zmp_oracle import lipm

pytestmark = pytest.mark.gpu

from mpc_bipedal import _native  # noqa: E402
from mpc_bipedal.controllers import herdt as H  # noqa: E402
from mpc_bipedal.solver import Plan  # noqa: E402

ST, DS, SS = HC.ST, HC.DS, HC.SS


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")


def _plan(cfg):
    return Plan(0, cfg.horizon, cfg.dt, cfg.h, cfg.g, 1.0, 1e-6, False)


def _step(plan, prm, case, idx=slice(None)):
    xn, step, st = plan.herdt_step(prm, case["x"][idx], case["v"][idx], case["win"][idx],
                                   case["cur"][idx], case["foot"][idx], case["side"][idx])
    return xn.cpu().numpy(), step.cpu().numpy(), st.cpu().numpy()


def _assert_steps(xn, step, ref_xn, ref_step, idx=None):
    """x_next to 1e-9 relative to max(1, |ref|) per axis, the first footstep to 1e-9 absolute,
    NaN exactly where the reference has no footstep."""
    idx = range(len(ref_xn)) if idx is None else idx
    bad = []
    for b in idx:
        for ax in (0, 1):
            err = np.abs(xn[b, ax] - ref_xn[b, ax]).max()
            if not err <= 1e-9 * max(1.0, np.abs(ref_xn[b, ax]).max()):
                bad.append((b, "x_next", ax, err))
        none = np.isnan(ref_step[b])
        if not np.array_equal(np.isnan(step[b]), none):
            bad.append((b, "NaN", step[b]))
        elif not none.any() and not np.abs(step[b] - ref_step[b]).max() <= 1e-9:
            bad.append((b, "footstep", step[b], ref_step[b]))
    assert not bad, bad


@pytest.mark.parametrize("N,variant", HC.STEP_PARAMS,
                         ids=[f"{N}-{v}" for N, v in HC.STEP_PARAMS])
def test_herdt_step_shapes_vs_oracle(N, variant):
    """One launch of the whole batch of step_cases(N, variant), max_footsteps the batch's own
    maximum: every window against HO.herdt_step."""
    case, ref_xn, ref_step = HC.step_reference(N, variant)
    cfg = HC.make_config(case["cfg_kw"])
    m, _ = HC.case_m(case)
    assert np.array_equal(np.isnan(ref_step[:, 0]), m == 0)
    xn, step, st = _step(_plan(cfg), H.make_params(cfg, int(m.max())), case)
    assert np.all(st == 0), st
    _assert_steps(xn, step, ref_xn, ref_step)


def test_herdt_step_instances_agree():
    """The N = 17 batch (75 windows, three workgroups, the last one partial) on every kernel
    instance and window by window: a window with more footsteps than the forced max_footsteps
    is flagged, as is its 32-walk wave (ZMPC_ST_FACTOR, include/zmpc.h); every window the
    instance can hold equals the own-maximum run to 1e-11, flagged or not; every window
    launched alone (B = 1, its own footstep count) equals it to 1e-11."""
    case, _, _ = HC.step_reference(17, "a")
    cfg = HC.make_config(case["cfg_kw"])
    plan = _plan(cfg)
    m, _ = HC.case_m(case)
    B = len(m)
    assert m.max() == 8
    xn0, step0, st0 = _step(plan, H.make_params(cfg, 8), case)
    assert np.all(st0 == 0)

    def same(xa, sa, b):
        assert np.abs(xa - xn0[b]).max() <= 1e-11, b
        assert np.array_equal(np.isnan(sa), np.isnan(step0[b])), b
        if m[b] > 0:
            assert np.abs(sa - step0[b]).max() <= 1e-11, b

    for forced in (2, 4, 6, 7, 8):
        xn, step, st = _step(plan, H.make_params(cfg, forced), case)
        for b in range(B):
            wave = m[32 * (b // 32): 32 * (b // 32) + 32]
            if m[b] > forced:
                assert st[b] != 0, (forced, b)
            else:
                assert st[b] == (_native.ST_FACTOR if wave.max() > forced else 0), (forced, b)
                same(xn[b], step[b], b)
    for b in range(B):
        xn, step, st = _step(plan, H.make_params(cfg, int(m[b])), case, slice(b, b + 1))
        assert st[0] == 0, b
        same(xn[0], step[0], b)


def test_herdt_step_long_horizons():
    """N = 300 and N = 702 (the longest horizon the LDS layout takes) against the stored oracle
    answers of tests/golden/herdt_shapes.npz, a standing window at rest at N = 702 against the
    live oracle, and N = 703 refused with the launcher's message, after which a valid plan still
    works."""
    d = golden("herdt_shapes.npz")
    for N in HC.LONG_HORIZONS:
        case = HC.long_cases(N)
        cfg = HC.make_config(case["cfg_kw"])
        xn, step, st = _step(_plan(cfg), H.make_params(cfg, int(d[f"n{N}_m"].max())), case)
        assert np.all(st == 0), (N, st)
        _assert_steps(xn, step, d[f"n{N}_x_next"], d[f"n{N}_step"])
    N = 702
    kw702 = HC.config_kwargs(N, 1.5 / N)
    cfg = HC.make_config(kw702)
    plan, prm = _plan(cfg), H.make_params(cfg, int(d["n702_m"].max()))
    rest = dict(x=np.array([[[0.0, 0.0, 0.0], [0.1, 0.0, 0.0]]]), v=np.zeros((1, N, 2)),
                win=np.zeros((1, N), np.int8), cur=np.array([ST], np.int8),
                foot=np.array([[0.0, 0.1]]), side=np.array([0], np.int8), cfg_kw=kw702)
    ref_xn, ref_step = HC.solve_case(rest)
    xn, step, st = _step(plan, prm, rest)
    assert st[0] == 0
    _assert_steps(xn, step, ref_xn, ref_step)
    # one row more than the LDS holds: 224·N + 6400 bytes > 160 KiB from N = 703
    cfg3 = HC.make_config(dict(kw702, horizon=703))
    with pytest.raises(ValueError, match="horizon too long for the Herdt solver"):
        plan3 = _plan(cfg3)
        plan3.herdt_step(H.make_params(cfg3, 0), np.zeros((1, 2, 3)), np.zeros((1, 703, 2)),
                         np.zeros((1, 703), np.int8), np.zeros(1, np.int8), np.zeros((1, 2)),
                         np.zeros(1, np.int8))
    xn, step, st = _step(plan, prm, rest)
    assert st[0] == 0
    _assert_steps(xn, step, ref_xn, ref_step)


def _rollout_inputs(cfg, states, n):
    N = cfg.horizon
    st2 = np.atleast_2d(states)
    pad = np.concatenate([st2, np.repeat(st2[:, -1:], N, axis=1)], axis=1)
    nb = np.array([[t[0] for t in H.find_nb_steps(p)][:n] for p in pad], np.int32)
    return H.make_params(cfg, H.max_footsteps(pad, N, n)), nb


ROLLOUT_NAMES = [c["name"] for c in HC.rollout_cases()]


@pytest.mark.parametrize("name", ROLLOUT_NAMES)
def test_herdt_rollout_shapes_vs_oracle(name):
    """Short walks on each kernel instance (max_footsteps 2, 4, 5, 6, 7 and 8), starting
    mid-step, ending in a standing tail, kicked at the first, the middle and the last step,
    with the triangular and the rectangle / 16-gon polytopes (the side flip with unequal
    facet counts), n = 2 and 3 — against the oracle's rollout."""
    case = {c["name"]: c for c in HC.rollout_cases()}[name]
    cfg = HC.make_config(case["cfg_kw"])
    n = case["n"]
    com_o, y_o, foot_o, x_o = HC.rollout_reference(name)
    prm, nb = _rollout_inputs(cfg, case["states"], n)
    kick = None if case["kick_step"] < 0 else np.array([HC.case_kick(case)])
    hist, foot, st = _plan(cfg).herdt_rollout(prm, case["v"], case["states"], nb[0],
                                              case["x0"][None], kick=kick,
                                              kick_step=case["kick_step"])
    hist, foot = hist[0].cpu().numpy(), foot[0].cpu().numpy()
    assert int(st[0]) == 0
    assert hist.shape == (n, 2, 3) and foot.shape == (n, 2)
    assert rmse(hist[:, :, 0], com_o) <= 1e-9
    assert np.abs(foot - foot_o).max() <= 1e-9
    assert np.abs(hist[:, 1, :] - y_o).max() <= 1e-8
    assert np.abs(hist[:, 0, :] - x_o).max() <= 1e-8


def test_herdt_rollout_single_sample():
    """n = 1: no solve; the history is x0, the foot (0, foot_spread), the status 0
    (zmpc_herdt_rollout accepts n >= 1)."""
    cfg = HC.make_config(HC.config_kwargs(17, 0.07, "b"))
    x0 = np.array(HC.X0_A)[None]
    prm, nb = _rollout_inputs(cfg, np.array([ST], np.int8), 1)
    hist, foot, st = _plan(cfg).herdt_rollout(prm, np.zeros((1, 2)), np.array([ST], np.int8),
                                              nb[0], x0, kick=np.array([0.1]), kick_step=0)
    assert np.array_equal(hist.cpu().numpy(), x0[:, None])
    assert np.array_equal(foot.cpu().numpy(), [[[0.0, cfg.foot_spread]]])
    assert int(st[0]) == 0


def test_herdt_rollout_batch_of_different_walks():
    """B = 33 different walks in one launch (a full wave and one walk in a second workgroup;
    per-walk v_ref, states, nb_next, x0 and kicks; footstep counts differing between the lanes):
    each walk against the oracle's rollout of that walk.

    Walk 23 (standing 6, ssp 5, tail 6, v = (0.1575, 0.01)) is the one on which the kernel's
    block exchange of working-set rows used to cycle from step 14 on (ZMPC_ST_MAXITER at any
    pass cap, CoM error 5.5e-3); with the least-index fallback of csrc/herdt.hip it converges
    in 23 passes and agrees to 9e-15."""
    batch = HC.rollout_batch()
    cfg = HC.make_config(batch["cfg_kw"])
    n, B = batch["n"], len(batch["x0"])
    prm, nb = _rollout_inputs(cfg, batch["states"], n)
    hist, foot, st = _plan(cfg).herdt_rollout(prm, batch["v"], batch["states"], nb, batch["x0"],
                                              kick=batch["kick"], kick_step=batch["kick_step"])
    hist, foot, st = hist.cpu().numpy(), foot.cpu().numpy(), st.cpu().numpy()
    errs = []
    for b in range(B):
        com_o, y_o, foot_o, _ = HC.rollout_ref(cfg, *HC.batch_walk(batch, b))
        errs.append((rmse(hist[b, :, :, 0], com_o), np.abs(foot[b] - foot_o).max(),
                     np.abs(hist[b, :, 1, :] - y_o).max()))
    errs = np.array(errs)
    print("batch of walks: status", st.tolist(), "worst CoM RMSE %.1e feet %.1e y history %.1e"
          % tuple(errs.max(axis=0)), "per walk", errs.max(axis=1).tolist())
    assert np.all(st == 0), st
    assert errs[:, 0].max() <= 1e-9 and errs[:, 1].max() <= 1e-9 and errs[:, 2].max() <= 1e-8


def _infeasible_params(cfg, max_steps, which):
    """make_params' struct with both swing polygons overwritten by hand (reachable through the
    C-ABI only): (i) the contradictory pair d_x <= −1, d_x >= 1; (ii) the single, unbounded
    half-space d_x <= −10 (the unconstrained footstep lies outside it).  The API wants at least
    three facets: the first half-space is repeated."""
    prm = H.make_params(cfg, max_steps)
    rows = {"contradictory": [(1.0, 0.0, -1.0), (-1.0, 0.0, -1.0), (1.0, 0.0, -1.0)],
            "unbounded": [(1.0, 0.0, -10.0)] * 3}[which]
    for sd in (0, 1):
        prm.nfacets[sd] = len(rows)
        for f in range(_native.HERDT_MAX_FACETS):
            for c in range(3):
                prm.facets[sd][f][c] = rows[f][c] if f < len(rows) else 0.0
    return prm


@pytest.mark.parametrize("which", ["contradictory", "unbounded"])
def test_herdt_infeasible_polytope_fallback(which):
    """ZMPC_ST_INFEASIBLE (include/zmpc.h): a swing polygon with no usable facet and the
    unconstrained footstep outside it.  Step mode, the N = 17 batch: every window with a
    footstep reports that bit (alone or with the pass cap's) and takes the fallback — zero jerk
    on both axes (x_next = A x), the footstep at the current foot; the windows without a
    footstep in the same waves are solved as ever.  Rollout mode: the status carries the bit and
    the walk equals the oracle's rollout in which every window with a footstep takes the
    fallback (zero jerk, the first footstep at the air foot's centre)."""
    case, ref_xn, ref_step = HC.step_reference(17, "a")
    cfg = HC.make_config(case["cfg_kw"])
    plan = _plan(cfg)
    m, _ = HC.case_m(case)
    A, _, _ = lipm(cfg.dt, cfg.h, cfg.g)
    xn, step, st = _step(plan, _infeasible_params(cfg, 8, which), case)
    assert np.any(m == 0) and np.any(m > 0)
    for b in range(len(m)):
        if m[b] == 0:
            assert st[b] == 0, b
            continue
        assert st[b] in (_native.ST_INFEASIBLE, _native.ST_INFEASIBLE | _native.ST_MAXITER), \
            (b, st[b])
        for ax in (0, 1):
            want = A @ case["x"][b, ax]
            assert np.abs(xn[b, ax] - want).max() <= 1e-15 * max(1.0, np.abs(want).max()), b
        assert np.array_equal(step[b], case["foot"][b]), b
    _assert_steps(xn, step, ref_xn, ref_step, idx=np.where(m == 0)[0])

    # rollout: a standing start longer than the horizon (windows without a footstep), a few
    # steps, a short standing tail
    n = 40
    states, v = HC.walk_schedule(n, 20, 1, 4, 5)
    kw = HC.config_kwargs(17, 0.07)
    cfg = HC.make_config(kw)
    x0 = np.array(HC.X0_A)
    kick, kick_step = 0.01, n // 2

    def fallback_step(cfg, x, y, vw, fx, fy, cur, win, side, air):
        if len(HO.support_segments(cur, win)) - 1 == 0:
            return HO.herdt_step(cfg, x, y, vw, fx, fy, cur, win, side)
        return A @ np.asarray(x, np.float64), A @ np.asarray(y, np.float64), air[0], air[1]

    com_o, y_o, foot_o, x_o = HC.rollout_ref(cfg, x0, v, states, kick, kick_step,
                                             step_fn=fallback_step)
    assert np.abs(x_o).max() <= 10 and np.abs(y_o).max() <= 10
    _, nb = _rollout_inputs(cfg, states, n)
    pad = np.concatenate([states, np.repeat(states[-1:], 17)])
    prm = _infeasible_params(cfg, H.max_footsteps(pad[None], 17, n), which)
    hist, foot, st = _plan(cfg).herdt_rollout(prm, v, states, nb[0], x0[None],
                                              kick=np.array([kick]), kick_step=kick_step)
    hist, foot = hist[0].cpu().numpy(), foot[0].cpu().numpy()
    assert int(st[0]) & _native.ST_INFEASIBLE
    assert (int(st[0]) & ~(_native.ST_INFEASIBLE | _native.ST_MAXITER)) == 0
    assert np.all(np.isfinite(hist)) and np.all(np.isfinite(foot))
    assert np.abs(hist[:, 0, :] - x_o).max() <= 1e-9
    assert np.abs(hist[:, 1, :] - y_o).max() <= 1e-9
    assert np.abs(foot - foot_o).max() <= 1e-9
