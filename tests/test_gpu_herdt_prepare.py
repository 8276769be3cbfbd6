"""Footstep bookkeeping of Herdt batches on the device (csrc/herdt_prep.hip, zmpc_herdt_prepare):
every seeded schedule of tests/herdt_prepare_cases.py against the host bookkeeping, exactly; the
batch paths of ZMPController prepare on the device and never call the host loop; a ragged batch
of different gaits equals its walks launched alone through the host route (the bars of
test_gpu_herdt.py::test_herdt_per_walk_schedules_equal_single_walks: CoM RMSE 1e-9, feet 1e-9,
every status 0); critical_force_herdt with walk_lengths equals the single-walk calls bracket for
bracket; generate_speed_and_state_batch equals generate_speed_and_state of each configuration
(1e-12, the bar of test_gpu_parity.py::test_speed_generator_wieber_vs_reference; classic:
exactly)."""
import ctypes

import numpy as np
import pytest
import torch

import herdt_prepare_cases as pc
from conftest import rmse

pytestmark = pytest.mark.gpu

from mpc_bipedal import _native  # noqa: E402
from mpc_bipedal.config import MPCConfig  # noqa: E402
from mpc_bipedal.controllers import ZMPController, herdt  # noqa: E402
from mpc_bipedal.generators import SpeedTrajectoryGenerator  # noqa: E402
from mpc_bipedal.generators.cop_generator import cop_params  # noqa: E402
from mpc_bipedal.solver import Plan  # noqa: E402

GUARD = 192   # sentinel elements on either side of every output
SENTINEL = -77
_PLANS = {}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")


def _plan(N):
    if N not in _PLANS:
        _PLANS[N] = Plan(0, N, 0.03, 0.75, 9.81, 1.0, 1e-6, False)
    return _PLANS[N]


def _guarded(count, dtype):
    """A sentinel-filled device buffer with guard zones: (whole tensor, pointer to its interior)."""
    t = torch.full((count + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda:0")
    return t, ctypes.c_void_p(t.data_ptr() + GUARD * t.element_size())


def _raw(plan, case, clean=True, steps=True, host=True):
    """One zmpc_herdt_prepare call into guarded, sentinel-filled outputs: (states_out, nb_next,
    max_steps, max_footsteps), None for an output that was not asked for."""
    B, n = case["states"].shape
    st = torch.tensor(np.array(case["states"]), device="cuda:0")  # (the cases are read-only)
    ln = None if case["lengths"] is None else torch.tensor(np.array(case["lengths"]),
                                                           device="cuda:0")
    bufs = {"nb": _guarded(B * n, torch.int32)}
    if clean:
        bufs["clean"] = _guarded(B * n, torch.int8)
    if steps:
        bufs["steps"] = _guarded(B, torch.int32)
    word = ctypes.c_int32(SENTINEL)
    ptr = lambda k: bufs[k][1] if k in bufs else None  # noqa: E731
    rc = _native.load().zmpc_herdt_prepare(
        plan.handle, B, n, ctypes.c_void_p(st.data_ptr()), n,
        None if ln is None else ctypes.c_void_p(ln.data_ptr()), ptr("clean"), ptr("nb"),
        ptr("steps"), ctypes.byref(word) if host else None)
    _native.check(rc, "zmpc_herdt_prepare")
    # synchronous: no torch.cuda.synchronize() before the outputs are read
    out = {}
    for k, (t, _) in bufs.items():
        h = t.cpu().numpy()
        assert (h[:GUARD] == SENTINEL).all() and (h[-GUARD:] == SENTINEL).all(), k
        out[k] = h[GUARD:-GUARD].reshape((B, n) if k != "steps" else (B,))
    return out.get("clean"), out["nb"], out.get("steps"), word.value if host else None


@pytest.mark.parametrize("n,N", pc.SHAPES)
def test_prepare_equals_the_host_bookkeeping(n, N):
    """All four outputs exactly, each batch in one call: no lengths, ragged with −1 past the walk,
    ragged with a valid pattern past the walk; every output element is overwritten (the wanted
    values never equal the sentinel) and nothing outside them is."""
    plan = _plan(N)
    for variant in pc.VARIANTS:
        c = pc.case(n, N, variant)
        clean, nb, steps, most = _raw(plan, c)
        assert np.array_equal(clean, c["want_states"]), variant
        assert np.array_equal(nb, c["want_nb"]), variant
        assert np.array_equal(steps, c["want_steps"]), variant
        assert most == c["want_most"], variant
    # the optional outputs left out, one at a time and together
    c = pc.case(n, N, "ragged_alt")
    for kw in (dict(clean=False), dict(steps=False), dict(host=False),
               dict(clean=False, steps=False, host=False)):
        clean, nb, steps, most = _raw(plan, c, **kw)
        assert np.array_equal(nb, c["want_nb"]), kw
        assert clean is None or np.array_equal(clean, c["want_states"]), kw
        assert steps is None or np.array_equal(steps, c["want_steps"]), kw
        assert most is None or most == c["want_most"], kw


def test_plan_herdt_prepare_forms():
    """Plan.herdt_prepare: NumPy and device-tensor input, the shared [n] form ([n], [n], [1]), one
    schedule cut at B lengths, and an empty batch."""
    n, N = 359, 150
    plan = _plan(N)
    c = pc.case(n, N, "ragged_pad")
    for states, lengths in ((np.array(c["states"]), np.array(c["lengths"])),
                            (torch.tensor(np.array(c["states"]), device="cuda:0"),
                             torch.tensor(np.array(c["lengths"]), device="cuda:0"))):
        clean, nb, steps, most = plan.herdt_prepare(states, lengths)
        assert (clean.dtype, nb.dtype, steps.dtype) == (torch.int8, torch.int32, torch.int32)
        assert clean.device == nb.device == steps.device == torch.device("cuda", 0)
        assert np.array_equal(clean.cpu().numpy(), c["want_states"])
        assert np.array_equal(nb.cpu().numpy(), c["want_nb"])
        assert np.array_equal(steps.cpu().numpy(), c["want_steps"])
        assert isinstance(most, int) and most == c["want_most"]
    st = pc.default_states()
    want = pc.answer(st, None, N)
    clean, nb, steps, most = plan.herdt_prepare(st)
    assert tuple(clean.shape) == tuple(nb.shape) == (len(st),) and tuple(steps.shape) == (1,)
    assert np.array_equal(clean.cpu().numpy(), want[0][0])
    assert np.array_equal(nb.cpu().numpy(), want[1][0]) and most == int(want[2][0])
    lengths = np.array([302, 1, 2, 251, 252, 253, 0, 400, 77, 130])
    clean, nb, steps, most = plan.herdt_prepare(st, lengths)
    want = pc.answer(np.broadcast_to(st, (len(lengths), len(st))), lengths, N)
    assert np.array_equal(clean.cpu().numpy(), want[0]) and np.array_equal(nb.cpu().numpy(), want[1])
    assert np.array_equal(steps.cpu().numpy(), want[2]) and most == int(want[2].max())
    clean, nb, steps, most = plan.herdt_prepare(np.zeros((0, 5), np.int8))
    assert tuple(nb.shape) == (0, 5) and tuple(steps.shape) == (0,) and most == 0
    with pytest.raises(ValueError, match="lengths must be"):
        plan.herdt_prepare(np.array(c["states"]), np.array(c["lengths"][:5]))


# --------------------------------------------------------------------------- the controller

N_WALK, DT_WALK = 33, 0.03
# (distance, step_length, ssp_duration, dsp_duration, standing_duration): 66, 71, 78, 108, 87 and
# 74 samples at dt = 0.03
GAITS = ((0.9, 0.3, 0.24, 0.03, 0.30), (1.2, 0.3, 0.21, 0.03, 0.45), (0.6, 0.2, 0.27, 0.06, 0.30),
         (1.0, 0.25, 0.30, 0.03, 0.60), (0.8, 0.2, 0.24, 0.06, 0.36), (0.5, 0.25, 0.36, 0.03, 0.30))
COUNTS = (66, 71, 78, 108, 87, 74)
FORCES = np.array([20.0, 35.0, 0.0, 40.0, 15.0, 30.0])


def _cfg(gait=None, **kw):
    base = dict(method="herdt", horizon=N_WALK, dt=DT_WALK, strict=False, add_force=True)
    if gait is not None:
        d, sl, ssp, dsp, sd = gait
        base.update(distance=d, step_length=sl, ssp_duration=ssp, dsp_duration=dsp,
                    standing_duration=sd)
    base.update(kw)
    return MPCConfig(**base)


@pytest.fixture(scope="module")
def ragged():
    """The six gaits as one ragged batch on the device, classic speeds: (controller, v_ref,
    states, lengths, lengths on the host)."""
    cfg = _cfg(speed_generation="classic")
    params = np.array([cop_params(_cfg(g)) for g in GAITS])
    v, st, nlen = SpeedTrajectoryGenerator(cfg).generate_speed_and_state_batch(params)
    return ZMPController(cfg), v, st, nlen, nlen.cpu().numpy()


def test_ragged_batch_equals_the_walks_alone(ragged):
    """Each walk of the ragged batch against the same walk launched alone on its own n_b rows
    through the host route (herdt.find_nb_steps, herdt.max_footsteps, the one-step kick of
    zmpc_herdt_rollout at n_b // 2)."""
    c, v, st, nlen, nl = ragged
    assert tuple(nl) == COUNTS and tuple(st.shape) == (6, max(COUNTS))
    com, hist, foot, status = c.generate_com_trajectory_herdt_batch(
        None, v, st, F_ext=FORCES, walk_lengths=nlen, return_status=True)
    assert torch.isfinite(hist).all() and torch.isfinite(foot).all()
    assert (status == 0).all()
    com, hist, foot = com.cpu().numpy(), hist.cpu().numpy(), foot.cpu().numpy()
    vh, sh = v.cpu().numpy(), st.cpu().numpy()
    kick = c.config.dt * FORCES / c.config.m
    for b, k in enumerate(nl):
        assert (sh[b, k:] == -1).all()
        h1, f1, s1 = c._herdt_rollout(np.zeros((1, 2, 3)), vh[b, :k], sh[b, :k], kick[b:b + 1],
                                      k // 2, check=False)
        h1, f1 = h1[0].cpu().numpy(), f1[0].cpu().numpy()
        assert int(s1[0]) == 0
        print(f"walk {b}: n_b {k}, CoM RMSE {rmse(com[b, :k], h1[:, :, 0]):.3g}, feet "
              f"{np.abs(foot[b, :k] - f1).max():.3g}")
        assert rmse(com[b, :k], h1[:, :, 0]) <= 1e-9, b
        assert np.abs(foot[b, :k] - f1).max() <= 1e-9, b
        if FORCES[b]:
            # the kick landed at n_b // 2: sample n_b // 2 + 1 is the first that differs from
            # the unkicked walk, by the whole velocity step
            h0, _, _ = c._herdt_rollout(np.zeros((1, 2, 3)), vh[b, :k], sh[b, :k], None, -1,
                                        check=False)
            d = np.abs(hist[b, :k] - h0[0].cpu().numpy()).max(axis=(1, 2))
            assert (d[:k // 2 + 1] <= 1e-9).all() and abs(d[k // 2 + 1] - kick[b]) <= 1e-9, b


def test_batch_paths_do_not_call_the_host_loop(ragged, monkeypatch):
    """With the states on the device neither batch path runs the host bookkeeping."""
    c, v, st, nlen, nl = ragged

    def refuse(*a, **k):
        raise AssertionError("host bookkeeping called on a batch path")
    monkeypatch.setattr(herdt, "find_nb_steps", refuse)
    monkeypatch.setattr(herdt, "max_footsteps", refuse)
    k = int(nl[0])
    com, hist, foot = c.generate_com_trajectory_herdt_batch(None, v[:1, :k], st[:1, :k])
    assert torch.isfinite(com).all()
    c.generate_com_trajectory_herdt_batch(None, v, st, walk_lengths=nlen)
    lo, hi = c.critical_force_herdt(v[:2, :k], st[:1, :k].expand(2, k), max_dcm_dev=1.0, iters=1)
    assert torch.isfinite(lo).all()
    c.critical_force_herdt(v[:2], st[:2], max_dcm_dev=1.0, iters=1, walk_lengths=nlen[:2])
    m = c.herdt_walk_metrics(hist, foot, st[:1, :k])
    assert torch.isfinite(m.dcm_dev_max).all()


def test_critical_force_with_walk_lengths_equals_single_walks(ragged):
    """critical_force_herdt on the ragged batch against the same call on each walk alone, bracket
    for bracket, on all six walks.  Gaits 3 and 5 already leave the 1 m DCM bound with no push at
    all (their unpushed dcm_dev_max is 1.34 m and 15.9 m, alone as in the batch): their bracket
    is NaN in both, which the ragged call has to reproduce too; the other four compare numbers,
    so more than the three walks asked for do."""
    c, v, st, nlen, nl = ragged
    lo, hi = c.critical_force_herdt(v, st, max_dcm_dev=1.0, walk_lengths=nlen, duration=5,
                                    iters=8)
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    alone = []
    for b, k in enumerate(nl):
        l1, h1 = c.critical_force_herdt(v[b:b + 1, :k], st[b:b + 1, :k], max_dcm_dev=1.0,
                                        duration=5, iters=8)
        alone.append((float(l1[0]), float(h1[0])))
        print(f"walk {b}: bracket [{lo[b]}, {hi[b]}], alone [{alone[-1][0]}, {alone[-1][1]}]")
    alone = np.array(alone)
    finite = np.isfinite(alone[:, 0])
    assert finite.sum() >= 3 and (alone[finite, 1] - alone[finite, 0] == 1000.0 / 2 ** 8).all()
    assert np.array_equal(lo, alone[:, 0], equal_nan=True)
    assert np.array_equal(hi, alone[:, 1], equal_nan=True)


@pytest.mark.parametrize("mode", ("classic", "wieber"))
def test_speed_and_state_batch_equals_each_configuration(mode):
    cfgs = [_cfg(g, speed_generation=mode) for g in GAITS]
    v, st, nlen = SpeedTrajectoryGenerator(cfgs[0]).generate_speed_and_state_batch(cfgs)
    assert tuple(v.shape) == (6, max(COUNTS), 2) and st.dtype == torch.int8
    assert nlen.dtype == torch.int64 and tuple(nlen.cpu().numpy()) == COUNTS
    v, st = v.cpu().numpy(), st.cpu().numpy()
    for b, cfg in enumerate(cfgs):
        vx, vy, states = SpeedTrajectoryGenerator(cfg).generate_speed_and_state(
            save_footsteps=False)
        k = COUNTS[b]
        assert len(states) == k and np.array_equal(st[b, :k], herdt.encode_states(states))
        assert (st[b, k:] == -1).all()
        if mode == "classic":
            assert np.array_equal(v[b, :k, 0], vx) and np.array_equal(v[b, :k, 1], vy)
        else:
            assert np.abs(v[b, :k, 0] - vx).max() <= 1e-12, b
            assert np.abs(v[b, :k, 1] - vy).max() <= 1e-12, b


def test_speed_and_state_batch_refuses_another_dt():
    g = SpeedTrajectoryGenerator(_cfg(speed_generation="classic"))
    with pytest.raises(ValueError, match="dt column"):
        g.generate_speed_and_state_batch([_cfg(GAITS[0]), _cfg(GAITS[1], dt=0.02)])
