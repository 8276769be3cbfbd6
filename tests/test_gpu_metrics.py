"""Device tests of the per-walk robustness metrics (zmpc_walk_metrics, csrc/metrics.hip) against
their NumPy statement (mpc_bipedal.analysis.walk_metrics_reference), and of the critical-push
search built on them (ZMPController.critical_force) against the closed form that the
unconstrained controller's linearity gives."""
import numpy as np
import pytest
import torch

from conftest import golden
from metrics_cases import (B_RANDOM, N_RANDOM, assert_metrics, contraction_safe, random_case)

pytestmark = pytest.mark.gpu

from mpc_bipedal import _native  # noqa: E402
from mpc_bipedal.analysis import (SLOT_NAMES, WalkMetrics, critical_force_affine,  # noqa: E402
                                  walk_metrics_reference)
from mpc_bipedal.config import MPCConfig  # noqa: E402
from mpc_bipedal.controllers import ZMPController  # noqa: E402
from mpc_bipedal.solver import Plan  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    _native.load()


@pytest.fixture(scope="module")
def plan():
    """Any plan serves: the metrics read only its h/g."""
    return Plan(torch.cuda.current_device(), 16, 1.5 / 16, 0.75, 9.81, 1.0, 1e-6, False)


def dev(a, dtype=torch.float64):
    return torch.as_tensor(a, dtype=dtype, device="cuda")


def run(plan, hist, zmax, zmin, lengths=None):
    return plan.walk_metrics(dev(hist), zmax, zmin, lengths=lengths).cpu().numpy()


def ref(plan, hist, zmax, zmin, lengths=None):
    return walk_metrics_reference(hist, zmax, zmin, plan.consts["hg"], lengths)


# --------------------------------------------------------------------------- the kernel


@pytest.mark.parametrize("shared", (False, True), ids=("per_walk", "shared"))
@pytest.mark.parametrize("n", N_RANDOM)
def test_random_history_matches_reference(plan, n, shared):
    """All twelve slots on a random state history: 67 walks (a last workgroup with three of its
    four waves idle), walk lengths below, at and past one and two 64-lane passes."""
    hist, zmax, zmin = random_case(n, shared)
    # precondition of the exact comparison of indices and counts: they do not depend on whether
    # z = c − hg·c̈ is contracted into a fused multiply-add
    assert contraction_safe(hist, zmax, zmin, plan.consts["hg"])
    want = ref(plan, hist, zmax, zmin)
    assert (want[:, 4:6] > 0).any() and (want[:, 4:6] < n).any()  # (boxes left and kept)
    assert_metrics(run(plan, hist, zmax, zmin), want)


def test_ragged_lengths_equal_truncated_walks(plan):
    n = 129
    hist, zmax, zmin = random_case(n, False)
    rng = np.random.default_rng(5)
    lengths = rng.integers(1, n + 1, B_RANDOM)
    lengths[:6] = (1, 2, 64, 65, 128, n)
    for b, nb in enumerate(lengths):  # the dead tail: NaN and 1e300, never read into a result
        hist[b, nb:, 0], hist[b, nb:, 1] = np.nan, 1e300
        zmax[b, nb:], zmin[b, nb:] = 1e300, np.nan
    want = np.concatenate([ref(plan, hist[b:b + 1, :nb], zmax[b:b + 1, :nb], zmin[b:b + 1, :nb])
                           for b, nb in enumerate(lengths)])
    assert np.isfinite(want).all()
    assert_metrics(run(plan, hist, zmax, zmin, lengths), want)
    # one shared CoP with ragged lengths
    hist2, zmax2, zmin2 = random_case(n, True)
    want2 = np.concatenate([ref(plan, hist2[b:b + 1, :nb], zmax2[:nb], zmin2[:nb])
                            for b, nb in enumerate(lengths)])
    assert_metrics(run(plan, hist2, zmax2, zmin2, lengths), want2)


def _quiet_case(n, B):
    """Walks that never leave their boxes."""
    hist, zmax, zmin = random_case(n, False, B=B)
    return hist, zmax + 1.0, zmin - 1.0


def test_planted_extremes_and_ties(plan):
    """The largest violation at the first sample, at the last lane of the first pass, at the
    first lane of the second pass and at the last sample; then the same sample and bounds row
    at two indices (in one lane: 0/64, 64/128; in two lanes: 63/64, 5/70): the lower index wins."""
    n = 129
    spots = [(0,), (63,), (64,), (n - 1,), (0, 64), (64, 128), (63, 64), (5, 70), (128, 1)]
    hist, zmax, zmin = _quiet_case(n, len(spots))
    for b, at in enumerate(spots):
        for i in at:
            hist[b, i] = [[3.0, 0.1, -2.0], [-3.0, 0.2, 2.0]]  # x far above, y far below
            zmax[b, i], zmin[b, i] = zmax[b, at[0]], zmin[b, at[0]]
    got = run(plan, hist, zmax, zmin)
    assert_metrics(got, ref(plan, hist, zmax, zmin))
    for b, at in enumerate(spots):
        assert got[b, 2:4].tolist() == [float(min(at))] * 2, at
        assert got[b, 4:6].tolist() == [float(len(at))] * 2, at
        assert (got[b, 0:2] > 1.0).all()


def test_no_violation(plan):
    hist, zmax, zmin = _quiet_case(65, 9)
    got = run(plan, hist, zmax, zmin)
    assert_metrics(got, ref(plan, hist, zmax, zmin))
    assert (got[:, 0:2] == 0).all() and (got[:, 2:4] == -1).all() and (got[:, 4:6] == 0).all()


def test_nan_injection_fails_safe(plan):
    n = 129
    hist, zmax, zmin = random_case(n, False, B=9)
    clean = ref(plan, hist, zmax, zmin)
    hist[4, 70, 1, 1] = np.nan  # the y velocity of one live sample of one walk
    got = run(plan, hist, zmax, zmin)
    assert got[4, 1] == np.inf and got[4, 3] == 70.0 and np.isnan(got[4, 5::2]).all()
    assert not (got[4, 1] <= 1e-9)
    want = clean.copy()
    want[4, 1::2] = got[4, 1::2]
    assert_metrics(got, want)  # the x axis of that walk and every other walk: as without the NaN
    assert_metrics(got, ref(plan, hist, zmax, zmin))


def test_two_launches_agree_bitwise(plan):
    hist, zmax, zmin = random_case(421, False)
    hist[3, 100, 0, 2] = np.inf
    h, zx, zn = dev(hist), dev(zmax), dev(zmin)
    a = plan.walk_metrics(h, zx, zn)
    b = plan.walk_metrics(h, zx, zn, out=torch.full_like(a, 7.0))
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_offsets_past_2_31(plan):
    """B·n·6 doubles exceed 2³¹: the last walks of a batch of that size, the rest uninitialised."""
    n = 421
    B = 2 ** 31 // (6 * n) + 16
    try:
        hist = torch.empty((B, n, 2, 3), dtype=torch.float64, device="cuda")
    except torch.cuda.OutOfMemoryError:
        pytest.skip(f"no {B * n * 48 / 2 ** 30:.0f} GiB free on the device")
    h, zmax, zmin = random_case(n, True, B=4)
    assert (B - 4) * n * 6 > 2 ** 31
    hist[B - 4:] = dev(h)
    got = plan.walk_metrics(hist, zmax, zmin)[B - 4:].cpu().numpy()
    del hist
    assert_metrics(got, ref(plan, h, zmax, zmin))


def test_sweep_size_batch_sampled_against_reference(walk150):
    """The disturbance sweep's own shape (125 000 scenarios of the 420-sample default walk on
    one shared CoP, 2.5 GB of history): every 997th walk against the NumPy statement."""
    d = walk150
    B = 125000
    c = ZMPController(MPCConfig(horizon=150, strict=False))
    F = np.random.default_rng(4).uniform(0.0, 800.0, B)
    hist, _ = c.generate_state_trajectory_batch(np.zeros((B, 2, 3)), d["zmax"], d["zmin"],
                                                F_ext=F)
    m = c.walk_metrics(hist, d["zmax"], d["zmin"])
    pick = torch.arange(0, B, 997, device="cuda")
    want = walk_metrics_reference(hist[pick].cpu().numpy(), d["zmax"], d["zmin"],
                                  c.config.h / c.config.g)
    del hist
    assert_metrics(m.data[pick].cpu().numpy(), want)
    assert (m.viol_max[:, 1] > 1e-3).all()  # (the nominal excursion, and the push on top)


def test_python_argument_checks(plan):
    hist, zmax, zmin = (dev(a) for a in random_case(5, False, B=3))
    with pytest.raises(ValueError, match="hist must be"):
        plan.walk_metrics(hist.float(), zmax, zmin)
    with pytest.raises(ValueError, match="hist must be"):
        plan.walk_metrics(hist[:, ::2], zmax[:, ::2], zmin[:, ::2])
    with pytest.raises(ValueError, match="hist must be"):
        plan.walk_metrics(hist.cpu(), zmax, zmin)
    with pytest.raises(ValueError, match="z_max must be"):
        plan.walk_metrics(hist, zmax[:2], zmin[:2])
    with pytest.raises(ValueError, match="expected shape"):
        plan.walk_metrics(hist, zmax, zmin[0])
    with pytest.raises(ValueError, match="lengths must be"):
        plan.walk_metrics(hist, zmax, zmin, lengths=[1, 2])
    with pytest.raises(ValueError, match="out must be"):
        plan.walk_metrics(hist, zmax, zmin, out=torch.empty((3, 11), dtype=torch.float64,
                                                            device="cuda"))
    assert tuple(plan.walk_metrics(hist[:0], zmax[:0], zmin[:0]).shape) == (0, 12)


# --------------------------------------------------------------------------- end to end


def test_unconstrained_default_walk_leaves_its_box(walk150):
    """The reference's default unconstrained walk (N = 150), pushed with the default 400 N:
    the device metrics of the device rollout equal the reference function on the reference's own
    state history; and with no push at all the walk already leaves the support box by more
    than a millimetre in y — nothing reported that before the metrics looked."""
    d = walk150
    c = ZMPController(MPCConfig(horizon=150, strict=False, add_force=True))
    hg = c.config.h / c.config.g
    n = len(d["zmax"])
    _, hist = c.generate_com_trajectory_batch(None, d["zmax"], d["zmin"], F_ext=[c.config.F_ext])
    m = c.walk_metrics(hist, d["zmax"], d["zmin"])
    assert isinstance(m, WalkMetrics) and tuple(m.viol_max.shape) == (1, 2)
    gold = hist.cpu().numpy().copy()
    gold[0, :, 1, :] = d["y_hist_force"].reshape(n, 3)
    want = WalkMetrics(walk_metrics_reference(gold, d["zmax"], d["zmin"], hg))
    assert abs(float(m.viol_max[0, 1]) - want.viol_max[0, 1]) <= 1e-9
    assert abs(float(m.zmp_rms[0, 1]) - want.zmp_rms[0, 1]) <= 1e-9
    _, hist0 = c.generate_com_trajectory_batch(None, d["zmax"], d["zmin"])
    m0 = c.walk_metrics(hist0, d["zmax"], d["zmin"])
    assert float(m0.viol_max[0, 1]) > 1e-3 and float(m0.viol_count[0, 1]) > 0


def test_strict_walk_stays_inside_under_push():
    d = golden("walk_n64.npz")
    c = ZMPController(MPCConfig(horizon=64, strict=True, add_force=True))
    _, hist = c.generate_com_trajectory_batch(None, d["zmax"], d["zmin"], F_ext=[400.0])
    m = c.walk_metrics(hist, d["zmax"], d["zmin"])
    print("strict N=64 F=400 viol_max", m.viol_max.cpu().numpy())
    assert float(m.viol_max.max()) <= 1e-9


# --------------------------------------------------------------------------- critical force

F_TOP, ITERS = 1024.0, 30


@pytest.fixture(scope="module")
def push_scenarios():
    """33 pushes of the N = 64 walk (n = 179): 17 steps from the first to the last strides, both
    directions (one dropped)."""
    steps = np.array([5, 20, 33, 44, 52, 60, 71, 80, 89, 97, 104, 112, 120, 131, 140, 150, 160])
    step = np.repeat(steps, 2)[:33]
    sign = np.tile([1.0, -1.0], 17)[:33]
    return step, sign


def test_critical_force_brackets_closed_form(push_scenarios):
    """Unconstrained N = 64: the ZMP is affine in F, so two device rollouts (F = 0 and a unit
    push) give every scenario's critical force in closed form; each bisection bracket must hold
    it, and be F_hi/2^iters wide."""
    step, sign = push_scenarios
    d = golden("walk_n64.npz")
    cfg = MPCConfig(horizon=64, strict=False)
    c = ZMPController(cfg)
    B, tol = len(step), 1e-9
    lo, hi = c.critical_force(d["zmax"], d["zmin"], force_step=step, direction=sign, F_hi=F_TOP,
                              iters=ITERS, max_violation=tol)
    assert lo.is_cuda and hi.is_cuda and tuple(lo.shape) == tuple(hi.shape) == (B,)
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    # closed form from the device's own rollouts
    p = c._plan()
    x0 = np.zeros((B, 2, 3))
    h0, _ = p.rollout(d["zmax"], d["zmin"], x0, kick=np.zeros(B), kick_step=step)
    h1, _ = p.rollout(d["zmax"], d["zmin"], x0, kick=cfg.dt * sign / cfg.m, kick_step=step)
    z0, z1 = c.zmp(h0).cpu().numpy(), c.zmp(h1).cpu().numpy()
    assert np.array_equal(z0[..., 0], z1[..., 0])  # only y is pushed
    fstar = critical_force_affine(z0[..., 1], z1[..., 1] - z0[..., 1], d["zmax"][:, 1],
                                  d["zmin"][:, 1], tol)
    print("F* [N]:", np.round(fstar, 3).tolist())
    assert np.isfinite(fstar).all() and (fstar > 1.0).all() and (fstar < F_TOP).all()
    width = F_TOP / 2 ** ITERS
    assert np.array_equal(hi - lo, np.full(B, width))
    slack = width + 1e-6 * fstar
    assert (lo - slack <= fstar).all() and (fstar <= hi + slack).all(), (lo, hi, fstar)
    assert len(np.unique(np.round(fstar, 3))) > B // 2  # (the scenarios do differ)


def test_critical_force_edge_cases(walk150):
    d150, d64 = walk150, golden("walk_n64.npz")
    # the default N = 150 walk is outside its box with no push: no critical force
    c = ZMPController(MPCConfig(horizon=150, strict=False))
    lo, hi = c.critical_force(d150["zmax"], d150["zmin"], direction=[1.0, -1.0], iters=3)
    assert torch.isnan(lo).all() and torch.isnan(hi).all() and tuple(lo.shape) == (2,)
    # a search limit the walk survives: the bracket closes on it
    c = ZMPController(MPCConfig(horizon=64, strict=False))
    lo, hi = c.critical_force(d64["zmax"], d64["zmin"], force_step=89, F_hi=1.0, iters=5)
    assert lo.tolist() == [1.0] and hi.tolist() == [1.0]
    # further criteria tighten it: a push nine samples before the walk's end moves the final
    # DCM by 6.6e-5 m per newton (affine again, from −2.6e-6 m), long before the ZMP leaves
    lo2, _ = c.critical_force(d64["zmax"], d64["zmin"], force_step=160, iters=12)
    lo3, _ = c.critical_force(d64["zmax"], d64["zmin"], force_step=160, iters=12,
                              max_dcm_end=0.0065)
    assert 400.0 < float(lo2) < 600.0 and 95.0 < float(lo3) < 102.0
    # one no walk meets (the CoM is 0.1 m from the box centre on the nominal walk): NaN
    lo4, _ = c.critical_force(d64["zmax"], d64["zmin"], force_step=160, iters=2,
                              max_com_dev=0.05)
    assert torch.isnan(lo4).all()
    assert SLOT_NAMES[3] == "com_dev_max" and SLOT_NAMES[5] == "dcm_end"
