"""Device tests of the fused rollout-to-metrics launch (zmpc_rollout_metrics, csrc/rollout.hip
split_walk with MET; Plan.rollout_metrics, ZMPController.generate_walk_metrics_batch and
critical_force(fused=True)).

Two expectations.  A (independent): mpc_bipedal.analysis.walk_metrics_reference (NumPy) on the
oracle's rollout_gain history of the same inputs.  B (device): Plan.rollout followed by
Plan.walk_metrics.  Value slots (viol_max, com_dev_max, zmp_rms, dcm_end) must agree to 1e-11
absolute, the bar include/zmpc.h holds equivalent forms to on O(1) states.  The fused states may
differ from the history kernel's in the last bits, so the discrete slots (viol_argmax, viol_count)
get a bracket of EPS = 1e-11 on the violation — and every test first asserts, on expectation A
alone, that for every walk of its inputs the bracket has zero width (no sample within EPS of a
bound, the largest violation more than 2·EPS ahead of the runner-up at another sample, or 0).  The
comparison of the discrete slots is then exact."""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

from mpc_bipedal import _native  # noqa: E402
from mpc_bipedal.analysis import (WalkMetrics, critical_force_affine,  # noqa: E402
                                  walk_metrics_reference)
from mpc_bipedal.config import MPCConfig  # noqa: E402
from mpc_bipedal.controllers import ZMPController  # noqa: E402
from mpc_bipedal.solver import Plan  # noqa: E402
from oracle import zmp_oracle as O  # noqa: E402

EPS = 1e-11
H, G, Q, R = 0.75, 9.81, 1.0, 1e-6
HG = H / G
# CW = 1..8, both sides of every change of CW, a last lane with one live step
N_CW = (2, 3, 65, 66, 129, 193, 257, 321, 385, 421, 449, 513)
VALUE_SLOTS = (0, 1, 6, 7, 8, 9, 10, 11)
DISCRETE_SLOTS = (2, 3, 4, 5)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    _native.load()


_PLANS = {}


def plan_of(N):
    """Non-strict plan of horizon N over 1.5 s (dt = 0.01 at N = 150, the default walk's)."""
    if N not in _PLANS:
        _PLANS[N] = Plan(torch.cuda.current_device(), N, 1.5 / N, H, G, Q, R, False)
    return _PLANS[N]


def dev(a, dtype=torch.float64):
    return torch.as_tensor(a, dtype=dtype, device="cuda")


# --------------------------------------------------------------------------- inputs, expectations


def cop_case(n, B, seed, shared=False):
    """Piecewise-constant CoP boxes (a stair in x, alternating sides in y, 23 samples per support
    phase) of per-walk stride, sway and half widths from 4 mm to 6 cm, so that some walks leave
    their boxes and some stay; initial states and pushes that differ per walk.
    → zmax, zmin [B,n,2] (shared: [n,2]), x0 [B,2,3], kick [B]."""
    rng = np.random.default_rng([20261020, seed, n, int(shared)])
    Bc = 1 if shared else B
    nph = n // 23 + 1
    stride = rng.uniform(0.0, 0.06, (Bc, 1))
    sway = rng.uniform(0.0, 0.07, (Bc, 1))
    cx = np.cumsum(stride * rng.uniform(0.5, 1.0, (Bc, nph)), axis=1)
    cy = sway * (-1.0) ** np.arange(nph) + rng.uniform(-0.005, 0.005, (Bc, nph))
    centre = np.repeat(np.stack([cx, cy], axis=-1), 23, axis=1)[:, :n]
    centre = centre + rng.uniform(-0.02, 0.02, (Bc, 1, 2))
    half = np.repeat(rng.uniform(0.004, 0.06, (Bc, nph, 2)), 23, axis=1)[:, :n]
    zmax, zmin = centre + half, centre - half
    if shared:
        zmax, zmin = zmax[0], zmin[0]
    x0 = rng.uniform(-1.0, 1.0, (B, 2, 3)) * np.array([0.02, 0.05, 0.1])
    kick = rng.uniform(-0.1, 0.1, B)  # dt·F/m of up to ±400 N at dt = 0.01, m = 40
    return zmax, zmin, x0, kick


def oracle_hist(N, zmax, zmin, x0, kick, kick_step):
    """Expectation A's history: the oracle's gain-form rollout; kick_step an int or a [B] array."""
    B = len(x0)
    zx = np.broadcast_to(zmax, (B,) + zmax.shape[-2:])
    zn = np.broadcast_to(zmin, (B,) + zmin.shape[-2:])
    dt = 1.5 / N
    if np.ndim(kick_step) == 0:
        return O.rollout_gain(zx, zn, x0, N, dt, H, G, Q, R, kick, int(kick_step))
    hist = np.empty((B, zx.shape[1], 2, 3))
    steps = np.asarray(kick_step)
    for s in np.unique(steps):
        w = steps == s
        hist[w] = O.rollout_gain(zx[w], zn[w], x0[w], N, dt, H, G, Q, R,
                                 None if kick is None else kick[w], int(s))
    return hist


def assert_sharp(hist, zmax, zmin, lengths=None):
    """The precondition of the exact comparison, on the expectation alone: every walk's bracket
    of the discrete slots has zero width."""
    B, n = hist.shape[:2]
    for b in range(B):
        nb = n if lengths is None else int(lengths[b])
        hi = (zmax if zmax.ndim == 2 else zmax[b])[:nb]
        lo = (zmin if zmin.ndim == 2 else zmin[b])[:nb]
        for a in range(2):
            s = hist[b, :nb, a]
            if not np.isfinite(s).all():
                continue
            z = s[:, 0] - HG * s[:, 2]
            raw = np.maximum(z - hi[:, a], lo[:, a] - z)
            assert np.count_nonzero(raw > EPS) == np.count_nonzero(raw > -EPS), (b, a)
            v = np.sort(np.maximum(raw, 0.0))
            assert v[-1] == 0.0 or nb == 1 or v[-1] - v[-2] > 2 * EPS, (b, a, v[-2:])


def assert_fused(got, want, what=""):
    """Value slots to 1e-11 absolute (inf and NaN where the expectation has them), discrete slots
    exactly (zero-width brackets, assert_sharp)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    fin = np.isfinite(want[:, VALUE_SLOTS]) & np.isfinite(got[:, VALUE_SLOTS])
    err = np.abs(np.where(fin, got[:, VALUE_SLOTS], 0.0) -
                 np.where(fin, want[:, VALUE_SLOTS], 0.0)).max(initial=0.0)
    print(f"{what}: largest value-slot difference {err:.3e}")
    for s in DISCRETE_SLOTS:
        np.testing.assert_array_equal(got[:, s], want[:, s], err_msg=f"{what} slot {s}")
    for s in VALUE_SLOTS:
        np.testing.assert_allclose(got[:, s], want[:, s], rtol=0, atol=EPS,
                                   err_msg=f"{what} slot {s}")


def two_launch(plan, zmax, zmin, x0, kick, kick_step, lengths=None):
    """Expectation B: the history launch and the metrics launch."""
    hist, st = plan.rollout(zmax, zmin, x0, kick=kick, kick_step=kick_step)
    return plan.walk_metrics(hist, zmax, zmin, lengths=lengths).cpu().numpy(), st.cpu().numpy()


def fused(plan, zmax, zmin, x0, kick, kick_step, lengths=None):
    m, st = plan.rollout_metrics(zmax, zmin, x0, kick=kick, kick_step=kick_step, lengths=lengths,
                                 fused_only=True)
    return m.cpu().numpy(), st.cpu().numpy()


_EXPECT = {}


def expect_a(N, n, B, seed, shared=False):
    """(inputs, expectation A), computed once per shape; no test writes to them."""
    key = (N, n, B, seed, shared)
    if key not in _EXPECT:
        zmax, zmin, x0, kick = cop_case(n, B, seed, shared)
        hist = oracle_hist(N, zmax, zmin, x0, kick, n // 2)
        assert_sharp(hist, zmax, zmin)
        want = walk_metrics_reference(hist, zmax, zmin, HG)
        _EXPECT[key] = (zmax, zmin, x0, kick, want)
    return _EXPECT[key]


# --------------------------------------------------------------------------- the kernel


@pytest.mark.parametrize("corr", (0, 1), ids=("sparse_first", "dense"))
@pytest.mark.parametrize("n", N_CW)
@pytest.mark.parametrize("N", (10, 64, 150))
def test_every_chunk_width(N, n, corr):
    """Per-walk bounds, 67 walks, every chunk width CW = 1..8, both correlation forms."""
    zmax, zmin, x0, kick, want = expect_a(N, n, 67, 1)
    if n >= 65:
        assert (want[:, 4:6] > 0).any() and (want[:, 4:6] == 0).any()  # boxes left and kept
    plan = plan_of(N)
    plan.set_option("correlation", corr)
    try:
        got, st = fused(plan, zmax, zmin, x0, kick, n // 2)
        assert_fused(got, want, f"N={N} n={n} vs oracle")
        wb, stb = two_launch(plan, zmax, zmin, x0, kick, n // 2)
    finally:
        plan.set_option("correlation", 0)
    assert_fused(got, wb, f"N={N} n={n} vs two launches")
    assert np.array_equal(st, stb) and not st.any()


@pytest.mark.parametrize("n", N_CW)
def test_shared_cop(n):
    """One CoP for 130 walks (stride 0) whose initial states and pushes differ; also against the
    per-walk form of the same CoP, replicated."""
    N, B = 150, 130
    zmax, zmin, x0, kick, want = expect_a(N, n, B, 2, shared=True)
    plan = plan_of(N)
    got, st = fused(plan, zmax, zmin, x0, kick, n // 2)
    assert_fused(got, want, f"shared n={n} vs oracle")
    wb, stb = two_launch(plan, zmax, zmin, x0, kick, n // 2)
    assert_fused(got, wb, f"shared n={n} vs two launches")
    rep, _ = fused(plan, np.repeat(zmax[None], B, 0), np.repeat(zmin[None], B, 0), x0, kick, n // 2)
    assert_fused(got, rep, f"shared n={n} vs per-walk form")
    assert np.array_equal(st, stb) and not st.any()


KICK_STEPS = (0, 6, 7, 210, 419, 420, -1, 1000)  # CW = 7: a lane's last and first step, ...


def _kick_case():
    n, N = 421, 150
    zmax, zmin, x0, _ = cop_case(n, 16, 3)
    steps = np.repeat(KICK_STEPS, 2)
    kick = np.tile([0.5, -0.5], 8) * np.linspace(1.0, 1.4, 16)  # ±2000..2800 N: y leaves its box
    return n, N, zmax, zmin, x0, kick, steps


@pytest.mark.parametrize("step", KICK_STEPS)
def test_kick_placement_scalar_step(step):
    n, N, zmax, zmin, x0, kick, _ = _kick_case()
    hist = oracle_hist(N, zmax, zmin, x0, kick, step)
    assert_sharp(hist, zmax, zmin)
    want = walk_metrics_reference(hist, zmax, zmin, HG)
    plan = plan_of(N)
    got, _ = fused(plan, zmax, zmin, x0, kick, step)
    assert_fused(got, want, f"kick step {step} vs oracle")
    assert_fused(got, two_launch(plan, zmax, zmin, x0, kick, step)[0], f"kick step {step}")
    quiet = walk_metrics_reference(oracle_hist(N, zmax, zmin, x0, None, -1), zmax, zmin, HG)
    if 0 <= step <= 210:
        assert (want[:, 1] > quiet[:, 1] + 0.01).all()  # the push drove y out of its box
    elif step == 419:  # the last step: only the final velocity, so only dcm_end, sees the push
        assert np.array_equal(want[:, :10], quiet[:, :10])
        assert (np.abs(want[:, 11] - quiet[:, 11]) > 0.1).all()
    else:
        assert np.array_equal(want, quiet)  # a step outside [0, n − 1): no push
    if step == 0:
        assert (want[:, 3] >= 1).all()


def test_kick_placement_per_walk_steps():
    n, N, zmax, zmin, x0, kick, steps = _kick_case()
    hist = oracle_hist(N, zmax, zmin, x0, kick, steps)
    assert_sharp(hist, zmax, zmin)
    want = walk_metrics_reference(hist, zmax, zmin, HG)
    plan = plan_of(N)
    got, _ = fused(plan, zmax, zmin, x0, kick, steps)
    assert_fused(got, want, "per-walk kick steps vs oracle")
    assert_fused(got, two_launch(plan, zmax, zmin, x0, kick, steps)[0], "per-walk kick steps")


def test_ragged_lengths():
    """Live lengths below, at and past a lane's chunk (CW = 7) and the wave, 0 and 500 clamped to
    1 and n; dcm_end from sample n_b − 1; violations that exist only past n_b are not counted."""
    n, N = 421, 150
    lengths = np.array([1, 2, 7, 8, 64, 65, 420, 421, 0, 500] * 2)
    B = len(lengths)
    live = np.clip(lengths, 1, n)
    zmax, zmin, x0, kick = cop_case(n, B, 4)
    zmax, zmin = zmax.copy(), zmin.copy()
    centre = (zmax + zmin) / 2
    for b in range(10):  # the same z_ref, wide boxes on the live rows and hair-thin ones past n_b
        half = np.where(np.arange(n) < live[b], 0.7, 1e-4)[:, None]
        zmax[b], zmin[b] = centre[b] + half, centre[b] - half
    hist = oracle_hist(N, zmax, zmin, x0, kick, n // 2)
    assert_sharp(hist, zmax, zmin, live)
    want = walk_metrics_reference(hist, zmax, zmin, HG, live)
    full = walk_metrics_reference(hist, zmax, zmin, HG)
    assert (want[:10, 4:6] == 0).all() and (full[:7, 4:6] > 0).all()  # only the dead rows violate
    plan = plan_of(N)
    got, st = fused(plan, zmax, zmin, x0, kick, n // 2, lengths)
    assert_fused(got, want, "ragged vs oracle")
    for b in range(B):
        s = hist[b, live[b] - 1]
        zr = (zmax[b, live[b] - 1] + zmin[b, live[b] - 1]) * 0.5
        assert np.abs(got[b, 10:12] - (s[:, 0] + s[:, 1] * np.sqrt(HG) - zr)).max() <= EPS, b
    wb, stb = two_launch(plan, zmax, zmin, x0, kick, n // 2, lengths)
    assert_fused(got, wb, "ragged vs two launches")
    assert np.array_equal(st, stb)
    # shared CoP with the same lengths
    zs, zn, x0s, ks = cop_case(n, B, 5, shared=True)
    hs = oracle_hist(N, zs, zn, x0s, ks, n // 2)
    assert_sharp(hs, zs, zn, live)
    got2, _ = fused(plan, zs, zn, x0s, ks, n // 2, lengths)
    assert_fused(got2, walk_metrics_reference(hs, zs, zn, HG, live), "ragged shared vs oracle")


@pytest.mark.parametrize("shared", (False, True), ids=("per_walk", "shared"))
def test_single_sample_walk(shared):
    """n = 1: the metrics of x0 alone, status 0."""
    zmax, zmin, x0, kick = cop_case(1, 67, 6, shared)
    hist = x0[:, None]
    assert_sharp(hist, zmax, zmin)
    want = walk_metrics_reference(hist, zmax, zmin, HG)
    plan = plan_of(64)
    got, st = fused(plan, zmax, zmin, x0, kick, 0)
    assert_fused(got, want, "n=1 vs NumPy")
    assert_fused(got, two_launch(plan, zmax, zmin, x0, kick, 0)[0], "n=1 vs two launches")
    assert not st.any()


def test_non_finite_fails_safe():
    """NaN in one walk's x-axis initial state, an infinite push of another walk at step 100: that
    axis reports (+inf, first bad sample, NaN ...) and the walk's status has ZMPC_ST_NONFINITE; the
    other axis and every other walk are bitwise as in a launch without them."""
    n, N, B = 421, 150, 9
    zmax, zmin, x0, kick = cop_case(n, B, 7)
    plan = plan_of(N)
    clean, st0 = fused(plan, zmax, zmin, x0, kick, 100)
    assert not st0.any() and np.isfinite(clean).all()
    x0b, kickb = x0.copy(), kick.copy()
    x0b[2, 0, 1] = np.nan
    kickb[5] = np.inf
    got, st = fused(plan, zmax, zmin, x0b, kickb, 100)
    for b, a, first in ((2, 0, 0.0), (5, 1, 101.0)):
        assert got[b, a] == np.inf and got[b, 2 + a] == first, (b, got[b])
        assert np.isnan(got[b, 4 + a::2]).all() and not (got[b, a] <= 1e-9)
        assert st[b] & _native.ST_NONFINITE
    same = np.ones((B, 12), bool)
    same[2, 0::2] = same[5, 1::2] = False
    assert np.array_equal(got.view(np.int64)[same], clean.view(np.int64)[same])
    assert not np.delete(st, (2, 5)).any()
    wb, stb = two_launch(plan, zmax, zmin, x0b, kickb, 100)
    assert_fused(got, wb, "non-finite vs two launches")
    assert np.array_equal(st, stb)


def test_two_launches_agree_bitwise():
    n, N = 421, 150
    plan = plan_of(N)
    for shared in (False, True):
        zmax, zmin, x0, kick = cop_case(n, 130, 8, shared)
        zx, zn, x, k = dev(zmax), dev(zmin), dev(x0), dev(kick)
        a, _ = plan.rollout_metrics(zx, zn, x, kick=k, kick_step=n // 2, fused_only=True)
        b, _ = plan.rollout_metrics(zx, zn, x, kick=k, kick_step=n // 2, fused_only=True,
                                    out=torch.full_like(a, 7.0))
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_refusals_and_fallback():
    """A strict plan and a walk of 514 samples have no fused form: fused_only=True raises and
    leaves `out` as it was; without the flag the method returns the two-launch result."""
    dt = 1.5 / 16
    strict = Plan(torch.cuda.current_device(), 16, dt, H, G, Q, R, True)
    loose = Plan(torch.cuda.current_device(), 16, dt, H, G, Q, R, False)
    for plan, n, word in ((strict, 65, "strict"), (loose, 514, "513 samples")):
        zmax, zmin, x0, kick = cop_case(n, 5, 9)
        zmax, zmin = zmax + 0.2, zmin - 0.2  # (room for the strict solver)
        out = torch.full((5, 12), 7.0, dtype=torch.float64, device="cuda")
        with pytest.raises(_native.NativeError, match=word):
            plan.rollout_metrics(zmax, zmin, x0, kick=kick, kick_step=n // 2, out=out,
                                 fused_only=True)
        torch.cuda.synchronize()
        assert (out == 7.0).all()
        m, st = plan.rollout_metrics(zmax, zmin, x0, kick=kick, kick_step=n // 2, out=out)
        assert m is out
        hist, st2 = plan.rollout(zmax, zmin, x0, kick=kick, kick_step=n // 2)
        want = plan.walk_metrics(hist, zmax, zmin)
        assert torch.equal(m.view(torch.int64), want.view(torch.int64)) and torch.equal(st, st2)
    # the one-wave cross-check kernel has no fused form either
    zmax, zmin, x0, kick = cop_case(65, 5, 9)
    loose.set_option("rollout_kernel", 1)
    try:
        with pytest.raises(_native.NativeError, match="one-wave"):
            loose.rollout_metrics(zmax, zmin, x0, fused_only=True)
    finally:
        loose.set_option("rollout_kernel", 0)


def test_python_argument_checks():
    plan = plan_of(64)
    zmax, zmin, x0, kick = cop_case(5, 3, 10)
    with pytest.raises(ValueError, match="x0 must be"):
        plan.rollout_metrics(zmax, zmin, x0[:, 0])
    with pytest.raises(ValueError, match="z_max must be"):
        plan.rollout_metrics(zmax[:2], zmin[:2], x0)
    with pytest.raises(ValueError, match="lengths must be"):
        plan.rollout_metrics(zmax, zmin, x0, lengths=[1, 2])
    with pytest.raises(ValueError, match="kick_step must be"):
        plan.rollout_metrics(zmax, zmin, x0, kick=kick, kick_step=[1, 2])
    with pytest.raises(ValueError, match="out must be"):
        plan.rollout_metrics(zmax, zmin, x0, out=torch.empty((3, 11), dtype=torch.float64,
                                                              device="cuda"))
    m, st = plan.rollout_metrics(zmax[:0], zmin[:0], x0[:0], fused_only=True)
    assert tuple(m.shape) == (0, 12) and tuple(st.shape) == (0,)


# --------------------------------------------------------------------------- end to end


@pytest.mark.parametrize("horizon", (64, 150))
def test_reference_fixture(horizon):
    """The reference's default walks, unpushed and with the default 400 N: the fused metrics
    against the NumPy metrics of the fixture's stored state history, and the findings of
    DESIGN.md §4.6."""
    d = golden(f"walk_n{horizon}.npz")
    n = len(d["zmax"])
    c = ZMPController(MPCConfig(horizon=horizon, strict=False))
    hg = c.config.h / c.config.g
    stored = np.empty((2, n, 2, 3))
    stored[:, :, 0] = d["state_x_hist"].reshape(n, 3)  # (only y is pushed)
    stored[0, :, 1] = d["state_y_hist"].reshape(n, 3)
    stored[1, :, 1] = d["y_hist_force"].reshape(n, 3)
    assert np.array_equal(d["state_y_hist"], d["y_hist_noforce"])
    assert_sharp(stored, d["zmax"], d["zmin"])
    want = walk_metrics_reference(stored, d["zmax"], d["zmin"], hg)
    m, st = c.generate_walk_metrics_batch(np.zeros((2, 2, 3)), d["zmax"], d["zmin"],
                                          F_ext=[0.0, float(d["F_ext"])])
    assert isinstance(m, WalkMetrics) and tuple(m.viol_max.shape) == (2, 2) and not st.any()
    got = m.data.cpu().numpy()
    print(f"N={horizon} fused metrics:\n{got}")
    assert_fused(got, want, f"fixture N={horizon}")
    if horizon == 150:
        # unpushed: out of its box by 0.9 mm in x (one sample, 180) and 13.3 mm in y (16 samples)
        assert abs(got[0, 0] - 0.9e-3) < 0.05e-3 and abs(got[0, 1] - 13.3e-3) < 0.05e-3
        assert got[0, 2:6].tolist() == [180.0, 126.0, 1.0, 16.0]
    else:
        assert got[0, 0:4].tolist() == [0.0, 0.0, -1.0, -1.0] and got[0, 4:6].tolist() == [0.0, 0.0]


F_TOP, ITERS = 1024.0, 30


def test_critical_force_fused():
    """The 33-scenario search of tests/test_gpu_metrics.py through the fused launch: every bracket
    holds the closed form and is F_hi/2^iters wide."""
    steps = np.array([5, 20, 33, 44, 52, 60, 71, 80, 89, 97, 104, 112, 120, 131, 140, 150, 160])
    step, sign = np.repeat(steps, 2)[:33], np.tile([1.0, -1.0], 17)[:33]
    d = golden("walk_n64.npz")
    cfg = MPCConfig(horizon=64, strict=False)
    c = ZMPController(cfg)
    B, tol = len(step), 1e-9
    kw = dict(force_step=step, direction=sign, F_hi=F_TOP, iters=ITERS, max_violation=tol)
    lo, hi = c.critical_force(d["zmax"], d["zmin"], fused=True, **kw)
    assert lo.is_cuda and hi.is_cuda and tuple(lo.shape) == tuple(hi.shape) == (B,)
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    p = c._plan()
    x0 = np.zeros((B, 2, 3))
    h0, _ = p.rollout(d["zmax"], d["zmin"], x0, kick=np.zeros(B), kick_step=step)
    h1, _ = p.rollout(d["zmax"], d["zmin"], x0, kick=cfg.dt * sign / cfg.m, kick_step=step)
    z0, z1 = c.zmp(h0).cpu().numpy(), c.zmp(h1).cpu().numpy()
    fstar = critical_force_affine(z0[..., 1], z1[..., 1] - z0[..., 1], d["zmax"][:, 1],
                                  d["zmin"][:, 1], tol)
    assert np.isfinite(fstar).all() and (fstar > 1.0).all() and (fstar < F_TOP).all()
    width = F_TOP / 2 ** ITERS
    assert np.array_equal(hi - lo, np.full(B, width))
    slack = width + 1e-6 * fstar
    assert (lo - slack <= fstar).all() and (fstar <= hi + slack).all(), (lo, hi, fstar)
    lo2, hi2 = c.critical_force(d["zmax"], d["zmin"], **kw)
    differ = int(np.count_nonzero((lo2.cpu().numpy() != lo) | (hi2.cpu().numpy() != hi)))
    print(f"brackets that differ between fused=True and fused=False: {differ} of {B}")


def test_critical_force_fused_edge_cases_and_memory(walk150):
    # the default N = 150 walk is outside its box with no push: no critical force
    c = ZMPController(MPCConfig(horizon=150, strict=False))
    lo, hi = c.critical_force(walk150["zmax"], walk150["zmin"], direction=[1.0, -1.0], iters=3,
                              fused=True)
    assert torch.isnan(lo).all() and torch.isnan(hi).all() and tuple(lo.shape) == (2,)
    # 4096 scenarios: no tensor of B·n·6 doubles is allocated during the call
    d = golden("walk_n64.npz")
    n, B = len(d["zmax"]), 4096
    c = ZMPController(MPCConfig(horizon=64, strict=False))
    rng = np.random.default_rng(11)
    step, sign = rng.integers(5, 161, B), rng.choice([-1.0, 1.0], B)
    zmax, zmin = dev(d["zmax"]), dev(d["zmin"])
    c.critical_force(zmax, zmin, force_step=step[:8], direction=sign[:8], iters=1, fused=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    lo, hi = c.critical_force(zmax, zmin, force_step=step, direction=sign, iters=8, fused=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"critical_force(fused=True), B={B}, n={n}: peak {peak} B above the inputs; a history "
          f"would be {B * n * 48} B")
    assert peak < 2 * B * n * 2 * 8 < B * n * 6 * 8
    assert torch.isfinite(lo).all() and (hi - lo == 1000.0 / 2 ** 8).all()
