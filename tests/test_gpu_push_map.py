"""Device tests of the push-robustness map (zmpc_push_map, csrc/pushmap.hip): the full map and
the single-step form against their NumPy statement (mpc_bipedal.analysis.push_map_reference) on
seeded synthetic histories, the response table against analysis.push_response, and
ZMPController.push_map / critical_force_exact against the bisection of critical_force."""
import numpy as np
import pytest
import torch

import push_map_cases as pc

pytestmark = pytest.mark.gpu

from mpc_bipedal import _native  # noqa: E402
from mpc_bipedal.analysis import PushMap, push_map_reference, push_response  # noqa: E402
from mpc_bipedal.config import MPCConfig  # noqa: E402
from mpc_bipedal.controllers import ZMPController  # noqa: E402
from mpc_bipedal.solver import Plan  # noqa: E402
from oracle import zmp_oracle as O  # noqa: E402

MASS = 40.0
PAR150 = (150, 0.01, 0.75, 9.81, 1.0, 1e-6)  # the default walk's plan (walk_n150.npz)
LDS_LIMIT = 10112                            # csrc/dispatch.h kPushMapMaxN


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    _native.load()


@pytest.fixture(scope="module")
def plan():
    return Plan(torch.cuda.current_device(), *PAR150, False)


_R_NP = {}


def numpy_response(n):
    """analysis.push_response of the default plan with the oracle's gain, computed once for the
    longest table and sliced."""
    if "r" not in _R_NP:
        N, dt, h, g, Q, R = PAR150
        A, B, C = O.lipm(dt, h, g)
        _R_NP["r"] = push_response(A, B, O.gain_row(*PAR150)[1], C, dt, MASS, LDS_LIMIT)
    return _R_NP["r"][:n]


def dev(a, dtype=torch.float64):
    return torch.as_tensor(a, dtype=dtype, device="cuda")


def run(plan, hist, zmax, zmin, lengths=None, t=0.0, steps=None):
    f, l, r = plan.push_map(dev(hist), zmax, zmin, lengths=lengths, push_steps=steps,
                            max_violation=t, mass=MASS, want_response=True)
    return f.cpu().numpy(), l.cpu().numpy(), r.cpu().numpy()


def check(got_f, got_l, r_dev, hist, zmax, zmin, lengths, t, what):
    """The comparisons every full-map case takes; prints the measured figures."""
    n = hist.shape[1]
    hg = pc.HG
    want_f, want_l = push_map_reference(hist, zmax, zmin, r_dev, hg, lengths, t)
    # NaN and +inf exactly where the statement has them
    assert np.array_equal(np.isnan(got_f), np.isnan(want_f)), what
    assert np.array_equal(np.isposinf(got_f), np.isposinf(want_f)), what
    fin = np.isfinite(want_f)
    assert (got_l[~fin] == -1).all(), what
    if not fin.any():
        return
    # finite forces: a reciprocal-multiply against a divide
    rel = np.abs(got_f[fin] - want_f[fin]) / np.where(want_f[fin] > 0, want_f[fin], 1.0)
    print(f"{what}: {fin.sum()} finite entries, worst relative error {rel.max():.2e}")
    assert rel.max() <= 1e-12, what
    # the limiting sample, wherever the runner-up is clear of the minimum; the share left out is
    # a property of the reference alone
    gap = pc.runner_up_gap(hist, zmax, zmin, r_dev, hg, lengths, t)
    clear = fin & (gap > 1e-9)
    left_out = fin.sum() - clear.sum()
    print(f"{what}: {left_out} of {fin.sum()} entries within 1e-9 of their runner-up")
    assert left_out <= 0.01 * fin.sum(), what
    assert np.array_equal(got_l[clear], want_l[clear]), what
    i = got_l[fin]
    assert (i > np.nonzero(fin)[1]).all() and (i < n).all(), what
    # the residual of the device's force under the NumPy response
    r_np = numpy_response(n)
    rmax = np.abs(r_np).max() if n > 2 else 0.0
    worst = 0.0
    for b, s, k in zip(*np.nonzero(fin)):
        nb = n if lengths is None else min(max(int(lengths[b]), 1), n)
        z0 = hist[b, :nb, 1, 0] - hg * hist[b, :nb, 1, 2]
        hi = (zmax if zmax.ndim == 2 else zmax[b])[:nb, 1]
        lo = (zmin if zmin.ndim == 2 else zmin[b])[:nb, 1]
        F = got_f[b, s, k]
        g = pc.residual(F, s, 1.0 - 2.0 * k, z0, hi, lo, r_np, t)
        worst = max(worst, abs(g) / max(1.0, F * rmax))
    print(f"{what}: worst |g(F_dev)| / max(1, F·max|r|) = {worst:.2e} m")
    assert worst <= 1e-11, what


# --------------------------------------------------------------------------- the full map

N_SHAPES = (1, 2, 3, 4, 63, 64, 65, 66, 129, 130, 420)


@pytest.mark.parametrize("shared", (False, True), ids=("per_walk", "shared"))
@pytest.mark.parametrize("n", N_SHAPES)
def test_ragged_batch_matches_reference(plan, n, shared):
    """Six walks of 1, 2, 3, 64, 65 and n live samples (clipped to n), garbage and NaN in the dead
    tails; t = 0 with per-walk boxes (margins down to 0), 1 mm with shared ones."""
    lengths = [min(v, n) for v in (1, 2, 3, 64, 65, n)]
    hist, zmax, zmin = pc.synthetic_case(n, shared, 6, lengths=lengths)
    t = 1e-3 if shared else 0.0
    f, l, r = run(plan, hist, zmax, zmin, lengths, t)
    assert f.shape == (6, n, 2) and l.shape == (6, n, 2) and r.shape == (n,)
    check(f, l, r, hist, zmax, zmin, lengths, t, f"n = {n}, shared = {shared}")
    # the same walks with no lengths array: the tails are live and hold NaN, every walk shorter
    # than n is NaN in every entry
    f2, l2, _ = run(plan, hist, zmax, zmin, None, t)
    for b, nb in enumerate(lengths):
        if nb == n:
            assert np.array_equal(f2[b], f[b]) and np.array_equal(l2[b], l[b])
        else:
            assert np.isnan(f2[b]).all() and (l2[b] == -1).all()


def test_several_workgroups_and_a_partial_last_one(plan):
    """259 walks of 130 samples, no lengths array: 259 workgroups of the full map, and 64 full
    workgroups plus one with three walks of the single-step form."""
    n, B = 130, 259
    hist, zmax, zmin = pc.synthetic_case(n, False, B)
    f, l, r = run(plan, hist, zmax, zmin, None, 1e-9)
    check(f, l, r, hist, zmax, zmin, None, 1e-9, f"n = {n}, B = {B}")
    steps = (np.arange(B) * 7) % (n - 2)
    f1, l1, _ = run(plan, hist, zmax, zmin, None, 1e-9, steps=steps)
    assert np.array_equal(f1, f[np.arange(B), steps]) and np.array_equal(l1, l[np.arange(B), steps])


def test_long_walk_n1431(plan):
    n = 1431
    hist, zmax, zmin = pc.synthetic_case(n, False, 2)
    f, l, r = run(plan, hist, zmax, zmin, None, 0.0)
    check(f, l, r, hist, zmax, zmin, None, 0.0, f"n = {n}, B = 2")


def test_lds_limit_and_one_past_it(plan):
    """The longest walk choose_push_map takes (159 KiB of LDS, 16 waves), and its refusal one
    sample further: ZMPC_ESTATE, nothing launched, force untouched."""
    n = LDS_LIMIT
    hist, zmax, zmin = pc.synthetic_case(n, False, 1)
    f, l, r = run(plan, hist, zmax, zmin, None, 0.0)
    check(f, l, r, hist, zmax, zmin, None, 0.0, f"n = {n}, B = 1")
    n += 1
    h = torch.zeros((1, n, 2, 3), dtype=torch.float64, device="cuda")
    b = torch.ones((1, n, 2), dtype=torch.float64, device="cuda")
    force = torch.full((1, n, 2), -7.0, dtype=torch.float64, device="cuda")
    limit = torch.full((1, n, 2), -7, dtype=torch.int32, device="cuda")
    with pytest.raises(_native.NativeError, match="10112 samples"):
        plan.push_map(h, b, -b, mass=MASS, out=(force, limit))
    torch.cuda.synchronize()
    assert (force == -7.0).all() and (limit == -7).all()
    # the single-step form has no such limit
    f1, l1 = plan.push_map(h, b, -b, mass=MASS, push_steps=[5])
    assert np.isfinite(f1.cpu().numpy()).all() and (l1.cpu().numpy() > 5).all()


def test_strict_plan_is_refused_and_force_untouched():
    p = Plan(torch.cuda.current_device(), 16, 1.5 / 16, 0.75, 9.81, 1.0, 1e-6, True)
    n = 20
    h = torch.zeros((2, n, 2, 3), dtype=torch.float64, device="cuda")
    b = torch.ones((n, 2), dtype=torch.float64, device="cuda")
    for steps, shape in ((None, (2, n, 2)), ([3, 4], (2, 2))):
        force = torch.full(shape, -7.0, dtype=torch.float64, device="cuda")
        limit = torch.full(shape, -7, dtype=torch.int32, device="cuda")
        with pytest.raises(_native.NativeError, match="strict") as e:
            p.push_map(h, b, -b, mass=MASS, push_steps=steps, out=(force, limit))
        assert f"({_native.ZMPC_ESTATE})" in str(e.value) and "critical_force" in str(e.value)
        torch.cuda.synchronize()
        assert (force == -7.0).all() and (limit == -7).all()
    c = ZMPController(MPCConfig(horizon=16, strict=True))
    with pytest.raises(RuntimeError, match="strict"):
        c.critical_force_exact(np.ones((n, 2)), -np.ones((n, 2)))
    with pytest.raises(RuntimeError, match="strict"):
        c.push_map(np.ones((n, 2)), -np.ones((n, 2)))


# --------------------------------------------------------------------------- the response table


@pytest.mark.parametrize("name", pc.WALKS)
def test_response_table(name):
    """The device's table at the default weights, N ∈ {64, 10, 150, 512}, over the stored walk's n
    samples: within 1e-10·max|r| of analysis.push_response with the oracle's kx (16 × the 6.4e-12
    the plan's scan tables measure there); r_0 = r_1 = 0 exactly."""
    d, par, kx, r_np, hist, hg = pc.walk(name)
    n = hist.shape[1]
    p = Plan(torch.cuda.current_device(), *par, False)
    _, _, r = p.push_map(dev(hist), d["zmax"], d["zmin"], mass=float(d["m"]),
                         max_violation=1.0, want_response=True)
    r = r.cpu().numpy()
    assert r[0] == 0.0 and r[1] == 0.0
    err = np.abs(r - r_np).max() / np.abs(r_np).max()
    print(f"N = {par[0]}, n = {n}: max|r_dev − r_numpy| / max|r| = {err:.2e}")
    assert err <= 1e-10
    p.destroy()


# --------------------------------------------------------------------------- ties, bounds, order


def test_two_launches_agree_bitwise(plan):
    hist, zmax, zmin = pc.synthetic_case(420, True, 67)
    a = run(plan, hist, zmax, zmin, None, 1e-9)
    b = run(plan, hist, zmax, zmin, None, 1e-9)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x,
                              y.view(np.int64) if y.dtype == np.float64 else y)
    assert np.isfinite(a[0]).any()


def test_on_the_bound_and_constructed_tie(plan):
    """A walk at rest (z0 = 0) in a ±0.1 box, t = 0.  Sample 70 exactly on its upper bound: every
    push that drives it up has F = 0, not NaN.  Then samples 70 and 75 both on the bound: every
    step whose response raises both meets the same candidate 0 twice, and the lower index wins."""
    n = 140
    hist, zmax, zmin = pc.quiet_walk(n)
    zmax[0, 70, 1] = 0.0
    f, l, r = run(plan, hist, zmax, zmin, None, 0.0)
    want_f, want_l = push_map_reference(hist, zmax, zmin, r, pc.HG)
    assert not np.isnan(f).any()
    assert np.array_equal(f == 0.0, want_f == 0.0) and (f == 0.0).sum() >= 10
    assert (l[f == 0.0] == 70).all()
    zmax[0, 75, 1] = 0.0
    f, l, r = run(plan, hist, zmax, zmin, None, 0.0)
    want_f, want_l = push_map_reference(hist, zmax, zmin, r, pc.HG)
    s = np.arange(n)
    both_up = np.zeros((n, 2), bool)  # steps whose push raises the ZMP of samples 70 and 75
    for k, sign in enumerate((1.0, -1.0)):
        ok = s < 69
        both_up[ok, k] = (sign * r[70 - s[ok]] > 0) & (sign * r[75 - s[ok]] > 0)
    assert both_up.sum() >= 10
    assert (f[0][both_up] == 0.0).all() and (l[0][both_up] == 70).all()
    assert np.array_equal(l[f == 0.0], want_l[want_f == 0.0])
    assert np.array_equal(f == 0.0, want_f == 0.0)
    # the single-step form breaks the tie the same way (lanes 6 and 11 of the butterfly)
    steps = np.nonzero(both_up.any(axis=1))[0][:1]
    f1, l1, _ = run(plan, hist, zmax, zmin, None, 0.0, steps=steps)
    assert np.array_equal(f1[0], f[0, steps[0]]) and np.array_equal(l1[0], l[0, steps[0]])


def test_nan_in_a_live_x_sample_fails_the_whole_walk(plan):
    n = 130
    hist, zmax, zmin = pc.synthetic_case(n, False, 3)
    hist[1, 100, 0, 1] = np.nan
    hist[2, 129, 0, 2] = -np.inf
    f, l, r = run(plan, hist, zmax, zmin, None, 0.0)
    assert np.isfinite(f[0, :n - 2]).all()
    assert np.isnan(f[1:]).all() and (l[1:] == -1).all()
    f1, l1, _ = run(plan, hist, zmax, zmin, None, 0.0, steps=[5, 5, 5])
    assert np.array_equal(f1[0], f[0, 5]) and np.isnan(f1[1:]).all() and (l1[1:] == -1).all()
    f, l, _ = run(plan, hist, zmax, zmin, [n, 100, 129], 0.0)
    assert not np.isnan(f).any()


# --------------------------------------------------------------------------- the single-step form


@pytest.mark.parametrize("n", (3, 66, 420))
def test_single_step_equals_rows_of_the_full_map(plan, n):
    """force bit for bit (a minimum does not depend on its order), limit where the full map's is
    unique; steps 0, n_b − 3, n_b − 2 (+inf), −1 and n (outside: +inf and −1)."""
    lengths = [n, max(n - 1, 1), max(n // 2, 1), n, n, n, n]
    B = len(lengths)
    hist, zmax, zmin = pc.synthetic_case(n, False, B, seed=1, lengths=lengths)
    f, l, _ = run(plan, hist, zmax, zmin, lengths, 1e-9)
    steps = np.array([0, lengths[1] - 3, lengths[2] - 2, -1, n, n // 3, n - 3])
    f1, l1, _ = run(plan, hist, zmax, zmin, lengths, 1e-9, steps=steps)
    assert f1.shape == (B, 2) and l1.shape == (B, 2) and l1.dtype == np.int32
    for b, s in enumerate(steps):
        if 0 <= s < lengths[b] - 2:
            assert np.array_equal(f1[b].view(np.int64), f[b, s].view(np.int64)), (b, s)
            assert np.array_equal(l1[b], l[b, s]), (b, s)
            assert np.isfinite(f1[b]).all()
        else:
            assert np.isposinf(f1[b]).all() and (l1[b] == -1).all(), (b, s)


# --------------------------------------------------------------------------- end to end


def test_brackets_of_critical_force_hold_the_exact_value():
    """The 33 scenarios of tests/test_gpu_metrics.py on the N = 64 walk: each bisection bracket of
    the unchanged critical_force, widened by 1e-6 N, holds critical_force_exact's value and the
    map's entry; the pinned numbers; the weakest phase."""
    steps = np.array([5, 20, 33, 44, 52, 60, 71, 80, 89, 97, 104, 112, 120, 131, 140, 150, 160])
    step = np.repeat(steps, 2)[:33]
    sign = np.tile([1.0, -1.0], 17)[:33]
    d = pc.golden("walk_n64.npz")
    c = ZMPController(MPCConfig(horizon=64, strict=False))
    lo, hi = c.critical_force(d["zmax"], d["zmin"], force_step=step, direction=sign, F_hi=1024.0,
                              iters=30, max_violation=1e-9)
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    exact = c.critical_force_exact(d["zmax"], d["zmin"], force_step=step, direction=sign,
                                   max_violation=1e-9)
    assert exact.is_cuda and tuple(exact.shape) == (33,)
    exact = exact.cpu().numpy()
    pm = c.push_map(d["zmax"], d["zmin"], max_violation=1e-9)
    assert isinstance(pm, PushMap) and pm.force.is_cuda and tuple(pm.force.shape) == (1, 179, 2)
    F = pm.force.cpu().numpy()[0]
    entry = F[step, (sign < 0).astype(int)]
    print("bracket:", lo.tolist(), hi.tolist(), "exact:", exact.tolist())
    assert np.isfinite(exact).all()
    assert (lo - 1e-6 <= exact).all() and (exact <= hi + 1e-6).all()
    assert (lo - 1e-6 <= entry).all() and (entry <= hi + 1e-6).all()
    assert np.array_equal(entry, exact)
    assert abs(F[89, 0] - 32.331749) <= 1e-6 and abs(F[89, 1] - 34.058429) <= 1e-6
    assert abs(F[44, 0] - 12.444837) <= 1e-6
    val, s, direction = pm.weakest()
    assert abs(float(val[0]) - 7.608461) <= 1e-6 and int(s[0]) == 62 and int(direction[0]) == -1
    assert np.isposinf(F[177:]).all()
    # defaults as critical_force: step n//2, direction +1, one scenario
    one = c.critical_force_exact(d["zmax"], d["zmin"])
    assert tuple(one.shape) == (1,) and float(one[0]) == F[89, 0]


def test_default_walk_is_nan_from_both(walk150):
    c = ZMPController(MPCConfig(horizon=150, strict=False))
    lo, hi = c.critical_force(walk150["zmax"], walk150["zmin"], direction=[1.0, -1.0], iters=3)
    exact = c.critical_force_exact(walk150["zmax"], walk150["zmin"], direction=[1.0, -1.0])
    assert torch.isnan(lo).all() and torch.isnan(hi).all() and torch.isnan(exact).all()
    pm = c.push_map(walk150["zmax"], walk150["zmin"])
    assert torch.isnan(pm.force).all() and (pm.limit == -1).all()
    pm = c.push_map(walk150["zmax"], walk150["zmin"], max_violation=0.02)
    F = pm.force.cpu().numpy()[0, :418]
    assert np.isfinite(F).all() and abs(F.min() - 60.44) <= 1e-2 and abs(F.max() - 2245.35) <= 1e-2


def test_python_argument_checks(plan):
    h = torch.zeros((2, 10, 2, 3), dtype=torch.float64, device="cuda")
    b = np.ones((10, 2))
    with pytest.raises(ValueError, match="hist"):
        plan.push_map(h.cpu(), b, -b, mass=MASS)
    with pytest.raises(ValueError, match="z_max"):
        plan.push_map(h, np.ones((3, 10, 2)), -np.ones((3, 10, 2)), mass=MASS)
    with pytest.raises(ValueError, match="lengths"):
        plan.push_map(h, b, -b, lengths=[1], mass=MASS)
    with pytest.raises(ValueError, match="push_steps"):
        plan.push_map(h, b, -b, push_steps=[1, 2, 3], mass=MASS)
    with pytest.raises(ValueError, match="max_violation"):
        plan.push_map(h, b, -b, max_violation=-1.0, mass=MASS)
    with pytest.raises(ValueError, match="mass"):
        plan.push_map(h, b, -b, mass=0.0)
    with pytest.raises(ValueError, match="out"):
        plan.push_map(h, b, -b, mass=MASS, out=(torch.empty((2, 10, 2), device="cuda"),
                                                 torch.empty((2, 10, 2), device="cuda")))
    with pytest.raises(TypeError):
        plan.push_map(h, b, -b)  # the plan does not hold the mass
