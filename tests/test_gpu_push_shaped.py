"""Device tests of sustained, shaped and two-axis pushes (zmpc_push_map_shaped,
csrc/pushmap.hip): bitwise anchors against zmpc_push_map and among its own forms, the shaped
table against analysis.shaped_response, the map against its NumPy statement
(analysis.push_map_shaped_reference) on seeded synthetic histories, the edge cases, and the
critical pushes of the stored N = 64 walk bracketed by pushed rollouts on the device."""
import ctypes

import numpy as np
import pytest
import torch

import push_map_cases as pc
import push_shaped_cases as ps

pytestmark = pytest.mark.gpu

from mpc_bipedal import _native  # noqa: E402
from mpc_bipedal.analysis import (AXES, PushMap, push_map_shaped_reference,  # noqa: E402
                                  shaped_response)
from mpc_bipedal.config import MPCConfig  # noqa: E402
from mpc_bipedal.controllers import ZMPController  # noqa: E402
from mpc_bipedal.solver import Plan  # noqa: E402

MASS = 40.0
PAR150 = (150, 0.01, 0.75, 9.81, 1.0, 1e-6)  # the default walk's plan (walk_n150.npz)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    _native.load()


@pytest.fixture(scope="module")
def plan():
    return Plan(torch.cuda.current_device(), *PAR150, False)


def dev(a, dtype=torch.float64):
    return torch.as_tensor(a, dtype=dtype, device="cuda").contiguous()


def bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def run(plan, hist, zmax, zmin, lengths=None, t=0.0, steps=None, D=1, w=None, axes="y"):
    """One zmpc_push_map_shaped call, straight through ctypes (Plan.push_map sends the default
    arguments to zmpc_push_map) → force, limit, response on the host."""
    B, n = hist.shape[:2]
    h, zx, zn = dev(hist), dev(zmax), dev(zmin)
    C = 4 if axes == "xy" else 2
    shape = (B, n, C) if steps is None else (B, C)
    force = torch.full(shape, -7.0, dtype=torch.float64, device="cuda")
    limit = torch.full(shape, -7, dtype=torch.int32, device="cuda")
    resp = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    len_t = None if lengths is None else dev(lengths, torch.int64)
    st_t = None if steps is None else dev(steps, torch.int64)
    w_t = None if w is None else dev(w)
    vp = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())  # noqa: E731
    rc = _native.load().zmpc_push_map_shaped(
        plan.handle, B, n, vp(h), vp(zx), vp(zn), 0 if np.ndim(zmax) == 2 else 2 * n, vp(len_t),
        vp(st_t), vp(w_t), D, AXES[axes], t, MASS, vp(force), vp(limit), vp(resp),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, "zmpc_push_map_shaped")
    torch.cuda.synchronize()
    return force.cpu().numpy(), limit.cpu().numpy(), resp.cpu().numpy()


def base_table(plan, n):
    """The device's one-sample response r_0 .. r_(n−1) (zmpc_push_map on one resting walk)."""
    h = torch.zeros((1, n, 2, 3), dtype=torch.float64, device="cuda")
    b = torch.ones((n, 2), dtype=torch.float64, device="cuda")
    return plan.push_map(h, b, -b, mass=MASS, push_steps=[0], want_response=True)[2].cpu().numpy()


# --------------------------------------------------------------------------- bitwise anchors


@pytest.mark.parametrize("n", (3, 66, 420))
def test_bitwise_anchors(plan, n):
    """axes = y, D = 1, no profile: zmpc_push_map's force, limit and response bit for bit.  An
    "xy" launch equals the "x" and "y" launches column for column, the single-step form equals
    the map's rows, and two launches agree — ragged lengths, shaped and unshaped."""
    lengths = [n, max(n - 1, 1), max(n // 2, 1), n, max(n - 7, 1), 2, 1]
    B = len(lengths)
    hist, zmax, zmin = pc.synthetic_case(n, False, B, seed=1, lengths=lengths)
    f0, l0, r0 = plan.push_map(dev(hist), zmax, zmin, lengths=lengths, max_violation=1e-9,
                               mass=MASS, want_response=True)
    f, l, r = run(plan, hist, zmax, zmin, lengths, 1e-9)
    assert same_bits(f, f0.cpu().numpy()) and same_bits(l, l0.cpu().numpy())
    assert same_bits(r, r0.cpu().numpy())
    steps = np.array([0, lengths[1] - 3, lengths[2] - 2, -1, n, n // 3, 0])
    for D, w in ((1, None), (5, ps.half_sine(5)), (n + 3, None)):
        fx, lx, rx = run(plan, hist, zmax, zmin, lengths, 1e-9, D=D, w=w, axes="x")
        fy, ly, ry = run(plan, hist, zmax, zmin, lengths, 1e-9, D=D, w=w, axes="y")
        f4, l4, r4 = run(plan, hist, zmax, zmin, lengths, 1e-9, D=D, w=w, axes="xy")
        assert f4.shape == (B, n, 4) and l4.dtype == np.int32
        assert same_bits(f4, np.concatenate([fx, fy], axis=2))
        assert same_bits(l4, np.concatenate([lx, ly], axis=2))
        assert same_bits(rx, ry) and same_bits(rx, r4)
        # the x columns are the y columns of the axis-swapped walks
        fs, ls, _ = run(plan, *ps.swap_axes(hist, zmax, zmin), lengths, 1e-9, D=D, w=w, axes="y")
        assert same_bits(fs, fx) and same_bits(ls, lx)
        again = run(plan, hist, zmax, zmin, lengths, 1e-9, D=D, w=w, axes="xy")
        assert all(same_bits(a, b) for a, b in zip(again, (f4, l4, r4)))
        for axes, full_f, full_l in (("x", fx, lx), ("y", fy, ly), ("xy", f4, l4)):
            f1, l1, _ = run(plan, hist, zmax, zmin, lengths, 1e-9, steps=steps, D=D, w=w, axes=axes)
            assert f1.shape == (B, full_f.shape[2])
            for b, s in enumerate(steps):
                if 0 <= s < lengths[b] - 2:
                    assert same_bits(f1[b], full_f[b, s]) and same_bits(l1[b], full_l[b, s]), (b, s)
                else:
                    assert np.isposinf(f1[b]).all() and (l1[b] == -1).all(), (b, s)
    if n > 3:
        assert np.isfinite(f4).any() and not np.array_equal(fx, fy)


# --------------------------------------------------------------------------- the shaped table


@pytest.mark.parametrize("n", (2, 66, 130, 420, 1431))
def test_shaped_table(plan, n):
    """`response` against shaped_response of the device's own one-sample table.  Per delay the
    bound is 2·(D + 1)·2⁻⁵³·Σ_j |w_j·r_(d−j)|: twice the standard bound of a D-term sum of rounded
    products, which holds for any order (derived, not measured).  D = 1 without a profile copies
    the table."""
    r = base_table(plan, n)
    assert r.shape == (n,) and r[0] == 0.0 and (n < 2 or r[1] == 0.0)
    hist, zmax, zmin = pc.quiet_walk(n)
    worst = 0.0
    for D in (1, 2, 5, 64, 65, n + 3):
        for kind in ("ones", "half_sine"):
            w = ps.profile_of(kind, D)
            _, _, R = run(plan, hist, zmax[0], zmin[0], D=D, w=w, axes="x")
            want = shaped_response(r, D, w)
            bound = ps.summation_bound(r, D, w)
            err = np.abs(R - want)
            assert (err <= bound).all(), (n, D, kind, float((err - bound).max()))
            assert R[0] == 0.0 and (n < 2 or R[1] == 0.0)
            if bound.max() > 0:
                worst = max(worst, float((err / np.where(bound > 0, bound, np.inf)).max()))
            if D == 1 and w is None:
                assert same_bits(R, r)
    print(f"n = {n}: worst |R_dev − R_numpy| = {worst:.3f} of the bound")


# --------------------------------------------------------------------------- against the checker


def check(got_f, got_l, R_dev, hist, zmax, zmin, lengths, t, what, steps=None):
    """The comparisons every map case takes, against the checker fed the device's own shaped
    table; prints the measured figures."""
    want_f, want_l, gap = push_map_shaped_reference(hist, zmax, zmin, R_dev, pc.HG, lengths, t,
                                                    push_steps=steps, axes="xy", return_gap=True)
    assert got_f.shape == want_f.shape and got_l.shape == want_l.shape
    assert np.array_equal(np.isnan(got_f), np.isnan(want_f)), what
    assert np.array_equal(np.isposinf(got_f), np.isposinf(want_f)), what
    fin = np.isfinite(want_f)
    assert (got_l[~fin] == -1).all(), what
    if not fin.any():
        return
    rel = np.abs(got_f[fin] - want_f[fin]) / np.where(want_f[fin] > 0, want_f[fin], 1.0)
    clear = fin & (gap > 1e-9)
    left_out = int(fin.sum() - clear.sum())
    print(f"{what}: {fin.sum()} finite entries, worst relative error {rel.max():.2e}, "
          f"{left_out} within 1e-9 of their runner-up, smallest gap {gap[fin].min():.1e}")
    assert rel.max() <= 1e-12, what
    assert left_out <= 0.001 * fin.sum(), what
    assert np.array_equal(got_l[clear], want_l[clear]), what


@pytest.mark.parametrize("shared", (False, True), ids=("per_walk", "shared"))
@pytest.mark.parametrize("n", (1, 2, 3, 63, 64, 65, 66, 130, 420))
def test_map_matches_reference(plan, n, shared):
    """Six walks of n − 7b live samples, garbage and NaN in the dead tails, a five-sample
    half-sine push on both axes; t = 0 with per-walk boxes (margins down to 0), 1 mm with shared
    ones.  The full map and the single-step form."""
    B = 6
    lengths = [max(n - 7 * b, 1) for b in range(B)]
    hist, zmax, zmin = pc.synthetic_case(n, shared, B, seed=1, lengths=lengths)
    t = 1e-3 if shared else 0.0
    w = ps.half_sine(5)
    f, l, R = run(plan, hist, zmax, zmin, lengths, t, D=5, w=w, axes="xy")
    check(f, l, R, hist, zmax, zmin, lengths, t, f"n = {n}, shared = {shared}")
    steps = [(3 * b) % max(n - 2, 1) for b in range(B)]
    f1, l1, _ = run(plan, hist, zmax, zmin, lengths, t, steps=steps, D=5, w=w, axes="xy")
    check(f1, l1, R, hist, zmax, zmin, lengths, t, f"n = {n}, shared = {shared}, single step",
          steps=steps)


def test_several_workgroups_and_a_partial_last_one(plan):
    """259 walks of 130 samples: 259 workgroups of the full map, and 64 full workgroups plus one
    with three walks of the single-step form; a constant 20-sample push."""
    n, B = 130, 259
    lengths = [max(n - 7 * (b % 19), 1) for b in range(B)]
    hist, zmax, zmin = pc.synthetic_case(n, False, B, seed=1, lengths=lengths)
    f, l, R = run(plan, hist, zmax, zmin, lengths, 1e-9, D=20, axes="xy")
    check(f, l, R, hist, zmax, zmin, lengths, 1e-9, f"n = {n}, B = {B}")
    steps = (np.arange(B) * 7) % (n - 2)
    f1, l1, _ = run(plan, hist, zmax, zmin, lengths, 1e-9, steps=steps, D=20, axes="xy")
    live = steps < np.array(lengths) - 2
    assert same_bits(f1[live], f[np.arange(B), steps][live])
    assert same_bits(l1[live], l[np.arange(B), steps][live])
    assert np.isposinf(f1[~live]).all()


def test_two_axis_limit_and_one_past_it(plan):
    """The longest walk choose_push_shaped takes on two axes (159 KiB of LDS, 16 waves), and its
    refusal one sample further: ZMPC_ESTATE, nothing launched, force untouched."""
    n = ps.AXIS_LIMIT
    hist, zmax, zmin = pc.synthetic_case(n, False, 1, seed=1, lengths=[n])
    f, l, R = run(plan, hist, zmax, zmin, None, 0.0, D=5, w=ps.half_sine(5), axes="xy")
    check(f, l, R, hist, zmax, zmin, None, 0.0, f"n = {n}, B = 1")
    n += 1
    h = torch.zeros((1, n, 2, 3), dtype=torch.float64, device="cuda")
    b = torch.ones((1, n, 2), dtype=torch.float64, device="cuda")
    for axes in ("x", "xy"):
        C = 4 if axes == "xy" else 2
        force = torch.full((1, n, C), -7.0, dtype=torch.float64, device="cuda")
        limit = torch.full((1, n, C), -7, dtype=torch.int32, device="cuda")
        with pytest.raises(_native.NativeError, match="10112 samples"):
            plan.push_map(h, b, -b, mass=MASS, out=(force, limit), axes=axes, duration=3)
        torch.cuda.synchronize()
        assert (force == -7.0).all() and (limit == -7).all()
    # the single-step form has no such limit
    f1, l1 = plan.push_map(h, b, -b, mass=MASS, push_steps=[5], axes="xy", duration=3)
    assert f1.shape == (1, 4) and np.isfinite(f1.cpu().numpy()).all()
    assert (l1.cpu().numpy() > 5).all()


# --------------------------------------------------------------------------- edges


def test_on_the_bound_and_constructed_tie(plan):
    """A walk at rest (z0 = 0) in a ±0.1 box, t = 0, a three-sample push.  x sample 70 exactly
    on its upper bound: every push that drives it up has F = 0, not NaN, and y is untouched.
    Then x samples 70 and 75 both on the bound: the lower index wins, in both forms."""
    n = 140
    hist, zmax, zmin = pc.quiet_walk(n)
    f_free, _, R = run(plan, hist, zmax, zmin, None, 0.0, D=3, axes="xy")
    zmax[0, 70, 0] = 0.0
    f, l, _ = run(plan, hist, zmax, zmin, None, 0.0, D=3, axes="xy")
    want_f, want_l = push_map_shaped_reference(hist, zmax, zmin, R, pc.HG, axes="xy")
    assert not np.isnan(f).any()
    assert np.array_equal(f == 0.0, want_f == 0.0) and (f[..., :2] == 0.0).sum() >= 10
    assert (l[f == 0.0] == 70).all() and not (f[..., 2:] == 0.0).any()
    assert same_bits(f[..., 2:], f_free[..., 2:])
    zmax[0, 75, 0] = 0.0
    f, l, _ = run(plan, hist, zmax, zmin, None, 0.0, D=3, axes="xy")
    want_f, want_l = push_map_shaped_reference(hist, zmax, zmin, R, pc.HG, axes="xy")
    s = np.arange(n)
    both_up = np.zeros((n, 2), bool)  # steps whose push raises the ZMP of samples 70 and 75
    for k, sign in enumerate((1.0, -1.0)):
        ok = s < 69
        both_up[ok, k] = (sign * R[70 - s[ok]] > 0) & (sign * R[75 - s[ok]] > 0)
    assert both_up.sum() >= 10
    assert (f[0, :, :2][both_up] == 0.0).all() and (l[0, :, :2][both_up] == 70).all()
    assert np.array_equal(f == 0.0, want_f == 0.0)
    assert np.array_equal(l[f == 0.0], want_l[want_f == 0.0])
    steps = np.nonzero(both_up.any(axis=1))[0][:1]
    f1, l1, _ = run(plan, hist, zmax, zmin, None, 0.0, steps=steps, D=3, axes="xy")
    assert same_bits(f1[0], f[0, steps[0]]) and same_bits(l1[0], l[0, steps[0]])


def test_nan_in_a_live_x_sample_fails_every_column(plan):
    n = 130
    hist, zmax, zmin = pc.synthetic_case(n, False, 3, seed=1)
    hist[1, 100, 0, 1] = np.nan
    hist[2, 129, 0, 2] = -np.inf
    for axes in ("x", "y", "xy"):
        f, l, _ = run(plan, hist, zmax, zmin, None, 0.0, D=2, axes=axes)
        assert np.isfinite(f[0, :n - 2]).all()
        assert np.isnan(f[1:]).all() and (l[1:] == -1).all()
        f1, l1, _ = run(plan, hist, zmax, zmin, None, 0.0, steps=[5, 5, 5], D=2, axes=axes)
        assert same_bits(f1[0], f[0, 5]) and np.isnan(f1[1:]).all() and (l1[1:] == -1).all()
        f, l, _ = run(plan, hist, zmax, zmin, [n, 100, 129], 0.0, D=2, axes=axes)
        assert not np.isnan(f).any()


def test_strict_plan_is_refused_and_force_untouched():
    p = Plan(torch.cuda.current_device(), 16, 1.5 / 16, 0.75, 9.81, 1.0, 1e-6, True)
    n = 20
    h = torch.zeros((2, n, 2, 3), dtype=torch.float64, device="cuda")
    b = torch.ones((n, 2), dtype=torch.float64, device="cuda")
    for steps, shape in ((None, (2, n, 4)), ([3, 4], (2, 4))):
        force = torch.full(shape, -7.0, dtype=torch.float64, device="cuda")
        limit = torch.full(shape, -7, dtype=torch.int32, device="cuda")
        with pytest.raises(_native.NativeError, match="strict") as e:
            p.push_map(h, b, -b, mass=MASS, push_steps=steps, out=(force, limit), axes="xy",
                       duration=4)
        assert f"({_native.ZMPC_ESTATE})" in str(e.value) and "critical_force" in str(e.value)
        torch.cuda.synchronize()
        assert (force == -7.0).all() and (limit == -7).all()
    c = ZMPController(MPCConfig(horizon=16, strict=True))
    with pytest.raises(RuntimeError, match="strict"):
        c.push_map(np.ones((n, 2)), -np.ones((n, 2)), duration=3, axes="xy")
    with pytest.raises(RuntimeError, match="strict"):
        c.critical_force_exact(np.ones((n, 2)), -np.ones((n, 2)), direction=[[1.0, 1.0]])


def test_python_argument_checks(plan):
    h = torch.zeros((2, 10, 2, 3), dtype=torch.float64, device="cuda")
    b = np.ones((10, 2))
    for kw in (dict(duration=0), dict(duration=2.0), dict(duration=2, profile=[1.0]),
               dict(duration=2, profile=[1.0, np.nan]), dict(duration=1, profile=[np.inf]),
               dict(axes="z"), dict(axes=3),
               dict(duration=2, profile=torch.ones(2, dtype=torch.float64)),          # on the host
               dict(duration=2, profile=torch.ones(3, dtype=torch.float64, device="cuda")),
               dict(duration=2, profile=torch.ones(2, dtype=torch.float32, device="cuda"))):
        with pytest.raises(ValueError):
            plan.push_map(h, b, -b, mass=MASS, **kw)
    with pytest.raises(ValueError, match="out"):  # two columns for a four-column map
        plan.push_map(h, b, -b, mass=MASS, axes="xy",
                      out=(torch.empty((2, 10, 2), dtype=torch.float64, device="cuda"),
                           torch.empty((2, 10, 2), dtype=torch.int32, device="cuda")))
    # a device profile is taken as it is; a host one gives the same
    w = ps.half_sine(4)
    f_a, l_a = plan.push_map(h, b, -b, mass=MASS, duration=4, profile=w, axes="xy")
    f_b, l_b = plan.push_map(h, b, -b, mass=MASS, duration=4, profile=dev(w), axes="xy")
    assert tuple(f_a.shape) == (2, 10, 4) and torch.equal(f_a, f_b) and torch.equal(l_a, l_b)


# --------------------------------------------------------------------------- end to end


def pushed_rollouts(plan, zmax, zmin, dvel):
    """Device histories of one walk under velocity kicks at many samples, by chained
    Plan.rollout restarts: x0 = the kicked state, bounds sliced from the restart sample.
    dvel [S, n, 2] → hist [S, n, 2, 3] on the device."""
    S, n = dvel.shape[:2]
    stops = [int(q) for q in np.nonzero(np.any(dvel != 0, axis=(0, 2)))[0]]
    dv = dev(dvel)
    hist = torch.empty((S, n, 2, 3), dtype=torch.float64, device="cuda")
    x0, start = torch.zeros((S, 2, 3), dtype=torch.float64, device="cuda"), 0
    for q in stops + [None]:
        seg, _ = plan.rollout(zmax[start:], zmin[start:], x0)
        upto = n if q is None else q
        hist[:, start:upto] = seg[:, :upto - start]
        if q is None:
            break
        x0 = seg[:, q - start].clone()
        x0[:, :, 1] -= dv[:, q, :]
        start = q
    return hist


def test_critical_pushes_are_bracketed_by_pushed_rollouts():
    """N = 64 walk, t = 1e-9, D ∈ {1, 3, 20} on both axes: the weakest entry of each column, and
    the four entries of step 89 at D = 20.  Rolled out with the push at F·(1 − 1e-6) the walk
    passes walk_metrics' test, at F·(1 + 1e-6) it fails.  For y at D = 1 also with the rollout's
    own kick."""
    d = pc.golden("walk_n64.npz")
    n, dt, m, t = d["zmax"].shape[0], float(d["dt"]), float(d["m"]), 1e-9
    c = ZMPController(MPCConfig(horizon=64, strict=False))
    plan = c._plan()
    zmax, zmin = dev(d["zmax"]), dev(d["zmin"])
    count = 0
    for D in (1, 3, 20):
        pm = c.push_map(d["zmax"], d["zmin"], max_violation=t, duration=D, axes="xy")
        assert isinstance(pm, PushMap) and pm.axes == "xy" and tuple(pm.force.shape) == (1, n, 4)
        F = pm.force.cpu().numpy()[0]
        entries = [(int(np.argmin(F[:n - 2, col])), col) for col in range(4)]
        if D == 20:
            entries += [(89, col) for col in range(4)]
        dvel = np.zeros((2 * len(entries), n, 2))
        for e, (s, col) in enumerate(entries):
            sign = 1.0 - 2.0 * (col % 2)
            for k, scale in enumerate((1.0 - 1e-6, 1.0 + 1e-6)):
                dvel[2 * e + k] = ps.kicks_of(n, s, np.ones(D), col // 2, dt, m) \
                    * (sign * scale * F[s, col])
        hist = pushed_rollouts(plan, zmax, zmin, dvel)
        viol = plan.walk_metrics(hist, zmax, zmin).cpu().numpy()[:, :2].max(axis=1)
        for e, (s, col) in enumerate(entries):
            print(f"D = {D}, step {s}, column {col}: F = {F[s, col]:.6f} N, violation "
                  f"{viol[2 * e]:.3e} below, {viol[2 * e + 1]:.3e} above")
            assert np.isfinite(F[s, col])
            assert viol[2 * e] <= t < viol[2 * e + 1], (D, s, col)
            count += 1
        if D == 1:
            for s, col in entries:
                if col < 2:
                    continue
                sign = 1.0 - 2.0 * (col % 2)
                kick = dt * sign * F[s, col] / m * np.array([1.0 - 1e-6, 1.0 + 1e-6])
                h2, _ = plan.rollout(zmax, zmin, torch.zeros((2, 2, 3), dtype=torch.float64,
                                                             device="cuda"),
                                     kick=kick, kick_step=s)
                v2 = plan.walk_metrics(h2, zmax, zmin).cpu().numpy()[:, :2].max(axis=1)
                assert v2[0] <= t < v2[1], (s, col)
    assert count == 16
    # the pinned numbers, and a planar direction against the rose
    pm = c.push_map(d["zmax"], d["zmin"], max_violation=t, duration=20, axes="xy")
    val, step, axis, sign = pm.weakest_push()
    assert abs(float(val[0]) - 0.580999) <= 1e-6
    assert (int(step[0]), int(axis[0]), int(sign[0])) == (44, 1, -1)
    F = pm.force.cpu().numpy()[0]
    assert abs(F[89, 0] - 9.962989) <= 1e-6 and abs(F[89, 3] - 2.066079) <= 1e-6
    mag, lim = pm.rose([[1.0, 1.0], [0.0, -2.0]])
    one = c.critical_force_exact(d["zmax"], d["zmin"], force_step=89, direction=[[1.0, 1.0]],
                                 max_violation=t, duration=20)
    assert tuple(one.shape) == (1,) and float(one[0]) == float(mag[0, 89, 0])
    assert float(mag[0, 89, 1]) == F[89, 3]
    # the defaults are the one-sample y map, as before
    old = c.critical_force_exact(d["zmax"], d["zmin"], direction=[1.0, -1.0], max_violation=t)
    pm1 = c.push_map(d["zmax"], d["zmin"], max_violation=t)
    assert pm1.axes == "y" and torch.equal(old, pm1.force[0, n // 2])
