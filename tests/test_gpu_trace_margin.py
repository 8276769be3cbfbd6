"""Device tests of the trace margin (zmpc_trace_margin, csrc/trace_margin.hip): the exact critical
scale of a per-walk trace, K draws per walk, from one unpushed history.

The reference is the extended-precision statement of tests/trace_margin_cases.py (ρ from
trace_cases.response in np.longdouble, margins in double, quotients in extended precision), which
tests/test_trace_margin_host.py shows to be a fair one: the double-precision statement stays within
1e-12 of it on every input used here.  Bar: 1e-11 relative, the header's bar for forms that compute
the same solution; limit is compared wherever the runner-up candidate lies more than 1e-12 off."""
import ctypes

import numpy as np
import pytest
import torch

import push_map_cases as pm
import trace_cases as tc
import trace_margin_cases as mc

pytestmark = pytest.mark.gpu

from mpc_bipedal import _native  # noqa: E402
from mpc_bipedal.analysis import PushTrace, TraceMargin  # noqa: E402
from mpc_bipedal.config import MPCConfig  # noqa: E402
from mpc_bipedal.controllers import ZMPController  # noqa: E402
from mpc_bipedal.solver import Plan  # noqa: E402

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


def unc_plan(par=mc.PAR150):
    if par not in _PLANS:
        _PLANS[par] = Plan(torch.cuda.current_device(), *par, False)
    return _PLANS[par]


def plan_consts(plan, par):
    """closed_loop constants with the plan's own gain row (zmpc_plan_export): the header states Ā
    from the plan's kx, which the device computes itself and which differs from the oracle's in
    its last digits — a difference the quotients would carry at full size."""
    return tc.closed_loop(par, plan.export(_native.EXPORT_KX))


def dev(a, dtype=torch.float64):
    return torch.as_tensor(a, dtype=dtype, device="cuda").contiguous()


def bits(t):
    return t.cpu().numpy().view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def margin(case, plan=None, trace=None, **kw):
    """Plan.trace_margin on a case of trace_margin_cases → (scale, limit) device tensors."""
    plan = plan or unc_plan()
    if trace is None:
        trace = PushTrace.from_velocity_steps(np.ascontiguousarray(case["dv"]), case["steps"],
                                              case["axes"])
    return plan.trace_margin(dev(case["hist"]), case["zmax"], case["zmin"], trace,
                             draws=case["K"], lengths=case["lengths"], max_violation=case["t"],
                             **kw)


def sub(case, rows):
    """The rows [r0, r1) of one walk of a case as a case of their own (K = r1 − r0)."""
    r0, r1 = rows
    b = r0 // case["K"]
    assert (r1 - 1) // case["K"] == b
    zx, zn = case["zmax"], case["zmin"]
    return dict(case, hist=case["hist"][b:b + 1], zmax=zx if zx.ndim == 2 else zx[b:b + 1],
                zmin=zn if zn.ndim == 2 else zn[b:b + 1], dv=case["dv"][r0:r1],
                steps=case["steps"][r0:r1], K=r1 - r0,
                lengths=None if case["lengths"] is None else case["lengths"][b:b + 1])


# ------------------------------------------------------------- 1: the grid vs extended precision

@pytest.mark.parametrize("n", tc.EMU_N)
def test_grid_vs_extended_precision(n):
    """The emulation's grid: every start step of emu_steps(n) with every length of emu_lengths(n),
    axes x, y and xy, K = 1, 3, 5, per-walk and shared bounds; at n = 129 the ragged variant too."""
    consts = plan_consts(unc_plan(), mc.PAR150)
    worst = 0.0
    cases = list(mc.grid(n)) + (mc.ragged_cases() if n == 129 else [])
    for case in cases:
        ref = mc.grid_extended(case, consts)
        scale, limit = margin(case)
        err, same, idx = mc.compare(scale.cpu().numpy(), limit.cpu().numpy(), ref)
        worst = max(worst, err)
        label = (n, case["L"], case["axes"], case["K"], case["zmax"].ndim == 2,
                 case["lengths"] is not None)
        assert same and idx, label
        assert err <= mc.BAR, (label, err)
    print(f"MEASURED trace margin grid n={n}: worst relative error {worst:.2e}")


# ------------------------------------------------------------- 2: bit-for-bit properties

def test_bitwise_repeat_row_alone_draws_and_scalar_step():
    """Two calls agree; a row alone equals the row in its batch; a K-draw call equals K one-draw
    calls; a scalar step equals the [R] form; a NULL limit leaves scale as it is."""
    n, L = 129, 70
    for K, shared in ((3, False), (5, True)):
        case = mc.grid_case(n, L, "xy", K, shared)
        s, l = margin(case)
        s2, l2 = margin(case)
        assert same_bits(s, s2) and torch.equal(l, l2)
        R = case["dv"].shape[0]
        for r in range(R):
            s1, l1 = margin(sub(case, (r, r + 1)))
            assert same_bits(s1[0, 0], s[r // K, r % K]) and torch.equal(l1[0, 0], l[r // K, r % K])
        for b in range(R // K):
            sk, lk = margin(sub(case, (b * K, b * K + K)))
            assert same_bits(sk[0], s[b]) and torch.equal(lk[0], l[b])
    case = mc.grid_case(n, L, "xy", 3, False)
    case["steps"] = np.full(9, 17, np.int64)
    a, la = margin(case)
    tr = PushTrace.from_velocity_steps(case["dv"], 17, "xy")
    b, lb = margin(case, trace=tr)
    assert same_bits(a, b) and torch.equal(la, lb)
    # the C call with limit = NULL
    plan = unc_plan()
    h, zx, zn, dv = dev(case["hist"]), dev(case["zmax"]), dev(case["zmin"]), dev(case["dv"])
    out = torch.full((3, 3, 2), -7.0, dtype=torch.float64, device="cuda")
    c = _native.ZmpcTrace(dv.data_ptr(), 3, None, 17, L, torch.cuda.current_stream().cuda_stream)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = _native.load().zmpc_trace_margin(plan.handle, 3, n, vp(h), vp(zx), vp(zn), 2 * n, None, 3,
                                          ctypes.addressof(c), 0.0, vp(out), None)
    torch.cuda.synchronize()
    assert rc == 0 and same_bits(out, a)


# ------------------------------------------------------------- 3: edges

def test_edges():
    """A zero trace and an out-of-range start step give +inf and −1; a failing nominal sample
    before s, or NaN in a live state, gives NaN in every draw of that walk and in no other; NaN in
    one dv entry stays in its row; a sample planted on its bound with t = 0 gives exactly 0; a
    one-axis trace draws no candidate from the other axis but takes its nominal test."""
    n, L, K = 70, 30, 3
    base = mc.grid_case(n, L, "xy", K, False)
    base["steps"] = np.full(9, 20, np.int64)
    s0, l0 = margin(base)
    assert bool(torch.isfinite(s0).all()) and bool((l0 >= 2 * 21).all())
    keep = torch.ones((3, 3), dtype=torch.bool, device="cuda")
    keep[1, 1] = False
    c = dict(base, dv=base["dv"].copy(), steps=base["steps"].copy())
    c["dv"][4] = 0.0
    c["steps"][[0, 8]] = (n - 1, -1)
    s, l = margin(c)
    for b, k in ((1, 1), (0, 0), (2, 2)):
        assert bool(torch.isposinf(s[b, k]).all()) and bool((l[b, k] == -1).all()), (b, k)
    c = dict(base, dv=base["dv"].copy())
    c["dv"][4, 3, 1] = np.nan
    s, l = margin(c)
    assert same_bits(s[keep], s0[keep]) and torch.equal(l[keep], l0[keep])
    for plant in ("bound", "nan", "inf_velocity"):
        c = dict(base, hist=base["hist"].copy(), zmax=base["zmax"].copy())
        if plant == "bound":
            c["zmax"][2, 5, 0] -= 1.0     # sample 5 lies before s = 20
        elif plant == "nan":
            c["hist"][2, 40, 1, 2] = np.nan
        else:
            c["hist"][2, 7, 0, 1] = np.inf
        s, l = margin(c)
        assert bool(torch.isnan(s[2]).all()) and bool((l[2] == -1).all()), plant
        assert same_bits(s[:2], s0[:2]) and torch.equal(l[:2], l0[:2]), plant
    cy = dict(base, axes="y", dv=np.ascontiguousarray(base["dv"][:, :, 1:]))
    s, l = margin(cy)
    assert bool(torch.isfinite(s).all()) and bool((l % 2 == 1).all())
    consts = plan_consts(unc_plan(), mc.PAR150)
    err, same, idx = mc.compare(s.cpu().numpy(), l.cpu().numpy(), mc.extended(cy, consts))
    assert same and idx and err <= mc.BAR
    c = dict(cy, zmin=base["zmin"].copy())
    c["zmin"][0, 3, 0] += 1.0             # the x axis fails the nominal test
    s, l = margin(c)
    assert bool(torch.isnan(s[0]).all()) and bool(torch.isfinite(s[1:]).all())
    # planted on its bound
    hist, zmax, zmin = pm.quiet_walk(n)
    dv = np.zeros((2, 4, 2))
    dv[:, 0, 1] = 0.01
    q = dict(hist=hist, zmax=zmax.copy(), zmin=zmin.copy(), lengths=None, dv=dv,
             steps=np.array([10, 10]), axes="xy", K=2, n=n, L=4, t=0.0)
    p = 20
    sign = np.sign(float(mc.rho_rows(dv, q["steps"], [n], n, 2, consts, "xy")[0, p, 1]))
    assert sign != 0
    (q["zmax"] if sign > 0 else q["zmin"])[0, p, 1] = 0.0
    s, l = margin(q)
    assert float(s[0, 0, 0]) == 0.0 and int(l[0, 0, 0]) == 2 * p + 1 and float(s[0, 0, 1]) > 0.0


# ------------------------------------------------------------- 4 – 6, 8: the N = 64 stored walk

def controller():
    return ZMPController(MPCConfig(horizon=64, strict=False))


def walk64_bounds():
    """Writable copies of the stored walk's bounds (the shared arrays are read-only, which torch
    warns about when it wraps them)."""
    zmax, zmin, _, _ = mc.walk64()
    return zmax.copy(), zmin.copy()


def test_constant_rows_equal_the_windows_exact_form():
    """Rows that hold the constant (dx, dy)·1 N over L = D samples: scale[:, 0] is
    critical_force_exact(direction=[[dx, dy]], duration=D, force_step=s), to 1e-11."""
    zmax, zmin = walk64_bounds()
    ctl = controller()
    dirs = np.array([[0.6, 0.8], [-0.8, 0.6], [0.0, -1.0]])
    s = 20
    worst = 0.0
    for D in (1, 20):
        force = np.repeat(dirs[:, None, :], D, axis=1)             # [3, D, 2] newtons
        m = ctl.trace_margin(zmax, zmin, PushTrace(force, s), draws=3)
        got = m.critical[0].cpu().numpy()
        for k, d in enumerate(dirs):
            ref = float(ctl.critical_force_exact(zmax, zmin, direction=d[None], duration=D,
                                                 force_step=s)[0])
            assert np.isfinite(ref) and ref > 0
            worst = max(worst, abs(got[k] - ref) / ref)
    print(f"MEASURED trace margin vs critical_force_exact: {worst:.2e}")
    assert worst <= mc.BAR


def test_brackets_and_bisection_on_the_device():
    """K = 4 draws on the N = 64 walk (two dense, the sparse shoves, one on y alone): the traced
    rollout plus walk_metrics passes at λ·(1 − 1e-6) and fails at λ·(1 + 1e-6), for column 1 with
    the negated trace; and the bracket of critical_force(trace=, iters=30), widened by 1e-6,
    holds TraceMargin.critical."""
    zmax, zmin = walk64_bounds()
    ctl = controller()
    cfg = ctl.config
    consts = plan_consts(ctl._plan(), (64, cfg.dt, cfg.h, cfg.g, cfg.Q, cfg.R))
    t = 1e-9
    dv = mc.walk64_draws()
    trace = PushTrace.from_velocity_steps(dv, 0, "xy")
    m = ctl.trace_margin(zmax, zmin, trace, draws=4, max_violation=t)
    assert isinstance(m, TraceMargin) and tuple(m.scale.shape) == (1, 4, 2)
    scale = m.scale.cpu().numpy()[0]                                # [4, 2]
    assert np.isfinite(scale).all() and (scale > 0).all()
    assert bool((m.axis[0, 3] == 1).all())                          # the y draw is limited on y
    case = mc.walk64_case(t)
    plan = ctl._plan()
    case["hist"] = plan.rollout(zmax, zmin, np.zeros((1, 2, 3)))[0].cpu().numpy()
    err, same, idx = mc.compare(m.scale.cpu().numpy(), m.limit.cpu().numpy(),
                                mc.extended(case, consts))
    print(f"MEASURED trace margin, N = 64 walk: {err:.2e}; λ {scale[:, 0].tolist()}")
    assert same and idx and err <= mc.BAR
    # one traced rollout of 16 rows: (draw, column, below or above)
    rows, want = [], []
    for k in range(4):
        for col, sign in ((0, 1.0), (1, -1.0)):
            for f, ok in ((1 - 1e-6, True), (1 + 1e-6, False)):
                rows.append(dv[k] * (sign * scale[k, col] * f))
                want.append(ok)
    hist, _ = plan.rollout(zmax, zmin, np.zeros((16, 2, 3)),
                           trace=PushTrace.from_velocity_steps(np.stack(rows), 0, "xy"))
    ok = (ctl.walk_metrics(hist, zmax, zmin).viol_max <= t).all(dim=1).cpu().numpy()
    assert np.array_equal(ok, want), ok
    assert np.array_equal(m.survives(0.03).cpu().numpy()[0], scale[:, 0] >= 0.03)
    assert float(m.survival(0.05)[0]) == float((scale[:, 0] >= 0.05).mean())
    # the bisection, one walk per draw
    lo, hi = ctl.critical_force(np.broadcast_to(zmax, (4,) + zmax.shape).copy(),
                                np.broadcast_to(zmin, (4,) + zmin.shape).copy(), trace=trace,
                                iters=30, max_violation=t)
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    print(f"MEASURED critical_force(trace=) brackets {lo.tolist()} .. {hi.tolist()}")
    assert (lo * (1 - 1e-6) <= scale[:, 0]).all() and (scale[:, 0] <= hi * (1 + 1e-6)).all()
    assert (hi - lo <= 1000.0 / 2 ** 30 * 1.0001).all()


def test_controller_errors():
    zmax, zmin = walk64_bounds()
    strict = ZMPController(MPCConfig(horizon=64, strict=True))
    trace = PushTrace.from_velocity_steps(mc.walk64_draws(), 0, "xy")
    with pytest.raises(RuntimeError, match="not affine"):
        strict.trace_margin(zmax, zmin, trace, draws=4)
    ctl = controller()
    with pytest.raises(ValueError, match="rows"):
        ctl.trace_margin(np.stack([zmax] * 3), np.stack([zmin] * 3), trace, draws=4)
    with pytest.raises(ValueError):
        ctl.trace_margin(np.stack([zmax] * 3), np.stack([zmin] * 3), trace, draws=2)
    plan = ctl._plan()
    hist, _ = plan.rollout(zmax, zmin, np.zeros((2, 2, 3)))
    with pytest.raises(ValueError, match="B·draws"):
        plan.trace_margin(hist, zmax, zmin, trace, draws=4)
    with pytest.raises(ValueError, match="draws must be"):
        plan.trace_margin(hist, zmax, zmin, trace, draws=0)
    with pytest.raises(ValueError, match="mass"):
        plan.trace_margin(hist, zmax, zmin, PushTrace(np.ones((4, 3, 2))), draws=2)
    s, l = plan.trace_margin(hist, zmax, zmin, trace, draws=2)
    assert tuple(s.shape) == (2, 2, 2) and l.dtype == torch.int32
    with pytest.raises(ValueError, match="scale and limit"):
        plan.trace_margin(hist, zmax, zmin, trace, draws=2, scale=s[:1])
    sp = strict._plan()
    with pytest.raises(_native.NativeError, match="not affine"):
        sp.trace_margin(hist, zmax, zmin, trace, draws=2)


# ------------------------------------------------------------- 7: the stream contract

def _busy(x):
    """Work that keeps the current stream occupied for a while before what follows on it."""
    for _ in range(8):
        x = x @ x
        x = x / x.abs().max()
    return x


def test_stream_contract():
    """On a non-null stream, with dv written by a torch operation on that stream immediately before
    the call, the results equal the null-stream results bit for bit; two streams with different
    batches do not mix."""
    n, L = 129, 70
    plan = unc_plan()
    ca, cb = mc.grid_case(n, L, "xy", 3, False), mc.grid_case(n, L, "xy", 5, True)

    def run(case):
        src = dev(case["dv"])
        torch.cuda.current_stream().wait_stream(torch.cuda.default_stream())
        _busy(torch.rand((1024, 1024), dtype=torch.float32, device="cuda"))
        dv = src * 1.0  # a kernel on the current stream: the call must come after it
        tr = PushTrace.from_velocity_steps(dv, case["steps"], "xy")
        return margin(case, plan=plan, trace=tr)

    ref_a, ref_b = run(ca), run(cb)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        got_a = run(ca)
    with torch.cuda.stream(s2):
        got_b = run(cb)
    s1.synchronize()
    s2.synchronize()
    for g, r in zip(got_a + got_b, ref_a + ref_b):
        assert torch.equal(g, r)
    assert bool(torch.isfinite(got_a[0]).any()) and got_a[0].shape != got_b[0].shape
