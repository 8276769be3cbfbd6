"""Rollouts under per-walk traces without a GPU (zmpc_rollout_traced, zmpc_herdt_rollout_traced):
the symbols are exported and bound and refuse bad arguments before any device call;
analysis.PushTrace; the fixed inputs of tests/trace_cases.py are fair to the device bars (the
oracle loops answer x0 + 1e-12 below 1e-9 under them, and every trace moves its walk); and the
extended-precision statement of the unconstrained response is anchored on chained oracle
rollouts."""
import ctypes
import multiprocessing
import os
import re
import subprocess
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import herdt_cases as hc
import push_rollout_cases as pr
import trace_cases as tc
from conftest import golden
from oracle import zmp_oracle as O

from mpc_bipedal import _native  # noqa: E402
from mpc_bipedal.analysis import Push, PushTrace  # noqa: E402
from mpc_bipedal.config import MPCConfig  # noqa: E402
from mpc_bipedal.controllers import ZMPController  # noqa: E402

PTR = 4096  # a non-NULL device address, never read


def _pool():
    # spawn, as every pool of the suite; 15 workers, so that with this process at most 16 exist
    return ProcessPoolExecutor(max_workers=min(15, os.cpu_count() or 1),
                               mp_context=multiprocessing.get_context("spawn"))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        pytest.fail("libzmpc.so not built (run __graft_entry__.build())")
    lib = _native.load()
    yield lib
    blk = ctypes.create_string_buffer(4096)  # a passing call leaves no message behind
    tr = _trace()
    lib.zmpc_rollout_traced(ctypes.addressof(blk), 0, 2, PTR, PTR, 4, PTR, ctypes.addressof(tr),
                            PTR, None)


def _trace(dv=PTR, axes=3, steps=None, step=3, length=4, stream=None):
    return _native.ZmpcTrace(dv, axes, steps, step, length, stream)


# --------------------------------------------------------------------------- export and binding

def test_symbols_exported_and_bound(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True,
                         text=True).stdout
    names = set(re.findall(r" T (zmpc_\w+)", out))
    assert {"zmpc_rollout_traced", "zmpc_herdt_rollout_traced"} <= names
    res, args = _native.SIGNATURES["zmpc_rollout_traced"]
    assert res is ctypes.c_int and len(args) == 10 and lib.zmpc_rollout_traced.argtypes == args
    res, args = _native.SIGNATURES["zmpc_herdt_rollout_traced"]
    assert res is ctypes.c_int and len(args) == 15
    assert lib.zmpc_herdt_rollout_traced.argtypes == args
    # struct zmpc_trace of include/zmpc.h: pointer, int32 (+ padding), pointer, int64, int64, pointer
    T = _native.ZmpcTrace
    assert ctypes.sizeof(T) == 48
    assert [getattr(T, f).offset for f, _ in T._fields_] == [0, 8, 16, 24, 32, 40]
    assert [f for f, _ in T._fields_] == ["dv", "axes", "steps", "step", "length", "stream"]
    assert ctypes.sizeof(_native.ZmpcPush) == 48
    assert lib.zmpc_abi_version() == _native.ABI_VERSION == 7  # additive: the version stays


def test_header_declares_the_calls_without_a_stream_parameter():
    """The stream travels in the descriptor: neither call is declared with `void* stream`, so the
    stream-contract table's rule does not reach them, and the header says why."""
    import stream_cases as S
    assert not {"zmpc_rollout_traced", "zmpc_herdt_rollout_traced"} & set(S.stream_symbols())
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "zmpc.h")).read()
    assert "The trace, stated once" in text and "tests/stream_cases.py" in text
    assert re.search(r"void\*\s+stream;\s*/\* hipStream_t", text)


def test_rollout_traced_argument_checks_without_gpu(lib):
    """Every bad argument is ZMPC_EINVAL with a message.  The plan is never dereferenced on these
    paths, so a zeroed block stands in for one (N = 0, not strict)."""
    fake_plan = ctypes.create_string_buffer(4096)
    plan = ctypes.addressof(fake_plan)

    def call(plan=plan, B=2, n=10, zmax=PTR, zmin=PTR, stride=20, x0=PTR, trace=_trace(),
             hist=PTR):
        rc = lib.zmpc_rollout_traced(plan, B, n, zmax, zmin, stride, x0,
                                     None if trace is None else ctypes.addressof(trace), hist,
                                     None)
        return rc, lib.zmpc_last_error()

    rc, msg = call(plan=None)
    assert rc == _native.ZMPC_EINVAL and b"NULL plan" in msg
    rc, msg = call(trace=None)
    assert rc == _native.ZMPC_EINVAL and b"trace is NULL" in msg
    rc, msg = call(trace=_trace(dv=None))
    assert rc == _native.ZMPC_EINVAL and b"dv is NULL" in msg
    for axes in (0, 4, -1, 7):
        rc, msg = call(trace=_trace(axes=axes))
        assert rc == _native.ZMPC_EINVAL and b"axes" in msg, axes
    for length in (0, -1, -2 ** 40):
        rc, msg = call(trace=_trace(length=length))
        assert rc == _native.ZMPC_EINVAL and b"length" in msg, length
    # a length whose B·length·16 bytes pass int64 names no array
    for length in (2 ** 62, 2 ** 63 - 1, 2 ** 59):
        rc, msg = call(trace=_trace(length=length))
        assert rc == _native.ZMPC_EINVAL and b"length too large" in msg, length
    assert call(B=0, trace=_trace(length=2 ** 58)) == (0, b"")
    # the checks of zmpc_rollout
    for bad in (dict(zmax=None), dict(zmin=None), dict(x0=None), dict(hist=None)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"NULL array" in msg, bad
    for bad in (dict(B=-1), dict(n=0), dict(n=-3)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"B >= 0 and n >= 1" in msg, bad
    for stride in (19, 1, -20):
        rc, msg = call(stride=stride)
        assert rc == _native.ZMPC_EINVAL and b"bounds_stride" in msg, stride
    rc, msg = call(B=2 ** 31)
    assert rc == _native.ZMPC_EINVAL and b"batch too large" in msg
    rc, msg = call(n=2 ** 24 + 1, stride=0)
    assert rc == _native.ZMPC_EINVAL and b"walk too long" in msg
    # an empty batch is a no-op, a NULL dv included
    for axes in (1, 2, 3):
        assert call(B=0, trace=_trace(axes=axes, dv=None)) == (0, b"")
        assert call(B=0, trace=_trace(axes=axes), zmax=None, hist=None) == (0, b"")


def test_herdt_rollout_traced_argument_checks_without_gpu(lib):
    fake_plan = ctypes.create_string_buffer(4096)
    plan = ctypes.addressof(fake_plan)
    from mpc_bipedal.controllers import herdt
    prm = herdt.make_params(MPCConfig(), 2)

    def call(plan=plan, prm=prm, B=2, n=10, v=PTR, vs=20, st=PTR, ss=10, nb=PTR, ns=10, x0=PTR,
             trace=_trace(), hist=PTR, foot=PTR):
        rc = lib.zmpc_herdt_rollout_traced(
            plan, None if prm is None else ctypes.addressof(prm), B, n, v, vs, st, ss, nb, ns, x0,
            None if trace is None else ctypes.addressof(trace), hist, foot, None)
        return rc, lib.zmpc_last_error()

    for bad in (dict(plan=None), dict(prm=None)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"NULL plan or params" in msg
    rc, msg = call(trace=None)
    assert rc == _native.ZMPC_EINVAL and b"trace is NULL" in msg
    rc, msg = call(trace=_trace(dv=None))
    assert rc == _native.ZMPC_EINVAL and b"dv is NULL" in msg
    for axes in (0, 4, -1):
        rc, msg = call(trace=_trace(axes=axes))
        assert rc == _native.ZMPC_EINVAL and b"axes" in msg, axes
    for length in (0, -5):
        rc, msg = call(trace=_trace(length=length))
        assert rc == _native.ZMPC_EINVAL and b"length" in msg, length
    for bad in (dict(v=None), dict(st=None), dict(nb=None), dict(x0=None), dict(hist=None),
                dict(foot=None)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"NULL array" in msg, bad
    rc, msg = call(n=0)
    assert rc == _native.ZMPC_EINVAL and b"n >= 1" in msg
    rc, msg = call(B=-1)
    assert rc == _native.ZMPC_EINVAL and b"B < 0" in msg
    for bad in (dict(vs=19), dict(ss=9), dict(ns=3)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"strides" in msg, bad
    assert call(B=0) == (0, b"")
    assert call(B=0, trace=_trace(dv=None)) == (0, b"")


def test_reduced_cholesky_solvers_refuse_a_trace_before_any_launch(lib):
    """ZMPC_ESTATE with the reason, decided on the host from the plan's fields alone: a zeroed
    block with `strict` set and ZMPC_OPT_STRICT_SOLVER 1 or 2."""
    blk = ctypes.create_string_buffer(4096)
    ints = (ctypes.c_int * 5).from_buffer(blk)  # (device, cus, N, Kpad, strict)
    ints[2], ints[4] = 64, 1
    plan = ctypes.addressof(blk)
    tr = _trace(length=1, axes=2)  # (even the shape of the legacy kick: a trace is never forwarded)
    for solver in (1, 2):
        assert lib.zmpc_plan_set_option(plan, _native.OPTIONS["strict_solver"], solver) == 0
        rc = lib.zmpc_rollout_traced(plan, 4, 40, PTR, PTR, 80, PTR, ctypes.addressof(tr), PTR,
                                     None)
        msg = lib.zmpc_last_error()
        assert rc == _native.ZMPC_ESTATE and b"reduced-Cholesky" in msg, (solver, msg)
        assert b"zmpc_rollout_traced" in msg and b"use strict solver 0, 3 or 4" in msg
    assert lib.zmpc_plan_set_option(plan, _native.OPTIONS["strict_solver"], 0) == 0
    ints[2] = 1000
    rc = lib.zmpc_rollout_traced(plan, 4, 40, PTR, PTR, 80, PTR, ctypes.addressof(tr), PTR, None)
    msg = lib.zmpc_last_error()
    assert rc == _native.ZMPC_ESTATE and b"N = 1000" in msg and b"use strict solver" not in msg


# --------------------------------------------------------------------------- analysis.PushTrace

def test_push_trace_validation_and_axes():
    f = np.arange(12.0).reshape(2, 3, 2) + 1.0
    t = PushTrace(f, [4, -1])
    assert t.axes == "xy" and t.length == 3 and t.batch() == 2 and t.unit == "N"
    assert np.array_equal(t.step, [4, -1]) and PushTrace(f).step == 0
    assert PushTrace(f[:, :, 0]).axes == "y"                  # [B, L]: the reference's y
    fx, fy = f.copy(), f.copy()
    fx[:, :, 1], fy[:, :, 0] = 0.0, 0.0
    assert PushTrace(fx).axes == "x" and PushTrace(fy).axes == "y"
    assert PushTrace(fx).values.shape == (2, 3, 1)
    assert PushTrace(np.zeros((2, 3, 2))).axes == "y"        # nothing to apply: a y trace of zeros
    dv = t.dv(0.01, 40.0, 2)
    assert np.array_equal(dv, 0.01 * f / 40.0)
    with pytest.raises(ValueError, match="batch holds"):
        t.dv(0.01, 40.0, 3)
    v = PushTrace.from_velocity_steps(f, 2, "xy")
    assert v.unit == "m/s" and v.dv(0.01, 40.0, 2) is v.values  # taken as they are
    assert PushTrace.from_velocity_steps(f[:, :, 0], 0, "x").axes == "x"
    assert np.array_equal(t.scaled(0.5).values, 0.5 * f) and t.values is not t.scaled(1.0).values
    for bad in (dict(force=np.ones(3)), dict(force=np.ones((2, 3, 3))),
                dict(force=np.ones((2, 0, 2))), dict(force=np.ones((0, 3))),
                dict(force=f, step=1.5), dict(force=f, step=[1, 2, 3]),
                dict(force=f, step=np.zeros((2, 2), int))):
        with pytest.raises(ValueError):
            PushTrace(**bad)
    for bad in (dict(dv=f, axes="x"), dict(dv=f[:, :, 0], axes="xy"), dict(dv=f, axes="z")):
        with pytest.raises(ValueError):
            PushTrace.from_velocity_steps(step=0, **bad)


def test_velocity_steps_of_a_trace_spelled_from_a_push_are_the_pushs_bit_for_bit():
    """A constant window as force rows, and any push through its own table of velocity steps."""
    dt, m, n, B = 0.01, 40.0, 12, 3
    F = np.array([2.0, -3.0, 7.5])
    unit = np.array([[0.6, 0.8], [0.0, 1.0], [-1.0, 0.0]])
    steps = np.array([9, -1, 4])
    for D in (1, 4, 20):
        p = Push(F, unit, steps, duration=D)
        t = PushTrace(np.repeat((F[:, None] * p.direction)[:, None, :], D, axis=1), steps)
        assert t.axes == p.axes == "xy"
        assert np.array_equal(t.velocity_steps(dt, m, B, n), p.velocity_steps(dt, m, B, n))
    w = np.array([0.25, 1.0, 0.5, 0.125])
    p = Push(F, unit, steps, duration=4, profile=w)
    dvel = p.velocity_steps(dt, m, B, n)
    rows = np.zeros((B, 4, 2))  # the table's own rows from each start step on
    for b, s in enumerate(steps):
        if 0 <= s < n - 1:
            rows[b, :min(4, n - s)] = dvel[b, s:s + 4]
    t = PushTrace.from_velocity_steps(rows, steps, "xy")
    assert np.array_equal(t.velocity_steps(dt, m, B, n), dvel)
    # one axis, and the table form of tests/trace_cases.py
    py = Push(F, +1, steps, duration=3)
    ty = PushTrace(np.repeat(F[:, None], 3, axis=1), steps)
    assert ty.axes == "y"
    assert np.array_equal(ty.velocity_steps(dt, m, B, n), py.velocity_steps(dt, m, B, n))
    for b in range(B):
        assert np.array_equal(ty.velocity_steps(dt, m, B, n)[b],
                              tc.table(n, ty.dv(dt, m, B)[b], int(steps[b]), "y"))


def test_python_argument_errors_before_any_device_call():
    """trace= together with push, F_ext, force_step or a kick raises ValueError before a plan is
    built (no device is needed to see them); push= keeps its own check."""
    ctl = ZMPController(MPCConfig())
    z = np.zeros((10, 2))
    p = Push(10.0, 1, 3, duration=2)
    t = PushTrace(np.ones((1, 4, 2)), 3)
    for kw in (dict(F_ext=[1.0]), dict(push=p)):
        with pytest.raises(ValueError, match="either trace or F_ext or push"):
            ctl.generate_state_trajectory_batch(None, z + 1, z - 1, trace=t, **kw)
        with pytest.raises(ValueError, match="either trace or F_ext or push"):
            ctl.generate_com_trajectory_batch(None, z + 1, z - 1, trace=t, **kw)
        with pytest.raises(ValueError, match="either trace or F_ext or push"):
            ctl.generate_com_trajectory_herdt_batch(None, z, np.zeros(10, np.int8), trace=t, **kw)
    for kw in (dict(force_step=3), dict(walk_lengths=[10])):
        with pytest.raises(ValueError, match="its own start step"):
            ctl.generate_state_trajectory_batch(None, z + 1, z - 1, trace=t, **kw)
    with pytest.raises(ValueError, match="either F_ext or push"):
        ctl.generate_state_trajectory_batch(None, z + 1, z - 1, F_ext=[1.0], push=p)
    for kw in (dict(fused=True), dict(force_step=3), dict(direction=-1), dict(duration=2),
               dict(direction=[[0.0, 1.0]]), dict(profile=[1.0])):
        with pytest.raises(ValueError):
            ctl.critical_force(z + 1, z - 1, trace=t, **kw)
    with pytest.raises(ValueError, match="analysis.PushTrace"):
        ctl.critical_force(z + 1, z - 1, trace=p)
    for kw in (dict(force_step=3), dict(direction=-1), dict(duration=2)):
        with pytest.raises(ValueError):
            ctl.critical_force_herdt(z, np.zeros(10, np.int8), 1.0, trace=t, **kw)


# --------------------------------------------------------------------------- fairness of the bars

def test_strict_traces_are_fair_and_move_the_walk():
    """Families "jitter" and "narrow" at N = 8, 33, 64, dense and sparse traces, the first 3 walks:
    the oracle loop answers x0 + 1e-12 below 1e-9 (3.5e-11 at the worst) and every trace shifts
    the CoM by more than a millimetre against the unpushed loop."""
    jobs = [(f, N, kind) for f in tc.STRICT_FAMILIES for N in tc.STRICT_HORIZONS
            for kind in ("dense", "sparse")]
    with _pool() as pool:
        out = list(pool.map(tc.strict_probe, jobs))
    for job, (resp, shift) in zip(jobs, out):
        print(f"strict loop {job}: response to x0 + 1e-12 {resp:.3g}, CoM shift {shift:.3g} m")
        assert resp < tc.BAR, job
        assert shift > tc.MOVES, job


def test_herdt_traces_are_fair_and_move_the_walk():
    """Walks "n17_triangle" and "seven" under the dense and the sparse trace, and the 33 walks of
    rollout_batch() under their own traces: CoM and feet of the pushed loop answer x0 + 1e-12
    below 1e-9, and every trace whose start step lies in the range shifts the CoM by more than a
    millimetre."""
    B = len(hc.rollout_batch()["x0"])
    keys = [(w, k) for w in tc.HERDT_WALKS for k in ("dense", "sparse")] + \
        [("batch", b) for b in range(B)]
    with _pool() as pool:
        out = list(pool.map(tc.herdt_probe, keys))
    n = hc.rollout_batch()["n"]
    steps = pr.herdt_batch_steps(n, B)
    for key, (resp, shift) in zip(keys, out):
        print(f"herdt loop {key}: response to x0 + 1e-12 {resp:.3g}, CoM shift {shift:.3g} m")
        assert resp < tc.BAR, key
        if key[0] == "batch" and not 0 <= steps[key[1]] < n - 1:
            assert shift == 0.0, key  # (a start step outside the range: no disturbance)
        else:
            assert shift > tc.MOVES, key


# --------------------------------------------------------------------------- unconstrained

PAR64 = (64, 0.01, 0.75, 9.81, 1.0, 1e-6)  # the plan of walk_n64.npz


def test_extended_precision_response_is_anchored_on_chained_rollouts():
    """The reference of the unconstrained device tests — the oracle's unpushed history minus the
    recurrence in np.longdouble — against push_rollout_cases.chained on the sparse traces (both
    patterns, one walk each): 1e-12."""
    d = golden("walk_n64.npz")
    zmax, zmin = d["zmax"], d["zmin"]
    n = len(zmax)
    consts = tc.closed_loop(PAR64)
    h0 = O.rollout_gain(zmax[None], zmin[None], np.zeros((1, 2, 3)), *PAR64)
    traces = np.stack([tc.strict_sparse(n), tc.herdt_sparse(n)])
    dvel = np.stack([tc.table(n, t, 0) for t in traces])
    ref = tc.traced_reference(np.repeat(h0, 2, axis=0), traces, np.zeros(2, int), consts)
    chain = pr.chained(zmax, zmin, PAR64, dvel)
    err = float(np.abs(ref - chain).max())
    print(f"extended-precision response vs chained rollouts: {err:.3g}")
    assert err <= 1e-12
    assert np.abs(chain[0] - h0[0]).max() > tc.MOVES
