"""Pushed rollouts without a GPU (zmpc_rollout_pushed, zmpc_herdt_rollout_pushed): the symbols
are exported and bound and refuse bad arguments before any device call; the oracle loops the
device tests compare with (tests/push_rollout_cases.py) are anchored to the oracles they restate
and answer x0 + 1e-12 under the existing 1e-10 bar on every case used; analysis.Push and the
argument errors of critical_force."""
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
import push_shaped_cases as ps
import strict_cases as sc

from mpc_bipedal import _native  # noqa: E402
from mpc_bipedal.analysis import Push  # noqa: E402
from mpc_bipedal.config import MPCConfig  # noqa: E402
from mpc_bipedal.controllers import ZMPController  # noqa: E402

PTR = 4096  # a non-NULL device address, never read
BAR = 1e-10


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
    push = _native.ZmpcPush(PTR, 2, None, 0, None, 1)
    lib.zmpc_rollout_pushed(ctypes.addressof(blk), 0, 2, PTR, PTR, 4, PTR, ctypes.addressof(push),
                            PTR, None, None)


# --------------------------------------------------------------------------- export and binding

def test_symbols_exported_and_bound(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True,
                         text=True).stdout
    names = set(re.findall(r" T (zmpc_\w+)", out))
    assert {"zmpc_rollout_pushed", "zmpc_herdt_rollout_pushed"} <= names
    res, args = _native.SIGNATURES["zmpc_rollout_pushed"]
    assert res is ctypes.c_int and len(args) == 11 and lib.zmpc_rollout_pushed.argtypes == args
    res, args = _native.SIGNATURES["zmpc_herdt_rollout_pushed"]
    assert res is ctypes.c_int and len(args) == 16
    assert lib.zmpc_herdt_rollout_pushed.argtypes == args
    # struct zmpc_push of include/zmpc.h: pointer, int32 (+ padding), pointer, int64, pointer, int64
    P = _native.ZmpcPush
    assert ctypes.sizeof(P) == 48
    assert [getattr(P, f).offset for f, _ in P._fields_] == [0, 8, 16, 24, 32, 40]
    assert lib.zmpc_abi_version() == _native.ABI_VERSION == 7  # additive: the version stays


def _push(amp=PTR, axes=3, steps=None, step=3, profile=None, duration=4):
    return _native.ZmpcPush(amp, axes, steps, step, profile, duration)


def test_rollout_pushed_argument_checks_without_gpu(lib):
    """Every bad argument is ZMPC_EINVAL with a message.  The plan is never dereferenced on these
    paths, so a zeroed block stands in for one (N = 0, not strict)."""
    fake_plan = ctypes.create_string_buffer(4096)
    plan = ctypes.addressof(fake_plan)

    def call(plan=plan, B=2, n=10, zmax=PTR, zmin=PTR, stride=20, x0=PTR, push=_push(), hist=PTR):
        rc = lib.zmpc_rollout_pushed(plan, B, n, zmax, zmin, stride, x0,
                                     None if push is None else ctypes.addressof(push), hist, None,
                                     None)
        return rc, lib.zmpc_last_error()

    rc, msg = call(plan=None)
    assert rc == _native.ZMPC_EINVAL and b"NULL plan" in msg
    rc, msg = call(push=None)
    assert rc == _native.ZMPC_EINVAL and b"push is NULL" in msg
    rc, msg = call(push=_push(amp=None))
    assert rc == _native.ZMPC_EINVAL and b"amp is NULL" in msg
    for axes in (0, 4, -1, 7):
        rc, msg = call(push=_push(axes=axes))
        assert rc == _native.ZMPC_EINVAL and b"axes" in msg, axes
    for duration in (0, -1, -2 ** 40):
        rc, msg = call(push=_push(duration=duration))
        assert rc == _native.ZMPC_EINVAL and b"duration" in msg, duration
    # the checks of zmpc_rollout, for a general push and for the legacy one (which is forwarded)
    for push in (_push(), _push(axes=2, duration=1)):
        for bad in (dict(zmax=None), dict(zmin=None), dict(x0=None), dict(hist=None)):
            rc, msg = call(push=push, **bad)
            assert rc == _native.ZMPC_EINVAL and b"NULL array" in msg, bad
        for bad in (dict(B=-1), dict(n=0), dict(n=-3)):
            rc, msg = call(push=push, **bad)
            assert rc == _native.ZMPC_EINVAL and b"B >= 0 and n >= 1" in msg, bad
        for stride in (19, 1, -20):
            rc, msg = call(push=push, stride=stride)
            assert rc == _native.ZMPC_EINVAL and b"bounds_stride" in msg, stride
        rc, msg = call(push=push, B=2 ** 31)
        assert rc == _native.ZMPC_EINVAL and b"batch too large" in msg
        rc, msg = call(push=push, n=2 ** 24 + 1, stride=0)
        assert rc == _native.ZMPC_EINVAL and b"walk too long" in msg
    # an empty batch is a no-op, a NULL amp included
    for axes in (1, 2, 3):
        assert call(B=0, push=_push(axes=axes, amp=None)) == (0, b"")
        assert call(B=0, push=_push(axes=axes, duration=1), zmax=None, hist=None) == (0, b"")


def test_herdt_rollout_pushed_argument_checks_without_gpu(lib):
    fake_plan = ctypes.create_string_buffer(4096)
    plan = ctypes.addressof(fake_plan)
    from mpc_bipedal.controllers import herdt
    prm = herdt.make_params(MPCConfig(), 2)

    def call(plan=plan, prm=prm, B=2, n=10, v=PTR, vs=20, st=PTR, ss=10, nb=PTR, ns=10, x0=PTR,
             push=_push(), hist=PTR, foot=PTR):
        rc = lib.zmpc_herdt_rollout_pushed(
            plan, None if prm is None else ctypes.addressof(prm), B, n, v, vs, st, ss, nb, ns, x0,
            None if push is None else ctypes.addressof(push), hist, foot, None, None)
        return rc, lib.zmpc_last_error()

    for bad in (dict(plan=None), dict(prm=None)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"NULL plan or params" in msg
    rc, msg = call(push=None)
    assert rc == _native.ZMPC_EINVAL and b"push is NULL" in msg
    rc, msg = call(push=_push(amp=None))
    assert rc == _native.ZMPC_EINVAL and b"amp is NULL" in msg
    for axes in (0, 4, -1):
        rc, msg = call(push=_push(axes=axes))
        assert rc == _native.ZMPC_EINVAL and b"axes" in msg, axes
    for duration in (0, -5):
        rc, msg = call(push=_push(duration=duration))
        assert rc == _native.ZMPC_EINVAL and b"duration" in msg, duration
    for push in (_push(), _push(axes=2, duration=1)):
        for bad in (dict(v=None), dict(st=None), dict(nb=None), dict(x0=None), dict(hist=None),
                    dict(foot=None)):
            rc, msg = call(push=push, **bad)
            assert rc == _native.ZMPC_EINVAL and b"NULL array" in msg, bad
        rc, msg = call(push=push, n=0)
        assert rc == _native.ZMPC_EINVAL and b"n >= 1" in msg
        rc, msg = call(push=push, B=-1)
        assert rc == _native.ZMPC_EINVAL and b"B < 0" in msg
        for bad in (dict(vs=19), dict(ss=9), dict(ns=3)):
            rc, msg = call(push=push, **bad)
            assert rc == _native.ZMPC_EINVAL and b"strides" in msg, bad
        assert call(push=push, B=0) == (0, b"")


def test_reduced_cholesky_solvers_refuse_a_shove_before_any_launch(lib):
    """ZMPC_ESTATE with the reason, decided on the host from the plan's fields alone: a zeroed
    block with `strict` set and ZMPC_OPT_STRICT_SOLVER 1 or 2."""
    blk = ctypes.create_string_buffer(4096)
    ints = (ctypes.c_int * 5).from_buffer(blk)  # (device, cus, N, Kpad, strict)
    ints[2], ints[4] = 64, 1
    plan = ctypes.addressof(blk)
    for solver in (1, 2):
        assert lib.zmpc_plan_set_option(plan, _native.OPTIONS["strict_solver"], solver) == 0
        for push in (_push(duration=2, axes=2), _push(duration=1, axes=1),
                     _push(duration=1, axes=2, profile=PTR)):
            rc = lib.zmpc_rollout_pushed(plan, 4, 40, PTR, PTR, 80, PTR, ctypes.addressof(push),
                                         PTR, None, None)
            msg = lib.zmpc_last_error()
            assert rc == _native.ZMPC_ESTATE and b"reduced-Cholesky" in msg, (solver, msg)
            assert b"use strict solver 0, 3 or 4" in msg
    # solver 0 at a horizon neither other kernel takes (no LQ table, N past the scan kernel's):
    # the message names the horizon instead of advising solver 0
    assert lib.zmpc_plan_set_option(plan, _native.OPTIONS["strict_solver"], 0) == 0
    ints[2] = 1000
    push = _push(duration=2, axes=2)
    rc = lib.zmpc_rollout_pushed(plan, 4, 40, PTR, PTR, 80, PTR, ctypes.addressof(push), PTR, None,
                                 None)
    msg = lib.zmpc_last_error()
    assert rc == _native.ZMPC_ESTATE and b"N = 1000" in msg and b"use strict solver" not in msg


# --------------------------------------------------------------------------- the oracle loops

def test_window_table():
    """The push as a table of velocity steps: truncation, a start outside the range, no product
    without a profile; analysis.Push.velocity_steps states the same."""
    n = 12
    w = ps.half_sine(4)
    dv = pr.window(n, 9, 4, w, (0.5, -0.25))
    assert np.array_equal(np.nonzero(dv[:, 0])[0], [9, 10])  # step n − 1 is never applied
    assert dv[9, 0] == 0.5 * w[0] and dv[10, 1] == -0.25 * w[1]
    for s in (-1, n - 1, n, 10 ** 6):
        assert not pr.window(n, s, 4, w, (0.5, -0.25)).any()
    assert np.array_equal(pr.window(n, 2, 1, None, (0.0, 0.3)), pr.kick_window(n, 0.3, 2))
    dt, m = 0.01, 40.0
    p = Push([2.0, -3.0], [[3.0, 4.0], [0.0, 1.0]], [9, -1], duration=4, profile=w)
    got = p.velocity_steps(dt, m, 2, n)
    amp = p.amplitudes(dt, m, 2)
    assert p.axes == "xy" and np.allclose(amp[0], dt * 2.0 * np.array([0.6, 0.8]) / m, rtol=1e-15)
    assert np.array_equal(got[0], pr.window(n, 9, 4, w, amp[0])) and not got[1].any()


def test_strict_loop_is_the_oracle_and_answers_within_the_bar():
    """On every (family, N, weights) of the device test, 3 walks: the loop equals
    O.rollout_strict bit for bit on the case's own one-sample y kick, and under each of the three
    pushes it answers x0 + 1e-12 under the existing 1e-10 bar (7.11e-11 at the worst case,
    |state| <= 45): no case needs dropping."""
    jobs = [(f, N, wi, pi) for f in sc.FAMILIES for N in pr.STRICT_HORIZONS
            for wi in range(len(sc.WEIGHTS)) for pi in range(len(pr.PUSHES))]
    # ... and the rising (asymmetric) profile on its case, push indices 3 and 4
    jobs += [pr.RAMP_CASE + (wi, len(pr.PUSHES) + k) for wi in range(len(sc.WEIGHTS))
             for k in range(len(pr.ramp_pushes()))]
    with _pool() as pool:
        out = list(pool.map(pr.strict_probe, jobs, chunksize=2))
    anchor = max(o[0] for o in out)
    resp = max(o[1] for o in out)
    big = max(o[2] for o in out)
    print(f"strict loop: anchor {anchor:.3g}, response to x0 + 1e-12 {resp:.3g}, "
          f"max |state| {big:.3g}")
    assert anchor == 0.0
    assert resp < BAR
    assert big <= 45.0


def test_herdt_loop_is_rollout_ref_and_answers_within_the_bar():
    """The pushed Herdt loop equals herdt_cases.rollout_ref on the one-sample y kicks of
    rollout_cases(), and on the walks the device test pushes its CoM and feet answer x0 + 1e-12
    under the 1e-10 of test_oracle_alone_within_bound: the five single walks, the rising profile
    on its walk, and the 33 walks of rollout_batch() under their per-walk push."""
    for case in hc.rollout_cases():
        cfg = hc.make_config(case["cfg_kw"])
        kick, ks = hc.case_kick(case), case["kick_step"]
        ref = hc.rollout_reference(case["name"])
        mine = pr.herdt_rollout_pushed(cfg, case["x0"], case["v"], case["states"],
                                       pr.kick_window(case["n"], kick, ks))
        assert all(np.array_equal(a, b) for a, b in zip(mine, ref)), case["name"]
    keys = list(pr.HERDT_WALKS) + [(pr.HERDT_RAMP_WALK, "ramp")] + \
        [("batch", b) for b in range(len(hc.rollout_batch()["x0"]))]
    with _pool() as pool:
        out = list(pool.map(pr.herdt_probe, keys))
    for key, resp in zip(keys, out):
        print(f"herdt loop {key}: response to x0 + 1e-12 {resp:.3g}")
        assert resp < BAR, key


# --------------------------------------------------------------------------- Python layer

def test_push_normalisation_and_argument_errors():
    p = Push(60.0, +1, 45)
    assert p.axes == "y" and p.duration == 1 and p.profile is None and p.step == 45
    assert np.array_equal(p.amplitudes(0.01, 40.0, 3), np.full((3, 1), 0.01 * 60.0 / 40.0))
    assert np.array_equal(Push(60.0, -2.5, 45).amplitudes(0.01, 40.0, 1), [[-0.01 * 60.0 / 40.0]])
    assert Push(1.0, (0, -1), 0).axes == "y" and Push(1.0, (1, 0), 0).axes == "x"
    q = Push([1.0, 2.0], (1, 1), [3, 4], duration=3, profile=[0.5, 1.0, 0.5])
    assert q.axes == "xy" and q.batch() == 2
    a = q.amplitudes(0.02, 10.0, 2)
    assert a.shape == (2, 2) and np.allclose(a[1], 0.02 * 2.0 / np.sqrt(2) / 10.0, rtol=1e-15)
    assert np.allclose(np.hypot(*Push(1.0, [[3, 4]], 0).direction[0]), 1.0)
    with pytest.raises(ValueError, match="batch holds"):
        q.amplitudes(0.02, 10.0, 3)
    for bad in (dict(direction=0), dict(direction=(0, 0)), dict(direction=float("nan")),
                dict(direction=np.ones((2, 2, 2))), dict(force=float("inf")),
                dict(force=np.ones((2, 2))), dict(step=1.5), dict(duration=0),
                dict(duration=2.0), dict(duration=2, profile=[1.0]),
                dict(duration=2, profile=[1.0, float("nan")])):
        kw = dict(force=1.0, direction=1, step=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            Push(**kw)
    with pytest.raises(ValueError, match="disagree"):
        Push([1.0, 2.0], 1, [1, 2, 3]).batch()


def test_python_argument_errors_before_any_device_call():
    """push= together with F_ext, and the shove arguments of critical_force, raise ValueError
    before a plan is built (no device is needed to see them)."""
    ctl = ZMPController(MPCConfig())
    z = np.zeros((10, 2))
    p = Push(10.0, 1, 3, duration=2)
    with pytest.raises(ValueError, match="either F_ext or push"):
        ctl.generate_state_trajectory_batch(None, z + 1, z - 1, F_ext=[1.0], push=p)
    with pytest.raises(ValueError, match="either F_ext or push"):
        ctl.generate_com_trajectory_batch(None, z + 1, z - 1, F_ext=[1.0], push=p)
    for kw in (dict(force_step=3), dict(walk_lengths=[10])):
        with pytest.raises(ValueError, match="its own start step"):
            ctl.generate_state_trajectory_batch(None, z + 1, z - 1, push=p, **kw)
    with pytest.raises(ValueError, match="either F_ext or push"):
        ctl.generate_com_trajectory_herdt_batch(None, z, np.zeros(10, np.int8), F_ext=[1.0],
                                                push=p)
    for kw in (dict(duration=0), dict(duration=1.5), dict(duration=2, profile=[1.0]),
               dict(duration=2, fused=True), dict(profile=[1.0], fused=True),
               dict(direction=[[0.0, -1.0]], fused=True), dict(direction=[[0.0, 0.0]])):
        with pytest.raises(ValueError):
            ctl.critical_force(z + 1, z - 1, **kw)
