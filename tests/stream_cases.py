"""The registry of stream-taking entry points behind the stream and thread contract tests
(tests/test_stream_cases_host.py on the CPU, tests/test_gpu_streams.py on the device).  Not a
test module.

include/zmpc.h promises that every call is asynchronous on the stream it is given, that
zmpc_last_error is per thread and that a plan may be shared across threads and streams.  One Case
per path that takes a stream:

  name, family     the path; the family groups cases for the two-streams-one-plan pairs (PAIRS)
  symbols          the C-ABI symbols the case calls
  plan, options    Plan(device, *plan) with set_option(*o) for o in options (None: no plan);
                   cases with equal (plan, options) share one plan object (plan_key)
  make(variant)    seeded HOST inputs for variant "A" or "B": a dict of NumPy arrays already in
                   the layout the C-ABI takes, and of scalars, which are the same in A and B (so a
                   buffer that holds B can be overwritten with A on the device).  Both variants are
                   valid and finite, and their results differ
  outputs(d)       name -> (shape, dtype) of the preallocated outputs
  launch(lib, handle, d, o, stream)
                   issues the library call(s) on `stream` with d, o dicts of DEVICE tensors (and
                   the scalars): pointer arithmetic and ctypes calls only, no host work on the
                   data and no synchronisation.  Returns the (last nonzero) return code
  prepare(plan, d, o)
                   optional, run once under the default stream after the buffers exist: what it
                   returns is d["_prep"] (the launcher closures are built here)
  dispatch         None, or (tag, query, expected leading answer) for tests/emu/dispatch_main.cpp
  oracle(d)        None, or the plain NumPy reference of variant A -> dict
  check(got, want, d)
                   compares the outputs (NumPy arrays) with the oracle's dict at the bar of the
                   path's existing device test
  blocking         None, or the reason the call may not return before its stream has run
"""
import ctypes
import functools
import re
import os

import numpy as np

import herdt_cases as hc
import herdt_metrics_cases as hm
import metrics_cases as mc
import push_map_cases as pc
import push_rollout_cases as pr
import push_shaped_cases as ps
import strict_cases as SC
from conftest import ROOT, rmse
from oracle import zmp_oracle as O

H, G, Q, R = 0.75, 9.81, 1.0, 1e-6
HG = H / G
MASS = 40.0
# (N = 16 previews 1.6 s at dt = 0.1: at dt = 0.01 the 0.16 s preview is shorter than the pendulum's
# time constant sqrt(h/g) = 0.28 s, the closed loop is unstable and a walk of 700 samples reaches
# 1e9, where an absolute bar says nothing)
UNC16 = (16, 0.1, H, G, Q, R, False)
UNC150 = (150, 0.01, H, G, Q, R, False)
STRICT64 = (64, SC.case_dt(64), SC.WEIGHTS[0][2], G, SC.WEIGHTS[0][0], SC.WEIGHTS[0][1], True)
AXIS_X, AXIS_Y = 1, 2
VARIANTS = ("A", "B")
F8, I4, I8, I1 = "float64", "int32", "int64", "int8"


class Case:
    def __init__(self, name, family, symbols, plan, make, outputs, launch, options=(),
                 prepare=None, dispatch=None, oracle=None, check=None, blocking=None):
        self.name, self.family, self.symbols = name, family, tuple(symbols)
        self.plan, self.options = plan, tuple(options)
        self.make, self.outputs, self.launch = make, outputs, launch
        self.prepare, self.dispatch = prepare, dispatch
        self.oracle, self.check, self.blocking = oracle, check, blocking

    @property
    def plan_key(self):
        return None if self.plan is None else (self.plan, self.options)

    def __repr__(self):
        return f"Case({self.name})"


def stream_symbols():
    """The symbols include/zmpc.h declares with a `void* stream` parameter."""
    with open(os.path.join(ROOT, "include", "zmpc.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    out = []
    for m in re.finditer(r"\b(zmpc_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        if re.search(r"void\s*\*\s*stream\b", m.group(2)):
            out.append(m.group(1))
    return sorted(set(out))


def _rng(name, variant):
    return np.random.default_rng([SC.seed_of(name), ord(variant)])


def _flip(d, variant, keys):
    """Variant B of inputs that come from a fixed seed: the walks in reverse order."""
    if variant == "B":
        for k in keys:
            if d.get(k) is not None:
                d[k] = np.ascontiguousarray(d[k][::-1])
    return d


def _ptr(t):
    return None if t is None else t.data_ptr()


def _hist_out(d):
    return {"hist": ((d["B"], d["n"], 2, 3), F8), "status": ((d["B"],), I4)}


def _push_struct(d):
    """zmpc_push of the device tensors of d (read by the library during the call)."""
    from mpc_bipedal._native import ZmpcPush
    return ZmpcPush(_ptr(d["amp"]), d["axes"], _ptr(d.get("steps")), d.get("step", -1),
                    _ptr(d.get("profile")), d["duration"])


# ----------------------------------------------------------------------------- unconstrained

def unc_inputs(name, variant, B, n, shared=False, dense=False, seg=4, steps=False):
    """B walks of n samples: piecewise-constant boxes of `seg` samples (n / seg changes per axis:
    the sparse-difference correlation takes them) or, dense, boxes that move at every sample."""
    rng = _rng(name, variant)
    shape = (n, 2) if shared else (B, n, 2)
    if dense:
        zc = np.cumsum(rng.uniform(-0.01, 0.01, shape), axis=-2)
    else:
        lv = np.cumsum(rng.uniform(-0.05, 0.05, shape[:-2] + (-(-n // seg), 2)), axis=-2)
        zc = np.ascontiguousarray(np.repeat(lv, seg, axis=-2)[..., :n, :])
    x0 = np.zeros((B, 2, 3))
    x0[:, :, 0] = rng.uniform(-0.01, 0.01, (B, 2))
    x0[:, :, 1] = rng.uniform(-0.1, 0.1, (B, 2))
    d = dict(B=B, n=n, zmax=zc + 0.05, zmin=zc - 0.05, bstride=0 if shared else 2 * n, x0=x0,
             kick=rng.uniform(0.02, 0.2, B), kick_step=n // 2)
    if steps:
        d["kick_steps"] = rng.integers(0, max(n - 1, 1), B).astype(np.int64)
    return d


def launch_rollout(lib, h, d, o, s):
    if d.get("kick_steps") is not None:
        return lib.zmpc_rollout_kicks(h, d["B"], d["n"], _ptr(d["zmax"]), _ptr(d["zmin"]),
                                      d["bstride"], _ptr(d["x0"]), _ptr(d["kick"]),
                                      _ptr(d["kick_steps"]), _ptr(o["hist"]), _ptr(o["status"]), s)
    return lib.zmpc_rollout(h, d["B"], d["n"], _ptr(d["zmax"]), _ptr(d["zmin"]), d["bstride"],
                            _ptr(d["x0"]), _ptr(d["kick"]), d["kick_step"], _ptr(o["hist"]),
                            _ptr(o["status"]), s)


def launch_rollout_pushed(lib, h, d, o, s):
    push = _push_struct(d)
    return lib.zmpc_rollout_pushed(h, d["B"], d["n"], _ptr(d["zmax"]), _ptr(d["zmin"]),
                                   d["bstride"], _ptr(d["x0"]), ctypes.addressof(push),
                                   _ptr(o["hist"]), _ptr(o["status"]), s)


def _dense_bounds(d):
    zmax, zmin = d["zmax"], d["zmin"]
    if zmax.ndim == 2:
        zmax, zmin = (np.broadcast_to(a, (d["B"],) + a.shape) for a in (zmax, zmin))
    return zmax, zmin


def unc_oracle(plan):
    def oracle(d):
        zmax, zmin = _dense_bounds(d)
        ks = d["kick_steps"] if d.get("kick_steps") is not None else d["kick_step"]
        return {"hist": O.rollout_gain(zmax, zmin, d["x0"], *plan[:6], d["kick"], ks)}
    return oracle


def unc_check(got, want, d):
    # tests/test_gpu_parity.py test_batch_unconstrained_vs_oracle: every state within 1e-8, CoM
    # RMSE 1e-10, every status 0
    assert not got["status"].any()
    err, r = np.abs(got["hist"] - want["hist"]).max(), rmse(got["hist"][..., 0],
                                                            want["hist"][..., 0])
    assert err <= 1e-8 and r <= 1e-10, (err, r)


def _unc(name, plan, options, kind, B, n, query, sparse=None, **kw):
    """query: the six numbers of dispatch_main's `unc` line; the answer must begin with `kind`
    (and, where given, stage the sparse attempt or not)."""
    want = (kind,) if sparse is None else (kind, sparse)
    return Case(name, "unc", ("zmpc_rollout_kicks" if kw.get("steps") else "zmpc_rollout",),
                plan, lambda v: unc_inputs(name, v, B, n, **kw), _hist_out, launch_rollout,
                options=options, dispatch=("unc", query, want), oracle=unc_oracle(plan),
                check=unc_check)


def unc_pushed_inputs(name, variant, B=5, n=23):
    d = unc_inputs(name, variant, B, n)
    d["x0"] = np.zeros_like(d["x0"])     # (the chained oracle starts its walks at rest)
    rng = _rng(name + "-push", variant)
    d.update(amp=rng.uniform(-0.05, 0.05, (B, 2)), axes=AXIS_X | AXIS_Y,
             steps=rng.integers(0, n - 1, B).astype(np.int64), profile=pr.ramp(3), duration=3)
    return d


def unc_pushed_oracle(d):
    """Chained O.rollout_gain segments (push_rollout_cases.chained), walk by walk: each walk has
    its own bounds."""
    w = d["profile"]
    return {"hist": np.concatenate([
        pr.chained(d["zmax"][b], d["zmin"][b], UNC16[:6],
                   pr.window(d["n"], int(d["steps"][b]), d["duration"], w, d["amp"][b])[None])
        for b in range(d["B"])])}


def unc_pushed_check(got, want, d):
    # tests/test_gpu_push_rollout.py test_unconstrained_vs_chained_rollouts: CoM RMSE 1e-9, every
    # state within 1e-7, every status 0
    assert not got["status"].any()
    r, e = rmse(got["hist"][..., 0], want["hist"][..., 0]), np.abs(got["hist"]
                                                                   - want["hist"]).max()
    assert r <= 1e-9 and e <= 1e-7, (r, e)


def unc_step_inputs(name, variant, B=70, N=16):
    rng = _rng(name, variant)
    zc = np.cumsum(rng.uniform(-0.01, 0.01, (B, N)), axis=1)
    x = rng.uniform(-1.0, 1.0, (B, 3)) * np.array([0.05, 0.2, 0.5])
    return dict(B=B, x=x, zmax_win=zc + 0.05, zmin_win=zc - 0.05)


def launch_step(lib, h, d, o, s):
    return lib.zmpc_step(h, d["B"], _ptr(d["x"]), _ptr(d["zmax_win"]), _ptr(d["zmin_win"]),
                         _ptr(o["x_next"]), _ptr(o["status"]), s)


def _step_out(d):
    return {"x_next": ((d["B"], 3), F8), "status": ((d["B"],), I4)}


def unc_step_oracle(d):
    N, dt = UNC16[:2]
    k, kx = O.gain_row(N, dt, H, G, Q, R)
    A, Bv, _ = O.lipm(dt, H, G)
    u = ((d["zmax_win"] + d["zmin_win"]) / 2) @ k - d["x"] @ kx
    return {"x_next": d["x"] @ A.T + u[:, None] * Bv[:, 0]}


def step_check(got, want, d):
    # tests/test_gpu_parity.py test_batched_step_vs_reference, tests/test_gpu_strict_cases.py
    # assert_step: 1e-9 relative to max(1, |reference|), every status 0
    assert not got["status"].any()
    k = len(want["x_next"])
    e = SC.rel_err(got["x_next"][:k], want["x_next"])
    assert e <= 1e-9, e


# ----------------------------------------------------------------------------- strict

ORACLE_WALKS = 7    # one walk of each kind of the mixed batch


def strict_inputs(variant, B, n=40, shared=False, steps=True):
    c = SC.mixed_case(B, 64, n)
    d = dict(B=B, n=n, zmax=c["zmax"], zmin=c["zmin"], bstride=2 * n, x0=c["x0"], kick=c["kick"],
             kick_step=n // 2)
    if steps:
        d["kick_steps"] = c["kick_step"]
    _flip(d, variant, ("zmax", "zmin", "x0", "kick", "kick_steps"))
    if shared:   # one benign CoP for every walk: walk 0's boxes widened to hold every start
        zc = (c["zmax"][0] + c["zmin"][0]) / 2
        d.update(zmax=zc + 1.0, zmin=zc - 1.0, bstride=0)
    return d


def strict_oracle(d):
    """The C restatement of the device algorithm (oracle/strict_cpu.py) on the first seven walks."""
    k = min(ORACLE_WALKS, d["B"])
    zmax, zmin = _dense_bounds(d)
    ks = d["kick_steps"][:k] if d.get("kick_steps") is not None else np.full(k, d["kick_step"])
    case = dict(zmax=zmax[:k], zmin=zmin[:k], x0=d["x0"][:k], kick=d["kick"][:k],
                kick_step=np.asarray(ks, np.int64), N=STRICT64[0], dt=STRICT64[1])
    hist, status, _ = SC.restatement(case, threads=min(8, os.cpu_count() or 1))
    assert not status.any()
    return {"hist": hist}


def strict_check(got, want, d):
    # tests/test_gpu_strict_cases.py assert_hist (test_mixed_wave_lq_kernel,
    # test_mixed_wave_scan_kernel): CoM RMSE and relative state error <= 1e-9, every status 0
    assert not got["status"].any()
    k = len(want["hist"])
    r, e = rmse(got["hist"][:k, ..., 0], want["hist"][..., 0]), SC.rel_err(got["hist"][:k],
                                                                             want["hist"])
    assert r <= 1e-9 and e <= 1e-9, (r, e)


def _strict(name, family, solver, B, n=40, bounds=0, kind=None, **kw):
    options = (("strict_solver", solver),) + ((("strict_bounds", bounds),) if bounds else ())
    sym = "zmpc_rollout_kicks" if kw.get("steps", True) else "zmpc_rollout"
    return Case(name, family, (sym,), STRICT64, lambda v: strict_inputs(v, B, n, **kw), _hist_out,
                launch_rollout, options=options,
                dispatch=("strict", (64, 2 * B, solver, 1), (kind,)), oracle=strict_oracle,
                check=strict_check)


def strict_pushed_inputs(variant, B=10, n=24):
    d = strict_inputs(variant, B, n, steps=False)
    D, s, w, amp, _ = pr.strict_pushes(n)[0]
    steps = (np.arange(B, dtype=np.int64) * 3) % (n - 1)
    d.update(amp=np.tile(amp, (B, 1)) * (1.0 + 0.1 * np.arange(B))[:, None], axes=AXIS_X | AXIS_Y,
             steps=steps, profile=w, duration=D)
    return _flip(d, variant, ("amp", "steps"))


def task_queue_inputs(variant, reps=360):
    """tests/test_gpu_push_rollout.py test_lq_task_queue_instance: the 200 mixed walks tiled 360
    times under a rising D = 7 push on xy, each copy's amplitudes scaled differently."""
    base = SC.mixed_case(200)
    w = pr.ramp(7)
    amp1 = np.stack([-base["kick"], base["kick"]], axis=1) / w.sum()
    scale = 1.0 - 0.002 * (np.arange(reps) % 5)
    tile = lambda a: np.tile(a, (reps,) + (1,) * (a.ndim - 1))  # noqa: E731
    d = dict(B=200 * reps, n=40, zmax=tile(base["zmax"]), zmin=tile(base["zmin"]), bstride=80,
             x0=tile(base["x0"]), amp=(amp1[None] * scale[:, None, None]).reshape(-1, 2),
             axes=AXIS_X | AXIS_Y, steps=tile(base["kick_step"]), profile=w, duration=7)
    return _flip(d, variant, ("zmax", "zmin", "x0", "amp", "steps"))


def strict_step_inputs(variant, B=70):
    c = SC.mixed_case(B, 64, 40)
    idx = np.minimum(np.arange(64) + 1, 39)
    d = dict(B=B, x=np.ascontiguousarray(c["x0"][:, 1, :]),
             zmax_win=np.ascontiguousarray(c["zmax"][:, idx, 1]),
             zmin_win=np.ascontiguousarray(c["zmin"][:, idx, 1]))
    return _flip(d, variant, ("x", "zmax_win", "zmin_win"))


def strict_step_oracle(d):
    """The exact box-QP oracle on the first seven windows."""
    return {"x_next": np.stack([SC.solve_window(d["x"][b], d["zmax_win"][b], d["zmin_win"][b], 64,
                                                STRICT64[1])[0] for b in range(ORACLE_WALKS)])}


# ----------------------------------------------------------------------------- metrics and maps

def metrics_inputs(variant, n=65, shared=False, B=9):
    hist, zmax, zmin = mc.random_case(n, shared, B)
    lengths = np.array([max(1, n - 3 * b) for b in range(B)], np.int64)
    d = dict(B=B, n=n, hist=hist, zmax=zmax, zmin=zmin, bstride=0 if shared else 2 * n,
             lengths=lengths)
    return _flip(d, variant, ("hist", "lengths") + (() if shared else ("zmax", "zmin")))


def launch_walk_metrics(lib, h, d, o, s):
    return lib.zmpc_walk_metrics(h, d["B"], d["n"], _ptr(d["hist"]), _ptr(d["zmax"]),
                                 _ptr(d["zmin"]), d["bstride"], _ptr(d.get("lengths")),
                                 _ptr(o["metrics"]), s)


def metrics_oracle(d):
    from mpc_bipedal.analysis import walk_metrics_reference
    return {"metrics": walk_metrics_reference(d["hist"], d["zmax"], d["zmin"], HG, d["lengths"])}


def metrics_check(got, want, d):
    # tests/test_gpu_metrics.py (metrics_cases.assert_metrics): values 1e-12, indices exact
    mc.assert_metrics(got["metrics"], want["metrics"])


def launch_rollout_metrics(lib, h, d, o, s):
    return lib.zmpc_rollout_metrics(h, d["B"], d["n"], _ptr(d["zmax"]), _ptr(d["zmin"]),
                                    d["bstride"], _ptr(d["x0"]), _ptr(d["kick"]), d["kick_step"],
                                    _ptr(d.get("kick_steps")), _ptr(d.get("lengths")),
                                    _ptr(o["metrics"]), _ptr(o["status"]), s)


def rollout_metrics_history(d):
    zmax, zmin = _dense_bounds(d)
    return O.rollout_gain(zmax, zmin, d["x0"], *UNC16[:6], d["kick"], d["kick_step"])


def rollout_metrics_oracle(d):
    from mpc_bipedal.analysis import walk_metrics_reference
    return {"metrics": walk_metrics_reference(rollout_metrics_history(d), d["zmax"], d["zmin"],
                                              HG)}


METRICS_EPS = 1e-11


def discrete_slots_sharp(hist, zmax, zmin, eps=METRICS_EPS):
    """The precondition of comparing counts and indices exactly (assert_sharp of
    tests/test_gpu_rollout_metrics.py), on the oracle's history alone: on every walk and axis no
    sample lies within eps of a bound, and the largest violation is 0 or more than 2·eps ahead
    of the runner-up."""
    B, n = hist.shape[:2]
    for b in range(B):
        hi, lo = (zmax if zmax.ndim == 2 else zmax[b]), (zmin if zmin.ndim == 2 else zmin[b])
        for a in range(2):
            z = hist[b, :, a, 0] - HG * hist[b, :, a, 2]
            raw = np.maximum(z - hi[:, a], lo[:, a] - z)
            if np.count_nonzero(raw > eps) != np.count_nonzero(raw > -eps):
                return False
            v = np.sort(np.maximum(raw, 0.0))
            if not (v[-1] == 0.0 or n == 1 or v[-1] - v[-2] > 2 * eps):
                return False
    return True


def rollout_metrics_check(got, want, d):
    # tests/test_gpu_rollout_metrics.py assert_fused against its expectation A (the NumPy metrics
    # of the oracle's history): value slots to 1e-11 absolute, counts and indices exactly
    # (tests/test_stream_cases_host.py proves discrete_slots_sharp of these inputs first, as that
    # test does of its own)
    assert not got["status"].any()
    for s in mc.EXACT_SLOTS:
        np.testing.assert_array_equal(got["metrics"][:, s], want["metrics"][:, s],
                                      err_msg=f"slot {s}")
    for s in mc.VALUE_SLOTS + mc.RMS_SLOTS:
        np.testing.assert_allclose(got["metrics"][:, s], want["metrics"][:, s], rtol=0,
                                   atol=METRICS_EPS, err_msg=f"slot {s}")


def _metrics_out(d):
    return {"metrics": ((d["B"], 12), F8), "status": ((d["B"],), I4)}


def _rollout_metrics(name, B, n, shared, kind):
    return Case(name, "unc", ("zmpc_rollout_metrics",), UNC16,
                lambda v: unc_inputs(name, v, B, n, shared=shared), _metrics_out,
                launch_rollout_metrics, dispatch=("unc", (16, n, int(shared), 0, 0, 0), (kind,)),
                oracle=rollout_metrics_oracle, check=rollout_metrics_check)


def push_map_inputs(variant, n, B=6, steps=False, D=1, profile=None, axes=AXIS_Y):
    lengths = np.array([min(v, n) for v in (n, n - 1, 3, 2, n, n - 5)][:B], np.int64)
    hist, zmax, zmin = pc.synthetic_case(n, False, B, seed=VARIANTS.index(variant))
    d = dict(B=B, n=n, hist=hist, zmax=zmax, zmin=zmin, bstride=2 * n, lengths=lengths,
             max_violation=0.0, mass=MASS, duration=D, axes=axes, profile=profile)
    if steps:
        d["push_steps"] = np.array([(3 * b + 1) % (n - 2) for b in range(B)], np.int64)
    return d


def _push_map_out(d):
    C = 4 if d["axes"] == (AXIS_X | AXIS_Y) else 2
    shape = (d["B"], C) if d.get("push_steps") is not None else (d["B"], d["n"], C)
    return {"force": (shape, F8), "limit": (shape, I4), "response": ((d["n"],), F8)}


def launch_push_map(lib, h, d, o, s):
    return lib.zmpc_push_map(h, d["B"], d["n"], _ptr(d["hist"]), _ptr(d["zmax"]), _ptr(d["zmin"]),
                             d["bstride"], _ptr(d["lengths"]), _ptr(d.get("push_steps")),
                             d["max_violation"], d["mass"], _ptr(o["force"]), _ptr(o["limit"]),
                             _ptr(o["response"]), s)


def launch_push_map_shaped(lib, h, d, o, s):
    return lib.zmpc_push_map_shaped(h, d["B"], d["n"], _ptr(d["hist"]), _ptr(d["zmax"]),
                                    _ptr(d["zmin"]), d["bstride"], _ptr(d["lengths"]),
                                    _ptr(d.get("push_steps")), _ptr(d.get("profile")),
                                    d["duration"], d["axes"], d["max_violation"], d["mass"],
                                    _ptr(o["force"]), _ptr(o["limit"]), _ptr(o["response"]), s)


def push_map_oracle(d):
    """analysis.push_response with the oracle's gain, shaped; and the map it gives."""
    from mpc_bipedal.analysis import push_map_shaped_reference, push_response, shaped_response
    N, dt = UNC16[:2]
    A, Bv, C = O.lipm(dt, H, G)
    r = push_response(A, Bv, O.gain_row(N, dt, H, G, Q, R)[1], C, dt, MASS, d["n"])
    axes = {1: "x", 2: "y", 3: "xy"}[d["axes"]]
    force, limit = push_map_shaped_reference(
        d["hist"], d["zmax"], d["zmin"], r, HG, d["lengths"], d["max_violation"],
        d.get("push_steps"), d["duration"], d.get("profile"), axes)
    return {"response": shaped_response(r, d["duration"], d.get("profile")), "force": force,
            "limit": limit}


def push_map_check(got, want, d):
    # tests/test_gpu_push_map.py test_response_table: the table within 1e-10 of max|r|; check():
    # NaN and +inf where the statement has them and the finite forces within 1e-12 relative of
    # the statement evaluated with the device's own table
    from mpc_bipedal.analysis import push_map_shaped_reference
    scale = np.abs(want["response"]).max()
    assert np.abs(got["response"] - want["response"]).max() <= 1e-10 * scale
    axes = {1: "x", 2: "y", 3: "xy"}[d["axes"]]
    f, _ = push_map_shaped_reference(d["hist"], d["zmax"], d["zmin"], got["response"], HG,
                                     d["lengths"], d["max_violation"], d.get("push_steps"), 1,
                                     None, axes)
    assert np.array_equal(np.isnan(got["force"]), np.isnan(f))
    assert np.array_equal(np.isposinf(got["force"]), np.isposinf(f))
    assert np.array_equal(np.isnan(f), np.isnan(want["force"]))
    fin = np.isfinite(f)
    assert fin.any() and (got["limit"][~fin] == -1).all()
    rel = np.abs(got["force"][fin] - f[fin]) / np.where(f[fin] > 0, f[fin], 1.0)
    assert rel.max() <= 1e-12, rel.max()


def _push_map(name, shaped, n, **kw):
    return Case(name, "push_map", ("zmpc_push_map_shaped" if shaped else "zmpc_push_map",), UNC16,
                lambda v: push_map_inputs(v, n, **kw), _push_map_out,
                launch_push_map_shaped if shaped else launch_push_map, oracle=push_map_oracle,
                check=push_map_check)


# ----------------------------------------------------------------------------- Herdt

HERDT_N, HERDT_DT = 17, 0.07    # the horizon of the smallest walks of herdt_cases


@functools.lru_cache(maxsize=None)
def herdt_config():
    return hc.make_config(hc.config_kwargs(HERDT_N, HERDT_DT))


def herdt_plan():
    cfg = herdt_config()
    return (cfg.horizon, cfg.dt, cfg.h, cfg.g, 1.0, 1e-6, False)


def herdt_rollout_inputs(variant, B=4, n=12, pushed=False):
    """herdt_cases.rollout_batch at its smallest: 2·B walks of n samples, variant A the first B,
    variant B the rest; one parameter block (the footstep bound of all of them) for both."""
    from mpc_bipedal.controllers import herdt as Hd
    batch = hc.rollout_batch(2 * B, HERDT_N, HERDT_DT, n)
    cfg = hc.make_config(batch["cfg_kw"])
    pad = np.concatenate([batch["states"], np.repeat(batch["states"][:, -1:], HERDT_N, axis=1)],
                         axis=1)
    nb = np.array([[t[0] for t in Hd.find_nb_steps(p)][:n] for p in pad], np.int32)
    sl = slice(0, B) if variant == "A" else slice(B, 2 * B)
    d = dict(B=B, n=n, params=Hd.make_params(cfg, Hd.max_footsteps(pad, HERDT_N, n)),
             v=np.ascontiguousarray(batch["v"][sl]),
             states=np.ascontiguousarray(batch["states"][sl]), nb=np.ascontiguousarray(nb[sl]),
             x0=np.ascontiguousarray(batch["x0"][sl]), kick=np.ascontiguousarray(batch["kick"][sl]),
             kick_step=int(batch["kick_step"]))
    if pushed:
        d.update(amp=np.tile(pr.HERDT_BATCH_AMP, (B, 1)) * (1.0 + 0.25 * np.arange(B))[:, None],
                 axes=AXIS_X | AXIS_Y, steps=pr.herdt_batch_steps(n, 2 * B)[sl].astype(np.int64),
                 profile=ps.half_sine(pr.HERDT_D), duration=pr.HERDT_D)
    return d


def _herdt_out(d):
    return {"hist": ((d["B"], d["n"], 2, 3), F8), "foot": ((d["B"], d["n"], 2), F8),
            "status": ((d["B"],), I4)}


def launch_herdt_rollout(lib, h, d, o, s):
    n = d["n"]
    return lib.zmpc_herdt_rollout(h, ctypes.addressof(d["params"]), d["B"], n, _ptr(d["v"]), 2 * n,
                                  _ptr(d["states"]), n, _ptr(d["nb"]), n, _ptr(d["x0"]),
                                  _ptr(d["kick"]), d["kick_step"], _ptr(o["hist"]),
                                  _ptr(o["foot"]), _ptr(o["status"]), s)


def launch_herdt_rollout_pushed(lib, h, d, o, s):
    n = d["n"]
    push = _push_struct(d)
    return lib.zmpc_herdt_rollout_pushed(h, ctypes.addressof(d["params"]), d["B"], n, _ptr(d["v"]),
                                         2 * n, _ptr(d["states"]), n, _ptr(d["nb"]), n,
                                         _ptr(d["x0"]), ctypes.addressof(push), _ptr(o["hist"]),
                                         _ptr(o["foot"]), _ptr(o["status"]), s)


def herdt_step_inputs(variant, B=12):
    from mpc_bipedal.controllers import herdt as Hd
    case = hc.step_cases(HERDT_N, dt=HERDT_DT, B=75)
    m, _ = hc.case_m(case)
    sl = slice(0, B) if variant == "A" else slice(B, 2 * B)
    take = lambda k: np.ascontiguousarray(case[k][sl])  # noqa: E731
    return dict(B=B, params=Hd.make_params(herdt_config(), int(m[:2 * B].max())), x=take("x"),
                v=take("v"), win=take("win"), cur=take("cur"), foot=take("foot"),
                side=take("side"))


def launch_herdt_step(lib, h, d, o, s):
    return lib.zmpc_herdt_step(h, ctypes.addressof(d["params"]), d["B"], _ptr(d["x"]),
                               _ptr(d["v"]), _ptr(d["win"]), _ptr(d["cur"]), _ptr(d["foot"]),
                               _ptr(d["side"]), _ptr(o["x_next"]), _ptr(o["step"]),
                               _ptr(o["status"]), s)


def herdt_metrics_inputs(variant, n=65):
    c = hm.emu_case(n, False, "walk")
    d = dict(B=hm.EMU_B, n=n, params=hm.make_params(), hist=c["hist"], foot=c["foot"],
             states=c["states"], foot_ref=c["foot_ref"],
             lengths=np.array([n, n - 1, 64, 2, n], np.int64), count_tol=hm.COUNT_TOL)
    return _flip(d, variant, ("hist", "foot", "states", "foot_ref", "lengths"))


def launch_herdt_metrics(lib, h, d, o, s):
    n = d["n"]
    return lib.zmpc_herdt_walk_metrics(h, ctypes.addressof(d["params"]), d["B"], n,
                                       _ptr(d["hist"]), _ptr(d["foot"]), _ptr(d["states"]), n,
                                       _ptr(d["foot_ref"]), 2 * n, _ptr(d["lengths"]),
                                       d["count_tol"], _ptr(o["metrics"]), s)


def herdt_metrics_oracle(d):
    return {"metrics": hm.reference(dict(hist=d["hist"], foot=d["foot"], states=d["states"],
                                         foot_ref=d["foot_ref"], lengths=d["lengths"]),
                                    hg=herdt_config().h / herdt_config().g)}


def herdt_metrics_check(got, want, d):
    # tests/test_gpu_herdt_metrics.py (herdt_metrics_cases.assert_close): integer slots exact,
    # the others 1e-12 relative
    hm.assert_close(got["metrics"], want["metrics"])


# ----------------------------------------------------------------------------- the rest

def cop_inputs(variant, B=5):
    """Producer parameters of B short walks (distance, step_length, foot_spread, ssp, dsp,
    standing, dt); n_cap holds the longest of both variants."""
    k = np.arange(B) + (0 if variant == "A" else B)
    p = np.stack([0.3 + 0.05 * k, 0.1 + 0.01 * (k % 3), 0.1 + 0.005 * k, 0.3 + 0.02 * (k % 4),
                  0.1 + 0.01 * (k % 2), 0.2 + 0.0 * k, np.full(len(k), 0.01)], axis=1)
    return dict(B=B, params=np.ascontiguousarray(p), n_cap=700)


def _cop_out(d):
    return {"zmax": ((d["B"], d["n_cap"], 2), F8), "zmin": ((d["B"], d["n_cap"], 2), F8),
            "states": ((d["B"], d["n_cap"]), I1), "n_out": ((d["B"],), I8)}


def launch_cop(lib, h, d, o, s):
    return lib.zmpc_cop_generate(d["device"], d["B"], _ptr(d["params"]), d["n_cap"],
                                 _ptr(o["zmax"]), _ptr(o["zmin"]), _ptr(o["states"]),
                                 _ptr(o["n_out"]), s)


def cop_oracle(d):
    """The host generator walk by walk (generators/cop_generator.py, the reference's own loop)."""
    from mpc_bipedal.config import MPCConfig
    from mpc_bipedal.generators import CoPGenerator, State
    code = {State.STANDING: 0, State.DOUBLE_SUPPORT: 1, State.SINGLE_SUPPORT: 2}
    B, cap = d["B"], d["n_cap"]
    zmax, zmin = np.empty((B, cap, 2)), np.empty((B, cap, 2))
    states, n_out = np.full((B, cap), -1, np.int8), np.empty(B, np.int64)
    for b, p in enumerate(d["params"]):
        cfg = MPCConfig(distance=float(p[0]), step_length=float(p[1]), foot_spread=float(p[2]),
                        ssp_duration=float(p[3]), dsp_duration=float(p[4]),
                        standing_duration=float(p[5]), dt=float(p[6]))
        hx, hn, hs = CoPGenerator(cfg).generate_cop_trajectory()
        nb = len(hx)
        assert 0 < nb <= cap, (b, nb)
        zmax[b, :nb], zmax[b, nb:], zmin[b, :nb], zmin[b, nb:] = hx, hx[-1], hn, hn[-1]
        states[b, :nb], n_out[b] = [code[s] for s in hs], nb
    return dict(zmax=zmax, zmin=zmin, states=states, n_out=n_out)


def cop_check(got, want, d):
    # tests/test_gpu_parity.py test_device_cop_producer_bit_exact: bounds, states, sample counts
    # and padding rows bit for bit
    for k in ("zmax", "zmin", "states", "n_out"):
        assert np.array_equal(got[k], want[k]), k


PLAN_CREATE = {"A": (24, False), "B": (33, True)}
PLAN_EXPORTS = (0, 1, 2, 3, 4, 6, 8, 9, 10, 13, 14)   # what every plan holds
STRICT_EXPORTS = (5, 7, 11, 12)


def plan_create_inputs(variant):
    N, strict = PLAN_CREATE[variant]
    return dict(N=N, strict=strict, dt=0.01)


def launch_plan_create(lib, h, d, o, s):
    """zmpc_plan_create on `stream`; the plan's handle lands in o["_handle"] (a c_void_p the
    caller exports from and destroys)."""
    from mpc_bipedal.models.lipm_model import plan_constants
    c = plan_constants(d["dt"], H, G)
    return lib.zmpc_plan_create(d["device"], d["N"], c["T"], c["T2_2"], c["T3_6"], c["hg"],
                                c["Thg"], Q, R, int(d["strict"]), s, ctypes.byref(o["_handle"]))


def prepare_rollout_launcher(plan, d, o):
    return plan.rollout_launcher(d["zmax"], d["zmin"], d["x0"], kick=d["kick"],
                                 kick_step=d["kick_step"], hist=o["hist"], status=o["status"])


def prepare_rollout_metrics_launcher(plan, d, o):
    return plan.rollout_metrics_launcher(d["zmax"], d["zmin"], d["x0"], kick=d["kick"],
                                         kick_step=d["kick_step"], out=o["metrics"],
                                         status=o["status"])


def prepare_herdt_launcher(plan, d, o):
    from mpc_bipedal.analysis import Push
    a = np.asarray(pr.HERDT_BATCH_AMP, np.float64)
    cfg = herdt_config()
    push = Push(np.full(d["B"], np.hypot(a[0], a[1]) * cfg.m / cfg.dt), a[None],
                d["steps_host"], duration=pr.HERDT_D, profile=ps.half_sine(pr.HERDT_D))
    return plan.herdt_rollout_launcher(d["params"], d["v"], d["states"], d["nb"], d["x0"], push,
                                       cfg.m, hist=o["hist"], foot=o["foot"], status=o["status"])


def herdt_launcher_inputs(variant):
    d = herdt_rollout_inputs(variant)
    d.pop("kick")
    # (host data of the push: the launcher's own copy of it is made once, in prepare)
    d["steps_host"] = tuple(int(s) for s in pr.herdt_batch_steps(d["n"], 8)[:d["B"]])
    return d


def fire_prepared(lib, h, d, o, s):
    d["_prep"]()     # the closure looks the current stream up itself
    return 0


def _build():
    cases = [
        # unconstrained zmpc_rollout, one case per kernel of csrc/dispatch.h choose_unc
        _unc("unc_copy", UNC16, (), "Copy", 5, 1, (16, 1, 0, 0, 0, 0)),
        _unc("unc_split_sparse", UNC16, (), "Split", 5, 16, (16, 16, 0, 0, 0, 0)),
        _unc("unc_split_dense_cw3", UNC16, (("correlation", 1),), "Split", 3, 150,
             (16, 150, 0, 0, 0, 1), dense=True),
        _unc("unc_split_shared", UNC16, (), "SplitShared", 3, 23, (16, 23, 1, 0, 0, 0),
             shared=True),
        _unc("unc_generic", UNC16, (("rollout_kernel", 1),), "Generic", 5, 16,
             (16, 16, 0, 1, 0, 0)),
        _unc("unc_wide_direct", UNC16, (("correlation", 1),), "Wide", 3, 520,
             (16, 520, 0, 0, 0, 1), dense=True),
        _unc("unc_wide_fft", UNC150, (("long_walk", 2),), "Wide", 3, 1100,
             (150, 1100, 0, 0, 2, 0), dense=True),
        _unc("unc_wide_sparse", UNC16, (), "Wide", 3, 520, (16, 520, 0, 0, 0, 0), seg=10),
        _unc("unc_chunk", UNC16, (("long_walk", 3),), "Chunk", 3, 700, (16, 700, 0, 0, 3, 0),
             dense=True),
        _unc("unc_kicks", UNC16, (), "Split", 5, 16, (16, 16, 0, 0, 0, 0), steps=True),
        Case("unc_pushed", "unc", ("zmpc_rollout_pushed",), UNC16,
             lambda v: unc_pushed_inputs("unc_pushed", v), _hist_out, launch_rollout_pushed,
             dispatch=("unc", (16, 23, 0, 0, 0, 0), ("Split",)), oracle=unc_pushed_oracle,
             check=unc_pushed_check),
        # zmpc_step
        Case("step_unc", "unc", ("zmpc_step",), UNC16, lambda v: unc_step_inputs("step_unc", v),
             _step_out, launch_step, oracle=unc_step_oracle, check=step_check),
        Case("step_lq", "strict_lq", ("zmpc_step",), STRICT64, strict_step_inputs, _step_out,
             launch_step, options=(("strict_solver", 3), ("strict_bounds", 2)),
             dispatch=("strict", (64, 70, 3, 1), ("Lq",)), oracle=strict_step_oracle,
             check=step_check),
        Case("step_scan", "strict_scan", ("zmpc_step",), STRICT64, strict_step_inputs, _step_out,
             launch_step, options=(("strict_solver", 4),),
             dispatch=("strict", (64, 70, 4, 1), ("Scan",)), oracle=strict_step_oracle,
             check=step_check),
        # strict zmpc_rollout on the mixed batch
        _strict("strict_tile", "strict_chol", 1, 10, kind="Tile"),
        _strict("strict_wave", "strict_chol", 2, 10, kind="Wave"),
        _strict("strict_lq_kicks_rows", "strict_lq", 3, 200, bounds=1, kind="Lq"),
        _strict("strict_lq_kicks_runs", "strict_lq", 3, 200, bounds=2, kind="Lq"),
        _strict("strict_lq_shared", "strict_lq", 3, 70, n=24, bounds=2, kind="Lq", shared=True,
                steps=False),
        Case("strict_lq_task_queue", "strict_lq", ("zmpc_rollout_pushed",), STRICT64,
             task_queue_inputs, _hist_out, launch_rollout_pushed,
             options=(("strict_solver", 3), ("strict_bounds", 2)),
             dispatch=("strict", (64, 144000, 3, 1), ("Lq",))),
        _strict("strict_scan_wave", "strict_scan", 4, 40, kind="Scan"),
        _strict("strict_scan_32", "strict_scan", 4, 1200, kind="Scan"),
        Case("strict_lq_pushed", "strict_lq", ("zmpc_rollout_pushed",), STRICT64,
             strict_pushed_inputs, _hist_out, launch_rollout_pushed,
             options=(("strict_solver", 3), ("strict_bounds", 2)),
             dispatch=("strict", (64, 20, 3, 1), ("Lq",))),
        Case("strict_scan_pushed", "strict_scan", ("zmpc_rollout_pushed",), STRICT64,
             strict_pushed_inputs, _hist_out, launch_rollout_pushed,
             options=(("strict_solver", 4),), dispatch=("strict", (64, 20, 4, 1), ("Scan",))),
        # metrics and maps
        Case("walk_metrics", "unc", ("zmpc_walk_metrics",), UNC16, metrics_inputs,
             lambda d: {"metrics": ((d["B"], 12), F8)}, launch_walk_metrics,
             oracle=metrics_oracle, check=metrics_check),
        _rollout_metrics("rollout_metrics_sample0", 5, 1, False, "Copy"),
        _rollout_metrics("rollout_metrics_split", 5, 16, False, "Split"),
        _rollout_metrics("rollout_metrics_shared", 3, 23, True, "SplitShared"),
        _push_map("push_map_full", False, 66),
        _push_map("push_map_steps", False, 66, steps=True),
        _push_map("push_map_shaped_y", True, 33, D=3, profile=pr.ramp(3)),
        _push_map("push_map_shaped_xy", True, 33, B=5, D=5, profile=ps.half_sine(5),
                  axes=AXIS_X | AXIS_Y),
        # Herdt
        Case("herdt_step", "herdt", ("zmpc_herdt_step",), herdt_plan(), herdt_step_inputs,
             lambda d: {"x_next": ((d["B"], 2, 3), F8), "step": ((d["B"], 2), F8),
                        "status": ((d["B"],), I4)}, launch_herdt_step),
        Case("herdt_rollout", "herdt", ("zmpc_herdt_rollout",), herdt_plan(), herdt_rollout_inputs,
             _herdt_out, launch_herdt_rollout),
        Case("herdt_rollout_pushed", "herdt", ("zmpc_herdt_rollout_pushed",), herdt_plan(),
             lambda v: herdt_rollout_inputs(v, B=3, n=15, pushed=True), _herdt_out,
             launch_herdt_rollout_pushed),
        Case("herdt_walk_metrics", "herdt", ("zmpc_herdt_walk_metrics",), herdt_plan(),
             herdt_metrics_inputs, lambda d: {"metrics": ((d["B"], 16), F8)}, launch_herdt_metrics,
             oracle=herdt_metrics_oracle, check=herdt_metrics_check),
        # the rest
        Case("cop_generate", "rest", ("zmpc_cop_generate",), None, cop_inputs, _cop_out,
             launch_cop, oracle=cop_oracle, check=cop_check),
        Case("plan_create", "rest", ("zmpc_plan_create",), None, plan_create_inputs,
             lambda d: {}, launch_plan_create,
             blocking="zmpc_plan_create synchronises its stream before it returns (zmpc.h: "
                      "\"stream-ordered on `stream`, then synchronised\"): the build reads the "
                      "factorisation's status back to decide whether the plan exists"),
        Case("launcher_rollout", "unc", ("zmpc_rollout",), UNC16,
             lambda v: unc_inputs("launcher_rollout", v, 5, 16), _hist_out, fire_prepared,
             prepare=prepare_rollout_launcher, oracle=unc_oracle(UNC16), check=unc_check),
        Case("launcher_rollout_metrics", "unc", ("zmpc_rollout_metrics",), UNC16,
             lambda v: unc_inputs("launcher_rollout_metrics", v, 5, 16), _metrics_out,
             fire_prepared, prepare=prepare_rollout_metrics_launcher,
             oracle=rollout_metrics_oracle, check=rollout_metrics_check),
        Case("launcher_herdt_rollout", "herdt", ("zmpc_herdt_rollout_pushed",), herdt_plan(),
             herdt_launcher_inputs, _herdt_out, fire_prepared, prepare=prepare_herdt_launcher),
    ]
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return {c.name: c for c in cases}


CASES = _build()

# negative controls (a launch issued under the default stream while A is still being produced):
# the split, strict LQ and push-map cases
CONTROLS = ("unc_split_sparse", "strict_lq_kicks_runs", "push_map_full")

# two streams, one plan: (case X with variant A, a case of the same plan with another n and
# another B, and where the path has them another duration or axis set, with variant B), one pair
# per family
PAIRS = (("unc_split_sparse", "unc_split_shared"),
         ("strict_lq_kicks_runs", "strict_lq_shared"),
         ("strict_scan_wave", "strict_scan_pushed"),
         ("push_map_full", "push_map_shaped_xy"),
         ("herdt_rollout", "herdt_rollout_pushed"))

# Cases with no plain reference here: their serial result is held to launch-to-launch bit equality,
# status 0, finite histories and A != B, and the arithmetic of their paths is pinned elsewhere.
# The C restatement of the strict solver (oracle/strict_cpu.py) takes one kick and no shove, and
# the exact loop under a shove (push_rollout_cases.strict_walk) is held to 1e-9 only on the
# rollout families, whose response to a 1e-12 change of x0 the host test measures first; on the
# mixed batch's degenerate walks no such bar is established.  The Herdt paths are pinned against
# their oracle in tests/test_gpu_herdt*.py and tests/test_gpu_push_rollout.py; a created plan is
# compared with a plan created serially (test_contended_first_creation_in_a_fresh_process).
NO_REFERENCE = ("strict_lq_pushed", "strict_scan_pushed", "strict_lq_task_queue", "herdt_step",
                "herdt_rollout", "herdt_rollout_pushed", "launcher_herdt_rollout", "plan_create")

# two host threads: thread 1 and thread 2 alternate between a strict and an unconstrained case
# each, on the two plans they share
THREAD_CASES = (("strict_lq_kicks_runs", "unc_split_sparse"),
                ("strict_lq_shared", "unc_split_shared"))


UNCACHED = ("strict_lq_task_queue",)   # 72 000 walks, some 150 MB a variant: built when asked for


@functools.lru_cache(maxsize=None)
def _inputs(name, variant):
    d = CASES[name].make(variant)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def inputs(name, variant):
    """make(variant) of a case, built once and kept (the cases of UNCACHED: built at every call
    and not kept); callers must not write into the arrays."""
    return (_inputs.__wrapped__ if name in UNCACHED else _inputs)(name, variant)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle of variant A, computed once (None where the case has none)."""
    case = CASES[name]
    return None if case.oracle is None else case.oracle(inputs(name, "A"))


def fire(case, lib, handle, d, o):
    """One launch of a case on torch's current stream; raises on a nonzero return code."""
    import torch
    from mpc_bipedal import _native
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = case.launch(lib, handle, d, o, stream)
    if rc != 0:
        _native.check(rc, case.name)
