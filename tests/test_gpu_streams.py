"""The stream and thread contract of include/zmpc.h on the device: "calls are asynchronous on
`stream`", "zmpc_last_error() returns a thread-local message", "a plan ... may be shared across
threads and streams of its device".  Every stream-taking entry point of the registry
tests/stream_cases.py (tests/test_stream_cases_host.py proves the registry on the CPU):

  serial  variants A and B on the default stream, synchronised; A against the plain reference of
          the path at the bar of its existing device test
  a       on a side stream that is held back by a bounded delay: the call returns while its
          inputs do not exist yet, and computes serial A bit for bit once they do
  b       negative control: the same construction with the launch on the default stream computes
          on the stale inputs (serial B), so (a) does catch a launch on the wrong stream (run in
          a fresh child process: their docstring says why)
  c       two held-back streams, one plan, two shapes: each result its own serial one, and the
          plan's work counters the sum (maxima: the maximum) of the two serial launches
  d       two host threads on shared plans, one of them making a rejected call: results serial,
          the other thread's zmpc_last_error() stays ""; two threads asking for the same cached
          plan
  e       two threads creating the first two plans of a fresh process at once

How a stream is held back: ordinary torch work — in-place elementwise passes over a 1 GiB
tensor, timed once with events — is enqueued on a fresh non-blocking side stream, then
device-to-device copies of variant A into input buffers that hold variant B, then the launch.
Outputs start as NaN (-77 for integers).  A launch, memset or copy of the chain that went to the
null stream, or work done at call time, meets B or is overwritten, and a call that waits for its
stream finds the stream idle afterwards.  Nothing here provokes a fault: every input is valid
and finite.

Bitwise comparison: the suite already asserts launch-to-launch bit equality of these kernels
(test_two_launches_agree_bitwise in tests/test_gpu_metrics.py, test_gpu_push_map.py and
test_gpu_rollout_metrics.py, test_lq_task_queue_instance in tests/test_gpu_push_rollout.py); the
serial fixture asserts it again for every case (two launches of A).
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import threading
import time
import types

import numpy as np
import pytest
import torch

import stream_cases as S
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

from mpc_bipedal import _native  # noqa: E402
from mpc_bipedal.solver import Plan, clear_plan_cache, get_plan  # noqa: E402

NAMES = sorted(S.CASES)
DELAY_FACTOR = 10       # the delay is this many times the slowest enqueue ...
DELAY_MIN_MS = 20.0     # ... at least this (host jitter on a shared machine) ...
DELAY_MAX_MS = 100.0    # ... and at most this
DTYPES = {S.F8: torch.float64, S.I4: torch.int32, S.I8: torch.int64, S.I1: torch.int8}
_PLANS = {}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    _native.load()
    yield
    torch.cuda.synchronize()
    for p in _PLANS.values():
        p.destroy()
    _PLANS.clear()


# ----------------------------------------------------------------------------- plumbing

def plan_of(case):
    """The plan a case shares with every case of the same (parameters, options); the options are
    set once, before the plan is used (zmpc.h: set_option belongs before a plan is shared)."""
    key = case.plan_key
    if key is None:
        return None
    if key not in _PLANS:
        p = Plan(torch.cuda.current_device(), *case.plan)
        for name, value in case.options:
            p.set_option(name, value)
        _PLANS[key] = p
    return _PLANS[key]


def handle_of(case):
    p = plan_of(case)
    return None if p is None else p.handle


def to_device(d):
    """The inputs on the device (arrays become tensors; scalars and parameter blocks stay)."""
    out = {k: (torch.tensor(v, device="cuda") if isinstance(v, np.ndarray) else v)
           for k, v in d.items()}
    out["device"] = torch.cuda.current_device()
    return out


def blank(o):
    for k, t in o.items():
        if isinstance(t, torch.Tensor):
            t.fill_(float("nan") if t.dtype.is_floating_point else -77)


def fresh_outputs(case, d):
    if case.name == "plan_create":
        return {"_handle": ctypes.c_void_p()}
    o = {k: torch.empty(shape, dtype=DTYPES[dt], device="cuda")
         for k, (shape, dt) in case.outputs(d).items()}
    blank(o)
    return o


def prepare(case, d, o):
    if case.prepare is not None:
        d["_prep"] = case.prepare(plan_of(case), d, o)


def collect(case, o, d=None):
    """What a finished launch produced, as tensors to compare; a created plan is exported (every
    table it holds) and destroyed here."""
    if case.name != "plan_create":
        return {k: t.clone() for k, t in o.items()}
    lib, h = _native.load(), o["_handle"]
    assert h.value
    try:
        return plan_tables(lib, h, d["N"], d["strict"])
    finally:
        lib.zmpc_plan_destroy(h)
        o["_handle"] = ctypes.c_void_p()


def plan_tables(lib, h, N, strict):
    out = {}
    for what in S.PLAN_EXPORTS + (S.STRICT_EXPORTS if strict else ()):
        buf = np.empty(_native.EXPORTS[what][1](N), np.float64)
        rc = lib.zmpc_plan_export(h, what, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                  len(buf))
        _native.check(rc, "zmpc_plan_export")
        out[f"export{what}"] = torch.from_numpy(buf)
    return out


def same_bits(a, b):
    if a.dtype.is_floating_point:
        a, b = a.view(torch.int64), b.view(torch.int64)
    return a.shape == b.shape and bool(torch.equal(a, b))


def assert_same(got, want, what):
    assert got.keys() == want.keys(), what
    for k in want:
        assert same_bits(got[k], want[k].to(got[k].device)), (what, k)


def differs(got, want):
    return any(not same_bits(got[k], want[k]) for k in want)


def counters_of(case, reset=True):
    p = plan_of(case)
    if p is None:
        return None
    c = p.counters(reset=reset)
    return [c[k] for k in _native.COUNTER_NAMES]


class Delay:
    """A bounded delay out of ordinary torch work: in-place elementwise passes over 1 GiB."""

    def __init__(self):
        self.buf = torch.zeros(256 * 1024 * 1024, dtype=torch.float32, device="cuda")
        for _ in range(3):
            self.buf.add_(1.0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            self.buf.add_(1.0)
        e1.record()
        torch.cuda.synchronize()
        self.ms_per_pass = e0.elapsed_time(e1) / 20

    def enqueue(self, ms):
        """At least `ms` of work on the current stream."""
        for _ in range(int(np.ceil(ms / self.ms_per_pass))):
            self.buf.add_(1.0)


class Serial:
    """Every case on the default stream: results of A and B, counters, enqueue times."""

    def __init__(self):
        lib = _native.load()
        self.out, self.cnt, self.host_us = {}, {}, {}
        for name in NAMES:
            case = S.CASES[name]
            h = handle_of(case)
            for v in S.VARIANTS:
                d = to_device(S.inputs(name, v))
                o = fresh_outputs(case, d)
                prepare(case, d, o)
                torch.cuda.synchronize()
                S.fire(case, lib, h, d, o)        # (first call: code objects load here)
                torch.cuda.synchronize()
                first = collect(case, o, d)
                blank(o)
                counters_of(case)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                S.fire(case, lib, h, d, o)
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                self.out[name, v] = collect(case, o, d)
                self.cnt[name, v] = counters_of(case)
                self.host_us[name, v] = (t1 - t0) * 1e6
                # two identical launches agree bit for bit: what the bitwise bars below rest on
                assert_same(first, self.out[name, v], (name, v, "launch to launch"))
        free = [k for k in self.host_us if S.CASES[k[0]].blocking is None]
        slow = max(free, key=lambda k: self.host_us[k])
        self.slowest = (slow, self.host_us[slow])
        self.delay_ms = min(DELAY_MAX_MS, max(DELAY_MIN_MS,
                                              DELAY_FACTOR * self.host_us[slow] / 1e3))
        self.delays = (Delay(), Delay())
        print(f"MEASURED slowest enqueue {slow[0]} ({slow[1]}): {self.host_us[slow]:.0f} us of "
              f"host time; delay {self.delay_ms:.1f} ms; one delay pass "
              f"{self.delays[0].ms_per_pass:.3f} ms")
        for k in sorted(self.host_us, key=lambda k: -self.host_us[k])[:8]:
            print(f"MEASURED enqueue {k[0]} {k[1]}: {self.host_us[k]:.0f} us")


@pytest.fixture(scope="module")
def serial():
    return Serial()


class Held:
    """One case on one side stream: buffers that hold variant `stale`, staged variant `fresh`,
    NaN outputs, the case warmed once on the stream (pool growth does not count as blocking)."""

    def __init__(self, case, fresh="A", stale="B", side=None, warm_on=None):
        self.case, self.lib, self.h = case, _native.load(), handle_of(case)
        self.side = torch.cuda.Stream() if side is None else side
        self.d = to_device(S.inputs(case.name, stale))
        self.stage = to_device(S.inputs(case.name, fresh))
        if case.name == "plan_create":   # (its inputs are arguments: there is nothing to stage)
            self.d = self.stage
        self.o = fresh_outputs(case, self.d)
        prepare(case, self.d, self.o)
        torch.cuda.synchronize()
        with torch.cuda.stream(self.side if warm_on is None else warm_on):
            S.fire(case, self.lib, self.h, self.d, self.o)
        torch.cuda.synchronize()
        collect(case, self.o, self.d)
        blank(self.o)
        torch.cuda.synchronize()

    def hold(self, delay, ms):
        with torch.cuda.stream(self.side):
            delay.enqueue(ms)

    def stage_inputs(self):
        """The copies of the fresh variant into the input buffers, on the side stream."""
        with torch.cuda.stream(self.side):
            for k, t in self.stage.items():
                if isinstance(t, torch.Tensor) and self.d[k] is not t:
                    self.d[k].copy_(t, non_blocking=True)

    def launch(self, stream=None):
        """The launch under `stream` (default: the side stream) → whether the side stream was
        still busy when the call returned."""
        with torch.cuda.stream(self.side if stream is None else stream):
            S.fire(self.case, self.lib, self.h, self.d, self.o)
            return not self.side.query()

    def result(self):
        self.side.synchronize()
        torch.cuda.synchronize()
        return collect(self.case, self.o, self.d)


# ----------------------------------------------------------------------------- serial

@pytest.mark.parametrize("name", NAMES)
def test_serial_result_against_reference(serial, name):
    """The serial results the other tests compare with: every output written (no NaN or
    sentinel left where the reference has a value), A and B different, and A against the plain
    reference of the path (stream_cases.reference; each case's check names the existing test
    whose bar it takes)."""
    case = S.CASES[name]
    a, b = serial.out[name, "A"], serial.out[name, "B"]
    assert differs(a, b), "variants A and B give the same result"
    for k, t in a.items():
        if k == "status":
            assert not t.any(), (k, t.unique())
    want = S.reference(name)
    if want is not None:
        case.check({k: t.cpu().numpy() for k, t in a.items()}, want, S.inputs(name, "A"))
    elif "hist" in a:
        assert torch.isfinite(a["hist"]).all()


# ----------------------------------------------------------------------------- b: control

CONTROL_TRIES = 8

CONTROL_CHILD = r"""
import sys
sys.path[:0] = [{tests!r}, {root!r}, {pkg!r}]
import test_gpu_streams
test_gpu_streams.control_main({device!r})
"""


def digest(outs):
    """One hash over the bits of every output of a launch."""
    h = hashlib.sha256()
    for k in sorted(outs):
        h.update(k.encode())
        h.update(outs[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def control_rounds(name, delay):
    """The negative control of one case, in the child process: A is produced on the delayed side
    stream, the launch goes to the default stream.  A round shows something only if the default
    stream finished at least 10 ms ahead of the held side stream; otherwise it is repeated on a
    fresh side stream.  → what the launch produced in the first round that shows something."""
    case = S.CASES[name]
    log = []
    for attempt in range(CONTROL_TRIES):
        run = Held(case, warm_on=torch.cuda.default_stream())
        t0 = time.perf_counter()
        run.hold(delay, DELAY_MAX_MS)
        run.stage_inputs()
        busy = run.launch(stream=torch.cuda.default_stream())
        torch.cuda.default_stream().synchronize()
        t1 = time.perf_counter()
        still = not run.side.query()
        got = {k: t.clone() for k, t in run.o.items()}
        run.side.synchronize()
        t2 = time.perf_counter()
        torch.cuda.synchronize()
        log.append(f"round {attempt}: default stream done after {1e3 * (t1 - t0):.2f} ms, "
                   f"side stream after {1e3 * (t2 - t0):.2f} ms")
        if not busy:
            return dict(busy=False, clear=False, log=log)
        if still and t2 - t1 >= 10e-3:
            return dict(busy=True, clear=True, got=digest(got), log=log)
    return dict(busy=True, clear=False, log=log)


def control_main(device):
    """The child process of the negative controls: every control case, one after the other."""
    torch.cuda.set_device(device)
    _native.load()
    try:
        delay = Delay()
        out = {name: control_rounds(name, delay) for name in S.CONTROLS}
    finally:
        torch.cuda.synchronize()
    print("RESULT " + json.dumps(out))


@pytest.fixture(scope="module")
def controls():
    """The negative controls run in one fresh child process (subprocess.run with a timeout, the
    program after `python`): there the stream-ordered pool holds no workspace block that a side
    stream freed, whatever ran before this test in the session."""
    code = CONTROL_CHILD.format(tests=os.path.join(ROOT, "tests"), root=ROOT, pkg=PKG,
                                device=torch.cuda.current_device())
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, r.stdout[-2000:]
    return json.loads(line[-1][len("RESULT "):])


@pytest.mark.parametrize("name", S.CONTROLS)
def test_negative_control_default_stream_launch_sees_stale_inputs(serial, controls, name):
    """The harness itself makes the mistake (a) is there to catch: A is produced on the delayed
    side stream, the launch goes to the default stream.  It computes on what the buffers hold, B:
    the result differs from serial A and equals serial B.  Valid finite inputs throughout.

    The control shows something only if the default stream's work finishes while the side stream
    is still held, by a clear margin.  Three things can prevent that, none of them the library's
    doing, all measured:
      - the runtime spreads its streams over a few hardware queues (four by default): when the
        held stream and the default stream share one, the default stream's kernels run behind
        the delay (two of six fresh side streams in one measurement);
      - a chain of many small kernels — the kick order's key kernel and radix sort before the LQ
        solve — competes with the delay's passes for the device: 13 to 20 ms on a chain that
        takes 1.5 ms alone;
      - a workspace block of the stream-ordered pool that was last freed on another stream makes
        the launch wait for what that stream has queued.
    The third is excluded by construction: the controls run in a fresh child process that
    launches on the default stream alone (control_main).  For the other two the control uses the
    longest delay, and repeats a round in which the default stream did not finish at least 10 ms
    ahead of the side stream on a fresh side stream (control_rounds); the comparison is made in
    the first round that shows something."""
    res = controls[name]
    for ln in res["log"]:
        print(f"MEASURED control {name} {ln}")
    assert res["busy"], "the delay ended before the launch had returned"
    assert res["clear"], (f"in {CONTROL_TRIES} rounds the default stream never finished clear of "
                          "the held side stream")
    assert res["got"] != digest(serial.out[name, "A"])
    assert res["got"] == digest(serial.out[name, "B"]), name


# ----------------------------------------------------------------------------- a: held back

@pytest.mark.parametrize("name", NAMES)
def test_side_stream_held_back(serial, name):
    """The call returns while the side stream is still busy with work enqueued before it — its
    inputs do not exist yet — and the result is serial A bit for bit.  A case marked `blocking`
    (its reason is in the registry and in zmpc.h) is only held to the result."""
    case = S.CASES[name]
    try:
        run = Held(case)
        run.hold(serial.delays[0], serial.delay_ms)
        run.stage_inputs()
        busy = run.launch()
        if case.blocking is None:
            assert busy, "the call waited for its stream (or the delay was too short)"
        assert_same(run.result(), serial.out[name, "A"], name)
    finally:
        torch.cuda.synchronize()


# ----------------------------------------------------------------------------- c: two streams

@pytest.mark.parametrize("x,y", S.PAIRS, ids=[S.CASES[x].family for x, _ in S.PAIRS])
def test_two_streams_one_plan(serial, x, y):
    """Case x (variant A) and a case of the same plan with another shape (variant B) on two
    held-back streams, both enqueued before either can start: each equals its own serial
    result bit for bit, and the plan's counters are the sum ([8..9]: the maximum) of the two
    serial launches.  This catches per-call state kept in the plan (tables keyed on n, queues,
    scratch).  It cannot prove the absence of a data race: two launches that share state may
    still happen to run one after the other, or race without changing a bit."""
    cx, cy = S.CASES[x], S.CASES[y]
    assert plan_of(cx) is plan_of(cy)
    try:
        rx, ry = Held(cx, "A", "B"), Held(cy, "B", "A")
        counters_of(cx)
        rx.hold(serial.delays[0], serial.delay_ms)
        ry.hold(serial.delays[1], serial.delay_ms)
        rx.stage_inputs()
        bx = rx.launch()
        ry.stage_inputs()
        by = ry.launch()
        both = not rx.side.query() and not ry.side.query()
        assert bx and by and both, "a call waited for its stream (or the delay was too short)"
        got_x, got_y = rx.result(), ry.result()
        assert_same(got_x, serial.out[x, "A"], x)
        assert_same(got_y, serial.out[y, "B"], y)
        if cx.plan[6] or cx.family == "herdt":
            c, sx, sy = counters_of(cx), serial.cnt[x, "A"], serial.cnt[y, "B"]
            assert sum(sx[:8]) + sum(sy[:8]) > 0
            assert c[:8] == [p + q for p, q in zip(sx[:8], sy[:8])], (c, sx, sy)
            assert c[8:10] == [max(p, q) for p, q in zip(sx[8:10], sy[8:10])], (c, sx, sy)
    finally:
        torch.cuda.synchronize()


# ----------------------------------------------------------------------------- d: two threads

def test_two_host_threads_share_plans(serial):
    """Two Python threads, each under its own side stream, three rounds over one shared strict
    plan and one shared unconstrained plan with different cases per thread: every result serial A
    bit for bit.  Thread 0 makes two calls the library itself rejects and reads their messages:
    zmpc_rollout_kicks without kick_steps (ZMPC_EINVAL; the bad calls of
    tests/python_errors_cases.py are all caught by the Python layer before they reach the library,
    so this one is made at the C-ABI, as tests/test_host.py makes it) and that table's
    "export/not_held" (ZMPC_ESTATE, with the recorded text).

    Every entry point clears the message when it is entered, so a message that was one global
    would show only to a thread that reads it with no call of its own since.  The threads are
    therefore ordered by barriers, in every round:
      1  both threads have launched (and read "")
         thread 0 makes its rejected calls and reads its messages
      2  thread 1 reads zmpc_last_error() with no call of its own since barrier 1: still ""
         thread 1 launches again, successfully
      3  thread 0 reads zmpc_last_error() with no call of its own since barrier 2: still its own
         message
    Both readings fail every time if the message is shared between the threads."""
    import python_errors_cases as pe
    lib = _native.load()
    device = torch.cuda.current_device()
    not_held = dict(pe.rows())["export/not_held"]
    with open(os.path.join(ROOT, "tests", "golden", pe.FILE)) as f:
        want_not_held = json.load(f)["errors"]["export/not_held"]
    runs = [[Held(S.CASES[n]) for n in S.THREAD_CASES[t]] for t in range(2)]
    ctx = types.SimpleNamespace(up=plan_of(S.CASES[S.THREAD_CASES[0][1]]))
    barrier = threading.Barrier(2)
    seen, errors = [[], []], []
    rounds = 3

    def last():
        return lib.zmpc_last_error().decode()

    def work(t):
        try:
            torch.cuda.set_device(device)
            for _ in range(rounds):
                barrier.wait(timeout=60)
                for run in runs[t]:
                    run.stage_inputs()
                    run.launch()
                    seen[t].append(last())
                barrier.wait(timeout=60)                                          # 1
                if t == 0:
                    rc = lib.zmpc_rollout_kicks(None, 1, 10, None, None, 20, None, None, None,
                                                None, None, None)
                    seen[t].append((rc, "kick_steps" in last()))
                    seen[t].append(pe.raised(not_held, ctx))
                    seen[t].append(last())
                barrier.wait(timeout=60)                                          # 2
                if t == 1:
                    seen[t].append(last())
                    runs[t][0].stage_inputs()
                    runs[t][0].launch()
                    seen[t].append(last())
                barrier.wait(timeout=60)                                          # 3
                if t == 0:
                    seen[t].append(last())
            for run in runs[t]:
                run.side.synchronize()
        except Exception as e:  # noqa: BLE001 (reported by the main thread)
            errors.append((t, repr(e)))
            barrier.abort()

    try:
        threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout=120)
        assert not errors and not any(th.is_alive() for th in threads), errors
        assert seen[1] == [""] * (4 * rounds), seen[1]
        assert seen[0] == ["", "", (_native.ZMPC_EINVAL, True), want_not_held,
                           "quantity not held by this plan",
                           "quantity not held by this plan"] * rounds, seen[0]
        for t in range(2):
            for run in runs[t]:
                assert_same(run.result(), serial.out[run.case.name, "A"], run.case.name)
    finally:
        torch.cuda.synchronize()


def test_two_threads_ask_for_the_same_cached_plan():
    """Two threads asking solver.get_plan (what ZMPController does at every call) for one new
    configuration at once get one plan, and controllers of that configuration built in both
    threads roll the same walk out bit for bit."""
    from mpc_bipedal.config import MPCConfig
    from mpc_bipedal.controllers import ZMPController
    d = S.CASES["unc_split_sparse"].make("A")
    barrier = threading.Barrier(2)
    got, errors = [None, None], []
    device = torch.cuda.current_device()

    def work(t):
        try:
            torch.cuda.set_device(device)
            cfg = MPCConfig(horizon=21, strict=False)
            barrier.wait(timeout=60)
            c = ZMPController(cfg)
            p = c._plan()
            hist, st = p.rollout(d["zmax"], d["zmin"], d["x0"], kick=d["kick"],
                                 kick_step=d["kick_step"])
            torch.cuda.synchronize()
            got[t] = (p, hist.clone(), st.clone(), p.export(_native.EXPORT_K))
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    try:
        clear_plan_cache()
        threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout=120)
        assert not errors and all(g is not None for g in got), errors
        assert got[0][0] is got[1][0]
        assert got[0][0] is get_plan(MPCConfig(horizon=21, strict=False))
        assert same_bits(got[0][1], got[1][1]) and not got[0][2].any() and not got[1][2].any()
        assert np.array_equal(got[0][3], got[1][3])
        assert torch.isfinite(got[0][1]).all()
    finally:
        torch.cuda.synchronize()
        clear_plan_cache()


# ----------------------------------------------------------------------------- e: first creation

CHILD = r"""
import ctypes, hashlib, json, sys, threading
sys.path[:0] = [{root!r}, {pkg!r}]
import numpy as np
import torch
from mpc_bipedal import _native
from mpc_bipedal.solver import Plan
specs = {specs!r}
barrier = threading.Barrier(len(specs))
out, errors = {{}}, []
def work(i):
    try:
        N, strict = specs[i]
        barrier.wait(timeout=60)
        p = Plan({device!r}, N, 0.01, {h!r}, {g!r}, {q!r}, {r!r}, strict)  # (first HIP use)
        ids = {every!r} + ({strict_ids!r} if strict else ())
        out[i] = {{str(w): hashlib.sha256(np.ascontiguousarray(p.export(w)).tobytes()).hexdigest()
                  for w in ids}}
    except Exception as e:
        errors.append(repr(e))
threads = [threading.Thread(target=work, args=(i,)) for i in range(len(specs))]
[t.start() for t in threads]
[t.join(timeout=100) for t in threads]
torch.cuda.synchronize()
print("RESULT " + json.dumps({{"out": out, "errors": errors}}))
"""


def test_contended_first_creation_in_a_fresh_process():
    """A fresh child process whose first act is two threads creating plans of different N at
    once (the one-time kernel attributes of csrc/capi.hip are set under a lock for this): the
    exported gain rows and tables equal those of plans created one after the other here, bit
    for bit."""
    specs = [S.PLAN_CREATE["A"], S.PLAN_CREATE["B"]]
    want = {}
    for i, (N, strict) in enumerate(specs):
        p = Plan(torch.cuda.current_device(), N, 0.01, S.H, S.G, S.Q, S.R, strict)
        try:
            ids = S.PLAN_EXPORTS + (S.STRICT_EXPORTS if strict else ())
            want[str(i)] = {str(w): hashlib.sha256(
                np.ascontiguousarray(p.export(w)).tobytes()).hexdigest() for w in ids}
        finally:
            p.destroy()
    code = CHILD.format(root=ROOT, pkg=PKG, specs=specs, device=torch.cuda.current_device(),
                        h=S.H, g=S.G, q=S.Q, r=S.R, every=S.PLAN_EXPORTS,
                        strict_ids=S.STRICT_EXPORTS)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, r.stdout[-2000:]
    res = json.loads(line[-1][len("RESULT "):])
    assert not res["errors"], res["errors"]
    assert res["out"] == want
