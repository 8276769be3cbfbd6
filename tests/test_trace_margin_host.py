"""The trace margin without a GPU (zmpc_trace_margin): the symbol is exported and bound and refuses
bad arguments before any device call; the header declares it without a stream parameter;
analysis.TraceMargin and the Python argument errors; and the fixed inputs of the device tests
(tests/trace_margin_cases.py) are fair to the device bar: the double-precision statement
analysis.trace_margin_reference stays within 1e-12 relative of the extended-precision one on every
one of them, a tenth of the device's 1e-11."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import trace_cases as tc
import trace_margin_cases as mc
from conftest import ROOT

from mpc_bipedal import _native  # noqa: E402
from mpc_bipedal.analysis import (Push, PushTrace, TraceMargin,  # noqa: E402
                                  trace_margin_reference)
from mpc_bipedal.config import MPCConfig  # noqa: E402
from mpc_bipedal.controllers import ZMPController  # noqa: E402

PTR = 4096  # a non-NULL device address, never read


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        pytest.fail("libzmpc.so not built (run __graft_entry__.build())")
    lib = _native.load()
    yield lib
    blk = ctypes.create_string_buffer(4096)  # a passing call leaves no message behind
    tr = _trace()
    lib.zmpc_trace_margin(ctypes.addressof(blk), 0, 2, PTR, PTR, PTR, 4, None, 1,
                          ctypes.addressof(tr), 0.0, PTR, None)


def _trace(dv=PTR, axes=3, steps=None, step=3, length=4, stream=None):
    return _native.ZmpcTrace(dv, axes, steps, step, length, stream)


# --------------------------------------------------------------------------- export and binding

def test_symbol_exported_and_bound(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True,
                         text=True).stdout
    assert "zmpc_trace_margin" in set(re.findall(r" T (zmpc_\w+)", out))
    res, args = _native.SIGNATURES["zmpc_trace_margin"]
    assert res is ctypes.c_int and len(args) == 13 and lib.zmpc_trace_margin.argtypes == args
    assert args[8] is ctypes.c_int64 and args[10] is ctypes.c_double
    assert ctypes.sizeof(_native.ZmpcTrace) == 48  # the descriptor is the traced rollouts'
    assert lib.zmpc_abi_version() == _native.ABI_VERSION == 7  # additive: the version stays


def test_header_declares_the_call_without_a_stream_parameter():
    """The stream travels in trace->stream, so the stream-contract table's rule does not reach the
    call, and the header says so where it says it for the traced rollouts."""
    import stream_cases as S
    assert "zmpc_trace_margin" not in S.stream_symbols()
    text = open(os.path.join(ROOT, "include", "zmpc.h")).read()
    m = re.search(r"int zmpc_trace_margin\(([^;]*)\);", text)
    assert m and "stream" not in m.group(1) and "const zmpc_trace* trace" in m.group(1)
    doc = text[text.index("Trace margin: the exact critical scale"):m.start()]
    assert "The trace margin, stated once" in doc and "trace->stream" in doc
    assert "tests/stream_cases.py" in doc and "Additive to ABI 7" in doc
    assert re.fullmatch(r"[a-z_]+", "zmpc_trace_margin")


def test_argument_checks_without_gpu(lib):
    """Every bad argument is ZMPC_EINVAL with a message.  The plan is never dereferenced on these
    paths, so a zeroed block stands in for one (N = 0, not strict)."""
    fake_plan = ctypes.create_string_buffer(4096)
    plan = ctypes.addressof(fake_plan)

    def call(plan=plan, B=2, n=10, hist=PTR, zmax=PTR, zmin=PTR, stride=20, lengths=None, draws=3,
             trace=_trace(), t=1e-9, scale=PTR, limit=None):
        rc = lib.zmpc_trace_margin(plan, B, n, hist, zmax, zmin, stride, lengths, draws,
                                   None if trace is None else ctypes.addressof(trace), t, scale,
                                   limit)
        return rc, lib.zmpc_last_error()

    rc, msg = call(plan=None)
    assert rc == _native.ZMPC_EINVAL and b"NULL plan" in msg
    rc, msg = call(trace=None)
    assert rc == _native.ZMPC_EINVAL and b"trace is NULL" in msg
    rc, msg = call(trace=_trace(dv=None))
    assert rc == _native.ZMPC_EINVAL and b"dv is NULL" in msg
    for bad in (dict(hist=None), dict(zmax=None), dict(zmin=None), dict(scale=None)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"NULL array" in msg, bad
    for bad in (dict(B=-1), dict(n=0), dict(n=-3)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"B >= 0 and n >= 1" in msg, bad
    for draws in (0, -1, -2 ** 40):
        rc, msg = call(draws=draws)
        assert rc == _native.ZMPC_EINVAL and b"draws >= 1" in msg, draws
    # B·draws beyond the batch limit: rows are what the grid counts
    for B, draws in ((2 ** 31, 1), (2 ** 16, 2 ** 15), (1, 2 ** 31), (3, 2 ** 62)):
        rc, msg = call(B=B, draws=draws)
        assert rc == _native.ZMPC_EINVAL and b"batch too large" in msg, (B, draws)
    for axes in (0, 4, -1, 7):
        rc, msg = call(trace=_trace(axes=axes))
        assert rc == _native.ZMPC_EINVAL and b"axes" in msg, axes
    for length in (0, -1, -2 ** 40):
        rc, msg = call(trace=_trace(length=length))
        assert rc == _native.ZMPC_EINVAL and b"length" in msg, length
    # a length whose B·draws·length·16 bytes pass int64 names no array
    for length in (2 ** 62, 2 ** 63 - 1, 2 ** 57):
        rc, msg = call(trace=_trace(length=length))
        assert rc == _native.ZMPC_EINVAL and b"length too large" in msg, length
    for t in (-1e-12, -1.0, float("nan"), float("-inf")):
        rc, msg = call(t=t)
        assert rc == _native.ZMPC_EINVAL and b"max_violation" in msg, t
    for stride in (19, 1, -20):
        rc, msg = call(stride=stride)
        assert rc == _native.ZMPC_EINVAL and b"bounds_stride" in msg, stride
    # an empty batch is a no-op, NULL arrays included; limit may always be NULL
    assert call(B=0) == (0, b"")
    assert call(B=0, trace=_trace(dv=None), hist=None, zmax=None, zmin=None, scale=None) == (0, b"")
    assert call(B=0, stride=0, t=0.0, draws=2 ** 40) == (0, b"")


def test_strict_plan_is_refused_before_any_launch(lib):
    """ZMPC_ESTATE with the reason, decided on the host from the plan's fields alone: a zeroed
    block with `strict` set."""
    blk = ctypes.create_string_buffer(4096)
    ints = (ctypes.c_int * 5).from_buffer(blk)  # (device, cus, N, Kpad, strict)
    ints[2], ints[4] = 64, 1
    tr = _trace()
    for B in (4, 0):
        rc = lib.zmpc_trace_margin(ctypes.addressof(blk), B, 40, PTR, PTR, PTR, 80, None, 2,
                                   ctypes.addressof(tr), 1e-9, PTR, PTR)
        msg = lib.zmpc_last_error()
        assert rc == _native.ZMPC_ESTATE, (B, msg)
        assert b"zmpc_trace_margin" in msg and b"not affine" in msg and b"clamped" in msg
        assert b"ZMPController.critical_force" in msg
    # the argument checks come first
    rc = lib.zmpc_trace_margin(ctypes.addressof(blk), 4, 40, PTR, PTR, PTR, 80, None, 0,
                               ctypes.addressof(tr), 1e-9, PTR, PTR)
    assert rc == _native.ZMPC_EINVAL


# --------------------------------------------------------------------------- analysis.TraceMargin

def test_trace_margin_decoding_and_survival():
    inf, nan = np.inf, np.nan
    scale = np.array([[[2.0, 0.5], [0.9, 3.0], [inf, inf], [1.0, 1.0]],
                      [[nan, nan], [nan, nan], [nan, nan], [nan, nan]]])
    limit = np.array([[[2 * 17 + 1, 2 * 5], [2 * 40, 2 * 41 + 1], [-1, -1], [0, 1]],
                      [[-1, -1]] * 4], np.int32)
    m = TraceMargin(scale, limit)
    assert len(m) == 2 and "draws=4" in repr(m)
    assert m.scale is scale and np.array_equal(m.critical, scale[..., 0], equal_nan=True)
    assert np.array_equal(m.sample[0], [[17, 5], [40, 41], [-1, -1], [0, 0]])
    assert np.array_equal(m.axis[0], [[1, 0], [0, 1], [-1, -1], [0, 1]])
    assert (m.sample[1] == -1).all() and (m.axis[1] == -1).all()
    assert np.array_equal(m.survives(), [[True, False, True, True], [False] * 4])
    assert np.array_equal(m.survives(2.0), [[True, False, True, False], [False] * 4])
    assert np.array_equal(m.survives(-1.0), [[False, True, True, True], [False] * 4])
    assert np.array_equal(m.survives(-3.0), [[False, True, True, False], [False] * 4])
    assert np.array_equal(m.survival(), [0.75, 0.0])
    assert np.array_equal(m.survival(-1.0), [0.75, 0.0])
    assert np.array_equal(m.survival(0.0), [1.0, 0.0])  # NaN never survives
    torch = pytest.importorskip("torch")
    mt = TraceMargin(torch.as_tensor(scale), torch.as_tensor(limit))
    assert np.array_equal(mt.survives(2.0).numpy(), m.survives(2.0))
    assert np.array_equal(mt.survival().numpy(), m.survival())
    assert np.array_equal(mt.sample.numpy(), m.sample) and np.array_equal(mt.axis.numpy(), m.axis)
    for bad in ((scale[0], limit[0]), (scale, limit[:1]), (scale[..., :1], limit[..., :1])):
        with pytest.raises(ValueError, match=r"\[B, K, 2\]"):
            TraceMargin(*bad)


def test_python_argument_errors_before_any_device_call():
    """ZMPController.trace_margin: a trace that is none, draws that are no count, and rows that
    do not divide into draws raise ValueError before a plan is built."""
    ctl = ZMPController(MPCConfig(strict=False))
    z = np.zeros((10, 2))
    t = PushTrace(np.ones((6, 4, 2)), 3)
    with pytest.raises(ValueError, match="analysis.PushTrace"):
        ctl.trace_margin(z + 1, z - 1, Push(10.0, 1, 3))
    for draws in (0, -2, 1.5, True, None):
        with pytest.raises(ValueError, match="draws must be an integer >= 1"):
            ctl.trace_margin(z + 1, z - 1, t, draws=draws)
    for draws in (4, 5, 7):
        with pytest.raises(ValueError, match="not a multiple of draws"):
            ctl.trace_margin(z + 1, z - 1, t, draws=draws)
    with pytest.raises(ValueError, match="dv must be"):
        trace_margin_reference(np.zeros((2, 10, 2, 3)), z + 1, z - 1, np.zeros((5, 4, 2)), 0,
                               np.eye(3), 0.07, draws=3)
    # critical_force(trace=, fused=True) keeps raising
    with pytest.raises(ValueError, match="no traced form"):
        ctl.critical_force(z + 1, z - 1, trace=PushTrace(np.ones((1, 4, 2)), 3), fused=True)


# --------------------------------------------------------------------------- fairness of the bar

def _reference(case, consts):
    return trace_margin_reference(case["hist"], case["zmax"], case["zmin"], case["dv"],
                                  case["steps"], mc.closed_loop_matrix(consts), mc.HG,
                                  draws=case["K"], axes=case["axes"], lengths=case["lengths"],
                                  max_violation=case["t"])


@pytest.mark.parametrize("n", tc.EMU_N)
def test_double_precision_statement_is_fair_on_the_grid(n):
    """On every case of the device grid the NumPy statement in double stays within 1e-12 relative
    of the extended-precision one, with the same +inf entries, and names the same (sample, axis)
    wherever the runner-up lies more than 1e-12 off."""
    consts = tc.closed_loop(mc.PAR150)
    worst, fair, total = 0.0, 0, 0
    cases = list(mc.grid(n)) + (mc.ragged_cases() if n == 129 else [])
    for case in cases:
        ref = mc.grid_extended(case, consts)
        scale, limit = _reference(case, consts)
        err, same, idx = mc.compare(scale, limit, ref)
        worst = max(worst, err)
        assert same and idx and err <= mc.FAIR, (n, case["L"], case["axes"], case["K"], err)
        fin = np.isfinite(ref[2])
        fair += int((ref[2][fin] > mc.FAIR).sum())
        total += int(fin.sum())
    print(f"MEASURED trace margin reference n={n}: double vs extended {worst:.2e}; index compared "
          f"on {fair} of {total} entries with a runner-up")


def test_double_precision_statement_is_fair_on_the_stored_walk():
    """The N = 64 walk under the four draws of the bracket tests, at t = 1e-9 and 0: 1e-12, finite
    scales in both columns of every draw, and the single-axis draw limited on y."""
    zmax, zmin, h, consts = mc.walk64()
    for t in (1e-9, 0.0):
        case = mc.walk64_case(t)
        ref = mc.extended(case, consts)
        scale, limit = _reference(case, consts)
        err, same, idx = mc.compare(scale, limit, ref)
        print(f"MEASURED trace margin reference, N = 64 walk, t = {t}: {err:.2e}; scales "
              f"{scale[0, :, 0].tolist()}")
        assert same and idx and err <= mc.FAIR
        assert np.isfinite(scale).all() and (scale > 0).all()
        assert (limit[0, 3] % 2 == 1).all()
