"""zmpc_rollout_metrics without a GPU: the symbol is exported and bound, and its argument checks
run before any device call (as tests/test_metrics_host.py does for zmpc_walk_metrics)."""
import ctypes
import os
import re
import subprocess

import pytest

from mpc_bipedal import _native


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libzmpc.so not built (run __graft_entry__.build())")
    lib = _native.load()
    yield lib
    blk = ctypes.create_string_buffer(4096)  # a passing call leaves no message behind
    lib.zmpc_rollout_metrics(ctypes.addressof(blk), 0, 2, 4096, 4096, 4, 4096, None, -1, None,
                             None, 4096, None, None)


def test_symbol_exported_and_bound(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True,
                         text=True).stdout
    assert "zmpc_rollout_metrics" in set(re.findall(r" T (zmpc_\w+)", out))
    res, args = _native.SIGNATURES["zmpc_rollout_metrics"]
    assert res is ctypes.c_int and len(args) == 14
    assert lib.zmpc_rollout_metrics.argtypes == args
    assert lib.zmpc_abi_version() == _native.ABI_VERSION == 7  # additive: the version stays


def test_c_abi_argument_checks_without_gpu(lib):
    """Every bad argument is ZMPC_EINVAL with a message.  The plan is never dereferenced on these
    paths, so a zeroed block stands in for one (N = 0, not strict, options 0)."""
    fake_plan = ctypes.create_string_buffer(4096)
    plan, ptr = ctypes.addressof(fake_plan), 4096  # ptr: a non-NULL device address, never read

    def call(plan=plan, B=2, n=10, zmax=ptr, zmin=ptr, stride=20, x0=ptr, kick=None, step=-1,
             steps=None, lengths=None, metrics=ptr, status=None):
        rc = lib.zmpc_rollout_metrics(plan, B, n, zmax, zmin, stride, x0, kick, step, steps,
                                      lengths, metrics, status, None)
        return rc, lib.zmpc_last_error()

    rc, msg = call(plan=None)
    assert rc == _native.ZMPC_EINVAL and b"NULL plan" in msg
    for bad in (dict(zmax=None), dict(zmin=None), dict(x0=None), dict(metrics=None)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"NULL" in msg, bad
    for bad in (dict(B=-1), dict(n=0), dict(n=-3)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"B >= 0 and n >= 1" in msg, bad
    for stride in (19, 1, -20):
        rc, msg = call(stride=stride)
        assert rc == _native.ZMPC_EINVAL and b"bounds_stride" in msg, stride
    rc, msg = call(B=2 ** 31)
    assert rc == _native.ZMPC_EINVAL and b"batch too large" in msg
    # an empty batch of a supported shape is a no-op, shared CoP or not
    assert call(B=0) == (0, b"")
    assert call(B=0, stride=0) == (0, b"")


def test_shapes_without_a_fused_form_are_refused_before_any_launch(lib):
    """ZMPC_ESTATE with the reason, decided on the host from the plan's fields alone: a zeroed
    block with `strict` set, and a non-strict one asked for a walk of more than 513 samples."""
    ptr = 4096
    blk = ctypes.create_string_buffer(4096)
    # (device, cus, N, Kpad, strict): the first five ints of zmpc_plan
    ints = (ctypes.c_int * 5).from_buffer(blk)
    ints[2] = 150
    rc = lib.zmpc_rollout_metrics(ctypes.addressof(blk), 4, 514, ptr, ptr, 1028, ptr, None, -1,
                                  None, None, ptr, None, None)
    assert rc == _native.ZMPC_ESTATE and b"513 samples" in lib.zmpc_last_error()
    ints[4] = 1
    rc = lib.zmpc_rollout_metrics(ctypes.addressof(blk), 4, 420, ptr, ptr, 840, ptr, None, -1,
                                  None, None, ptr, None, None)
    assert rc == _native.ZMPC_ESTATE and b"strict" in lib.zmpc_last_error()
