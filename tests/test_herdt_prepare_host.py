"""zmpc_herdt_prepare without a GPU: the symbol is exported and bound with no stream, it refuses
bad arguments before any device call and before the plan is read, an empty batch writes the host
word and nothing else, and the seeded cases of tests/herdt_prepare_cases.py tell the walk-alone
rule from "pad to the batch's n"."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import herdt_prepare_cases as pc
import stream_cases as S

from mpc_bipedal import _native  # noqa: E402
from mpc_bipedal.config import MPCConfig  # noqa: E402
from mpc_bipedal.controllers import herdt  # noqa: E402

PTR = 4096  # a non-NULL device address, never read


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        pytest.fail("libzmpc.so not built (run __graft_entry__.build())")
    lib = _native.load()
    yield lib
    blk = ctypes.create_string_buffer(4096)  # a passing call leaves no message behind
    lib.zmpc_herdt_prepare(ctypes.addressof(blk), 0, 1, None, 0, None, None, None, None, None)


def test_symbol_exported_bound_and_takes_no_stream(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True,
                         text=True).stdout
    assert "zmpc_herdt_prepare" in set(re.findall(r" T (zmpc_\w+)", out))
    res, args = _native.SIGNATURES["zmpc_herdt_prepare"]
    assert res is ctypes.c_int and len(args) == 10 and lib.zmpc_herdt_prepare.argtypes == args
    assert args[-1] == ctypes.POINTER(ctypes.c_int32)  # the host word, typed
    # synchronous by declaration: the header gives it no stream, so the stream registry owes it
    # no case
    assert "zmpc_herdt_prepare" not in S.stream_symbols()
    assert lib.zmpc_abi_version() == _native.ABI_VERSION == 7  # additive: the version stays


def test_argument_checks_without_gpu(lib):
    """Every bad argument is ZMPC_EINVAL with a message.  The plan is never read on these paths,
    so a zeroed block stands in for one."""
    fake_plan = ctypes.create_string_buffer(4096)
    plan = ctypes.addressof(fake_plan)
    word = ctypes.c_int32(-5)

    def call(plan=plan, B=2, n=10, states=PTR, ss=10, lengths=None, clean=None, nb=PTR,
             steps=None, host=True):
        word.value = -5
        rc = lib.zmpc_herdt_prepare(plan, B, n, states, ss, lengths, clean, nb, steps,
                                    ctypes.byref(word) if host else None)
        return rc, lib.zmpc_last_error()

    rc, msg = call(plan=None)
    assert rc == _native.ZMPC_EINVAL and b"NULL plan" in msg and word.value == -5
    for bad in (dict(B=-1), dict(n=0), dict(n=-3)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"B >= 0 and n >= 1" in msg, bad
    rc, msg = call(n=2 ** 24 + 1, ss=0)
    assert rc == _native.ZMPC_EINVAL and b"walk too long" in msg
    for bad in (dict(states=None), dict(nb=None)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"NULL array" in msg, bad
    for ss in (9, 1, -10):
        rc, msg = call(ss=ss)
        assert rc == _native.ZMPC_EINVAL and b"s_stride" in msg, ss
    assert word.value == -5  # a refusal writes nothing
    # an empty batch: the host word is written, nothing else is touched (every array NULL)
    assert call(B=0, states=None, nb=None) == (0, b"") and word.value == 0
    assert call(B=0, states=None, nb=None, host=False) == (0, b"")
    assert call(B=0, n=2 ** 24, ss=0) == (0, b"") and word.value == 0


def test_rollouts_keep_their_nb_next_check(lib):
    """zmpc_herdt_rollout(_pushed) still refuse a NULL nb_next: preparing is a call of its own."""
    fake_plan = ctypes.create_string_buffer(4096)
    prm = herdt.make_params(MPCConfig(), 2)
    rc = lib.zmpc_herdt_rollout(ctypes.addressof(fake_plan), ctypes.addressof(prm), 2, 10, PTR, 20,
                                PTR, 10, None, 10, PTR, None, -1, PTR, PTR, None, None)
    assert rc == _native.ZMPC_EINVAL and b"NULL array" in lib.zmpc_last_error()


def test_cases_cover_what_they_claim():
    """The seeded batches hold walks ending in each of the three states, all-standing walks, runs
    that cross chunk edges, and lengths 1, 2, n − 1, n and two that must clamp."""
    c = pc.case(200, 64, "ragged_pad")
    n = c["n"]
    live = np.clip(c["lengths"], 1, n)
    assert {1, 2, n - 1, n} <= set(live.tolist())
    assert (c["lengths"] < 1).any() and (c["lengths"] > n).any()
    assert (c["states"][np.arange(pc.B), live - 1] >= 0).all()
    assert all((c["states"][b, live[b]:] == -1).all() for b in range(pc.B))
    alt = pc.case(200, 64, "ragged_alt")
    assert all(set(alt["states"][b, live[b]:].tolist()) <= {1, 2} for b in range(pc.B))
    full = pc.case(200, 64, "full")
    assert {int(s[-1]) for s in full["states"]} == {0, 1, 2}
    assert any(not s.any() for s in full["states"])
    runs = [np.diff(np.flatnonzero(np.diff(s) != 0)) for s in full["states"]]
    assert any(len(r) and r.max() >= 60 for r in runs) and any(len(r) and r.max() <= 5 for r in runs)
    # the padding never reaches the answer: both fills give the same one
    for key in ("want_states", "want_nb", "want_steps"):
        assert np.array_equal(c[key], alt[key]), key
    assert (c["want_nb"][np.arange(n)[None, :] >= live[:, None]] == 1).all()
    assert c["want_steps"].max() > 0 and c["want_states"].min() >= 0


def test_the_walk_alone_rule_differs_from_padding_to_the_batch():
    """The default walk (302 samples, N = 150) inside an n = 359 batch: entry 251, the double-
    support sample before the final stand, counts to the end of the padded sequence, so it is
    302 + 150 − 251 for the walk alone and 359 + 150 − 251 when the walk is first padded to the
    batch's n.  Its window holds a footstep; a call that read the padded rows would be caught."""
    n, N = 359, 150
    c = pc.case(n, N, "ragged_pad")
    assert c["lengths"][0] == 302 and np.array_equal(c["states"][0, :302], pc.default_states())
    st = c["states"][0]
    assert st[251] == herdt.DOUBLE_SUPPORT and st[252] == herdt.STANDING
    assert not (st[252:302] != herdt.STANDING).any()
    alone = c["want_nb"]
    _, padded, steps_padded = pc.padded_to_batch(c["states"], c["lengths"], N)
    assert alone[0, 251] == 302 + N - 251 and padded[0, 251] == n + N - 251
    # ... and it is the drop-in answer for that walk by itself
    d = np.load(os.path.join(pc.GOLDEN, "herdt_default.npz"))
    assert np.array_equal(alone[0, :302], d["nb_steps"][:302, 0])
    # a footstep in that entry's window: the transition DOUBLE → STANDING at 251 is a break
    pad = np.concatenate([st[:302], np.repeat(st[301:302], N)])
    assert herdt.max_footsteps(pad[None, 251:], N, 2) >= 1
    live = np.clip(c["lengths"], 1, n)
    differ = [(b, i) for b in range(pc.B) for i in range(live[b]) if alone[b, i] != padded[b, i]]
    assert (0, 251) in differ and len({b for b, _ in differ}) > 5
    assert np.array_equal(c["want_steps"], steps_padded)  # (the tail is constant: no break in it)


def test_python_layer_argument_errors_before_any_device_call():
    from mpc_bipedal.generators import SpeedTrajectoryGenerator
    g = SpeedTrajectoryGenerator(MPCConfig(horizon=33, dt=0.03, speed_generation="nope"))
    with pytest.raises(ValueError, match="Unknown speed_generation mode"):
        g.generate_speed_and_state_batch(np.zeros((2, 7)))
    g = SpeedTrajectoryGenerator(MPCConfig(horizon=33, dt=0.03))
    with pytest.raises(ValueError, match=r"\[B, 7\]"):
        g.generate_speed_and_state_batch(np.zeros((2, 6)))
    p = np.array([[1.0, 0.3, 0.1, 0.24, 0.03, 0.3, 0.03], [1.0, 0.3, 0.1, 0.24, 0.03, 0.3, 0.01]])
    with pytest.raises(ValueError, match="dt column"):
        g.generate_speed_and_state_batch(p)
    with pytest.raises(ValueError, match="dt column"):
        g.generate_speed_and_state_batch([MPCConfig(horizon=33, dt=0.03), MPCConfig()])
