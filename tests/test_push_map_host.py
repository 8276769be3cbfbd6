"""zmpc_push_map without a GPU: the symbol is exported and bound and refuses bad arguments before
any device call (as tests/test_rollout_metrics_host.py does for zmpc_rollout_metrics); the launch
rule choose_push_map answers on the host; and the statement the kernels are held to — the
response table by delay (analysis.push_response) and the map in NumPy
(analysis.push_map_reference) — agrees with pushed oracle rollouts, with the closed form
critical_force_affine and with the pinned numbers of the stored N = 64 walk."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import push_map_cases as pc

from mpc_bipedal import _native  # noqa: E402
from mpc_bipedal.analysis import (PushMap, critical_force_affine, push_map_reference,  # noqa: E402
                                  push_response)
from oracle import zmp_oracle as O  # noqa: E402

CSRC = os.path.join(ROOT, "model-predictive-control-for-bipedal-locomotion_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu")


# --------------------------------------------------------------------------- export and binding


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libzmpc.so not built (run __graft_entry__.build())")
    lib = _native.load()
    yield lib
    blk = ctypes.create_string_buffer(4096)  # a passing call leaves no message behind
    lib.zmpc_push_map(ctypes.addressof(blk), 0, 2, 4096, 4096, 4096, 4, None, None, 0.0, 40.0,
                      4096, None, None, None)


def test_symbol_exported_and_bound(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True,
                         text=True).stdout
    assert "zmpc_push_map" in set(re.findall(r" T (zmpc_\w+)", out))
    res, args = _native.SIGNATURES["zmpc_push_map"]
    assert res is ctypes.c_int and len(args) == 15
    assert args[9] is ctypes.c_double and args[10] is ctypes.c_double  # max_violation, mass
    assert lib.zmpc_push_map.argtypes == args
    assert lib.zmpc_abi_version() == _native.ABI_VERSION == 7  # additive: the version stays


def test_c_abi_argument_checks_without_gpu(lib):
    """Every bad argument is ZMPC_EINVAL with a message.  The plan is never dereferenced on these
    paths, so a zeroed block stands in for one (N = 0, not strict)."""
    fake_plan = ctypes.create_string_buffer(4096)
    plan, ptr = ctypes.addressof(fake_plan), 4096  # ptr: a non-NULL device address, never read

    def call(plan=plan, B=2, n=10, hist=ptr, zmax=ptr, zmin=ptr, stride=20, lengths=None,
             steps=None, t=1e-9, mass=40.0, force=ptr, limit=None, response=None):
        rc = lib.zmpc_push_map(plan, B, n, hist, zmax, zmin, stride, lengths, steps, t, mass,
                               force, limit, response, None)
        return rc, lib.zmpc_last_error()

    rc, msg = call(plan=None)
    assert rc == _native.ZMPC_EINVAL and b"NULL plan" in msg
    for bad in (dict(hist=None), dict(zmax=None), dict(zmin=None), dict(force=None)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"NULL" in msg, bad
    for bad in (dict(B=-1), dict(n=0), dict(n=-3)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"B >= 0 and n >= 1" in msg, bad
    for t in (-1e-300, -1.0, float("nan")):
        rc, msg = call(t=t)
        assert rc == _native.ZMPC_EINVAL and b"max_violation" in msg, t
    for mass in (0.0, -40.0, float("nan"), float("inf")):
        rc, msg = call(mass=mass)
        assert rc == _native.ZMPC_EINVAL and b"mass" in msg, mass
    for stride in (19, 1, -20):
        rc, msg = call(stride=stride)
        assert rc == _native.ZMPC_EINVAL and b"bounds_stride" in msg, stride
    rc, msg = call(B=2 ** 31)
    assert rc == _native.ZMPC_EINVAL and b"batch too large" in msg
    # an empty batch is a no-op, both forms, shared CoP or not
    assert call(B=0) == (0, b"")
    assert call(B=0, stride=0, steps=ptr, hist=None, force=None) == (0, b"")


def test_strict_plans_and_long_walks_are_refused_before_any_launch(lib):
    """ZMPC_ESTATE with the reason, decided on the host from the plan's fields alone: a zeroed
    block with `strict` set, and a non-strict one asked for a full map past the LDS limit (the
    message states the limit)."""
    ptr = 4096
    blk = ctypes.create_string_buffer(4096)
    ints = (ctypes.c_int * 5).from_buffer(blk)  # (device, cus, N, Kpad, strict)
    ints[2] = 150
    n = 10113
    rc = lib.zmpc_push_map(ctypes.addressof(blk), 4, n, ptr, ptr, ptr, 2 * n, None, None, 0.0,
                           40.0, ptr, None, None, None)
    assert rc == _native.ZMPC_ESTATE and b"10112 samples" in lib.zmpc_last_error()
    ints[4] = 1
    for steps in (None, ptr):
        rc = lib.zmpc_push_map(ctypes.addressof(blk), 4, 420, ptr, ptr, ptr, 840, None, steps,
                               0.0, 40.0, ptr, None, None, None)
        msg = lib.zmpc_last_error()
        assert rc == _native.ZMPC_ESTATE and b"strict" in msg and b"critical_force" in msg


def test_choose_push_map(tmp_path):
    """The launch rule on the host: n = 4096 is taken, the rule's own limit is taken and one past
    it refused with a reason; the LDS holds n + 64 pairs of doubles; one wave per pair of 64-step
    blocks up to 16; the single-step form takes any n with no LDS."""
    exe = tmp_path / "push_map_dispatch_main"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{CSRC}", "-o", str(exe),
                    os.path.join(EMU, "push_map_dispatch_main.cpp")], check=True,
                   capture_output=True)

    def ask(queries):
        text = "".join(f"{n} {int(s)}\n" for n, s in queries)
        r = subprocess.run([str(exe)], input=text.encode(), capture_output=True, check=True,
                           timeout=60)
        return [tuple(int(v) for v in ln.split()) for ln in r.stdout.decode().splitlines()]

    (_, _, _, limit, _), = ask([(1, 0)])
    assert limit >= 4096
    assert (limit + 64) * 16 <= 159 * 1024 < (limit + 65) * 16
    ns = [1, 2, 64, 65, 128, 129, 420, 1431, 4096, limit]
    for n, (ok, waves, lds, _, why) in zip(ns, ask([(n, 0) for n in ns])):
        blocks = (n + 63) // 64
        assert ok == 1 and not why, n
        assert lds == (n + 64) * 16 and waves == min(16, max(1, (blocks + 1) // 2)), n
    assert ask([(limit + 1, 0), (1 << 24, 0)]) == [(0, 0, 0, limit, 1)] * 2
    assert ask([(limit + 1, 1), (1 << 24, 1), (1, 1)]) == [(1, 1, 0, limit, 0)] * 3


# --------------------------------------------------------------------------- the statement


@pytest.fixture(scope="module", params=pc.WALKS)
def stored(request):
    return pc.walk(request.param)


def test_response_is_time_invariant(stored):
    """Pushed minus unpushed oracle rollout = the response table shifted by the push step, at
    s ∈ {0, 1, n//2, n − 3}: to 1e-13 m per newton (measured: 1e-16)."""
    d, par, kx, r, hist, hg = stored
    n, dt, m = hist.shape[1], par[1], float(d["m"])
    assert r[0] == 0.0 and r[1] == 0.0
    z0 = hist[0, :, 1, 0] - hg * hist[0, :, 1, 2]
    for s in (0, 1, n // 2, n - 3):
        h1 = O.rollout_gain(d["zmax"][None], d["zmin"][None], np.zeros((1, 2, 3)), *par,
                            kick=np.array([dt * 1.0 / m]), kick_step=s)
        assert np.array_equal(h1[0, :, 0], hist[0, :, 0])  # only y is pushed
        z1 = h1[0, :, 1, 0] - hg * h1[0, :, 1, 2]
        want = np.zeros(n)
        want[s + 1:] = r[1:n - s]
        err = np.abs((z1 - z0) - want).max()
        print(f"n = {n}, s = {s}: {err:.2e}")
        assert err <= 1e-13


def test_reference_equals_affine_closed_form():
    """push_map_reference against critical_force_affine with the shifted response, every step and
    both directions of the N = 64 walk: the same doubles at t = 0 (the two then form the same
    margins), 1e-12 relative at t = 1e-9 (zmax + t − z0 against (zmax − z0) + t)."""
    d, par, kx, r, hist, hg = pc.walk("walk_n64.npz")
    n = hist.shape[1]
    z0 = hist[0, :, 1, 0] - hg * hist[0, :, 1, 2]
    for t, rtol in ((0.0, 0.0), (1e-9, 1e-12)):
        F, L = push_map_reference(hist, d["zmax"], d["zmin"], r, hg, max_violation=t)
        for s in range(n):
            rs = np.zeros(n)
            rs[s + 1:] = r[1:n - s]
            for k, sign in enumerate((1.0, -1.0)):
                fa = critical_force_affine(z0, sign * rs, d["zmax"][:, 1], d["zmin"][:, 1], t)
                if s >= n - 2:
                    assert fa == np.inf and F[0, s, k] == np.inf and L[0, s, k] == -1
                else:
                    assert abs(F[0, s, k] - fa) <= rtol * fa, (t, s, k, F[0, s, k], fa)
                    i = L[0, s, k]
                    assert s < i < n and rs[i] != 0


def test_pinned_numbers_of_the_n64_walk():
    d, par, kx, r, hist, hg = pc.walk("walk_n64.npz")
    n = hist.shape[1]
    F, L = push_map_reference(hist, d["zmax"], d["zmin"], r, hg, max_violation=1e-9)
    assert F.shape == (1, n, 2) and L.shape == (1, n, 2) and L.dtype == np.int32
    assert abs(F[0, 89, 0] - 32.331749) <= 1e-6
    assert abs(F[0, 89, 1] - 34.058429) <= 1e-6
    assert abs(F[0, 44, 0] - 12.444837) <= 1e-6
    fin = F[0, :n - 2]
    assert np.isfinite(fin).all() and fin.size == 354
    assert abs(fin.min() - 7.608461) <= 1e-6 and abs(fin.max() - 548.87) <= 1e-2
    assert np.unravel_index(np.argmin(fin), fin.shape) == (62, 1)
    assert np.isposinf(F[0, n - 2:]).all() and (L[0, n - 2:] == -1).all()
    val, step, direction = PushMap(F, L).weakest()
    assert abs(val[0] - 7.608461) <= 1e-6 and step[0] == 62 and direction[0] == -1
    # the single-step form is the rows of the full map
    for s, want in ((89, F[0, 89]), (0, F[0, 0]), (n - 3, F[0, n - 3])):
        f1, l1 = push_map_reference(hist, d["zmax"], d["zmin"], r, hg, max_violation=1e-9,
                                    push_steps=[s])
        assert np.array_equal(f1[0], want) and np.array_equal(l1[0], L[0, s])
    for s in (n - 2, n - 1, n, -1):
        f1, l1 = push_map_reference(hist, d["zmax"], d["zmin"], r, hg, push_steps=[s])
        assert np.isposinf(f1).all() and (l1 == -1).all()


def test_default_walk_fails_unpushed_at_1e9_and_passes_at_2cm():
    """walk_n150, the reference's default walk: its unconstrained ZMP leaves the boxes, so the
    map is NaN at max_violation = 1e-9 (critical_force's "fails with no push"); at 2 cm every
    entry before n − 2 is finite."""
    d, par, kx, r, hist, hg = pc.walk("walk_n150.npz")
    n = hist.shape[1]
    F, L = push_map_reference(hist, d["zmax"], d["zmin"], r, hg, max_violation=1e-9)
    assert np.isnan(F).all() and (L == -1).all()
    val, step, direction = PushMap(F, L).weakest()
    assert np.isnan(val[0]) and step[0] == -1 and direction[0] == 0
    F, L = push_map_reference(hist, d["zmax"], d["zmin"], r, hg, max_violation=0.02)
    fin = F[0, :n - 2]
    assert np.isfinite(fin).all() and fin.size == 836
    assert abs(fin.min() - 60.44) <= 1e-2 and abs(fin.max() - 2245.35) <= 1e-2


@pytest.mark.parametrize("name,t,entries", (("walk_n64.npz", 1e-9, 354), ("walk_n10.npz", 1e-9, 52),
                                            ("walk_n150.npz", 0.02, 836),
                                            ("walk_n512.npz", 0.03, 2858)))
def test_limit_is_decided_clearly_on_the_stored_walks(name, t, entries):
    """The device tests compare `limit` only where the runner-up candidate is more than 1e-9
    (relative) above the minimum.  How many entries that leaves out is a property of the statement
    alone: on the four stored walks none (the N = 150 and N = 512 walks need 2 and 3 cm of
    allowance to pass unpushed at all)."""
    d, par, kx, r, hist, hg = pc.walk(name)
    F, L = push_map_reference(hist, d["zmax"], d["zmin"], r, hg, max_violation=t)
    fin = np.isfinite(F)
    assert fin.sum() == entries
    gap = pc.runner_up_gap(hist, d["zmax"], d["zmin"], r, hg, max_violation=t)
    left_out = int((gap[fin] <= 1e-9).sum())
    print(f"{name}: {left_out} of {entries} entries within 1e-9 of their runner-up")
    assert left_out <= 0.01 * entries
    assert (L[fin] > np.nonzero(fin)[1]).all() and (L[~fin] == -1).all()


# --------------------------------------------------------------------------- edge cases


def test_sample_on_its_bound_gives_zero_not_nan():
    """t = 0 and a sample exactly on its upper bound: the push that drives it further out is 0
    (never 0·inf or 0/0 = NaN), the opposite push is limited elsewhere."""
    hist, zmax, zmin = pc.quiet_walk(12)
    r = np.zeros(12)
    r[2:] = [1e-3, -2e-3, 5e-4, 1e-300, 5e-324, -5e-324, 0.0, 1e-4, 1e-4, 1e-4]
    zmax[0, 6, 1] = 0.0  # z0 = 0: up_6 = 0
    F, L = push_map_reference(hist, zmax, zmin, r, 0.1, max_violation=0.0)
    assert not np.isnan(F).any()
    assert F[0, 4, 0] == 0.0 and L[0, 4, 0] == 6          # d = 2, r > 0: up limits +y
    assert F[0, 3, 1] == 0.0 and L[0, 3, 1] == 6          # d = 3, r < 0: up limits −y
    assert F[0, 0, 0] == 0.0 and L[0, 0, 0] == 6          # d = 6: a denormal response
    assert F[0, 4, 1] == 0.1 / 2e-3 and L[0, 4, 1] == 7   # −y from step 4: d = 3 at sample 7


def test_tie_goes_to_the_lower_index():
    """Two samples that give the same candidate bit for bit: margins 0.1 and 0.05 under responses
    2e-3 and 1e-3 (a power of two apart)."""
    hist, zmax, zmin = pc.quiet_walk(10)
    r = np.zeros(10)
    r[2], r[4] = 2 ** -9, 2 ** -10
    zmax[0, 6, 1] = 0.05
    F, L = push_map_reference(hist, zmax, zmin, r, 0.1)
    assert F[0, 2, 0] == 0.1 / 2 ** -9 == 0.05 / 2 ** -10  # samples 4 and 6 tie
    assert L[0, 2, 0] == 4
    assert F[0, 2, 1] == 0.1 / 2 ** -9 and L[0, 2, 1] == 4  # −y: dn limits, sample 4 alone
    # a walk no response reaches: +inf and −1
    F, L = push_map_reference(hist, zmax, zmin, np.zeros(10), 0.1)
    assert np.isposinf(F).all() and (L == -1).all()


def test_ragged_lengths_ignore_dead_tails():
    """Walks of 1, 2, 3, 64, 65 and n live samples padded to n with NaN and garbage: each equals
    the map of the truncated walk, rows from n_b − 2 on are +inf."""
    n, lengths = 130, [1, 2, 3, 64, 65, 130]
    r = pc.synthetic_response(n)
    for shared in (False, True):
        hist, zmax, zmin = pc.synthetic_case(n, shared, 6, lengths=lengths)
        F, L = push_map_reference(hist, zmax, zmin, r, pc.HG, lengths=lengths)
        for b, nb in enumerate(lengths):
            hi = zmax[:nb] if shared else zmax[b:b + 1, :nb]
            lo = zmin[:nb] if shared else zmin[b:b + 1, :nb]
            Fb, Lb = push_map_reference(hist[b:b + 1, :nb], hi, lo, r[:nb], pc.HG)
            assert np.array_equal(F[b, :nb], Fb[0]) and np.array_equal(L[b, :nb], Lb[0])
            assert np.isposinf(F[b, max(nb - 2, 0):]).all() and (L[b, max(nb - 2, 0):] == -1).all()
            assert np.isfinite(F[b, :max(nb - 2, 0)]).any() or nb <= 3
        # lengths outside [1, n] are clamped as zmpc_walk_metrics clamps them
        F2, _ = push_map_reference(hist[5:], zmax if shared else zmax[5:],
                                   zmin if shared else zmin[5:], r, pc.HG, lengths=[n + 7])
        assert np.array_equal(F2[0], F[5])


def test_nan_in_a_live_x_sample_fails_the_whole_walk():
    n = 66
    hist, zmax, zmin = pc.synthetic_case(n, False, 3)
    r = pc.synthetic_response(n)
    F0, _ = push_map_reference(hist, zmax, zmin, r, pc.HG)
    assert np.isfinite(F0[:, :n - 2]).any(axis=(1, 2)).all()
    hist[1, 40, 0, 1] = np.nan            # an x-axis velocity
    hist[2, 65, 0, 0] = np.inf            # the last x position
    F, L = push_map_reference(hist, zmax, zmin, r, pc.HG)
    assert np.array_equal(F[0], F0[0])
    assert np.isnan(F[1:]).all() and (L[1:] == -1).all()
    # ... unless the sample is dead
    F, _ = push_map_reference(hist, zmax, zmin, r, pc.HG, lengths=[n, 40, 65])
    assert not np.isnan(F).any()
    # a violation above t on the x axis alone fails the walk as well
    hist, zmax, zmin = pc.synthetic_case(n, False, 2)
    zmax[1, 10, 0] -= 0.2
    F, _ = push_map_reference(hist, zmax, zmin, r, pc.HG)
    assert not np.isnan(F[0]).any() and np.isnan(F[1]).all()


def test_push_response_matches_matrix_powers():
    """r_d = −(dt/m)·C·Ā^(d−1)·e1 against explicit matrix powers in extended precision."""
    d, par, kx, r, hist, hg = pc.walk("walk_n150.npz")
    N, dt, h, g, Q, R = par
    A, B, C = O.lipm(dt, h, g)
    Abar = (A - np.outer(B[:, 0], kx)).astype(np.longdouble)
    v = np.array([0, 1, 0], np.longdouble)
    want = np.zeros(len(r), np.longdouble)
    for k in range(1, len(r)):
        want[k] = -(np.longdouble(dt) / np.longdouble(float(d["m"]))) * (C.astype(np.longdouble) @ v)
        v = Abar @ v
    assert np.abs(r - want.astype(np.float64)).max() <= 1e-10 * np.abs(r).max()
    assert np.array_equal(r, push_response(A, B, kx, C, dt, float(d["m"]), len(r)))
