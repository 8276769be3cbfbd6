"""The four strict (ZMP box-QP) device solvers on hostile bounds and at every kernel shape, against
the exact box-QP oracle and the C restatement of the device algorithm (tests/strict_cases.py;
tests/test_strict_cases_host.py proves every case used here on the CPU: the oracle's KKT
residuals, the restatement against the oracle and the oracle's own sensitivity, all <= 1e-10).

Bars, the project's existing ones: rollouts CoM RMSE <= 1e-9 and every state within
1e-9 x max(1, largest |reference state|); cold steps <= 1e-9 relative; every status asserted.

  a  families (jitter, narrow, steps, zigzag) x N = 1, 5, 8, 9, 33, 64, 65: solvers 3 and 4 at
     four (Q, R, h) points, solvers 1 and 2 at the default weights; vs the exact oracle.
  b  a wave with unlike lanes: the mixed batch at N = 64 — solver 3 with B = 200 (kick order on
     and off, both bound forms, bitwise equal), solver 4 with B = 40 (whole-wave instances) and
     B = 1200 (two 32-lane instances per wave); every walk vs the C restatement, one walk of
     each kind vs the exact oracle.
  c  the reduced-Cholesky branches of strict.hip (registers to 64 in four instantiations, packed
     LDS to 128, global scratch beyond: the reduced system is the smaller of the pinned and the
     free set): pinned windows of m = 0 .. 150 at N = 150 and m = 128 .. 512 at N = 512 in one
     launch each, all four solvers, vs the exact oracle.
  d  every workgroup shape of the LQ kernel (csrc/dispatch.h lq_shape) and the longest horizon:
     cold pinned windows and six-sample rollouts at N = 320 .. 2464; the scan kernel at
     N = 512, 513, 960.
  e  one walk with NaN bounds: flagged alone, every other walk bitwise untouched.
"""
import functools
import os
import time

import numpy as np
import pytest
import torch

import strict_cases as SC
from conftest import golden, rmse

pytestmark = pytest.mark.gpu

from mpc_bipedal.solver import Plan  # noqa: E402
from mpc_bipedal import _native  # noqa: E402

BAR = 1e-9
THREADS = min(16, os.cpu_count() or 1)
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


def plan(N, dt, weights=SC.WEIGHTS[0], solver=0, kick_order=1, bounds=0):
    """The module's plan of (N, dt, weights), with its options set for this use."""
    key = (N, dt, weights)
    if key not in _PLANS:
        Q, R, h = weights
        _PLANS[key] = Plan(torch.cuda.current_device(), N, dt, h, SC.G, Q, R, True)
    p = _PLANS[key]
    p.set_option("strict_solver", solver)
    p.set_option("kick_order", kick_order)
    p.set_option("strict_bounds", bounds)
    return p


def run_rollout(p, case):
    h, st = p.rollout(case["zmax"], case["zmin"], case["x0"], kick=case["kick"],
                      kick_step=case["kick_step"])
    return h.cpu().numpy(), st.cpu().numpy()


def hist_err(h, ref):
    """(CoM RMSE, largest state difference relative to max(1, largest |reference state|))."""
    return rmse(h[..., 0], ref[..., 0]), SC.rel_err(h, ref)


def assert_hist(h, st, ref, label):
    assert not st.any(), (label, st)
    r, e = hist_err(h, ref)
    print(f"MEASURED {label}: CoM RMSE {r:.2e} state {e:.2e}")
    assert r <= BAR and e <= BAR, (label, r, e)
    return r, e


@functools.lru_cache(maxsize=None)
def family_reference(family, N, weights):
    """The exact oracle's histories of rollout_case(family, N); not to be written into."""
    case = SC.rollout_case(family, N)
    ref = np.stack([SC.oracle_walk(case, b, weights) for b in range(len(case["kick"]))])
    ref.setflags(write=False)
    return ref


# ----------------------------------------------------------------------------- a: the families

@pytest.mark.parametrize("N", SC.SMALL_HORIZONS)
@pytest.mark.parametrize("family", SC.FAMILIES)
def test_families_vs_exact_oracle(family, N):
    case = SC.rollout_case(family, N)
    for wi, weights in enumerate(SC.WEIGHTS):
        ref = family_reference(family, N, weights)
        for solver in ((3, 4, 1, 2) if wi == 0 else (3, 4)):
            p = plan(N, case["dt"], weights, solver)
            p.counters(reset=True)
            h, st = run_rollout(p, case)
            assert_hist(h, st, ref, f"{family} N={N} w{wi} solver {solver}")
            if solver == 3:
                c = p.counters(reset=True)
                solves = 2 * h.shape[0] * (h.shape[1] - 1)
                print(f"MEASURED {family} N={N} w{wi} passes/solve "
                      f"{c['instance_passes'] / solves:.2f} max {c['max_passes_per_solve']}")


# ----------------------------------------------------------------------------- b: unlike lanes

@functools.lru_cache(maxsize=None)
def mixed_reference(B):
    """The C restatement on the mixed batch (tied to the exact oracle on the same 1200 walks in
    the host test) and the exact oracle on its first seven walks, one of each kind."""
    case = SC.mixed_case(B)
    hist, status, _ = SC.restatement(case, threads=THREADS)
    assert not status.any()
    exact = np.stack([SC.oracle_walk(case, b) for b in range(7)])
    assert len(set(case["kinds"][:7])) == 7
    return case, hist, exact


def test_mixed_wave_lq_kernel():
    case, ref, exact = mixed_reference(200)     # three full waves and a partial one per axis
    outs = []
    for kick_order, bounds in ((1, 1), (0, 1), (1, 2), (0, 2)):
        p = plan(64, case["dt"], solver=3, kick_order=kick_order, bounds=bounds)
        p.counters(reset=True)
        h, st = run_rollout(p, case)
        c = p.counters(reset=True)
        assert_hist(h, st, ref, f"mixed B=200 solver 3 order {kick_order} bounds {bounds}")
        assert_hist(h[:7], st[:7], exact, "mixed B=200 solver 3, exact oracle")
        outs.append((h, c["instance_passes"]))
    solves = 2 * 200 * 39
    print(f"MEASURED mixed B=200 solver 3 passes/solve {outs[0][1] / solves:.2f} "
          f"max {c['max_passes_per_solve']}")
    for h, passes in outs[1:]:
        assert np.array_equal(h, outs[0][0]) and passes == outs[0][1]


@pytest.mark.parametrize("B", (40, 1200))
def test_mixed_wave_scan_kernel(B):
    """B = 40: whole-wave instances; B = 1200: more than four instances per compute unit, so
    32-lane instances and two unlike neighbours in a wave."""
    case, ref, exact = mixed_reference(B)
    h, st = run_rollout(plan(64, case["dt"], solver=4), case)
    assert_hist(h, st, ref, f"mixed B={B} solver 4")
    assert_hist(h[:7], st[:7], exact, f"mixed B={B} solver 4, exact oracle")


# ----------------------------------------------------------------------------- c: reduced Cholesky

@functools.lru_cache(maxsize=None)
def window_reference(kind, N):
    case = SC.chol_case(N) if kind == "chol" else SC.lq_case(N)
    if kind == "lq" and N > SC.LQ_LIVE_MAX and N in SC.LQ_HORIZONS:
        d = golden("strict_cases.npz")
        return case, d[f"step{N}_out"]
    out, m, _ = SC.solve_windows(case)
    assert np.array_equal(m, case["m"])
    return case, out


def assert_step(p, case, ref, label):
    out, st = p.step(case["x"], case["zmax"], case["zmin"])
    out, st = out.cpu().numpy(), st.cpu().numpy()
    assert not st.any(), (label, st)
    e = SC.rel_err(out, ref)
    print(f"MEASURED {label}: step {e:.2e}")
    assert e <= BAR, (label, e)
    return out


@pytest.mark.parametrize("solver", (1, 2, 3, 4))
@pytest.mark.parametrize("N", (150, 512))
def test_reduced_cholesky_branches(N, solver):
    """Several working-set sizes in one launch (the tile kernel's 16 instances of a workgroup
    differ in branch)."""
    case, ref = window_reference("chol", N)
    assert_step(plan(N, case["dt"], solver=solver), case, ref, f"chol N={N} solver {solver}")


# ----------------------------------------------------------------------------- d: LQ shapes

LQ_SHAPES = {320: (8, 2), 321: (8, 1), 608: (8, 1), 609: (8, 0), 896: (8, 0), 897: (4, 2),
             1600: (4, 2), 1601: (4, 1), 1888: (4, 1), 1889: (4, 0), 2176: (4, 0), 2177: (2, 2),
             2464: (2, 2)}     # (waves per workgroup, LDS checkpoints): csrc/dispatch.h lq_shape


@pytest.mark.parametrize("N", SC.LQ_HORIZONS)
def test_lq_shapes(N):
    """One plan per horizon (built once, here): cold pinned windows (m = 20, 40, 60; pins in the
    first segment, across its edge, in LDS- and global-checkpoint segments and at slot N − 1) vs
    the exact oracle — live to N = 897, stored beyond — and six-sample rollouts in both bound
    forms vs the C restatement and, to N = 897, the stored exact oracle.  Solver 3 and the
    automatic choice (the scan kernel to N = 960, the LQ kernel beyond).  N = 2464 is the longest
    horizon a strict plan accepts: that it builds is asserted here, where it is built anyway."""
    assert set(LQ_SHAPES) == set(SC.LQ_HORIZONS)
    case, ref = window_reference("lq", N)
    t0 = time.perf_counter()
    p = Plan(torch.cuda.current_device(), N, case["dt"], SC.WEIGHTS[0][2], SC.G,
             SC.WEIGHTS[0][0], SC.WEIGHTS[0][1], True)
    torch.cuda.synchronize()
    print(f"MEASURED plan N={N}: wall {time.perf_counter() - t0:.2f} s, stages (ms) " +
          " ".join(f"{k} {v:.0f}" for k, v in p.timings().items()))
    try:
        assert p.timings()["total"] > 0.0
        p.set_option("strict_solver", 3)
        o3 = assert_step(p, case, ref, f"lq N={N} solver 3")
        p.set_option("strict_solver", 0)
        o0 = assert_step(p, case, ref, f"lq N={N} auto")
        if N > 960:
            assert np.array_equal(o0, o3)
        roll = SC.lq_rollout_case(N)
        cref, cst, _ = SC.restatement(roll, threads=THREADS)
        assert not cst.any()
        outs = []
        for solver, bounds in ((3, 1), (3, 2), (0, 0)):
            p.set_option("strict_solver", solver)
            p.set_option("strict_bounds", bounds)
            h, st = run_rollout(p, roll)
            assert_hist(h, st, cref, f"lq rollout N={N} solver {solver} bounds {bounds}")
            if N <= SC.LQ_LIVE_MAX:
                assert_hist(h, st, golden("strict_cases.npz")[f"roll{N}_hist"],
                            f"lq rollout N={N} solver {solver}, exact oracle")
            outs.append(h)
        assert np.array_equal(outs[0], outs[1])
        if N > 960:
            assert np.array_equal(outs[2], outs[0])
    finally:
        p.destroy()


@pytest.mark.parametrize("N", SC.SCAN_HORIZONS)
def test_scan_kernel_widest_chunks(N):
    """The scan kernel where it goes from 32 lanes to a whole wave (512 | 513) and at its last
    horizon (960), on the pinned windows, vs the exact oracle (B = 3: whole-wave instances at
    every N; B = 1200 copies at N = 512: 32-lane instances of 16 slots per lane)."""
    case, ref = window_reference("lq", N)
    p = plan(N, case["dt"], solver=4)
    assert_step(p, case, ref, f"scan N={N} B=3")
    if N == 512:
        big = dict(case, x=np.tile(case["x"], (400, 1)), zmax=np.tile(case["zmax"], (400, 1)),
                   zmin=np.tile(case["zmin"], (400, 1)))
        assert_step(p, big, np.tile(ref, (400, 1)), "scan N=512 B=1200")


# ----------------------------------------------------------------------------- e: one bad lane

@pytest.mark.parametrize("solver", (3, 4))
def test_nan_lane_leaves_its_neighbours_alone(solver):
    good, bad = SC.nan_case()
    p = plan(16, good["dt"], solver=solver)
    hg, sg = run_rollout(p, good)
    hb, sb = run_rollout(p, bad)           # (the launch returns)
    others = np.arange(70) != 37
    assert not sg.any() and not sb[others].any()
    assert sb[37] & _native.ST_NONFINITE
    assert np.array_equal(hg[others], hb[others])
    ref, cst, _ = SC.restatement(good, threads=THREADS)
    assert_hist(hg, sg, ref, f"benign B=70 N=16 solver {solver}")
