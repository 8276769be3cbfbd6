"""Herdt walk metrics without a GPU (zmpc_herdt_walk_metrics): the symbol and its binding, every
argument check of the C-ABI, and the NumPy statement of the metric (analysis.
herdt_walk_metrics_reference) on the oracle's walks — the rules of include/zmpc.h hold the
realised ZMP inside its box on every walk, the landed steps inside their polytope, and the DCM
verdict gives an interval-shaped passing set under a shove."""
import ctypes
import multiprocessing
import os
import re
import subprocess
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import herdt_cases as hc
import herdt_metrics_cases as mc

from mpc_bipedal import _native  # noqa: E402
from mpc_bipedal import analysis  # noqa: E402
from mpc_bipedal.config import MPCConfig  # noqa: E402

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
    prm = mc.make_params()
    lib.zmpc_herdt_walk_metrics(ctypes.addressof(blk), ctypes.addressof(prm), 0, 2, PTR, PTR, PTR,
                                0, None, 0, None, 0.0, PTR, None)


def test_symbol_exported_and_bound(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True,
                         text=True).stdout
    assert "zmpc_herdt_walk_metrics" in set(re.findall(r" T (zmpc_\w+)", out))
    res, args = _native.SIGNATURES["zmpc_herdt_walk_metrics"]
    assert res is ctypes.c_int and len(args) == 14
    assert lib.zmpc_herdt_walk_metrics.argtypes == args
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                               "include", "zmpc.h")).read()
    assert re.search(r"#define ZMPC_NHERDT_METRICS 16\b", header)
    assert _native.NHERDT_METRICS == analysis.NHERDT_METRICS == 16
    assert len(analysis.HERDT_SLOT_NAMES) == 7
    assert lib.zmpc_abi_version() == _native.ABI_VERSION == 7  # additive: the version stays


def test_argument_checks_without_gpu(lib):
    """Every bad argument is ZMPC_EINVAL with a message, before any device call.  The plan is
    never dereferenced on these paths, so a zeroed block stands in for one."""
    fake_plan = ctypes.create_string_buffer(4096)
    plan = ctypes.addressof(fake_plan)
    good = mc.make_params()

    def call(plan=plan, prm=good, B=2, n=10, hist=PTR, foot=PTR, st=PTR, ss=10, ref=PTR, rs=20,
             lengths=None, tol=1e-9, metrics=PTR):
        rc = lib.zmpc_herdt_walk_metrics(plan, None if prm is None else ctypes.addressof(prm), B,
                                         n, hist, foot, st, ss, ref, rs, lengths, tol, metrics,
                                         None)
        return rc, lib.zmpc_last_error()

    for bad in (dict(plan=None), dict(prm=None)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"NULL plan or params" in msg, bad
    for bad in (dict(hist=None), dict(foot=None), dict(st=None), dict(metrics=None)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"NULL array" in msg, bad
    for bad in (dict(B=-1), dict(n=0), dict(n=-3)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"B >= 0 and n >= 1" in msg, bad
    for tol in (-1e-300, -1.0, float("nan"), -float("inf")):
        rc, msg = call(tol=tol)
        assert rc == _native.ZMPC_EINVAL and b"count_tol" in msg, tol
    for side in (0, 1):
        for nf in (-1, 17):
            prm = mc.make_params()
            prm.nfacets[side] = nf
            rc, msg = call(prm=prm)
            assert rc == _native.ZMPC_EINVAL and b"facets" in msg, (side, nf)
    for bad in (dict(ss=9), dict(ss=-10), dict(rs=19), dict(rs=1), dict(ref=None, rs=19)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"stride" in msg, bad
    rc, msg = call(B=2 ** 31)
    assert rc == _native.ZMPC_EINVAL and b"batch too large" in msg
    rc, msg = call(n=2 ** 24 + 1, ss=0, rs=0)
    assert rc == _native.ZMPC_EINVAL and b"walk too long" in msg
    # an empty batch is a no-op, NULL arrays included; no facets at all are fine
    assert call(B=0) == (0, b"")
    assert call(B=0, hist=None, foot=None, st=None, metrics=None, ref=None, rs=0) == (0, b"")
    assert call(B=0, prm=mc.make_params(nfacets=False)) == (0, b"")


def test_named_columns():
    data = np.arange(32.0).reshape(2, 16)
    m = analysis.HerdtWalkMetrics(data)
    assert len(m) == 2 and m.dcm_dev_max.tolist() == [[8.0, 9.0], [24.0, 25.0]]
    assert m.step_shift_max[:, 1].tolist() == [13.0, 29.0]
    assert m.reach_slack_min.tolist() == [14.0, 30.0] and m.steps_landed.tolist() == [15.0, 31.0]
    with pytest.raises(AttributeError):
        m.zmp_rms
    with pytest.raises(ValueError):
        analysis.HerdtWalkMetrics(np.zeros((2, 12)))


def test_reference_rules_by_hand():
    """The statement on a walk small enough to do by hand: sample i against foot[i − 1], the
    STANDING hull on the side the landings leave, the landing's slack from its side's facets."""
    n = 6
    st = np.array([mc.ST, mc.SS, mc.DS, mc.SS, mc.ST, mc.ST], np.int8)   # landings at 1 and 3
    foot = np.array([[0.0, 0.1]] * 2 + [[0.3, -0.1]] * 2 + [[0.6, 0.1]] * 2)
    hist = np.zeros((1, n, 2, 3))
    hist[0, :, :, 0] = foot[np.maximum(np.arange(n) - 1, 0)]             # the CoM on its foot
    hist[0, 2, 0, 0] = 0.0 + 0.1 + 0.03     # sample 2 (x): 3 cm past the box of foot[1], not [2]
    hist[0, 5, 1, 0] = 0.1 + 0.05 + 0.02    # sample 5 (y, STANDING): the other foot is at −0.14
    fac = (np.array([[1.0, 0.0, 0.35]]), np.array([[0.0, 1.0, 0.25]]))
    m = analysis.herdt_walk_metrics_reference(hist, foot[None], st, mc.HG, 0.2, 0.1, 0.12,
                                              facets=fac, count_tol=0.0)[0]
    assert m[15] == 2 and np.isclose(m[0], 0.03) and m[2] == 2 and m[4] == 1
    assert np.isclose(m[1], 0.02) and m[3] == 5 and m[5] == 1
    # landing 1 is the left side's (0.35 − 0.3), landing 2 the right side's (0.25 − 0.2)
    assert np.isclose(m[14], 0.05)
    # the same excursion towards the other foot stays inside the hull
    hist[0, 5, 1, 0] = 0.1 - 0.05 - 0.02
    m = analysis.herdt_walk_metrics_reference(hist, foot[None], st, mc.HG, 0.2, 0.1, 0.12,
                                              facets=fac, count_tol=0.0)[0]
    assert m[1] == 0 and m[3] == -1
    # step_shift_max against a nominal walk
    m = analysis.herdt_walk_metrics_reference(hist, foot[None], st, mc.HG, 0.2, 0.1, 0.12,
                                              foot_ref=foot - [0.0, 0.04])[0]
    assert m[12] == 0 and np.isclose(m[13], 0.04)


@pytest.fixture(scope="module")
def oracle_walks():
    keys = mc.walk_keys()
    with _pool() as pool:
        return keys, list(pool.map(mc.oracle_walk, keys))


def test_reference_on_the_oracles_walks(oracle_walks):
    """On the 11 rollout_cases(), the 10 pushed HERDT_WALKS and the 33 pushed rollout_batch()
    walks of the oracle the realised ZMP stays in the box of foot[i − 1] to the project's bar
    (1.7e-13 m measured) and every landed step inside its swing polytope.  Pairing sample i with
    foot[i] instead reports a step length at every landing."""
    keys, walks = oracle_walks
    assert len(keys) == 54
    worst_v, worst_s, landed = 0.0, np.inf, 0
    for key, (kw, st, hist, foot) in zip(keys, walks):
        cfg = MPCConfig(**kw)
        m = mc.walk_reference(cfg, st, hist, foot)
        assert np.isfinite(m[:14]).all(), key
        assert m[0:2].max() <= 1e-9, (key, m[0:2])
        assert m[14] >= -1e-9, (key, m[14])
        assert m[15] == len(mc.landings_of(st)), key
        assert (m[4:6] == 0).all(), key
        worst_v, worst_s, landed = max(worst_v, m[0:2].max()), min(worst_s, m[14]), landed + m[15]
    print(f"54 oracle walks: viol_max {worst_v:.3g}, reach_slack_min {worst_s:.3g}, "
          f"{int(landed)} landings")
    assert landed > 100
    # the wrong pairing, on a walk that steps: shift the feet by one row
    kw, st, hist, foot = walks[0]
    wrong = np.concatenate([foot[1:], foot[-1:]])
    m = mc.walk_reference(MPCConfig(**kw), st, hist, wrong)
    assert m[0] > 0.01


def test_oracle_bisection_gives_an_interval():
    """n17_triangle under a 5-sample half-sine shove from step 25, max_dcm_dev = 1 m: in each of
    the four directions the oracle's bisection lands on the critical force of the issue, the
    passing set over 41 samples of [0, 2F*] is one interval from 0, and dcm_dev_max rises through
    the bound across F*·(1 ± 1e-3)."""
    with _pool() as pool:
        out = list(pool.map(mc.shove_probe, mc.SHOVES))
    for (direction, fstar), (lo, hi, sweep, near) in zip(mc.SHOVES, out):
        print(f"shove {direction}: bracket [{lo:.4f}, {hi:.4f}] N, dcm_dev_max {near}")
        assert lo <= fstar + 5e-5 and hi >= fstar - 5e-5 and hi - lo == 1000.0 / 2 ** 24
        k = sweep.index(False)  # (sample 20 is F* to four decimals: either side of the bracket)
        assert k in (20, 21) and all(sweep[:k]) and not any(sweep[k:]), (direction, sweep)
        assert near[0] < mc.MAX_DCM_DEV < near[1]


def test_unpushed_walk_is_far_from_the_bound():
    """The verdict's scale: unpushed and under a push it recovers from, the DCM of n17_triangle
    stays within a step length of its foot; past the critical push it runs away while the ZMP
    stays in its box (the QP is always feasible)."""
    quiet, gone = mc.shove_metrics(40.0, (0.0, -1.0)), mc.shove_metrics(160.0, (0.0, -1.0))
    assert quiet[8:10].max() < 0.5 and gone[8:10].max() > 10.0
    assert quiet[0:2].max() <= 1e-9 and gone[0:2].max() <= 1e-9
