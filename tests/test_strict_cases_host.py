"""The inputs and the references of the strict case tests, on the CPU (tests/strict_cases.py; the
device side is tests/test_gpu_strict_cases.py).

Every case the device file uses is solved here by the exact box-QP oracle, certified by its KKT
report (oracle/zmp_oracle.kkt_check, with zero-width slots as equalities), and by the C
restatement of the device algorithm (oracle/strict_lq_cpu.c), which the device file uses as the
reference of its large batches and longest rollouts.  Bars: KKT residuals, the restatement
against the oracle (relative to max(1, largest |state|)) and the oracle's own response to
x0 + 1e-12 all <= 1e-10, ten times under the device tests' 1e-9.

Measured (8 cores, about 18 s for the file):
  families x N = 1 .. 65 x four weight points (672 walks): stationarity 9.1e-14, primal and dual
    residuals 0, restatement vs oracle 2.0e-14, response to x0 + 1e-12 7.1e-11, largest |state|
    71; every restatement status 0.
  mixed, B = 1200 at N = 64: stationarity 5.0e-15, restatement vs oracle 9.1e-16, response
    3.5e-11 (first 200 walks), largest |state| 39.
  pinned windows (N = 150 .. 2464, m = 0 .. 512): working-set size = m everywhere, stationarity
    <= 6.2e-14, primal and dual residuals 0.
  long-horizon rollouts (n = 6): restatement vs the stored exact oracle <= 1.4e-13 (N <= 897).
"""
import multiprocessing
import os
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import strict_cases as SC
from conftest import golden
from oracle import zmp_oracle as O

BAR = 1e-10
KKT_KEYS = ("primal", "stationarity", "dual_hi", "dual_lo")


def _pool():
    # spawn, as every pool of the suite: the workers must not inherit a GPU the process may have
    # opened in an earlier test; 15 of them, so that with this process at most 16 exist
    return ProcessPoolExecutor(max_workers=min(15, os.cpu_count() or 1),
                               mp_context=multiprocessing.get_context("spawn"))


def _merge(worst, kkt):
    for k in KKT_KEYS:
        worst[k] = max(worst.get(k, 0.0), kkt[k])
    return worst


# ----------------------------------------------------------------------------- kkt_check

def test_kkt_check_zero_width_is_an_equality():
    """A window of zero-width boxes, solved exactly (z = lo = hi): the multipliers of equalities
    are free in sign, so the report holds no dual violation.  (Before the fix every slot counted
    as active at both bounds and dual_hi was the largest positive multiplier.)"""
    N, dt = 16, 0.01
    Q, R, h = SC.WEIGHTS[0]
    H, Px, p0, A, Bv = SC.matrices(N, dt, Q, R, h)
    rng = np.random.default_rng(SC.seed_of("kkt-zero-width"))
    lo = np.cumsum(rng.uniform(-0.01, 0.01, N))
    x = np.array([0.3, -0.5, 1.0])
    u0, W, z, q = O.strict_u0(x, lo.copy(), lo.copy(), H, Px, p0, Q)
    assert np.array_equal(z, lo) and np.all(W != 0)
    gr = (H @ z + q) / max(1.0, np.abs(q).max())
    assert gr.max() > 1e-3 and gr.min() < -1e-3           # multipliers of both signs
    r = O.kkt_check(H, q, z, lo, lo, scale=max(1.0, float(np.abs(q).max())))
    assert max(r.values()) <= 1e-12, r
    # a box with width keeps its dual term: the same point, slot 3 given room above — it then
    # sits at its lower bound and its multiplier is reported (dual_lo = −gradient)
    hi = lo.copy()
    hi[3] += 0.1
    r1 = O.kkt_check(H, q, z, lo, hi)
    assert r1["dual_lo"] == pytest.approx(-(H @ z + q)[3]) and r1["dual_lo"] != 0.0
    assert r1["dual_hi"] == 0.0 and r1["stationarity"] == 0.0
    # and a violated equality shows in `primal`
    z2 = z.copy()
    z2[5] += 1e-3
    assert O.kkt_check(H, q, z2, lo, lo)["primal"] == pytest.approx(1e-3)


def test_walk_with_zero_width_boxes_is_certified():
    """rollout_strict(return_kkt=True) on the `narrow` family (half of the boxes of zero width)
    now certifies its own answers."""
    case = SC.rollout_case("narrow", 33)
    assert np.count_nonzero(case["zmax"] == case["zmin"]) >= case["zmax"].size // 2
    _, kkt = SC.oracle_walk(case, 0, return_kkt=True)
    assert max(kkt.values()) <= BAR, kkt


# ----------------------------------------------------------------------------- the generators

def _centres(case):
    return (case["zmax"] + case["zmin"]) / 2, (case["zmax"] - case["zmin"]) / 2


@pytest.mark.parametrize("family", SC.FAMILIES)
def test_families_as_specified(family):
    case = SC.rollout_case(family, 33)
    again = SC.rollout_case(family, 33)
    assert all(np.array_equal(case[k], again[k]) for k in ("zmax", "zmin", "x0", "kick",
                                                           "kick_step"))
    assert not np.array_equal(case["zmax"], SC.rollout_case(family, 64)["zmax"])
    assert case["zmax"].shape == case["zmin"].shape == (6, 40, 2)
    assert case["x0"].shape == (6, 2, 3) and case["kick"].shape == case["kick_step"].shape == (6,)
    assert np.all(case["zmax"] >= case["zmin"])
    x0 = case["x0"]
    assert np.abs(x0[..., 0]).max() <= 0.5 and np.abs(x0[..., 1]).max() <= 1.0
    assert np.abs(x0[..., 2]).max() <= 3.0 and np.abs(x0[..., 2]).max() > 1.0
    assert np.abs(case["kick"]).max() <= 0.3 and len(set(case["kick_step"].tolist())) > 1
    assert case["kick_step"].min() >= 10 and case["kick_step"].max() < 30
    c, hw = _centres(case)
    dc = np.abs(np.diff(c, axis=1))
    if family == "jitter":
        assert dc.max() <= 0.02 + 1e-15 and dc.min() > 0          # changes every sample
        assert hw.min() >= 0.005 - 1e-15 and hw.max() <= 0.06 + 1e-15
        assert np.all(np.diff(hw, axis=1) != 0)
    elif family == "narrow":
        assert dc.max() <= 0.01 + 1e-15
        assert np.all(np.count_nonzero(case["zmax"] == case["zmin"], axis=1) == 20)
        assert hw.max() <= 0.002
    elif family == "steps":
        assert dc.max() <= 0.3 + 1e-15 and dc.max() > 0.13          # larger than a foot's half
        assert hw.max() <= 0.08 + 1e-15
        for b in range(6):
            for a in range(2):
                edges = np.flatnonzero(np.diff(c[b, :, a]) != 0)
                runs = np.diff(np.concatenate([[-1], edges, [39]]))
                assert runs.max() <= 11 and runs.min() >= 1 and len(runs) >= 4
    else:
        assert np.allclose(hw, 0.01, atol=1e-15)
        d = np.diff(c, axis=1)
        assert np.all(d[:, :-1] * d[:, 1:] < 0)                     # alternates every sample
        assert dc.min() >= 0.2 - 1e-12 and dc.max() <= 0.4 + 1e-12
    # a state far outside its box
    out = np.maximum(x0[..., 0] - case["zmax"][:, 0], case["zmin"][:, 0] - x0[..., 0])
    assert out.max() > 0.1


def test_mixed_batch_neighbours_differ():
    order = SC.mixed_order()
    assert sorted(order) == sorted(SC.MIXED_KINDS) and len(order) == 7
    big = SC.mixed_case(1200)
    kinds = big["kinds"]
    assert all(kinds[b] != kinds[b + 1] for b in range(1199))
    assert all(kinds[b] != kinds[b + 32] for b in range(1200 - 32))   # two 32-lane neighbours
    assert all(set(kinds[b:b + 64]) == set(SC.MIXED_KINDS) for b in range(0, 1200 - 64, 7))
    for B in (40, 200):                                               # prefixes of one another
        small = SC.mixed_case(B)
        assert all(np.array_equal(small[k], big[k][:B]) for k in ("zmax", "zmin", "x0", "kick",
                                                                  "kick_step"))
    c, hw = _centres(big)
    k = np.array(kinds)
    assert hw[k == "wide"].min() == 50.0
    assert np.count_nonzero(hw[k == "pinned"] < 1e-3) >= 8 * np.count_nonzero(k == "pinned")
    assert np.abs(big["x0"][k == "benign"][..., 0]).max() <= 0.01
    assert len(set(big["kick_step"].tolist())) >= 15                  # kick steps per walk


# ----------------------------------------------------------------------------- rollouts

def _check_rollouts(cases, sens_upto=None):
    """cases: list of (label, case, weights).  Every walk by the exact oracle (KKT report,
    response to x0 + 1e-12), every batch by the C restatement."""
    jobs = [(case, b, w, sens_upto is None or b < sens_upto)
            for _, case, w in cases for b in range(len(case["kick"]))]
    with _pool() as ex:
        res = list(ex.map(SC.walk_probe, jobs, chunksize=8))
    worst, resp, diff, big, i = {}, 0.0, 0.0, 0.0, 0
    for label, case, w in cases:
        B = len(case["kick"])
        mine = res[i:i + B]
        i += B
        ref = np.stack([r[0] for r in mine])
        for _, kkt, r in mine:
            _merge(worst, kkt)
            if r is not None:
                resp = max(resp, r)
                assert r <= BAR, (label, r)
            assert max(kkt.values()) <= BAR, (label, kkt)
        hist, status, passes = SC.restatement(case, w)
        assert not status.any(), (label, status)
        assert np.all(passes >= 2 * (ref.shape[1] - 1))
        e = SC.rel_err(hist, ref)
        assert e <= BAR, (label, e)
        diff, big = max(diff, e), max(big, float(np.abs(ref).max()))
    print(" ".join(f"{k} {v:.1e}" for k, v in worst.items()),
          f"restatement {diff:.1e} response {resp:.1e} max|state| {big:.1f}")


@pytest.mark.parametrize("family", SC.FAMILIES)
def test_family_rollouts_oracle_and_restatement(family):
    """See the module docstring for the measured maxima."""
    _check_rollouts([(f"{family}-{N}-{w}", SC.rollout_case(family, N), w)
                     for N in SC.SMALL_HORIZONS for w in SC.WEIGHTS])


def test_mixed_rollouts_oracle_and_restatement():
    """All 1200 walks of the mixed batch (its B = 40 and 200 batches are prefixes)."""
    _check_rollouts([("mixed", SC.mixed_case(1200), SC.WEIGHTS[0])], sens_upto=200)


def test_nan_lane_in_the_restatement():
    """One walk's zmax is NaN from sample 12 on: the C restatement flags that walk alone and
    leaves every other walk's history bitwise as without the NaN."""
    good, bad = SC.nan_case()
    assert np.count_nonzero(np.isnan(bad["zmax"]).any(axis=(1, 2))) == 1
    assert not np.isnan(bad["zmax"][37, :12]).any() and np.isnan(bad["zmax"][37, 12:]).all()
    hg, sg, _ = SC.restatement(good)
    hb, sb, _ = SC.restatement(bad)
    others = np.arange(70) != 37
    assert not sg.any() and not sb[others].any() and sb[37] & 2
    assert np.array_equal(hg[others], hb[others])


# ----------------------------------------------------------------------------- pinned windows

@pytest.mark.parametrize("N", (150, 512))
def test_reduced_cholesky_windows_pin_their_m(N):
    case = SC.chol_case(N)
    assert tuple(case["m"]) == SC.CHOL_M[N]
    if N == 150:   # both sides of every branch of reduced_solve
        assert set(case["m"]) >= {16, 17, 32, 33, 48, 49, 64, 65, 128, 129, 150}
    out, m, worst = SC.solve_windows(case)
    print(N, " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert np.array_equal(m, case["m"])
    assert max(worst.values()) <= BAR and np.all(np.isfinite(out))


@pytest.mark.parametrize("N", [N for N in SC.LQ_HORIZONS if N <= SC.LQ_LIVE_MAX] +
                         [N for N in SC.SCAN_HORIZONS])
def test_long_windows_pin_their_m(N):
    case = SC.lq_case(N)
    NS = (N + 7) // 8
    for hi, lo in zip(case["zmax"], case["zmin"]):
        pos = set(np.flatnonzero(hi - lo < 1e-3).tolist())
        assert {1, 3, 7, 8, N - 1} <= pos                    # first segment, its edge, the end
        segs = {p // 8 for p in pos}
        assert {NS - 1, NS - 2, NS - 3} <= segs              # LDS checkpoints: NS − 2, NS − 3
        assert {NS // 2, NS // 3, NS // 5} <= segs           # global checkpoints
    out, m, worst = SC.solve_windows(case)
    print(N, " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert np.array_equal(m, SC.LQ_M) and max(worst.values()) <= BAR


def test_stored_answers_match_the_generator():
    """tests/golden/strict_cases.npz: the cold windows at N >= 1600 pin their m and are KKT
    points; the stored N = 1601 answers and the stored N = 320 rollout equal a fresh solve of the
    regenerated inputs."""
    d = golden("strict_cases.npz")
    assert tuple(d["kkt_keys"]) == KKT_KEYS
    seeds = d["seeds"].tolist()
    for N in SC.LQ_HORIZONS:
        if N > SC.LQ_LIVE_MAX:
            assert d[f"step{N}_out"].shape == (3, 3) and np.all(np.isfinite(d[f"step{N}_out"]))
            assert np.array_equal(d[f"step{N}_m"], SC.LQ_M)
            assert d[f"step{N}_kkt"].max() <= BAR
            assert all(SC.seed_of(f"pinned-lq-N{N}-m{m}") in seeds for m in SC.LQ_M)
        else:
            assert d[f"roll{N}_hist"].shape == (3, 6, 2, 3) and d[f"roll{N}_kkt"].max() <= BAR
            assert SC.seed_of(f"pinned-lq-rollout-N{N}-n6") in seeds
    out, m, worst = SC.solve_windows(SC.lq_case(1601))
    assert np.array_equal(m, SC.LQ_M)
    assert SC.rel_err(out, d["step1601_out"]) <= 1e-12
    case = SC.lq_rollout_case(320)
    fresh = np.stack([SC.oracle_walk(case, b) for b in range(3)])
    assert SC.rel_err(fresh, d["roll320_hist"]) <= 1e-12


def test_long_rollouts_restatement_vs_stored_oracle():
    """The six-sample rollouts at every LQ horizon: the C restatement returns status 0 and, at
    N <= 897, the stored exact-oracle histories."""
    d = golden("strict_cases.npz")
    worst = 0.0
    for N in SC.LQ_HORIZONS:
        case = SC.lq_rollout_case(N)
        assert case["zmax"].shape == (3, 6, 2)
        hist, status, passes = SC.restatement(case)
        assert not status.any() and np.all(np.isfinite(hist)), N
        if N <= SC.LQ_LIVE_MAX:
            e = SC.rel_err(hist, d[f"roll{N}_hist"])
            worst = max(worst, e)
            assert e <= BAR, (N, e)
    print(f"long rollouts: restatement vs oracle {worst:.1e}")
