"""The inputs and the reference of the Herdt shape tests, on the CPU (tests/herdt_cases.py; the
device side is tests/test_gpu_herdt_shapes.py).

Coverage: every batch of step_cases holds the footstep counts and window shapes the device tests
rely on, the rollout cases reach every kernel instance.

The oracle alone (test_oracle_alone_within_bound): on every step case the oracle's solution is
checked by itself — KKT stationarity relative to max(1, ‖p‖∞) (with an empty footstep column:
of the reduced problem herdt_solve solves, i.e. on every other variable), primal violation,
and, for the windows without an empty footstep column, x_next and the first footstep against a
re-solve of the KKT system on the oracle's final active set, iteratively refined with
extended-precision residuals.  Where the first column is empty (M = 0) the footstep is checked
by geometry against the rule: inside the polytope, and equal to the foot or to the nearest of
the foot's projections onto the hull's edges.  Bound 1e-10, ten times under the device tests'
1e-9.  Measured maxima over all 21 batches: stationarity 5.5e-12, primal violation 4.5e-12,
x_next 1.9e-11 (relative to max(1, |x_next|); N = 33), first footstep 9.5e-13, nearest-point
rule 1.7e-16.

The oracle's rollouts (test_rollout_oracle_bounded_and_stable): every walk stays bounded
(|state| <= 10, measured <= 3.3) and its CoM and feet move by <= 1e-10 when x0 moves by 1e-12
(measured <= 5.6e-11; the coarse (N, dt) = (17, 0.07) walks amplify most).
"""
import multiprocessing
import os
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import herdt_cases as HC
from conftest import golden
from oracle import herdt_oracle as HO
from oracle.zmp_oracle import lipm

from mpc_bipedal.controllers import herdt as H

ST, DS, SS = HC.ST, HC.DS, HC.SS
IDS = [f"{N}-{v}" for N, v in HC.STEP_PARAMS]


def _empty_columns(cfg, case, b):
    """Footstep columns of window b that do not enter the objective (zero block of Q)."""
    Q, p, G, h, N, m = HC.window_qp(cfg, case, b)
    return [i for i in range(m) if np.abs(Q[N + i, N:N + m]).sum() == 0.0], m


@pytest.mark.parametrize("N,variant", HC.STEP_PARAMS, ids=IDS)
def test_step_cases_cover_the_window_shapes(N, variant):
    case = HC.step_cases(N, variant)
    cfg = HC.make_config(case["cfg_kw"])
    B = len(case["cur"])
    assert B == (12 if N == 150 else 75 if (N, variant) == (17, "a") else 40)
    assert case["x"].shape == (B, 2, 3) and case["v"].shape == (B, N, 2)
    assert case["win"].shape == (B, N) and case["win"].dtype == np.int8
    m, M = HC.case_m(case)
    # every footstep count the horizon holds, none beyond the device's 8
    assert set(range(HC.max_fit(N) + 1)) <= set(m.tolist()) and m.max() <= 8
    if N >= 16:
        assert set(m.tolist()) == set(range(9))
    assert set(case["side"].tolist()) == {0, 1} and set(case["cur"].tolist()) == {ST, DS, SS}
    # states and feet as specified
    spread = cfg.foot_spread
    assert np.array_equal(case["foot"][:, 1], np.where(case["side"] == 0, spread, -spread))
    assert np.abs(case["x"][:, :, 0] - case["foot"]).max() <= 0.01
    assert np.all(case["v"] == case["v"][:, :1]) and case["v"][..., 0].min() >= 0.0
    assert case["v"][..., 0].max() <= 0.4 and np.abs(case["v"][..., 1]).max() <= 0.05
    win, cur = case["win"], case["cur"]
    allstand = np.all(win == ST, axis=1)
    for c in (ST, DS, SS):
        assert np.any(allstand & (cur == c)), c          # all-standing window under each state
    # the window shapes, by the oracle's own segments and the footstep block of its Q
    seg = [HO.support_segments(int(c), w) for c, w in zip(cur, win)]
    empties = [_empty_columns(cfg, case, b) for b in range(B)]
    for b in range(B):
        e, mq = empties[b]
        assert mq == m[b] == len(seg[b]) - 1
        assert e == ([mq - 1] if M[b] < m[b] else [])     # only the last column can be empty
    assert any(m[b] == 1 and empties[b][0] == [0] for b in range(B))            # M = 0
    assert any(cur[b] == ST and np.any(win[b] != ST) for b in range(B))          # stand → walk
    if N >= 3:
        assert any(m[b] >= 2 and empties[b][0] == [m[b] - 1] for b in range(B))  # empty last
        assert any(cur[b] != ST and win[b, 0] != ST and win[b, -1] == ST and m[b] >= 2
                   for b in range(B))                                            # walk → stand
    # seeded: the same call gives the same batch
    again = HC.step_cases(N, variant)
    assert all(np.array_equal(case[k], again[k]) for k in ("x", "v", "win", "cur", "foot", "side"))


def test_variant_polytopes_and_facet_limit():
    facets = {}
    for variant in "abcd":
        prm = H.make_params(HC.make_config(HC.config_kwargs(17, 0.07, variant)), 8)
        facets[variant] = (prm.nfacets[0], prm.nfacets[1])
    assert facets == {"a": (9, 9), "b": (3, 3), "c": (4, 16), "d": (9, 9)}
    cfg = HC.make_config(HC.config_kwargs(17, 0.07, "b"))
    assert (cfg.foot_length, cfg.foot_width, cfg.foot_spread) == (0.2, 0.1, 0.12)
    mirror = tuple((x, -y) for x, y in cfg.left_foot_polytope)
    assert cfg.right_foot_polytope == mirror
    cfg = HC.make_config(HC.config_kwargs(17, 0.07, "d"))
    assert (cfg.h, cfg.g) == (0.9, 3.71)
    kw = HC.config_kwargs(17, 0.07)
    kw["right_foot_polytope"] = HC.HEPTADECAGON
    with pytest.raises(ValueError, match="17 facets"):
        H.make_params(HC.make_config(kw), 8)


def _nearest_rule_error(cfg, side, foot, q):
    """How far q is from the point of the swing polytope (the hull of the side's vertices, moved
    to the current foot) nearest that foot, found by geometry alone: the foot itself if it lies
    inside, else the nearest of its projections onto the hull's edges (vertices included).
    Asserts on the way that q lies inside and that no edge or vertex is closer to the foot."""
    from scipy.spatial import ConvexHull
    verts = np.asarray(cfg.left_foot_polytope if side == "left" else cfg.right_foot_polytope,
                       np.float64)
    foot = np.asarray(foot, np.float64)
    Ap, bp = HO.polytope_halfspace(verts)
    assert (Ap @ (q - foot) - bp).max() <= 1e-10                    # inside
    hull = verts[ConvexHull(verts).vertices] + foot                 # in order round the hull
    best, dist = foot, 0.0
    if (-bp).max() > 0.0:                                           # the foot lies outside
        dist = np.inf
        for a, b in zip(hull, np.roll(hull, -1, axis=0)):
            t = np.clip((foot - a) @ (b - a) / ((b - a) @ (b - a)), 0.0, 1.0)
            c = a + t * (b - a)
            if np.linalg.norm(c - foot) < dist:
                best, dist = c, float(np.linalg.norm(c - foot))
    assert np.linalg.norm(q - foot) <= dist + 1e-10                 # nothing is closer
    return float(np.abs(q - best).max())


@pytest.mark.parametrize("N,variant", HC.STEP_PARAMS, ids=IDS)
def test_oracle_alone_within_bound(N, variant):
    """See the module docstring for the measured maxima (all batches <= 1.9e-11)."""
    case = HC.step_cases(N, variant)
    cfg = HC.make_config(case["cfg_kw"])
    A, Bm, _ = lipm(cfg.dt, cfg.h, cfg.g)
    m_, M_ = HC.case_m(case)
    worst = dict(stationarity=0.0, primal=0.0, x_next=0.0, footstep=0.0, nearest=0.0)
    for b in range(len(m_)):
        Q, p, G, h, Nq, m = HC.window_qp(cfg, case, b)
        # (raises if the oracle cannot solve the case)
        u, lam = HO.herdt_solve(Q, p, G, h, Nq, m, case["foot"][b])
        n1 = Nq + m
        if len(h):
            worst["primal"] = max(worst["primal"], float((G @ u - h).max()))
            assert lam.min() >= 0.0
        # An empty footstep column is fixed by rule and herdt_solve returns λ = 0 on the rows
        # that only it enters, so r on the other indices is the stationarity of the reduced
        # problem it solved; without an empty column that is every index.
        kept = np.ones(2 * n1, bool)
        if M_[b] < m_[b]:
            kept[[Nq + m - 1, n1 + Nq + m - 1]] = False
        r = (Q @ u + p + (G.T @ lam if len(lam) else 0.0))[kept]
        worst["stationarity"] = max(worst["stationarity"],
                                    float(np.abs(r).max() / max(1.0, np.abs(p).max())))
        if M_[b] < m_[b]:
            if m == 1:   # M = 0: the footstep is the polytope point nearest the current foot
                side = "left" if int(case["side"][b]) == 0 else "right"
                worst["nearest"] = max(worst["nearest"], _nearest_rule_error(
                    cfg, side, case["foot"][b], np.array([u[Nq], u[n1 + Nq]])))
            else:        # M = m − 1: the last footstep enters neither objective nor constraints
                assert not np.any(Q[:, ~kept]) and not np.any(G[:, ~kept])
            continue     # (the re-solve below is for the windows without an empty column)
        ur = HC.refined_kkt(Q, p, G, h, lam)
        for ax, off in ((0, 0), (1, n1)):
            xa = A @ case["x"][b, ax] + Bm[:, 0] * u[off]
            xb = A @ case["x"][b, ax] + Bm[:, 0] * ur[off]
            worst["x_next"] = max(worst["x_next"],
                                  float(np.abs(xa - xb).max() / max(1.0, np.abs(xb).max())))
            if m > 0:
                worst["footstep"] = max(worst["footstep"], float(abs(u[off + Nq] - ur[off + Nq])))
    print(f"oracle alone N={N} {variant}: " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1e-10, (k, v)


def test_rollout_cases_reach_every_kernel_instance():
    cases = HC.rollout_cases()
    inst, kicks = set(), set()
    for c in cases:
        N, n, st = c["cfg_kw"]["horizon"], c["n"], c["states"]
        assert (N, c["cfg_kw"]["dt"]) in {(17, 0.07), (33, 0.03), (40, 0.03), (41, 0.03)}
        assert st.shape == (n,) and c["v"].shape == (n, 2) and c["x0"].shape == (2, 3)
        pad = np.concatenate([st, np.repeat(st[-1:], N)])
        mf = H.max_footsteps(pad[None], N, n)
        assert mf == HC.case_max_footsteps(st, N)
        inst.add(HC.INSTANCE_OF[mf])
        ks = c["kick_step"]
        kicks.add("none" if ks < 0 else "first" if ks == 0 else "last" if ks == n - 2 else
                  "mid" if ks == n // 2 else "other")
    assert inst == {2, 4, 6, 7, 8}
    mfs = {c["name"]: HC.case_max_footsteps(c["states"], c["cfg_kw"]["horizon"]) for c in cases}
    assert [mfs[k] for k in ("n40_ssp9_kickmid", "n40_ssp6_x0", "n40_ssp5_kick0",
                             "n40_midstep_ss_kicklast", "n33_onestep", "seven")] == \
        [5, 6, 8, 4, 2, 7]
    assert {"none", "first", "last", "mid"} <= kicks and "other" not in kicks
    assert {int(c["states"][0]) for c in cases} == {ST, DS, SS}      # two walks start mid-step
    tails = [c for c in cases if c["states"][-1] == ST and
             0 < len(c["states"]) - 1 - np.max(np.nonzero(c["states"])[0]) < c["cfg_kw"]["horizon"]]
    assert len(tails) >= 2                                           # standing tail shorter than N
    assert {c["n"] for c in cases} >= {2, 3} and all(40 <= c["n"] <= 90 or c["n"] <= 3
                                                    for c in cases)
    assert any(np.any(c["x0"] != 0) for c in cases)
    variants = {c["name"]: H.make_params(HC.make_config(c["cfg_kw"]), 8).nfacets[:] for c in cases}
    assert variants["n17_triangle"] == [3, 3] and variants["n33_rect_16gon"] == [4, 16]
    # variant c's walk flips sides (unequal facet counts left and right)
    st = next(c for c in cases if c["name"] == "n33_rect_16gon")["states"]
    assert np.count_nonzero((st[:-1] == SS) & (st[1:] != SS)) >= 2
    # the B = 33 batch: footstep counts differ between the lanes of the first wave
    b = HC.rollout_batch()
    assert b["states"].shape == (33, 40) and b["v"].shape == (33, 40, 2)
    pad = np.concatenate([b["states"], np.repeat(b["states"][:, -1:], 17, axis=1)], axis=1)
    ms = [[len(HO.support_segments(p[i], p[i + 1: i + 18])) - 1 for p in pad[:32]]
          for i in range(39)]
    assert any(len(set(row)) > 1 for row in ms) and max(max(row) for row in ms) <= 8


def test_rollout_oracle_bounded_and_stable():
    """See the module docstring: |state| <= 10 and the response of CoM and feet to
    x0 + 1e-12 <= 1e-10 on every rollout case, and rollout_ref equal to HO.herdt_rollout where
    the case kicks at n // 2 or not at all."""
    keys = [c["name"] for c in HC.rollout_cases()] + [("batch", b) for b in range(33)]
    # spawn, as every pool of the suite: the workers must not inherit a GPU the process may have
    # opened in an earlier test; 15 of them, so that with this process at most 16 exist
    with ProcessPoolExecutor(max_workers=min(15, os.cpu_count() or 1),
                             mp_context=multiprocessing.get_context("spawn")) as ex:
        res = list(ex.map(HC.rollout_probe, keys))
    print("rollout oracle: max |state| %.2f, max response %.1e" % (
        max(r["max_state"] for r in res), max(r["response"] for r in res)))
    for k, r in zip(keys, res):
        assert r["max_state"] <= 10.0, (k, r)
        assert r["response"] <= 1e-10, (k, r)
        assert r["same"] in (None, True), (k, r)
    assert sum(r["same"] is True for r in res) >= 7


def test_stored_long_horizon_inputs_match_the_generator():
    """tests/golden/herdt_shapes.npz holds the inputs long_cases() regenerates from its seed,
    with the footstep counts the device test relies on."""
    d = golden("herdt_shapes.npz")
    for N, k in HC.LONG_HORIZONS.items():
        case = HC.long_cases(N)
        m, M = HC.case_m(case)
        assert len(m) == k and float(d[f"n{N}_dt"]) == case["cfg_kw"]["dt"]
        for key in ("x", "win", "cur", "foot", "side"):
            assert np.array_equal(d[f"n{N}_{key}"], case[key]), (N, key)
        assert np.array_equal(d[f"n{N}_v"], case["v"][:, 0, :])
        assert np.array_equal(d[f"n{N}_m"], m) and np.array_equal(d[f"n{N}_M"], M)
        assert d[f"n{N}_x_next"].shape == (k, 2, 3) and d[f"n{N}_step"].shape == (k, 2)
        assert np.all(np.isfinite(d[f"n{N}_x_next"])) and np.all(np.isfinite(d[f"n{N}_step"]))
        assert np.all(case["cur"] != ST) and np.all(np.any(case["win"] != ST, axis=1))  # walking
    m300, M300 = d["n300_m"], d["n300_M"]
    assert set(m300.tolist()) >= {2, 5, 8} and np.count_nonzero(M300 < m300) == 1
    assert np.all(d["n702_m"] > 0)
