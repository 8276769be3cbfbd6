"""Seeded inputs, oracle walks and comparison helpers shared by the tests of the Herdt walk
metrics (the host tests, tests/test_herdt_metrics_host.py; the host emulation of the kernel,
tests/test_herdt_metrics_emulation.py; the device tests, tests/test_gpu_herdt_metrics.py).  Not a
test module."""
import numpy as np

import herdt_cases as hc
import push_rollout_cases as pr
import push_shaped_cases as ps
from mpc_bipedal.analysis import (Push, herdt_params_facets, herdt_walk_metrics_reference)

HG = 0.75 / 9.81
ST, DS, SS = hc.ST, hc.DS, hc.SS

# ----------------------------------------------------------------------------- kernel cases
GEOM = dict(foot_length=0.2, foot_width=0.1, foot_spread=0.12)
# (a_x, a_y, b) rows: three facets for the left foot's steps, four for the right foot's
FACETS = (np.array([[1.0, 0.25, 0.08], [-0.5, 1.0, 0.05], [-0.25, -1.0, 0.11]]),
          np.array([[1.0, 0.0, 0.07], [0.0, 1.0, 0.09], [-1.0, 0.0, 0.06], [0.0, -1.0, 0.04]]))
COUNT_TOL = 0.01
EMU_B = 5                        # one full workgroup of four walks and a tail
EMU_N = (1, 2, 3, 64, 65, 129)   # below, at and past one and two 64-lane passes
# landings per walk: at steps 62, 63 and 64 (the last lanes of a block and the first of the next:
# the parity crosses lanes and blocks), in consecutive blocks, an even and an odd number; walk 4
# never lands (all STANDING: the hull on the left side)
LANDINGS = ((5, 62, 70, 100, 126), (10, 63, 90), (20, 64, 66, 125), (61, 63, 65, 120), ())
TAIL = 2                         # STANDING samples at the end of walks 0-3


def schedule(n, steps, standing=False):
    """int8 states [n]: DOUBLE_SUPPORT with one SINGLE_SUPPORT sample at every step of `steps`
    (a landing there when the next sample exists), two STANDING samples first and TAIL last;
    standing=True: STANDING throughout."""
    st = np.full(n, ST if standing else DS, np.int8)
    if standing:
        return st
    st[:2] = ST
    for k in steps:
        if k < n:
            st[k] = SS
    if n > 8:
        st[n - TAIL:] = ST
    return st


def landings_of(st, nb=None):
    """Steps k of a schedule with a landing (the statement of include/zmpc.h, L_k)."""
    nb = len(st) if nb is None else nb
    return [k for k in range(nb - 1) if st[k] == SS and st[k + 1] != SS]


def emu_case(n, shared_states=False, ref="none", B=EMU_B):
    """Seeded random history (not a rollout) of O(0.1) magnitude round random feet, so that about
    half of the ZMP samples leave their box → dict(hist [B,n,2,3], foot [B,n,2], states [B,n] or
    [n], foot_ref None, [n,2] ("shared") or [B,n,2] ("walk"))."""
    rng = np.random.default_rng([20260412, n, int(shared_states), len(ref)])
    foot = rng.uniform(-0.05, 0.05, (B, n, 2))
    hist = rng.uniform(-1.0, 1.0, (B, n, 2, 3)) * np.array([0.1, 0.5, 1.0])
    states = np.stack([schedule(n, LANDINGS[b % 5], standing=(b % 5 == 4)) for b in range(B)])
    if shared_states:
        states = states[0]
    fr = None
    if ref != "none":
        fr = rng.uniform(-0.05, 0.05, (n, 2) if ref == "shared" else (B, n, 2))
    return dict(hist=hist, foot=foot, states=states, foot_ref=fr, lengths=None)


def hostile_case():
    """B = 8, n = 129: ragged lengths (1, 64, 65, 129) whose dead tails hold NaN and 1e300, a walk
    with no violation, a tie of the largest violation in lanes 63 and 64, a NaN velocity on one
    axis, a NaN foot coordinate, and STANDING tails reached after an odd and an even number of
    landings."""
    n = 129
    c = emu_case(n, False, "walk", B=8)
    hist, foot, states, fr = c["hist"], c["foot"], c["states"], c["foot_ref"]
    lengths = np.array([1, 64, 65, 129, 129, 129, 129, 129])
    for b, nb in enumerate(lengths):  # dead tails never reach a result
        hist[b, nb:], foot[b, nb:], fr[b, nb:] = np.nan, 1e300, np.nan
        states[b, nb:] = DS  # (walk 1 ends on a SINGLE_SUPPORT sample: no landing past the end)
    # walk 3: no violation at all (the CoM, still, on its supporting foot)
    hist[3] = 0.0
    foot[3] = 0.0
    # walk 4: the largest violation twice, in lane 63 of the first block and lane 0 of the second
    states[4] = DS
    hist[4, 63] = hist[4, 64] = [[5.0, 0.0, 0.0], [-5.0, 0.0, 0.0]]
    foot[4, 63] = foot[4, 62]
    hist[5, 70, 1, 1] = np.nan   # walk 5: the y axis meets a NaN velocity at sample 70
    foot[6, 33, 0] = np.nan      # walk 6: the x axis meets a NaN foot coordinate at row 33
    c["lengths"] = lengths
    return c


def reference(case, hg=HG, count_tol=COUNT_TOL, facets=FACETS, geom=GEOM):
    return herdt_walk_metrics_reference(case["hist"], case["foot"], case["states"], hg,
                                        facets=facets, lengths=case["lengths"],
                                        foot_ref=case["foot_ref"], count_tol=count_tol, **geom)


def tol_is_clear(case, **kw):
    """True when no sample's violation lies within 1e-12 of COUNT_TOL: the counts then do not
    depend on the last bits of v."""
    a = reference(case, count_tol=COUNT_TOL - 1e-12, **kw)
    b = reference(case, count_tol=COUNT_TOL + 1e-12, **kw)
    return np.array_equal(a[:, 4:6], b[:, 4:6], equal_nan=True)


def make_params(nfacets=True, geom=GEOM, facets=FACETS):
    """A HerdtParams holding GEOM and FACETS (nfacets=False: no facets at all)."""
    from mpc_bipedal.controllers.herdt import HerdtParams
    p = HerdtParams()
    p.foot_length, p.foot_width, p.foot_spread = (geom[k] for k in ("foot_length", "foot_width",
                                                                    "foot_spread"))
    p.alpha = p.beta = p.gamma = 1.0
    if nfacets:
        for sd, f in enumerate(facets):
            p.nfacets[sd] = len(f)
            for k, row in enumerate(f):
                for c in range(3):
                    p.facets[sd][k][c] = float(row[c])
    return p


INT_SLOTS = (2, 3, 4, 5, 15)     # viol_argmax, viol_count, steps_landed


def assert_exact(got, want):
    """Every slot equal, NaN and inf where the statement has them."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    for s in range(want.shape[1]):
        np.testing.assert_array_equal(got[:, s], want[:, s], err_msg=f"slot {s}")


def assert_close(got, want, rtol=1e-12):
    """The integer slots equal, the others within rtol relative."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    for s in range(want.shape[1]):
        if s in INT_SLOTS:
            np.testing.assert_array_equal(got[:, s], want[:, s], err_msg=f"slot {s}")
        else:
            np.testing.assert_allclose(got[:, s], want[:, s], rtol=rtol, atol=0,
                                       err_msg=f"slot {s}")


# ----------------------------------------------------------------------------- oracle walks

def walk_keys():
    """The 54 walks of the oracle the metric's rules were checked on: the 11 rollout_cases(), the
    5 HERDT_WALKS under both profiles, the 33 walks of rollout_batch() under the device test's
    push."""
    keys = [("case", c["name"]) for c in hc.rollout_cases()]
    keys += [("pushed", name, prof) for name in pr.HERDT_WALKS for prof in ("half_sine", "ramp")]
    keys += [("batch", b) for b in range(33)]
    return keys


def config_facets(cfg):
    from mpc_bipedal.controllers import herdt
    return herdt_params_facets(herdt.make_params(cfg, 0))


def oracle_walk(key):
    """Pool worker: one walk of walk_keys() on the oracle → (cfg_kw, states [n], hist [n,2,3],
    foot [n,2])."""
    if key[0] == "case":
        case = pr.herdt_case(key[1])
        kw, st = case["cfg_kw"], case["states"]
        _, yh, foot, xh = hc.rollout_reference(key[1])
    elif key[0] == "pushed":
        case = pr.herdt_case(key[1])
        kw, st = case["cfg_kw"], case["states"]
        dvel = pr.herdt_window(case, ps.half_sine if key[2] == "half_sine" else pr.ramp)[2]
        _, yh, foot, xh = pr.herdt_rollout_pushed(hc.make_config(kw), case["x0"], case["v"], st,
                                                  dvel)
    else:
        batch = hc.rollout_batch()
        b, n, kw = key[1], batch["n"], batch["cfg_kw"]
        st = batch["states"][b]
        s = int(pr.herdt_batch_steps(n, len(batch["x0"]))[b])
        dvel = pr.window(n, s, pr.HERDT_D, ps.half_sine(pr.HERDT_D), pr.HERDT_BATCH_AMP)
        _, yh, foot, xh = pr.herdt_rollout_pushed(hc.make_config(kw), batch["x0"][b],
                                                  batch["v"][b], st, dvel)
    return kw, np.asarray(st), np.stack([xh, yh], axis=1), np.asarray(foot)


def walk_reference(cfg, states, hist, foot, foot_ref=None, count_tol=1e-9):
    """herdt_walk_metrics_reference of one walk [n, ...] under its MPCConfig → [16]."""
    return herdt_walk_metrics_reference(
        hist[None], foot[None], states, cfg.h / cfg.g, cfg.foot_length, cfg.foot_width,
        cfg.foot_spread, facets=config_facets(cfg), count_tol=count_tol,
        foot_ref=None if foot_ref is None else foot_ref[None])[0]


# ----------------------------------------------------------------------------- the shove

SHOVE_WALK = "n17_triangle"      # N = 17, dt = 0.07, n = 50
SHOVE_STEP, SHOVE_D = 25, 5      # a 5-sample half-sine from step 25 on
MAX_DCM_DEV = 1.0
# direction → the critical force the oracle's bisection gave, N
SHOVES = (((0.0, -1.0), 77.2629), ((0.0, 1.0), 115.0752), ((1.0, 0.0), 103.8922),
          ((0.6, 0.8), 144.0061))


def shove_dvel(cfg, n, F, direction):
    """dvel [n, 2] of a half-sine shove of F newtons along `direction`, as Push states it."""
    push = Push(float(F), np.asarray(direction, np.float64)[None], SHOVE_STEP, duration=SHOVE_D,
                profile=ps.half_sine(SHOVE_D))
    return push.velocity_steps(cfg.dt, cfg.m, 1, n)[0]


def shove_metrics(F, direction):
    """The oracle's walk under the shove → its metrics [16] (reference statement)."""
    case = pr.herdt_case(SHOVE_WALK)
    cfg = hc.make_config(case["cfg_kw"])
    _, yh, foot, xh = pr.herdt_rollout_pushed(cfg, case["x0"], case["v"], case["states"],
                                              shove_dvel(cfg, case["n"], F, direction))
    return walk_reference(cfg, case["states"], np.stack([xh, yh], axis=1), foot)


def shove_passes(F, direction, max_dcm_dev=MAX_DCM_DEV, max_violation=1e-9):
    m = shove_metrics(F, direction)
    return bool((m[0:2] <= max_violation).all() and (m[8:10] <= max_dcm_dev).all())


def shove_probe(job):
    """Pool worker: (direction, F*) → (bisection bracket of the oracle over [0, 1000] to 1000/2²⁴,
    pass/fail over 41 samples of [0, 2F*], dcm_dev_max (worse axis) at F*·(1 ∓ 1e-3))."""
    direction, fstar = job
    lo, hi = 0.0, 1000.0
    for _ in range(24):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if shove_passes(mid, direction) else (lo, mid)
    sweep = [shove_passes(F, direction) for F in np.linspace(0.0, 2 * fstar, 41)]
    near = [float(shove_metrics(fstar * (1 + e), direction)[8:10].max()) for e in (-1e-3, 1e-3)]
    return lo, hi, sweep, near
