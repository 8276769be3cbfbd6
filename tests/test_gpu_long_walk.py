"""The long-walk rollout kernels (csrc/rollout_long.hip: the wide kernel's 32 instances and the
chunk kernel, and the one-wave kernel past 64 KiB of LDS) against the extended-precision truth of
tests/long_walk_cases.py, whose cases, bars and sensitivity the host test
tests/test_long_walk_cases_host.py proves on the CPU.

Every history is held to the np.longdouble recursion with the refined gain row, relative to
max(1, max |truth|) of the case; the bar is max(1e-12, 16·e64), for an FFT leg
max(1e-12, 16·max(e64, efft64)), both distances measured on float64 references and never on the
device.  Families: A every reachable (W, CW, E, sparse staged, LDS > 64 KiB) answer of the launch
rule at both ends of its range, B walk ends (a wave of the 8-wave kernel wholly past the end),
C the chunk kernel (partial and one-step chunks, 69 and 141 KB of LDS, the one-wave kernel at
105 KB), D kick placement (wave and chunk boundaries, step 0 and n − 2, out-of-range steps,
per-walk steps), E correlation forms around kSparseMaxWide, F weight points, G a 1000 m offset,
H more walks than two dispatch rounds, I a shared CoP, J non-finite input.

`pytest -s` prints the error and the bar of every launch and, at the end, the worst per kernel
family.
"""
import numpy as np
import pytest
import torch

import long_walk_cases as LC

pytestmark = pytest.mark.gpu

from mpc_bipedal.solver import Plan  # noqa: E402
from mpc_bipedal import _native  # noqa: E402

_PLANS = {}
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    _native.load()
    yield
    for p in _PLANS.values():
        p.destroy()
    _PLANS.clear()
    print("\ndevice vs truth, per kernel family: launches, worst error / bar (its bar)")
    for fam, (count, err, bar, ratio) in sorted(_WORST.items()):
        print(f"  {fam}: {count} launches, {err:.1e} ({bar:.1e}), {ratio:.3f} of the bar")


def plan(case):
    key = (case.N, case.w)
    if key not in _PLANS:
        Q, R, h, g = LC.POINTS[case.w]
        _PLANS[key] = Plan(torch.cuda.current_device(), case.N, LC.case_dt(case.N), h, g, Q, R,
                           False)
    return _PLANS[key]


def launch(case, opt, rc, kick=True, kick_step=None):
    """One rollout of the batch rc under the options of opt → (hist, status) on the host."""
    p = plan(case).set_option("long_walk", opt.long_walk).set_option("correlation",
                                                                     opt.correlation)
    ks = rc["kick_step"] if kick_step is None else kick_step
    ks = int(ks) if np.ndim(ks) == 0 else np.array(ks, np.int64)
    h, st = p.rollout(np.array(rc["zmax"]), np.array(rc["zmin"]), np.array(rc["x0"]),
                      kick=np.array(rc["kick"]) if kick else None, kick_step=ks)
    return h.cpu().numpy(), st.cpu().numpy()


def family_of(opt):
    return {"Wide": "wide FFT" if opt.fft else "wide direct/sparse", "Chunk": "chunk",
            "Generic": "one-wave"}[opt.kind]


def hold(case, opt, hist, status, ref, what=""):
    """The history of one launch against the truth ref, at the bar of (case, opt)."""
    assert not status.any(), (case.name, opt, status)
    err, bar = LC.rel_err(hist, ref), LC.bar(case, opt)
    print(f"\n{case.name} lw={opt.long_walk} corr={opt.correlation} {what}: {err:.2e} "
          f"(bar {bar:.1e})")
    w = _WORST.get(family_of(opt), (0, 0.0, bar, -1.0))
    _WORST[family_of(opt)] = (w[0] + 1,) + ((err, bar, err / bar) if err / bar > w[3] else w[1:])
    assert err <= bar, (case.name, opt, what, err, bar)


def ids(cases):
    return [c.name for c in cases]


PLAIN = [c for c in LC.all_cases() if c.family in "ABCFG"]


@pytest.mark.parametrize("case", PLAIN, ids=ids(PLAIN))
def test_long_walk_vs_truth(case):
    """Families A, B, C, F and G: every launch of the case, per-walk kicks at per-walk steps."""
    rc, ref = LC.batch(case), LC.truth(case)
    for opt in case.opts:
        h, st = launch(case, opt, rc)
        hold(case, opt, h, st, ref)


@pytest.mark.parametrize("case", LC.family("D"), ids=ids(LC.family("D")))
def test_kick_placement(case):
    """Launch-wide kick steps at the first and last step, on both sides of a lane, a wave and a
    chunk boundary and at the last wave's or chunk's first step, each against the truth; steps
    −1, n − 1 and n + 4 bit-identical to a launch without a kick; and the same placements as
    per-walk steps mixed over the walks of one launch."""
    rc = LC.batch(case)
    steps, outside = LC.kick_placements(case)
    for opt in case.opts:
        plain, st = launch(case, opt, rc, kick=False)
        hold(case, opt, plain, st, LC.truth(case, kick_step=-1), "no kick")
        for s in steps:
            h, st = launch(case, opt, rc, kick_step=s)
            hold(case, opt, h, st, LC.truth(case, kick_step=s), f"kick at {s}")
            assert not np.array_equal(h, plain)
        for s in outside:
            h, st = launch(case, opt, rc, kick_step=s)
            assert not st.any() and np.array_equal(h, plain), (case.name, opt, s)
        for ks in LC.per_walk_kick_steps(case):
            h, st = launch(case, opt, rc, kick_step=ks)
            hold(case, opt, h, st, LC.truth(case, kick_step=ks), f"per-walk kicks {ks.tolist()}")
            out = np.isin(ks, outside)
            assert out.any() and not out.all()
            assert np.array_equal(h[out], plain[out]), (case.name, opt, ks)


@pytest.mark.parametrize("case", LC.family("E"), ids=ids(LC.family("E")))
def test_correlation_forms(case):
    """0, 1, 63, 64 and 65 z_ref changes per axis, an x-sparse y-dense walk, changes at the walk's
    ends, across a wave boundary and N − 1 and N samples ahead of a wave's first output: the direct
    and the FFT instance, with and without the sparse attempt, all four against the truth."""
    rc, ref = LC.batch(case), LC.truth(case)
    for opt in case.opts:
        h, st = launch(case, opt, rc)
        hold(case, opt, h, st, ref)


@pytest.mark.parametrize("case", LC.family("H"), ids=ids(LC.family("H")))
def test_more_walks_than_two_rounds(case):
    """2·(16/W)·CUs + 37 walks, more than two rounds at any occupancy, so the launch goes without
    the next-round prefetch: eight distinct walks repeated and a ninth as the last, every walk
    compared with its truth."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    idx = LC.big_batch_index(case, cus)
    rc, ref = LC.batch(case), LC.truth(case)
    big = {key: v[idx] for key, v in rc.items()}
    opt = case.opts[0]
    h, st = launch(case, opt, big)
    assert h.shape[0] == len(idx) == 2 * (16 // LC.wide_shape(case.n)[0]) * cus + 37
    assert not st.any()
    scale = max(1.0, float(np.abs(ref).max()))
    err = max(float(np.abs(h[idx == j] - ref[j]).max()) for j in range(9)) / scale
    bar = LC.bar(case, opt)
    print(f"\n{case.name} B={len(idx)}: {err:.2e} (bar {bar:.1e})")
    assert err <= bar, (case.name, err, bar)
    assert not np.array_equal(h[-1], h[len(idx) - 2])


@pytest.mark.parametrize("case", LC.family("I"), ids=ids(LC.family("I")))
def test_shared_cop(case):
    """One CoP for every walk: the shared form (bounds [n, 2], stride 0) and the same bounds
    repeated per walk, both against the truth."""
    rc, ref = LC.batch(case), LC.truth(case)
    zmax, zmin = LC.per_walk_bounds(case, rc)
    for opt in case.opts:
        h, st = launch(case, opt, rc)
        hold(case, opt, h, st, ref, "shared")
        h, st = launch(case, opt, dict(rc, zmax=zmax, zmin=zmin))
        hold(case, opt, h, st, ref, "repeated")


@pytest.mark.parametrize("where", LC.J_WHERE)
@pytest.mark.parametrize("case", LC.family("J"), ids=ids(LC.family("J")))
def test_nonfinite_walk_is_flagged_alone(case, where):
    """One walk of six with a NaN in x0, in a bound at sample 0, at sample n − 1 or in the last
    wave's and chunk's range, or with zmax = +inf and zmin = −inf at one sample: that walk reports
    ZMPC_ST_NONFINITE, every other walk has status 0 and the clean batch's history bit for bit.
    (Sample 0 of the bounds has weight zero in every window; the direct form and the chunk kernel,
    which never read it, reported status 0 there until their status epilogue looked at it.)"""
    rc, opt = LC.batch(case), case.opts[0]
    clean, st = launch(case, opt, rc)
    hold(case, opt, clean, st, LC.truth(case), "clean batch")
    h, st = launch(case, opt, LC.poison(case, rc, where))
    others = np.arange(case.B) != LC.J_BAD
    assert st[LC.J_BAD] & _native.ST_NONFINITE, (case.name, where, st)
    assert not st[others].any(), (case.name, where, st)
    assert np.array_equal(h[others], clean[others]), (case.name, where)
