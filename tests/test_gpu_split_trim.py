"""The split rollout kernel (csrc/rollout.hip split_walk) at the shapes where its address
arithmetic can go wrong: walk ends, kick placement, the sparse correlation's clamped table
offset, the next-round prefetch rule and non-finite inputs.

Every case holds the default kernel (dispatch.h choose_unc: Split) against two references:
the one-wave cross-check kernel (plan option rollout_kernel = 1) at 1e-12 of the batch's scale
max(1, max |history|) (the bar of test_rollout_kernel_variants_agree: absolute 1e-12 on histories
below 1), and the oracle's rollout_gain at the 1e-8 of test_sparse_correlation_equals_dense.
Batches are a handful of walks; the largest (B = 12000 at n = 9) is 5 MB of history.
"""
import numpy as np
import pytest
import torch

from conftest import golden
from oracle import zmp_oracle as O

pytestmark = pytest.mark.gpu

from mpc_bipedal.solver import Plan  # noqa: E402
from mpc_bipedal import _native  # noqa: E402

H, G, Q, R = 0.75, 9.81, 1.0, 1e-6
SPARSE_MAX = 40  # rollout.hip kSparseMax

_PLANS = {}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    _native.load()
    yield
    _PLANS.clear()


def plans(N):
    """(default plan, cross-check plan with the one-wave kernel, dt) for horizon N."""
    if N not in _PLANS:
        dt = float(golden("walk_n150.npz")["dt"]) if N == 150 else 1.5 / N
        dev = torch.cuda.current_device()
        _PLANS[N] = (Plan(dev, N, dt, H, G, Q, R, False),
                     Plan(dev, N, dt, H, G, Q, R, False).set_option("rollout_kernel", 1), dt)
    return _PLANS[N]


def oracle(zmax, zmin, x0, N, dt, kick, ks):
    """rollout_gain, with a per-walk array of kick steps served one distinct step at a time."""
    if np.ndim(ks) == 0:
        return O.rollout_gain(zmax, zmin, x0, N, dt, H, G, Q, R, kick, int(ks))
    ks = np.asarray(ks)
    ref = np.empty(zmax.shape[:2] + (2, 3))
    for v in np.unique(ks):
        w = ks == v
        ref[w] = O.rollout_gain(zmax[w], zmin[w], x0[w], N, dt, H, G, Q, R, kick[w], int(v))
    return ref


def check(N, zmax, zmin, x0, kick, ks, what=""):
    """Split kernel vs the one-wave kernel (1e-12 relative) and vs the oracle (1e-8)."""
    p, pg, dt = plans(N)
    h, st = p.rollout(zmax, zmin, x0, kick=kick, kick_step=ks)
    hg, sg = pg.rollout(zmax, zmin, x0, kick=kick, kick_step=ks)
    h, hg = h.cpu().numpy(), hg.cpu().numpy()
    assert int(st.abs().max()) == 0 and int(sg.abs().max()) == 0, what
    ref = oracle(zmax, zmin, x0, N, dt, kick, ks)
    scale = max(1.0, float(np.abs(hg).max()))
    e_kern, e_ref = float(np.abs(h - hg).max()) / scale, float(np.abs(h - ref).max())
    print(f"{what}: N={N} B={zmax.shape[0]} n={zmax.shape[1]} vs one-wave {e_kern:.2e} "
          f"vs oracle {e_ref:.2e}")
    assert e_kern <= 1e-12, what
    assert e_ref <= 1e-8, what
    return h


def piecewise(rng, B, n, changes_x, changes_y=(3,)):
    """Piecewise-constant bounds: walk b's z_ref changes on axis 0 at the samples m of
    changes_x[b % len] (z_ref[m + 1] != z_ref[m]) when that is a list, or at that many random
    samples when it is an int; likewise axis 1."""
    z = np.empty((B, n, 2))
    for b in range(B):
        for ax, spec in ((0, changes_x), (1, changes_y)):
            c = spec[b % len(spec)]
            if isinstance(c, (int, np.integer)):
                pos = rng.choice(np.arange(n - 1), size=min(int(c), n - 1), replace=False)
            else:
                pos = np.asarray([m for m in c if 0 <= m <= n - 2], int)
            steps = np.zeros(n)
            steps[pos + 1] = rng.choice([-1.0, 1.0], pos.size) * rng.uniform(0.01, 0.05, pos.size)
            z[b, :, ax] = 0.1 * (ax + 1) + np.cumsum(steps)
    return z + 0.05, z - 0.05


def batch(rng, B, n, changes_x=(4,), changes_y=(3,)):
    zmax, zmin = piecewise(rng, B, n, changes_x, changes_y)
    x0 = np.zeros((B, 2, 3))
    x0[:, :, 0] = rng.uniform(-0.01, 0.01, (B, 2))
    x0[:, :, 1] = rng.uniform(-0.05, 0.05, (B, 2))
    return zmax, zmin, x0, rng.uniform(0.05, 0.2, B)


# ------------------------------------------------------------------------------- walk ends


@pytest.mark.parametrize("CW", range(1, 9))
def test_walk_ends(CW):
    """n − 1 = 1, CW, CW + 1 (lanes past the end), 64·CW − 1 (a last lane with a partial chunk)
    and 64·CW (a full grid, chunk width CW) at N = 16."""
    rng = np.random.default_rng(100 + CW)
    for ns in (1, CW, CW + 1, 64 * CW - 1, 64 * CW):
        zmax, zmin, x0, kick = batch(rng, 5, ns + 1, (0, 1, 4, (0, ns - 1), 9))
        check(16, zmax, zmin, x0, kick, ns // 2, f"walk end CW={CW} n-1={ns}")


@pytest.mark.parametrize("n", (420, 449))
def test_walk_ends_n150(n):
    """N = 150: the default walk length (chunk width 7, four lanes past the end) and the full
    grid n − 1 = 448 = 64·7."""
    rng = np.random.default_rng(n)
    zmax, zmin, x0, kick = batch(rng, 6, n, (0, 1, 16, (0, n - 2), 30, 40), (3, 16))
    check(150, zmax, zmin, x0, kick, n // 2, f"walk end n={n}")


# --------------------------------------------------------------------------- kick placement

# (N, n, CW): an odd and an even chunk width with a partial last lane, and the default shape
KICK_SHAPES = ((16, 191, 3), (16, 255, 4), (150, 420, 7))


def _kick_steps(n, CW):
    ns = n - 1
    last_lane = (ns - 1) // CW  # the last live lane
    return [0, CW - 1,                        # lane 0: first and last place of its chunk
            10 * CW, 10 * CW + CW - 1,        # a middle lane: first and last place
            last_lane * CW, ns - 1,           # the last live lane; n − 2 is the last step
            -1, ns, ns + 5]                   # out of range: no kick


@pytest.mark.parametrize("N,n,CW", KICK_SHAPES)
def test_kick_placement(N, n, CW):
    """One launch-wide kick step per launch: step 0, n − 2, the first and last place of a chunk,
    lane 0 and the last live lane, and steps out of range."""
    rng = np.random.default_rng(7 * n)
    zmax, zmin, x0, kick = batch(rng, 3, n)
    hs = {}
    for ks in _kick_steps(n, CW):
        hs[ks] = check(N, zmax, zmin, x0, kick, ks, f"kick step {ks}")
    assert np.array_equal(hs[-1], hs[n - 1]) and np.array_equal(hs[-1], hs[n + 4])  # no kick
    assert not np.array_equal(hs[-1], hs[n - 2])


@pytest.mark.parametrize("N,n,CW", KICK_SHAPES)
def test_kick_placement_per_walk(N, n, CW):
    """The same placements mixed over the walks of one launch (zmpc_rollout_kicks)."""
    rng = np.random.default_rng(11 * n)
    steps = np.array(_kick_steps(n, CW) * 2, np.int64)
    zmax, zmin, x0, kick = batch(rng, steps.size, n)
    check(N, zmax, zmin, x0, kick, steps, "per-walk kick steps")


# ----------------------------------------------------------- change positions (address clamp)


@pytest.mark.parametrize("N,n,CW", ((16, 191, 3), (16, 255, 4), (150, 420, 7), (150, 449, 7)))
def test_change_positions(N, n, CW):
    """z_ref changes at the ends of the sparse correlation's table reach.  Lane l's first output
    is t = l·CW and a change at sample m reaches outputs t with 1 ≤ m − t ≤ N − 1: changes at
    m = 0 and m = n − 2, exactly N − 1 and exactly N samples ahead of a lane's first output, one
    whose only new value is the last sample (so every row of the window padding differs from the
    walk before it), and walks with 0, 1, SPARSE_MAX and SPARSE_MAX + 1 changes on the x axis
    (the last takes the dense form) beside a sparse y axis."""
    rng = np.random.default_rng(13 * n + N)
    t0, t1 = 5 * CW, ((n - 2 - N) // CW) * CW  # first outputs of lane 5 and of a late lane
    xs = ([0], [n - 2], [0, n - 2], [t0 + N - 1], [t0 + N], [t1 + N - 1], [t1 + N],
          [t0 + N - 1, t0 + N], [t0, t0 + 1, t0 + CW - 1, t0 + CW], [n - 2 - N, n - 1 - N],
          0, 1, SPARSE_MAX, SPARSE_MAX + 1)
    zmax, zmin, x0, kick = batch(rng, len(xs), n, xs, (3, [0, n - 2], 0))
    check(N, zmax, zmin, x0, kick, n // 3, "change positions")


# ------------------------------------------------------------------------------ prefetch rule


@pytest.mark.parametrize("B", (1, 3, 5000, 12000))
def test_prefetch_rule(B):
    """n = 9 at B = 1 and 3 (the prefetch instance, every walk's next-round index past the batch),
    B = 5000 (two dispatch rounds at most) and B = 12000 (more than two rounds of any occupancy
    the kernel can reach: the instance without prefetch)."""
    rng = np.random.default_rng(B)
    zmax, zmin, x0, kick = batch(rng, min(B, 64), 9, (0, 1, 2, [0, 7]), (1, [7]))
    idx = np.arange(B) % zmax.shape[0]
    check(16, zmax[idx], zmin[idx], x0[idx], kick[idx], 4, f"prefetch rule B={B}")


@pytest.mark.parametrize("N,n,B", ((16, 9, 5000), (150, 420, 2100)))
def test_last_walk_differs(N, n, B):
    """Every walk equal but the last one, which a second-round workgroup solves: a workgroup that
    skips its next-round loads must still produce its own walk."""
    rng = np.random.default_rng(n + B)
    zmax, zmin, x0, kick = batch(rng, 2, n, (2, 5), (3, 1))
    idx = np.zeros(B, int)
    idx[-1] = 1
    h = check(N, zmax[idx], zmin[idx], x0[idx], kick[idx], n // 2, "last walk differs")
    assert np.array_equal(h[:-1], np.broadcast_to(h[0], h[:-1].shape))
    assert not np.array_equal(h[-1], h[0])


# ---------------------------------------------------------------------------- non-finite inputs


@pytest.mark.parametrize("N,n", ((16, 191), (150, 420)))
@pytest.mark.parametrize("where", ("x0", "bounds"))
def test_nonfinite_walk_is_flagged_alone(N, n, where):
    """A NaN in one walk's x0 or bounds: that walk reports ZMPC_ST_NONFINITE, every other walk
    of the batch has status 0 and the history of the clean batch, bit for bit."""
    rng = np.random.default_rng(n)
    B, bad = 9, 4
    zmax, zmin, x0, kick = batch(rng, B, n)
    good = check(N, zmax, zmin, x0, kick, n // 2, "clean batch")
    if where == "x0":
        x0 = x0.copy()
        x0[bad, 1, 2] = np.nan
    else:
        zmax = zmax.copy()
        zmax[bad, n // 3, 0] = np.nan
    p, pg, _ = plans(N)
    others = np.arange(B) != bad
    for pl in (p, pg):
        h, st = pl.rollout(zmax, zmin, x0, kick=kick, kick_step=n // 2)
        st = st.cpu().numpy()
        assert st[bad] & _native.ST_NONFINITE
        assert not st[others].any()
        if pl is p:
            assert np.array_equal(h.cpu().numpy()[others], good[others])
