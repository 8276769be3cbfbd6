"""The split rollout kernel's load phase and kick placement (csrc/rollout.hip split_walk): every
global load of a walk is issued before the first wait (bounds stored to LDS without a branch,
table rows in registers), the next-dispatch-round prefetch is a kernel instance of its own with
a clamped walk index, and the kick is placed by wave-uniform scalar values (the owning lane, the
step's place in its chunk).

Tolerances are the project's: 1e-12 against the cross-check kernel (ZMPC_OPT_ROLLOUT_KERNEL = 1)
and 1e-8 against the gain-form oracle.  N = 150 (dt = 0.01) unless stated; every case runs the
same dt so that short horizons stay small (N = 1 grows a walk of 130 samples by ≈ e^(ω·1.3)).
"""
import numpy as np
import pytest
import torch

from conftest import golden
from oracle import zmp_oracle as O

pytestmark = pytest.mark.gpu

from mpc_bipedal.solver import Plan  # noqa: E402
from mpc_bipedal import _native  # noqa: E402

H, G, Q, R, M = 0.75, 9.81, 1.0, 1e-6, 40.0
DT = 0.01


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    _native.load()


def plan(N):
    return Plan(torch.cuda.current_device(), N, DT, H, G, Q, R, False)


def chunk_width(n):
    """Steps per lane of the single-pass kernels (dispatch.h: ⌈(n − 1)/64⌉, at least 1)."""
    return max((n - 1 + 63) // 64, 1)


def offset_walks(rng, B, n):
    """The default CoP's first n samples under a rigid offset per walk: every walk distinct."""
    cop = golden("walk_n150.npz")
    off = rng.uniform(-0.02, 0.02, (B, 1, 2))
    x0 = np.zeros((B, 2, 3))
    x0[:, :, 0] = rng.uniform(-0.01, 0.01, (B, 2))
    return cop["zmax"][None, :n] + off, cop["zmin"][None, :n] + off, x0


def piecewise_walks(rng, B, n, changes):
    """Piecewise-constant bounds, `changes` z_ref changes per axis at distinct samples that always
    include the first and the last possible one (m = 0 and m = n − 2)."""
    ctr = np.empty((B, n, 2))
    for b in range(B):
        for ax in range(2):
            inner = rng.choice(np.arange(1, n - 2), size=max(changes - 2, 0), replace=False)
            pos = np.unique(np.concatenate([inner, [0, n - 2]]))[-changes:] if changes > 1 \
                else np.array([(0, n - 2)[(b + ax) % 2]])
            steps = np.zeros(n)
            steps[pos + 1] = rng.uniform(0.01, 0.05, pos.size) * rng.choice([-1.0, 1.0], pos.size)
            ctr[b, :, ax] = 0.1 + np.cumsum(steps)
    return ctr + 0.05, ctr - 0.05


@pytest.mark.parametrize("n", (65, 130))
@pytest.mark.parametrize("rounds", ("R+1", "2R", "2R+1"))
def test_prefetch_boundary(rounds, n):
    """Batches at the edges of the next-round prefetch rule (R = 8 workgroups per CU: on up to
    B = 2R, off beyond): the first and the last workgroup that prefetches a real walk, the
    workgroups whose clamped index touches walk B − 1 again, and the instance without prefetch.
    Every walk against the cross-check kernel; the walks at both ends of each round against the
    oracle."""
    Rr = 8 * torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    B = {"R+1": Rr + 1, "2R": 2 * Rr, "2R+1": 2 * Rr + 1}[rounds]
    rng = np.random.default_rng(1000 * n + B % 7)
    zmax, zmin, x0 = offset_walks(rng, B, n)
    assert np.unique(zmax[:, 0, 0]).size == B
    kick = rng.uniform(0.0, 0.2, B)
    outs = []
    for kern in (0, 1):
        h, st = plan(150).set_option("rollout_kernel", kern).rollout(zmax, zmin, x0, kick=kick,
                                                                      kick_step=n // 2)
        assert int(st.abs().max()) == 0
        outs.append(h.cpu().numpy())
    err_x = np.abs(outs[0] - outs[1]).max()
    idx = np.unique([0, Rr - 1, Rr, B - Rr - 1, B - 1])
    ref = O.rollout_gain(zmax[idx], zmin[idx], x0[idx], 150, DT, H, G, Q, R, kick[idx], n // 2)
    err_o = np.abs(outs[0][idx] - ref).max()
    print(f"B={B} n={n}: cross-check {err_x:.3e}, oracle {err_o:.3e}")
    assert err_x <= 1e-12
    assert err_o <= 1e-8


@pytest.mark.parametrize("N", (1, 110, 238, 239, 300))
def test_table_staging(N):
    """The suffix-sum table's rows reach LDS from registers (rows tid and tid + 128) and, past
    256 rows, from a loop: ksum_rows(N) = N + 18 is 19, 128 (one full register row), 256 (both),
    257 (the loop's first row) and 318.  n = 130 (chunk width 3), 70 walks: piecewise-constant
    bounds with 1, 2 and 3 changes per axis (m = 0 and m = n − 2 among them: the sparse form)
    and random-walk bounds (the dense fallback) in one launch.  Sparse-first against dense-only
    as test_sparse_correlation_equals_dense scales it, and against the oracle."""
    n = 130
    rng = np.random.default_rng(N)
    hi, lo = [], []
    for c in (1, 2, 3):
        a, b = piecewise_walks(rng, 16, n, c)
        hi.append(a)
        lo.append(b)
    ctr = np.cumsum(rng.normal(0, 0.01, (22, n, 2)), 1)
    zmax, zmin = np.concatenate(hi + [ctr + 0.05]), np.concatenate(lo + [ctr - 0.05])
    B = zmax.shape[0]
    assert B == 70
    x0 = np.zeros((B, 2, 3))
    x0[:, :, 0] = rng.uniform(-0.01, 0.01, (B, 2))
    kick = rng.uniform(0.0, 0.2, B)
    outs = []
    for corr in (0, 1):  # sparse where it applies (default) / dense only
        h, st = plan(N).set_option("correlation", corr).rollout(zmax, zmin, x0, kick=kick,
                                                                kick_step=n // 3)
        assert int(st.abs().max()) == 0
        outs.append(h.cpu().numpy())
    scale = np.abs(outs[1]).max(axis=1, keepdims=True) + 1.0
    err_d = (np.abs(outs[0] - outs[1]) / scale).max()
    ref = O.rollout_gain(zmax, zmin, x0, N, DT, H, G, Q, R, kick, n // 3)
    err_o = np.abs(outs[0] - ref).max()
    print(f"N={N}: sparse vs dense {err_d:.3e} (scaled), oracle {err_o:.3e}, "
          f"largest state {np.abs(ref).max():.3e}")
    assert err_d <= 1e-12
    assert err_o <= 1e-8


@pytest.mark.parametrize("n", (2, 3, 65, 130, 420))
def test_kick_placement(n):
    """The kick at the first and last step of a lane's chunk, the first step of the next lane,
    the walk's last step, and out of range on both sides (−1, n − 1, n + 5), launch-wide and as
    a per-walk array cycling through them.  Every walk against the oracle; the x axis never
    sees the kick (bit-identical to the launch without one), and a walk whose step is out of
    range equals the no-kick history bit for bit."""
    cw, B = chunk_width(n), 16
    steps = [-1, 0, cw - 1, cw, n - 2, n - 1, n + 5]
    rng = np.random.default_rng(n)
    zmax, zmin, x0 = offset_walks(rng, B, n)
    kick = rng.uniform(0.05, 0.2, B)
    p = plan(150)
    h0, st = p.rollout(zmax, zmin, x0)
    assert int(st.abs().max()) == 0
    h0 = h0.cpu().numpy()
    ref0 = O.rollout_gain(zmax, zmin, x0, 150, DT, H, G, Q, R)
    assert np.abs(h0 - ref0).max() <= 1e-8
    refs = {s: O.rollout_gain(zmax, zmin, x0, 150, DT, H, G, Q, R, kick, s) for s in set(steps)}
    worst = 0.0
    for s in steps:
        h, st = p.rollout(zmax, zmin, x0, kick=kick, kick_step=s)
        assert int(st.abs().max()) == 0
        h = h.cpu().numpy()
        worst = max(worst, np.abs(h - refs[s]).max())
        assert np.abs(h - refs[s]).max() <= 1e-8, s
        assert np.array_equal(h[:, :, 0], h0[:, :, 0]), s
        if 0 <= s < n - 1:
            assert not np.array_equal(h[:, :, 1], h0[:, :, 1]), s
        else:
            assert np.array_equal(h, h0), s
    per_walk = np.array([steps[b % len(steps)] for b in range(B)], np.int64)
    h, st = p.rollout(zmax, zmin, x0, kick=kick, kick_step=per_walk)
    assert int(st.abs().max()) == 0
    h = h.cpu().numpy()
    assert np.array_equal(h[:, :, 0], h0[:, :, 0])
    for b in range(B):
        s = int(per_walk[b])
        worst = max(worst, np.abs(h[b] - refs[s][b]).max())
        assert np.abs(h[b] - refs[s][b]).max() <= 1e-8, (b, s)
        if not 0 <= s < n - 1:
            assert np.array_equal(h[b], h0[b]), (b, s)
    print(f"n={n} cw={cw}: oracle {worst:.3e}")
