"""Seeded inputs and comparison helpers shared by the walk-metrics tests (the host emulation of
the kernel, tests/test_metrics_emulation.py, and the device tests, tests/test_gpu_metrics.py).
Not a test module."""
import numpy as np

HG = 0.75 / 9.81
B_RANDOM = 67
# below, at and past one and two 64-lane passes; one more than the default walk's 420
N_RANDOM = (1, 2, 63, 64, 65, 129, 421)
VALUE_SLOTS = (0, 1, 6, 7, 10, 11)   # viol_max, com_dev_max, dcm_end: 1e-12 absolute
RMS_SLOTS = (8, 9)                   # zmp_rms: 1e-12 relative
EXACT_SLOTS = (2, 3, 4, 5)           # viol_argmax, viol_count: exact


def random_case(n, shared, B=B_RANDOM):
    """Random state history (not a rollout) of O(0.1) magnitude and boxes that about half of
    its ZMP samples leave.  → hist [B,n,2,3], zmax, zmin [B,n,2] or [n,2]."""
    rng = np.random.default_rng([20260119, n, int(shared)])
    hist = rng.uniform(-1.0, 1.0, (B, n, 2, 3)) * np.array([0.1, 0.5, 1.0])
    shape = (n, 2) if shared else (B, n, 2)
    centre = rng.uniform(-0.05, 0.05, shape)
    half = rng.uniform(0.02, 0.12, shape)
    return hist, centre + half, centre - half


def fma_neg(hg, a, c):
    """c − hg·a with one rounding, element by element (what a fused multiply-add gives), by exact
    integer arithmetic on the doubles' ratios (their denominators are powers of two)."""
    nh, dh = float(hg).as_integer_ratio()
    out = np.empty(a.size)
    for k, (ak, ck) in enumerate(zip(a.ravel().tolist(), c.ravel().tolist())):
        na, da = ak.as_integer_ratio()
        nc, dc = ck.as_integer_ratio()
        out[k] = (nc * dh * da - nh * na * dc) / (dc * dh * da)  # int / int: correctly rounded
    return out.reshape(a.shape)


def decisions(z, zmax, zmin):
    """(viol_argmax, viol_count) [B,2] that a ZMP array z [B,n,2] gives: the part of the metrics
    that a last-bit change of z could flip."""
    v = np.maximum(np.maximum(z - zmax, zmin - z), 0.0)
    idx = np.where(v.max(axis=1) > 0, v.argmax(axis=1), -1)
    return idx, np.count_nonzero(v > 0, axis=1)


def contraction_safe(hist, zmax, zmin, hg=HG):
    """True when z evaluated with and without a fused multiply-add gives the same indices and
    counts, so that exact comparison of those slots is fair whatever the device contracts."""
    c, a = hist[..., 0], hist[..., 2]
    i0, k0 = decisions(c - hg * a, zmax, zmin)
    i1, k1 = decisions(fma_neg(hg, a, c), zmax, zmin)
    return np.array_equal(i0, i1) and np.array_equal(k0, k1)


def assert_metrics(got, want):
    """got [B,12] against the NumPy statement: values to 1e-12 absolute, zmp_rms to 1e-12
    relative, indices and counts exactly; NaN and inf must sit where the statement has them."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    for s in EXACT_SLOTS:
        np.testing.assert_array_equal(got[:, s], want[:, s], err_msg=f"slot {s}")
    for s in VALUE_SLOTS:
        np.testing.assert_allclose(got[:, s], want[:, s], rtol=0, atol=1e-12, err_msg=f"slot {s}")
    for s in RMS_SLOTS:
        np.testing.assert_allclose(got[:, s], want[:, s], rtol=1e-12, atol=0, err_msg=f"slot {s}")
