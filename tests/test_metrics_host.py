"""Walk metrics without a GPU: the NumPy statement of the twelve slots on hand-written walks, the
named view, the argument checks of zmpc_walk_metrics (which run before any device call) and the
closed-form critical force."""
import ctypes
import os

import numpy as np
import pytest

from mpc_bipedal import _native, analysis
from mpc_bipedal.analysis import (WalkMetrics, critical_force_affine, walk_metrics_reference)

NAN, INF = float("nan"), float("inf")
HG = 0.25  # sqrt(h/g) = 0.5: every slot of the walk below is an exact binary fraction


def _walk():
    """One walk of three samples.  x: z = c − c̈/4 = (−0.25, 0.75, 0.75) against boxes
    [0, 0.5], [0, 0.5], [−0.5, 1] (centre 0.25 each); y: z = c = (0.5, −0.5, 0.5) in [−1, 1]."""
    hist = np.array([[[[0.0, 0.0, 1.0], [0.5, 0.0, 0.0]],
                      [[0.5, 1.0, -1.0], [-0.5, 0.0, 0.0]],
                      [[1.0, 2.0, 1.0], [0.5, -1.0, 0.0]]]])
    zmax = np.array([[[0.5, 1.0], [0.5, 1.0], [1.0, 1.0]]])
    zmin = np.array([[[0.0, -1.0], [0.0, -1.0], [-0.5, -1.0]]])
    return hist, zmax, zmin


def test_reference_hand_written_walk():
    m = walk_metrics_reference(*_walk(), HG)
    assert m.shape == (1, 12)
    #       viol_max     argmax       count      com_dev_max  zmp_rms     dcm_end
    want = [0.25, 0.0,   0.0, -1.0,   2.0, 0.0,  0.75, 0.5,   0.5, 0.5,   1.75, 0.0]
    assert m[0].tolist() == want  # the tie of samples 0 and 1 goes to sample 0; y never leaves
    # one shared CoP [n, 2] is the same statement
    hist, zmax, zmin = _walk()
    assert np.array_equal(walk_metrics_reference(hist, zmax[0], zmin[0], HG), m)


def test_reference_ragged_walk_ignores_dead_rows():
    hist, zmax, zmin = _walk()
    hist[0, 2], zmax[0, 2], zmin[0, 2] = NAN, 1e300, NAN
    m = walk_metrics_reference(hist, zmax, zmin, HG, lengths=[2])
    want = [0.25, 0.0,   0.0, -1.0,   2.0, 0.0,  0.25, 0.5,   0.5, 0.5,   0.75, -0.5]
    assert m[0].tolist() == want


@pytest.mark.parametrize("bad", (NAN, INF, -INF))
@pytest.mark.parametrize("component", (0, 1, 2))
def test_reference_non_finite_rule(bad, component):
    """A non-finite value in any of an axis' three state components: +inf, the sample's index,
    NaN elsewhere on that axis — the other axis and the other walk keep their values."""
    hist, zmax, zmin = (np.concatenate([a, a]) for a in _walk())
    clean = walk_metrics_reference(hist, zmax, zmin, HG)
    hist[1, 1, 0, component] = bad
    hist[1, 2, 0, 0] = NAN  # a later one does not move the index
    m = walk_metrics_reference(hist, zmax, zmin, HG)
    assert np.array_equal(m[0], clean[0]) and np.array_equal(m[1, 1::2], clean[1, 1::2])
    assert m[1, 0] == INF and m[1, 2] == 1.0 and np.isnan(m[1, 4::2]).all()
    assert not (m[1, 0] <= 1e-9)  # a threshold on viol_max fails safe


def test_walk_metrics_view_names_columns_without_copies():
    data = np.arange(36.0).reshape(3, 12)
    w = WalkMetrics(data)
    assert len(w) == 3 and analysis.NMETRICS == _native.NMETRICS == 12
    for k, name in enumerate(analysis.SLOT_NAMES):
        col = getattr(w, name)
        assert col.shape == (3, 2) and np.shares_memory(col, data)
        assert np.array_equal(col, data[:, 2 * k:2 * k + 2])
    with pytest.raises(AttributeError):
        w.no_such_metric
    with pytest.raises(ValueError, match=r"\[B, 12\]"):
        WalkMetrics(np.zeros((3, 11)))


def test_c_abi_argument_checks_without_gpu():
    """zmpc_walk_metrics validates before any device call: every bad argument is ZMPC_EINVAL with
    a message, an empty batch is a no-op.  The plan is never dereferenced on these paths, so a
    zeroed block stands in for one."""
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libzmpc.so not built (run __graft_entry__.build())")
    lib = _native.load()
    fake_plan = ctypes.create_string_buffer(4096)
    plan, ptr = ctypes.addressof(fake_plan), 4096  # ptr: a non-NULL device address, never read

    def call(plan=plan, B=2, n=10, hist=ptr, zmax=ptr, zmin=ptr, stride=20, metrics=ptr):
        rc = lib.zmpc_walk_metrics(plan, B, n, hist, zmax, zmin, stride, None, metrics, None)
        return rc, lib.zmpc_last_error()

    rc, msg = call(plan=None)
    assert rc == _native.ZMPC_EINVAL and b"NULL plan" in msg
    for bad in (dict(hist=None), dict(zmax=None), dict(zmin=None), dict(metrics=None)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"NULL" in msg, bad
    for bad in (dict(B=-1), dict(n=0), dict(n=-3)):
        rc, msg = call(**bad)
        assert rc == _native.ZMPC_EINVAL and b"B >= 0 and n >= 1" in msg, bad
    for stride in (19, 1, -20):
        rc, msg = call(stride=stride)
        assert rc == _native.ZMPC_EINVAL and b"bounds_stride" in msg, stride
    assert call(B=0) == (0, b"")
    assert call(B=0, stride=0) == (0, b"")


def test_critical_force_affine_on_synthetic_response():
    """z(F) = z0 + F·r against [−1, 1]: the first sample to reach a bound decides."""
    z0 = np.array([0.0, 0.5, -0.5, 0.25])
    r = np.array([0.0, 0.125, -0.0625, -0.5])
    one = np.ones(4)
    # sample 1 reaches +1 at F = 4, sample 2 reaches −1 at F = 8, sample 3 at F = 2.5
    assert critical_force_affine(z0, r, one, -one) == 2.5
    assert critical_force_affine(z0[:3], r[:3], one[:3], -one[:3]) == 4.0
    assert critical_force_affine(z0, -r, one, -one) == 1.5  # the mirrored push: sample 3 at +1
    # the allowance widens both bounds
    assert critical_force_affine(z0, r, one, -one, max_violation=0.25) == 3.0
    # batched; a walk outside its box with no push has no critical force; r = 0 never leaves
    f = critical_force_affine(np.stack([z0, z0 + 1.0, 0 * z0]), np.stack([r, r, 0 * r]),
                              np.ones((3, 4)), -np.ones((3, 4)))
    assert f[0] == 2.5 and np.isnan(f[1]) and f[2] == INF
    # pass at F* (to rounding), fail just past it
    z = lambda F: z0 + F * r
    assert np.abs(z(2.5)).max() <= 1.0 and np.abs(z(2.5 * 1.01)).max() > 1.0
