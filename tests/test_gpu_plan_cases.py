"""Every table of the plan build (csrc/plan.hip) against extended-precision truth, at the horizons
next to the code's edges and at seven weight points (tests/plan_cases.py; the truth is stored,
tests/golden/plan_truth.npz, and proven on the CPU by tests/test_plan_cases_host.py).

Per case one strict plan (and at N = 17, 65, 129 one non-strict), every export id read back:
  bit-exact    p, Px against the oracle; the fast-FIR rows and every structural zero of the suffix-
               sum layout against the device's own exported k (copies and one addition); the
               strictly upper triangle of L
  measured bar M, k, kx, rows of L, X, G and Hz, v, the suffix sums, the scan tables (each 3x3
               propagator and 3-vector relative to its own largest entry), the FFT twiddles and
               gain spectra: each relative to the quantity's largest magnitude, the bar 16 x the
               float64 reference's own distance from truth (plan_cases.e_ref, the maximum over the
               cases sharing the weight point), floor 64 ulp
  identities   on the full float64 matrices: |L·Lᵀ − M| <= (2N + 4)·u·max|M| (Cholesky's backward
               error γ_{N+1}·|L||Lᵀ| plus the product's own γ_N·|L||Lᵀ|, and (|L||Lᵀ|)_ij <=
               sqrt(M_ii·M_jj); u = 2^-53); |L·X − Puᵀ| <= (2N + 4)·u·max(|L||X|) (the substitution's
               backward error γ_N·|L||X| plus the product's); |G·Hz − I| and |XᵀX/Q − G| / max|G|
               <= 16 x the same residual of the float64 reference (G = np.linalg.inv(Hz),
               X = solve(L, Puᵀ)), floors 64 ulp of max(|G||Hz|) and 64 ulp: both join matrices
               that come from differently conditioned factorisations (M's and Hz's), on the
               device as in the reference
(G = Pu·M⁻¹·Puᵀ/Q = XᵀX/Q with X = L⁻¹·Puᵀ; X·Xᵀ is another matrix.  The device keeps that Gram
product as G only where M's pivots spread less than Hz's, and G = Hz⁻¹ from Hz's own factor
elsewhere: plan.hip regain_G.)

The unconstrained rollouts at the weight points: N = 17, 65, 129 x seven points, six walks (random-
walk and piecewise-constant bounds, x0 != 0, a kick and a kick step per walk) of n = 40, 130 (chunk
widths 1, 3) and 420 (7) where ρ(Ā) <= 1, rollout kernels 0 and 1, against oracle.rollout_gain with
the true gain; bar 16 x the distance between that and rollout_gain with numpy's gain, floor 1e-12,
relative to max(1, |ref|).  No (point, n) pair reaches ρ(Ā)^n > 1e6, so none is left out.

`pytest -s` prints every measured figure and, at the end, the worst per weight point.
"""
import ctypes

import numpy as np
import pytest
import torch

import plan_cases as PC

pytestmark = pytest.mark.gpu

from mpc_bipedal.solver import Plan  # noqa: E402
from mpc_bipedal import _native  # noqa: E402

U = 2.0 ** -53
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    _native.load()
    yield
    print("\ndevice vs truth, worst per weight point (bar):")
    for point, w in _WORST.items():
        print(point, "  ".join(f"{key} {v:.1e} ({b:.1e})" for key, (v, b) in w.items()))


def make_plan(case, strict):
    _, N, (Q, R, h, g) = case
    return Plan(torch.cuda.current_device(), N, PC.case_dt(N), h, g, Q, R, strict)


def note(point, key, value, bar):
    w = _WORST.setdefault(point, {})
    w[key] = (max(value, w.get(key, (0.0, bar))[0]), bar)


def check_plan(case, strict):
    name, N, point = case
    Q = point[0]
    inp, s, bars = PC.inputs(case), PC.stored(name), PC.bars(point)
    p = make_plan(case, strict)
    try:
        ex = {key: p.export(getattr(_native, "EXPORT_" + key)) for key in
              ("P", "PX", "M", "K", "KX", "L", "KFFA", "KSUM", "SCAN", "FFT_TW", "FFT_G")}
        if strict:
            ex.update({key: p.export(getattr(_native, "EXPORT_" + key))
                       for key in ("G", "HZ", "X", "V")})
    finally:
        p.destroy()
    label = f"{name} strict={int(strict)}"
    # bit-exact
    assert np.array_equal(ex["P"], inp["p"]) and np.array_equal(ex["PX"], inp["Px"]), label
    assert ex["K"].shape == (N,) and ex["KFFA"].shape == ((N + 2) // 2 + 8, 4)
    assert np.array_equal(ex["KFFA"], PC.kffa_from(ex["K"])), label
    assert ex["KSUM"].shape == (N + 18,) and np.all(ex["KSUM"][s["ksum_zero"]] == 0.0), label
    assert np.array_equal(np.triu(ex["L"], 1), np.zeros((N, N))), label
    # against truth
    q = dict(M=ex["M"], k=ex["K"], kx=ex["KX"], L=ex["L"], ksum=ex["KSUM"], scan=ex["SCAN"],
             fft_tw=ex["FFT_TW"], fft_g=PC.device_fft_g(ex["FFT_G"]))
    if strict:
        q.update(X=ex["X"], G=ex["G"], Hz=ex["HZ"], v=ex["V"])
    d = PC.distances(q, name)
    print(f"\n{label}: " + "  ".join(f"{key} {v:.1e}" for key, v in d.items()))
    for key, v in d.items():
        note(point, key, v, bars[key])
    bad = {key: (v, bars[key]) for key, v in d.items() if not v <= bars[key]}
    # identities on the full matrices
    L, M = ex["L"], ex["M"]
    res = float(np.abs(L @ L.T - M).max())
    bar = (2 * N + 4) * U * float(np.abs(M).max())
    note(point, "LLt-M", res, bar)
    if not res <= bar:
        bad["LLt-M"] = (res, bar)
    if strict:
        X, G, Hz = ex["X"], ex["G"], ex["HZ"]
        res = float(np.abs(L @ X - inp["Pu"].T).max())
        bar = (2 * N + 4) * U * float((np.abs(L) @ np.abs(X)).max())
        note(point, "LX-PuT", res, bar)
        if not res <= bar:
            bad["LX-PuT"] = (res, bar)
        ghz_bar, gram_bar = PC.identity_bars(point)
        res = PC.gram_residual(X, G, Q)
        note(point, "XtX/Q-G", res, gram_bar)
        if not res <= gram_bar:
            bad["XtX/Q-G"] = (res, gram_bar)
        res, scale = PC.identity_residual(G, Hz)
        bar = max(ghz_bar, PC.BAR_FLOOR * scale)
        note(point, "GHz-I", res, bar)
        if not res <= bar:
            bad["GHz-I"] = (res, bar)
    assert not bad, (label, bad)


@pytest.mark.parametrize("case", PC.all_cases(), ids=[c[0] for c in PC.all_cases()])
def test_plan_tables_vs_truth(case):
    check_plan(case, strict=True)
    if case[1] in PC.WEIGHT_N:
        check_plan(case, strict=False)


ROLLOUTS = [(PC.case_name(N, w), N, PC.POINTS[w]) for N in PC.WEIGHT_N
            for w in range(len(PC.POINTS))]


@pytest.mark.parametrize("case", ROLLOUTS, ids=[c[0] for c in ROLLOUTS])
def test_unconstrained_rollout_at_weight_point(case):
    s = PC.stored(case[0])
    run, left_out = PC.rollout_lengths(s["rho"])
    assert not left_out and len(run) == (3 if s["rho"] <= 1.0 else 2)
    p = make_plan(case, strict=False)
    try:
        for n in run:
            rc = PC.rollout_case(case[0], n)
            ref = PC.rollout_reference(case, rc, gain=(s["k"], s["kx"]))
            bar = max(1e-12, 16.0 * PC.rel_hist(PC.rollout_reference(case, rc), ref))
            for kernel in (0, 1):
                p.set_option("rollout_kernel", kernel)
                h, st = p.rollout(rc["zmax"], rc["zmin"], rc["x0"], kick=rc["kick"],
                                  kick_step=rc["kick_step"])
                assert int(st.abs().max()) == 0, (case[0], n, kernel)
                err = PC.rel_hist(h.cpu().numpy(), ref)
                print(f"\n{case[0]} n={n} kernel={kernel}: {err:.1e} (bar {bar:.1e})")
                assert err <= bar, (case[0], n, kernel, err, bar)
    finally:
        p.destroy()


def test_export_refusals():
    lib = _native.load()
    N = 17
    case = (PC.case_name(N, 0), N, PC.POINTS[0])
    sizes = {what: count(N) for what, (_, count, _) in _native.EXPORTS.items() if what >= 8}
    assert sorted(sizes) == list(range(8, 15)) and sizes[11] == N * N and sizes[12] == N
    assert sizes[13] == 2 * _native.FFT_PT
    assert sizes[8] == 4 * ((N + 2) // 2 + 8) and sizes[9] == N + 18
    assert sizes[10] == PC.SCAN_DOUBLES and sizes[14] == 2 * PC.FFT_G_COMPLEX
    buf = np.full(max(sizes.values()) + 1, np.nan)
    ptr = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    for strict in (False, True):
        p = make_plan(case, strict)
        try:
            for what, n in sizes.items():
                held = strict or what not in (11, 12)
                rc = lib.zmpc_plan_export(p.handle, what, ptr, len(buf))
                assert rc == (_native.ZMPC_OK if held else _native.ZMPC_ESTATE), (strict, what)
                if held:
                    # exactly n doubles written, and one fewer is refused
                    assert np.isfinite(buf[:n]).all() and np.isnan(buf[n:]).all(), (strict, what)
                    buf[:] = np.nan
                    assert lib.zmpc_plan_export(p.handle, what, ptr, n - 1) == _native.ZMPC_EINVAL
                    assert np.isnan(buf).all()
                    assert lib.zmpc_plan_export(p.handle, what, ptr, n) == _native.ZMPC_OK
                    buf[:] = np.nan
                else:
                    assert np.isnan(buf).all()
                    assert b"not held" in lib.zmpc_last_error()
            assert lib.zmpc_plan_export(p.handle, 15, ptr, len(buf)) == _native.ZMPC_EINVAL
            assert b"unknown export id" in lib.zmpc_last_error()
            assert lib.zmpc_plan_export(p.handle, -1, ptr, len(buf)) == _native.ZMPC_EINVAL
            assert np.isnan(buf).all()
            with pytest.raises(ValueError):
                p.export(15)
            if not strict:
                with pytest.raises(_native.NativeError):
                    p.export(_native.EXPORT_X)
                with pytest.raises(_native.NativeError):
                    p.export(_native.EXPORT_V)
        finally:
            p.destroy()
