"""The plan-build cases on the CPU (tests/plan_cases.py): the stored truth
tests/golden/plan_truth.npz re-derived live with mpmath at the short horizons, the truth's own
residuals, the integer-arithmetic truths (M, the scan tables, the twiddle symmetries) against
mpmath, and the float64 reference's distance from truth (e_ref), from which the device test's bars
follow.  `pytest -s` prints the e_ref table of DESIGN §3.
"""
import numpy as np
import pytest

import plan_cases as PC

LIVE = [c for c in PC.CASES + (PC.R0_CASE,) if c[1] <= PC.LIVE_MAX]


def test_case_list():
    names = [c[0] for c in PC.all_cases()]
    assert len(set(names)) == len(names)
    assert set(c[0] for c in PC.CASES) <= set(names)
    assert {c[1] for c in PC.CASES if c[2] == PC.POINTS[0]} == set(PC.DEFAULT_N)
    for w in range(1, len(PC.POINTS)):
        assert {c[1] for c in PC.CASES if c[2] == PC.POINTS[w]} == set(PC.WEIGHT_N)
    # the R = 0 case is in the file exactly when the reference alone meets the keep condition
    r0 = PC._file()["r0_eref"]
    assert (PC.R0_CASE[0] in names) == bool(r0.max() <= PC.KEEP_BAR)
    assert PC.SCAN_DOUBLES == 2928 and PC.FFT_G_COMPLEX == sum(PC.FFT_SIZES)


@pytest.mark.parametrize("case", LIVE, ids=[c[0] for c in LIVE])
def test_truth_live(case):
    """Every case with N <= 33 solved again: the file bit for bit; the truth's residuals
    L·Lᵀ − M, G·Hz − I and Pu·v − e0 in mpmath (60 digits; the worst condition number of these
    cases, R = 0, leaves more than 30); M from exact integers and the scan tables from
    fixed-point integers against mpmath's own, bit for bit."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    name, N, _ = case
    if name not in [c[0] for c in PC.all_cases()]:
        pytest.skip("case not kept in the stored file")
    t = PC.truth(case, full=True)
    r = PC.rounded(t)
    d = PC._file()
    for key, a in r.items():
        assert np.array_equal(a, d[f"{name}/{key}"]), key
    inp = PC.inputs(case)
    with mp.workdps(60):
        L, M, Hz, G, v, p = t["L"], t["M"], t["Hz"], t["G"], t["v"], t["p"]
        res_l = max(abs(mp.fdot(L[i], L[j]) - M[i][j]) for i in range(N) for j in range(N))
        res_g = max(abs(mp.fdot(G[i], [Hz[m][j] for m in range(N)]) - (1 if i == j else 0))
                    for i in range(N) for j in range(N))
        res_v = max(abs(mp.fdot(p[:i + 1][::-1], v[:i + 1]) - (1 if i == 0 else 0))
                    for i in range(N))
        mmax = max(abs(x) for row in M for x in row)
        assert res_l <= mp.mpf(10) ** -55 * mmax
        assert res_g <= mp.mpf(10) ** -30
        assert res_v <= mp.mpf(10) ** -30
        s = PC.stored(name)
        assert np.array_equal(s["M"], np.array([[float(x) for x in row] for row in M]))
        # the scan tables: mpmath's powers of Ā from the full 60-digit kx
        A = mp.matrix([[1, inp["T"], inp["T2_2"]], [0, 1, inp["T"]], [0, 0, 1]])
        Bv = mp.matrix([inp["T3_6"], inp["T2_2"], inp["T"]])
        Ab = A - Bv * mp.matrix(t["kx"]).T
        flat = lambda W: [float(W[i, j]) for i in range(3) for j in range(3)]
        pw = [mp.eye(3)]
        for _ in range(8 * 64):
            pw.append(pw[-1] * Ab)
        want = np.zeros(PC.SCAN_DOUBLES)
        for C in range(1, 9):
            for rr in range(PC.SCAN_LEVELS):
                o = (C - 1) * PC.SCAN_STRIDE + 9 * rr
                want[o:o + 9] = flat(pw[C << rr])
            for k in range(PC.SCAN_POWERS):
                o = PC.SCAN_POW_OFF + ((C - 1) * PC.SCAN_POWERS + k) * 9
                want[o:o + 9] = flat(pw[C * k])
        for q in range(8):
            V = pw[q] * Bv
            o = PC.SCAN_G_OFF + 6 * q
            want[o:o + 3] = [float(V[i]) for i in range(3)]
            want[o + 3:o + 6] = [float(pw[q][i, 1]) for i in range(3)]
        assert np.array_equal(s["scan"], want)
        # the table layouts from the rounded truth
        tab, zero = s["ksum_table"], s["ksum_zero"]
        assert len(tab) == N + 18 and np.all(tab[zero] == 0.0) and tab[N + 16] == float(t["ksum"][0])
        for j in range(1, N):
            assert tab[j + 8] == float(t["ksum"][j]) and not zero[j + 8]
        assert int(zero.sum()) == 18


def test_twiddle_symmetries():
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    tw = PC.twiddles_from_octant(PC._file()["tw_octant"])
    assert tw.shape == (PC.FFT_PT,)
    with mp.workdps(60):
        for m in list(range(0, PC.FFT_PT, 97)) + [1023, 1024, 1025, 2048, 4096, 6144, 8191]:
            z = mp.expjpi(mp.mpf(-2 * m) / PC.FFT_PT)
            assert tw[m] == complex(float(z.real), float(z.imag)), m


def test_layout_helpers():
    k = np.arange(1.0, 8.0)                                   # N = 7
    t = PC.kffa_from(k)
    assert t.shape == ((7 + 2) // 2 + 8, 4)
    assert t[:5].tolist() == [[1, 2, 1, 0], [3, 4, 5, 0], [5, 6, 9, 0], [7, 0, 13, 0],
                              [0, 0, 0, 0]]
    assert not t[4:].any()
    S = PC.ksum_sequential(k)
    assert S.tolist() == [28, 27, 25, 22, 18, 13, 7]
    tab, zero = PC.ksum_layout(S)
    assert tab.tolist() == [0] * 9 + [27, 25, 22, 18, 13, 7] + [0] * 8 + [28, 0]
    assert zero.tolist() == [True] * 9 + [False] * 6 + [True] * 8 + [False, True]


def test_reference_distance_from_truth():
    """e_ref: the float64 oracle's own distance from truth, every stored quantity of every case.
    The keep condition (k and kx within 1e-10 of truth by the reference alone) holds for every
    case in the file, and every bar that follows lies between its floor and 1e-8."""
    lines = []
    for point in PC.POINTS + (PC.R0_POINT,):
        cases = PC.point_cases(point)
        if not cases:
            continue
        worst = {}
        for c in cases:
            e = PC.e_ref(c[0])
            assert all(np.isfinite(v) for v in e.values()), (c[0], e)
            assert e["k"] <= PC.KEEP_BAR and e["kx"] <= PC.KEEP_BAR, (c[0], e)
            for key, v in e.items():
                worst[key] = max(worst.get(key, 0.0), v)
        b = PC.bars(point)
        assert all(PC.BAR_FLOOR <= b[key] < 1e-8 for key in PC.QUANTITIES), (point, b)
        rho = [PC.stored(c[0])["rho"] for c in cases]
        lines.append(f"{point}: rho {min(rho):.3f}..{max(rho):.3f}  " +
                     "  ".join(f"{key} {worst[key]:.1e}" for key in PC.QUANTITIES))
    print("\ne_ref (float64 reference vs truth, worst per weight point):")
    print("\n".join(lines))


def test_rollout_cases_on_the_cpu():
    """The unconstrained rollouts of the weight points: which (case, n) pairs the ρ(Ā)^n cut
    leaves out (at most a quarter), and on the rest the distance between the reference's two runs
    (true gain, numpy's gain) that sets the device bar."""
    pairs, dropped, lines = 0, [], []
    for N in PC.WEIGHT_N:
        for w, point in enumerate(PC.POINTS):
            case = (PC.case_name(N, w), N, point)
            s = PC.stored(case[0])
            run, out = PC.rollout_lengths(s["rho"])
            pairs += len(run) + len(out)
            dropped += [(case[0], n) for n in out]
            for n in run:
                rc = PC.rollout_case(case[0], n)
                ref = PC.rollout_reference(case, rc, gain=(s["k"], s["kx"]))
                own = PC.rollout_reference(case, rc)
                assert np.isfinite(ref).all()
                # per-walk kicks land: the walk differs from the same walk without its kick
                nokick = PC.rollout_reference(case, dict(rc, kick=np.zeros(PC.ROLLOUT_B)),
                                              gain=(s["k"], s["kx"]))
                assert all(np.array_equal(nokick[b, :rc["kick_step"][b] + 1],
                                          ref[b, :rc["kick_step"][b] + 1]) and
                           not np.array_equal(nokick[b], ref[b]) for b in range(PC.ROLLOUT_B))
                lines.append(f"{case[0]} n={n} rho^n={s['rho'] ** n:.1e} "
                             f"|ref|max={np.abs(ref).max():.1e} two runs {PC.rel_hist(own, ref):.1e}")
    assert 4 * len(dropped) <= pairs, (dropped, pairs)
    print(f"\nrollout pairs {pairs}, left out {dropped}")
    print("\n".join(lines))
