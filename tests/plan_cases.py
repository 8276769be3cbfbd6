"""Cases, extended-precision truth and float64 references of the plan build (csrc/plan.hip), shared
by the host test tests/test_plan_cases_host.py, the device test tests/test_gpu_plan_cases.py and
the generator of the stored truth, tests/golden/make_plan_truth_golden.py.  Not a test module.

A case is (N, weight point); its inputs are regenerated from its name, never stored.  `truth`
solves a case with mpmath at 60 digits, starting from the float64 p and Px (bit-exact with the
device, so taken as exact inputs, as are the host-evaluated LIPM constants the device receives;
R/Q is the exact quotient, so that G·Hz = I holds in the truth: the device's float64 quotient
moves M's diagonal by half an ulp of R/Q at most, a 2^-7 part of the bars' floor).
tests/golden/plan_truth.npz holds that truth rounded to float64; everything that runs with the
device reads only the file (`stored`) and never imports mpmath.

Two truths need no mpmath and are therefore derived where they are used, from exact inputs, in
Python integers: M (`exact_gram`: sums of products of doubles are dyadic rationals) and the
rollout scan tables (`scan_truth`: powers of Ā = A − B·kxᵀ in 400-bit fixed point from the true
kx, stored as three doubles kx + kx_lo + kx_lo2).  Storing the scan block itself would cost 23 KB
per case; the host test holds `scan_truth` to mpmath's matrix powers bit for bit.

Table layouts, restated from csrc/zmpc_internal.h and csrc/dispatch.h (a layout change there has
to edit this file):
  kffa   [(N + 2)//2 + 8][4]  row m = (E_m, O_m, E_m + O_{m−1}, 0), E_m = k_{2m}, O_m = k_{2m+1},
                              zero outside [0, N)
  ksum   [N + 18]             entry i = S_{i−8} for 1 <= i − 8 <= N − 1, S_0 at N + 16, zero
                              elsewhere; S_j = Σ_{j' >= j} k_{j'}
  scan   [2928]               [8][7][9] (Ā^C)^(2^r) at (C − 1)·63 + 9r, C = 1..8, r = 0..6; then at
                              504 [8][33][9] (Ā^C)^k, k = 0..32; then at 2880 [8][6] (Ā^p·B, Ā^p·e1),
                              p = 0..7; 3x3 matrices row-major
  fft_tw [8192] complex       e^{−2πi m/8192}
  fft_g  [16128] complex      for P = 256, 512, .., 8192 at offset P − 256: DFT(g)[q]/P, q < P,
                              g[d] = k_{d−1} for d = 1..N, zero elsewhere
"""
import functools
import os

import numpy as np

from oracle import zmp_oracle as O

# (Q, R, h, g): the default weights, the five strict weight points, and the fourth (Q, R, h)
# point of tests/strict_cases.py
POINTS = ((1.0, 1e-6, 0.75, 9.81),
          (1.0, 1e-9, 0.75, 9.81), (100.0, 1e-2, 1.0, 9.81), (0.1, 1e-3, 0.5, 9.81),
          (10.0, 1e-5, 0.9, 3.71), (0.1, 1e-11, 1.0, 9.81),
          (1.0, 1e-2, 0.75, 9.81))
R0_POINT = (1.0, 0.0, 0.75, 9.81)
DEFAULT_N = (1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 66, 67, 68, 69,
             70, 71, 72, 127, 128, 129, 150)
WEIGHT_N = (17, 65, 129)
ROWS = (0, 15, 16, 17, -1)      # stored rows of L (-1: N − 1)
WIDE_ROWS = (0, 16, -1)         # stored rows of X, G and Hz (15 and 17 dropped for the file size)
LIVE_MAX = 33                   # the host test re-derives cases up to this horizon

KFFA_PAD = 8
KSUM_LEAD, KSUM_TAIL = 8, 18
SCAN_LEVELS, SCAN_POWERS = 7, 33
SCAN_STRIDE = SCAN_LEVELS * 9
SCAN_POW_OFF = 8 * SCAN_STRIDE
SCAN_G_OFF = SCAN_POW_OFF + 8 * SCAN_POWERS * 9
SCAN_DOUBLES = SCAN_G_OFF + 8 * 6
FFT_PT, FFT_PMIN = 8192, 256
FFT_SIZES = tuple(FFT_PMIN << i for i in range(6))
FFT_G_COMPLEX = 2 * FFT_PT - FFT_PMIN

ULP = 2.0 ** -52
BAR_FACTOR, BAR_FLOOR = 16.0, 64 * ULP
KEEP_BAR = 1e-10                # a case is kept only if the reference alone has k, kx within this

TRUTH_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_truth.npz")


def case_dt(N):
    return 0.01 if N <= 64 else 1.5 / N


def case_name(N, w):
    return f"N{N}-w{w}"


CASES = tuple([(case_name(N, 0), N, POINTS[0]) for N in DEFAULT_N] +
              [(case_name(N, w), N, POINTS[w]) for N in WEIGHT_N for w in range(1, len(POINTS))])
# R = 0 at N = 16: kept only if it meets KEEP_BAR (the generator decides and says)
R0_CASE = ("N16-R0", 16, R0_POINT)


def point_cases(point):
    return [c for c in all_cases() if c[2] == point]


@functools.lru_cache(maxsize=None)
def all_cases():
    """The cases of the stored file: CASES, and R0_CASE if the generator kept it."""
    names = set(str(s) for s in _file()["names"])
    return tuple(c for c in CASES + (R0_CASE,) if c[0] in names)


def inputs(case):
    """→ dict of the float64 inputs of a case: p [N], Px [N,3], the host constants and weights."""
    _, N, (Q, R, h, g) = case
    dt = case_dt(N)
    Px, Pu = O.prediction_matrices(N, dt, h, g)
    return dict(N=N, dt=dt, Q=Q, R=R, h=h, g=g, p=Pu[:, 0].copy(), Px=Px, Pu=Pu,
                T=dt, T2_2=dt ** 2 / 2., T3_6=dt ** 3 / 6.)


def rows_of(N, which):
    return sorted({r % N for r in which if -N <= r < N})


def fft_q(P):
    return (0, 1, P // 2 - 1, P // 2, P - 1)


# ----------------------------------------------------------------------------- exact integers

def _fix(x, S):
    """The double x as an integer multiple of 2^−S, exactly."""
    num, den = float(x).as_integer_ratio()
    k = den.bit_length() - 1
    assert S >= k, (x, S)
    return num << (S - k)


def exact_gram(c, R, Q):
    """C = TᵀT + (R/Q)·I for the lower-triangular Toeplitz T[k][a] = c[k − a], correctly rounded
    to float64 from exact rationals: C[a][b] = C[a+1][b+1] + c[N−1−a]·c[N−1−b]."""
    from fractions import Fraction
    N, S = len(c), 1100
    ci = [_fix(x, S) for x in c]
    den = 1 << (2 * S)
    diag = Fraction(R) / Fraction(Q)
    C = np.empty((N, N))
    prev = [0] * (N + 1)
    for a in range(N - 1, -1, -1):
        row = [0] * (N + 1)
        for b in range(N):
            row[b] = prev[b + 1] + ci[N - 1 - a] * ci[N - 1 - b]
            C[a, b] = row[b] / den if a != b else float(Fraction(row[b], den) + diag)
        prev = row
    return C


SCAN_FRAC = 400


def _mat_powers(Ab, upto):
    """[Ā^0 .. Ā^upto] of a 3x3 fixed-point matrix (flat 9 ints at 2^−SCAN_FRAC)."""
    one = 1 << SCAN_FRAC
    W = [one, 0, 0, 0, one, 0, 0, 0, one]
    out = [W]
    for _ in range(upto):
        W = [(W[3 * i] * Ab[j] + W[3 * i + 1] * Ab[3 + j] + W[3 * i + 2] * Ab[6 + j]) >> SCAN_FRAC
             for i in range(3) for j in range(3)]
        out.append(W)
    return out


def scan_fixed(kx_parts, T, T2_2, T3_6):
    """Ā = A − B·kxᵀ and its powers 0..512 in fixed point; kx_parts: arrays [3] whose sum is kx."""
    S = SCAN_FRAC
    kx = [sum(_fix(part[j], 1100) for part in kx_parts) for j in range(3)]      # at 2^−1100
    A = [1.0, T, T2_2, 0.0, 1.0, T, 0.0, 0.0, 1.0]
    Bv = [T3_6, T2_2, T]
    Ab = [(_fix(A[3 * i + j], 1100) << 1100) - _fix(Bv[i], 1100) * kx[j]
          for i in range(3) for j in range(3)]                                    # at 2^−2200
    Ab = [x >> (2200 - S) for x in Ab]
    return Ab, _mat_powers(Ab, 8 * (1 << (SCAN_LEVELS - 1))), [_fix(b, S) for b in Bv]


def scan_truth(kx_parts, T, T2_2, T3_6):
    """The scan block [SCAN_DOUBLES] from the true kx, each entry correctly rounded."""
    _, pw, Bv = scan_fixed(kx_parts, T, T2_2, T3_6)
    S, den = SCAN_FRAC, 1 << SCAN_FRAC
    out = np.zeros(SCAN_DOUBLES)
    for C in range(1, 9):
        for r in range(SCAN_LEVELS):
            o = (C - 1) * SCAN_STRIDE + 9 * r
            out[o:o + 9] = [x / den for x in pw[C << r]]
        for k in range(SCAN_POWERS):
            o = SCAN_POW_OFF + ((C - 1) * SCAN_POWERS + k) * 9
            out[o:o + 9] = [x / den for x in pw[C * k]]
    for p in range(8):
        W = pw[p]
        for i in range(3):
            v = (W[3 * i] * Bv[0] + W[3 * i + 1] * Bv[1] + W[3 * i + 2] * Bv[2]) >> S
            out[SCAN_G_OFF + 6 * p + i] = v / den
            out[SCAN_G_OFF + 6 * p + 3 + i] = W[3 * i + 1] / den
    return out


def scan_groups():
    """Slices of the scan block that are one quantity each (a 3x3 matrix, a 3-vector): errors are
    taken relative to the largest magnitude of the group, not of the block (Ā^512 reaches 1e70 at
    the weight points with ρ(Ā) > 1)."""
    g = [slice(o, o + 9) for o in range(0, SCAN_G_OFF, 9)]
    return g + [slice(o, o + 3) for o in range(SCAN_G_OFF, SCAN_DOUBLES, 3)]


def scan_float64(kx, T, T2_2, T3_6):
    """The float64 run of the device's scan-table recurrences (plan.hip zmpc_scan_matrices: the
    same order of products, plain multiply-adds)."""
    A = np.array([[1.0, T, T2_2], [0.0, 1.0, T], [0.0, 0.0, 1.0]])
    Bv = np.array([T3_6, T2_2, T])
    Ab = A - np.outer(Bv, kx)
    out = np.zeros(SCAN_DOUBLES)
    V, E = Bv.copy(), np.array([0.0, 1.0, 0.0])
    for p in range(8):
        out[SCAN_G_OFF + 6 * p:SCAN_G_OFF + 6 * p + 3] = V
        out[SCAN_G_OFF + 6 * p + 3:SCAN_G_OFF + 6 * p + 6] = E
        V, E = Ab @ V, Ab @ E
    P = Ab.copy()
    for C in range(1, 9):
        if C > 1:
            P = P @ Ab
        W = np.eye(3)
        for k in range(SCAN_POWERS):
            o = SCAN_POW_OFF + ((C - 1) * SCAN_POWERS + k) * 9
            out[o:o + 9] = W.ravel()
            W = W @ P
        Qm = P.copy()
        for r in range(SCAN_LEVELS):
            o = (C - 1) * SCAN_STRIDE + 9 * r
            out[o:o + 9] = Qm.ravel()
            Qm = Qm @ Qm
    return out


def spectral_radius(kx, T, T2_2, T3_6):
    A = np.array([[1.0, T, T2_2], [0.0, 1.0, T], [0.0, 0.0, 1.0]])
    return float(np.abs(np.linalg.eigvals(A - np.outer([T3_6, T2_2, T], kx))).max())


# ----------------------------------------------------------------------------- layouts from k

def kffa_from(k):
    """The fast-FIR rows of a gain row: copies and one addition, so bit-exact from the same k."""
    N = len(k)
    rows = (N + 2) // 2 + KFFA_PAD
    kz = np.concatenate([k, np.zeros(2 * rows + 2 - N)])
    t = np.zeros((rows, 4))
    m = np.arange(rows)
    t[:, 0], t[:, 1] = kz[2 * m], kz[2 * m + 1]
    t[1:, 2] = kz[2 * m[1:]] + kz[2 * m[1:] - 1]
    t[0, 2] = kz[0] + 0.0
    return t


def ksum_layout(S):
    """Suffix sums S [N] (S[j] = Σ_{j' >= j} k_{j'}) in the ksum layout, and the mask of its
    structural zeros."""
    N = len(S)
    t = np.zeros(N + KSUM_TAIL)
    t[KSUM_LEAD + 1:KSUM_LEAD + N] = S[1:]
    t[N + 16] = S[0]
    zero = np.ones(N + KSUM_TAIL, bool)
    zero[KSUM_LEAD + 1:KSUM_LEAD + N] = False
    zero[N + 16] = False
    return t, zero


def ksum_sequential(k):
    """The float64 sequential suffix sum, in the device's order (from j = N − 1 down)."""
    S = np.empty(len(k))
    acc = 0.0
    for j in range(len(k) - 1, -1, -1):
        acc = acc + k[j]
        S[j] = acc
    return S


def twiddles_from_octant(octant):
    """e^{−2πi m/8192}, m < 8192, from the stored first octant (cos, sin of 2π m/8192 for
    m = 0..1024) by the exact symmetries of the circle."""
    n8 = FFT_PT // 8
    c, s = np.empty(FFT_PT // 4 + 1), np.empty(FFT_PT // 4 + 1)
    c[:n8 + 1], s[:n8 + 1] = octant[:, 0], octant[:, 1]
    c[n8:] = octant[::-1, 1]                       # cos(π/2 − x) = sin x
    s[n8:] = octant[::-1, 0]
    q = FFT_PT // 4
    cos = np.concatenate([c[:q], -s[:q], -c[:q], s[:q]])
    sin = np.concatenate([s[:q], c[:q], -s[:q], -c[:q]])
    return cos - 1j * sin


def fft_g_float64(k, tw):
    """DFT(g)/P at the stored q of every P, float64, from a gain row and a twiddle table."""
    N = len(k)
    out = {}
    d = np.arange(1, N + 1)
    for P in FFT_SIZES:
        sh = FFT_PT // P
        out[P] = np.array([np.sum(k * tw[((q * d) % P) * sh]) / P for q in fft_q(P)])
    return out


# ----------------------------------------------------------------------------- truth (mpmath)

def truth(case, full=False):
    """A case solved with mpmath at 60 digits → dict of mp values: M, L (lists of rows), y, k,
    kx, ksum (S_0..S_{N−1}), v, Xt (columns of X), Hz, G rows (every row when full), fft_g
    {P: [5]}.  Host only."""
    import mpmath
    mp = mpmath.mp
    inp = inputs(case)
    N, Q, R = inp["N"], inp["Q"], inp["R"]
    with mp.workdps(60):
        mpf, fdot = mp.mpf, mp.fdot
        p = [mpf(float(x)) for x in inp["p"]]
        Px = [[mpf(float(x)) for x in row] for row in inp["Px"]]
        Qm, Rm = mpf(Q), mpf(R)
        RQ = Rm / Qm

        def gram(c, scale, diag):
            C = [[None] * N for _ in range(N)]
            for a in range(N - 1, -1, -1):
                for b in range(N):
                    nxt = C[a + 1][b + 1] if a + 1 < N and b + 1 < N else mpf(0)
                    C[a][b] = nxt + c[N - 1 - a] * c[N - 1 - b]
            return [[scale * C[a][b] + (diag if a == b else 0) for b in range(N)]
                    for a in range(N)]

        M = gram(p, mpf(1), RQ)
        L = [[mpf(0)] * N for _ in range(N)]
        for j in range(N):
            L[j][j] = mp.sqrt(M[j][j] - fdot(L[j][:j], L[j][:j]))
            for i in range(j + 1, N):
                L[i][j] = (M[i][j] - fdot(L[i][:j], L[j][:j])) / L[j][j]
        Lt = [[L[i][j] for i in range(N)] for j in range(N)]
        w = []
        for i in range(N):
            w.append(((1 if i == 0 else 0) - fdot(L[i][:i], w)) / L[i][i])
        y = [None] * N
        for i in range(N - 1, -1, -1):
            y[i] = (w[i] - fdot(Lt[i][i + 1:], y[i + 1:])) / L[i][i]
        k = [fdot(p[:j + 1][::-1], y[:j + 1]) for j in range(N)]
        kx = [fdot(k, [Px[j][c] for j in range(N)]) for c in range(3)]
        ksum, acc = [None] * N, mpf(0)
        for j in range(N - 1, -1, -1):
            acc = acc + k[j]
            ksum[j] = acc
        Xt = []
        for c in range(N):
            col = []
            for i in range(N):
                rhs = p[c - i] if i <= c else mpf(0)
                col.append((rhs - fdot(L[i][:i], col)) / L[i][i])
            Xt.append(col)
        grows = range(N) if full else rows_of(N, WIDE_ROWS)
        G = {r: [fdot(Xt[r], Xt[c]) / Qm for c in range(N)] for r in grows}
        v = [1 / p[0]]
        for kk in range(1, N):
            v.append(-fdot(p[1:kk + 1], v[kk - 1::-1]) / p[0])
        Hz = gram(v, Rm, Qm)
        fft_g = {}
        for P in FFT_SIZES:
            fft_g[P] = [sum(k[d - 1] * mp.expjpi(mpf(-2 * ((q * d) % P)) / P)
                            for d in range(1, N + 1)) / P for q in fft_q(P)]
        return dict(N=N, p=p, M=M, L=L, y=y, k=k, kx=kx, ksum=ksum, Xt=Xt, G=G, v=v, Hz=Hz,
                    fft_g=fft_g)


def twiddle_octant_truth():
    import mpmath
    mp = mpmath.mp
    with mp.workdps(60):
        return np.array([[float(mp.cospi(mp.mpf(2 * m) / FFT_PT)),
                          float(mp.sinpi(mp.mpf(2 * m) / FFT_PT))]
                         for m in range(FFT_PT // 8 + 1)])


def split3(x):
    """An mp number as three doubles hi + lo + lo2 (round to nearest each time)."""
    import mpmath
    with mpmath.mp.workdps(60):
        a = float(x)
        b = float(x - mpmath.mpf(a))
        c = float(x - mpmath.mpf(a) - mpmath.mpf(b))
    return a, b, c


def rounded(t):
    """The stored form of a truth: every quantity rounded to float64 (plan_truth.npz's arrays of
    one case, without the name prefix)."""
    N = t["N"]
    f = lambda seq: np.array([float(x) for x in seq])
    kx3 = np.array([split3(x) for x in t["kx"]])
    out = dict(k=f(t["k"]), kx=kx3[:, 0].copy(), kx_lo=kx3[:, 1].copy(), kx_lo2=kx3[:, 2].copy(),
               v=f(t["v"]), ksum=f(t["ksum"]))
    out["L"] = np.concatenate([f(t["L"][r][:r + 1]) for r in rows_of(N, ROWS)])
    wide = rows_of(N, WIDE_ROWS)
    out["X"] = np.array([[float(t["Xt"][c][r]) for c in range(N)] for r in wide])
    out["G"] = np.array([f(t["G"][r]) for r in wide])
    out["Hz"] = np.array([f(t["Hz"][r]) for r in wide])
    out["fft_g"] = np.array([[complex(z) for z in t["fft_g"][P]] for P in FFT_SIZES])
    return out


# ----------------------------------------------------------------------------- the stored truth

@functools.lru_cache(maxsize=None)
def _file():
    return np.load(TRUTH_FILE, allow_pickle=False)


@functools.lru_cache(maxsize=None)
def stored(name):
    """The stored truth of a case → dict as `rounded`, L rows unpacked to {row: [row + 1]}, plus
    the truths derived in exact integers: M, scan; and the twiddles, the layouts of k."""
    case = next(c for c in CASES + (R0_CASE,) if c[0] == name)
    d = _file()
    s = {key: d[f"{name}/{key}"] for key in ("k", "kx", "kx_lo", "kx_lo2", "v", "ksum", "L", "X",
                                             "G", "Hz", "fft_g")}
    inp = inputs(case)
    N = inp["N"]
    rows, o = {}, 0
    for r in rows_of(N, ROWS):
        rows[r] = s["L"][o:o + r + 1]
        o += r + 1
    assert o == len(s["L"])
    s["L"] = rows
    s["wide_rows"] = rows_of(N, WIDE_ROWS)
    s["M"] = exact_gram(inp["p"], inp["R"], inp["Q"])
    s["scan"] = scan_truth((s["kx"], s["kx_lo"], s["kx_lo2"]), inp["T"], inp["T2_2"], inp["T3_6"])
    s["fft_tw"] = twiddles_from_octant(d["tw_octant"])
    s["ksum_table"], s["ksum_zero"] = ksum_layout(s["ksum"])
    s["rho"] = spectral_radius(s["kx"], inp["T"], inp["T2_2"], inp["T3_6"])
    return s


# ----------------------------------------------------------------------------- float64 reference

def reference(case):
    """The float64 oracle's own value of every compared quantity (what the project's tests held
    the device to before): gain_row, strict_matrices, np.linalg.inv(Hz), LAPACK's Cholesky and
    solve, the float64 sequential suffix sum and scan recurrences, numpy's exp."""
    inp = inputs(case)
    N, dt, Q, R, h, g = (inp[key] for key in ("N", "dt", "Q", "R", "h", "g"))
    k, kx = O.gain_row(N, dt, h, g, Q, R)
    Hz, V, _, Pu = O.strict_matrices(N, dt, h, g, Q, R)
    M = Pu.T @ Pu + R / Q * np.eye(N)
    L = np.linalg.cholesky(M)
    tw = np.exp(-2j * np.pi * np.arange(FFT_PT) / FFT_PT)
    return dict(M=M, k=k, kx=kx, L=L, X=np.linalg.solve(L, Pu.T), G=np.linalg.inv(Hz), Hz=Hz,
                v=V[:, 0].copy(), ksum=ksum_layout(ksum_sequential(k))[0],
                scan=scan_float64(kx, inp["T"], inp["T2_2"], inp["T3_6"]), fft_tw=tw,
                fft_g=fft_g_float64(k, tw))


QUANTITIES = ("M", "k", "kx", "L", "X", "G", "Hz", "v", "ksum", "scan", "fft_tw", "fft_g")


def _rel(a, ref):
    ref = np.asarray(ref)
    scale = float(np.abs(ref).max())
    diff = float(np.abs(np.asarray(a) - ref).max())
    return diff / scale if scale > 0 else (0.0 if diff == 0 else np.inf)


def distances(q, name):
    """Distance of a set of quantities q (dict as `reference` returns; full matrices, tables in
    the device layout) from the stored truth of a case: {quantity: largest |difference| relative
    to the quantity's largest true magnitude} over what the file stores of it."""
    s = stored(name)
    N = len(s["k"])
    out = dict(M=_rel(q["M"], s["M"]), k=_rel(q["k"][:N], s["k"]), kx=_rel(q["kx"], s["kx"]),
               ksum=_rel(q["ksum"], s["ksum_table"]), fft_tw=_rel(q["fft_tw"], s["fft_tw"]))
    Lrows = np.concatenate([q["L"][r, :r + 1] for r in s["L"]])
    out["L"] = _rel(Lrows, np.concatenate([s["L"][r] for r in s["L"]]))
    if "v" in q:                # (a non-strict plan holds neither v nor X, G, Hz)
        out["v"] = _rel(q["v"], s["v"])
        for key in ("X", "G", "Hz"):
            out[key] = _rel(q[key][s["wide_rows"]], s[key])
    out["scan"] = max(_rel(q["scan"][g], s["scan"][g]) for g in scan_groups())
    out["fft_g"] = max(_rel(q["fft_g"][P], s["fft_g"][i]) for i, P in enumerate(FFT_SIZES))
    return out


@functools.lru_cache(maxsize=None)
def e_ref(name):
    case = next(c for c in CASES + (R0_CASE,) if c[0] == name)
    return distances(reference(case), name)


@functools.lru_cache(maxsize=None)
def bars(point):
    """{quantity: bar} of a weight point: BAR_FACTOR x the float64 reference's own distance from
    truth, the maximum over the cases sharing the point, floor 64 ulp."""
    es = [e_ref(c[0]) for c in point_cases(point)]
    return {key: max(BAR_FLOOR, BAR_FACTOR * max(e[key] for e in es)) for key in QUANTITIES}


def identity_residual(G, Hz):
    """max |G·Hz − I| in float64, and the scale of the product's own rounding, max (|G|·|Hz|)."""
    N = len(G)
    return (float(np.abs(G @ Hz - np.eye(N)).max()), float((np.abs(G) @ np.abs(Hz)).max()))


def gram_residual(X, G, Q):
    """max |XᵀX/Q − G| in float64, relative to the largest |G|."""
    return float(np.abs(X.T @ X / Q - G).max() / np.abs(G).max())


@functools.lru_cache(maxsize=None)
def identity_bars(point):
    """Bars of the two identities that join separately computed matrices, at a weight point:
    BAR_FACTOR x the reference's own residual (G = np.linalg.inv(Hz), X = solve(L, Puᵀ)), the
    maximum over the point's cases → (bar of max |G·Hz − I|, to which the caller adds the floor of
    64 ulp of its own max (|G|·|Hz|); bar of max |XᵀX/Q − G| / max |G|, floor included)."""
    ghz = gram = 0.0
    for c in point_cases(point):
        r = reference(c)
        ghz = max(ghz, identity_residual(r["G"], r["Hz"])[0])
        gram = max(gram, gram_residual(r["X"], r["G"], c[2][0]))
    return BAR_FACTOR * ghz, max(BAR_FLOOR, BAR_FACTOR * gram)


def device_fft_g(table):
    """The stored q of every P out of an exported fft_g table [16128] complex."""
    return {P: table[P - FFT_PMIN + np.array(fft_q(P))] for P in FFT_SIZES}


# ----------------------------------------------------------------------------- rollouts

ROLLOUT_N = (40, 130, 420)      # chunk widths 1, 3 and 7; 420 only where ρ(Ā) <= 1
ROLLOUT_B = 6
RHO_CUT = 1e6                   # a walk with ρ(Ā)^n beyond is left out: the reference's own two
#                                 runs (true gain, numpy's gain) disagree there


def rollout_lengths(rho):
    """→ (lengths run, lengths left out) at a spectral radius."""
    want = [n for n in ROLLOUT_N if n != 420 or rho <= 1.0]
    run = [n for n in want if rho ** n <= RHO_CUT]
    return run, [n for n in want if n not in run]


def rollout_case(name, n):
    """B = 6 walks of n samples: walks 0, 2, 4 on random-walk bounds (z_ref changes at every
    sample: the dense correlation), walks 1, 3, 5 on piecewise-constant bounds of 5 to 9 runs per
    axis (the sparse-difference correlation); x0 != 0, a kick and a kick step per walk."""
    import zlib
    B = ROLLOUT_B
    zc = np.empty((B, n, 2))
    for b in range(B):
        rng = np.random.default_rng([zlib.crc32(name.encode()), n, b])
        if b % 2 == 0:
            zc[b] = np.cumsum(rng.uniform(-0.01, 0.01, (n, 2)), axis=0)
        else:
            for a in range(2):
                cuts = np.sort(rng.permutation(np.arange(1, n))[:int(rng.integers(4, 9))])
                lev = np.cumsum(rng.uniform(-0.1, 0.1, len(cuts) + 1))
                zc[b, :, a] = lev[np.searchsorted(cuts, np.arange(n), side="right")]
    rng = np.random.default_rng([zlib.crc32(name.encode()), n, B])
    hw = rng.uniform(0.01, 0.06, (B, 1, 2))
    x0 = np.empty((B, 2, 3))
    x0[:, :, 0] = rng.uniform(-0.05, 0.05, (B, 2))
    x0[:, :, 1] = rng.uniform(-0.2, 0.2, (B, 2))
    x0[:, :, 2] = rng.uniform(-0.5, 0.5, (B, 2))
    kick = rng.uniform(-0.1, 0.1, B)
    ks = rng.integers(n // 4, 3 * n // 4, B).astype(np.int64)
    return dict(zmax=zc + hw, zmin=zc - hw, x0=x0, kick=kick, kick_step=ks)


def rollout_reference(case, rc, gain=None):
    _, N, (Q, R, h, g) = case
    return O.rollout_gain(rc["zmax"], rc["zmin"], rc["x0"], N, case_dt(N), h, g, Q, R,
                          kick=rc["kick"], kick_step=rc["kick_step"], gain=gain)


def rel_hist(a, ref):
    return float((np.abs(a - ref) / np.maximum(1.0, np.abs(ref))).max())
