"""Cases, extended-precision truth and bars of the long-walk rollout kernels (csrc/rollout_long.hip:
the wide kernel's 32 instances and the chunk kernel), shared by the host test
tests/test_long_walk_cases_host.py and the device test tests/test_gpu_long_walk.py.  Not a test
module.

Truth.  The gain row k = Pu·y, kx = k·Px with (PuᵀPu + (R/Q)·I)·y = e0: scipy's float64 Cholesky,
refined with residuals in np.longdouble (Pu is lower-triangular Toeplitz, so a residual is two
O(N²) products on its first column; M is never formed in long double) until the correction falls
below 2^-60 relative.  The rollout: the recursion of oracle.rollout_gain in np.longdouble
throughout, from the float64 inputs of the case (bounds, x0, kick, the LIPM constants as the host
evaluates them).  One truth per case, cached across kernel options.

Bars, relative to max(1, max |truth|) over the whole history of a case:
  direct, sparse and chunk forms   max(1e-12, 16·e64)
  FFT legs                         max(1e-12, 16·max(e64, efft64))
e64 is the distance of float64 oracle.rollout_gain (numpy's own gain) from the truth, efft64 the
same float64 recursion fed by a numpy-FFT correlation of the launch's period P: the FFT's own
rounding is measured on the reference, never on the device.

A case regenerates its inputs from its name.  Families (the issue's letters): A every reachable
(W, CW, E, sparse staged, LDS > 64 KiB) answer of the launch rule at the first and last n that
return it (A_TABLE, pinned against csrc/dispatch.h by the host test), B walk ends, C the chunk
kernel, D kick placement, E correlation forms, F weight points, G magnitude, H batch size,
I shared CoP, J non-finite input.
"""
import collections
import functools
import os
import zlib

import numpy as np
import scipy.linalg

import plan_cases as PC
from oracle import zmp_oracle as O

LD = np.longdouble
if np.finfo(LD).eps > 2.0 ** -63:
    raise RuntimeError("long_walk_cases needs an extended-precision np.longdouble "
                       f"(eps <= 2^-63), this platform's has eps = {np.finfo(LD).eps}")

HORIZONS = (16, 65, 129, 150, 512, 920, 1300, 4096)
POINTS = PC.POINTS
STABLE_POINTS = (0, 2, 3, 6)        # the stored weight points with ρ(Ā) <= 1 at N = 65 and 129
BAR_FLOOR, BAR_FACTOR = 1e-12, 16.0
TEETH = 100.0                       # a deliberate change must move the truth by TEETH x the bar
OFFSET = 1000.0                     # family G's rigid offset, metres

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def case_dt(N):
    if N == 150:
        return float(np.load(os.path.join(_GOLDEN, "walk_n150.npz"), allow_pickle=False)["dt"])
    return 1.5 / N


# ----------------------------------------------------------------------------- the true gain row
# The Toeplitz products of the residual carry their rounding errors along (error-free sums and
# products in np.longdouble, as compensated dot products do), and y is kept as a pair hi + lo: a
# plain long-double residual leaves y at cond(M)·2^-64, which the sums kx = k·Px (|Σ k_j| well
# below Σ |k_j|) turn into several float64 ulps at the weight points with R/Q <= 1e-9.

def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


_SPLITTER = LD(2.0 ** 32 + 1)      # Veltkamp's constant of a 64-bit significand


def _split(a):
    c = _SPLITTER * a
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    a1, a2 = _split(a)
    b1, b2 = _split(b)
    return p, a2 * b2 - (((p - a1 * b1) - a2 * b1) - a1 * b2)


def _toeplitz(p, v, transpose=False):
    """Pu·v (Puᵀ·v) for the lower-triangular Toeplitz Pu with first column p, v = (hi, lo) a pair
    of long-double vectors → (hi, lo)."""
    N = len(p)
    vh, vl = v
    hi, lo = np.zeros(N, LD), np.zeros(N, LD)
    for j in range(N):
        o, i = (slice(0, N - j), slice(j, N)) if transpose else (slice(j, N), slice(0, N - j))
        x, e = _two_prod(p[j], vh[i])
        hi[o], e2 = _two_sum(hi[o], x)
        lo[o] += (e + e2) + p[j] * vl[i]
    return hi, lo


def refine_gain(N, dt, h, g, Q, R):
    """→ (k [N], kx [3]) in np.longdouble, and (refinements, last residual max |e0 − M·y|)."""
    Px, Pu = O.prediction_matrices(N, dt, h, g)
    M = Pu.T @ Pu + R / Q * np.eye(N)
    c = scipy.linalg.cho_factor(M, lower=True)
    p, rq = Pu[:, 0].astype(LD), LD(R) / LD(Q)
    e0 = np.zeros(N, LD)
    e0[0] = 1

    def residual(y):
        sh, sl = _toeplitz(p, _toeplitz(p, y), transpose=True)
        x, e = _two_prod(rq, y[0])
        sh, e2 = _two_sum(sh, x)
        return (e0 - sh) - (sl + (e + e2) + rq * y[1])

    y = (scipy.linalg.cho_solve(c, e0.astype(np.float64)).astype(LD), np.zeros(N, LD))
    for it in range(1, 13):
        d = scipy.linalg.cho_solve(c, residual(y).astype(np.float64)).astype(LD)
        yh, e = _two_sum(y[0], d)
        y = _two_sum(yh, e + y[1])
        if np.abs(d).max() <= LD(2.0) ** -60 * np.abs(y[0]).max():
            break
    else:
        raise RuntimeError(f"gain refinement did not settle at N = {N}, R/Q = {R / Q}")
    res = float(np.abs(residual(y)).max())
    kh, kl = _toeplitz(p, y)
    kx = np.empty(3, LD)
    for a in range(3):
        x, e = _two_prod(kh, Px[:, a].astype(LD))
        acc, err = LD(0), (e + kl * Px[:, a]).sum()
        for t in x:
            acc, e2 = _two_sum(acc, t)
            err += e2
        kx[a] = acc + err
    return kh + kl, kx, (it, res)


@functools.lru_cache(maxsize=None)
def true_gain(N, w):
    Q, R, h, g = POINTS[w]
    return refine_gain(N, case_dt(N), h, g, Q, R)


@functools.lru_cache(maxsize=None)
def numpy_gain(N, w):
    Q, R, h, g = POINTS[w]
    return O.gain_row(N, case_dt(N), h, g, Q, R)


# ----------------------------------------------------------------------------- the recursion

def z_ref(zmax, zmin, N, dtype, pad_row=-1):
    """(zmax + zmin)/2 [B, n, 2] padded with N copies of row pad_row (−1: the last, as the
    reference; −2 is the deliberate change of the sensitivity conditions)."""
    zr = (np.asarray(zmax, dtype) + np.asarray(zmin, dtype)) / 2
    return np.concatenate([zr, np.repeat(zr[:, [pad_row]], N, axis=1)], axis=1)


def correlate(zr, k, n):
    """f_i = Σ_j k_j·z_ref[i + 1 + j], i < n − 1 → [B, n − 1, 2], in k's type: N vector operations."""
    f = np.zeros((zr.shape[0], n - 1, 2), k.dtype)
    for j in range(len(k)):
        f += k[j] * zr[:, 1 + j:j + n]
    return f


def correlate_fft(zr, k, n, P):
    """The same f in float64 by a circular correlation of period P >= n − 1 + N (the wide kernel's
    algorithm: both axes as one complex signal, rows past the walk's end the last row)."""
    N = len(k)
    assert P >= n - 1 + N and zr.shape[1] == n + N
    t = np.minimum(np.arange(P), n - 1)
    s = zr[:, t, 0] + 1j * zr[:, t, 1]
    gq = np.zeros(P)
    gq[1:N + 1] = k
    F = np.fft.ifft(np.fft.fft(s, axis=1) * np.conj(np.fft.fft(gq))[None, :], axis=1)
    return np.stack([F.real[:, :n - 1], F.imag[:, :n - 1]], axis=-1)


def recursion(f, x0, dt, h, g, kx, kick, kick_step):
    """x⁺ = A·x + B·(f_i − kx·x), the kick subtracted from y's velocity after the update of step
    kick_step (an int, or per-walk steps [B]); in f's type → hist [B, n, 2, 3]."""
    dtype = f.dtype
    A, Bv, _ = O.lipm(dt, h, g)
    A, Bv, kx = A.astype(dtype), Bv[:, 0].astype(dtype), np.asarray(kx, dtype)
    Bn, n = f.shape[0], f.shape[1] + 1
    x = np.asarray(x0, dtype).copy()
    hist = np.empty((Bn, n, 2, 3), dtype)
    hist[:, 0] = x
    kk = np.zeros(Bn, dtype) if kick is None else np.asarray(kick, dtype)
    ks = np.broadcast_to(np.asarray(kick_step, np.int64), (Bn,))
    hits = collections.defaultdict(list)
    for b, s in enumerate(ks):
        hits[int(s)].append(b)
    for i in range(n - 1):
        u = f[:, i, :] - x @ kx
        x = x @ A.T + u[..., None] * Bv
        if i in hits:
            x[hits[i], 1, 1] -= kk[hits[i]]
        hist[:, i + 1] = x
    return hist


def fft_period(N, n):
    P = 256
    while P < n - 1 + N:
        P *= 2
    return P


# ----------------------------------------------------------------------------- cases

# One launch of a case: ZMPC_OPT_LONG_WALK, ZMPC_OPT_CORRELATION, whether the launch is an FFT leg,
# and the kernel kind the launch rule answers (the host test holds both to csrc/dispatch.h)
Opt = collections.namedtuple("Opt", "long_walk correlation fft kind")
# gen: the batch generator ("mix", "dense", "sparse", "forms", "shared", "big"); inst: family A's
# named (W, CW, E, sparse staged, LDS > 64 KiB), None elsewhere; offset: rigid offset in metres
Case = collections.namedtuple("Case", "name family N w n B gen opts inst offset")


def _case(family, N, n, opts, B=4, gen="mix", w=0, inst=None, offset=0.0, tag=""):
    name = f"{family}-N{N}-w{w}-n{n}" + (f"-{tag}" if tag else "")
    return Case(name, family, N, w, n, B, gen, tuple(opts), inst, offset)


def wide(lw, fft, corr=0):
    return Opt(lw, corr, fft, "Wide")


DIRECT, FFT, CHUNK = wide(1, False), wide(2, True), Opt(3, 0, False, "Chunk")

# (W, CW, E, sparse staged, LDS > 64 KiB) -> (smallest horizon that reaches it, first n,
# its ZMPC_OPT_LONG_WALK, last n, its ZMPC_OPT_LONG_WALK): the sweep of n = 514..4098 over HORIZONS
# and ZMPC_OPT_LONG_WALK 0, 1, 2 (the smallest option value that returns the answer at that n)
A_TABLE = {
    (2, 5, 0, 1, 0): (16, 514, 0, 641, 0), (2, 5, 4, 1, 0): (16, 514, 2, 641, 2),
    (2, 5, 8, 1, 0): (512, 514, 0, 641, 0), (2, 6, 0, 1, 0): (16, 642, 0, 769, 0),
    (2, 6, 4, 1, 0): (16, 642, 2, 769, 2), (2, 6, 8, 1, 0): (512, 642, 0, 769, 0),
    (2, 7, 0, 1, 0): (16, 770, 0, 897, 0), (2, 7, 4, 1, 0): (16, 770, 2, 897, 2),
    (2, 7, 8, 1, 0): (129, 897, 2, 897, 2), (2, 8, 0, 1, 0): (16, 898, 0, 1025, 0),
    (2, 8, 4, 1, 0): (16, 898, 2, 1009, 2), (2, 8, 8, 1, 0): (16, 1010, 2, 1025, 2),
    (4, 5, 0, 1, 0): (16, 1026, 0, 1281, 0), (4, 5, 4, 1, 0): (16, 1026, 2, 1281, 2),
    (4, 5, 8, 1, 0): (920, 1130, 0, 1281, 0), (4, 6, 0, 1, 0): (16, 1282, 0, 1537, 0),
    (4, 6, 4, 1, 0): (16, 1282, 2, 1537, 2), (4, 6, 8, 1, 0): (920, 1282, 0, 1537, 0),
    (4, 7, 0, 1, 0): (16, 1538, 0, 1793, 0), (4, 7, 4, 1, 0): (16, 1538, 2, 1793, 2),
    (4, 7, 8, 1, 0): (512, 1538, 0, 1793, 0), (4, 8, 0, 0, 0): (1300, 1794, 1, 2049, 1),
    (4, 8, 0, 1, 0): (16, 1794, 0, 2049, 0), (4, 8, 4, 1, 0): (16, 1794, 2, 2033, 2),
    (4, 8, 8, 0, 0): (1300, 1794, 0, 2049, 0), (4, 8, 8, 1, 0): (16, 2034, 2, 2049, 2),
    (8, 5, 0, 1, 0): (16, 2050, 0, 2561, 0), (8, 5, 0, 1, 1): (1300, 2050, 1, 2561, 1),
    (8, 5, 4, 1, 0): (16, 2050, 2, 2561, 2), (8, 5, 4, 1, 1): (1300, 2050, 0, 2561, 0),
    (8, 6, 0, 1, 0): (16, 2562, 0, 3073, 0), (8, 6, 0, 1, 1): (512, 2562, 1, 3073, 1),
    (8, 6, 4, 1, 0): (16, 2562, 2, 3073, 2), (8, 6, 4, 1, 1): (512, 2562, 0, 3073, 0),
    (8, 7, 0, 1, 0): (16, 3074, 0, 3585, 0), (8, 7, 0, 1, 1): (512, 3074, 1, 3585, 1),
    (8, 7, 4, 1, 0): (16, 3074, 2, 3585, 2), (8, 7, 4, 1, 1): (512, 3074, 0, 3585, 0),
    (8, 8, 0, 1, 1): (16, 3586, 0, 4097, 0), (8, 8, 4, 1, 1): (16, 3586, 2, 4081, 2),
}


def wide_shape(n):
    """(W, CW) of the wide kernel at n samples (dispatch.h wide_geom)."""
    ns = n - 1
    W = 2 if ns <= 1024 else 4 if ns <= 2048 else 8
    return W, (ns + 64 * W - 1) // (64 * W)


def _family_a():
    out = []
    for inst, (N, n_lo, lw_lo, n_hi, lw_hi) in sorted(A_TABLE.items()):
        ends = [(n_lo, lw_lo)] + ([(n_hi, lw_hi)] if n_hi != n_lo else [])
        for n, lw in ends:
            tag = "W%dC%dE%ds%db%d-lw%d" % (inst + (lw,))
            out.append(_case("A", N, n, [wide(lw, inst[2] > 0)], inst=inst, tag=tag))
    return out


def _family_b():
    out = []
    for W in (2, 4, 8):
        for ns in (64 * W * 4 + 1, 64 * W * 5):
            out.append(_case("B", 65, ns + 1, [DIRECT, FFT]))
    # W = 8: wave 7 of each axis has no live lane at n − 1 = 2049 (above) .. 2240, one at 2241
    out += [_case("B", 65, ns + 1, [DIRECT, FFT]) for ns in (2240, 2241)]
    return out


def _family_c():
    out = [_case("C", 16, ns + 1, [CHUNK]) for ns in (513, 1024, 1025, 1087, 1088, 1089, 2048,
                                                      2049)]
    out += [_case("C", 16, ns + 1, [Opt(0, 0, False, "Chunk")]) for ns in (4097, 4160)]
    out += [_case("C", 1300, ns + 1, [CHUNK]) for ns in (1099, 2099)]
    out.append(_case("C", 4096, 2000, [Opt(0, 0, False, "Chunk")]))
    out.append(_case("C", 4096, 420, [Opt(0, 0, False, "Generic")]))
    return out


# family D: one wide shape per W and the chunk kernel, N = 65, five walks
D_SHAPES = ((700, (DIRECT, FFT)), (1500, (DIRECT, FFT)), (2300, (DIRECT, FFT)), (2301, (CHUNK,)))


def kick_placements(case):
    """→ (in-range launch-wide kick steps, out-of-range steps) of a family D case."""
    n = case.n
    if case.opts[0].kind == "Chunk":
        steps = [0, 15, 16, 1023, 1024, (n - 2) // 1024 * 1024, n - 2]
    else:
        W, CW = wide_shape(n)
        steps = [0, CW - 1, CW, 64 * CW - 1, 64 * CW, (W - 1) * 64 * CW, n - 2]
    steps = list(dict.fromkeys(steps))      # (W = 2: (W − 1)·64·CW is 64·CW)
    assert all(0 <= s <= n - 2 for s in steps)
    return steps, [-1, n - 1, n + 4]


def per_walk_kick_steps(case):
    """The same placements mixed over the walks of one launch: two launches' per-walk steps [B]
    (in-range and out-of-range steps side by side; the list repeats from its start to fill)."""
    steps, out = kick_placements(case)
    every = steps + out
    every += every[:2 * case.B - len(every)]
    assert len(every) == 2 * case.B
    return [np.array(every[0::2], np.int64), np.array(every[1::2], np.int64)]


def _family_d():
    return [_case("D", 65, n, opts, B=5) for n, opts in D_SHAPES]


# family E: one direct and one FFT instance per W (the FFT ones at CW >= 7 are the shuffle-scan
# variant), both correlation options
E_SHAPES = (900, 1700, 2300)


def _family_e():
    opts = [wide(lw, lw == 2, corr) for lw in (1, 2) for corr in (0, 1)]
    return [_case("E", 65, n, opts, B=6, gen="forms") for n in E_SHAPES]


def _family_f():
    out = []
    for N in (65, 129):
        for w in STABLE_POINTS:
            for n in (514, 1026, 2050):
                out.append(_case("F", N, n, [DIRECT, FFT] + ([CHUNK] if n == 1026 else []), w=w))
    return out


def _family_g():
    return [_case("G", 129, 1431, [DIRECT, FFT, CHUNK], offset=OFFSET)]


def _family_h():
    # B is set on the device: 2·(16/W)·CUs + 37 walks, arange(B) % 8 over eight distinct walks and
    # a ninth as the last (big_batch_index)
    return [_case("H", 65, n, [Opt(0, 0, False, "Wide")], B=9, gen="big") for n in (514, 1026)]


def big_batch_index(case, cus):
    W, _ = wide_shape(case.n)
    B = 2 * (16 // W) * cus + 37
    idx = np.arange(B) % 8
    idx[-1] = 8
    return idx


def _family_i():
    return [_case("I", 150, 1100, [DIRECT, FFT, CHUNK], B=5, gen="shared")]


# family J: per kernel family, six walks of which walk J_BAD gets a non-finite input
J_BAD = 3
J_FAMILIES = (("direct", "dense", DIRECT), ("fft", "dense", FFT), ("sparse", "sparse", DIRECT),
              ("chunk", "dense", CHUNK))
J_WHERE = ("x0", "bound-first", "bound-last", "bound-tail", "inf-pair")


def _family_j():
    return [_case("J", 65, 1500, [opt], B=6, gen=gen, tag=tag) for tag, gen, opt in J_FAMILIES]


def poison(case, rc, where):
    """A copy of the batch rc with walk J_BAD made non-finite at `where` (J_WHERE)."""
    n, b = case.n, J_BAD
    out = {key: np.array(v, copy=True) for key, v in rc.items()}
    if where == "x0":
        out["x0"][b, 0, 1] = np.nan
    elif where == "bound-first":
        out["zmax"][b, 0, 1] = np.nan
    elif where == "bound-last":
        out["zmin"][b, n - 1, 0] = np.nan
    elif where == "bound-tail":            # inside the last wave's range and the last chunk
        out["zmax"][b, n - 20, 0] = np.nan
    else:
        out["zmax"][b, n // 3, 1] = np.inf
        out["zmin"][b, n // 3, 1] = -np.inf
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = (_family_a() + _family_b() + _family_c() + _family_d() + _family_e() + _family_f() +
             _family_g() + _family_h() + _family_i() + _family_j())
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def family(letter):
    return [c for c in all_cases() if c.family == letter]


# ----------------------------------------------------------------------------- batches

def _piecewise(n, changes, steps):
    """[n] levels: z[m + 1] − z[m] = steps[i] at m = changes[i] (a change at m), else 0."""
    d = np.zeros(n)
    d[np.asarray(changes, int) + 1] = steps
    return np.cumsum(d)


def _random_changes(rng, n, count):
    m = np.sort(rng.permutation(np.arange(n - 1))[:count])
    s = rng.uniform(0.02, 0.1, count) * rng.choice([-1.0, 1.0], count)
    return m, s


def forms_changes(case, shift=0):
    """Family E: per walk and axis the z_ref changes (positions m, where z[m + 1] != z[m]), None
    for a random-walk axis.  shift moves walk 0's one y change by that many samples."""
    n, N = case.n, case.N
    W, CW = wide_shape(n)
    rng = np.random.default_rng([zlib.crc32(case.name.encode()), 99])
    r = lambda c: _random_changes(rng, n, c)
    one = (np.array([n // 2 + 3 + shift]), np.array([0.07]))
    i1, i2 = 64 * CW, max(W - 2, 1) * 64 * CW   # first outputs of wave 1 and of wave W − 2
    assert i2 + N <= n - 2
    sx = np.array([0, 64 * CW - 1, 64 * CW, n - 2])
    sy = np.unique([i1 + N - 1, i2 + N])
    return [(r(0), one), (r(63), r(64)), (r(64), r(65)), (r(65), r(0)), (r(5), None),
            ((sx, np.array([0.05, -0.08, 0.06, 0.04])), (sy, np.array([0.09, -0.05])[:len(sy)]))]


def _walk_centres(case, b, kind):
    """Bound centres [n, 2] of walk b: a random walk, or piecewise-constant levels of 5 to 9 runs
    per axis; the last row differs from the one before in both."""
    n = case.n
    rng = np.random.default_rng([zlib.crc32(case.name.encode()), n, b])
    zc = np.empty((n, 2))
    if kind == "dense":
        zc[:] = np.cumsum(rng.uniform(-0.01, 0.01, (n, 2)), axis=0)
        zc[-1] += rng.choice([-0.03, 0.03], 2)
    else:
        for a in range(2):
            m = np.sort(rng.permutation(np.arange(n - 2))[:int(rng.integers(4, 9))])
            m = np.concatenate([m, [n - 2]])
            zc[:, a] = _piecewise(n, m, rng.uniform(0.02, 0.1, len(m)) *
                                  rng.choice([-1.0, 1.0], len(m)))
    return zc


@functools.lru_cache(maxsize=None)
def _batch(case, shift):
    n, B = case.n, case.B
    if case.gen == "forms":
        zc = np.empty((B, n, 2))
        for b, axes in enumerate(forms_changes(case, shift)):
            for a, ch in enumerate(axes):
                if ch is None:
                    rng = np.random.default_rng([zlib.crc32(case.name.encode()), n, b, a])
                    zc[b, :, a] = np.cumsum(rng.uniform(-0.01, 0.01, n))
                else:
                    zc[b, :, a] = _piecewise(n, ch[0], ch[1])
    else:
        kinds = {"dense": ["dense"] * B, "sparse": ["sparse"] * B}.get(
            case.gen, ["dense" if b % 2 == 0 else "sparse" for b in range(B)])
        zc = np.stack([_walk_centres(case, b, kinds[b]) for b in range(B)])
    rng = np.random.default_rng([zlib.crc32(case.name.encode()), n, B])
    hi, lo = rng.uniform(0.01, 0.06, (2, B, 1, 2))      # asymmetric half-widths
    x0 = np.empty((B, 2, 3))
    x0[:, :, 0] = rng.uniform(-0.05, 0.05, (B, 2)) + case.offset
    x0[:, :, 1] = rng.uniform(-0.2, 0.2, (B, 2))
    x0[:, :, 2] = rng.uniform(-0.5, 0.5, (B, 2))
    kick = rng.uniform(0.02, 0.1, B) * rng.choice([-1.0, 1.0], B)
    ks = rng.integers(0, n - 1, B).astype(np.int64)
    zmax, zmin = zc + hi + case.offset, zc - lo + case.offset
    if case.gen == "shared":                            # one CoP for every walk
        zmax, zmin = zmax[0], zmin[0]
    for a in (zmax, zmin, x0, kick, ks):
        a.setflags(write=False)
    return dict(zmax=zmax, zmin=zmin, x0=x0, kick=kick, kick_step=ks)


def batch(case, shift=0):
    """The float64 inputs of a case: zmax, zmin [B, n, 2] ([n, 2] for a shared CoP), x0 [B, 2, 3],
    kick [B], kick_step [B] (read-only arrays, shared between callers)."""
    return _batch(case, shift)


def per_walk_bounds(case, rc):
    if rc["zmax"].ndim == 3:
        return rc["zmax"], rc["zmin"]
    return (np.broadcast_to(rc["zmax"], (case.B,) + rc["zmax"].shape),
            np.broadcast_to(rc["zmin"], (case.B,) + rc["zmin"].shape))


# ----------------------------------------------------------------------------- truth and bars

@functools.lru_cache(maxsize=16)
def _true_f(case, drop_tap=False, pad_row=-1, shift=0):
    k, _, _ = true_gain(case.N, case.w)
    if drop_tap:
        k = k.copy()
        k[-1] = 0
    zmax, zmin = per_walk_bounds(case, batch(case, shift))
    return correlate(z_ref(zmax, zmin, case.N, LD, pad_row), k, case.n)


def truth(case, kick_step=None, drop_tap=False, pad_row=-1, shift=0, kick_late=0):
    """The rollout of a case in np.longdouble with the true gain → [B, n, 2, 3]; kick_step
    replaces the batch's per-walk steps.  drop_tap, pad_row, shift and kick_late are the
    deliberate changes of the sensitivity conditions."""
    return _truth(case, None if kick_step is None else tuple(np.broadcast_to(
        np.asarray(kick_step, np.int64), (case.B,)).tolist()), drop_tap, pad_row, shift, kick_late)


@functools.lru_cache(maxsize=64)
def _truth(case, kick_step, drop_tap, pad_row, shift, kick_late):
    rc = batch(case, shift)
    _, _, h, g = POINTS[case.w]
    ks = np.asarray(rc["kick_step"] if kick_step is None else kick_step, np.int64) + kick_late
    hist = recursion(_true_f(case, drop_tap, pad_row, shift), rc["x0"], case_dt(case.N), h, g,
                     true_gain(case.N, case.w)[1], rc["kick"], ks)
    hist.setflags(write=False)
    return hist


def rel_err(hist, ref):
    """max |hist − ref| relative to max(1, max |ref|) over the whole history of the case."""
    ref = np.asarray(ref)
    return float(np.abs(np.asarray(hist, ref.dtype) - ref).max() /
                 max(LD(1), np.abs(ref).max()))


def _float64_oracle(case, rc):
    Q, R, h, g = POINTS[case.w]
    zmax, zmin = per_walk_bounds(case, rc)
    gain = numpy_gain(case.N, case.w)
    # (walk by walk: rollout_gain's window view times k is B·n·N doubles at once)
    return np.concatenate([O.rollout_gain(zmax[b:b + 1], zmin[b:b + 1], rc["x0"][b:b + 1], case.N,
                                          case_dt(case.N), h, g, Q, R, kick=rc["kick"][b:b + 1],
                                          kick_step=rc["kick_step"][b:b + 1], gain=gain)
                           for b in range(case.B)])


@functools.lru_cache(maxsize=None)
def e64(case):
    return rel_err(_float64_oracle(case, batch(case)), truth(case))


@functools.lru_cache(maxsize=None)
def efft64(case):
    rc = batch(case)
    _, _, h, g = POINTS[case.w]
    k, kx = numpy_gain(case.N, case.w)
    zmax, zmin = per_walk_bounds(case, rc)
    f = correlate_fft(z_ref(zmax, zmin, case.N, np.float64), k, case.n,
                      fft_period(case.N, case.n))
    return rel_err(recursion(f, rc["x0"], case_dt(case.N), h, g, kx, rc["kick"], rc["kick_step"]),
                   truth(case))


def bar(case, opt):
    """The bar of one launch of a case (the kick placement does not enter: family D's launches
    take the bar of the case's own per-walk steps)."""
    e = max(e64(case), efft64(case)) if opt.fft else e64(case)
    return max(BAR_FLOOR, BAR_FACTOR * e)
