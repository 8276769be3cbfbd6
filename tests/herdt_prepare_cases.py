"""Seeded support schedules for zmpc_herdt_prepare and their host answers (not a test module):
shared by the host, emulation and device tests of the device-side footstep bookkeeping.

The host answer for walk b is the product's own drop-in bookkeeping, herdt.find_nb_steps and
herdt.max_footsteps, on states[b, :n_b] followed by N copies of its last live state — the
restatement tests/test_herdt_host.py pins to the reference and the oracle — so the walk alone
decides it, never the batch it sits in."""
import functools
import os

import numpy as np

from mpc_bipedal.controllers import herdt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

B = 37
SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 359)
HORIZONS = (1, 2, 17, 64, 150)
# lengths None; per-walk lengths with the rows past n_b filled with the producer's −1; the same
# with a valid alternating DOUBLE, SINGLE pattern there, so that reading them changes the answer
VARIANTS = ("full", "ragged_pad", "ragged_alt")
SHAPES = [(n, N) for n in SIZES for N in HORIZONS]


def default_states():
    """The reference's default schedule (302 samples, int8 codes)."""
    return np.load(os.path.join(GOLDEN, "herdt_default.npz"))["states"].astype(np.int8)


def _runs(rng, n, lo, hi, last):
    """n samples in runs of lo..hi samples, the three states in any order, ending in `last`
    (None: wherever it ends)."""
    out = []
    while len(out) < n:
        out += [int(rng.integers(0, 3))] * int(rng.integers(lo, hi + 1))
    s = np.array(out[:n], np.int8)
    if last is not None:
        k = n - 1  # the final run takes the wanted state
        while k > 0 and s[k - 1] == s[n - 1]:
            k -= 1
        s[k:] = last
    return s


def schedule(rng, n, b):
    """Walk b of a batch: short runs, long runs that cross chunk edges, a mix, ending in each of
    the three states in turn; all standing; gait-like (STANDING, then DOUBLE ⇄ SINGLE, then
    STANDING)."""
    kind = b % 6
    last = (b // 6) % 3 if b % 2 else None
    if kind == 0:
        return _runs(rng, n, 1, 5, last)
    if kind == 1:
        return _runs(rng, n, 60, 70, last)
    if kind == 2:
        s = _runs(rng, n, 1, 5, None)
        long = _runs(rng, n, 60, 70, None)
        cut = int(rng.integers(0, n + 1))
        s[cut:] = long[cut:]
        return s
    if kind == 3:
        return _runs(rng, n, 1, 70, last)
    if kind == 4:
        return np.zeros(n, np.int8)
    lead, tail = int(rng.integers(0, 9)), int(rng.integers(0, 9))
    ds, ss = int(rng.integers(1, 8)), int(rng.integers(1, 30))
    body = ([herdt.DOUBLE_SUPPORT] * ds + [herdt.SINGLE_SUPPORT] * ss) * (n // (ds + ss) + 1)
    s = np.array(([herdt.STANDING] * lead + body)[:n], np.int8)
    if tail and tail < n:
        s[n - tail:] = herdt.STANDING
    return s


def _lengths(rng, n):
    """Per-walk lengths: 1, 2, n − 1 and n, then 0 and n + 5 (which must clamp), then random."""
    fixed = [1, 2, n - 1, n, 0, n + 5, -3, 2 * n + 64]
    return np.array(fixed + [int(rng.integers(1, n + 1)) for _ in range(B - len(fixed))], np.int64)


def answer(states, lengths, N):
    """The host answer: (states_out [B, n] int8, nb_next [B, n] int32, max_steps [B] int32)."""
    states = np.atleast_2d(states)
    Bn, n = states.shape
    clean = np.empty((Bn, n), np.int8)
    nb = np.ones((Bn, n), np.int32)
    steps = np.empty(Bn, np.int32)
    for b in range(Bn):
        nl = n if lengths is None else int(min(max(int(lengths[b]), 1), n))
        live = states[b, :nl]
        pad = np.concatenate([live, np.repeat(live[-1:], N)])
        clean[b] = np.concatenate([live, np.repeat(live[-1:], n - nl)])
        nb[b, :nl] = [t[0] for t in herdt.find_nb_steps(pad)][:nl]
        steps[b] = herdt.max_footsteps(pad[None], N, nl)
    return clean, nb, steps


@functools.lru_cache(maxsize=None)
def case(n, N, variant):
    """One batch of B walks: dict(n, N, states [B, n] int8, lengths [B] int64 or None, and the host
    answers want_states, want_nb, want_steps, want_most)."""
    # (the two ragged variants share their schedules and lengths: only the fill differs)
    rng = np.random.default_rng([n, N, int(variant != "full"), 20251])
    states = np.stack([schedule(rng, n, b) for b in range(B)])
    lengths = None
    if n >= 302:  # the reference's default walk inside a longer batch
        states[0, :302] = default_states()
    if variant != "full":
        lengths = _lengths(rng, n)
        if n >= 302:
            lengths[0] = 302
            lengths[1] = n
        live = np.clip(lengths, 1, n)
        for b in range(B):
            k = np.arange(n - live[b])
            states[b, live[b]:] = -1 if variant == "ragged_pad" else 1 + (k & 1)
    clean, nb, steps = answer(states, lengths, N)
    for a in (states, clean, nb, steps):
        a.setflags(write=False)
    if lengths is not None:
        lengths.setflags(write=False)
    return dict(n=n, N=N, states=states, lengths=lengths, want_states=clean, want_nb=nb,
                want_steps=steps, want_most=int(steps.max()))


def padded_to_batch(states, lengths, N):
    """The other rule, which the call must not follow: every walk padded with its last live state
    to the batch's n first, then treated as an n-sample walk (what the host route does to a
    rectangular batch)."""
    states = np.atleast_2d(states)
    n = states.shape[1]
    live = np.clip(lengths, 1, n)
    filled = np.stack([np.concatenate([s[:k], np.repeat(s[k - 1:k], n - k)])
                       for s, k in zip(states, live)])
    return answer(filled, None, N)
