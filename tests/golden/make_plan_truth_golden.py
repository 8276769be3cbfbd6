"""Writes tests/golden/plan_truth.npz: the plan-build cases of tests/plan_cases.py solved with
mpmath at 60 digits and rounded to float64 (plan_cases.rounded: the vectors k, kx (as three
doubles), v and the suffix sums, rows of L, X, G and Hz, the sampled gain spectra), plus the first
octant of the FFT twiddles.  Inputs are regenerated from the case names and are not stored.

The R = 0 case is stored only if the float64 reference alone is within plan_cases.KEEP_BAR of its
truth on k and kx; its two distances are stored either way (r0_eref).

Run from the repository root (needs mpmath; about two minutes on 16 cores):
    python tests/golden/make_plan_truth_golden.py
"""
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import plan_cases as PC  # noqa: E402
from oracle import zmp_oracle as O  # noqa: E402


def solve(case):
    return case[0], PC.rounded(PC.truth(case))


def main():
    cases = sorted(PC.CASES + (PC.R0_CASE,), key=lambda c: -c[1])
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        solved = dict(pool.imap_unordered(solve, cases, chunksize=1))
    _, N, (Q, R, h, g) = PC.R0_CASE
    k, kx = O.gain_row(N, PC.case_dt(N), h, g, Q, R)
    t = solved[PC.R0_CASE[0]]
    r0 = np.array([PC._rel(k, t["k"]), PC._rel(kx, t["kx"])])
    keep_r0 = bool(np.all(np.isfinite(r0)) and r0.max() <= PC.KEEP_BAR)
    print(f"R = 0 at N = {N}: reference k {r0[0]:.2e}, kx {r0[1]:.2e} from truth ->",
          "kept" if keep_r0 else "dropped")
    names = [c[0] for c in PC.CASES] + ([PC.R0_CASE[0]] if keep_r0 else [])
    out = {"names": np.array(names), "r0_eref": r0, "tw_octant": PC.twiddle_octant_truth()}
    for name in names:
        for key, a in solved[name].items():
            out[f"{name}/{key}"] = a
    np.savez_compressed(PC.TRUTH_FILE, **out)
    print(PC.TRUTH_FILE, os.path.getsize(PC.TRUTH_FILE), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
