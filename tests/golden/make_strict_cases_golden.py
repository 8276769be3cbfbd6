"""Stored exact-oracle answers for the strict cases at the long horizons →
tests/golden/strict_cases.npz.

The exact box-QP oracle (oracle/zmp_oracle.py) takes seconds per solve at the longest horizons,
too long for a device test, so its answers are kept: the cold `pinned` windows of
tests/strict_cases.lq_case at N >= 1600 (three doubles per answer, with the working-set size and
the KKT residuals of each batch), and the six-sample rollouts of lq_rollout_case at N <= 897,
whose first solves pin up to 150 slots.  The inputs are not stored: the tests regenerate them
from the case names (the seeds) and check a stored answer against a fresh solve.  Oracle only:
nothing of the reference controller is imported.

    python tests/golden/make_strict_cases_golden.py        # CPU; about a minute
"""
import multiprocessing
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import strict_cases as SC  # noqa: E402

KKT_KEYS = ("primal", "stationarity", "dual_hi", "dual_lo")


def _job(key):
    kind, N = key
    if kind == "step":
        xn, m, worst = SC.solve_windows(SC.lq_case(N))
        return {f"step{N}_out": xn, f"step{N}_m": m.astype(np.int32),
                f"step{N}_kkt": np.array([worst[k] for k in KKT_KEYS])}
    case = SC.lq_rollout_case(N)
    hist, worst = [], dict.fromkeys(KKT_KEYS, 0.0)
    for b in range(len(case["kick"])):
        h, kkt = SC.oracle_walk(case, b, return_kkt=True)
        hist.append(h)
        worst = {k: max(worst[k], kkt[k]) for k in KKT_KEYS}
    return {f"roll{N}_hist": np.stack(hist),
            f"roll{N}_kkt": np.array([worst[k] for k in KKT_KEYS])}


def main():
    keys = [("step", N) for N in SC.LQ_HORIZONS if N > SC.LQ_LIVE_MAX] + \
           [("roll", N) for N in SC.LQ_HORIZONS if N <= SC.LQ_LIVE_MAX]
    out = {"kkt_keys": np.array(KKT_KEYS)}
    names = []
    with ProcessPoolExecutor(max_workers=min(4, os.cpu_count() or 1),
                             mp_context=multiprocessing.get_context("spawn")) as ex:
        for key, res in zip(keys, ex.map(_job, keys)):
            out.update(res)
            names.append(f"{key[0]}{key[1]}")
            print(key, {k: (v if v.size <= 4 else v.shape) for k, v in res.items()})
    out["names"] = np.array(names)
    out["seeds"] = np.array([SC.seed_of(f"pinned-lq-N{N}-m{m}") if kind == "step" else
                             SC.seed_of(f"pinned-lq-rollout-N{N}-n6")
                             for kind, N in keys for m in (SC.LQ_M if kind == "step" else (0,))],
                            np.int64)
    np.savez_compressed(os.path.join(HERE, "strict_cases.npz"), **out)


if __name__ == "__main__":
    main()
