"""One-off check for the strict.hip clean-up that took PhaseClock, StrictArgs::dbg and
StrictArgs::lds_chol out of the reduced-Cholesky kernels (their argument layout, and so their
machine code, changed; their arithmetic must not have).

    ZMPC_LIB=<library> python scripts/strict_chol_bitcompare.py dump OUT.npz
    python scripts/strict_chol_bitcompare.py compare PARENT.npz TREE.npz

`dump` runs solvers 1 (tile kernel) and 2 (wave kernel) of the library ZMPC_LIB names (default:
the tree's) at N = 33, 64, 150 and 512 on tests/strict_cases.py's four rollout families (6 walks
of 40 samples) and on cold pinned windows (N = 150, 512: chol_case, every reduced-solve branch;
N = 33, 64: the same construction at m = 0, 1, N/4, N/2, N/2 + 1, N − 1, N), and stores every
hist / x_next and status.  `compare` demands the two files be equal bit for bit, array by array;
exit status 1 otherwise.  One process per library.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"),
          os.path.join(ROOT, "model-predictive-control-for-bipedal-locomotion_amd")):
    sys.path.insert(0, p)

HORIZONS = (33, 64, 150, 512)


def windows(SC, N):
    if N in SC.CHOL_M:
        return SC.chol_case(N)
    ms = sorted({0, 1, N // 4, N // 2, N // 2 + 1, N - 1, N})
    wins = []
    for i, m in enumerate(ms):
        name = f"bitcompare-chol-N{N}-m{m}-{i}"
        wins.append(SC.pinned_window(name, N, SC.chol_positions(N, m, SC._rng(name, 1))))
    return SC._windows(wins, ms, N)


def dump(out):
    import torch
    import strict_cases as SC
    from mpc_bipedal.solver import Plan
    from mpc_bipedal import _native

    Q, R, h = SC.WEIGHTS[0]
    arrays = {}
    for N in HORIZONS:
        win = windows(SC, N)
        for dt, kind in ((SC.case_dt(N), "roll"), (win["dt"], "step")):
            p = Plan(torch.cuda.current_device(), N, dt, h, SC.G, Q, R, True)
            try:
                for solver in (1, 2):
                    p.set_option("strict_solver", solver)
                    if kind == "step":
                        x, st = p.step(win["x"], win["zmax"], win["zmin"])
                        arrays[f"step_N{N}_s{solver}_x"] = x.cpu().numpy()
                        arrays[f"step_N{N}_s{solver}_status"] = st.cpu().numpy()
                        continue
                    for family in SC.FAMILIES:
                        c = SC.rollout_case(family, N)
                        assert c["dt"] == dt
                        hist, st = p.rollout(c["zmax"], c["zmin"], c["x0"], kick=c["kick"],
                                             kick_step=c["kick_step"])
                        arrays[f"roll_{family}_N{N}_s{solver}_hist"] = hist.cpu().numpy()
                        arrays[f"roll_{family}_N{N}_s{solver}_status"] = st.cpu().numpy()
            finally:
                p.destroy()
        print(f"N={N} done", flush=True)
    np.savez(out, **arrays)
    print(f"{_native.LIB_PATH}: {len(arrays)} arrays -> {out}")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for k in sorted(set(A.files) & set(B.files)):
        same = A[k].shape == B[k].shape and A[k].tobytes() == B[k].tobytes()
        flagged = k.endswith("status") and bool(A[k].any())
        print(f"{k}: {'identical' if same else 'DIFFERS'}{' (nonzero status)' if flagged else ''}")
        if not same:
            bad.append(k)
    print(f"{len(A.files)} arrays, {len(bad)} differing or one-sided")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
