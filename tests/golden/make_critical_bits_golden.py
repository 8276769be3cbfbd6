"""Writes tests/golden/critical_bits.npz: the brackets (F_lo, F_hi) of every critical-force search
of tests/critical_bits_cases.py, from whichever mpc_bipedal package comes first on the path and
its library (the commit whose results are to be pinned: a PYTHONPATH entry wins over the package
in the tree), and a SHA-256 of the regenerated inputs.  Needs a HIP device.

    PYTHONPATH=/path/to/parent/model-predictive-control-for-bipedal-locomotion_amd \\
    python tests/golden/make_critical_bits_golden.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "model-predictive-control-for-bipedal-locomotion_amd"),
          os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.append(p)

import torch  # noqa: E402

import critical_bits_cases as cb  # noqa: E402


def main():
    if not torch.cuda.is_available():
        raise SystemExit("make_critical_bits_golden.py needs a HIP device")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, cb.FILE)
    arrays = cb.run_all()
    for k in sorted(arrays):
        print(k, arrays[k].tolist())
    arrays["inputs_sha256"] = np.array(cb.inputs_hash())
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print(f"{out}: {len(arrays)} arrays, {os.path.getsize(out)} bytes, from "
          f"{sys.modules[cb.ZMPController.__module__].__file__}")


if __name__ == "__main__":
    main()
