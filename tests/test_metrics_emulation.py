"""CPU check of the walk-metrics kernel's wave logic (csrc/metrics.hip): its kernel source,
compiled for the host against tests/emu's emulation of the HIP wave facilities (64 lanes as
coroutines, lockstep at every shuffle), against the NumPy statement of the metrics on the seeded
cases of the device tests.  Catches index, tie-break and reduction errors before a GPU run; what
only the hardware decides stays with the -m gpu tests."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from metrics_cases import HG, assert_metrics, random_case
from mpc_bipedal.analysis import walk_metrics_reference

CSRC = os.path.join(ROOT, "model-predictive-control-for-bipedal-locomotion_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu")


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    d = tmp_path_factory.mktemp("metrics_emu")
    src = open(os.path.join(CSRC, "metrics.hip")).read()
    body = src[:src.index("hipError_t zmpc_launch_walk_metrics(")]
    body = body.replace("namespace {\n", "namespace emu {\n", 1)
    assert body.rstrip().endswith("}  // namespace")
    (d / "metrics_kernel_emu.h").write_text(body)
    exe = d / "metrics_emu"
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", f"-I{EMU}", f"-I{d}",
                    f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}", "-o", str(exe),
                    os.path.join(EMU, "metrics_emu.cpp")], check=True, capture_output=True)
    return d, exe


def _run(emulator, hist, zmax, zmin, lengths=None):
    d, exe = emulator
    B, n = hist.shape[:2]
    inp = d / "in.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<qqqqd", B, n, 0 if zmax.ndim == 2 else 2 * n,
                            int(lengths is not None), HG))
        for a in (hist, zmax, zmin):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
        if lengths is not None:
            f.write(np.asarray(lengths, np.int64).tobytes())
    r = subprocess.run([str(exe), str(inp)], capture_output=True, check=True, timeout=120)
    return np.frombuffer(r.stdout, np.float64).reshape(B, 12)


@pytest.mark.parametrize("shared", (False, True))
@pytest.mark.parametrize("n", (1, 64, 65, 129))
def test_metrics_kernel_emulated_random(emulator, n, shared):
    hist, zmax, zmin = random_case(n, shared, B=5)
    assert_metrics(_run(emulator, hist, zmax, zmin), walk_metrics_reference(hist, zmax, zmin, HG))


def test_metrics_kernel_emulated_ragged_ties_and_non_finite(emulator):
    n = 129
    hist, zmax, zmin = random_case(n, False, B=6)
    lengths = np.array([1, 64, 65, 129, 100, 129])
    for b, nb in enumerate(lengths):  # dead tails never reach a result
        hist[b, nb:], zmax[b, nb:], zmin[b, nb:] = np.nan, 1e300, np.nan
    # walk 3: no violation at all; walk 4: the largest violation twice, in two lanes (63, 64)
    zmax[3], zmin[3] = 10.0, -10.0
    hist[4, 63] = hist[4, 64] = [[5.0, 0.0, 0.0], [-5.0, 0.0, 0.0]]
    zmax[4, 63], zmin[4, 63] = zmax[4, 64], zmin[4, 64]
    hist[5, 70, 1, 1] = np.nan  # walk 5: the y axis meets a NaN velocity at sample 70
    got = _run(emulator, hist, zmax, zmin, lengths)
    assert_metrics(got, walk_metrics_reference(hist, zmax, zmin, HG, lengths))
    assert got[3, :6].tolist() == [0.0, 0.0, -1.0, -1.0, 0.0, 0.0]
    assert got[4, 2:4].tolist() == [63.0, 63.0]
    assert got[5, 1] == np.inf and got[5, 3] == 70.0 and np.isnan(got[5, 5::2]).all()
    assert np.isfinite(got[5, 0::2]).all()
