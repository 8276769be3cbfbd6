"""Both push-map calls against the results of the library before their kernels were folded into
one unit (tests/golden/push_parent_bits.npz): every form of tests/push_bits_cases.py, force,
limit and response, bit for bit.  The suite's other anchors compare the kernels with each other;
this one cannot pass on a changed arithmetic order, a changed tie rule or a wrong column."""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

import push_bits_cases as bc  # noqa: E402


def bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def test_push_maps_equal_parent_bits():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    ref = golden(bc.FILE)
    assert str(ref["inputs_sha256"]) == bc.inputs_hash(), \
        "the generator of the inputs changed, not the kernels"
    got = bc.run_all()
    assert set(got) == set(ref.files) - {"inputs_sha256"}
    assert len(got) == 3 * len(bc.NS) * 14
    diff = [k for k in sorted(got)
            if got[k].shape != ref[k].shape or got[k].dtype != ref[k].dtype
            or not np.array_equal(bits(got[k]), bits(ref[k]))]
    assert not diff, diff
