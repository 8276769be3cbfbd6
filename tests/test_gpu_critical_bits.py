"""critical_force and critical_force_herdt against the brackets of the commit before the host
side of the disturbances was merged into one path (tests/golden/critical_bits.npz): every form of
tests/critical_bits_cases.py — a sign kick, a shaped shove, planar directions and a trace, on an
unconstrained and on a strict plan, and a shove and a trace on Herdt walks — bit for bit.  The
kernels and their launch arguments are the same on both sides, so the arithmetic is too: equality
is the bar, NaN and inf compared as patterns."""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

import critical_bits_cases as cb  # noqa: E402


def same(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    nan = torch.isnan(a)
    zero = torch.zeros_like(a)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(nan, torch.isnan(b)) and \
        torch.equal(torch.where(nan, zero, a), torch.where(nan, zero, b))


def test_brackets_equal_parent_bits():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    ref = golden(cb.FILE)
    assert str(ref["inputs_sha256"]) == cb.inputs_hash(), \
        "the generator of the inputs changed, not the searches"
    got = cb.run_all()
    assert set(got) == set(ref.files) - {"inputs_sha256"}
    assert len(got) == 2 * (2 * len(cb.forms()) + 1 + len(cb.herdt_forms()))
    for k in sorted(got):
        print(k, got[k].tolist())
    diff = [k for k in sorted(got) if not same(got[k], np.asarray(ref[k]))]
    assert not diff, diff
