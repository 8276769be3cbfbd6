"""The Python binding's checks, pinned: every bad call of tests/python_errors_cases.py raises
the exception type and the message, character for character, that the commit before the
checked-argument layer raised (tests/golden/python_errors.json, recorded there with the same
library), and the launchers keep alive and expose what they did then."""
import json
import os

import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

import python_errors_cases as ec  # noqa: E402

ROWS = ec.rows()
with open(os.path.join(GOLDEN, ec.FILE)) as _f:
    RECORD = json.load(_f)


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    c = ec.Context()
    yield c
    torch.cuda.synchronize()
    c.close()


def test_table_and_record_hold_the_same_rows():
    assert sorted(name for name, _ in ROWS) == sorted(RECORD["errors"])
    assert all(kind is not None for kind, _ in RECORD["errors"].values())


@pytest.mark.parametrize("name,fn", ROWS, ids=[name for name, _ in ROWS])
def test_bad_call_raises_what_it_raised(ctx, name, fn):
    got = ec.raised(fn, ctx)
    print(f"\n{name}: {got}")
    assert got == RECORD["errors"][name]


def test_launchers_keep_and_expose_what_they_did(ctx):
    launches = ec.launchers(ctx)
    assert sorted(launches) == sorted(RECORD["launchers"])
    for name, launch in launches.items():
        assert ec.launcher_record(launch) == RECORD["launchers"][name], name
        launch()
    # the ZmpcPush struct the arguments point to is the one held, and it points to the held
    # tensors; push_amp is the held amplitude tensor itself
    for name in ("rollout_launcher/push", "rollout_launcher/push_steps_profile",
                 "rollout_launcher/strict_push"):
        launch = launches[name]
        c, (amp, steps, prof) = launch.inputs[3], launch.inputs[4]
        assert launch.push_amp is amp and c.amp == amp.data_ptr(), name
        assert c.steps == (None if steps is None else steps.data_ptr()), name
        assert c.profile == (None if prof is None else prof.data_ptr()), name
    assert launches["rollout_launcher/kick"].push_amp is None
    assert launches["rollout_metrics_launcher"].metrics.shape == (ec.B, 12)


@pytest.mark.parametrize("name", ["rollout_launcher/push", "rollout_launcher/push_steps_profile",
                                  "rollout_launcher/strict_push"])
def test_push_amp_is_the_buffer_the_launch_reads(ctx, name):
    launch = ec.launchers(ctx)[name]
    launch()
    first = launch.hist.clone()
    launch()
    assert torch.equal(launch.hist, first)  # (the same launch writes the same history)
    launch.push_amp.mul_(3.0)
    launch()
    assert not torch.equal(launch.hist, first)
    assert torch.isfinite(launch.hist).all() and int(launch.status.abs().max()) == 0


def test_kick_is_the_buffer_the_launch_reads(ctx):
    for name in ("rollout_launcher/kick", "rollout_launcher/kick_steps"):
        launch = ec.launchers(ctx)[name]
        launch()
        first = launch.hist.clone()
        launch.inputs[3].mul_(3.0)
        launch()
        assert not torch.equal(launch.hist, first), name
    launch = ec.launchers(ctx)["rollout_metrics_launcher"]
    launch()
    first = launch.metrics.clone()
    launch.inputs[3].mul_(3.0)
    launch()
    assert not torch.equal(launch.metrics, first)
