"""The critical-force searches whose brackets are pinned bit for bit
(tests/golden/critical_bits.npz, written by tests/golden/make_critical_bits_golden.py from the
commit before the host side of the disturbances was merged into one path; compared by
tests/test_gpu_critical_bits.py): every disturbance form of critical_force on an unconstrained and
on a strict plan, and the shove and the trace of critical_force_herdt, at the smallest shapes that
take every branch — horizon 8, B = 3 walks of n = 24 samples with per-walk steps, 6 halvings, one
ragged case.  Not a test module."""
import hashlib

import numpy as np

import herdt_cases as hc

from mpc_bipedal.analysis import PushTrace
from mpc_bipedal.config import MPCConfig
from mpc_bipedal.controllers import ZMPController

FILE = "critical_bits.npz"
N, B, n, ITERS = 8, 3, 24, 6
STEPS = [9, 12, 15]
SIGNS = [1.0, -1.0, 1.0]
PLANAR = [[1.0, 0.0], [-1.0, 2.0], [0.5, -0.5]]
PROFILE = [0.5, 1.0, 0.25]
LENGTHS = [24, 19, 14]
L = 4
HERDT_DT = 0.07  # the coarse step of the short Herdt walks of tests/herdt_cases.py


def inputs():
    """→ zmax, zmin [B, n, 2], x0 [B, 2, 3], trace force [B, L, 2] in newtons, and of the Herdt
    walks v_ref [n, 2], states [n] int8 and x0 [B, 2, 3] (the CoM over the first foot)."""
    rng = np.random.default_rng(20261)
    centre = rng.uniform(-0.01, 0.01, (B, 1, 2)) + \
        0.02 * np.sign(np.sin(np.arange(n) * 0.7))[None, :, None] * np.array([0.0, 1.0])
    half = rng.uniform(0.05, 0.07, (B, 1, 2))
    zmax, zmin = centre + half, centre - half
    x0 = np.zeros((B, 2, 3))
    x0[:, :, 0] = rng.uniform(-2e-3, 2e-3, (B, 2))
    force = rng.uniform(-1.0, 1.0, (B, L, 2))
    states, v = hc.walk_schedule(n, 3, 1, 4, 2, vx=0.1)
    hx0 = x0.copy()
    hx0[:, 1, 0] += 0.1
    return zmax, zmin, x0, force, v, states, hx0


def inputs_hash():
    h = hashlib.sha256()
    for a in inputs():
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def forms():
    """name → keyword arguments of critical_force beside the bounds, x_init and iters."""
    force = inputs()[3]
    com = dict(max_com_dev=0.08, max_dcm_end=0.15)
    return {
        "kick": dict(force_step=STEPS, direction=SIGNS),
        "kick_criteria": dict(force_step=STEPS, direction=SIGNS, **com),
        "kick_ragged": dict(direction=SIGNS, walk_lengths=LENGTHS),
        "shove": dict(force_step=STEPS, direction=SIGNS, duration=3, profile=PROFILE, **com),
        "shove_one_step": dict(force_step=11, direction=-1, duration=3, profile=PROFILE),
        "planar": dict(force_step=STEPS, direction=PLANAR),
        "trace": dict(trace=PushTrace(force, np.array(STEPS)), F_hi=4000.0, **com),
    }


def herdt_forms():
    """name → keyword arguments of critical_force_herdt beside v_ref, state_ref, max_dcm_dev and
    iters."""
    force = inputs()[3]
    return {
        "herdt_shove": dict(force_step=STEPS, direction=SIGNS, duration=3, profile=PROFILE),
        "herdt_shove_ragged": dict(direction=PLANAR, duration=3, walk_lengths=LENGTHS),
        "herdt_trace": dict(trace=PushTrace(force, np.array(STEPS)), F_hi=4000.0),
    }


def run_all():
    """Every form → {"<plan>/<form>/<lo|hi>": [B] float64 array}."""
    zmax, zmin, x0, _, v, states, hx0 = inputs()
    out = {}

    def keep(name, bracket):
        for key, t in zip(("lo", "hi"), bracket):
            out[f"{name}/{key}"] = t.cpu().numpy()

    for plan, strict in (("unc", False), ("strict", True)):
        ctl = ZMPController(MPCConfig(horizon=N, strict=strict))
        for name, kw in forms().items():
            keep(f"{plan}/{name}", ctl.critical_force(zmax, zmin, x_init=x0, iters=ITERS, **kw))
    ctl = ZMPController(MPCConfig(horizon=N, strict=False))
    keep("unc/kick_fused", ctl.critical_force(zmax, zmin, x_init=x0, iters=ITERS, fused=True,
                                              force_step=STEPS, direction=SIGNS))
    ctl = ZMPController(MPCConfig(horizon=N, method="herdt", dt=HERDT_DT))
    vb = np.broadcast_to(v, (B, n, 2)).copy()
    sb = np.broadcast_to(states, (B, n)).copy()
    for name, kw in herdt_forms().items():
        keep(f"herdt/{name}", ctl.critical_force_herdt(vb, sb, 1.0, x_init=hx0, iters=ITERS,
                                                       **kw))
    return out
