"""The push-map calls whose results are pinned bit for bit (tests/golden/push_parent_bits.npz,
written by tests/golden/make_push_bits_golden.py from the library before the push kernels were
folded into one unit; compared by tests/test_gpu_push_bits.py).  Not a test module."""
import ctypes
import hashlib

import numpy as np
import torch

import push_map_cases as pc
import push_shaped_cases as ps

from mpc_bipedal import _native
from mpc_bipedal.analysis import AXES
from mpc_bipedal.solver import Plan

PAR = (150, 0.01, 0.75, 9.81, 1.0, 1e-6)
MASS = 40.0
T = 1e-9
NS = (3, 66, 130)  # one 64-step block, a block with its mirror, three blocks with a middle one
D_SHAPED = 5
FILE = "push_parent_bits.npz"


def inputs(n):
    """→ hist, zmax, zmin, lengths, steps of the n-sample case."""
    lengths = [n, max(n - 1, 1), max(n // 2, 1), max(n - 7, 1)]
    hist, zmax, zmin = pc.synthetic_case(n, False, 4, seed=1, lengths=lengths)
    steps = [0, lengths[1] - 3, -1, n // 3]
    return hist, zmax, zmin, np.array(lengths, np.int64), np.array(steps, np.int64)


def inputs_hash():
    h = hashlib.sha256()
    for n in NS:
        for a in inputs(n):
            h.update(np.ascontiguousarray(a).tobytes())
    h.update(ps.half_sine(D_SHAPED).tobytes())
    return h.hexdigest()


def forms():
    """name → (shaped call?, axes, D, profile, single-step?)"""
    out = {}
    for step in (False, True):
        sfx = "_step" if step else ""
        out["map" + sfx] = (False, "y", 1, None, step)
        for axes in ("x", "y", "xy"):
            out[f"shaped_{axes}_d1{sfx}"] = (True, axes, 1, None, step)
            out[f"shaped_{axes}_d{D_SHAPED}{sfx}"] = (True, axes, D_SHAPED,
                                                      ps.half_sine(D_SHAPED), step)
    return out


def run_all():
    """Every form at every n on the loaded library → {"n<n>/<form>/<force|limit|response>": array},
    straight through ctypes into buffers filled with −7."""
    lib = _native.load()
    plan = Plan(torch.cuda.current_device(), *PAR, False)
    dev = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device="cuda").contiguous()  # noqa: E731
    vp = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())  # noqa: E731
    out = {}
    for n in NS:
        hist, zmax, zmin, lengths, steps = inputs(n)
        B = hist.shape[0]
        h, zx, zn = dev(hist), dev(zmax), dev(zmin)
        len_t, st_t = dev(lengths, torch.int64), dev(steps, torch.int64)
        for name, (shaped, axes, D, w, step) in forms().items():
            C = 4 if axes == "xy" else 2
            shape = (B, C) if step else (B, n, C)
            force = torch.full(shape, -7.0, dtype=torch.float64, device="cuda")
            limit = torch.full(shape, -7, dtype=torch.int32, device="cuda")
            resp = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
            w_t = None if w is None else dev(w)
            head = (plan.handle, B, n, vp(h), vp(zx), vp(zn), 2 * n, vp(len_t),
                    vp(st_t) if step else None)
            tail = (T, MASS, vp(force), vp(limit), vp(resp),
                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            if shaped:
                rc = lib.zmpc_push_map_shaped(*head, vp(w_t), D, AXES[axes], *tail)
            else:
                rc = lib.zmpc_push_map(*head, *tail)
            _native.check(rc, name)
            torch.cuda.synchronize()
            for key, t in (("force", force), ("limit", limit), ("response", resp)):
                out[f"n{n}/{name}/{key}"] = t.cpu().numpy()
    return out
