"""The trace margin (zmpc_trace_margin) timed beside what it replaces and its yardstick.

    timeout -k 10 300 python scripts/trace_margin_ab.py --out profiles/tracemargin

Shapes: bench.py's config 2 (4096 walks x 420 samples, N = 150, per-walk bounds) and one walk of
420 samples.  Forms, alternating round by round in one process (HIP events around back-to-back
calls on prepared arguments, every round's time recorded; 5 rounds x 100 launches, the bisection
10 per round):
  unpushed     zmpc_rollout without a kick
  margin_k1    zmpc_trace_margin, one draw per walk: B rows, dense noise on xy from step 0
  margin_k16   zmpc_trace_margin, 16 draws per walk over the same number of rows (4096 x 420: 256
               walks x 16 draws; 1 x 420: the one walk's 16 draws, 16 rows)
  traced       zmpc_rollout_traced on the same rows; `trace_add` = traced − unpushed is what the
               trace kernel adds to the rollout: the yardstick
  bisect30     ZMPController.critical_force(trace=, iters=30) on the same rows: 32 evaluations of
               a traced rollout, walk_metrics and the bracket update
The record holds medians with round ranges and the ratio bisect30 / (unpushed + margin_k1).
Reads no file outside the tree.  Needs a HIP device: there is no CPU path."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "model-predictive-control-for-bipedal-locomotion_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from mpc_bipedal import _native  # noqa: E402
from mpc_bipedal.analysis import PushTrace  # noqa: E402
from mpc_bipedal.config import MPCConfig  # noqa: E402
from mpc_bipedal.controllers import ZMPController  # noqa: E402
from mpc_bipedal.generators import CoPGenerator  # noqa: E402

SEED = 20261021
DRAWS = 16


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def forms_of(lib, ctl, B, keep):
    cfg = ctl.config
    plan = ctl._plan()
    zmax, zmin, _ = CoPGenerator(cfg).generate_cop_trajectory()
    n = len(zmax)
    rng = np.random.default_rng([SEED, B])
    off = rng.uniform(-0.02, 0.02, (B, 1, 2))
    f64 = dict(dtype=torch.float64, device="cuda")
    zx, zn = torch.as_tensor(zmax[None] + off, **f64), torch.as_tensor(zmin[None] + off, **f64)
    x0 = torch.zeros((B, 2, 3), **f64)
    Bk = max(B // DRAWS, 1)          # walks of the 16-draw form
    R16 = Bk * DRAWS
    rows = max(B, R16)
    dv = torch.as_tensor(0.002 * rng.standard_normal((rows, n - 1, 2)), **f64)
    hist = torch.empty((B, n, 2, 3), **f64)
    hist0, _ = plan.rollout(zx, zn, x0)  # the unpushed history the margins read
    status = torch.empty(B, dtype=torch.int32, device="cuda")
    scale = torch.empty((rows, 2), **f64)
    limit = torch.empty((rows, 2), dtype=torch.int32, device="cuda")
    tr = _native.ZmpcTrace(dv.data_ptr(), 3, None, 0, n - 1, None)
    keep += [zx, zn, x0, dv, hist, hist0, status, scale, limit, tr]
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    walks = (plan.handle, B, n, vp(zx), vp(zn), 2 * n, vp(x0))

    def unpushed():
        rc = lib.zmpc_rollout(*walks, None, -1, vp(hist), vp(status), ctypes.c_void_p(stream()))
        assert rc == 0, lib.zmpc_last_error()

    def traced():
        tr.stream = stream()
        rc = lib.zmpc_rollout_traced(*walks, ctypes.addressof(tr), vp(hist), vp(status))
        assert rc == 0, lib.zmpc_last_error()

    def margin(walks_, draws):
        def run():
            tr.stream = stream()
            rc = lib.zmpc_trace_margin(plan.handle, walks_, n, vp(hist0), vp(zx), vp(zn), 2 * n,
                                       None, draws, ctypes.addressof(tr), 1e-9, vp(scale),
                                       vp(limit))
            assert rc == 0, lib.zmpc_last_error()
        return run

    trace = PushTrace.from_velocity_steps(dv[:B], 0, "xy")

    def bisect():
        ctl.critical_force(zx, zn, x_init=x0, trace=trace, iters=30)

    return {"unpushed": unpushed, "margin_k1": margin(B, 1), "margin_k16": margin(Bk, DRAWS),
            "traced": traced, "bisect30": bisect}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--batches", default="4096,1", help="the shapes' walk counts (a profiler run "
                    "of its own takes one: its kernel statistics are then that shape's)")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if not torch.cuda.is_available():
        raise SystemExit("trace_margin_ab.py needs a HIP device (no CPU path)")
    lib = _native.load()
    ctl = ZMPController(MPCConfig(horizon=150, strict=False))
    keep, rec = [], {"rounds": args.rounds, "launches_per_round": args.launches,
                     "bisect30_launches_per_round": max(args.launches // 10, 1), "shapes": {}}
    for B in (int(b) for b in args.batches.split(",")):
        forms = forms_of(lib, ctl, B, keep)
        for fn in forms.values():  # warm-up of every form the timed window uses
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                reps = args.launches if k != "bisect30" else max(args.launches // 10, 1)
                ms[k].append(timed(fn, reps))
        torch.cuda.synchronize()
        med = {k: float(np.median(v)) for k, v in ms.items()}
        shape = {"ms_rounds": ms,
                 "ms": {k: {"median": med[k], "min": min(v), "max": max(v)}
                        for k, v in ms.items()},
                 "trace_add_ms": med["traced"] - med["unpushed"],
                 "bisect30_over_unpushed_plus_margin_k1":
                     med["bisect30"] / (med["unpushed"] + med["margin_k1"])}
        rec["shapes"][f"{B}x420"] = shape
        print(f"{B}x420", json.dumps(shape["ms"]), "trace_add", shape["trace_add_ms"], "ratio",
              shape["bisect30_over_unpushed_plus_margin_k1"], flush=True)
    with open(os.path.join(args.out, "trace_margin_ab.json"), "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
