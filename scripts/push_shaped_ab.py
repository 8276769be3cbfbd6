"""Shaped and two-axis push maps (zmpc_push_map_shaped) against zmpc_push_map, in one process.

    timeout -k 10 600 python scripts/push_shaped_ab.py --out profiles/pushshaped --only config2 && \
    timeout -k 10 300 python scripts/push_shaped_ab.py --out profiles/pushshaped --only b1

(each shape is one GPU step under a time limit of its own; chain them with &&.)

Forms, alternating round by round on one unpushed history of the reference's default walk (420
CoP samples, N = 150, per-walk bounds at rigid offsets, max_violation 5 cm so that every walk
passes the nominal test, as scripts/push_map_ab.py); HIP events around back-to-back ctypes calls
on prepared arguments, every round's time recorded:
  map_y            zmpc_push_map, unchanged: the yardstick
  shaped_y_d1/d20  zmpc_push_map_shaped, axes = y, D = 1 / 20: the same map kernel on the shaped
                   table, plus the shaping kernel                                  (a) vs map_y
  shaped_x_d1      axes = x: the new one-axis kernel
  shaped_xy_d1/d20 axes = x | y: both axes in turn in one launch                   (b) vs shaped_y
  flip_route       today's only route to the x and y tables at D = 1: zmpc_push_map on y,
                   axis-flipped copies of the history and the bounds, zmpc_push_map again
                                                                                   (c) vs shaped_xy_d1
  step_y           zmpc_push_map, single-step form at push_steps = n // 2 of every walk
  step_x, step_xy  zmpc_push_map_shaped, axes = x / x | y, D = 1: the same single step

Against another build of the library (it is named by ZMPC_LIB, one process per build and shape,
in alternation, each into a directory of its own), then without a device:

    python scripts/push_shaped_ab.py --out profiles/pushunit \
        --compare-parent p1,p2,p3 --compare-new n1,n2,n3

writes ab_vs_parent.json: per shape and form the median over processes of the per-process
medians, the parent's own spread (largest − smallest of its process medians) / smallest, the
ratio new / parent, and whether the ratio stays within 1 + spread.
Shapes: config2 4096 walks, b1 one walk.  Reads no file outside the tree.  Needs a HIP device:
there is no CPU path."""
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
from mpc_bipedal.config import MPCConfig  # noqa: E402
from mpc_bipedal.controllers import ZMPController  # noqa: E402

SEED = 20261020
T_VIOL = 0.05


def timed(fn, launches):
    """ms per call of `launches` back-to-back calls (HIP events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def summary(ms):
    return {k: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in ms.items()}


def shape_record(name, c, zmax, zmin, B, rounds, launches, rng):
    cfg, plan = c.config, c._plan()
    n = zmax.shape[0]
    f64 = dict(dtype=torch.float64, device="cuda")
    off = rng.uniform(-0.02, 0.02, (B, 1, 2))
    x0 = np.zeros((B, 2, 3))
    x0[:, :, 0] = rng.uniform(-0.01, 0.01, (B, 2))
    zx, zn = torch.as_tensor(zmax[None] + off, **f64), torch.as_tensor(zmin[None] + off, **f64)
    hist, _ = plan.rollout(zx, zn, torch.as_tensor(x0, **f64))
    lib, vp = _native.load(), ctypes.c_void_p
    f2 = torch.empty((B, n, 2), **f64)
    l2 = torch.empty((B, n, 2), dtype=torch.int32, device="cuda")
    f2b, l2b = torch.empty_like(f2), torch.empty_like(l2)
    f4 = torch.empty((B, n, 4), **f64)
    l4 = torch.empty((B, n, 4), dtype=torch.int32, device="cuda")
    hist_f, zx_f, zn_f = torch.empty_like(hist), torch.empty_like(zx), torch.empty_like(zn)

    def stream():
        return vp(torch.cuda.current_stream().cuda_stream)

    steps = torch.full((B,), n // 2, dtype=torch.int64, device="cuda")
    fs2, ls2 = torch.empty((B, 2), **f64), torch.empty((B, 2), dtype=torch.int32, device="cuda")
    fs4, ls4 = torch.empty((B, 4), **f64), torch.empty((B, 4), dtype=torch.int32, device="cuda")

    def old(h, hi, lo, f, l, st=None):
        rc = lib.zmpc_push_map(plan.handle, B, n, vp(h.data_ptr()), vp(hi.data_ptr()),
                               vp(lo.data_ptr()), 2 * n, None,
                               None if st is None else vp(st.data_ptr()), T_VIOL, cfg.m,
                               vp(f.data_ptr()), vp(l.data_ptr()), None, stream())
        if rc != 0:
            _native.check(rc, "zmpc_push_map")

    def new(D, axes, f, l, st=None):
        rc = lib.zmpc_push_map_shaped(plan.handle, B, n, vp(hist.data_ptr()), vp(zx.data_ptr()),
                                      vp(zn.data_ptr()), 2 * n, None,
                                      None if st is None else vp(st.data_ptr()), None, D, axes, T_VIOL,
                                      cfg.m, vp(f.data_ptr()), vp(l.data_ptr()), None, stream())
        if rc != 0:
            _native.check(rc, "zmpc_push_map_shaped")

    def flip_route():
        old(hist, zx, zn, f2, l2)
        hist_f.copy_(hist.flip(2))
        zx_f.copy_(zx.flip(2))
        zn_f.copy_(zn.flip(2))
        old(hist_f, zx_f, zn_f, f2b, l2b)

    forms = {"map_y": lambda: old(hist, zx, zn, f2, l2),
             "shaped_y_d1": lambda: new(1, 2, f2, l2),
             "shaped_y_d20": lambda: new(20, 2, f2, l2),
             "shaped_x_d1": lambda: new(1, 1, f2, l2),
             "shaped_xy_d1": lambda: new(1, 3, f4, l4),
             "shaped_xy_d20": lambda: new(20, 3, f4, l4),
             "flip_route": flip_route,
             "step_y": lambda: old(hist, zx, zn, fs2, ls2, steps),
             "step_x": lambda: new(1, 1, fs2, ls2, steps),
             "step_xy": lambda: new(1, 3, fs4, ls4, steps)}
    for fn in forms.values():  # warm-up of every form the timed window uses
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            ms[k].append(timed(fn, launches))
    torch.cuda.synchronize()
    # what the forms computed: the flip route's tables are the two-axis launch's columns
    new(1, 3, f4, l4)
    flip_route()
    torch.cuda.synchronize()
    same = bool(torch.equal(f4[..., 2:], f2) and torch.equal(f4[..., :2], f2b)
                and torch.equal(l4[..., 2:], l2) and torch.equal(l4[..., :2], l2b))
    med = {k: float(np.median(v)) for k, v in ms.items()}

    def ratio(a, b):
        r = [x / y for x, y in zip(ms[a], ms[b])]
        return {"median": med[a] / med[b], "min": min(r), "max": max(r)}

    return {"shape": name, "B": B, "n": n, "N": plan.N, "max_violation": T_VIOL,
            "rounds": rounds, "launches_per_round": launches, "ms_rounds": ms, "ms": summary(ms),
            "walks_passing_unpushed": float(np.mean(~np.isnan(f4[:, 0, 0].cpu().numpy()))),
            "xy_equals_flip_route_bitwise": same,
            "a_shaped_y_over_map_y": {"d1": ratio("shaped_y_d1", "map_y"),
                                      "d20": ratio("shaped_y_d20", "map_y")},
            "a_shaping_cost_ms": {"d1": med["shaped_y_d1"] - med["map_y"],
                                  "d20": med["shaped_y_d20"] - med["map_y"]},
            "x_over_y": ratio("shaped_x_d1", "shaped_y_d1"),
            "b_xy_over_y": {"d1": ratio("shaped_xy_d1", "shaped_y_d1"),
                            "d20": ratio("shaped_xy_d20", "shaped_y_d20")},
            "c_flip_route_over_xy_d1": ratio("flip_route", "shaped_xy_d1")}


def compare(parent_dirs, new_dirs, out):
    """ab_vs_parent.json from the per-process records of two builds (no device)."""
    res = {}
    for shape in ("config2", "b1"):
        def meds(dirs):
            recs = [json.load(open(os.path.join(d, f"push_shaped_ab_{shape}.json"))) for d in dirs]
            return {k: [r["ms"][k]["median"] for r in recs] for k in recs[0]["ms"]}
        par, new = meds(parent_dirs), meds(new_dirs)
        res[shape] = {}
        for k in par:
            mp, mn = float(np.median(par[k])), float(np.median(new[k]))
            spread = (max(par[k]) - min(par[k])) / min(par[k])
            res[shape][k] = {"parent_process_medians_ms": par[k], "new_process_medians_ms": new[k],
                             "parent_ms": mp, "new_ms": mn, "parent_spread": spread,
                             "new_over_parent": mn / mp,
                             "within_parent_spread": bool(mn / mp <= 1.0 + spread)}
    with open(os.path.join(out, "ab_vs_parent.json"), "w") as f:
        json.dump(res, f, indent=1)
    for shape, forms in res.items():
        for k, v in forms.items():
            print(f"{shape:8s} {k:14s} parent {v['parent_ms']:.4f} new {v['new_ms']:.4f} ms  "
                  f"ratio {v['new_over_parent']:.3f}  spread {v['parent_spread']:.3f}  "
                  f"{'ok' if v['within_parent_spread'] else 'SLOWER'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--compare-parent", default=None)
    ap.add_argument("--compare-new", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--only", choices=("config2", "b1"), default=None)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.compare_parent:
        return compare(args.compare_parent.split(","), args.compare_new.split(","), args.out)
    if not torch.cuda.is_available():
        raise SystemExit("push_shaped_ab.py needs a HIP device (no CPU path)")
    c = ZMPController(MPCConfig(horizon=150, strict=False))
    walk = np.load(os.path.join(ROOT, "tests", "golden", "walk_n150.npz"))
    zmax, zmin = walk["zmax"], walk["zmin"]
    assert len(zmax) == 420 and float(walk["dt"]) == c.config.dt and float(walk["m"]) == c.config.m
    rng = np.random.default_rng(SEED)
    for name, B in (("config2", 4096), ("b1", 1)):
        if args.only in (None, name):
            rec = shape_record(name, c, zmax, zmin, B, args.rounds, args.launches, rng)
            with open(os.path.join(args.out, f"push_shaped_ab_{name}.json"), "w") as f:
                json.dump(rec, f, indent=1)
            print(json.dumps({k: rec[k] for k in rec if k != "ms_rounds"}), flush=True)


if __name__ == "__main__":
    main()
