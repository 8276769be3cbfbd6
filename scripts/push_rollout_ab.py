"""Rollouts under the legacy kick and under a push window, timed for an A/B against another build.

    ZMPC_LIB=<library> timeout -k 10 300 python scripts/push_rollout_ab.py --out DIR

one process per build, the builds in alternation, three processes each, every process into a
directory of its own; with --legacy-only for the A/B proper, so that both builds issue the same
sequence of launches, and without it once more for the pushed forms
(the method of profiles/pushunit/ab_vs_parent.json); then, without a device,

    python scripts/push_rollout_ab.py --out profiles/pushroll \
        --compare-parent p1,p2,p3 --compare-new n1,n2,n3

writes ab_vs_parent.json: per form the median over processes of the per-process medians, the
parent's own spread (largest − smallest of its process medians) / smallest — the bar: a difference
inside what the parent shows against itself is none — and the ratio new / parent.

Forms (HIP events around back-to-back ctypes calls on prepared arguments, the forms alternating
round by round, every round's time recorded):
  strict_lq_kick      zmpc_rollout, bench.py's config 3: 65 536 walks x 420 samples, N = 150,
                      strict, F ~ U(0, 800) N at n // 2 (the LQ kernel)
  strict_scan_kick    the same walks' first 1024 (the parallel-in-time kernel)
  herdt_kick          zmpc_herdt_rollout, config 6: 32 768 walks of the default Herdt walk
  unc_kick            zmpc_rollout, config 2: 4096 x 420, unconstrained
and, where the library exports zmpc_rollout_pushed, beside them the pushed forms of the same
shapes: *_push_xy_d20, the walk's force spread over D = 20 samples along (0.6, 0.8).
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
from mpc_bipedal.config import MPCConfig  # noqa: E402
from mpc_bipedal.generators import CoPGenerator, SpeedTrajectoryGenerator  # noqa: E402
from mpc_bipedal.controllers import herdt as H  # noqa: E402

SEED = 20251226
D = 20
DIRECTION = (0.6, 0.8)


def load():
    """The library named by ZMPC_LIB (or the tree's), with the symbols this script calls; an
    earlier build has no pushed entry points."""
    lib = ctypes.CDLL(_native.LIB_PATH)
    names = ["zmpc_plan_create", "zmpc_plan_destroy", "zmpc_rollout", "zmpc_herdt_rollout",
             "zmpc_last_error"]
    pushed = hasattr(lib, "zmpc_rollout_pushed")
    if pushed:
        names += ["zmpc_rollout_pushed", "zmpc_herdt_rollout_pushed"]
    for name in names:
        res, args = _native.SIGNATURES[name]
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib, pushed


def make_plan(lib, cfg, N, strict):
    from mpc_bipedal.models.lipm_model import plan_constants
    c = plan_constants(cfg.dt, cfg.h, cfg.g)
    h = ctypes.c_void_p()
    rc = lib.zmpc_plan_create(0, N, c["T"], c["T2_2"], c["T3_6"], c["hg"], c["Thg"], cfg.Q, cfg.R,
                              int(strict), None, ctypes.byref(h))
    if rc != 0:
        raise SystemExit(f"zmpc_plan_create: {lib.zmpc_last_error()}")
    return h


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


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def wieber_forms(lib, pushed, cfg, B, strict, tag, forms, keep):
    """zmpc_rollout on B walks of the default CoP at rigid offsets (bench.py make_batch)."""
    zmax, zmin, _ = CoPGenerator(cfg).generate_cop_trajectory()
    n = len(zmax)
    rng = np.random.default_rng(SEED)
    off = rng.uniform(-0.02, 0.02, (B, 1, 2))
    x0 = np.zeros((B, 2, 3))
    x0[:, :, 0] = rng.uniform(-0.01, 0.01, (B, 2))
    F = rng.uniform(0.0, 800.0, B)
    f64 = dict(dtype=torch.float64, device="cuda")
    zx, zn = torch.as_tensor(zmax[None] + off, **f64), torch.as_tensor(zmin[None] + off, **f64)
    x0_t = torch.as_tensor(x0, **f64)
    kick = torch.as_tensor(cfg.dt * F / cfg.m, **f64)
    amp = torch.as_tensor((cfg.dt * F / cfg.m / D)[:, None] * np.array(DIRECTION), **f64)
    hist = torch.empty((B, n, 2, 3), **f64)
    status = torch.empty(B, dtype=torch.int32, device="cuda")
    plan = make_plan(lib, cfg, cfg.horizon, strict)
    push = _native.ZmpcPush(amp.data_ptr(), 3, None, n // 2, None, D)
    keep += [zx, zn, x0_t, kick, amp, hist, status, push, plan]

    def kicked(Bs):
        def f():
            rc = lib.zmpc_rollout(plan, Bs, n, vp(zx), vp(zn), 2 * n, vp(x0_t), vp(kick), n // 2,
                                  vp(hist), vp(status), stream())
            assert rc == 0, lib.zmpc_last_error()
        return f

    def shoved(Bs):
        def f():
            rc = lib.zmpc_rollout_pushed(plan, Bs, n, vp(zx), vp(zn), 2 * n, vp(x0_t),
                                         ctypes.addressof(push), vp(hist), vp(status), stream())
            assert rc == 0, lib.zmpc_last_error()
        return f

    for name, Bs in tag:
        forms[f"{name}_kick"] = kicked(Bs)
        if pushed:
            forms[f"{name}_push_xy_d20"] = shoved(Bs)


def herdt_forms(lib, pushed, B, forms, keep):
    """zmpc_herdt_rollout on bench.py's config 6."""
    cfg = MPCConfig(method="herdt", add_force=True, horizon=150)
    vx, vy, states = SpeedTrajectoryGenerator(cfg).generate_speed_and_state(save_footsteps=False)
    st = H.encode_states(states)
    n, N = len(st), cfg.horizon
    pad = H.pad_states(st, N)
    nb = np.array([t[0] for t in H.find_nb_steps(pad)][:n], np.int32)
    prm = H.make_params(cfg, H.max_footsteps(pad[None], N, n))
    rng = np.random.default_rng(SEED)
    x0 = np.zeros((B, 2, 3))
    x0[:, :, 0] = rng.uniform(-0.01, 0.01, (B, 2))
    F = rng.uniform(0.0, 800.0, B)
    f64 = dict(dtype=torch.float64, device="cuda")
    v = torch.as_tensor(np.stack([vx, vy], 1), **f64)
    s_t, nb_t = torch.as_tensor(st, device="cuda"), torch.as_tensor(nb, device="cuda")
    x0_t = torch.as_tensor(x0, **f64)
    kick = torch.as_tensor(cfg.dt * F / cfg.m, **f64)
    amp = torch.as_tensor((cfg.dt * F / cfg.m / D)[:, None] * np.array(DIRECTION), **f64)
    hist, foot = torch.empty((B, n, 2, 3), **f64), torch.empty((B, n, 2), **f64)
    status = torch.empty(B, dtype=torch.int32, device="cuda")
    plan = make_plan(lib, cfg, N, False)
    push = _native.ZmpcPush(amp.data_ptr(), 3, None, n // 2, None, D)
    keep += [v, s_t, nb_t, x0_t, kick, amp, hist, foot, status, push, plan, prm]

    def kicked():
        rc = lib.zmpc_herdt_rollout(plan, ctypes.addressof(prm), B, n, vp(v), 0, vp(s_t), 0,
                                    vp(nb_t), 0, vp(x0_t), vp(kick), n // 2, vp(hist), vp(foot),
                                    vp(status), stream())
        assert rc == 0, lib.zmpc_last_error()

    def shoved():
        rc = lib.zmpc_herdt_rollout_pushed(plan, ctypes.addressof(prm), B, n, vp(v), 0, vp(s_t), 0,
                                           vp(nb_t), 0, vp(x0_t), ctypes.addressof(push), vp(hist),
                                           vp(foot), vp(status), stream())
        assert rc == 0, lib.zmpc_last_error()

    forms["herdt_kick"] = kicked
    if pushed:
        forms["herdt_push_xy_d20"] = shoved


def compare(parent_dirs, new_dirs, out):
    """ab_vs_parent.json from the per-process records of two builds (no device)."""
    def meds(dirs):
        recs = [json.load(open(os.path.join(d, "push_rollout_ab.json"))) for d in dirs]
        return {k: [r["ms"][k]["median"] for r in recs] for k in recs[0]["ms"]}
    par, new = meds(parent_dirs), meds(new_dirs)
    res = {}
    for k in new:
        mn = float(np.median(new[k]))
        res[k] = {"new_process_medians_ms": new[k], "new_ms": mn}
        if k in par:
            mp = float(np.median(par[k]))
            spread = (max(par[k]) - min(par[k])) / min(par[k])
            res[k].update({"parent_process_medians_ms": par[k], "parent_ms": mp,
                           "parent_spread": spread, "new_over_parent": mn / mp,
                           "within_parent_spread": bool(mn / mp <= 1.0 + spread)})
    with open(os.path.join(out, "ab_vs_parent.json"), "w") as f:
        json.dump(res, f, indent=1)
    for k, v in res.items():
        if "parent_ms" in v:
            print(f"{k:26s} parent {v['parent_ms']:.4f} new {v['new_ms']:.4f} ms  ratio "
                  f"{v['new_over_parent']:.4f}  spread {v['parent_spread']:.4f}  "
                  f"{'ok' if v['within_parent_spread'] else 'SLOWER'}")
        else:
            print(f"{k:26s} new {v['new_ms']:.4f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--compare-parent", default=None)
    ap.add_argument("--compare-new", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--duration", type=int, default=D,
                    help="samples of the push window of the *_push_xy forms (the record names "
                         "them *_push_xy_d20 whatever the value)")
    ap.add_argument("--legacy-only", action="store_true",
                    help="time the *_kick forms alone (the same sequence of launches for both "
                         "builds: the A/B proper)")
    args = ap.parse_args()
    globals()["D"] = args.duration
    os.makedirs(args.out, exist_ok=True)
    if args.compare_parent:
        return compare(args.compare_parent.split(","), args.compare_new.split(","), args.out)
    if not torch.cuda.is_available():
        raise SystemExit("push_rollout_ab.py needs a HIP device (no CPU path)")
    lib, pushed = load()
    pushed = pushed and not args.legacy_only
    forms, keep = {}, []
    wieber_forms(lib, pushed, MPCConfig(horizon=150, strict=True), 65536, True,
                 (("strict_lq", 65536), ("strict_scan", 1024)), forms, keep)
    wieber_forms(lib, pushed, MPCConfig(horizon=150, strict=False), 4096, False,
                 (("unc", 4096),), forms, keep)
    herdt_forms(lib, pushed, 32768, forms, keep)
    for fn in forms.values():  # warm-up of every form the timed window uses
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            ms[k].append(timed(fn, args.launches))
    torch.cuda.synchronize()
    rec = {"library": os.path.basename(_native.LIB_PATH), "pushed_entry_points": pushed,
           "push_duration": D,
           "rounds": args.rounds, "launches_per_round": args.launches, "ms_rounds": ms,
           "ms": {k: {"median": float(np.median(v)), "min": min(v), "max": max(v)}
                  for k, v in ms.items()}}
    with open(os.path.join(args.out, "push_rollout_ab.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec["ms"]), flush=True)


if __name__ == "__main__":
    main()
