"""zmpc_herdt_walk_metrics timed on bench.py's config 6 (32 768 walks of the default Herdt walk,
302 samples, N = 150), beside the same sixteen numbers formed from torch tensor operations and
beside zmpc_walk_metrics on the same histories, and ZMPController.critical_force_herdt at 32 768
scenarios split into rollout and metrics time.

    timeout -k 10 600 python scripts/herdt_metrics_bench.py --out profiles/herdtmetrics

HIP events round back-to-back launches on prepared arguments, 5 rounds x 50 launches, the forms
alternating round by round in one process; medians with the round ranges.  The kernels' shares
of the 6.29 TB/s copy ceiling count B·n·(48 + 16 + 1) bytes for zmpc_herdt_walk_metrics (+16 with
foot_ref) and B·n·(48 + 32) for zmpc_walk_metrics with per-walk bounds.  Reads no file outside the
tree.  Needs a HIP device: there is no CPU path."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "model-predictive-control-for-bipedal-locomotion_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from mpc_bipedal.analysis import herdt_params_facets  # noqa: E402
from mpc_bipedal.config import MPCConfig  # noqa: E402
from mpc_bipedal.controllers import ZMPController  # noqa: E402
from mpc_bipedal.controllers import herdt as H  # noqa: E402
from mpc_bipedal.generators import SpeedTrajectoryGenerator  # noqa: E402

SEED = 20251226
COPY_CEILING = 6.29e12  # bytes/s, the device's measured copy rate
SS = H.SINGLE_SUPPORT
SHOVE_D = 20            # samples (0.2 s) of the −y shove that critical_force_herdt searches


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def torch_form(hist, foot, st, ref, hg, cfg, facets, tol):
    """The sixteen numbers from tensor operations (shared states [n]) → [B, 16]."""
    B, n = hist.shape[:2]
    dev = hist.device
    fs = torch.cat([foot[:, :1], foot[:, :-1]], dim=1)
    c, cd, cdd = hist[..., 0], hist[..., 1], hist[..., 2]
    z = c - hg * cdd
    land = torch.zeros(n, dtype=torch.bool, device=dev)
    land[:-1] = (st[:-1] == SS) & (st[1:] != SS)
    before = torch.cumsum(land, 0) - land.long()                  # landings at steps < k
    j = torch.clamp(torch.arange(n, device=dev) - 1, min=0)
    side = before[j] % 2
    half = torch.tensor([0.5 * cfg.foot_length, 0.5 * cfg.foot_width], dtype=hist.dtype,
                        device=dev)
    lo, hi = fs - half, fs + half
    other = torch.where(side == 1, fs[..., 1] + 2 * cfg.foot_spread,
                        fs[..., 1] - 2 * cfg.foot_spread)
    stand = st == 0
    lo_y = torch.where(stand, torch.minimum(fs[..., 1], other) - half[1], lo[..., 1])
    hi_y = torch.where(stand, torch.maximum(fs[..., 1], other) + half[1], hi[..., 1])
    lo = torch.stack([lo[..., 0], lo_y], dim=-1)
    hi = torch.stack([hi[..., 0], hi_y], dim=-1)
    v = torch.clamp(torch.maximum(z - hi, lo - z), min=0.0)
    v[:, 0] = 0.0
    vmax, arg = v.max(dim=1)
    arg = torch.where(vmax > 0, arg, torch.full_like(arg, -1)).to(hist.dtype)
    count = (v > tol).sum(dim=1).to(hist.dtype)
    dcm = c + cd * float(np.sqrt(hg)) - fs
    shift = (foot - ref).abs().amax(dim=1) if ref is not None else torch.zeros_like(vmax)
    k = land.nonzero()[:, 0]
    d = foot[:, k + 1] - foot[:, k]                               # [B, L, 2]
    slack = torch.full((B,), float("inf"), dtype=hist.dtype, device=dev)
    for sd in range(2):
        f = torch.as_tensor(facets[sd], dtype=hist.dtype, device=dev)
        sel = before[k] % 2 == sd
        if len(f) and bool(sel.any()):
            s = f[:, 2] - (d[:, sel, 0:1] * f[:, 0] + d[:, sel, 1:2] * f[:, 1])
            slack = torch.minimum(slack, s.amin(dim=(1, 2)))
    landed = torch.full((B,), float(len(k)), dtype=hist.dtype, device=dev)
    return torch.cat([vmax, arg, count, (c - fs).abs().amax(dim=1), dcm.abs().amax(dim=1),
                      dcm[:, -1], shift, slack[:, None], landed[:, None]], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "herdtmetrics"))
    ap.add_argument("--walks", type=int, default=32768)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    B = a.walks
    cfg = MPCConfig(method="herdt", add_force=True, horizon=150)
    ctl = ZMPController(cfg)
    vx, vy, states = SpeedTrajectoryGenerator(cfg).generate_speed_and_state(save_footsteps=False)
    st = H.encode_states(states)
    n = len(st)
    v = np.stack([vx, vy], 1)
    rng = np.random.default_rng(SEED)
    x0 = np.zeros((B, 2, 3))
    x0[:, :, 0] = rng.uniform(-0.01, 0.01, (B, 2))
    F = rng.uniform(0.0, 800.0, B)
    plan = ctl._plan()
    dev = torch.device("cuda", plan.device)
    _, _, foot_ref, st0 = ctl.generate_com_trajectory_herdt_batch(x0, v, st, return_status=True)
    _, hist, foot, st1 = ctl.generate_com_trajectory_herdt_batch(x0, v, st, F_ext=F,
                                                                 return_status=True)
    prm = H.make_params(cfg, 0)
    facets = herdt_params_facets(prm)
    st_t = torch.as_tensor(st, device=dev)
    hg = plan.consts["hg"]
    half = torch.tensor([0.5 * cfg.foot_length, 0.5 * cfg.foot_width], dtype=torch.float64,
                        device=dev)
    zmax, zmin = (foot + half).contiguous(), (foot - half).contiguous()
    m16 = torch.empty((B, 16), dtype=torch.float64, device=dev)
    m12 = torch.empty((B, 12), dtype=torch.float64, device=dev)
    forms = {
        "herdt_walk_metrics": lambda: plan.herdt_walk_metrics(prm, hist, foot, st_t, out=m16),
        "herdt_walk_metrics_foot_ref": lambda: plan.herdt_walk_metrics(
            prm, hist, foot, st_t, foot_ref=foot_ref, out=m16),
        "walk_metrics": lambda: plan.walk_metrics(hist, zmax, zmin, out=m12),
        "torch_ops": lambda: torch_form(hist, foot, st_t, foot_ref, hg, cfg, facets, 1e-9),
    }
    # the two forms give the same numbers (the value slots to rounding: torch may contract)
    got = plan.herdt_walk_metrics(prm, hist, foot, st_t, foot_ref=foot_ref).cpu().numpy()
    want = torch_form(hist, foot, st_t, foot_ref, hg, cfg, facets, 1e-9).cpu().numpy()
    ok = np.isfinite(want).all(axis=1) & np.isfinite(got).all(axis=1)
    value = [s for s in range(16) if s not in (2, 3, 4, 5)]
    agree = float(np.abs(got[ok][:, value] - want[ok][:, value]).max())
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, fn in forms.items():
            times[k].append(timed(fn, a.launches if k != "torch_ops" else max(a.launches // 10, 1)))
    bytes_of = {"herdt_walk_metrics": B * n * 65, "herdt_walk_metrics_foot_ref": B * n * 81,
                "walk_metrics": B * n * 80}
    out = {"walks": B, "samples": n, "N": cfg.horizon, "rounds": a.rounds,
           "launches_per_round": a.launches, "device": torch.cuda.get_device_name(dev),
           "torch_agreement_max_abs": agree,
           "status_nonzero": [int((st0 != 0).sum()), int((st1 != 0).sum())], "forms": {}}
    for k, ts in times.items():
        med = float(np.median(ts))
        row = {"ms_median": med, "ms_min": float(min(ts)), "ms_max": float(max(ts))}
        if k in bytes_of:
            row["bytes"] = bytes_of[k]
            row["share_of_copy_ceiling"] = bytes_of[k] / (med * 1e-3) / COPY_CEILING
            row["share_range"] = [bytes_of[k] / (t * 1e-3) / COPY_CEILING
                                  for t in (max(ts), min(ts))]
        out["forms"][k] = row
    # critical_force_herdt: the whole search by the wall clock, its rollout alone by events
    evals = a.iters + 2
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lo, hi = ctl.critical_force_herdt(v, st, 1.0, x_init=x0, direction=-1, iters=a.iters,
                                      duration=SHOVE_D)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    _, nb = ctl._herdt_host(plan, st)
    from mpc_bipedal.analysis import Push
    prm_r, _ = ctl._herdt_host(plan, st)
    launch = plan.herdt_rollout_launcher(prm_r, v, st, nb, x0,
                                         Push(F, -1, n // 2, duration=SHOVE_D), cfg.m)
    launch()
    roll = [timed(launch, 3) for _ in range(3)]
    lo_c = lo.cpu().numpy()
    out["critical_force_herdt"] = {
        "scenarios": B, "evaluations": evals, "shove_samples": SHOVE_D, "max_dcm_dev": 1.0, "ms_total_wall": wall,
        "ms_per_evaluation": wall / evals, "ms_rollout_per_evaluation": float(np.median(roll)),
        "ms_metrics_per_evaluation": out["forms"]["herdt_walk_metrics_foot_ref"]["ms_median"],
        "F_lo_min_median_max": [float(np.nanmin(lo_c)), float(np.nanmedian(lo_c)),
                                float(np.nanmax(lo_c))],
        "nan": int(np.isnan(lo_c).sum())}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "herdt_metrics_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
