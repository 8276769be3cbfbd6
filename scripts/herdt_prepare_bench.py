"""The preparation of a heterogeneous Herdt batch timed beside the rollout it feeds: 32 768
different schedules (the default gait, 302 samples at N = 150, shifted per walk), the same with
ragged lengths, and one walk.

    timeout -k 10 900 python scripts/herdt_prepare_bench.py --out profiles/herdtprep

Host route: what ZMPController._herdt_host does with states that live on the device — the copy to
the host, herdt.max_footsteps and the herdt.find_nb_steps loop, nb_next back up.  Device route:
Plan.herdt_prepare (zmpc_herdt_prepare, synchronous).  The two alternate in one process, 5
rounds, wall clock round a synchronised call; medians with the round ranges.  The host route has
no ragged form (it pads to the batch's n), so the ragged batch times the device route alone.  One
zmpc_herdt_rollout of the same batch is timed the same way.  Reads no file outside the tree.
Needs a HIP device: there is no CPU path."""
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

from mpc_bipedal.config import MPCConfig  # noqa: E402
from mpc_bipedal.controllers import ZMPController  # noqa: E402
from mpc_bipedal.controllers import herdt as H  # noqa: E402

SEED = 20251226
ROUNDS = 5


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def summary(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)),
                rounds=len(ms))


def schedules(B, rng):
    """B different walks: the default schedule with its first stand lengthened by a shift of its
    own, cut to the default's 302 samples; and ragged lengths for them."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "herdt_default.npz"))["states"]
    n = len(d)
    shift = rng.integers(0, 100, B)
    st = np.stack([np.concatenate([np.zeros(s, np.int8), d])[:n] for s in shift]).astype(np.int8)
    return st, rng.integers(n // 2, n + 1, B)


def measure(B, rounds, host_rounds):
    rng = np.random.default_rng([SEED, B])
    ctl = ZMPController(MPCConfig(method="herdt"))
    plan = ctl._plan()
    dev = torch.device("cuda", plan.device)
    st, lengths = schedules(B, rng)
    n = st.shape[1]
    st_d = torch.as_tensor(st, device=dev)
    len_d = torch.as_tensor(lengths, device=dev)

    def host_route():
        h = st_d.cpu().numpy()
        prm, nb = ctl._herdt_host(plan, h)
        return prm, torch.as_tensor(nb, device=dev)

    plan.herdt_prepare(st_d)  # (first launch: the code object loads)
    t_host, t_dev, t_rag = [], [], []
    for r in range(rounds):
        if r < host_rounds:
            ms, (prm_h, nb_h) = wall(host_route)
            t_host.append(ms)
        ms, (clean, nb, steps, most) = wall(lambda: plan.herdt_prepare(st_d))
        t_dev.append(ms)
        ms, ragged = wall(lambda: plan.herdt_prepare(st_d, len_d))
        t_rag.append(ms)
    assert torch.equal(nb, nb_h) and most == prm_h.max_footsteps and torch.equal(clean, st_d)
    v = torch.zeros((B, n, 2), dtype=torch.float64, device=dev)
    v[..., 0] = 0.3
    v[..., 0].masked_fill_(st_d == 0, 0.0)
    x0 = torch.zeros((B, 2, 3), dtype=torch.float64, device=dev)
    prm = H.make_params(ctl.config, most)
    plan.herdt_rollout(prm, v, clean, nb, x0)
    t_roll = []
    for r in range(rounds):
        ms, (_, _, status) = wall(lambda: plan.herdt_rollout(prm, v, clean, nb, x0))
        t_roll.append(ms)
    return dict(B=B, n=n, N=plan.N, max_footsteps=most, max_footsteps_ragged=ragged[3],
                rollout_status_nonzero=int((status != 0).sum()),
                host_route=summary(t_host), device_prepare=summary(t_dev),
                device_prepare_ragged=summary(t_rag), herdt_rollout=summary(t_roll),
                host_over_device=float(np.median(t_host) / np.median(t_dev)),
                prepare_over_rollout=float(np.median(t_dev) / np.median(t_roll)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "herdtprep"))
    ap.add_argument("--walks", type=int, default=32768)
    ap.add_argument("--host-rounds", type=int, default=ROUNDS,
                    help="rounds of the host route at the large batch (seconds each)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    res = dict(device=torch.cuda.get_device_name(0), rounds=ROUNDS,
               one_walk=measure(1, ROUNDS, ROUNDS),
               batch=measure(a.walks, ROUNDS, a.host_rounds))
    path = os.path.join(a.out, "herdt_prepare_bench.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
