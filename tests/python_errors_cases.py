"""The bad calls of tests/test_gpu_python_errors.py: one table over every Python-side raise of
mpc_bipedal/solver.py and controllers/zmp_controller.py (and generate_cop_batch), at the
smallest shapes — unconstrained and strict plans at N = 8, B = 2 walks of n = 4 samples.

Each row is (id, callable of the shared context).  What a row must raise — the exception type
and str(exc), character for character — was recorded from the commit before the checked-argument
layer (tests/golden/make_python_errors_golden.py → tests/golden/python_errors.json), and so was
what the launchers keep alive (LAUNCHERS, describe).  The rows that involve a trace, the sizing of
critical_force_herdt and the Herdt and traced launchers were recorded the same way from the commit
before the disturbances' host side was merged into one path.  Needs a HIP device: the checks
build device tensors.
"""
import numpy as np
import torch

from mpc_bipedal import _native
from mpc_bipedal.analysis import Push, PushTrace
from mpc_bipedal.config import MPCConfig
from mpc_bipedal.controllers import ZMPController, herdt
from mpc_bipedal.generators.cop_generator import generate_cop_batch
from mpc_bipedal.solver import Plan, get_plan

FILE = "python_errors.json"
N, B, n = 8, 2, 4
MASS = 40.0


class Context:
    """Plans, controllers and one set of valid inputs; nothing in it is written by a row."""

    def __init__(self):
        self.dev = torch.device("cuda", 0)
        cfg = MPCConfig(horizon=N, strict=False)
        self.up = Plan(0, N, cfg.dt, cfg.h, cfg.g, cfg.Q, cfg.R, False)
        self.sp = Plan(0, N, cfg.dt, cfg.h, cfg.g, cfg.Q, cfg.R, True)
        self.cu = ZMPController(cfg)
        self.cs = ZMPController(MPCConfig(horizon=N, strict=True))
        self.ch = ZMPController(MPCConfig(horizon=N, method="herdt"))
        self.zmax = np.full((B, n, 2), 0.05)
        self.zmin = -self.zmax
        self.x0 = np.zeros((B, 2, 3))
        self.hist, _ = self.up.rollout(self.zmax, self.zmin, self.x0)
        self.push = Push(1.0, +1, 1)
        # Herdt: every check of Plan.herdt_rollout comes before the launch
        self.prm = herdt.make_params(self.ch.config, 1)
        self.v = np.zeros((B, n, 2))
        self.st = np.zeros((B, n), np.int8)
        self.nb = np.ones((B, n), np.int32)
        self.trace = PushTrace(np.ones((B, 2)), 1)  # newtons on y: it needs the mass
        # ... and one short gait whose launchers are issued (launchers)
        hs = np.array([herdt.STANDING] * 2 + ([herdt.DOUBLE_SUPPORT] * 2
                                              + [herdt.SINGLE_SUPPORT] * 4) * 2, np.int8)
        self.hst, self.hnb, _, most = self.up.herdt_prepare(np.stack([hs, hs]))
        self.hprm = herdt.make_params(self.ch.config, most)
        self.hv = np.tile([0.1, 0.0], (B, len(hs), 1))

    def t(self, *shape, dtype=torch.float64):
        return torch.zeros(shape, dtype=dtype, device=self.dev)

    def close(self):
        self.up.destroy()
        self.sp.destroy()


def _destroyed(c):
    p = Plan(0, N, c.up.dt, c.up.h, c.up.g, c.up.Q, c.up.R, False)
    p.destroy()
    return p.handle


def _bad_hists(c):
    """(tag, hist) that walk_metrics and push_map refuse."""
    return (("dtype", c.t(B, n, 2, 3, dtype=torch.float32)), ("shape", c.t(B, n, 3, 2)),
            ("strided", c.t(B, n, 3, 2).transpose(2, 3)), ("numpy", np.zeros((B, n, 2, 3))),
            ("empty", c.t(B, 0, 2, 3)))


def rows():
    """[(id, callable(context))], ids unique."""
    r = []
    add = lambda name, fn: r.append((name, fn))  # noqa: E731
    three = [1, 2, 3]

    add("as_dev/shape", lambda c: c.up.step(np.zeros((B, 3)), np.zeros((B, N - 1)),
                                            np.zeros((B, N))))
    add("plan/destroyed", _destroyed)
    add("plan/backend", lambda c: get_plan(MPCConfig(horizon=N, backend="tpu")))
    add("export/unknown", lambda c: c.up.export(15))
    add("export/not_held", lambda c: c.up.export(_native.EXPORT_X))

    # Plan.rollout, on both kinds of plan where the check is shared
    for tag in ("up", "sp"):
        plan = lambda c, tag=tag: getattr(c, tag)  # noqa: E731
        add(f"rollout/{tag}/x0", lambda c, p=plan: p(c).rollout(c.zmax, c.zmin, np.zeros((B, 3))))
        add(f"rollout/{tag}/bounds_rank",
            lambda c, p=plan: p(c).rollout(c.zmax[0, :, 0], c.zmin[0, :, 0], c.x0))
        add(f"rollout/{tag}/bounds_B",
            lambda c, p=plan: p(c).rollout(np.zeros((3, n, 2)), np.zeros((3, n, 2)), c.x0))
        add(f"rollout/{tag}/zmin", lambda c, p=plan: p(c).rollout(c.zmax, c.zmin[:, :3], c.x0))
        add(f"rollout/{tag}/hist_dtype",
            lambda c, p=plan: p(c).rollout(c.zmax, c.zmin, c.x0,
                                           hist=c.t(B, n, 2, 3, dtype=torch.float32)))
        add(f"rollout/{tag}/hist_shape",
            lambda c, p=plan: p(c).rollout(c.zmax, c.zmin, c.x0, hist=c.t(B, n + 1, 2, 3)))
        add(f"rollout/{tag}/hist_strided",
            lambda c, p=plan: p(c).rollout(c.zmax, c.zmin, c.x0,
                                           hist=c.t(B, n, 3, 2).transpose(2, 3)))
        add(f"rollout/{tag}/kick_shape",
            lambda c, p=plan: p(c).rollout(c.zmax, c.zmin, c.x0, kick=np.zeros(3), kick_step=1))
        add(f"rollout/{tag}/kick_steps",
            lambda c, p=plan: p(c).rollout(c.zmax, c.zmin, c.x0, kick=np.zeros(B),
                                           kick_step=three))
        add(f"rollout/{tag}/kick_and_push",
            lambda c, p=plan: p(c).rollout(c.zmax, c.zmin, c.x0, kick=np.zeros(B), push=c.push,
                                           mass=MASS))
        add(f"rollout/{tag}/push_type",
            lambda c, p=plan: p(c).rollout(c.zmax, c.zmin, c.x0, push="shove", mass=MASS))
        for mtag, mass in (("none", None), ("zero", 0.0), ("inf", float("inf"))):
            add(f"rollout/{tag}/mass_{mtag}",
                lambda c, p=plan, mass=mass: p(c).rollout(c.zmax, c.zmin, c.x0, push=c.push,
                                                          mass=mass))
        add(f"rollout/{tag}/push_batch",
            lambda c, p=plan: p(c).rollout(c.zmax, c.zmin, c.x0, push=Push(np.ones(3), +1, 1),
                                           mass=MASS))
        add(f"launcher/{tag}/hist_shape",
            lambda c, p=plan: p(c).rollout_launcher(c.zmax, c.zmin, c.x0,
                                                    hist=c.t(B, n + 1, 2, 3)))
        add(f"launcher/{tag}/kick_and_push",
            lambda c, p=plan: p(c).rollout_launcher(c.zmax, c.zmin, c.x0, kick=np.zeros(B),
                                                    push=c.push, mass=MASS))

        # ... and a trace beside or instead of them
        roll = lambda c, p=plan, **kw: p(c).rollout(c.zmax, c.zmin, c.x0, **kw)  # noqa: E731
        add(f"rollout/{tag}/trace_and_kick",
            lambda c, roll=roll: roll(c, kick=np.zeros(B), trace=c.trace, mass=MASS))
        add(f"rollout/{tag}/trace_and_push",
            lambda c, roll=roll: roll(c, push=c.push, trace=c.trace, mass=MASS))
        add(f"rollout/{tag}/trace_type", lambda c, roll=roll: roll(c, trace=c.push, mass=MASS))
        for mtag, mass in (("none", None), ("zero", 0.0), ("inf", float("inf"))):
            add(f"rollout/{tag}/trace_mass_{mtag}",
                lambda c, roll=roll, mass=mass: roll(c, trace=c.trace, mass=mass))
        add(f"rollout/{tag}/trace_batch",
            lambda c, roll=roll: roll(c, trace=PushTrace(np.ones((3, 2)), 1), mass=MASS))
        add(f"launcher/{tag}/trace_and_kick",
            lambda c, p=plan: p(c).rollout_launcher(c.zmax, c.zmin, c.x0, kick=np.zeros(B),
                                                    trace=c.trace, mass=MASS))
        add(f"launcher/{tag}/trace_and_push",
            lambda c, p=plan: p(c).rollout_launcher(c.zmax, c.zmin, c.x0, push=c.push,
                                                    trace=c.trace, mass=MASS))

    # Plan.walk_metrics and Plan.push_map share the history, bounds and lengths rules
    calls = (("walk_metrics", lambda c, h, hi, lo, **kw: c.up.walk_metrics(h, hi, lo, **kw)),
             ("push_map", lambda c, h, hi, lo, **kw: c.up.push_map(h, hi, lo, mass=MASS, **kw)))
    for name, call in calls:
        for k, tag in enumerate(("dtype", "shape", "strided", "numpy", "empty")):
            add(f"{name}/hist_{tag}",
                lambda c, call=call, k=k: call(c, _bad_hists(c)[k][1], c.zmax, c.zmin))
        add(f"{name}/bounds_B",
            lambda c, call=call: call(c, c.hist, np.zeros((3, n, 2)), np.zeros((3, n, 2))))
        add(f"{name}/bounds_n",
            lambda c, call=call: call(c, c.hist, np.zeros((n + 1, 2)), np.zeros((n + 1, 2))))
        add(f"{name}/bounds_rank",
            lambda c, call=call: call(c, c.hist, np.zeros(n), np.zeros(n)))
        add(f"{name}/zmin", lambda c, call=call: call(c, c.hist, c.zmax, c.zmin[0]))
        add(f"{name}/lengths", lambda c, call=call: call(c, c.hist, c.zmax, c.zmin, lengths=three))
        add(f"{name}/lengths_2d",
            lambda c, call=call: call(c, c.hist, c.zmax, c.zmin, lengths=[[n], [n]]))
    add("walk_metrics/out_shape",
        lambda c: c.up.walk_metrics(c.hist, c.zmax, c.zmin, out=c.t(B, 11)))
    add("walk_metrics/out_dtype",
        lambda c: c.up.walk_metrics(c.hist, c.zmax, c.zmin, out=c.t(B, 12, dtype=torch.float32)))
    add("walk_metrics/out_strided",
        lambda c: c.up.walk_metrics(c.hist, c.zmax, c.zmin, out=c.t(12, B).t()))
    pm = lambda c, **kw: c.up.push_map(c.hist, c.zmax, c.zmin, mass=MASS, **kw)  # noqa: E731
    add("push_map/push_steps", lambda c: pm(c, push_steps=three))
    add("push_map/axes", lambda c: pm(c, axes="z"))
    add("push_map/duration", lambda c: pm(c, duration=0))
    add("push_map/profile_host", lambda c: pm(c, duration=2, profile=[1.0, 1.0, 1.0]))
    add("push_map/profile_length", lambda c: pm(c, duration=2, profile=c.t(3)))
    add("push_map/profile_dtype",
        lambda c: pm(c, duration=2, profile=c.t(2, dtype=torch.float32)))
    add("push_map/out_xy_two_columns",
        lambda c: pm(c, axes="xy", out=(c.t(B, n, 2), c.t(B, n, 2, dtype=torch.int32))))
    add("push_map/out_limit_dtype",
        lambda c: pm(c, out=(c.t(B, n, 2), c.t(B, n, 2, dtype=torch.int64))))
    add("push_map/out_single_step",
        lambda c: pm(c, push_steps=[1, 1], out=(c.t(B, n, 2), c.t(B, n, 2, dtype=torch.int32))))
    add("push_map/strict_plan",
        lambda c: c.sp.push_map(c.hist, c.zmax, c.zmin, mass=MASS))

    # Plan.rollout_metrics and its launcher
    for name in ("rollout_metrics", "rollout_metrics_launcher"):
        rm = lambda c, name=name, **kw: getattr(c.up, name)(c.zmax, c.zmin, c.x0, **kw)  # noqa: E731
        add(f"{name}/x0", lambda c, name=name: getattr(c.up, name)(c.zmax, c.zmin,
                                                                   np.zeros((B, 3))))
        add(f"{name}/bounds", lambda c, name=name: getattr(c.up, name)(
            np.zeros((3, n, 2)), np.zeros((3, n, 2)), c.x0))
        add(f"{name}/kick_steps", lambda c, rm=rm: rm(c, kick=np.zeros(B), kick_step=three))
        add(f"{name}/lengths", lambda c, rm=rm: rm(c, lengths=three))
        add(f"{name}/out", lambda c, rm=rm: rm(c, out=c.t(B, 11)))
    add("rollout_metrics/fused_only_strict",
        lambda c: c.sp.rollout_metrics(c.zmax, c.zmin, c.x0, fused_only=True))

    # Plan.herdt_rollout
    hr = lambda c, v=None, st=None, nb=None, x0=None, **kw: c.up.herdt_rollout(  # noqa: E731
        c.prm, c.v if v is None else v, c.st if st is None else st, c.nb if nb is None else nb,
        c.x0 if x0 is None else x0, **kw)
    add("herdt_rollout/x0", lambda c: hr(c, x0=np.zeros((B, 3))))
    add("herdt_rollout/v_rank1", lambda c: hr(c, v=np.zeros(n)))
    add("herdt_rollout/v_columns", lambda c: hr(c, v=np.zeros((n, 3))))
    add("herdt_rollout/v_B", lambda c: hr(c, v=np.zeros((3, n, 2))))
    add("herdt_rollout/states_n", lambda c: hr(c, st=np.zeros((B, n + 1), np.int8)))
    add("herdt_rollout/states_B", lambda c: hr(c, st=np.zeros((3, n), np.int8)))
    add("herdt_rollout/nb_next_n", lambda c: hr(c, nb=np.ones(n + 1, np.int32)))
    add("herdt_rollout/nb_next_B", lambda c: hr(c, nb=np.ones((3, n), np.int32)))
    add("herdt_rollout/kick_shape", lambda c: hr(c, kick=np.zeros(3)))
    add("herdt_rollout/kick_and_push",
        lambda c: hr(c, kick=np.zeros(B), push=c.push, mass=MASS))
    add("herdt_rollout/push_type", lambda c: hr(c, push=(10.0, 1), mass=MASS))
    add("herdt_rollout/mass_none", lambda c: hr(c, push=c.push))

    add("herdt_rollout/trace_and_kick",
        lambda c: hr(c, kick=np.zeros(B), trace=c.trace, mass=MASS))
    add("herdt_rollout/trace_and_push", lambda c: hr(c, push=c.push, trace=c.trace, mass=MASS))
    add("herdt_rollout/trace_type", lambda c: hr(c, trace=[[1.0]], mass=MASS))
    add("herdt_rollout/trace_mass_none", lambda c: hr(c, trace=c.trace))
    add("herdt_rollout/trace_batch",
        lambda c: hr(c, trace=PushTrace(np.ones((3, 2)), 1), mass=MASS))
    hl = lambda c, **kw: c.up.herdt_rollout_launcher(  # noqa: E731
        c.prm, c.v, c.st, c.nb, c.x0, **kw)
    add("herdt_rollout_launcher/trace_and_push",
        lambda c: hl(c, push=c.push, trace=c.trace, mass=MASS))
    add("herdt_rollout_launcher/push_type", lambda c: hl(c, push="shove", mass=MASS))
    add("herdt_rollout_launcher/trace_mass_none", lambda c: hl(c, trace=c.trace))
    add("herdt_rollout_launcher/foot_shape", lambda c: hl(c, push=c.push, mass=MASS,
                                                          foot=c.t(B, n, 3)))

    # Plan.trace_margin
    tm = lambda c, trace=None, plan="up", **kw: getattr(c, plan).trace_margin(  # noqa: E731
        c.hist, c.zmax, c.zmin, c.trace if trace is None else trace, **{"mass": MASS, **kw})
    add("trace_margin/trace_type", lambda c: tm(c, trace=c.push))
    add("trace_margin/rows", lambda c: tm(c, draws=2))
    add("trace_margin/rows_type_first", lambda c: tm(c, trace="trace", draws=2))
    add("trace_margin/draws_zero", lambda c: tm(c, draws=0))
    add("trace_margin/draws_bool", lambda c: tm(c, draws=True))
    add("trace_margin/draws_float", lambda c: tm(c, draws=1.0))
    add("trace_margin/mass_none", lambda c: tm(c, mass=None))
    add("trace_margin/mass_zero", lambda c: tm(c, mass=0.0))
    add("trace_margin/lengths", lambda c: tm(c, lengths=three))
    add("trace_margin/scale_shape", lambda c: tm(c, scale=c.t(B, 2)))
    add("trace_margin/limit_dtype", lambda c: tm(c, limit=c.t(B, 1, 2, dtype=torch.int64)))
    add("trace_margin/hist_numpy",
        lambda c: c.up.trace_margin(np.zeros((B, n, 2, 3)), c.zmax, c.zmin, c.trace, mass=MASS))
    add("trace_margin/strict_plan", lambda c: tm(c, plan="sp"))

    # ZMPController
    for name in ("generate_state_trajectory_batch", "generate_com_trajectory_batch"):
        sb = lambda c, name=name, **kw: getattr(c.cu, name)(None, c.zmax, c.zmin,  # noqa: E731
                                                            trace=c.trace, **kw)
        add(f"controller/{name}/trace_and_F_ext", lambda c, sb=sb: sb(c, F_ext=[1.0, 1.0]))
        add(f"controller/{name}/trace_and_push", lambda c, sb=sb: sb(c, push=c.push))
        add(f"controller/{name}/trace_and_force_step", lambda c, sb=sb: sb(c, force_step=1))
        add(f"controller/{name}/trace_and_walk_lengths",
            lambda c, sb=sb: sb(c, walk_lengths=[n, n]))
        add(f"controller/{name}/F_ext_push_and_trace",
            lambda c, sb=sb: sb(c, F_ext=[1.0, 1.0], push=c.push))
    add("controller/state_batch/trace_type",
        lambda c: c.cu.generate_state_trajectory_batch(c.x0, c.zmax, c.zmin, trace=c.push))
    hb = lambda c, **kw: c.ch.generate_com_trajectory_herdt_batch(None, c.v, c.st,  # noqa: E731
                                                                  trace=c.trace, **kw)
    add("controller/herdt_batch/trace_and_F_ext", lambda c: hb(c, F_ext=[1.0, 1.0]))
    add("controller/herdt_batch/trace_and_push", lambda c: hb(c, push=c.push))
    add("controller/herdt_batch/F_ext_push_and_trace",
        lambda c: hb(c, F_ext=[1.0, 1.0], push=c.push))
    for tag, ctl in (("up", "cu"), ("sp", "cs")):
        ct = lambda c, ctl=ctl, trace=None, **kw: getattr(c, ctl).critical_force(  # noqa: E731
            c.zmax, c.zmin, iters=0, trace=c.trace if trace is None else trace, **kw)
        add(f"controller/critical_force/{tag}/trace_type", lambda c, ct=ct: ct(c, trace=c.push))
        add(f"controller/critical_force/{tag}/trace_and_force_step",
            lambda c, ct=ct: ct(c, force_step=1))
        add(f"controller/critical_force/{tag}/trace_and_direction",
            lambda c, ct=ct: ct(c, direction=-1))
        add(f"controller/critical_force/{tag}/trace_and_signs",
            lambda c, ct=ct: ct(c, direction=[1, 1]))
        add(f"controller/critical_force/{tag}/trace_and_planar",
            lambda c, ct=ct: ct(c, direction=[[0.0, 1.0]]))
        add(f"controller/critical_force/{tag}/trace_and_duration",
            lambda c, ct=ct: ct(c, duration=2))
        add(f"controller/critical_force/{tag}/trace_and_profile",
            lambda c, ct=ct: ct(c, profile=[1.0]))
        add(f"controller/critical_force/{tag}/trace_fused", lambda c, ct=ct: ct(c, fused=True))
        add(f"controller/critical_force/{tag}/trace_sizes",
            lambda c, ct=ct: ct(c, trace=PushTrace(np.ones((3, 2)), 1)))
        add(f"controller/critical_force/{tag}/trace_bad_duration",
            lambda c, ct=ct: ct(c, duration=0))
    ch = lambda c, trace=None, max_dcm_dev=1.0, **kw: c.ch.critical_force_herdt(  # noqa: E731
        c.v, c.st, max_dcm_dev, iters=0, trace=c.trace if trace is None else trace, **kw)
    add("controller/critical_force_herdt/trace_type", lambda c: ch(c, trace=c.push))
    add("controller/critical_force_herdt/trace_and_force_step", lambda c: ch(c, force_step=1))
    add("controller/critical_force_herdt/trace_and_direction", lambda c: ch(c, direction=-1))
    add("controller/critical_force_herdt/trace_and_signs", lambda c: ch(c, direction=[1, 1]))
    add("controller/critical_force_herdt/trace_and_planar",
        lambda c: ch(c, direction=[[0.0, 1.0]]))
    add("controller/critical_force_herdt/trace_and_duration", lambda c: ch(c, duration=2))
    add("controller/critical_force_herdt/trace_and_profile", lambda c: ch(c, profile=[1.0]))
    add("controller/critical_force_herdt/trace_max_dcm_dev", lambda c: ch(c, max_dcm_dev=None))
    add("controller/critical_force_herdt/trace_F_hi", lambda c: ch(c, F_hi=0.0))
    add("controller/critical_force_herdt/trace_sizes",
        lambda c: ch(c, trace=PushTrace(np.ones((3, 2)), 1)))
    # ... and the sizing of critical_force_herdt without one, in its own words
    nh = lambda c, *a, **kw: c.ch.critical_force_herdt(*a, 1.0, iters=0, **kw)  # noqa: E731
    add("controller/critical_force_herdt/sizes", lambda c: nh(c, c.v, c.st, force_step=three))
    add("controller/critical_force_herdt/sizes_planar",
        lambda c: nh(c, c.v, c.st, direction=[[1, 0], [0, 1], [1, 1]]))
    add("controller/critical_force_herdt/sizes_first_force_step",
        lambda c: nh(c, c.v[0], c.st[0], force_step=three, direction=[1, 1]))
    add("controller/critical_force_herdt/sizes_direction_before_lengths",
        lambda c: nh(c, c.v[0], c.st[0], direction=[1, 1], walk_lengths=three))
    add("controller/critical_force_herdt/sizes_x_init",
        lambda c: nh(c, c.v[0], c.st[0], x_init=np.zeros((3, 2, 3)), force_step=[1, 1]))
    ctm = lambda c, ctl="cu", trace=None, **kw: getattr(c, ctl).trace_margin(  # noqa: E731
        c.zmax, c.zmin, c.trace if trace is None else trace, **kw)
    add("controller/trace_margin/trace_type", lambda c: ctm(c, trace=c.push))
    add("controller/trace_margin/draws", lambda c: ctm(c, draws=0))
    add("controller/trace_margin/rows_multiple",
        lambda c: ctm(c, trace=PushTrace(np.ones((3, 2)), 1), draws=2))
    add("controller/trace_margin/rows_named", lambda c: ctm(c, draws=2))
    add("controller/trace_margin/strict", lambda c: ctm(c, ctl="cs"))
    add("controller/state_batch/F_ext_and_push",
        lambda c: c.cu.generate_state_trajectory_batch(None, c.zmax, c.zmin, F_ext=[1.0, 1.0],
                                                       push=c.push))
    add("controller/state_batch/push_and_force_step",
        lambda c: c.cu.generate_state_trajectory_batch(None, c.zmax, c.zmin, force_step=1,
                                                       push=c.push))
    add("controller/state_batch/push_and_walk_lengths",
        lambda c: c.cu.generate_com_trajectory_batch(None, c.zmax, c.zmin, walk_lengths=[n, n],
                                                     push=c.push))
    add("controller/herdt_batch/F_ext_and_push",
        lambda c: c.ch.generate_com_trajectory_herdt_batch(None, c.v, c.st, F_ext=[1.0, 1.0],
                                                           push=c.push))
    cf = lambda c, *a, **kw: c.cu.critical_force(*a, iters=0, **kw)  # noqa: E731
    add("controller/critical_force/sizes",
        lambda c: cf(c, c.zmax, c.zmin, force_step=three))
    add("controller/critical_force/sizes_planar",
        lambda c: cf(c, c.zmax, c.zmin, direction=[[1, 0], [0, 1], [1, 1]]))
    # shared bounds: the first [B] argument sets B, in each method's own order
    add("controller/critical_force/sizes_first_force_step",
        lambda c: cf(c, c.zmax[0], c.zmin[0], force_step=three, walk_lengths=[n, n]))
    add("controller/critical_force/sizes_lengths_before_direction",
        lambda c: cf(c, c.zmax[0], c.zmin[0], walk_lengths=[n, n], direction=[1, 1, 1]))
    add("controller/critical_force/F_hi", lambda c: cf(c, c.zmax, c.zmin, F_hi=0.0))
    add("controller/critical_force/iters",
        lambda c: c.cu.critical_force(c.zmax, c.zmin, iters=-1))
    add("controller/critical_force/fused_duration",
        lambda c: cf(c, c.zmax, c.zmin, duration=2, fused=True))
    add("controller/critical_force/fused_planar",
        lambda c: cf(c, c.zmax, c.zmin, direction=[[1.0, 1.0]], fused=True))
    add("controller/critical_force/zero_direction",
        lambda c: cf(c, c.zmax, c.zmin, direction=[[0.0, 0.0]]))
    cx = lambda c, *a, **kw: c.cu.critical_force_exact(*a, **kw)  # noqa: E731
    add("controller/critical_force_exact/sizes", lambda c: cx(c, c.zmax, c.zmin, force_step=three))
    add("controller/critical_force_exact/sizes_planar",
        lambda c: cx(c, c.zmax, c.zmin, direction=[[1, 0], [0, 1], [1, 1]]))
    add("controller/critical_force_exact/sizes_direction_before_lengths",
        lambda c: cx(c, c.zmax[0], c.zmin[0], walk_lengths=[n, n], direction=[1, 1, 1]))
    add("controller/critical_force_exact/strict",
        lambda c: c.cs.critical_force_exact(c.zmax, c.zmin))
    add("controller/push_map/strict", lambda c: c.cs.push_map(c.zmax, c.zmin))
    add("controller/push_map/sizes",
        lambda c: c.cu.push_map(c.zmax, c.zmin, walk_lengths=three))
    add("controller/push_map/axes", lambda c: c.cu.push_map(c.zmax, c.zmin, axes="z"))
    add("controller/walk_metrics/bounds",
        lambda c: c.cu.walk_metrics(c.hist.cpu().numpy(), c.zmax[:, :3], c.zmin[:, :3]))
    add("controller/wieber/missing_bounds",
        lambda c: c.cu.generate_com_trajectory(np.zeros(3), np.zeros(3)))
    add("controller/herdt/missing_reference",
        lambda c: c.ch.generate_com_trajectory(np.zeros(3), np.zeros(3)))
    add("controller/unknown_method",
        lambda c: ZMPController(MPCConfig(horizon=N, method="kajita")).generate_com_trajectory(
            np.zeros(3), np.zeros(3)))
    add("controller/predict_wieber_axis/rows",
        lambda c: c.cu.predict_wieber_axis(np.zeros(3), N, np.zeros(N - 1), np.zeros(N - 1)))
    add("controller/state_trajectory_wieber/bounds",
        lambda c: c.cu.generate_state_trajectory_wieber(np.zeros(3), np.zeros(3), np.zeros((n, 3)),
                                                        np.zeros((n, 3))))

    add("generate_cop_batch/params", lambda c: generate_cop_batch(np.zeros((B, 6))))
    assert len({name for name, _ in r}) == len(r)
    return r


def raised(fn, ctx):
    """[exception type name, str(exc)] of fn(ctx); [None, None] if it raises nothing."""
    try:
        fn(ctx)
    except Exception as e:  # noqa: BLE001 (the table pins the type)
        return [type(e).__name__, str(e)]
    return [None, None]


# -- what the launchers keep alive -----------------------------------------------------------
def launchers(c):
    """name → launcher, one of each form."""
    kick = torch.full((B,), 0.01, dtype=torch.float64, device=c.dev)
    return {
        "rollout_launcher/kick": c.up.rollout_launcher(c.zmax, c.zmin, c.x0, kick=kick,
                                                       kick_step=1),
        "rollout_launcher/kick_steps": c.up.rollout_launcher(c.zmax, c.zmin, c.x0, kick=kick,
                                                             kick_step=[0, 1]),
        "rollout_launcher/push": c.up.rollout_launcher(c.zmax, c.zmin, c.x0, push=c.push,
                                                       mass=MASS),
        "rollout_launcher/push_steps_profile": c.up.rollout_launcher(
            c.zmax, c.zmin, c.x0, push=Push(1.0, [[1.0, 1.0]], np.array([0, 1]), duration=2,
                                            profile=[1.0, 0.5]), mass=MASS),
        "rollout_launcher/strict_push": c.sp.rollout_launcher(c.zmax, c.zmin, c.x0, push=c.push,
                                                              mass=MASS),
        "rollout_launcher/trace": c.up.rollout_launcher(c.zmax, c.zmin, c.x0, trace=c.trace,
                                                        mass=MASS),
        "rollout_launcher/trace_steps_device": c.up.rollout_launcher(
            c.zmax, c.zmin, c.x0, trace=PushTrace.from_velocity_steps(
                torch.full((B, 3, 2), 1e-3, dtype=torch.float64, device=c.dev), np.array([0, 1]))),
        "rollout_launcher/strict_trace": c.sp.rollout_launcher(c.zmax, c.zmin, c.x0,
                                                               trace=c.trace, mass=MASS),
        "herdt_rollout_launcher/push": c.up.herdt_rollout_launcher(
            c.hprm, c.hv, c.hst, c.hnb, c.x0, push=c.push, mass=MASS),
        "herdt_rollout_launcher/push_steps_profile": c.up.herdt_rollout_launcher(
            c.hprm, c.hv, c.hst, c.hnb, c.x0, mass=MASS,
            push=Push(1.0, [[1.0, 1.0]], np.array([0, 1]), duration=2, profile=[1.0, 0.5])),
        "herdt_rollout_launcher/trace": c.up.herdt_rollout_launcher(
            c.hprm, c.hv, c.hst, c.hnb, c.x0, trace=c.trace, mass=MASS),
        "rollout_metrics_launcher": c.up.rollout_metrics_launcher(
            c.zmax, c.zmin, c.x0, kick=kick, kick_step=[0, 1], lengths=[n, n - 1]),
    }


def describe(x):
    """The kind of an object a launcher holds: nested lists of type, dtype and shape."""
    if isinstance(x, (tuple, list)):
        return [describe(e) for e in x]
    if isinstance(x, torch.Tensor):
        return f"Tensor {str(x.dtype).replace('torch.', '')} {list(x.shape)} {x.device}"
    return type(x).__name__


def launcher_record(launch):
    """What a launcher exposes: its attributes' kinds."""
    return {k: describe(v) for k, v in sorted(vars(launch).items())}
