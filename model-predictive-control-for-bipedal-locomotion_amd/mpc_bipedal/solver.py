"""Device-side solver objects on top of the C-ABI (``include/zmpc.h``).

``Plan`` owns one ``zmpc_plan`` (batch-invariant matrices on one HIP device).  Its methods
take torch tensors that live on that device (PyTorch-ROCm is used for device buffers and
streams only) and launch the HIP kernels on torch's current stream.
"""

import ctypes
import os
import threading
import weakref
from collections import OrderedDict

import numpy as np
import torch

from . import _native
from .models.lipm_model import plan_constants

# get_plan's cache: least recently used plans beyond ZMPC_PLAN_CACHE (default 8) are dropped
# (a plan holds N² matrices and the FFT tables; a caller sweeping horizons, as
# run_compare_runtime.py:139 does, would otherwise keep one per N)
_PLAN_CACHE = OrderedDict()
_PLAN_CACHE_LOCK = threading.Lock()
PLAN_CACHE_MAX = max(1, int(os.environ.get("ZMPC_PLAN_CACHE", "8")))


class _Disturbance:
    """What disturbs the walks of a rollout, as the C-ABI takes it (Plan._disturbance): the C
    symbol's suffix ("", "_kicks", "_pushed" or "_traced"), the C arguments between x0 and the
    outputs, what they point to (keep: the kick tensors; else the struct and the tensors it points
    to), the device tensor a caller may rescale between launches (scaled: the kick [B], the
    amplitudes [B, C] or the velocity steps [B, L, C]; None without a kick) and the
    _native.ZmpcTrace whose `stream` field takes the stream (trace; None for the symbols that
    take a stream argument)."""
    __slots__ = ("suffix", "args", "keep", "scaled", "trace")

    def __init__(self, suffix, args, keep, scaled, trace=None):
        self.suffix, self.args, self.keep, self.scaled, self.trace = (suffix, args, keep, scaled,
                                                                      trace)

    def attrs(self):
        """What a rollout launcher exposes of it: push_amp on every form, trace_dv if traced."""
        amp = self.scaled if self.suffix == "_pushed" else None
        return dict(push_amp=amp, **({} if self.trace is None else {"trace_dv": self.scaled}))


# what Plan._out raises for a state history and for a metrics tensor
_HIST_MSG = "hist must be a contiguous float64 [B, n, 2, 3] tensor on the plan's device"
_METRICS_MSG = (f"out must be a contiguous float64 [B, {_native.NMETRICS}] tensor on the plan's "
                "device")


def _device_index(backend: str) -> int:
    if not torch.cuda.is_available():
        raise RuntimeError("the ZMP-MPC solver needs a HIP device (torch.cuda.is_available() is "
                           "False); there is no CPU fallback")
    if backend in ("hip", "cuda", None):
        return torch.cuda.current_device()
    for prefix in ("hip:", "cuda:"):
        if backend.startswith(prefix):
            return int(backend[len(prefix):])
    raise ValueError(f"unknown backend {backend!r} (expected 'hip' or 'hip:<index>')")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _ints(a, dtype, device):
    """Support states (np.int8) or step counts (np.int32) as a contiguous tensor of that type on
    the device; a tensor is converted where it is, never through the host."""
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a, dtype=dtype)
    return torch.as_tensor(a, dtype=getattr(torch, np.dtype(dtype).name),
                           device=device).contiguous()


class Plan:
    """Batch-invariant solver plan for one (N, dt, h, g, Q, R, strict) on one device."""

    def __init__(self, device: int, N: int, dt: float, h: float, g: float, Q: float, R: float,
                 strict: bool):
        lib = _native.load()
        self.device = int(device)
        self._device = torch.device("cuda", self.device)
        self.N = int(N)
        self.dt, self.h, self.g, self.Q, self.R = float(dt), float(h), float(g), float(Q), float(R)
        self.strict = bool(strict)
        c = plan_constants(self.dt, self.h, self.g)
        self.consts = c
        handle = ctypes.c_void_p()
        _native.call("zmpc_plan_create", self.device, self.device, self.N, c["T"], c["T2_2"],
                     c["T3_6"], c["hg"], c["Thg"], self.Q, self.R, int(self.strict),
                     after=(ctypes.byref(handle),))
        self._h = handle
        self._finalizer = weakref.finalize(self, lib.zmpc_plan_destroy, handle)

    @property
    def handle(self):
        return self._live()

    def _live(self):
        if self._h is None:
            raise RuntimeError("plan was destroyed")
        return self._h

    def destroy(self):
        """Free the device plan now (zmpc_plan_destroy) instead of at garbage collection; the
        object is unusable afterwards.  Idempotent."""
        if self._h is not None:
            self._finalizer()
            self._h = None

    def export(self, what: int) -> np.ndarray:
        """A plan quantity on the host (zmpc_plan_export, ids _native.EXPORT_*, table
        _native.EXPORTS).  Matrices come back [N, N], Px [N, 3], the fast-FIR taps [rows, 4], the
        FFT tables complex."""
        entry = _native.EXPORTS.get(what)
        if entry is None:
            raise ValueError(f"zmpc_plan_export: unknown export id {what}")
        _, count, shape = entry
        n = count(self.N)
        buf = np.empty(n, dtype=np.float64)
        rc = _native.load().zmpc_plan_export(
            self._live(), what, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n)
        _native.check(rc, "zmpc_plan_export")
        if shape is complex:
            return buf.view(np.complex128)
        return buf if shape is None else buf.reshape(shape(self.N))

    def counters(self, reset: bool = False) -> dict:
        """Active-set solver work counters (zmpc_plan_counters, include/zmpc.h), summed over this
        plan's launches since creation or the last reset; synchronises the device.  Strict
        solver: wave_passes .. launches; Herdt solver: the herdt_* keys."""
        buf = (ctypes.c_uint64 * _native.NCOUNTERS)()
        rc = _native.load().zmpc_plan_counters(self._live(), buf, _native.NCOUNTERS, int(reset))
        _native.check(rc, "zmpc_plan_counters")
        return {name: int(v) for name, v in zip(_native.COUNTER_NAMES, buf)}

    def set_option(self, option, value: int) -> "Plan":
        """zmpc_plan_set_option: choose between forms that compute the same solution (cross-checks
        and A/B timing).  option: a name of _native.OPTIONS ("correlation", "long_walk",
        "rollout_kernel", "kick_order", "strict_solver", "strict_bounds") or its ZMPC_OPT_* number."""
        opt = _native.OPTIONS[option] if isinstance(option, str) else int(option)
        rc = _native.load().zmpc_plan_set_option(self._live(), opt, int(value))
        _native.check(rc, "zmpc_plan_set_option")
        return self

    def get_option(self, option) -> int:
        opt = _native.OPTIONS[option] if isinstance(option, str) else int(option)
        v = ctypes.c_int64()
        rc = _native.load().zmpc_plan_get_option(self._live(), opt, ctypes.byref(v))
        _native.check(rc, "zmpc_plan_get_option")
        return int(v.value)

    def timings(self) -> dict:
        """Plan-build stage durations in ms (zmpc_plan_timings; HIP events on the creation
        stream): name → ms, names as _native.PLAN_STAGE_NAMES."""
        buf = (ctypes.c_float * _native.PLAN_STAGES)()
        rc = _native.load().zmpc_plan_timings(self._live(), buf, _native.PLAN_STAGES)
        _native.check(rc, "zmpc_plan_timings")
        return {name: float(buf[i]) for i, name in enumerate(_native.PLAN_STAGE_NAMES)}

    # -- checked arguments: each rule of the launch methods, stated once --------------------
    def _as_dev(self, a, shape=None):
        t = torch.as_tensor(a, dtype=torch.float64, device=self._device)
        t = t.contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def _x0(self, x0):
        """Initial states on the device and the batch size they set: (x0 [B, 2, 3], B)."""
        x0 = self._as_dev(x0)
        if x0.dim() != 3 or x0.shape[1:] != (2, 3):
            raise ValueError(f"x0 must be [B, 2, 3], got {tuple(x0.shape)}")
        return x0, int(x0.shape[0])

    def _hist_dims(self, hist):
        """(B, n) of a state history: a contiguous float64 [B, n, 2, 3] tensor on the plan's
        device with n >= 1, which is never copied."""
        if not isinstance(hist, torch.Tensor) or hist.dim() != 4 or hist.shape[2:] != (2, 3) \
                or hist.dtype != torch.float64 or hist.device != self._device \
                or not hist.is_contiguous():
            raise ValueError(_HIST_MSG)
        if hist.shape[1] < 1:
            raise ValueError("hist must hold at least one sample per walk")
        return int(hist.shape[0]), int(hist.shape[1])

    def _out(self, t, shape, dtype, msg):
        """An output to write into: t if it is a contiguous `dtype` tensor of `shape` on the
        plan's device (ValueError(msg) otherwise), a new one for None."""
        if t is None:
            return torch.empty(shape, dtype=dtype, device=self._device)
        if tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != self._device or \
                not t.is_contiguous():
            raise ValueError(msg)
        return t

    def _bounds(self, zmax, zmin, B, n=None):
        """CoP bounds on the device → (zmax, zmin, stride between walks): [B, n, 2] per walk
        (stride 2n), or [n, 2] one CoP shared by every walk (stride 0).  With n, both B and n are
        a history's and the message names them; n None: a rollout's bounds, which set n
        themselves (B is x0's)."""
        zmax = self._as_dev(zmax)
        if n is not None:
            shape = (n, 2) if zmax.dim() == 2 else (B, n, 2)
            if tuple(zmax.shape) != shape:
                raise ValueError(f"z_max must be [B, n, 2] = [{B}, {n}, 2] or [n, 2], got "
                                 f"{tuple(zmax.shape)}")
        elif (zmax.dim() == 2 and zmax.shape[1] == 2) or \
                (zmax.dim() == 3 and zmax.shape[2] == 2 and zmax.shape[0] == B):
            shape = tuple(zmax.shape)
        else:
            raise ValueError(f"z_max must be [B, n, 2] or [n, 2], got {tuple(zmax.shape)}")
        return zmax, self._as_dev(zmin, shape), 0 if zmax.dim() == 2 else 2 * shape[1]

    def _index(self, a, B, name, sized=True):
        """An optional [B] index array as an int64 tensor on the device (None stays None).
        Raises e.g. "lengths must be [B] = [4], got (3,)"; sized=False leaves the "= [4]" out."""
        if a is None:
            return None
        t = torch.as_tensor(a, dtype=torch.int64, device=self._device).contiguous()
        if tuple(t.shape) != (B,):
            raise ValueError(f"{name} must be [B]{f' = [{B}]' if sized else ''}, got "
                             f"{tuple(t.shape)}")
        return t

    def _kick(self, kick, kick_step, B):
        """The one-sample y kick as the C-ABI takes it: (kick [B] tensor or None, scalar step,
        per-walk steps).  kick_step an int: (.., step, None); a [B] array: (.., −1, tensor)."""
        kick_t = None if kick is None else self._as_dev(kick, (B,))
        if isinstance(kick_step, (int, np.integer)):
            return kick_t, int(kick_step), None
        return kick_t, -1, self._index(kick_step, B, "per-walk kick_step", sized=False)

    def _disturbance(self, kick, kick_step, push, trace, mass, B, kicks=True):
        """The one disturbance of B walks as the C-ABI takes it → _Disturbance: the one-sample y
        kick (kick [B] or None at kick_step; kicks=False for a call without that form), an
        analysis.Push or an analysis.PushTrace, each of which excludes the others.  Amplitudes and
        a trace in newtons need the robot's mass (the plan holds dt, not m); velocity steps on the
        plan's device are used as they are, without a copy."""
        from .analysis import AXES, Push, PushTrace
        if kicks and push is None and trace is None:
            kick_t, step, ks = self._kick(kick, kick_step, B)
            if ks is None:
                return _Disturbance("", (_ptr(kick_t), step), (kick_t,), kick_t)
            return _Disturbance("_kicks", (_ptr(kick_t), _ptr(ks)), (kick_t, ks), kick_t)
        if trace is not None and (kick is not None or push is not None):
            raise ValueError("give either trace or a kick or push, not both")
        if kick is not None:
            raise ValueError("give either kick or push, not both")
        what, kind, src = ("push", Push, push) if push is not None else ("trace", PushTrace, trace)
        if not isinstance(src, kind):
            raise ValueError(f"{what} must be an analysis.{kind.__name__}, got "
                             f"{type(src).__name__}")
        newtons = push is not None or trace.unit != "m/s"
        if newtons and (mass is None or not (float(mass) > 0) or not np.isfinite(float(mass))):
            raise ValueError("a push needs the robot's mass in kg (mass=), finite and positive"
                             if push is not None else "a trace in newtons needs the robot's mass "
                             "in kg (mass=), finite and positive")
        dev = self._device

        def start():  # the start step(s) as (scalar, [B] tensor): one of the two holds them
            if isinstance(src.step, int):
                return src.step, None
            return -1, torch.as_tensor(np.broadcast_to(src.step, (B,)).copy(), device=dev)
        # (the arguments hold the struct's address: it lives in what the caller keeps)
        if push is None:
            dv = trace.dv(self.dt, None if mass is None else float(mass), B)
            dv = torch.as_tensor(dv, dtype=torch.float64, device=dev).contiguous()
            step, steps = start()
            c = _native.ZmpcTrace(dv.data_ptr(), AXES[trace.axes], _ptr(steps), step,
                                  trace.length, None)
            return _Disturbance("_traced", (ctypes.addressof(c),), (c, (dv, steps)), dv, c)
        amp = torch.as_tensor(push.amplitudes(self.dt, float(mass), B), device=dev)
        prof = None if push.profile is None else torch.as_tensor(push.profile, device=dev)
        step, steps = start()
        c = _native.ZmpcPush(amp.data_ptr(), AXES[push.axes], _ptr(steps), step, _ptr(prof),
                             push.duration)
        return _Disturbance("_pushed", (ctypes.addressof(c),), (c, (amp, steps, prof)), amp)

    # -- launches --------------------------------------------------------------------------
    def _launcher(self, name, args, trace=None, **attrs):
        """A zero-argument callable that re-issues name(*args, current stream) and carries
        attrs.  One launch is one stream lookup and one ctypes call: no device context, no
        argument work, and _native.check only on a nonzero return.  trace: the ZmpcTrace among
        args of a call that takes its stream there — one launch is then one stream lookup, one
        store into the struct and one ctypes call."""
        fn = getattr(_native.load(), name)
        dev = self.device

        def launch():
            stream = torch.cuda.current_stream(dev).cuda_stream
            rc = fn(*args, ctypes.c_void_p(stream))
            if rc != 0:
                _native.check(rc, name)

        def launch_traced():
            trace.stream = torch.cuda.current_stream(dev).cuda_stream
            rc = fn(*args)
            if rc != 0:
                _native.check(rc, name)
        if trace is not None:
            launch = launch_traced
        launch.__dict__.update(attrs)
        return launch

    def step(self, x, zmax_win, zmin_win, status=None):
        """Batched predict_wieber_axis: x [B,3], windows [B,N] → x_next [B,3] (device)."""
        x = self._as_dev(x)
        B = x.shape[0]
        zmax_win = self._as_dev(zmax_win, (B, self.N))
        zmin_win = self._as_dev(zmin_win, (B, self.N))
        x = x.reshape(B, 3)
        out = torch.empty((B, 3), dtype=torch.float64, device=self._device)
        st = status if status is not None else torch.empty(B, dtype=torch.int32,
                                                           device=self._device)
        _native.call("zmpc_step", self.device, self._live(), B, _ptr(x), _ptr(zmax_win),
                     _ptr(zmin_win), _ptr(out), _ptr(st))
        return out, st

    def rollout_launcher(self, zmax, zmin, x0, kick=None, kick_step=-1, hist=None, status=None,
                         push=None, mass=None, trace=None):
        """Validate once and return a zero-argument callable that re-issues the same rollout
        launch on the current stream (one ctypes call, no tensor checks): for timing loops
        and graph capture.  The tensors must stay alive while the launcher is used.  push, mass:
        as rollout; launch.push_amp is then the [B, C] amplitude tensor the launch reads (write
        new amplitudes into it between launches, as critical_force does).  trace: an
        analysis.PushTrace instead; launch.trace_dv is then the [B, L, C] tensor of velocity steps
        the launch reads."""
        hist, status, name, args, walks, d = self._rollout_args(zmax, zmin, x0, kick, kick_step,
                                                                hist, status, push, mass, trace)
        # (inputs: the walks, then what the disturbance's arguments point to; a traced launch
        # shows the _Disturbance itself, one entry)
        return self._launcher(name, args, d.trace, hist=hist, status=status,
                              inputs=walks + (d.keep if d.trace is None else (d,)), **d.attrs())

    def rollout(self, zmax, zmin, x0, kick=None, kick_step=-1, hist=None, status=None,
                push=None, mass=None, trace=None):
        """Batched Wieber rollout → hist [B,n,2,3] (device), status [B] (see _rollout_args).
        push: an analysis.Push — a shove of any length, shape and direction instead of the
        one-sample y kick (zmpc_rollout_pushed; not together with kick); mass: the robot's mass
        in kg, needed with push.  trace: an analysis.PushTrace — a disturbance per walk, sample
        and axis (zmpc_rollout_traced; not together with kick or push); mass is needed when the
        trace is in newtons."""
        hist, status, name, args, _, d = self._rollout_args(zmax, zmin, x0, kick, kick_step, hist,
                                                            status, push, mass, trace)
        _native.call(name, self.device, *args, trace=d.trace)
        return hist, status

    def _walk_inputs(self, zmax, zmin, x0):
        """The walks of a rollout on the device: (zmax, zmin, x0, B, n, bounds stride)."""
        x0, B = self._x0(x0)
        zmax, zmin, bstride = self._bounds(zmax, zmin, B)
        return zmax, zmin, x0, B, int(zmax.shape[-2]), bstride

    def _rollout_args(self, zmax, zmin, x0, kick, kick_step, hist, status, push=None, mass=None,
                      trace=None):
        """Batched Wieber rollout → hist [B,n,2,3] (device), status [B].

        zmax/zmin: [B,n,2] per-walk CoP bounds, or [n,2] one CoP shared by every walk;
        x0: [B,2,3]; kick: [B] velocity impulse subtracted from y at step kick_step — an int,
        or a [B] array of per-walk steps (ragged walks: zmpc_rollout_kicks).
        Returns (hist, status, symbol, its arguments without the stream, the walks' tensors, the
        _Disturbance: a traced symbol takes the stream in its struct, no stream argument follows).
        """
        zmax, zmin, x0, B, n, bstride = self._walk_inputs(zmax, zmin, x0)
        hist = self._out(hist, (B, n, 2, 3), torch.float64, _HIST_MSG)
        if status is None:
            status = torch.empty(B, dtype=torch.int32, device=self._device)
        d = self._disturbance(kick, kick_step, push, trace, mass, B)
        args = (self._live(), B, n, _ptr(zmax), _ptr(zmin), bstride, _ptr(x0), *d.args,
                _ptr(hist), _ptr(status))
        return hist, status, "zmpc_rollout" + d.suffix, args, (zmax, zmin, x0), d

    def walk_metrics(self, hist, zmax, zmin, lengths=None, out=None):
        """Per-walk robustness metrics of a state history (zmpc_walk_metrics, include/zmpc.h)
        → [B, 12] device tensor, slot 2k + a = quantity k (analysis.SLOT_NAMES) of axis a.

        hist: a contiguous float64 [B, n, 2, 3] tensor on the plan's device (a rollout's
        output; it is never copied); zmax/zmin: [B, n, 2] per-walk CoP bounds, or [n, 2] one
        CoP shared by every walk; lengths: [B] live samples of ragged walks (1 <= n_b <= n) or
        None; out: a contiguous float64 [B, 12] tensor on the plan's device to write into.
        Asynchronous on the current stream.  Works on any plan: only h/g is read.
        """
        B, n = self._hist_dims(hist)
        zmax, zmin, bstride = self._bounds(zmax, zmin, B, n)
        len_t = self._index(lengths, B, "lengths")
        out = self._out(out, (B, _native.NMETRICS), torch.float64, _METRICS_MSG)
        _native.call("zmpc_walk_metrics", self.device, self._live(), B, n, _ptr(hist),
                     _ptr(zmax), _ptr(zmin), bstride, _ptr(len_t), _ptr(out))
        return out

    # -- push-robustness map (zmpc_push_map) -----------------------------------------------
    def push_map(self, hist, zmax, zmin, lengths=None, push_steps=None, max_violation=1e-9,
                 out=None, want_response=False, *, mass, duration=1, profile=None, axes="y"):
        """Exact critical push of every (walk, push step, direction) from an unpushed state
        history (zmpc_push_map, include/zmpc.h) → (force, limit) device tensors, with
        want_response=True (force, limit, response [n]).

        duration, profile, axes (zmpc_push_map_shaped; at their defaults the call is
        zmpc_push_map's): a push that lasts `duration` samples with force F·profile[j] during
        history steps s + j (profile None: constant; a finite host array of `duration` weights,
        or a float64 [duration] tensor on the plan's device, which is not inspected); axes "x",
        "y" or "xy" — the last dimension of force and limit is then (+x, −x), (+y, −y) or
        (+x, −x, +y, −y), and response is the shaped table.

        hist, zmax, zmin, lengths: as walk_metrics.  push_steps None: the full map, force float64
        and limit int32 [B, n, 2] ([..., 0] a +y push, [..., 1] a −y push at step s); push_steps
        [B]: the single-step form, [B, 2] for that step of each walk.  mass: the robot's mass in
        kg (the plan does not hold it).  out: a (force, limit) pair of contiguous tensors of
        those shapes on the plan's device to write into.  Asynchronous on the current stream.
        Non-strict plans only: a strict plan raises NativeError (ZMPC_ESTATE), as does a full map
        of walks longer than the kernel's LDS holds (10112 samples)."""
        dev = self._device
        B, n = self._hist_dims(hist)
        zmax, zmin, bstride = self._bounds(zmax, zmin, B, n)
        len_t = self._index(lengths, B, "lengths")
        steps_t = self._index(push_steps, B, "push_steps")
        from .analysis import AXES, check_profile
        if axes not in AXES:
            raise ValueError(f"axes must be 'x', 'y' or 'xy', got {axes!r}")
        if isinstance(profile, torch.Tensor):
            D, _ = check_profile(duration, None)
            if profile.dtype != torch.float64 or profile.device != dev or \
                    tuple(profile.shape) != (D,) or not profile.is_contiguous():
                raise ValueError(f"a device profile must be a contiguous float64 [duration] = "
                                 f"[{D}] tensor on the plan's device")
            prof_t = profile
        else:
            D, w = check_profile(duration, profile)
            prof_t = None if w is None else torch.as_tensor(w, device=dev)
        C = 4 if axes == "xy" else 2
        oshape = (B, n, C) if steps_t is None else (B, C)
        force, limit = (None, None) if out is None else out
        msg = out is not None and (f"out must be (float64, int32) contiguous {oshape} tensors "
                                   "on the plan's device")
        force = self._out(force, oshape, torch.float64, msg)
        limit = self._out(limit, oshape, torch.int32, msg)
        resp = torch.empty(n, dtype=torch.float64, device=dev) if want_response else None
        walks = (self._live(), B, n, _ptr(hist), _ptr(zmax), _ptr(zmin), bstride, _ptr(len_t),
                 _ptr(steps_t))
        outs = (float(max_violation), float(mass), _ptr(force), _ptr(limit), _ptr(resp))
        if D != 1 or prof_t is not None or axes != "y":
            _native.call("zmpc_push_map_shaped", self.device, *walks, _ptr(prof_t), D,
                         AXES[axes], *outs)
        else:
            _native.call("zmpc_push_map", self.device, *walks, *outs)
        return (force, limit, resp) if want_response else (force, limit)

    # -- trace margin (zmpc_trace_margin) --------------------------------------------------
    def trace_margin(self, hist, zmax, zmin, trace, draws=1, lengths=None, max_violation=1e-9,
                     mass=None, scale=None, limit=None):
        """Exact critical scale of every (walk, draw) row's trace from an unpushed state history
        (zmpc_trace_margin, include/zmpc.h) → (scale [B, K, 2] float64, limit [B, K, 2] int32) on
        the device.  scale[b, k, 0] is the largest multiple of draw k's trace walk b survives,
        [..., 1] that of the negated trace; limit holds 2·i + a of the sample and axis that leaves
        first, −1 where none does (+inf) or the walk fails undisturbed (NaN).

        hist, zmax, zmin, lengths: as walk_metrics.  trace: an analysis.PushTrace of B·draws rows,
        row b·draws + k the k-th draw of walk b (ValueError when trace.batch() != B·draws); a
        trace in newtons needs mass, as rollout.  scale, limit: contiguous tensors of those shapes
        on the plan's device to write into.  Asynchronous on the current stream.  Non-strict
        plans only: a strict plan raises NativeError (ZMPC_ESTATE)."""
        B, n = self._hist_dims(hist)
        if isinstance(draws, bool) or not isinstance(draws, (int, np.integer)) or draws < 1:
            raise ValueError(f"draws must be an integer >= 1, got {draws!r}")
        K = int(draws)
        zmax, zmin, bstride = self._bounds(zmax, zmin, B, n)
        len_t = self._index(lengths, B, "lengths")
        from .analysis import PushTrace
        if isinstance(trace, PushTrace) and trace.batch() != B * K:
            raise ValueError(f"the trace holds {trace.batch()} rows, B·draws = {B}·{K} = {B * K} "
                             "are needed (row b·draws + k is draw k of walk b)")
        d = self._disturbance(None, -1, None, trace, mass, B * K, kicks=False)
        msg = (f"scale and limit must be (float64, int32) contiguous {(B, K, 2)} tensors on the "
               "plan's device")
        scale = self._out(scale, (B, K, 2), torch.float64, msg)
        limit = self._out(limit, (B, K, 2), torch.int32, msg)
        _native.call("zmpc_trace_margin", self.device, self._live(), B, n, _ptr(hist), _ptr(zmax),
                     _ptr(zmin), bstride, _ptr(len_t), K, *d.args, float(max_violation),
                     _ptr(scale), _ptr(limit), trace=d.trace)
        return scale, limit

    # -- fused rollout-to-metrics (zmpc_rollout_metrics) -----------------------------------
    def _rollout_metrics_args(self, zmax, zmin, x0, kick, kick_step, lengths, out, status):
        zmax, zmin, x0, B, n, bstride = self._walk_inputs(zmax, zmin, x0)
        kick_t, step, ks = self._kick(kick, kick_step, B)
        len_t = self._index(lengths, B, "lengths")
        out = self._out(out, (B, _native.NMETRICS), torch.float64, _METRICS_MSG)
        if status is None:
            status = torch.empty(B, dtype=torch.int32, device=self._device)
        args = (self._live(), B, n, _ptr(zmax), _ptr(zmin), bstride, _ptr(x0), _ptr(kick_t), step,
                _ptr(ks), _ptr(len_t), _ptr(out), _ptr(status))
        return out, status, args, (zmax, zmin, x0, kick_t, ks, len_t)

    def rollout_metrics_launcher(self, zmax, zmin, x0, kick=None, kick_step=-1, lengths=None,
                                 out=None, status=None):
        """rollout_launcher's counterpart for the fused launch: validate once and return a
        zero-argument callable that re-issues zmpc_rollout_metrics on the current stream
        (launch.metrics, launch.status are its outputs).  Fused only: a shape without a fused
        form raises NativeError at the first call."""
        out, status, args, keep = self._rollout_metrics_args(zmax, zmin, x0, kick, kick_step,
                                                             lengths, out, status)
        return self._launcher("zmpc_rollout_metrics", args, metrics=out, status=status,
                              inputs=keep)

    def rollout_metrics(self, zmax, zmin, x0, kick=None, kick_step=-1, lengths=None, out=None,
                        status=None, fused_only=False):
        """Batched Wieber rollout reduced to the walk metrics in one launch
        (zmpc_rollout_metrics): (metrics [B,12], status [B]) on the device, what walk_metrics
        returns for rollout's history of the same arguments, with no [B,n,2,3] history in between.

        Arguments as rollout (zmax/zmin [B,n,2] or a shared [n,2]; x0 [B,2,3]; kick [B];
        kick_step an int or a [B] array of per-walk steps) and walk_metrics (lengths [B] or None;
        out a [B,12] tensor to write into).  Where the library has no fused form — strict plans,
        walks of more than 513 samples, the one-wave cross-check kernel — it answers ZMPC_ESTATE
        and this method runs rollout + walk_metrics instead (the same figures, with the history as
        a temporary); fused_only=True raises NativeError there."""
        out, status, args, keep = self._rollout_metrics_args(zmax, zmin, x0, kick, kick_step,
                                                             lengths, out, status)
        rc = _native.call("zmpc_rollout_metrics", self.device, *args, raises=False)
        if rc == _native.ZMPC_ESTATE and not fused_only:
            zmax_t, zmin_t, x0_t, kick_t, _, len_t = keep
            hist, status = self.rollout(zmax_t, zmin_t, x0_t, kick=kick_t, kick_step=kick_step,
                                        status=status)
            return self.walk_metrics(hist, zmax_t, zmin_t, lengths=len_t, out=out), status
        _native.check(rc, "zmpc_rollout_metrics")
        return out, status

    # -- Herdt joint footstep QP (zmpc_herdt_rollout / zmpc_herdt_step) --------------------
    def _herdt_rollout_args(self, params, v_ref, states, nb_next, x0, kick, kick_step, push, mass,
                            hist=None, foot=None, status=None, trace=None):
        """The checked arguments of one Herdt rollout → (hist, foot, status, symbol, its arguments
        without the stream, the walks' tensors, the _Disturbance); hist, foot, status: tensors to
        write into, or None for new ones."""
        x0, B = self._x0(x0)
        v = self._as_dev(v_ref)
        if v.dim() not in (2, 3) or v.shape[-1] != 2:
            raise ValueError(f"v_ref must be [B, n, 2] or [n, 2], got {tuple(v.shape)}")
        n = int(v.shape[-2])
        if v.dim() == 2:
            vs = 0
        elif v.shape[0] == B:
            vs = 2 * n
        else:
            raise ValueError(f"v_ref must be [B, n, 2] or [n, 2], got {tuple(v.shape)}")
        # per-walk [B, n] or shared [n]: a 2-D array must carry one row per walk (the kernel
        # reads row b of walk b)
        st, ss = self._states(states, B, n)
        nb = _ints(nb_next, np.int32, self._device)
        if tuple(nb.shape) not in ((n,), (B, n)):
            raise ValueError(f"nb_next must be [B, n] = [{B}, {n}] or [n], got {tuple(nb.shape)}")
        ns = 0 if nb.dim() == 1 else n
        kick_t = None if kick is None else self._as_dev(kick, (B,))
        hist = self._out(hist, (B, n, 2, 3), torch.float64, _HIST_MSG)
        foot = self._out(foot, (B, n, 2), torch.float64,
                         "foot must be a contiguous float64 [B, n, 2] tensor on the plan's device")
        status = self._out(status, (B,), torch.int32,
                           "status must be a contiguous int32 [B] tensor on the plan's device")
        step = int(kick_step) if push is None and trace is None else -1  # (no per-walk form)
        d = self._disturbance(kick_t, step, push, trace, mass, B)
        args = (self._live(), ctypes.addressof(params), B, n, _ptr(v), vs, _ptr(st), ss, _ptr(nb),
                ns, _ptr(x0), *d.args, _ptr(hist), _ptr(foot), _ptr(status))
        return (hist, foot, status, "zmpc_herdt_rollout" + d.suffix, args,
                (params, v, st, nb, x0, kick_t), d)

    def herdt_rollout(self, params, v_ref, states, nb_next, x0, kick=None, kick_step=-1,
                      push=None, mass=None, trace=None):
        """Batched generate_com_trajectory_herdt → (hist [B,n,2,3], foot [B,n,2], status [B]).

        v_ref [B,n,2] or a shared [n,2]; states [B,n] or [n] int8 codes; nb_next [B,n] or [n]
        int32 (find_nb_steps of the padded states, first element); x0 [B,2,3]; kick [B] or
        None: y-velocity impulse at kick_step.  params: controllers.herdt.HerdtParams.
        push: an analysis.Push instead of the kick (zmpc_herdt_rollout_pushed), with mass in kg.
        trace: an analysis.PushTrace instead of either (zmpc_herdt_rollout_traced).
        """
        hist, foot, status, name, args, _, d = self._herdt_rollout_args(
            params, v_ref, states, nb_next, x0, kick, kick_step, push, mass, trace=trace)
        _native.call(name, self.device, *args, trace=d.trace)
        return hist, foot, status

    def herdt_rollout_launcher(self, params, v_ref, states, nb_next, x0, push=None, mass=None,
                               hist=None, foot=None, status=None, trace=None):
        """rollout_launcher's counterpart for pushed Herdt walks: validate once and return a
        zero-argument callable that re-issues zmpc_herdt_rollout_pushed on the current stream.
        launch.hist, launch.foot, launch.status are its outputs, launch.states the int8 states on
        the device and launch.push_amp the [B, C] amplitude tensor the launch reads (write new
        amplitudes into it between launches, as critical_force_herdt does).  trace: an
        analysis.PushTrace instead of push (zmpc_herdt_rollout_traced); launch.trace_dv is then
        the [B, L, C] tensor of velocity steps the launch reads."""
        hist, foot, status, name, args, walks, d = self._herdt_rollout_args(
            params, v_ref, states, nb_next, x0, None, -1, push, mass, hist, foot, status, trace)
        _, _, st, *_ = walks
        # (inputs: the walks, the struct, then the tensors it points to; a traced launch shows
        # the _Disturbance itself there)
        return self._launcher(name, args, d.trace, hist=hist, foot=foot, status=status,
                              inputs=walks + (d.keep if d.trace is None else (d.trace, d)),
                              states=st, **d.attrs())

    def _states(self, states, B, n):
        """Support states on the device → (int8 tensor, stride in bytes between walks): [B, n]
        per walk (stride n) or a shared [n] (stride 0)."""
        st = _ints(states, np.int8, self._device)
        if tuple(st.shape) not in ((n,), (B, n)):
            raise ValueError(f"states must be [B, n] = [{B}, {n}] or [n], got {tuple(st.shape)}")
        return st, (0 if st.dim() == 1 else n)

    def herdt_prepare(self, states, lengths=None):
        """Footstep bookkeeping of a batch of Herdt walks on the device (zmpc_herdt_prepare,
        include/zmpc.h) → (states int8 [B, n], nb_next int32 [B, n], max_steps int32 [B],
        max_footsteps int): what herdt_rollout takes as states and nb_next, the most footsteps in
        one horizon window of each walk, and of the batch (HerdtParams.max_footsteps).

        states: [B, n] support codes of B different walks, or a shared [n] (NumPy or a tensor; a
        tensor on the plan's device is never copied to the host); lengths: [B] live samples of
        ragged walks or None — walk b is then its own n_b samples padded with its last live state,
        whatever rows n_b.. of the input hold.  A shared [n] input without lengths gives [n], [n]
        and [1]; with lengths [B] it is one schedule cut at B lengths.  Synchronous: the call
        waits for the device on entry and returns with every output complete."""
        st = _ints(states, np.int8, self._device)
        if st.dim() not in (1, 2) or st.shape[-1] < 1:
            raise ValueError(f"states must be [B, n] or [n] with n >= 1, got {tuple(st.shape)}")
        n = int(st.shape[-1])
        shared = st.dim() == 1
        if shared:
            B = 1 if lengths is None else int(np.shape(lengths)[0])
        else:
            B = int(st.shape[0])
        len_t = self._index(lengths, B, "lengths")
        clean = torch.empty((B, n), dtype=torch.int8, device=self._device)
        nb = torch.empty((B, n), dtype=torch.int32, device=self._device)
        steps = torch.empty(B, dtype=torch.int32, device=self._device)
        most = ctypes.c_int32(0)
        rc = _native.load().zmpc_herdt_prepare(self._live(), B, n, _ptr(st), 0 if shared else n,
                                               _ptr(len_t), _ptr(clean), _ptr(nb), _ptr(steps),
                                               ctypes.byref(most))
        _native.check(rc, "zmpc_herdt_prepare")
        if shared and lengths is None:
            clean, nb = clean[0], nb[0]
        return clean, nb, steps, int(most.value)

    def _herdt_walk_metrics_args(self, params, hist, foot, states, lengths, foot_ref, count_tol,
                                 out):
        """The checked arguments of zmpc_herdt_walk_metrics → (out, its arguments without the
        stream, what they point to)."""
        B, n = self._hist_dims(hist)
        nm = _native.NHERDT_METRICS
        if not isinstance(foot, torch.Tensor) or tuple(foot.shape) != (B, n, 2) \
                or foot.dtype != torch.float64 or foot.device != self._device \
                or not foot.is_contiguous():
            raise ValueError(f"foot must be a contiguous float64 [B, n, 2] = [{B}, {n}, 2] tensor "
                             "on the plan's device")
        st, ss = self._states(states, B, n)
        ref, rs = None, 0
        if foot_ref is not None:
            ref = self._as_dev(foot_ref)
            if tuple(ref.shape) not in ((n, 2), (B, n, 2)):
                raise ValueError(f"foot_ref must be [B, n, 2] = [{B}, {n}, 2] or [n, 2], got "
                                 f"{tuple(ref.shape)}")
            rs = 0 if ref.dim() == 2 else 2 * n
        len_t = self._index(lengths, B, "lengths")
        out = self._out(out, (B, nm), torch.float64,
                        f"out must be a contiguous float64 [B, {nm}] tensor on the plan's device")
        args = (self._live(), ctypes.addressof(params), B, n, _ptr(hist), _ptr(foot), _ptr(st), ss,
                _ptr(ref), rs, _ptr(len_t), float(count_tol), _ptr(out))
        return out, args, (params, hist, foot, st, ref, len_t)

    def herdt_walk_metrics(self, params, hist, foot, states, lengths=None, foot_ref=None,
                           count_tol=1e-9, out=None):
        """Per-walk survival metrics of a Herdt rollout (zmpc_herdt_walk_metrics, include/zmpc.h)
        → [B, 16] device tensor (analysis.HerdtWalkMetrics names the slots).

        params: controllers.herdt.HerdtParams (the foot dimensions, the spread and the facets are
        read); hist [B, n, 2, 3] and foot [B, n, 2]: herdt_rollout's outputs, contiguous float64
        tensors on the plan's device, never copied; states [B, n] or a shared [n] int8 codes, as
        the rollout took them; lengths [B] live samples or None; foot_ref [B, n, 2] or a shared
        [n, 2]: the feet of the nominal (unpushed) walk, or None; count_tol: the excursion above
        which a sample counts in viol_count; out: a contiguous float64 [B, 16] tensor on the
        plan's device to write into.  Asynchronous on the current stream; only h/g of the plan is
        read."""
        out, args, _ = self._herdt_walk_metrics_args(params, hist, foot, states, lengths, foot_ref,
                                                     count_tol, out)
        _native.call("zmpc_herdt_walk_metrics", self.device, *args)
        return out

    def herdt_walk_metrics_launcher(self, params, hist, foot, states, lengths=None, foot_ref=None,
                                    count_tol=1e-9, out=None):
        """Validate once and return a zero-argument callable that re-issues
        zmpc_herdt_walk_metrics on the current stream (launch.metrics is its output): for
        critical_force_herdt's loop and for timing.  The tensors must stay alive while the
        launcher is used; a foot_ref tensor on the device is read at every launch, so it may be
        filled after the launcher is made."""
        out, args, keep = self._herdt_walk_metrics_args(params, hist, foot, states, lengths,
                                                        foot_ref, count_tol, out)
        return self._launcher("zmpc_herdt_walk_metrics", args, metrics=out, inputs=keep)

    def herdt_step(self, params, x, v_win, s_win, current, foot, side):
        """Batched predict_herdt_joint: x [B,2,3], v_win [B,N,2], s_win [B,N] int8,
        current [B] int8, foot [B,2], side [B] int8 (0 left) → (x_next [B,2,3],
        first footstep [B,2] (NaN: none), status [B])."""
        x = self._as_dev(x)
        B = int(x.shape[0])
        dev = self._device
        v = self._as_dev(v_win, (B, self.N, 2))
        f = self._as_dev(foot, (B, 2))
        sw, cu, sd = (_ints(a, np.int8, dev).reshape(shape)
                      for a, shape in ((s_win, (B, self.N)), (current, (B,)), (side, (B,))))
        xn = torch.empty((B, 2, 3), dtype=torch.float64, device=dev)
        step = torch.empty((B, 2), dtype=torch.float64, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        _native.call("zmpc_herdt_step", self.device, self._live(), ctypes.byref(params), B,
                     _ptr(x), _ptr(v), _ptr(sw), _ptr(cu), _ptr(f), _ptr(sd), _ptr(xn), _ptr(step),
                     _ptr(status))
        return xn, step, status


def get_plan(config, device=None) -> Plan:
    """Cached plan for an MPCConfig (keyed on every field the hot path reads)."""
    dev = _device_index(getattr(config, "backend", "hip")) if device is None else int(device)
    key = (dev, int(config.horizon), float(config.dt), float(config.h), float(config.g),
           float(config.Q), float(config.R), bool(config.strict))
    # one lock over lookup, build and eviction: two threads that ask for the same configuration
    # at once get the same plan (not one build each, the loser's freed under its caller), and
    # the LRU bookkeeping never sees a key another thread has just evicted
    with _PLAN_CACHE_LOCK:
        p = _PLAN_CACHE.get(key)
        if p is not None and p._h is not None:
            _PLAN_CACHE.move_to_end(key)
            return p
        p = Plan(dev, key[1], key[2], key[3], key[4], key[5], key[6], key[7])
        _PLAN_CACHE[key] = p
        while len(_PLAN_CACHE) > PLAN_CACHE_MAX:
            # drop the cache's reference only: a caller still holding the plan keeps it alive,
            # the device memory is freed when the last reference goes (weakref finalizer)
            _PLAN_CACHE.popitem(last=False)
        return p


def clear_plan_cache(destroy: bool = False):
    """Empty get_plan's cache; with destroy=True also free every cached plan now (callers must
    not use those plans afterwards)."""
    with _PLAN_CACHE_LOCK:
        plans = list(_PLAN_CACHE.values())
        _PLAN_CACHE.clear()
    if destroy:
        for p in plans:
            p.destroy()
