"""ctypes binding of libzmpc.so, the C-ABI declared in ``include/zmpc.h``.

This is the only door to the solver: there is no CPU fallback.  If the shared library is
missing or a HIP device is absent, every solver entry point raises instead of computing
something else.
"""

import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZMPC_LIB", os.path.join(_HERE, "libzmpc.so"))

ABI_VERSION = 7  # include/zmpc.h ZMPC_ABI_VERSION this binding is written for
NCOUNTERS = 10   # include/zmpc.h ZMPC_NCOUNTERS
# zmpc_plan_counters' slots in order (include/zmpc.h)
COUNTER_NAMES = ("wave_passes", "instance_passes", "working_set_slots", "launches",
                 "herdt_wave_passes", "herdt_instance_passes", "herdt_footsteps",
                 "herdt_footsteps_sq", "max_passes_per_solve", "herdt_max_passes_per_solve")
PLAN_STAGES = 12  # include/zmpc.h ZMPC_PLAN_STAGES
PLAN_STAGE_NAMES = ("prediction", "gram_PuTPu", "cholesky", "gain", "scan", "fft_tables",
                    "strict_X", "strict_gram_G", "strict_Pu_inverse", "strict_gram_Hz",
                    "strict_lq_table", "total")
HERDT_MAX_FACETS = 16  # include/zmpc.h ZMPC_HERDT_MAX_FACETS
NMETRICS = 12    # include/zmpc.h ZMPC_NMETRICS
NHERDT_METRICS = 16  # include/zmpc.h ZMPC_NHERDT_METRICS

ZMPC_OK = 0
ZMPC_EINVAL = -1
ZMPC_EHIP = -2
ZMPC_ENOMEM = -3
ZMPC_ESTATE = -4

ST_MAXITER = 1
ST_NONFINITE = 2
ST_FACTOR = 4
ST_INFEASIBLE = 8

# sizes of the derived tables (csrc/zmpc_internal.h kScanDoubles; csrc/dispatch.h kFftPT,
# kFftPmin, kFftGComplex)
SCAN_DOUBLES = 2928
FFT_PT, FFT_PMIN = 8192, 256
FFT_G_COMPLEX = 2 * FFT_PT - FFT_PMIN



def kffa_rows(N: int) -> int:  # csrc/zmpc_internal.h kffa_rows
    return (N + 2) // 2 + 8


def ksum_rows(N: int) -> int:  # csrc/dispatch.h ksum_rows
    return N + 18


# zmpc_plan_export, id → (name: the id is EXPORT_<name>; doubles written, of N; what
# Plan.export returns: None the flat buffer, a shape of N, or complex for a complex128 view).
# From 8 on the derived tables (additive to ABI 7); X and V on strict plans only.
_vector, _square = (lambda N: N), (lambda N: (N, N))
EXPORTS = {
    0: ("P", _vector, None),
    1: ("PX", lambda N: 3 * N, lambda N: (N, 3)),
    2: ("M", lambda N: N * N, _square),
    3: ("K", _vector, None),
    4: ("KX", lambda N: 3, None),
    5: ("G", lambda N: N * N, _square),
    6: ("L", lambda N: N * N, _square),
    7: ("HZ", lambda N: N * N, _square),
    8: ("KFFA", lambda N: 4 * kffa_rows(N), lambda N: (-1, 4)),
    9: ("KSUM", ksum_rows, None),
    10: ("SCAN", lambda N: SCAN_DOUBLES, None),
    11: ("X", lambda N: N * N, _square),
    12: ("V", _vector, None),
    13: ("FFT_TW", lambda N: 2 * FFT_PT, complex),
    14: ("FFT_G", lambda N: 2 * FFT_G_COMPLEX, complex),
}
globals().update({"EXPORT_" + name: what for what, (name, _, _) in EXPORTS.items()})

# zmpc_plan_set_option (include/zmpc.h ZMPC_OPT_*): algorithm selection, same solutions
OPTIONS = {"correlation": 0, "long_walk": 1, "rollout_kernel": 2, "kick_order": 3,
           "strict_solver": 4, "strict_bounds": 5}

# every symbol include/zmpc.h declares, with (restype, argtypes).  _P: any pointer, host or
# device (device pointers travel as integers); _PD … _PP: typed host pointers
_C, _I, _L, _D, _P = (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_double,
                      ctypes.c_void_p)
_PD, _PF, _PL, _PU, _PP = (ctypes.POINTER(t) for t in (ctypes.c_double, ctypes.c_float,
                                                       ctypes.c_int64, ctypes.c_uint64, _P))
SIGNATURES = {
    "zmpc_abi_version": (_C, []),
    "zmpc_last_error": (ctypes.c_char_p, []),
    "zmpc_plan_create": (_C, [_C, _I, _D, _D, _D, _D, _D, _D, _D, _I, _P, _PP]),
    "zmpc_plan_destroy": (_C, [_P]),
    "zmpc_plan_export": (_C, [_P, _I, _PD, _L]),
    "zmpc_plan_counters": (_C, [_P, _PU, _I, _I]),
    "zmpc_plan_timings": (_C, [_P, _PF, _I]),
    "zmpc_plan_set_option": (_C, [_P, _I, _L]),
    "zmpc_plan_get_option": (_C, [_P, _I, _PL]),
    "zmpc_step": (_C, [_P, _L, _P, _P, _P, _P, _P, _P]),
    "zmpc_rollout": (_C, [_P, _L, _L, _P, _P, _L, _P, _P, _L, _P, _P, _P]),
    "zmpc_rollout_kicks": (_C, [_P, _L, _L, _P, _P, _L, _P, _P, _P, _P, _P, _P]),
    # ... x0, push (const zmpc_push*, a ZmpcPush passed byref), hist, status, stream
    "zmpc_rollout_pushed": (_C, [_P, _L, _L, _P, _P, _L, _P, _P, _P, _P, _P]),
    # ... x0, trace (const zmpc_trace*, a ZmpcTrace passed byref: it carries the stream), hist,
    # status
    "zmpc_rollout_traced": (_C, [_P, _L, _L, _P, _P, _L, _P, _P, _P, _P]),
    # plan, B, n, hist, zmax, zmin, bounds_stride, lengths, draws, trace (const zmpc_trace*: it
    # carries the stream), max_violation, scale, limit
    "zmpc_trace_margin": (_C, [_P, _L, _L, _P, _P, _P, _L, _P, _L, _P, _D, _P, _P]),
    "zmpc_walk_metrics": (_C, [_P, _L, _L, _P, _P, _P, _L, _P, _P, _P]),
    "zmpc_rollout_metrics": (_C, [_P, _L, _L, _P, _P, _L, _P, _P, _L, _P, _P, _P, _P, _P]),
    "zmpc_push_map": (_C, [_P, _L, _L, _P, _P, _P, _L, _P, _P, _D, _D, _P, _P, _P, _P]),
    # ... push_steps, profile, duration, axes, max_violation, mass, force, limit, response, stream
    "zmpc_push_map_shaped": (_C, [_P, _L, _L, _P, _P, _P, _L, _P, _P, _P, _L, _I, _D, _D, _P,
                                  _P, _P, _P]),
    "zmpc_cop_generate": (_C, [_C, _L, _P, _L, _P, _P, _P, _P, _P]),
    # params: const zmpc_herdt_params* (a ctypes.Structure passed byref)
    "zmpc_herdt_rollout": (_C, [_P, _P, _L, _L, _P, _L, _P, _L, _P, _L, _P, _P, _L, _P, _P, _P,
                                _P]),
    # ... x0, push (const zmpc_push*), hist, foot, status, stream
    "zmpc_herdt_rollout_pushed": (_C, [_P, _P, _L, _L, _P, _L, _P, _L, _P, _L, _P, _P, _P, _P,
                                       _P, _P]),
    # ... x0, trace (const zmpc_trace*), hist, foot, status
    "zmpc_herdt_rollout_traced": (_C, [_P, _P, _L, _L, _P, _L, _P, _L, _P, _L, _P, _P, _P, _P,
                                       _P]),
    # plan, B, n, states, s_stride, lengths, states_out, nb_next, max_steps, max_footsteps (host);
    # no stream: synchronous, called as zmpc_plan_export is
    "zmpc_herdt_prepare": (_C, [_P, _L, _L, _P, _L, _P, _P, _P, _P, ctypes.POINTER(_I)]),
    "zmpc_herdt_step": (_C, [_P, _P, _L, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    # params, B, n, hist, foot, states, s_stride, foot_ref, foot_ref_stride, lengths, count_tol,
    # metrics, stream
    "zmpc_herdt_walk_metrics": (_C, [_P, _P, _L, _L, _P, _P, _P, _L, _P, _L, _P, _D, _P, _P]),
}


class ZmpcPush(ctypes.Structure):
    """include/zmpc.h zmpc_push: the push window of zmpc_rollout_pushed and
    zmpc_herdt_rollout_pushed (device pointers as integers)."""
    _fields_ = [("amp", ctypes.c_void_p), ("axes", ctypes.c_int32), ("steps", ctypes.c_void_p),
                ("step", ctypes.c_int64), ("profile", ctypes.c_void_p),
                ("duration", ctypes.c_int64)]


class ZmpcTrace(ctypes.Structure):
    """include/zmpc.h zmpc_trace: the per-walk disturbance trace of zmpc_rollout_traced,
    zmpc_herdt_rollout_traced and zmpc_trace_margin (device pointers as integers).  The calls take
    their stream here."""
    _fields_ = [("dv", ctypes.c_void_p), ("axes", ctypes.c_int32), ("steps", ctypes.c_void_p),
                ("step", ctypes.c_int64), ("length", ctypes.c_int64),
                ("stream", ctypes.c_void_p)]


_lib = None
_lock = threading.Lock()


class NativeError(RuntimeError):
    """A libzmpc call failed (message from zmpc_last_error)."""


class DeviceOutOfMemory(NativeError, MemoryError):
    """ZMPC_ENOMEM: a plan or per-launch workspace allocation on the device failed."""


def load():
    """Load libzmpc.so once; raise with a build hint if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"libzmpc.so not found at {LIB_PATH}: build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C "
                "model-predictive-control-for-bipedal-locomotion_amd/csrc`).  There is no CPU "
                "fallback for the solver.")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def check(rc: int, what: str):
    if rc != ZMPC_OK:
        msg = load().zmpc_last_error().decode(errors="replace")
        if rc == ZMPC_EINVAL:
            raise ValueError(f"{what}: {msg}")
        if rc == ZMPC_ENOMEM:
            raise DeviceOutOfMemory(f"{what} failed ({rc}): {msg}")
        raise NativeError(f"{what} failed ({rc}): {msg}")


def call(name, device, *args, after=(), raises=True, trace=None):
    """One launch of a library symbol that takes a stream: enter HIP device `device`, call
    name(*args, torch's current stream there, *after) and run check on the result.
    raises=False hands the return code back unchecked.  trace: the ZmpcTrace among args of a
    symbol that takes its stream there; the stream is put into it and no stream argument is
    passed."""
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        if trace is None:
            args += (ctypes.c_void_p(stream),)
        else:
            trace.stream = stream
        rc = getattr(load(), name)(*args, *after)
    if raises:
        check(rc, name)
    return rc
