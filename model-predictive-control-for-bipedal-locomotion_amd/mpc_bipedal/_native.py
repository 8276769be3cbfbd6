"""ctypes binding of libzmpc.so, the C-ABI declared in ``include/zmpc.h``.

This is the only door to the solver: there is no CPU fallback.  If the shared library is
missing or a HIP device is absent, every solver entry point raises instead of computing
something else.
"""

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZMPC_LIB", os.path.join(_HERE, "libzmpc.so"))

ABI_VERSION = 7  # include/zmpc.h ZMPC_ABI_VERSION this binding is written for
NCOUNTERS = 10   # include/zmpc.h ZMPC_NCOUNTERS
PLAN_STAGES = 12  # include/zmpc.h ZMPC_PLAN_STAGES
PLAN_STAGE_NAMES = ("prediction", "gram_PuTPu", "cholesky", "gain", "scan", "fft_tables",
                    "strict_X", "strict_gram_G", "strict_Pu_inverse", "strict_gram_Hz",
                    "strict_lq_table", "total")
HERDT_MAX_FACETS = 16  # include/zmpc.h ZMPC_HERDT_MAX_FACETS
NMETRICS = 12    # include/zmpc.h ZMPC_NMETRICS

ZMPC_OK = 0
ZMPC_EINVAL = -1
ZMPC_EHIP = -2
ZMPC_ENOMEM = -3
ZMPC_ESTATE = -4

ST_MAXITER = 1
ST_NONFINITE = 2
ST_FACTOR = 4
ST_INFEASIBLE = 8

EXPORT_P, EXPORT_PX, EXPORT_M, EXPORT_K, EXPORT_KX, EXPORT_G, EXPORT_L, EXPORT_HZ = range(8)
# the derived tables (additive to ABI 7); X and V on strict plans only
(EXPORT_KFFA, EXPORT_KSUM, EXPORT_SCAN, EXPORT_X, EXPORT_V, EXPORT_FFT_TW,
 EXPORT_FFT_G) = range(8, 15)
# their sizes (csrc/zmpc_internal.h kffa_rows, kScanDoubles; csrc/dispatch.h ksum_rows, kFftPT,
# kFftPmin, kFftGComplex)
SCAN_DOUBLES = 2928
FFT_PT, FFT_PMIN = 8192, 256
FFT_G_COMPLEX = 2 * FFT_PT - FFT_PMIN


def kffa_rows(N: int) -> int:
    return (N + 2) // 2 + 8


def ksum_rows(N: int) -> int:
    return N + 18

# zmpc_plan_set_option (include/zmpc.h ZMPC_OPT_*): algorithm selection, same solutions
OPTIONS = {"correlation": 0, "long_walk": 1, "rollout_kernel": 2, "kick_order": 3,
           "strict_solver": 4, "strict_bounds": 5}

# every symbol include/zmpc.h declares, with (restype, argtypes)
_c_dbl_p = ctypes.c_void_p  # device pointers travel as integers
SIGNATURES = {
    "zmpc_abi_version": (ctypes.c_int, []),
    "zmpc_last_error": (ctypes.c_char_p, []),
    "zmpc_plan_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int32, ctypes.c_double,
                                        ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                        ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                        ctypes.c_int32, ctypes.c_void_p,
                                        ctypes.POINTER(ctypes.c_void_p)]),
    "zmpc_plan_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "zmpc_plan_export": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32,
                                        ctypes.POINTER(ctypes.c_double), ctypes.c_int64]),
    "zmpc_plan_counters": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
                                          ctypes.c_int32, ctypes.c_int32]),
    "zmpc_plan_timings": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float),
                                         ctypes.c_int32]),
    "zmpc_plan_set_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64]),
    "zmpc_plan_get_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32,
                                            ctypes.POINTER(ctypes.c_int64)]),
    "zmpc_step": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, _c_dbl_p, _c_dbl_p, _c_dbl_p,
                                 _c_dbl_p, ctypes.c_void_p, ctypes.c_void_p]),
    "zmpc_rollout": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, _c_dbl_p,
                                    _c_dbl_p, ctypes.c_int64, _c_dbl_p, _c_dbl_p, ctypes.c_int64,
                                    _c_dbl_p, ctypes.c_void_p, ctypes.c_void_p]),
    "zmpc_rollout_kicks": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                          _c_dbl_p, _c_dbl_p, ctypes.c_int64, _c_dbl_p, _c_dbl_p,
                                          ctypes.c_void_p, _c_dbl_p, ctypes.c_void_p,
                                          ctypes.c_void_p]),
    # ... x0, push (const zmpc_push*, a ZmpcPush passed byref), hist, status, stream
    "zmpc_rollout_pushed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                           _c_dbl_p, _c_dbl_p, ctypes.c_int64, _c_dbl_p,
                                           ctypes.c_void_p, _c_dbl_p, ctypes.c_void_p,
                                           ctypes.c_void_p]),
    "zmpc_walk_metrics": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                         _c_dbl_p, _c_dbl_p, _c_dbl_p, ctypes.c_int64,
                                         ctypes.c_void_p, _c_dbl_p, ctypes.c_void_p]),
    "zmpc_rollout_metrics": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                            _c_dbl_p, _c_dbl_p, ctypes.c_int64, _c_dbl_p, _c_dbl_p,
                                            ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                            _c_dbl_p, ctypes.c_void_p, ctypes.c_void_p]),
    "zmpc_push_map": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, _c_dbl_p,
                                     _c_dbl_p, _c_dbl_p, ctypes.c_int64, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_double, ctypes.c_double, _c_dbl_p,
                                     ctypes.c_void_p, _c_dbl_p, ctypes.c_void_p]),
    # ... push_steps, profile, duration, axes, max_violation, mass, force, limit, response, stream
    "zmpc_push_map_shaped": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                            _c_dbl_p, _c_dbl_p, _c_dbl_p, ctypes.c_int64,
                                            ctypes.c_void_p, ctypes.c_void_p, _c_dbl_p,
                                            ctypes.c_int64, ctypes.c_int32, ctypes.c_double,
                                            ctypes.c_double, _c_dbl_p, ctypes.c_void_p, _c_dbl_p,
                                            ctypes.c_void_p]),
    "zmpc_cop_generate": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, _c_dbl_p, ctypes.c_int64,
                                         _c_dbl_p, _c_dbl_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]),
    # params: const zmpc_herdt_params* (a ctypes.Structure passed byref)
    "zmpc_herdt_rollout": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                          ctypes.c_int64, _c_dbl_p, ctypes.c_int64,
                                          ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                          ctypes.c_int64, _c_dbl_p, _c_dbl_p, ctypes.c_int64,
                                          _c_dbl_p, _c_dbl_p, ctypes.c_void_p, ctypes.c_void_p]),
    # ... x0, push (const zmpc_push*), hist, foot, status, stream
    "zmpc_herdt_rollout_pushed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                 ctypes.c_int64, _c_dbl_p, ctypes.c_int64,
                                                 ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                 ctypes.c_int64, _c_dbl_p, ctypes.c_void_p,
                                                 _c_dbl_p, _c_dbl_p, ctypes.c_void_p,
                                                 ctypes.c_void_p]),
    "zmpc_herdt_step": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                       _c_dbl_p, _c_dbl_p, ctypes.c_void_p, ctypes.c_void_p,
                                       _c_dbl_p, ctypes.c_void_p, _c_dbl_p, _c_dbl_p,
                                       ctypes.c_void_p, ctypes.c_void_p]),
}


class ZmpcPush(ctypes.Structure):
    """include/zmpc.h zmpc_push: the push window of zmpc_rollout_pushed and
    zmpc_herdt_rollout_pushed (device pointers as integers)."""
    _fields_ = [("amp", ctypes.c_void_p), ("axes", ctypes.c_int32), ("steps", ctypes.c_void_p),
                ("step", ctypes.c_int64), ("profile", ctypes.c_void_p),
                ("duration", ctypes.c_int64)]


_lib = None
_lock = threading.Lock()


class NativeError(RuntimeError):
    """A libzmpc call failed (message from zmpc_last_error)."""


class DeviceOutOfMemory(NativeError, MemoryError):
    """ZMPC_ENOMEM: a plan or per-launch workspace allocation on the device failed."""


def load():
    """Load libzmpc.so once; raise with a build hint if it is not there."""
    global _lib
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
