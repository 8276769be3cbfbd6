"""The refusals of the C-ABI's launching entry points (csrc/capi.hip), as one table: for every
entry point each bad argument it checks before its first device call, the empty batch, the
ZMPC_ESTATE refusals decided from a plan's fields, and pairs of these, which pin the order of the
checks.  What each row answers — (return code, zmpc_last_error()) — was recorded from the library
of the commit before capi.hip's disturbance paths were merged
(tests/golden/make_capi_refusals_golden.py → tests/golden/capi_refusals.json); compared by
tests/test_capi_refusals_host.py.  No row reaches a device call, so no device is needed and
the addresses are never read.  Not a test module.

A plan is a zeroed block with its leading ints set (device, cus, N, Kpad, strict), as in
tests/test_push_rollout_host.py: "unc" N = 8, "strict" N = 64, "strict1"/"strict2" with that
strict-solver option, "strict1000" solver 0 at N = 1000 (no kernel but the reduced-Cholesky one).
"""
import ctypes
import itertools

from mpc_bipedal import _native
from mpc_bipedal.config import MPCConfig
from mpc_bipedal.controllers import herdt

FILE = "capi_refusals.json"
PTR = 4096  # a non-NULL device address, never read
PLAN, PRM, PUSH, TRACE, WORD = "<plan>", "<params>", "<push>", "<trace>", "<int32*>"
STRUCTS = {"push": dict(amp=PTR, axes=3, steps=None, step=3, profile=None, duration=4),
           "trace": dict(dv=PTR, axes=3, steps=None, step=3, length=4, stream=None),
           "prm": {}}
KICK_PUSH = dict(axes=2, duration=1)  # the legacy one-sample y kick as a push

_walks = [("B", 2), ("n", 10), ("zmax", PTR), ("zmin", PTR), ("bounds_stride", 20), ("x0", PTR)]
_hist = [("B", 2), ("n", 10), ("hist", PTR), ("zmax", PTR), ("zmin", PTR), ("bounds_stride", 20),
         ("lengths", None)]
_herdt = [("prm", PRM), ("B", 2), ("n", 10), ("v_ref", PTR), ("v_stride", 20), ("states", PTR),
          ("s_stride", 10), ("nb_next", PTR), ("nb_stride", 10), ("x0", PTR)]
_P = [("plan", PLAN)]
_S = [("stream", None)]
_out = [("hist", PTR), ("status", None)]
_hout = [("hist", PTR), ("foot", PTR), ("status", None)]

# variant → (symbol, [(argument, good value)], {struct: field overrides of the variant})
ENTRIES = {
    "zmpc_step": ("zmpc_step", _P + [("B", 2), ("x", PTR), ("zmax_win", PTR), ("zmin_win", PTR),
                                     ("x_next", PTR), ("status", None)] + _S, {}),
    "zmpc_rollout": ("zmpc_rollout", _P + _walks + [("kick", None), ("kick_step", 3)] + _out + _S,
                     {}),
    "zmpc_rollout_kicks": ("zmpc_rollout_kicks",
                           _P + _walks + [("kick", PTR), ("kick_steps", PTR)] + _out + _S, {}),
    "zmpc_rollout_pushed": ("zmpc_rollout_pushed", _P + _walks + [("push", PUSH)] + _out + _S, {}),
    "zmpc_rollout_pushed/kick": ("zmpc_rollout_pushed", _P + _walks + [("push", PUSH)] + _out + _S,
                                 {"push": KICK_PUSH}),
    "zmpc_rollout_pushed/kick_steps": ("zmpc_rollout_pushed",
                                       _P + _walks + [("push", PUSH)] + _out + _S,
                                       {"push": dict(KICK_PUSH, steps=PTR)}),
    "zmpc_rollout_traced": ("zmpc_rollout_traced", _P + _walks + [("trace", TRACE)] + _out, {}),
    "zmpc_walk_metrics": ("zmpc_walk_metrics", _P + _hist + [("metrics", PTR)] + _S, {}),
    "zmpc_rollout_metrics": ("zmpc_rollout_metrics",
                             _P + _walks + [("kick", None), ("kick_step", 3), ("kick_steps", None),
                                            ("lengths", None), ("metrics", PTR), ("status", None)]
                             + _S, {}),
    "zmpc_push_map": ("zmpc_push_map",
                      _P + _hist + [("push_steps", None), ("max_violation", 1e-9), ("mass", 40.0),
                                    ("force", PTR), ("limit", None), ("response", None)] + _S, {}),
    "zmpc_push_map_shaped": ("zmpc_push_map_shaped",
                             _P + _hist + [("push_steps", None), ("profile", None),
                                           ("duration", 2), ("axes", 3), ("max_violation", 1e-9),
                                           ("mass", 40.0), ("force", PTR), ("limit", None),
                                           ("response", None)] + _S, {}),
    "zmpc_trace_margin": ("zmpc_trace_margin",
                          _P + _hist + [("draws", 2), ("trace", TRACE), ("max_violation", 1e-9),
                                        ("scale", PTR), ("limit", None)], {}),
    "zmpc_herdt_rollout": ("zmpc_herdt_rollout",
                           _P + _herdt + [("kick", None), ("kick_step", 3)] + _hout + _S, {}),
    "zmpc_herdt_rollout_pushed": ("zmpc_herdt_rollout_pushed",
                                  _P + _herdt + [("push", PUSH)] + _hout + _S, {}),
    "zmpc_herdt_rollout_pushed/kick": ("zmpc_herdt_rollout_pushed",
                                       _P + _herdt + [("push", PUSH)] + _hout + _S,
                                       {"push": KICK_PUSH}),
    "zmpc_herdt_rollout_pushed/kick_steps": ("zmpc_herdt_rollout_pushed",
                                             _P + _herdt + [("push", PUSH)] + _hout + _S,
                                             {"push": dict(KICK_PUSH, steps=PTR)}),
    "zmpc_herdt_rollout_traced": ("zmpc_herdt_rollout_traced",
                                  _P + _herdt + [("trace", TRACE)] + _hout, {}),
    "zmpc_herdt_step": ("zmpc_herdt_step",
                        _P + [("prm", PRM), ("B", 2), ("x", PTR), ("v_win", PTR), ("s_win", PTR),
                              ("current", PTR), ("foot", PTR), ("side", PTR), ("x_next", PTR),
                              ("step", PTR), ("status", None)] + _S, {}),
    "zmpc_herdt_walk_metrics": ("zmpc_herdt_walk_metrics",
                                _P + [("prm", PRM), ("B", 2), ("n", 10), ("hist", PTR),
                                      ("foot", PTR), ("states", PTR), ("s_stride", 10),
                                      ("foot_ref", None), ("foot_ref_stride", 0),
                                      ("lengths", None), ("count_tol", 1e-9), ("metrics", PTR)]
                                + _S, {}),
    "zmpc_herdt_prepare": ("zmpc_herdt_prepare",
                           _P + [("B", 2), ("n", 10), ("states", PTR), ("s_stride", 10),
                                 ("lengths", None), ("states_out", None), ("nb_next", PTR),
                                 ("max_steps", None), ("max_footsteps_host", WORD)], {}),
    "zmpc_herdt_prepare/no_word": ("zmpc_herdt_prepare",
                                   _P + [("B", 2), ("n", 10), ("states", PTR), ("s_stride", 10),
                                         ("lengths", None), ("states_out", None), ("nb_next", PTR),
                                         ("max_steps", None), ("max_footsteps_host", None)], {}),
    "zmpc_cop_generate": ("zmpc_cop_generate",
                          [("device", 0), ("B", 2), ("params", PTR), ("n_cap", 10), ("zmax", PTR),
                           ("zmin", PTR), ("states", None), ("n_out", None)] + _S, {}),
}

NAN, INF = float("nan"), float("inf")
_B0 = ("B=0", {"B": 0})
_size = [("B=-1", {"B": -1}), ("n=0", {"n": 0}), _B0]
_big = [("B=2^31", {"B": 2 ** 31}), ("n=2^24+1", {"n": 2 ** 24 + 1, "bounds_stride": 0})]
_stride = [("bounds_stride=19", {"bounds_stride": 19})]
_strict_roll = [(f"plan={k}", {"plan": k}) for k in ("strict1", "strict2", "strict1000")]
_strict = [("plan=strict", {"plan": "strict"})]
_noplan = [("plan=NULL", {"plan": None})]


def _nulls(*names):
    """One NULL per array argument: the first pairs with the other faults, the rest stand alone
    (they give the same message)."""
    return [(f"{a}=NULL", {a: None}) for a in names[:1]], \
        [(f"{a}=NULL", {a: None}) for a in names[1:]]


def _fields(struct, *faults):
    return [(f"{struct}.{f}={v}", {struct: {f: v}}) for f, v in faults]


_push = [("push=NULL", {"push": None})] + _fields("push", ("axes", 0), ("duration", 0),
                                                  ("amp", None))
_push_solo = _fields("push", ("axes", 4), ("axes", -1), ("duration", -2 ** 40))
_trace = [("trace=NULL", {"trace": None})] + _fields("trace", ("axes", 0), ("length", 0),
                                                     ("dv", None), ("length", 2 ** 62))
_trace_solo = _fields("trace", ("axes", 4), ("length", -1), ("length", 2 ** 63 - 1))
_prm = [("prm=NULL", {"prm": None})] + _fields("prm", ("nfacets0", 2), ("max_footsteps", 9),
                                               ("max_passes", -1), ("alpha", 0.0))
_prm_solo = _fields("prm", ("nfacets1", 17), ("max_footsteps", -1), ("max_passes", 100001),
                    ("beta", -1.0), ("gamma", 0.0), ("alpha", NAN))


def _rollout(dist=(), dist_solo=(), strict=()):
    a, b = _nulls("zmax", "zmin", "x0", "hist")
    # ("n=2^24+1/stride": with the good stride 20 beside it, a pair of its own)
    return (_noplan + _size + a + _big + _stride + list(dist) + list(strict),
            b + list(dist_solo) + [("n=2^24+1/stride", {"n": 2 ** 24 + 1})])


def _herdt_rollout(dist=(), dist_solo=()):
    a, b = _nulls("v_ref", "states", "nb_next", "x0", "hist", "foot")
    return (_noplan + _prm + _size + a
            + [("B=2^31", {"B": 2 ** 31}), ("v_stride=19", {"v_stride": 19})] + list(dist),
            b + _prm_solo + list(dist_solo)
            + [("n=2^24+1", {"n": 2 ** 24 + 1, "v_stride": 0, "s_stride": 0, "nb_stride": 0}),
               ("s_stride=9", {"s_stride": 9}), ("nb_stride=3", {"nb_stride": 3})])


def _push_map(extra=()):
    a, b = _nulls("hist", "zmax", "zmin", "force")
    return (_noplan + _size + a + _big + _stride + _strict + list(extra)
            + [("max_violation=-1", {"max_violation": -1.0}), ("mass=0", {"mass": 0.0}),
               ("n=20000", {"n": 20000, "bounds_stride": 0})],
            b + [("max_violation=nan", {"max_violation": NAN}), ("mass=inf", {"mass": INF}),
                 ("mass=nan", {"mass": NAN})])


def _faults():
    """variant → (faults that are paired with each other, faults that stand alone)."""
    f = {}
    a, b = _nulls("x", "zmax_win", "zmin_win", "x_next")
    f["zmpc_step"] = (_noplan + [("B=-1", {"B": -1}), _B0] + a + [("B=2^33", {"B": 2 ** 33})], b)
    f["zmpc_rollout"] = _rollout()
    f["zmpc_rollout_kicks"] = _rollout([("kick_steps=NULL", {"kick_steps": None})])
    f["zmpc_rollout_pushed"] = _rollout(_push, _push_solo, _strict_roll)
    f["zmpc_rollout_pushed/kick"] = _rollout(_push[:1] + _push[3:])
    f["zmpc_rollout_pushed/kick_steps"] = _rollout(_push[3:])
    f["zmpc_rollout_traced"] = _rollout(_trace, _trace_solo, _strict_roll)
    a, b = _nulls("hist", "zmax", "zmin", "metrics")
    f["zmpc_walk_metrics"] = (_noplan + _size + a + _big + _stride,
                              b + [("n=2^24+1/stride", {"n": 2 ** 24 + 1})])
    a, b = _nulls("zmax", "zmin", "x0", "metrics")
    f["zmpc_rollout_metrics"] = (
        _noplan + _size + a + _big + _stride + _strict
        + [("n=600", {"n": 600, "bounds_stride": 1200})], b)
    f["zmpc_push_map"] = _push_map()
    f["zmpc_push_map_shaped"] = _push_map([("duration=0", {"duration": 0}),
                                           ("axes=0", {"axes": 0})])
    f["zmpc_push_map_shaped"][1].append(("axes=4", {"axes": 4}))
    a, b = _nulls("hist", "zmax", "zmin", "scale")
    f["zmpc_trace_margin"] = (
        _noplan + _size + a + _stride + _strict + _trace
        + [("draws=0", {"draws": 0}), ("B=2^31", {"B": 2 ** 31}),
           ("max_violation=-1", {"max_violation": -1.0}),
           ("n=2^30+1", {"n": 2 ** 30 + 1, "bounds_stride": 0})],
        b + _trace_solo + [("B=2^30,draws=4", {"B": 2 ** 30, "draws": 4}),
                           ("max_violation=nan", {"max_violation": NAN})])
    f["zmpc_herdt_rollout"] = _herdt_rollout()
    f["zmpc_herdt_rollout_pushed"] = _herdt_rollout(_push, _push_solo)
    f["zmpc_herdt_rollout_pushed/kick"] = _herdt_rollout(_push[:1] + _push[3:])
    f["zmpc_herdt_rollout_pushed/kick_steps"] = _herdt_rollout(_push[3:])
    f["zmpc_herdt_rollout_traced"] = _herdt_rollout(_trace, _trace_solo)
    a, b = _nulls("x", "v_win", "s_win", "current", "foot", "side", "x_next", "step")
    f["zmpc_herdt_step"] = (_noplan + _prm + [("B=-1", {"B": -1}), _B0] + a
                            + [("B=2^31", {"B": 2 ** 31})], b + _prm_solo)
    a, b = _nulls("hist", "foot", "states", "metrics")
    f["zmpc_herdt_walk_metrics"] = (
        _noplan + [("prm=NULL", {"prm": None})] + _size + a
        + [("B=2^31", {"B": 2 ** 31}), ("n=2^24+1", {"n": 2 ** 24 + 1, "s_stride": 0}),
           ("count_tol=-1", {"count_tol": -1.0}), ("s_stride=9", {"s_stride": 9})]
        + _fields("prm", ("nfacets0", -1)),
        b + [("count_tol=nan", {"count_tol": NAN}), ("foot_ref_stride=19", {"foot_ref_stride": 19})]
        + _fields("prm", ("nfacets1", 17)))
    a, b = _nulls("states", "nb_next")
    prep = (_noplan + _size + a + [("B=2^31", {"B": 2 ** 31}), ("s_stride=9", {"s_stride": 9}),
                                   ("n=2^24+1", {"n": 2 ** 24 + 1, "s_stride": 0})], b)
    f["zmpc_herdt_prepare"] = prep
    f["zmpc_herdt_prepare/no_word"] = (prep[0][:4], [])
    f["zmpc_cop_generate"] = (
        [("B=-1", {"B": -1}), ("n_cap=-1", {"n_cap": -1}), _B0, ("params=NULL", {"params": None}),
         ("zmax=NULL", {"zmax": None}), ("n_cap=0,n_out=NULL", {"n_cap": 0, "n_out": None})],
        [("zmin=NULL", {"zmin": None})])
    assert set(f) == set(ENTRIES)
    return f


def _merge(a, b):
    """Two faults in one call, None where they change the same argument or field."""
    out = dict(a)
    for k, v in b.items():
        if k not in out:
            out[k] = v
        elif isinstance(v, dict) and isinstance(out[k], dict) and not set(v) & set(out[k]):
            out[k] = {**out[k], **v}
        else:
            return None
    return out


def rows():
    """[(id, variant, overrides)], ids unique: every fault alone, then every pair of the paired
    faults that change different arguments."""
    r = []
    for variant, (paired, solo) in _faults().items():
        r += [(f"{variant}: {name}", variant, o) for name, o in paired + solo]
        for (na, a), (nb, b) in itertools.combinations(paired, 2):
            both = _merge(a, b)
            if both is not None:
                r.append((f"{variant}: {na} + {nb}", variant, both))
    assert len({name for name, _, _ in r}) == len(r)
    return r


def _plan_block(lib, kind, keep):
    blk = ctypes.create_string_buffer(4096)
    keep.append(blk)
    ints = (ctypes.c_int * 5).from_buffer(blk)  # (device, cus, N, Kpad, strict)
    ints[2] = 8
    if kind != "unc":
        ints[2], ints[4] = 64, 1
        solver = {"strict": 0, "strict1": 1, "strict2": 2, "strict1000": 0}[kind]
        rc = lib.zmpc_plan_set_option(ctypes.addressof(blk), _native.OPTIONS["strict_solver"],
                                      solver)
        assert rc == 0, lib.zmpc_last_error()
        if kind == "strict1000":
            ints[2] = 1000
    return ctypes.addressof(blk)


def _struct(kind, fields, keep):
    if kind == "prm":
        s = herdt.make_params(MPCConfig(), 2)
        for f, v in fields.items():
            if f.startswith("nfacets"):
                s.nfacets[int(f[-1])] = v
            else:
                setattr(s, f, v)
    else:
        cls = _native.ZmpcPush if kind == "push" else _native.ZmpcTrace
        s = cls(**{**STRUCTS[kind], **fields})
    keep.append(s)
    return ctypes.addressof(s)


def answer(lib, variant, overrides):
    """(return code, message) of one row on the loaded library."""
    symbol, args, base = ENTRIES[variant]
    keep, argv = [], []
    for name, good in args:
        v = overrides.get(name, good)
        if name == "plan":
            v = None if v is None else _plan_block(lib, "unc" if v == PLAN else v, keep)
        elif name in STRUCTS:
            fields = {**base.get(name, {}), **(v if isinstance(v, dict) else {})}
            v = None if v is None else _struct(name, fields, keep)
        elif v == WORD:
            keep.append(ctypes.c_int32(-7))
            v = ctypes.byref(keep[-1])
        argv.append(v)
    rc = getattr(lib, symbol)(*argv)
    return [int(rc), lib.zmpc_last_error().decode()]


def reaches_no_device(overrides, got):
    """A row stays on the host: it is refused with a reason, or it is the empty batch."""
    rc, msg = got
    if rc in (_native.ZMPC_EINVAL, _native.ZMPC_ESTATE):
        return bool(msg)
    return rc == _native.ZMPC_OK and overrides.get("B") == 0 and msg == ""
