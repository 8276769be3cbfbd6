// C-ABI of libzmpc.so (declared in include/zmpc.h).  Host-side only: argument checks,
// device selection, buffer ownership of plans, error reporting.  No compute runs here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

#include "zmpc_internal.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  return fail(ZMPC_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

// Switch to the plan's device for the duration of a call, restore the caller's device.
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    if ((err = hipGetDevice(&prev)) != hipSuccess) return;
    if (prev != dev) err = hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// A launcher's verdict: an argument it rejects comes with a reason (EINVAL), a failed
// per-launch workspace allocation is hipErrorOutOfMemory (ENOMEM), anything else is HIP's.
int launch_result(hipError_t e, const std::string& why, const char* what) {
  if (e == hipSuccess) return ZMPC_OK;
  if (!why.empty()) return fail(ZMPC_EINVAL, why);
  if (e == hipErrorOutOfMemory)
    return fail(ZMPC_ENOMEM, std::string(what) + ": device workspace allocation failed");
  return hip_fail(e, (std::string(what) + " launch").c_str());
}

void free_plan(zmpc_plan* p) {
  if (!p) return;
  double* bufs[] = {p->p, p->Px, p->M,  p->L,     p->k,      p->kx,     p->kffa,
                    p->ksum, p->X, p->G,  p->v,  p->Hz,    p->scanP,  p->fft_tw, p->fft_g};
  for (double* b : bufs)
    if (b) (void)hipFree(b);
  if (p->info) (void)hipFree(p->info);
  if (p->lqtab) (void)hipFree(p->lqtab);
  if (p->lqcnt) (void)hipFree(p->lqcnt);
  delete p;
}

// The checks several entry points state in the same words; each entry point applies them in its
// own order (`if (int rc = need_…) return rc;`)
int need_walks(int64_t B, int64_t n) {
  return B < 0 || n < 1 ? fail(ZMPC_EINVAL, "need B >= 0 and n >= 1") : ZMPC_OK;
}
int need_bounds_stride(int64_t stride, int64_t n) {
  if (stride == 0 || stride >= 2 * n) return ZMPC_OK;
  return fail(ZMPC_EINVAL, "bounds_stride must be 0 (shared CoP) or >= 2n");
}
int need_batch(int64_t B) {
  return B > 0x7fffffff ? fail(ZMPC_EINVAL, "batch too large") : ZMPC_OK;
}
int need_length(int64_t n) {
  return n > (1 << 24) ? fail(ZMPC_EINVAL, "walk too long") : ZMPC_OK;
}

// per-device one-time kernel attributes and pool threshold; plan creation may run on several
// host threads at once (zmpc.h: plans are shareable across threads), so the check-and-set is
// under a lock
std::mutex g_attrs_mu;
bool attrs_done[64] = {};

}  // namespace

extern "C" {

int zmpc_abi_version(void) { return ZMPC_ABI_VERSION; }

const char* zmpc_last_error(void) { return g_err.c_str(); }

int zmpc_plan_create(int device, int32_t N, double T, double T2_2, double T3_6, double hg,
                     double Thg, double Q, double R, int32_t strict, void* stream,
                     zmpc_plan** out) {
  g_err.clear();
  if (!out) return fail(ZMPC_EINVAL, "out is NULL");
  *out = nullptr;
  if (N < 1 || N > 4096) return fail(ZMPC_EINVAL, "horizon N must be in [1, 4096]");
  if (!(T > 0) || !(Q > 0) || !(R >= 0))
    return fail(ZMPC_EINVAL, "need dt > 0, Q > 0, R >= 0");
  if (strict && N > ZMPC_STRICT_MAX_N)
    return fail(ZMPC_EINVAL, "strict horizon N must be <= " + std::to_string(ZMPC_STRICT_MAX_N));
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
  if (device < 0 || device >= ndev) return fail(ZMPC_EINVAL, "device index out of range");
  DeviceGuard g(device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  std::unique_lock<std::mutex> attrs_lock(g_attrs_mu);
  if (device >= 64 || !attrs_done[device]) {
    if ((e = zmpc_rollout_unc_set_attrs()) != hipSuccess) return hip_fail(e, "set LDS attrs");
    if ((e = zmpc_strict_set_attrs()) != hipSuccess) return hip_fail(e, "set LDS attrs");
    if ((e = zmpc_strict_lq_set_attrs()) != hipSuccess) return hip_fail(e, "set LDS attrs");
    if ((e = zmpc_herdt_set_attrs()) != hipSuccess) return hip_fail(e, "set LDS attrs");
    if ((e = zmpc_push_map_set_attrs()) != hipSuccess) return hip_fail(e, "set LDS attrs");
    // the strict solvers' per-launch workspaces come from the stream-ordered pool: keep up to
    // ZMPC_POOL_KEEP_MB (default 4096) of freed blocks in the pool across synchronisations
    // instead of returning them to the driver every time; anything above is released
    hipMemPool_t pool = nullptr;
    if (hipDeviceGetDefaultMemPool(&pool, device) == hipSuccess && pool) {
      // (the only environment variable of the product library; memory retention only)
      const char* env = getenv("ZMPC_POOL_KEEP_MB");
      long long mb = 4096;
      if (env) {
        char* end = nullptr;
        const long long v = strtoll(env, &end, 10);
        if (end != env && *end == '\0' && v >= 0 && v <= (1ll << 22))
          mb = v;
        else
          fprintf(stderr, "libzmpc: ignoring ZMPC_POOL_KEEP_MB=%s (expected 0..%lld MiB)\n",
                  env, 1ll << 22);
      }
      uint64_t keep = (uint64_t)mb << 20;
      (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    }
    if (device < 64) attrs_done[device] = true;
  }
  attrs_lock.unlock();

  zmpc_plan* P = new zmpc_plan();
  P->device = device;
  if ((e = hipDeviceGetAttribute(&P->cus, hipDeviceAttributeMultiprocessorCount, device)) !=
      hipSuccess) {
    delete P;
    return hip_fail(e, "hipDeviceGetAttribute");
  }
  P->N = N;
  P->Kpad = (N + 15) & ~15;
  P->strict = strict ? 1 : 0;
  P->T = T;
  P->T2_2 = T2_2;
  P->T3_6 = T3_6;
  P->hg = hg;
  P->Thg = Thg;
  P->Q = Q;
  P->R = R;
  P->lc = LipmConsts{T, T2_2, T3_6};
  const size_t nn = (size_t)N * N;
  struct {
    double** ptr;
    size_t n;
  } allocs[] = {{&P->p, (size_t)N},  {&P->Px, 3 * (size_t)N}, {&P->M, nn}, {&P->L, nn},
                {&P->k, (size_t)P->Kpad + 64}, {&P->kx, 4}, {&P->kffa, 4 * (size_t)kffa_rows(N)},
                {&P->ksum, (size_t)ksum_rows(N)},
                {&P->scanP, kScanDoubles},
                {&P->X, strict ? nn : 0}, {&P->G, strict ? nn : 0},
                {&P->v, strict ? (size_t)N : 0}, {&P->Hz, strict ? nn : 0},
                {&P->fft_tw, 2 * (size_t)kFftPT}, {&P->fft_g, 2 * (size_t)kFftGComplex}};
  for (auto& a : allocs) {
    if (a.n == 0) continue;
    if ((e = hipMalloc((void**)a.ptr, a.n * sizeof(double))) != hipSuccess) {
      free_plan(P);
      return fail(ZMPC_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
  }
  if ((e = hipMalloc((void**)&P->info, sizeof(int))) != hipSuccess) {
    free_plan(P);
    return fail(ZMPC_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  }
  if (strict) {
    P->strict_slots = 2 * P->cus;
    if ((e = hipMalloc((void**)&P->lqtab, zmpc_strict_lq_table_doubles(N) * sizeof(double))) !=
        hipSuccess) {
      free_plan(P);
      return fail(ZMPC_ENOMEM, std::string("hipMalloc strict table: ") + hipGetErrorString(e));
    }
  }
  // work counters of the active-set solvers (strict and Herdt), every plan
  if ((e = hipMalloc((void**)&P->lqcnt, ZMPC_NCOUNTERS * sizeof(unsigned long long))) !=
      hipSuccess) {
    free_plan(P);
    return fail(ZMPC_ENOMEM, std::string("hipMalloc counters: ") + hipGetErrorString(e));
  }
  hipStream_t s = (hipStream_t)stream;
  (void)hipMemsetAsync(P->k, 0, ((size_t)P->Kpad + 64) * sizeof(double), s);
  if (P->lqcnt)
    (void)hipMemsetAsync(P->lqcnt, 0, ZMPC_NCOUNTERS * sizeof(unsigned long long), s);
  // stage timings (zmpc_plan_timings): events between the plan-build stages
  hipEvent_t ev[ZMPC_PLAN_STAGES] = {};
  bool timed = true;
  for (auto& x : ev) timed = timed && hipEventCreate(&x) == hipSuccess;
  struct EvGuard {
    hipEvent_t* ev;
    ~EvGuard() {
      for (int i = 0; i < ZMPC_PLAN_STAGES; ++i)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    }
  } evg{ev};
  if ((e = zmpc_launch_plan(P, s, timed ? ev : nullptr)) != hipSuccess) {
    free_plan(P);
    return hip_fail(e, "plan kernels");
  }
  if (P->lqtab && (e = zmpc_strict_lq_build_table(P, s)) != hipSuccess) {
    free_plan(P);
    return hip_fail(e, "strict table kernel");
  }
  if (timed) (void)hipEventRecord(ev[ZMPC_PLAN_STAGES - 1], s);
  if ((e = hipStreamSynchronize(s)) != hipSuccess) {
    free_plan(P);
    return hip_fail(e, "plan synchronize");
  }
  if (timed) {
    for (int i = 0; i + 1 < ZMPC_PLAN_STAGES; ++i)
      (void)hipEventElapsedTime(&P->stage_ms[i], ev[i], ev[i + 1]);
    (void)hipEventElapsedTime(&P->stage_ms[ZMPC_PLAN_STAGES - 1], ev[0],
                              ev[ZMPC_PLAN_STAGES - 1]);
  }
  int info = 0;
  if ((e = hipMemcpy(&info, P->info, sizeof(int), hipMemcpyDeviceToHost)) != hipSuccess) {
    free_plan(P);
    return hip_fail(e, "plan info copy");
  }
#ifdef ZMPC_DIAG
  const bool keep_failed = getenv("ZMPC_DEBUG_PLAN") != nullptr;  // diagnostics: export it
#else
  const bool keep_failed = false;
#endif
  if (info != 0 && !keep_failed) {
    free_plan(P);
    return fail(ZMPC_ESTATE, "PuᵀPu + (R/Q)I is not positive definite (pivot " +
                                 std::to_string(info) + ")");
  }
  *out = P;
  return ZMPC_OK;
}

int zmpc_plan_destroy(zmpc_plan* plan) {
  g_err.clear();
  if (!plan) return ZMPC_OK;
  DeviceGuard g(plan->device);
  (void)hipDeviceSynchronize();
  free_plan(plan);
  return ZMPC_OK;
}

int zmpc_plan_timings(const zmpc_plan* P, float* dst, int32_t count) {
  g_err.clear();
  if (!P || !dst) return fail(ZMPC_EINVAL, "NULL plan or destination");
  for (int i = 0; i < count && i < ZMPC_PLAN_STAGES; ++i) dst[i] = P->stage_ms[i];
  return ZMPC_OK;
}

int zmpc_plan_set_option(zmpc_plan* P, int32_t option, int64_t value) {
  g_err.clear();
  if (!P) return fail(ZMPC_EINVAL, "NULL plan");
  static const int64_t hi[ZMPC_NOPTIONS] = {1, 3, 1, 1, 4, 2};  // largest value of each option
  if (option < 0 || option >= ZMPC_NOPTIONS) return fail(ZMPC_EINVAL, "unknown option");
  if (value < 0 || value > hi[option])
    return fail(ZMPC_EINVAL, "option value out of range (0.." + std::to_string(hi[option]) + ")");
  if (option == ZMPC_OPT_STRICT_SOLVER && (value == 1 || value == 2) &&
      (!P->strict || P->N > kStrictCholMaxN))
    return fail(ZMPC_EINVAL, "the reduced-Cholesky strict kernels need a strict plan, N <= " +
                                  std::to_string(kStrictCholMaxN));
  if (option == ZMPC_OPT_STRICT_SOLVER && value == 4 &&
      (!P->strict || !zmpc_strict_scan_supported(P)))
    return fail(ZMPC_EINVAL, "the small-batch strict kernel needs a strict plan, N <= " +
                                  std::to_string(kScanMaxN));
  if (option == ZMPC_OPT_STRICT_SOLVER && value == 3 && !zmpc_strict_lq_supported(P))
    return fail(ZMPC_EINVAL, "the LQ strict kernel needs a strict plan, N <= " +
                                  std::to_string(ZMPC_STRICT_MAX_N));
  P->opt[option] = (int)value;
  return ZMPC_OK;
}

int zmpc_plan_get_option(const zmpc_plan* P, int32_t option, int64_t* value) {
  g_err.clear();
  if (!P || !value) return fail(ZMPC_EINVAL, "NULL plan or destination");
  if (option < 0 || option >= ZMPC_NOPTIONS) return fail(ZMPC_EINVAL, "unknown option");
  *value = P->opt[option];
  return ZMPC_OK;
}

int zmpc_plan_export(const zmpc_plan* P, int32_t what, double* dst, int64_t count) {
  g_err.clear();
  if (!P || !dst) return fail(ZMPC_EINVAL, "NULL plan or destination");
  const int64_t N = P->N;
  const double* src = nullptr;
  int64_t n = 0;
  switch (what) {
    case 0: src = P->p; n = N; break;
    case 1: src = P->Px; n = 3 * N; break;
    case 2: src = P->M; n = N * N; break;
    case 3: src = P->k; n = N; break;
    case 4: src = P->kx; n = 3; break;
    case 5: src = P->G; n = P->G ? N * N : 0; break;
    case 6: src = P->L; n = N * N; break;
    case 7: src = P->Hz; n = P->Hz ? N * N : 0; break;
    case 8: src = P->kffa; n = 4 * (int64_t)kffa_rows((int)N); break;
    case 9: src = P->ksum; n = ksum_rows((int)N); break;
    case 10: src = P->scanP; n = kScanDoubles; break;
    case 11: src = P->X; n = P->X ? N * N : 0; break;
    case 12: src = P->v; n = P->v ? N : 0; break;
    case 13: src = P->fft_tw; n = 2 * (int64_t)kFftPT; break;
    case 14: src = P->fft_g; n = 2 * (int64_t)kFftGComplex; break;
    default: return fail(ZMPC_EINVAL, "unknown export id");
  }
  if (!src || n == 0) return fail(ZMPC_ESTATE, "quantity not held by this plan");
  if (count < n) return fail(ZMPC_EINVAL, "destination too small");
  DeviceGuard g(P->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return hip_fail(e, "hipDeviceSynchronize");
  e = hipMemcpy(dst, src, n * sizeof(double), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_fail(e, "hipMemcpy");
  return ZMPC_OK;
}

int zmpc_plan_counters(const zmpc_plan* P, uint64_t* dst, int32_t count, int32_t reset) {
  g_err.clear();
  if (!P || !dst) return fail(ZMPC_EINVAL, "NULL plan or destination");
  if (count < 0) return fail(ZMPC_EINVAL, "count < 0");
  if (!P->lqcnt) return fail(ZMPC_ESTATE, "plan has no solver counters");
  DeviceGuard g(P->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return hip_fail(e, "hipDeviceSynchronize");
  unsigned long long h[ZMPC_NCOUNTERS];
  e = hipMemcpy(h, P->lqcnt, sizeof(h), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_fail(e, "hipMemcpy");
  for (int i = 0; i < count && i < ZMPC_NCOUNTERS; ++i) dst[i] = (uint64_t)h[i];
  if (reset) {
    e = hipMemset(P->lqcnt, 0, sizeof(h));
    if (e != hipSuccess) return hip_fail(e, "hipMemset");
  }
  return ZMPC_OK;
}

int zmpc_step(const zmpc_plan* P, int64_t B, const double* x, const double* zmax_win,
              const double* zmin_win, double* x_next, int32_t* status, void* stream) {
  g_err.clear();
  if (!P) return fail(ZMPC_EINVAL, "NULL plan");
  if (B < 0) return fail(ZMPC_EINVAL, "B < 0");
  if (B == 0) return ZMPC_OK;
  if (!x || !zmax_win || !zmin_win || !x_next)
    return fail(ZMPC_EINVAL, "NULL array argument");
  if (B > (int64_t)0x7fffffff * 4) return fail(ZMPC_EINVAL, "batch too large");
  DeviceGuard g(P->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  std::string why;
  const StepCall c{B, x, zmax_win, zmin_win, x_next, status};
  hipError_t e = P->strict ? zmpc_launch_step_strict(P, c, (hipStream_t)stream, &why)
                           : zmpc_launch_step_unc(P, c, (hipStream_t)stream);
  return launch_result(e, why, "zmpc_step");
}

// The checks of a zmpc_push (include/zmpc.h "The push, stated once"), before any device call
static int push_check(const zmpc_push* push, int64_t B) {
  if (!push) return fail(ZMPC_EINVAL, "push is NULL");
  if (push->axes < 1 || push->axes > (ZMPC_PUSH_AXIS_X | ZMPC_PUSH_AXIS_Y))
    return fail(ZMPC_EINVAL, "push axes must be 1 (the x axis), 2 (the y axis) or 3 (both)");
  if (push->duration < 1) return fail(ZMPC_EINVAL, "need push duration >= 1 (samples)");
  if (B > 0 && !push->amp) return fail(ZMPC_EINVAL, "push amp is NULL");
  return ZMPC_OK;
}

// the legacy push: one sample on y without a profile, the kick of zmpc_rollout itself
static bool push_is_kick(const zmpc_push* push) {
  return push->axes == ZMPC_PUSH_AXIS_Y && push->duration == 1 && push->profile == nullptr;
}

// The checks of a zmpc_trace (include/zmpc.h "The trace, stated once"), before any device call
static int trace_check(const zmpc_trace* trace, int64_t B) {
  if (!trace) return fail(ZMPC_EINVAL, "trace is NULL");
  if (trace->axes < 1 || trace->axes > (ZMPC_PUSH_AXIS_X | ZMPC_PUSH_AXIS_Y))
    return fail(ZMPC_EINVAL, "trace axes must be 1 (the x axis), 2 (the y axis) or 3 (both)");
  if (trace->length < 1) return fail(ZMPC_EINVAL, "need trace length >= 1 (samples)");
  if (B > 0 && !trace->dv) return fail(ZMPC_EINVAL, "trace dv is NULL");
  // dv holds B·length·C doubles: a length whose byte count passes int64 names no array
  if (trace->length > INT64_MAX / 16 / (B > 0 ? B : 1))
    return fail(ZMPC_EINVAL, "trace length too large (B * length * 16 bytes pass int64)");
  return ZMPC_OK;
}

// What disturbs the walks of a rollout, resolved once by the entry point: nothing or the
// one-sample y kick of the call's own kick fields (push all zero), a push window, or a trace
struct Disturbance {
  enum Kind { Kick, Window, Trace } kind;
  PushArgs push;     // as the launchers take it
  int64_t L;         // a trace's samples per walk as the caller gave them (push.dur is clamped)
  void* stream;
  const char* name;  // the entry point, for messages
};

// The window of `len` steps on `axes` in a walk of n samples: the axes-to-columns rule
static PushArgs window_args(const double* amp, int32_t axes, const int64_t* steps, int64_t step,
                            int64_t len, int64_t n) {
  PushArgs w{};
  w.amp = amp;
  w.steps = steps;
  w.step = step;
  w.dur = (int)(len < n ? len : n);
  w.cols = axes == (ZMPC_PUSH_AXIS_X | ZMPC_PUSH_AXIS_Y) ? 2 : 1;
  w.col[0] = (axes & ZMPC_PUSH_AXIS_X) ? 0 : -1;
  w.col[1] = (axes & ZMPC_PUSH_AXIS_Y) ? w.cols - 1 : -1;
  w.astride = w.cols;
  return w;
}

static Disturbance kick_of(void* stream, const char* name) {
  return {Disturbance::Kick, PushArgs{}, 0, stream, name};
}

// A checked zmpc_push in a walk of n samples
static Disturbance window_of(const zmpc_push* p, int64_t n, void* stream, const char* name) {
  Disturbance d{Disturbance::Window,
                window_args(p->amp, p->axes, p->steps, p->step, p->duration, n), 0, stream, name};
  d.push.w = p->profile;
  return d;
}

// A checked zmpc_trace in a walk of n samples: the window of L steps whose value is read from
// the walk's own row
static Disturbance trace_of(const zmpc_trace* t, int64_t n, const char* name) {
  Disturbance d{Disturbance::Trace, window_args(t->dv, t->axes, t->steps, t->step, t->length, n),
                t->length, t->stream, name};
  d.push.tstride = d.push.cols;
  d.push.astride = t->length * d.push.cols;
  return d;
}

// What the reduced-Cholesky strict kernels take instead of a window and of a trace: the tails of
// the two refusals below, by Disturbance::Kind
static const char* const kCholTakes[3][2] = {
    {nullptr, nullptr},
    {"takes the one-sample y push alone",
     "take the one-sample y push alone (the y axis, duration 1, no profile); "},
    {"takes no trace", "take no trace; "}};

// A filled call of zmpc_rollout, zmpc_rollout_kicks, zmpc_rollout_pushed (a push that is the
// legacy kick arrives as the kick) or zmpc_rollout_traced, under its disturbance
static int rollout_impl(const zmpc_plan* P, RolloutCall c, const Disturbance& d) {
  g_err.clear();
  if (!P) return fail(ZMPC_EINVAL, "NULL plan");
  if (int rc = need_walks(c.B, c.n)) return rc;
  if (c.B == 0) return ZMPC_OK;
  if (!c.zmax || !c.zmin || !c.x0 || !c.hist) return fail(ZMPC_EINVAL, "NULL array argument");
  if (int rc = need_batch(c.B)) return rc;
  if (int rc = need_length(c.n)) return rc;
  if (int rc = need_bounds_stride(c.bstride, c.n)) return rc;
  if (d.kind != Disturbance::Kick && P->strict) {
    // refused before any device call, nothing is launched
    const StrictKind kind =
        choose_strict(P->N, 2 * c.B, P->opt[ZMPC_OPT_STRICT_SOLVER], P->lqtab != nullptr);
    if (kind == StrictKind::Tile && P->opt[ZMPC_OPT_STRICT_SOLVER] == 0)
      return fail(ZMPC_ESTATE,
                  std::string(d.name) + ": at horizon N = " + std::to_string(P->N) +
                      " neither the LQ nor the parallel-in-time strict kernel runs, and the "
                      "reduced-Cholesky kernel left " + kCholTakes[d.kind][0]);
    if (kind == StrictKind::Tile || kind == StrictKind::Wave)
      return fail(ZMPC_ESTATE,
                  std::string(d.name) + ": the reduced-Cholesky strict kernels (strict solver "
                      "options 1 and 2) " + kCholTakes[d.kind][1] + "use strict solver 0, 3 or 4");
  }
  DeviceGuard g(P->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  std::string why;
  hipStream_t s = (hipStream_t)d.stream;
  hipError_t e;
  if (P->strict) {
    c.push = d.push;
    e = zmpc_launch_rollout_strict(P, c, s, &why);
  } else {
    // (unconstrained: the unpushed rollout, then the window's linear state response, or the
    // scan of the walk's own trace, trace.hip)
    e = zmpc_launch_rollout_unc(P, c, s, &why);
    if (d.kind != Disturbance::Kick && e == hipSuccess) {
      c.push = d.push;
      e = d.kind == Disturbance::Trace ? zmpc_launch_trace_response(P, c, d.L, s)
                                       : zmpc_launch_push_response(P, c, s);
    }
  }
  return launch_result(e, why, d.name);
}

// The walks of a rollout call: no kick, no push
static RolloutCall rollout_walks(int64_t B, int64_t n, const double* zmax, const double* zmin,
                                 int64_t bounds_stride, const double* x0, double* hist,
                                 int32_t* status) {
  RolloutCall c{};
  c.B = B, c.n = n, c.zmax = zmax, c.zmin = zmin, c.bstride = bounds_stride, c.x0 = x0;
  c.kick_step = -1, c.hist = hist, c.status = status;
  return c;
}

int zmpc_rollout(const zmpc_plan* P, int64_t B, int64_t n, const double* zmax,
                 const double* zmin, int64_t bounds_stride, const double* x0,
                 const double* kick, int64_t kick_step, double* hist, int32_t* status,
                 void* stream) {
  RolloutCall c = rollout_walks(B, n, zmax, zmin, bounds_stride, x0, hist, status);
  c.kick = kick, c.kick_step = kick_step;
  return rollout_impl(P, c, kick_of(stream, "zmpc_rollout"));
}

int zmpc_rollout_kicks(const zmpc_plan* P, int64_t B, int64_t n, const double* zmax,
                       const double* zmin, int64_t bounds_stride, const double* x0,
                       const double* kick, const int64_t* kick_steps, double* hist,
                       int32_t* status, void* stream) {
  if (!kick_steps) {
    g_err.clear();
    return fail(ZMPC_EINVAL, "kick_steps is NULL (use zmpc_rollout for one kick step)");
  }
  RolloutCall c = rollout_walks(B, n, zmax, zmin, bounds_stride, x0, hist, status);
  c.kick = kick, c.kick_steps = kick_steps;
  return rollout_impl(P, c, kick_of(stream, "zmpc_rollout"));
}

int zmpc_rollout_pushed(const zmpc_plan* P, int64_t B, int64_t n, const double* zmax,
                        const double* zmin, int64_t bounds_stride, const double* x0,
                        const zmpc_push* push, double* hist, int32_t* status, void* stream) {
  g_err.clear();
  if (!P) return fail(ZMPC_EINVAL, "NULL plan");
  if (int rc = push_check(push, B)) return rc;
  RolloutCall c = rollout_walks(B, n, zmax, zmin, bounds_stride, x0, hist, status);
  if (!push_is_kick(push))
    return rollout_impl(P, c, window_of(push, n, stream, "zmpc_rollout_pushed"));
  // what users get today, on every plan kind: the kick path, under its name
  c.kick = push->amp, c.kick_steps = push->steps;
  if (!push->steps) c.kick_step = push->step;
  return rollout_impl(P, c, kick_of(stream, "zmpc_rollout"));
}

int zmpc_rollout_traced(const zmpc_plan* P, int64_t B, int64_t n, const double* zmax,
                        const double* zmin, int64_t bounds_stride, const double* x0,
                        const zmpc_trace* trace, double* hist, int32_t* status) {
  g_err.clear();
  if (!P) return fail(ZMPC_EINVAL, "NULL plan");
  if (int rc = trace_check(trace, B)) return rc;
  return rollout_impl(P, rollout_walks(B, n, zmax, zmin, bounds_stride, x0, hist, status),
                      trace_of(trace, n, "zmpc_rollout_traced"));
}

int zmpc_walk_metrics(const zmpc_plan* P, int64_t B, int64_t n, const double* hist,
                      const double* zmax, const double* zmin, int64_t bounds_stride,
                      const int64_t* lengths, double* metrics, void* stream) {
  g_err.clear();
  if (!P) return fail(ZMPC_EINVAL, "NULL plan");
  if (int rc = need_walks(B, n)) return rc;
  if (int rc = need_bounds_stride(bounds_stride, n)) return rc;
  if (B == 0) return ZMPC_OK;
  if (!hist || !zmax || !zmin || !metrics) return fail(ZMPC_EINVAL, "NULL array argument");
  if (int rc = need_batch(B)) return rc;
  if (int rc = need_length(n)) return rc;
  DeviceGuard g(P->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  hipError_t e = zmpc_launch_walk_metrics(P, B, n, hist, zmax, zmin, bounds_stride, lengths,
                                          metrics, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "zmpc_walk_metrics launch");
  return ZMPC_OK;
}

int zmpc_rollout_metrics(const zmpc_plan* P, int64_t B, int64_t n, const double* zmax,
                         const double* zmin, int64_t bounds_stride, const double* x0,
                         const double* kick, int64_t kick_step, const int64_t* kick_steps,
                         const int64_t* lengths, double* metrics, int32_t* status, void* stream) {
  g_err.clear();
  if (!P) return fail(ZMPC_EINVAL, "NULL plan");
  if (int rc = need_walks(B, n)) return rc;
  if (int rc = need_bounds_stride(bounds_stride, n)) return rc;
  if (B > 0 && (!zmax || !zmin || !x0 || !metrics))
    return fail(ZMPC_EINVAL, "NULL array argument");
  if (int rc = need_batch(B)) return rc;
  if (int rc = need_length(n)) return rc;
  // the shapes without a fused form: refused before any device call, nothing is launched
  if (P->strict)
    return fail(ZMPC_ESTATE, "zmpc_rollout_metrics: strict plans have no fused form (use "
                             "zmpc_rollout + zmpc_walk_metrics)");
  const MetChoice c = choose_unc_metrics(P->N, n, bounds_stride == 0,
                                         P->opt[ZMPC_OPT_ROLLOUT_KERNEL],
                                         P->opt[ZMPC_OPT_CORRELATION]);
  if (c.kind == MetKind::None)
    return fail(ZMPC_ESTATE, std::string("zmpc_rollout_metrics: ") + c.why +
                                 " (use zmpc_rollout + zmpc_walk_metrics)");
  if (B == 0) return ZMPC_OK;
  DeviceGuard g(P->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  RolloutCall rc = rollout_walks(B, n, zmax, zmin, bounds_stride, x0, nullptr, status);
  rc.kick = kick, rc.kick_step = kick_step, rc.kick_steps = kick_steps;
  const hipError_t e =
      zmpc_launch_rollout_metrics(P, rc, lengths, metrics, (hipStream_t)stream);
  return launch_result(e, std::string(), "zmpc_rollout_metrics");
}

// Both push-map entry points: `name` prefixes the messages; zmpc_push_map is the call with
// duration 1, no profile and the y axis, under its own launch rule
static int push_map_impl(const char* name, bool shaped, const zmpc_plan* P, const PushCall& c,
                         void* stream) {
  g_err.clear();
  if (!P) return fail(ZMPC_EINVAL, "NULL plan");
  if (int rc = need_walks(c.B, c.n)) return rc;
  if (!(c.t >= 0)) return fail(ZMPC_EINVAL, "need max_violation >= 0");
  if (!(c.mass > 0) || !(c.mass < __builtin_inf()))
    return fail(ZMPC_EINVAL, "need a finite mass > 0");
  if (int rc = need_bounds_stride(c.bstride, c.n)) return rc;
  if (c.duration < 1) return fail(ZMPC_EINVAL, "need duration >= 1 (samples)");
  if (c.axes < 1 || c.axes > (ZMPC_PUSH_AXIS_X | ZMPC_PUSH_AXIS_Y))
    return fail(ZMPC_EINVAL, "axes must be 1 (the x axis), 2 (the y axis) or 3 (both)");
  if (c.B > 0 && (!c.hist || !c.zmax || !c.zmin || !c.force))
    return fail(ZMPC_EINVAL, "NULL array argument");
  if (int rc = need_batch(c.B)) return rc;
  if (int rc = need_length(c.n)) return rc;
  // refused before any device call, nothing is launched
  if (P->strict)
    return fail(ZMPC_ESTATE, std::string(name) +
                                 ": the ZMP response of a strict (clamped) controller is not "
                                 "affine in the push (bisect over pushed rollouts instead: "
                                 "ZMPController.critical_force)");
  const bool single = c.push_steps != nullptr;
  const PushMapChoice k =
      shaped ? choose_push_shaped(c.n, single, c.axes == 3 ? 2 : 1) : choose_push_map(c.n, single);
  if (!k.ok) return fail(ZMPC_ESTATE, std::string(name) + ": " + k.why);
  if (c.B == 0) return ZMPC_OK;
  DeviceGuard g(P->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  return launch_result(zmpc_launch_push_map(P, c, (hipStream_t)stream), std::string(), name);
}

int zmpc_push_map(const zmpc_plan* P, int64_t B, int64_t n, const double* hist,
                  const double* zmax, const double* zmin, int64_t bounds_stride,
                  const int64_t* lengths, const int64_t* push_steps, double max_violation,
                  double mass, double* force, int32_t* limit, double* response, void* stream) {
  return push_map_impl("zmpc_push_map", false, P,
                       PushCall{B, n, hist, zmax, zmin, bounds_stride, lengths, push_steps,
                                nullptr, 1, ZMPC_PUSH_AXIS_Y, max_violation, mass, force, limit,
                                response},
                       stream);
}

int zmpc_push_map_shaped(const zmpc_plan* P, int64_t B, int64_t n, const double* hist,
                         const double* zmax, const double* zmin, int64_t bounds_stride,
                         const int64_t* lengths, const int64_t* push_steps, const double* profile,
                         int64_t duration, int32_t axes, double max_violation, double mass,
                         double* force, int32_t* limit, double* response, void* stream) {
  return push_map_impl("zmpc_push_map_shaped", true, P,
                       PushCall{B, n, hist, zmax, zmin, bounds_stride, lengths, push_steps,
                                profile, duration, axes, max_violation, mass, force, limit,
                                response},
                       stream);
}

int zmpc_trace_margin(const zmpc_plan* P, int64_t B, int64_t n, const double* hist,
                      const double* zmax, const double* zmin, int64_t bounds_stride,
                      const int64_t* lengths, int64_t draws, const zmpc_trace* trace,
                      double max_violation, double* scale, int32_t* limit) {
  g_err.clear();
  if (!P) return fail(ZMPC_EINVAL, "NULL plan");
  if (int rc = need_walks(B, n)) return rc;
  if (draws < 1) return fail(ZMPC_EINVAL, "need draws >= 1 (traces per walk)");
  if (B > 0x7fffffff / draws) return fail(ZMPC_EINVAL, "batch too large (B * draws rows)");
  if (int rc = trace_check(trace, B * draws)) return rc;
  if (!(max_violation >= 0)) return fail(ZMPC_EINVAL, "need max_violation >= 0");
  if (int rc = need_bounds_stride(bounds_stride, n)) return rc;
  if (B > 0 && (!hist || !zmax || !zmin || !scale))
    return fail(ZMPC_EINVAL, "NULL array argument");
  // (no LDS per sample, so none of the rollouts' 2^24; limit holds 2·i + a in an int32)
  if (n > (1 << 30)) return fail(ZMPC_EINVAL, "walk too long (limit holds 2 * i + a in an int32)");
  // refused before any device call, nothing is launched
  if (P->strict)
    return fail(ZMPC_ESTATE,
                "zmpc_trace_margin: the ZMP response of a strict (clamped) controller is not "
                "affine in the trace's scale (bisect over traced rollouts instead: "
                "ZMPController.critical_force)");
  if (B == 0) return ZMPC_OK;
  DeviceGuard g(P->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  const Disturbance d = trace_of(trace, n, "zmpc_trace_margin");
  const MarginCall c{B,     n,      hist, zmax,          zmin,  bounds_stride, lengths,
                     draws, d.push, d.L,  max_violation, scale, limit};
  return launch_result(zmpc_launch_trace_margin(P, c, (hipStream_t)d.stream), std::string(),
                       d.name);
}

static int herdt_check(const zmpc_plan* P, const zmpc_herdt_params* prm, int64_t B) {
  if (!P || !prm) return fail(ZMPC_EINVAL, "NULL plan or params");
  if (B < 0) return fail(ZMPC_EINVAL, "B < 0");
  for (int sd = 0; sd < 2; ++sd)
    if (prm->nfacets[sd] < 3 || prm->nfacets[sd] > ZMPC_HERDT_MAX_FACETS)
      return fail(ZMPC_EINVAL, "polytope facets must be in [3, 16]");
  static_assert(kHerdtMaxFootsteps == 8, "the message states the limit");
  if (prm->max_footsteps < 0 || prm->max_footsteps > kHerdtMaxFootsteps)
    return fail(ZMPC_EINVAL, "max_footsteps must be in [0, 8]");
  if (prm->max_passes < 0 || prm->max_passes > 100000)
    return fail(ZMPC_EINVAL, "max_passes must be in [0, 100000] (0: default)");
  if (!(prm->alpha > 0) || !(prm->beta >= 0) || !(prm->gamma > 0))
    return fail(ZMPC_EINVAL, "need alpha > 0, beta >= 0, gamma > 0");
  return ZMPC_OK;
}

// A filled call of the three Herdt rollouts under its disturbance: its checks, and its launch
static int herdt_rollout_impl(const zmpc_plan* P, const zmpc_herdt_params* prm, HerdtCall c,
                              const Disturbance& d) {
  if (int rc = herdt_check(P, prm, c.B)) return rc;
  if (c.n < 1) return fail(ZMPC_EINVAL, "need n >= 1");
  if (c.B == 0) return ZMPC_OK;
  if (!c.vref || !c.st || !c.nb || !c.x0 || !c.hist || !c.foot)
    return fail(ZMPC_EINVAL, "NULL array argument");
  if (c.B > 0x7fffffff || c.n > (1 << 24)) return fail(ZMPC_EINVAL, "batch too large");
  if ((c.vs != 0 && c.vs < 2 * c.n) || (c.ss != 0 && c.ss < c.n) || (c.ns != 0 && c.ns < c.n))
    return fail(ZMPC_EINVAL, "strides must be 0 (shared) or cover a whole walk");
  DeviceGuard g(P->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  hipStream_t s = (hipStream_t)d.stream;
  if (c.status) {
    hipError_t e = hipMemsetAsync(c.status, 0, sizeof(int32_t) * c.B, s);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync");
  }
  c.push = d.push;
  std::string why;
  return launch_result(zmpc_launch_herdt_rollout(P, prm, c, s, &why), why, d.name);
}

// The walks of a Herdt rollout call: no kick, no push
static HerdtCall herdt_walks(int64_t B, int64_t n, const double* v_ref, int64_t v_stride,
                             const int8_t* states, int64_t s_stride, const int32_t* nb_next,
                             int64_t nb_stride, const double* x0, double* hist, double* foot,
                             int32_t* status) {
  HerdtCall c{};
  c.B = B, c.n = n, c.vref = v_ref, c.vs = v_stride, c.st = states, c.ss = s_stride;
  c.nb = nb_next, c.ns = nb_stride, c.x0 = x0, c.kick_step = -1;
  c.hist = hist, c.foot = foot, c.status = status;
  return c;
}

int zmpc_herdt_rollout(const zmpc_plan* P, const zmpc_herdt_params* prm, int64_t B, int64_t n,
                       const double* v_ref, int64_t v_stride, const int8_t* states,
                       int64_t s_stride, const int32_t* nb_next, int64_t nb_stride,
                       const double* x0, const double* kick, int64_t kick_step, double* hist,
                       double* foot, int32_t* status, void* stream) {
  g_err.clear();
  HerdtCall c = herdt_walks(B, n, v_ref, v_stride, states, s_stride, nb_next, nb_stride, x0, hist,
                            foot, status);
  c.kick = kick, c.kick_step = kick_step;
  return herdt_rollout_impl(P, prm, c, kick_of(stream, "zmpc_herdt_rollout"));
}

int zmpc_herdt_rollout_pushed(const zmpc_plan* P, const zmpc_herdt_params* prm, int64_t B,
                              int64_t n, const double* v_ref, int64_t v_stride,
                              const int8_t* states, int64_t s_stride, const int32_t* nb_next,
                              int64_t nb_stride, const double* x0, const zmpc_push* push,
                              double* hist, double* foot, int32_t* status, void* stream) {
  g_err.clear();
  if (!P || !prm) return fail(ZMPC_EINVAL, "NULL plan or params");
  if (int rc = push_check(push, B)) return rc;
  HerdtCall c = herdt_walks(B, n, v_ref, v_stride, states, s_stride, nb_next, nb_stride, x0, hist,
                            foot, status);
  if (!push_is_kick(push) || push->steps)
    return herdt_rollout_impl(P, prm, c,
                              window_of(push, n, stream, "zmpc_herdt_rollout_pushed"));
  // what users get today: zmpc_herdt_rollout's kick, under its name
  c.kick = push->amp, c.kick_step = push->step;
  return herdt_rollout_impl(P, prm, c, kick_of(stream, "zmpc_herdt_rollout"));
}

int zmpc_herdt_rollout_traced(const zmpc_plan* P, const zmpc_herdt_params* prm, int64_t B,
                              int64_t n, const double* v_ref, int64_t v_stride,
                              const int8_t* states, int64_t s_stride, const int32_t* nb_next,
                              int64_t nb_stride, const double* x0, const zmpc_trace* trace,
                              double* hist, double* foot, int32_t* status) {
  g_err.clear();
  if (!P || !prm) return fail(ZMPC_EINVAL, "NULL plan or params");
  if (int rc = trace_check(trace, B)) return rc;
  return herdt_rollout_impl(P, prm,
                            herdt_walks(B, n, v_ref, v_stride, states, s_stride, nb_next,
                                        nb_stride, x0, hist, foot, status),
                            trace_of(trace, n < 1 ? 1 : n, "zmpc_herdt_rollout_traced"));
}

int zmpc_herdt_walk_metrics(const zmpc_plan* P, const zmpc_herdt_params* prm, int64_t B,
                            int64_t n, const double* hist, const double* foot,
                            const int8_t* states, int64_t s_stride, const double* foot_ref,
                            int64_t foot_ref_stride, const int64_t* lengths, double count_tol,
                            double* metrics, void* stream) {
  g_err.clear();
  if (!P || !prm) return fail(ZMPC_EINVAL, "NULL plan or params");
  if (int rc = need_walks(B, n)) return rc;
  if (!(count_tol >= 0)) return fail(ZMPC_EINVAL, "need count_tol >= 0");
  for (int sd = 0; sd < 2; ++sd)
    if (prm->nfacets[sd] < 0 || prm->nfacets[sd] > ZMPC_HERDT_MAX_FACETS)
      return fail(ZMPC_EINVAL, "polytope facets must be in [0, 16]");
  if ((s_stride != 0 && s_stride < n) || (foot_ref_stride != 0 && foot_ref_stride < 2 * n))
    return fail(ZMPC_EINVAL, "s_stride must be 0 (shared) or >= n, foot_ref_stride 0 or >= 2n");
  if (B > 0 && (!hist || !foot || !states || !metrics))
    return fail(ZMPC_EINVAL, "NULL array argument");
  if (int rc = need_batch(B)) return rc;
  if (int rc = need_length(n)) return rc;
  if (B == 0) return ZMPC_OK;
  DeviceGuard g(P->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  hipError_t e = zmpc_launch_herdt_walk_metrics(P, prm, B, n, hist, foot, states, s_stride,
                                                foot_ref, foot_ref_stride, lengths, count_tol,
                                                metrics, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "zmpc_herdt_walk_metrics launch");
  return ZMPC_OK;
}

int zmpc_herdt_prepare(const zmpc_plan* P, int64_t B, int64_t n, const int8_t* states,
                       int64_t s_stride, const int64_t* lengths, int8_t* states_out,
                       int32_t* nb_next, int32_t* max_steps, int32_t* max_footsteps_host) {
  g_err.clear();
  if (!P) return fail(ZMPC_EINVAL, "NULL plan");
  if (int rc = need_walks(B, n)) return rc;
  if (int rc = need_length(n)) return rc;
  if (int rc = need_batch(B)) return rc;
  if (B > 0 && (!states || !nb_next)) return fail(ZMPC_EINVAL, "NULL array argument");
  if (s_stride != 0 && s_stride < n)
    return fail(ZMPC_EINVAL, "s_stride must be 0 (shared) or >= n");
  if (max_footsteps_host) *max_footsteps_host = 0;
  if (B == 0) return ZMPC_OK;
  DeviceGuard g(P->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  // whatever stream produced `states` has finished before the kernel reads them
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return hip_fail(e, "hipDeviceSynchronize");
  int32_t* word = nullptr;  // the batch's largest footstep count
  if (max_footsteps_host) {
    if (hipMalloc(&word, sizeof(int32_t)) != hipSuccess)
      return fail(ZMPC_ENOMEM, "zmpc_herdt_prepare: device workspace allocation failed");
    e = hipMemset(word, 0, sizeof(int32_t));
  }
  if (e == hipSuccess)
    e = zmpc_launch_herdt_prepare(P, B, n, states, s_stride, lengths, states_out, nb_next,
                                  max_steps, word, nullptr);
  // every output is complete when the call returns (the copy of the word waits for the kernel)
  if (e == hipSuccess)
    e = word ? hipMemcpy(max_footsteps_host, word, sizeof(int32_t), hipMemcpyDeviceToHost)
             : hipDeviceSynchronize();
  if (word) (void)hipFree(word);
  if (e != hipSuccess) return hip_fail(e, "zmpc_herdt_prepare");
  return ZMPC_OK;
}

int zmpc_herdt_step(const zmpc_plan* P, const zmpc_herdt_params* prm, int64_t B,
                    const double* x, const double* v_win, const int8_t* s_win,
                    const int8_t* current, const double* foot, const int8_t* side,
                    double* x_next, double* step, int32_t* status, void* stream) {
  g_err.clear();
  int rc = herdt_check(P, prm, B);
  if (rc != ZMPC_OK) return rc;
  if (B == 0) return ZMPC_OK;
  if (!x || !v_win || !s_win || !current || !foot || !side || !x_next || !step)
    return fail(ZMPC_EINVAL, "NULL array argument");
  if (int rc = need_batch(B)) return rc;
  DeviceGuard g(P->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  std::string why;
  const HerdtStepCall c{B, x, v_win, s_win, current, foot, side, x_next, step, status};
  return launch_result(zmpc_launch_herdt_step(P, prm, c, (hipStream_t)stream, &why), why,
                       "zmpc_herdt_step");
}

int zmpc_cop_generate(int device, int64_t B, const double* params, int64_t n_cap,
                      double* zmax, double* zmin, int8_t* states, int64_t* n_out,
                      void* stream) {
  g_err.clear();
  if (B < 0 || n_cap < 0) return fail(ZMPC_EINVAL, "need B >= 0 and n_cap >= 0");
  if (B == 0) return ZMPC_OK;
  if (!params) return fail(ZMPC_EINVAL, "params is NULL");
  if (n_cap > 0 && (!zmax || !zmin)) return fail(ZMPC_EINVAL, "NULL output bounds");
  if (n_cap == 0 && !n_out) return fail(ZMPC_EINVAL, "n_cap = 0 needs n_out");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
  if (device < 0 || device >= ndev) return fail(ZMPC_EINVAL, "device index out of range");
  DeviceGuard g(device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  e = zmpc_launch_cop(B, params, n_cap, n_cap > 0 ? zmax : nullptr, n_cap > 0 ? zmin : nullptr,
                      n_cap > 0 ? states : nullptr, n_out, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "zmpc_cop_generate launch");
  return ZMPC_OK;
}

}  // extern "C"
