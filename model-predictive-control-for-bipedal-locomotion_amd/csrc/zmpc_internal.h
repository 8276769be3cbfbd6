// Internal declarations shared by the HIP translation units of libzmpc.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "dispatch.h"
#include "zmpc.h"

// Scalar LIPM constants of zmp_controller.py:18-20 (A = [[1,T,T²/2],[0,1,T],[0,0,1]],
// B = [T³/6, T²/2, T]ᵀ), evaluated on the host as Python evaluates them.
// Rollout scan propagators per chunk width C = 1..8: (Ā^C)^(2^r), r = 0..kScanLevels-1
// (64-lane Kogge-Stone rounds use r <= 5; the 128-lane kernels' cross-wave offset uses r = 6).
constexpr int kScanLevels = 7;
constexpr int kScanStride = kScanLevels * 9;
// ... followed by the per-lane powers (Ā^C)^k, k = 0..32, [8][33][9] (the DPP scan's cross-row
// steps, rollout_common.h scan_dpp)
constexpr int kScanPowOff = 8 * kScanStride;
// ... and the chunk-sum columns Ā^p B, Ā^p e1 (p = 0..7), [8][6] (rollout.hip split_walk: a
// lane's chunk end state Σ_q Ā^(C−1−q) B f_q, and the kick's Ā^(C−1−q) e1)
constexpr int kScanGOff = kScanPowOff + 8 * 33 * 9;
constexpr int kScanDoubles = kScanGOff + 8 * 6;

struct LipmConsts {
  double T;     // A[0,1] = A[1,2] = B[2]
  double T2_2;  // A[0,2] = B[1]
  double T3_6;  // B[0]
};

struct zmpc_plan {
  int device = 0;
  int cus = 0;      // compute units of the plan's device (grid sizing of the launches)
  int N = 0;        // horizon (nb_steps)
  int Kpad = 0;     // N rounded up to a multiple of 16, the zero-padded length of k
  int strict = 0;
  double T = 0, T2_2 = 0, T3_6 = 0, hg = 0, Thg = 0, Q = 1, R = 0;
  LipmConsts lc{};
  // device buffers
  double* p = nullptr;   // [N] Toeplitz column of Pu
  double* Px = nullptr;  // [N,3]
  double* M = nullptr;   // [N,N] PuᵀPu + (R/Q) I
  double* L = nullptr;   // [N,N] lower Cholesky factor of M
  double* k = nullptr;   // [Kpad] gain row e0ᵀ M⁻¹ Puᵀ (zero-padded)
  double* kx = nullptr;  // [3]  k·Px
  double* kffa = nullptr;  // [kffa_rows(N)][4] two-parallel fast-FIR taps of k (rollout.hip):
                           // (E_m, O_m, E_m + O_{m−1}, 0), E_m = k_{2m}, O_m = k_{2m+1}, zero past N
  double* ksum = nullptr;  // [ksum_rows(N)] suffix sums of k for the sparse-difference
                           // correlation (rollout.hip axis_correlate_sparse; layout at ksum_rows)
  double* scanP = nullptr;  // [8][kScanLevels][9] (Ā^C)^(2^r) rollout scan propagators, then
                            // [8][33][9] (Ā^C)^k (kScanPowOff)
  double* X = nullptr;   // [N,N] L⁻¹ Puᵀ (strict plans)
  double* G = nullptr;   // [N,N] Pu (R I + Q PuᵀPu)⁻¹ Puᵀ (strict plans)
  double* v = nullptr;   // [N]   first column of Pu⁻¹ (strict plans)
  double* Hz = nullptr;  // [N,N] Q I + R Pu⁻ᵀPu⁻¹ = G⁻¹ (strict plans)
  int* info = nullptr;   // [1] factorisation status
  // strict reduced-Cholesky solver (strict.hip): persistent-grid slots (its factor scratch is
  // allocated per launch, stream-ordered)
  int strict_slots = 0;
  // strict LQ solver (strict_lq.hip): free-tail Riccati table [N][16] and work counters
  double* lqtab = nullptr;
  unsigned long long* lqcnt = nullptr;  // [ZMPC_NCOUNTERS]
  // FFT correlation of long unconstrained walks (rollout_long.hip): twiddles e^{−2πi m/PT}
  // [PT] complex, and per transform size P = 2^p in [kFftPmin, PT] the spectrum of the
  // gain kernel g[d] = k_{d−1} (d = 1..N), DFT(g)/P, at complex offset P − kFftPmin
  double* fft_tw = nullptr;
  double* fft_g = nullptr;
  // plan-build stage durations (zmpc_plan_timings), milliseconds
  float stage_ms[ZMPC_PLAN_STAGES] = {};
  // algorithm options (zmpc_plan_set_option), defaults as include/zmpc.h
  int opt[ZMPC_NOPTIONS] = {0, 0, 0, 1, 0, 0};
};

// rows of the fast-FIR tap table: m = 0..⌈(N+1)/2⌉−1, plus zero rows for an unrolled loop
__host__ __device__ constexpr int kffa_rows(int N) { return (N + 2) / 2 + 8; }

// (ksum_rows / ksum_s0, the layout of the suffix sums of k, and the FFT table sizes kFftPT,
// kFftPmin, kFftGComplex are in dispatch.h: they enter the LDS budgets of the launch rules)

// The push window of a pushed rollout (include/zmpc.h, "The push, stated once") as the strict and
// Herdt kernels take it, by value inside their argument structs.  All zero means the legacy
// one-sample y kick of the struct's own kick fields, so a zero-initialised argument struct filled
// by name behaves as before.  A per-walk trace (include/zmpc.h, "The trace, stated once") is the
// same window with a value per (walk, step, axis): amp is dv [B, L, cols], tstride = cols and
// astride = L·cols; a window has tstride = 0 and astride = cols.
struct PushArgs {
  const double* amp;     // [B, cols] device, or null: the legacy kick; a trace: dv [B, L, cols]
  const double* w;       // [dur] device profile, or null: ones (no product)
  const int64_t* steps;  // [B] start steps, or null: step
  int64_t step;
  int dur;     // D, clamped to n by the launcher (a push past the walk's end is truncated anyway)
  int cols;    // C, the columns of amp
  int col[2];  // the column of axis a (0: x, 1: y) in amp, −1: the axis is not pushed
  int tstride;      // doubles between consecutive samples of a walk's trace, 0: a window
  int64_t astride;  // doubles between consecutive walks of amp
};

// "no push" as a start step: (unsigned)(i − kNoPush) >= 2^31 for every timestep 0 <= i < 2^24
constexpr int kNoPush = 0x7fffffff;

// Where the amplitude of (walk b, axis) is read, null when the axis takes no push: amp[b, col] of
// a push window (dv[b, 0, col] of a trace), kick[b] on the y axis otherwise.  TRACE fixes the form
// at compile time for a kernel that keeps the trace in instantiations of its own (herdt.hip):
// false strides by the window's columns, as before the trace existed.
template <bool TRACE>
__host__ __device__ inline const double* push_amp_t(const PushArgs& p, const double* kick,
                                                    int64_t b, int axis) {
  if (p.amp)
    return p.col[axis] >= 0 ? p.amp + b * (TRACE ? p.astride : (int64_t)p.cols) + p.col[axis]
                            : nullptr;
  return (kick && axis == 1) ? kick + b : nullptr;
}

// ... with the form read from the struct: astride is the window's columns too
__host__ __device__ inline const double* push_amp(const PushArgs& p, const double* kick,
                                                  int64_t b, int axis) {
  return push_amp_t<true>(p, kick, b, axis);
}

// The start step of walk b's push in a walk of n samples, kNoPush outside [0, n − 1).
__host__ __device__ inline int push_start(const PushArgs& p, const int64_t* kick_steps,
                                          int64_t kick_step, int64_t b, int64_t n) {
  const int64_t s = p.amp ? (p.steps ? p.steps[b] : p.step)
                          : (kick_steps ? kick_steps[b] : kick_step);
  return (s >= 0 && s < n - 1) ? (int)s : kNoPush;
}

// The window's length as the range test (unsigned)(i − start) < D takes it
__host__ __device__ inline unsigned push_dur(const PushArgs& p) {
  return p.amp ? (unsigned)p.dur : 1u;
}

// What sample i + 1's velocity is lowered by at j = i − start, read at the point of use: a trace's
// own entry of step j as it is; of a window the amplitude itself without a profile, so that D = 1
// is the legacy kick's arithmetic.
template <bool TRACE>
__host__ __device__ inline double push_value_t(const PushArgs& p, const double* ap, unsigned j) {
  if (TRACE) return ap[(size_t)j * (unsigned)p.tstride];
  const double am = *ap;
  return p.w ? am * p.w[j] : am;
}

__host__ __device__ inline double push_value(const PushArgs& p, const double* ap, unsigned j) {
  return p.tstride ? push_value_t<true>(p, ap, j) : push_value_t<false>(p, ap, j);
}

// The arguments of one zmpc_rollout / zmpc_rollout_kicks / zmpc_rollout_pushed call
// (include/zmpc.h), filled once in capi.hip and handed down by reference.
struct RolloutCall {
  int64_t B, n;
  const double *zmax, *zmin;
  int64_t bstride;  // bounds stride in doubles, 0: one shared CoP
  const double *x0, *kick;
  int64_t kick_step;
  const int64_t* kick_steps;  // per-walk kick steps, or null: kick_step
  double* hist;
  int32_t* status;  // may be null
  PushArgs push;    // zmpc_rollout_pushed: the window (kick is null then); all zero otherwise
};

// The arguments of one zmpc_step call.
struct StepCall {
  int64_t B;
  const double *x, *zmax_win, *zmin_win;
  double* x_next;
  int32_t* status;  // may be null
};

// The arguments of one zmpc_herdt_rollout / zmpc_herdt_rollout_pushed call.
struct HerdtCall {
  int64_t B, n;
  const double* vref;  // [B,n,2], stride vs doubles per walk (0: one shared [n,2])
  int64_t vs;
  const int8_t* st;    // [B,n] support states, stride ss
  int64_t ss;
  const int32_t* nb;   // [B,n] steps to the next footstep change, stride ns
  int64_t ns;
  const double *x0, *kick;  // kick may be null
  int64_t kick_step;
  PushArgs push;       // zmpc_herdt_rollout_pushed: the window (kick is null then); else all zero
  double *hist, *foot; // [B,n,2,3], [B,n,2]
  int32_t* status;     // may be null
};

// The arguments of one zmpc_herdt_step call: windows of the plan's N rows per walk.
struct HerdtStepCall {
  int64_t B;
  const double *x, *v_win;   // [B,2,3], [B,N,2]
  const int8_t *s_win, *current;  // [B,N], [B]
  const double* foot;        // [B,2] the current foot
  const int8_t* side;        // [B] its side (0 left)
  double *x_next, *step;     // [B,2,3]; [B,2] the first footstep (NaN without one in the window)
  int32_t* status;           // may be null
};

// kernels launchers (plan.hip); ev (may be NULL): ZMPC_PLAN_STAGES events, ev[0] recorded
// before the first stage and ev[i + 1] after stage i for stages 0..9 of include/zmpc.h
// zmpc_plan_timings (stages the plan skips record their event right after the previous one);
// the caller records ev[11] after stage 10 (the strict LQ table)
hipError_t zmpc_launch_plan(zmpc_plan* p, hipStream_t s, hipEvent_t* ev);

// batched CoP-bound producer (cop.hip): params [B][7] = distance, step_length, foot_spread,
// ssp, dsp, standing, dt; n_cap = 0 counts only (n_out)
hipError_t zmpc_launch_cop(int64_t B, const double* params, int64_t n_cap, double* zmax,
                           double* zmin, int8_t* states, int64_t* n_out, hipStream_t s);

// per-walk robustness metrics of a state history (metrics.hip): one wavefront per walk, reads
// only p->hg and p->cus; lengths may be NULL (every walk has n live samples)
hipError_t zmpc_launch_walk_metrics(const zmpc_plan* p, int64_t B, int64_t n, const double* hist,
                                    const double* zmax, const double* zmin, int64_t bstride,
                                    const int64_t* lengths, double* metrics, hipStream_t s);

// per-walk survival metrics of a Herdt rollout (herdt_metrics.hip): one wavefront per walk, reads
// only p->hg and, of prm, the foot dimensions, the spread and the facets; foot_ref and lengths
// may be NULL
hipError_t zmpc_launch_herdt_walk_metrics(const zmpc_plan* p, const zmpc_herdt_params* prm,
                                          int64_t B, int64_t n, const double* hist,
                                          const double* foot, const int8_t* states,
                                          int64_t sstride, const double* foot_ref,
                                          int64_t rstride, const int64_t* lengths, double tol,
                                          double* metrics, hipStream_t s);

// footstep bookkeeping of a batch of Herdt walks (herdt_prep.hip): one wavefront per walk, reads
// only p->N; lengths, states_out and max_steps may be NULL; batch_max: one device word that
// holds 0 and receives the largest max_steps of the batch, or NULL
hipError_t zmpc_launch_herdt_prepare(const zmpc_plan* p, int64_t B, int64_t n,
                                     const int8_t* states, int64_t sstride,
                                     const int64_t* lengths, int8_t* states_out,
                                     int32_t* nb_next, int32_t* max_steps, int32_t* batch_max,
                                     hipStream_t s);

// The arguments of one zmpc_push_map / zmpc_push_map_shaped call (zmpc_push_map: duration 1, no
// profile, the y axis).
struct PushCall {
  int64_t B, n;
  const double *hist, *zmax, *zmin;
  int64_t bstride;
  const int64_t* lengths;     // may be null
  const int64_t* push_steps;  // null: the full map, else the single-step form
  const double* profile;      // device, [duration], may be null
  int64_t duration;
  int axes;  // ZMPC_PUSH_AXIS_X, _Y or both: force and limit hold 2 columns per step and axis
  double t;  // max_violation
  double mass;
  double* force;
  int32_t* limit;    // may be null
  double* response;  // may be null
};

// push-robustness maps of a state history (pushmap.hip): the shapes dispatch.h choose_push_map /
// choose_push_shaped take (the caller refuses the others first) on a non-strict plan, whose kx,
// T, T²/2, T³/6 and h/g it reads.  hipErrorOutOfMemory: the response table's stream-ordered
// workspace (2n doubles at duration 1 without a profile, which launches no shaping kernel; 5n
// otherwise) could not be allocated
hipError_t zmpc_launch_push_map(const zmpc_plan* p, const PushCall& c, hipStream_t s);
hipError_t zmpc_push_map_set_attrs();

// the state response of a push window added to an unpushed history of a non-strict plan
// (pushmap.hip): hist[b, s_b + d, a, :] −= amp[b, a]·Σ_j w_j·Ā^(d−j−1)·e1 on the axes of c.push.
// hipErrorOutOfMemory: the stream-ordered workspace (4n doubles, 8n with a profile or D > 1)
hipError_t zmpc_launch_push_response(const zmpc_plan* p, const RolloutCall& c, hipStream_t s);

// the state response of a per-walk trace (c.push in trace form: tstride != 0) subtracted from an
// unpushed history of a non-strict plan (trace.hip): one wave per walk, an O(n) scan, no workspace;
// L: the samples of a walk's trace as the caller gave them (c.push.dur is clamped to n)
hipError_t zmpc_launch_trace_response(const zmpc_plan* p, const RolloutCall& c, int64_t L,
                                      hipStream_t s);

// The arguments of one zmpc_trace_margin call: B walks with `draws` rows each; push is the trace
// of the B·draws rows in trace form (capi.hip), L its samples per row as the caller gave them.
struct MarginCall {
  int64_t B, n;
  const double *hist, *zmax, *zmin;
  int64_t bstride;
  const int64_t* lengths;  // may be null
  int64_t draws;
  PushArgs push;
  int64_t L;
  double t;        // max_violation
  double* scale;   // [B·draws, 2]
  int32_t* limit;  // [B·draws, 2], may be null
};

// the exact critical scale of every row's trace from an unpushed history of a non-strict plan
// (trace_margin.hip): one wave per row, trace.hip's scan, no workspace
hipError_t zmpc_launch_trace_margin(const zmpc_plan* p, const MarginCall& c, hipStream_t s);

// unconstrained rollout / step (rollout.hip)
hipError_t zmpc_launch_rollout_unc(const zmpc_plan* p, const RolloutCall& c, hipStream_t s,
                                   std::string* why);
hipError_t zmpc_launch_step_unc(const zmpc_plan* p, const StepCall& c, hipStream_t s);

// the wide and chunk kernels of long walks (rollout_long.hip), for zmpc_launch_rollout_unc and
// zmpc_rollout_unc_set_attrs alone: the launch of a Wide or Chunk choice with the caller's filled
// RolloutArgs (rollout_common.h; the struct is local to each unit, hence the untyped pointer)
hipError_t zmpc_launch_rollout_long(const UncChoice& c, const void* rollout_args, int cus,
                                    hipStream_t s);
hipError_t zmpc_rollout_long_set_attrs();

// fused rollout-to-metrics (rollout.hip): the shapes dispatch.h choose_unc_metrics takes (the
// caller refuses the others first); c.hist is unused, lengths may be NULL
hipError_t zmpc_launch_rollout_metrics(const zmpc_plan* p, const RolloutCall& c,
                                       const int64_t* lengths, double* metrics, hipStream_t s);

// strict box-QP rollout / step: the solver of the launch by dispatch.h choose_strict, then its
// backend below (strict_dispatch.hip)
hipError_t zmpc_launch_rollout_strict(const zmpc_plan* p, const RolloutCall& c, hipStream_t s,
                                      std::string* why);
hipError_t zmpc_launch_step_strict(const zmpc_plan* p, const StepCall& c, hipStream_t s,
                                   std::string* why);

// strict box-QP by reduced Cholesky (strict.hip): the tile kernel (16 instances per workgroup) and
// the one-instance-per-wave kernel, N <= kStrictCholMaxN; cross-checks of the two below
hipError_t zmpc_launch_rollout_strict_tile(const zmpc_plan* p, const RolloutCall& c,
                                           hipStream_t s, std::string* why);
hipError_t zmpc_launch_step_strict_tile(const zmpc_plan* p, const StepCall& c, hipStream_t s,
                                        std::string* why);
hipError_t zmpc_launch_rollout_strict_wave(const zmpc_plan* p, const RolloutCall& c,
                                           hipStream_t s, std::string* why);
hipError_t zmpc_launch_step_strict_wave(const zmpc_plan* p, const StepCall& c, hipStream_t s,
                                        std::string* why);

// strict box-QP in LQ form, one instance per lane (strict_lq.hip); the default strict path
hipError_t zmpc_launch_rollout_strict_lq(const zmpc_plan* p, const RolloutCall& c, hipStream_t s,
                                         std::string* why);
hipError_t zmpc_launch_step_strict_lq(const zmpc_plan* p, const StepCall& c, hipStream_t s,
                                      std::string* why);
bool zmpc_strict_lq_supported(const zmpc_plan* p);
hipError_t zmpc_strict_lq_set_attrs();
size_t zmpc_strict_lq_table_doubles(int N);
hipError_t zmpc_strict_lq_build_table(zmpc_plan* p, hipStream_t s);

// strict box-QP for small batches, one instance per wave, parallel in time (strict_scan.hip)
hipError_t zmpc_launch_rollout_strict_scan(const zmpc_plan* p, const RolloutCall& c,
                                           hipStream_t s, std::string* why);
hipError_t zmpc_launch_step_strict_scan(const zmpc_plan* p, const StepCall& c, hipStream_t s,
                                        std::string* why);
bool zmpc_strict_scan_supported(const zmpc_plan* p);

// walk order for the lane-per-instance kernels (order.hip): perm[B] = the walks sorted by
// (kick step, kick) — of a push window (push.amp set) by (start step, the larger |amp| of its
// axes) — so that a wave's lanes take similar disturbances; ws of zmpc_kick_order_bytes(B) bytes
// (device, stream-ordered)
size_t zmpc_kick_order_bytes(int64_t B);
hipError_t zmpc_kick_order(const double* kick, const int64_t* kick_steps, int64_t kick_step,
                           const PushArgs& push, int64_t B, int32_t* perm, void* ws,
                           hipStream_t s);

// Herdt joint footstep QP (herdt.hip); support states as cop_generator.State
constexpr int ZMPC_STANDING = 0, ZMPC_DOUBLE_SUPPORT = 1, ZMPC_SINGLE_SUPPORT = 2;
hipError_t zmpc_launch_herdt_rollout(const zmpc_plan* p, const zmpc_herdt_params* prm,
                                     const HerdtCall& c, hipStream_t s, std::string* why);
hipError_t zmpc_launch_herdt_step(const zmpc_plan* p, const zmpc_herdt_params* prm,
                                  const HerdtStepCall& c, hipStream_t s, std::string* why);
hipError_t zmpc_herdt_set_attrs();

hipError_t zmpc_rollout_unc_set_attrs();
hipError_t zmpc_strict_set_attrs();
