/*
 * zmpc.h — C-ABI of the MI355X batched Wieber LIPM-ZMP MPC solver (libzmpc.so).
 *
 * This is the drop-in boundary for the reference hot path
 *   src/mpc_bipedal/controllers/zmp_controller.py  (ZMPController, reference @ 2025-12-26)
 * Every entry point names the reference code it replaces.  The Python host layer
 * (mpc_bipedal/_native.py, ctypes) binds exactly these symbols; see INTEGRATION.md.
 *
 * Conventions
 *  - All array pointers are DEVICE pointers (e.g. torch tensor .data_ptr()), contiguous,
 *    IEEE fp64 unless stated.  Nothing is copied to or from the host by the solve calls.
 *  - Calls are asynchronous on `stream` (a hipStream_t; NULL = the null stream).
 *  - Return 0 on success, a negative ZMPC_E* code on failure; zmpc_last_error() returns a
 *    thread-local message for the last failure on the calling thread.  No C++ exception
 *    crosses the ABI.
 *  - A plan is immutable after creation (and after its zmpc_plan_set_option calls, which
 *    belong before it is shared) and may be shared across threads and streams of its device.
 *  - The library reads no environment variable that changes a result: algorithm choices are
 *    explicit plan options (zmpc_plan_set_option); diagnostic ablations exist only in the
 *    separate diagnostics build (make diag → libzmpc_diag.so, -DZMPC_DIAG).
 *  - status[b] (int32, may be NULL) receives ZMPC_OK, or a per-instance failure flag
 *    (ZMPC_ST_*).  The reference raises RuntimeError("QP solver did not find a solution")
 *    for a failed strict solve (zmp_controller.py:193-194); the host layer does the same
 *    when any status is non-zero.
 */
#ifndef ZMPC_H
#define ZMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZMPC_ABI_VERSION 7

/* return codes */
#define ZMPC_OK 0
#define ZMPC_EINVAL (-1)   /* bad argument (size, pointer, range) */
#define ZMPC_EHIP (-2)     /* HIP runtime error (message has hipGetErrorString) */
#define ZMPC_ENOMEM (-3)   /* device allocation failed */
#define ZMPC_ESTATE (-4)   /* plan does not support the request (e.g. strict workspace) */

/* per-instance status flags (bitwise OR) */
#define ZMPC_ST_MAXITER 1  /* strict active-set iteration cap reached */
#define ZMPC_ST_NONFINITE 2 /* a non-finite value was produced (unconstrained walks of more than
                               513 samples: also a non-finite bound at sample 0, which no
                               window reads) */
#define ZMPC_ST_FACTOR 4   /* reduced KKT matrix not positive definite (Herdt: also a
                              window with more footsteps than params.max_footsteps, flagged
                              on every walk of its 32-walk wave) */
#define ZMPC_ST_INFEASIBLE 8 /* Herdt: the swing polytope has no usable facet and the
                                unconstrained footstep lies outside it (degenerate or
                                unbounded half-spaces); since ABI 5 */

typedef struct zmpc_plan zmpc_plan;

/*
 * Build the batch-invariant solver plan on `device` (stream-ordered on `stream`, then
 * synchronised): the Toeplitz column p of Pu and Px (zmp_controller.py:162-171, built on
 * the device from the host-evaluated constants so they match the reference bit for bit),
 * M = PuᵀPu + (R/Q)·I (FP64 MFMA when N >= 64, zmp_controller.py:198), its Cholesky
 * factor, the gain row k = e0ᵀ M⁻¹ Puᵀ and kx = k·Px (the only part of
 * -inv(M) Puᵀ (Px x - z_ref) the reference uses, X[0], zmp_controller.py:198-199) and,
 * when strict != 0, the z-space inverse Hessian G = Pu (R·I + Q·PuᵀPu)⁻¹ Puᵀ of the
 * strict QP (zmp_controller.py:173-195).
 * Replaces the per-call matrix build in ZMPController.predict_wieber_axis
 * (zmp_controller.py:162-171) and the inverse at :198.
 *   T, T2_2 = T²/2, T3_6 = T³/6, hg = h/g, Thg = T·h/g: as Python evaluates them
 *   (mpc_bipedal/models/lipm_model.py:plan_constants).
 */
int zmpc_plan_create(int device, int32_t N, double T, double T2_2, double T3_6, double hg,
                     double Thg, double Q, double R, int32_t strict, void* stream,
                     zmpc_plan** out);

/* Release a plan (synchronises its device). */
int zmpc_plan_destroy(zmpc_plan* plan);

/* Plan quantities copied to HOST memory for inspection/tests.
 * what: 0 = p (N), 1 = Px (N*3, row-major), 2 = M (N*N), 3 = gain k (N), 4 = kx (3),
 *       5 = G (N*N, strict plans only), 6 = Cholesky factor L of M (N*N, lower),
 *       7 = Hz = Q·I + R·Pu⁻ᵀPu⁻¹ = G⁻¹ (N*N, strict plans only).
 * The derived tables the kernels read (additive to ABI 7; layouts as csrc/zmpc_internal.h and
 * csrc/dispatch.h document them):
 *       8 = fast-FIR taps of k ((N + 2)/2 + 8 rows of 4: E_m, O_m, E_m + O_{m−1}, 0),
 *       9 = suffix sums of k (N + 18: S_{i−8} at 9 <= i <= N + 7, S_0 at N + 16, zero elsewhere),
 *       10 = rollout scan tables (2928: [8][7][9] (Ā^C)^(2^r), then [8][33][9] (Ā^C)^k, then
 *            [8][6] (Ā^p·B, Ā^p·e1)),
 *       11 = X = L⁻¹·Puᵀ (N*N, strict plans only), 12 = v = first column of Pu⁻¹ (N, strict
 *            plans only),
 *       13 = FFT twiddles e^{−2πi m/8192} (2*8192, re/im interleaved), 14 = gain spectra
 *            DFT(g)/P for P = 256, 512, .., 8192 at complex offset P − 256 (2*16128).
 * count = number of doubles dst can hold; must be >= the quantity's size.  A quantity the plan
 * does not hold returns ZMPC_ESTATE, an unknown id or a short destination ZMPC_EINVAL. */
int zmpc_plan_export(const zmpc_plan* plan, int32_t what, double* dst_host, int64_t count);

/*
 * Work counters of a plan's active-set solvers, summed over its launches since creation or the
 * last reset (diagnostics for the roofline accounting; the reference has no equivalent).
 * Copied to HOST memory after synchronising the plan's device.  Strict box-QP solver
 * (zmpc_step / zmpc_rollout on a strict plan):
 *   [0] wave passes   (active-set passes of a 64-instance wave, lockstep)
 *   [1] instance passes (active-set iterations summed over instances and timesteps)
 *   [2] instance-slots through the working-set Riccati step (the rest of the
 *       [1] x N instance-slots took the free-tail step)
 *   [3] launches
 * Herdt joint footstep QP (zmpc_herdt_rollout / zmpc_herdt_step, any plan; since ABI 4):
 *   [4] wave passes, [5] instance passes (one instance = one walk axis),
 *   [6] sum over instance passes of the window's footstep count m, [7] the same of m^2
 * Maxima (since ABI 6): [8] the most active-set passes any one strict solve took,
 *   [9] the same for the Herdt solver (passes of the solve's lane pair)
 * count = number of uint64 dst can hold (at most ZMPC_NCOUNTERS are written); reset != 0
 * zeroes the counters after the copy.  Since ABI 3 ([0..3]); [4..7] since ABI 4; [8..9]
 * since ABI 6.
 */
#define ZMPC_NCOUNTERS 10
int zmpc_plan_counters(const zmpc_plan* plan, uint64_t* dst_host, int32_t count, int32_t reset);

/*
 * Durations in milliseconds of the plan-build stages of zmpc_plan_create (HIP events recorded
 * on the creation stream between the stages; the reference rebuilds the same quantities in
 * every predict_wieber_axis call, zmp_controller.py:162-171,198).  Since ABI 5.
 *   [0] p, Px                        [1] M = PuᵀPu + (R/Q)·I (FP64 MFMA Gram at N >= 64)
 *   [2] Cholesky M = L·Lᵀ (blocked)  [3] gain row k, kx (two triangular solves)
 *   [4] rollout scan propagators     [5] FFT correlation tables
 *   [6] strict: X = L⁻¹·Puᵀ          [7] strict: G = XᵀX / Q (FP64 MFMA Gram)
 *   [8] strict: v = Pu⁻¹·e0          [9] strict: Hz = Q·I + R·VᵀV (FP64 MFMA Gram), Hz's own
 *                                        Cholesky factor and, where its pivots spread less than
 *                                        M's, G again as Hz⁻¹ from that factor
 *   [10] strict: LQ free-tail table  [11] total
 * Stages a plan does not run read 0.  count = floats dst can hold (at most ZMPC_PLAN_STAGES
 * are written).
 */
#define ZMPC_PLAN_STAGES 12
int zmpc_plan_timings(const zmpc_plan* plan, float* dst_host, int32_t count);

/*
 * Algorithm selection on a plan (since ABI 7).  Every option chooses between forms that compute
 * the same solution — bitwise for ZMPC_OPT_KICK_ORDER, to rounding for the others (the tests hold
 * each pair to <= 1e-11 on O(1) states); zmpc_plan_create sets the defaults (value 0 unless
 * stated).  For cross-checks and A/B timing; the reference has no counterpart.
 *   ZMPC_OPT_CORRELATION    unconstrained rollouts: 0 = auto (the sparse-difference correlation
 *                           for walks whose z_ref changes at most 40 (64 for walks of more than
 *                           513 samples) times per axis), 1 = the dense forms only
 *   ZMPC_OPT_LONG_WALK      unconstrained walks of more than 513 samples: 0 = auto,
 *                           1 = direct correlation, 2 = FFT correlation (where the transform
 *                           fits the workgroup), 3 = the chunked one-wave kernel
 *   ZMPC_OPT_ROLLOUT_KERNEL unconstrained walks of at most 513 samples: 0 = auto, 1 = the
 *                           one-wave-per-walk kernel (the cross-check of the split kernels)
 *   ZMPC_OPT_KICK_ORDER     strict rollouts: 1 = walks mapped to lanes in (kick step, kick)
 *                           order (default), 0 = input order
 *   ZMPC_OPT_STRICT_SOLVER  strict plans: 0 = auto (small batches — up to 16384 (walk, axis)
 *                           instances — the parallel-in-time one-instance-per-wavefront kernel,
 *                           larger ones the LQ lane-per-instance kernel), 1 = the reduced-
 *                           Cholesky tile kernel (16 instances per workgroup; cross-check),
 *                           2 = the reduced-Cholesky one-instance-per-wavefront kernel
 *                           (cross-check), 3 = the LQ kernel, 4 = the parallel-in-time kernel
 *                           (1 and 2: horizons up to 512; 4: up to 960)
 *   ZMPC_OPT_STRICT_BOUNDS  strict rollouts on the LQ kernel: 0 = auto (run-length bounds;
 *                           rows for a shared CoP before round 5), 1 = the bounds staged one row
 *                           per sample, 2 = run-length bounds (one entry per run of equal
 *                           bounds); bitwise the same results
 * Returns ZMPC_EINVAL for an unknown option or value.
 */
#define ZMPC_OPT_CORRELATION 0
#define ZMPC_OPT_LONG_WALK 1
#define ZMPC_OPT_ROLLOUT_KERNEL 2
#define ZMPC_OPT_KICK_ORDER 3
#define ZMPC_OPT_STRICT_SOLVER 4
#define ZMPC_OPT_STRICT_BOUNDS 5
#define ZMPC_NOPTIONS 6
int zmpc_plan_set_option(zmpc_plan* plan, int32_t option, int64_t value);
int zmpc_plan_get_option(const zmpc_plan* plan, int32_t option, int64_t* value);

/*
 * Batched ZMPController.predict_wieber_axis (zmp_controller.py:149-201):
 * B independent one-axis QP solves, one per instance b:
 *   x[b] (3) state, zmax_win[b], zmin_win[b] (N) the preview window
 *   → x_next[b] (3) = A x + B·u0, u0 = first jerk of the QP solution
 *     (unconstrained: :196-198; strict box-QP: :173-195).
 */
int zmpc_step(const zmpc_plan* plan, int64_t B, const double* x, const double* zmax_win,
              const double* zmin_win, double* x_next, int32_t* status, void* stream);

/*
 * Batched Wieber rollout: ZMPController.generate_com_trajectory_wieber
 * (zmp_controller.py:59-108) and generate_state_trajectory_wieber (:110-147) for B walks.
 *   zmax, zmin : [B, n, 2]   CoP bounds per walk (x, y); the window at step i is rows
 *                            i+1 .. i+N, padded with the last row (:81-88)
 *   bounds_stride            doubles between consecutive walks' bound arrays: 2n for a
 *                            dense [B,n,2] batch, 0 when every walk shares one CoP
 *                            (e.g. a disturbance sweep over one footstep plan)
 *   x0         : [B, 2, 3]   initial (x-axis, y-axis) states
 *   kick       : [B] or NULL velocity impulse dt·F_ext/m subtracted from the y state
 *                            produced at step kick_step (:90,105-106); NULL = no force
 *   hist       : [B, n, 2, 3] output state history, hist[:,0] = x0
 * n >= 1.  The CoM trajectory of the reference is hist[:, :, :, 0].
 */
int zmpc_rollout(const zmpc_plan* plan, int64_t B, int64_t n, const double* zmax,
                 const double* zmin, int64_t bounds_stride, const double* x0,
                 const double* kick, int64_t kick_step, double* hist, int32_t* status,
                 void* stream);

/*
 * zmpc_rollout with a kick step per walk (ragged batches: the reference applies the force at
 * step n_b//2 of each walk, zmp_controller.py:90).  kick_steps: [B] int64 device array; a
 * step outside [0, n-1) means no kick for that walk.  Since ABI 2.
 */
int zmpc_rollout_kicks(const zmpc_plan* plan, int64_t B, int64_t n, const double* zmax,
                       const double* zmin, int64_t bounds_stride, const double* x0,
                       const double* kick, const int64_t* kick_steps, double* hist,
                       int32_t* status, void* stream);

/*
 * Per-walk robustness metrics of a state history, reduced on the device: the ZMP estimate
 * z = C·state = c − (h/g)·c̈ of run_mpc.py:294 held against the support box of its own sample,
 * as run_compare_resistance.py:173-197 plots the two (sample i with bounds row i) for the eye
 * to judge.  Replaces that plot-and-look step, and the chain of [B, n, 2] temporaries (or the
 * copy of hist to the host) that the same figures cost when built from array operations.
 *   hist       : [B, n, 2, 3]  state history of zmpc_rollout / zmpc_rollout_kicks /
 *                              zmpc_herdt_rollout, (c, ċ, c̈) per axis (a = 0: x, a = 1: y)
 *   zmax, zmin : [B, n, 2]     the walks' CoP bounds; bounds_stride as zmpc_rollout (2n or
 *                              more doubles between walks, 0 = one CoP for every walk)
 *   lengths    : [B] int64 or NULL  live samples n_b of ragged walks, 1 <= n_b <= n (a value
 *                              outside is clamped); rows at or past n_b are never read into a
 *                              result.  NULL: n_b = n
 *   metrics    : [B, ZMPC_NMETRICS]  per walk, slot 2k + a = quantity k of axis a.  With
 *                              zr = (zmax + zmin)/2 and v = max(z − zmax, zmin − z, 0) of
 *                              sample i against bounds row i, over 0 <= i < n_b:
 *     [0,1]   viol_max     max v
 *     [2,3]   viol_argmax  the smallest i that attains it, as a double; −1 when viol_max is 0
 *     [4,5]   viol_count   samples with v > 0
 *     [6,7]   com_dev_max  max |c − zr|
 *     [8,9]   zmp_rms      sqrt(mean (z − zr)²)
 *     [10,11] dcm_end      c + ċ·sqrt(h/g) − zr at i = n_b − 1: the divergent component of
 *                          motion at the last sample, relative to the final box centre
 * An axis with a non-finite state value in a live sample reports viol_max = +inf, viol_argmax =
 * the first such sample and NaN in its other slots (a threshold on viol_max fails safe); the
 * other axis and the other walks are unaffected.  The reductions run in a fixed order: two calls
 * on the same input agree bit for bit.  Any plan of the device serves, strict or not: only its
 * h/g is read.  No workspace, no status array.  Additive to ABI 7.
 */
#define ZMPC_NMETRICS 12
int zmpc_walk_metrics(const zmpc_plan* plan, int64_t B, int64_t n, const double* hist,
                      const double* zmax, const double* zmin, int64_t bounds_stride,
                      const int64_t* lengths, double* metrics, void* stream);

/*
 * Rollout and walk metrics in one launch: the reference's F_ext sweep plus the look at the plot
 * (run_compare_resistance.py:87-197 — :87-169 walks every force, :173-197 draws each ZMP against
 * its support boxes) as one call that keeps twelve doubles per walk and never materialises the
 * [B, n, 2, 3] state history.  `metrics` holds what zmpc_walk_metrics returns for the history
 * that zmpc_rollout (kick_steps NULL) / zmpc_rollout_kicks would write for the same arguments:
 * the same slots, the same sample-i-against-bounds-row-i rule, the same clamp of `lengths`, the
 * same non-finite rule, the same uncontracted z, box centre and v.  Value slots agree with that
 * pair of launches to rounding (1e-11 on O(1) states; the kernels' instruction streams differ),
 * so a count or an index may differ where a sample sits within rounding of its bound.
 *   zmax, zmin, bounds_stride, x0, kick, kick_step : as zmpc_rollout
 *   kick_steps : [B] int64 or NULL  per-walk kick steps as zmpc_rollout_kicks; NULL: kick_step
 *   lengths    : [B] int64 or NULL  live samples per walk, as zmpc_walk_metrics.  Every walk is
 *                                   still rolled out over all n samples (status covers them)
 *   metrics    : [B, ZMPC_NMETRICS] as zmpc_walk_metrics
 *   status     : [B] or NULL        what the rollout writes
 * The reductions run in an order fixed by the lane numbers: two calls on the same input agree bit
 * for bit.  Takes the walks the split kernels roll out: a non-strict plan, n − 1 <= 512 steps (one
 * correlation pass) within 64 KiB of LDS, ZMPC_OPT_ROLLOUT_KERNEL = 0; ZMPC_OPT_CORRELATION is
 * honoured.  Strict plans and every other shape return ZMPC_ESTATE with the reason and launch
 * nothing: use zmpc_rollout + zmpc_walk_metrics there.  Additive to ABI 7.
 */
int zmpc_rollout_metrics(const zmpc_plan* plan, int64_t B, int64_t n, const double* zmax,
                         const double* zmin, int64_t bounds_stride, const double* x0,
                         const double* kick, int64_t kick_step, const int64_t* kick_steps,
                         const int64_t* lengths, double* metrics, int32_t* status, void* stream);

/*
 * Push-robustness map: the exact largest push every (walk, push step, direction) survives, from
 * the unpushed state history in one call.  The reference can only sample a few forces at one step
 * and look (run_compare_resistance.py:87-197); ZMPController.critical_force brackets one step per
 * scenario with 32 pushed rollouts.  For the unconstrained controller neither is needed: the
 * closed loop x⁺ = Ā x + B f, Ā = A − B·kxᵀ, is linear and time-invariant, so the y-axis ZMP
 * response at sample i to a unit push at step s depends on the delay d = i − s alone,
 *     r_0 = 0,  r_d = −(dt/mass)·C·Ā^(d−1)·e1  (d >= 1),  C = (1, 0, −h/g)
 * (a push of +F at history step s lowers the y velocity of sample s + 1 by dt·F/mass,
 * zmp_controller.py:105-106; r_1 is exactly 0: a velocity kick moves neither c nor c̈ of the
 * next sample).
 *   hist, zmax, zmin, bounds_stride, lengths : as zmpc_walk_metrics (n_b clamped the same way)
 *   push_steps    : NULL: the full map, force and limit are [B, n, 2];
 *                   [B] int64: the single-step form, force and limit are [B, 2], the entries of
 *                   step push_steps[b] of walk b (a step outside [0, n_b − 2) gives +inf and −1)
 *   max_violation : t >= 0, the excursion beyond the support box that still passes
 *   mass          : the robot's mass m in kg (the plan holds dt, h/g and the gains, not m)
 *   force         : per walk b, with z0_i = c_i − (h/g)·c̈_i the y-axis ZMP of the history
 *                   (uncontracted, as zmpc_walk_metrics), up_i = (zmax_i − z0_i) + t and
 *                   dn_i = (z0_i − zmin_i) + t:
 *       force[b, s, 0] (a +y push) = min over s < i < n_b of
 *                      (r_d > 0 ? up_i / r_d : r_d < 0 ? dn_i / (−r_d) : +inf),  d = i − s
 *       force[b, s, 1] (a −y push) = the same with up and dn swapped
 *                   Entries with s >= n_b − 2, and entries that no sample constrains, are +inf.
 *                   A walk that fails with no push — v_i = max(z − zmax, zmin − z, 0) > t on
 *                   either axis at some i < n_b, zmpc_walk_metrics' test — or that holds a
 *                   non-finite state value in a live sample of either axis is NaN in every entry.
 *                   The map is not capped.  If the history already carries a push, the entries
 *                   are the largest additional push.
 *   limit         : int32, shaped as force, or NULL: the smallest i that attains the minimum
 *                   (the sample that leaves its box first); −1 for +inf and NaN entries
 *   response      : [n] or NULL: receives r_0 .. r_(n−1)
 * No candidate is formed from r_d = 0 and no product 0·inf: a sample exactly on its bound with
 * t = 0 gives 0.  The candidates are margin × (1/|r_d|), a few ulp from the quotient.  The
 * minima run in an order fixed by the lane numbers: two calls on the same input agree bit for
 * bit, and the single-step form returns the full map's rows bit for bit.  The response table is
 * recomputed per call into a stream-ordered workspace of 2n doubles.
 * The plan must be non-strict (it supplies kx, A, B, h/g and dt): a strict plan returns
 * ZMPC_ESTATE — the response of a clamped controller is not affine, bisect over pushed rollouts
 * there (ZMPController.critical_force).  The full map keeps a walk's margins in LDS: n > 10112
 * returns ZMPC_ESTATE with the limit in the message; the single-step form takes any n.  Nothing
 * is launched on a refusal.  ZMPC_EINVAL before any device call: NULL plan or (B > 0) NULL hist,
 * zmax, zmin or force; B < 0; n < 1; max_violation < 0 or NaN; mass not finite and positive; a
 * bad bounds_stride.  B = 0 does nothing.  Additive to ABI 7.
 */
int zmpc_push_map(const zmpc_plan* plan, int64_t B, int64_t n, const double* hist,
                  const double* zmax, const double* zmin, int64_t bounds_stride,
                  const int64_t* lengths, const int64_t* push_steps, double max_violation,
                  double mass, double* force, int32_t* limit, double* response, void* stream);

/*
 * Push-robustness map of sustained and shaped pushes, on either axis or both.  Everything is as
 * in zmpc_push_map unless said here: the nominal test, the clamping of n_b, max_violation, NaN
 * for a walk that fails unpushed, no cap, ties to the lower sample.  The same linear,
 * time-invariant argument, with no new approximation:
 *   - a push with force profile F·w_j during history steps s + j, j < duration = D, is a sum of
 *     one-sample pushes, so it moves the ZMP of sample s + d by F·R_d with
 *         R_d = Σ_{j = 0}^{min(D−1, d)} w_j·r_(d−j),  0 <= d < n,
 *     summed in ascending j, uncontracted (r_d as zmpc_push_map; R_0 = R_1 = 0 always);
 *   - the x axis runs the same closed loop with the same r: a push of +F on axis a lowers that
 *     axis' velocity of sample s + j + 1 by dt·F·w_j/mass (the reference's convention for y,
 *     mirrored for x);
 *   - the axes decouple, so the critical magnitude along any planar direction follows from the
 *     four columns +x, −x, +y, −y (analysis.PushMap.rose).
 *   profile  : [duration] device doubles w_0 .. w_(D−1), or NULL: all ones, and the product is
 *              skipped, so D = 1 gives R_d = r_d bit for bit.  Weights at j >= n are never read.
 *              A push that runs past n_b − 1 is truncated by itself.  A non-finite weight gives
 *              unspecified values in the entries it reaches; it never causes an out-of-range
 *              access and no 0·inf is formed (terms with r = 0 are skipped).
 *   duration : D >= 1, in samples
 *   axes     : ZMPC_PUSH_AXIS_X: columns (+x, −x); ZMPC_PUSH_AXIS_Y: (+y, −y); both: (+x, −x,
 *              +y, −y).  C = 2 or 4 columns.
 *   force    : [B, n, C], or [B, C] with push_steps (the step rule of zmpc_push_map).  Per axis a,
 *              with z0 that axis' uncontracted ZMP, up_i = (zmax_i − z0_i) + t and
 *              dn_i = (z0_i − zmin_i) + t:
 *       force[b, s, (+a)] = min over s < i < n_b of
 *                      (R_d > 0 ? up_i / R_d : R_d < 0 ? dn_i / (−R_d) : +inf),  d = i − s
 *       force[b, s, (−a)] = the same with up and dn swapped
 *   limit    : int32, shaped as force, or NULL: the smallest i that attains the minimum
 *   response : [n] or NULL: receives R_0 .. R_(n−1)
 * With axes = ZMPC_PUSH_AXIS_Y, D = 1 and a NULL profile, force, limit and response are
 * zmpc_push_map's bit for bit; a two-axis call equals the two one-axis calls column for column;
 * the single-step form returns the full map's rows bit for bit; two calls on the same input
 * agree bit for bit.  With D = 1 and a NULL profile the call is zmpc_push_map's on the axes
 * asked for: no shaping launch, a stream-ordered workspace of 2n doubles.  Otherwise the shaped
 * table is computed per call by a grid over the delays (n·min(D, n)/2 products) into a
 * stream-ordered workspace of 5n doubles (a profile of one weight w_0 included: w_0
 * multiplies).  In the full map the axes take
 * turns over the same LDS: n > 10112 returns ZMPC_ESTATE for one axis or two, with the limit in
 * the message; the single-step form takes any n.  A strict plan returns ZMPC_ESTATE.  Nothing
 * is launched on a refusal.  ZMPC_EINVAL before any device call: zmpc_push_map's cases,
 * duration < 1, axes outside 1..3.  B = 0 does nothing.  Additive to ABI 7.
 */
#define ZMPC_PUSH_AXIS_X 1
#define ZMPC_PUSH_AXIS_Y 2
int zmpc_push_map_shaped(const zmpc_plan* plan, int64_t B, int64_t n, const double* hist,
                         const double* zmax, const double* zmin, int64_t bounds_stride,
                         const int64_t* lengths, const int64_t* push_steps,
                         const double* profile /* [duration] device, or NULL */,
                         int64_t duration, int32_t axes, double max_violation, double mass,
                         double* force, int32_t* limit, double* response /* [n] R_d or NULL */,
                         void* stream);

/*
 * Rollouts under shoves: pushes of any length, shape and direction, on every controller.  The
 * reference can only disturb a walk the way zmp_controller.py:105-106 does it — one sample, the
 * y axis, one velocity impulse (kick, kick_step) — and the push maps above answer sustained pushes
 * for the unconstrained controller alone.
 *
 * The push, stated once.  Per walk b the inputs are a start step s_b, a duration D >= 1 shared by
 * the batch, an optional profile w_0 .. w_(D−1), shared, on the device (NULL: all ones), and one
 * amplitude per requested axis, amp[b, a] = dt·F_b·dir_(b,a)/m, in m/s.  For every history step i
 * with j = i − s_b, 0 <= j < D and i < n − 1, the state of sample i + 1 on axis a has its
 * velocity lowered by amp[b, a]·w_j.
 *   - This is applied after x⁺ = A x + B u0, where the reference applies its kick.
 *   - NULL profile: the velocity is lowered by amp[b, a] itself with no product, so D = 1
 *     reproduces the kick's arithmetic.
 *   - A start step outside [0, n − 1) means no push for that walk.
 *   - A push that runs past the walk's end is truncated.
 *   - An axis that was not requested is untouched, bit for bit.
 *   - Sign: +F on an axis lowers that axis' velocity — the reference's y convention, mirrored for
 *     x, as in zmpc_push_map_shaped.
 *   - A non-finite weight gives unspecified values in the samples it reaches and never an
 *     out-of-range access.
 */
typedef struct zmpc_push {
  const double*  amp;       /* [B, C] device; C = 1 or 2 columns in the order of `axes` (x, y) */
  int32_t        axes;      /* ZMPC_PUSH_AXIS_X | ZMPC_PUSH_AXIS_Y */
  const int64_t* steps;     /* [B] device start steps, or NULL: `step` for every walk */
  int64_t        step;
  const double*  profile;   /* [duration] device, or NULL: ones */
  int64_t        duration;  /* >= 1 */
} zmpc_push;

/*
 * zmpc_rollout / zmpc_rollout_kicks under a push window; every other argument as there.
 *   - The legacy push (axes = ZMPC_PUSH_AXIS_Y, duration 1, NULL profile) is zmpc_rollout_kicks
 *     itself (zmpc_rollout with NULL steps) on every plan kind: hist and status bit for bit.
 *   - Strict plans: the LQ and the parallel-in-time kernels (ZMPC_OPT_STRICT_SOLVER 0, 3, 4) take
 *     the window in their time loop; ZMPC_OPT_KICK_ORDER sorts the walks by (start step, the
 *     larger |amp| of the requested axes), and the results do not depend on the order.  The
 *     reduced-Cholesky cross-checks (solvers 1 and 2) return ZMPC_ESTATE with the reason for
 *     anything but the legacy push.
 *   - Unconstrained plans: the closed loop is linear and time-invariant, so the call runs the
 *     unpushed zmpc_rollout — any shape, any n — and then adds the state response
 *         hist[b, s_b + d, a, :] −= amp[b, a]·Σ_{j <= min(D−1, d−1)} w_j·Ā^(d−j−1)·e1,  d >= 1
 *     (the sum in ascending j, uncontracted; Ā = A − B·kxᵀ as zmpc_push_map) from a table computed
 *     per call into a stream-ordered workspace of 4n doubles (8n with a profile or D > 1).  It
 *     agrees with D + 1 chained restarts of zmpc_rollout to rounding; status is the unpushed
 *     rollout's.
 * ZMPC_EINVAL before any device call: NULL push, or NULL amp when B > 0; axes outside 1..3;
 * duration < 1; zmpc_rollout's own cases.  B = 0 does nothing.  Nothing is launched on a refusal.
 * Two calls on the same input agree bit for bit.  Additive to ABI 7.
 */
int zmpc_rollout_pushed(const zmpc_plan* plan, int64_t B, int64_t n, const double* zmax,
                        const double* zmin, int64_t bounds_stride, const double* x0,
                        const zmpc_push* push, double* hist, int32_t* status, void* stream);

/*
 * Batched CoP-bound producer: CoPGenerator.generate_cop_trajectory
 * (generators/cop_generator.py:34-115) over the footstep plan of
 * generators/footstep_generator.py:19-49, one walk per set of parameters.
 *   params : [B, 7] device doubles = distance, step_length, foot_spread, ssp_duration,
 *            dsp_duration, standing_duration, dt (the reference's float clock t += dt is
 *            reproduced exactly, so the sample counts match)
 *   n_cap = 0: count only — n_out[b] = samples of walk b (int64 device array)
 *   n_cap > 0: zmax, zmin [B, n_cap, 2] (rows past n_b repeat the walk's last row, the
 *            rollout's own window padding), states [B, n_cap] int8 (0 STANDING,
 *            1 DOUBLE_SUPPORT, 2 SINGLE_SUPPORT, -1 padding) or NULL, n_out or NULL.
 * Since ABI 2.
 */
int zmpc_cop_generate(int device, int64_t B, const double* params, int64_t n_cap,
                      double* zmax, double* zmin, int8_t* states, int64_t* n_out,
                      void* stream);

/*
 * Herdt joint footstep QP (config.method == "herdt"), since ABI 4.
 * The plan supplies N (horizon) and the LIPM constants (dt, h, g); its strict flag is unused.
 * Support states are int8: 0 STANDING, 1 DOUBLE_SUPPORT, 2 SINGLE_SUPPORT (cop_generator.py:11-15).
 */
#define ZMPC_HERDT_MAX_FACETS 16
typedef struct zmpc_herdt_params {
  double alpha, beta, gamma;         /* cost weights (config.py:42-45) */
  double foot_length, foot_width;    /* ZMP box around the foot centre: ±½·dim (:666, :680) */
  double foot_spread;                /* initial y foot position, standing hull (:457, :726-731) */
  int32_t nfacets[2];                /* facets of the left / right swing polytope */
  double facets[2][ZMPC_HERDT_MAX_FACETS][3]; /* (a_x, a_y, b): a·(f − f_current) <= b, the
                                        reference's _polytope_halfspace (:828-865) */
  int32_t max_footsteps;             /* most footsteps (support segments after the current
                                        one) inside any horizon window of the batch, <= 8 */
  int32_t max_passes;                /* active-set pass cap per joint QP (0: the default 64).
                                        A solve that reaches it keeps its last iterate (as OSQP
                                        returns its iterate at its own iteration limit) and sets
                                        ZMPC_ST_MAXITER.  A solve whose swing polytope is
                                        infeasible — the analogue of OSQP returning no solution
                                        — takes the reference's failure fallback
                                        (zmp_controller.py:796-802: zero jerk on both axes, the
                                        first footstep at the air foot's centre; the current
                                        foot for zmpc_herdt_step) and sets ZMPC_ST_INFEASIBLE */
} zmpc_herdt_params;

/*
 * Batched ZMPController.generate_com_trajectory_herdt (zmp_controller.py:435-531) over
 * predict_herdt_joint (:533-826) for B walks of n samples (exact QP solution; the reference's
 * cvxpy/OSQP result differs by up to OSQP's tolerances).
 *   v_ref [B, n, 2] reference velocities (v_stride doubles between walks, 0 = shared)
 *   states [B, n] int8 (s_stride bytes between walks, 0 = shared)
 *   nb_next [B, n] int32: find_nb_steps(padded states)[i][0] (:470), the divisor of the
 *            air-foot interpolation (:497-500) (nb_stride elements between walks, 0 = shared)
 *   x0 [B, 2, 3] initial (x, y) states; kick [B] or NULL: y-velocity impulse dt·F_ext/m
 *            subtracted at step kick_step (:525-526)
 *   hist [B, n, 2, 3] state history; foot [B, n, 2] foot positions (foot_hist, :529-530)
 */
int zmpc_herdt_rollout(const zmpc_plan* plan, const zmpc_herdt_params* params, int64_t B,
                       int64_t n, const double* v_ref, int64_t v_stride, const int8_t* states,
                       int64_t s_stride, const int32_t* nb_next, int64_t nb_stride,
                       const double* x0, const double* kick, int64_t kick_step, double* hist,
                       double* foot, int32_t* status, void* stream);

/*
 * zmpc_herdt_rollout under a push window (zmpc_push and "The push, stated once" above): the
 * footstep-adapting controller under a shove of any length, shape and direction, with a start
 * step per walk.  The window is applied in the (walk, axis) lane where the reference applies its
 * impulse (:525-526).  The legacy push (axes = ZMPC_PUSH_AXIS_Y, duration 1, NULL profile, NULL
 * steps) is zmpc_herdt_rollout's kick: hist, foot and status bit for bit.  ZMPC_EINVAL before any
 * device call: NULL push, or NULL amp when B > 0; axes outside 1..3; duration < 1;
 * zmpc_herdt_rollout's own cases.  B = 0 does nothing.  Additive to ABI 7.
 */
int zmpc_herdt_rollout_pushed(const zmpc_plan* plan, const zmpc_herdt_params* params, int64_t B,
                              int64_t n, const double* v_ref, int64_t v_stride,
                              const int8_t* states, int64_t s_stride, const int32_t* nb_next,
                              int64_t nb_stride, const double* x0, const zmpc_push* push,
                              double* hist, double* foot, int32_t* status, void* stream);

/*
 * Rollouts under per-walk force traces, on every controller.  A push window gives a batch one
 * length and one profile; a trace gives every walk its own disturbance per sample and axis: a walk
 * shoved twice, walks shoved for different lengths or with different shapes, force noise per walk,
 * a force trace recorded elsewhere.
 *
 * The trace, stated once.  It is "The push, stated once" above with the product amp[b, a]·w_j
 * replaced by a value read from the walk's own row; everything not said here is as there (where it
 * acts, the sign, truncation).  Per walk b the inputs are a start step s_b, a length L >= 1 shared
 * by the batch, and dv[b, j, col(a)] in m/s (= dt·F/m) for 0 <= j < L and every requested axis a.
 * For every history step i with j = i − s_b, 0 <= j < L and i < n − 1, after x⁺ = A x + B u0 the
 * velocity of sample i + 1 on axis a is lowered by dv[b, j, col(a)].
 *   - The read value is used as it is, with no product: a trace whose rows hold one constant is a
 *     NULL-profile window of duration L, bit for bit.
 *   - A start step outside [0, n − 1) means no disturbance for that walk.
 *   - A trace that runs past the walk's end is truncated; entries that reach no sample are never
 *     read.
 *   - An axis that was not requested is untouched, bit for bit.
 *   - A non-finite entry gives unspecified values in the samples it reaches and never causes an
 *     out-of-range access.
 *   - Two calls on the same input agree bit for bit, and a walk's result does not depend on which
 *     batch it sits in.
 *
 * The stream is a member of the descriptor, not a parameter of the calls: the two calls below
 * take no `void* stream`, so the rule that every entry point declared with one has a case in the
 * stream-contract table (tests/stream_cases.py) does not reach them; tests/test_gpu_trace.py holds
 * them to the same contract (work queued on trace.stream alone, ordered after what that stream
 * already holds, NULL = the null stream).
 */
typedef struct zmpc_trace {
  const double*  dv;      /* [B, length, C] device: what the velocity of sample s_b + j + 1 is
                             lowered by on axis a, in m/s (= dt·F/m); C = 1 or 2 columns in the
                             order of `axes` (x, y) */
  int32_t        axes;    /* ZMPC_PUSH_AXIS_X | ZMPC_PUSH_AXIS_Y */
  const int64_t* steps;   /* [B] device start steps s_b, or NULL: `step` for every walk */
  int64_t        step;
  int64_t        length;  /* L >= 1 samples per walk */
  void*          stream;  /* hipStream_t, NULL = the null stream */
} zmpc_trace;

/*
 * zmpc_rollout under a trace; every other argument as there.
 *   - Strict plans: the LQ and the parallel-in-time kernels (ZMPC_OPT_STRICT_SOLVER 0, 3, 4) read
 *     the trace in their time loop, in the instances that take a push window;
 *     ZMPC_OPT_KICK_ORDER sorts the walks by (start step, the larger |dv[b, 0, ·]| of the
 *     requested axes), and the results do not depend on the order.  The reduced-Cholesky
 *     cross-checks (solvers 1 and 2) return ZMPC_ESTATE with the reason.
 *   - Unconstrained plans: the closed loop is linear and time-invariant, so the call runs the
 *     unpushed zmpc_rollout — any shape, any n — and then subtracts the state response of the
 *     walk's own trace,
 *         δ_(s_b) = 0,  δ_(i+1) = Ā·δ_i + e1·dv[b, i − s_b, a],  hist[b, i, a, :] −= δ_i,  s_b < i < n
 *     (Ā = A − B·kxᵀ as zmpc_push_map), one wavefront per walk, as a scan over blocks of 64
 *     samples: O(n) per walk, dv read once, no workspace.  Samples at or before s_b are neither
 *     read nor written; an all-zero trace leaves hist the unpushed rollout's bit for bit.  The
 *     sums run in an order fixed by lane and block numbers, uncontracted.  It agrees with chained
 *     restarts of zmpc_rollout to rounding; status is the unpushed rollout's.
 * ZMPC_EINVAL before any device call: NULL trace, or NULL dv when B > 0; axes outside 1..3;
 * length < 1, or so large that B·length·16 bytes pass int64; zmpc_rollout's own cases.  B = 0 does
 * nothing.  Nothing is launched on a refusal.  Additive to ABI 7.
 */
int zmpc_rollout_traced(const zmpc_plan* plan, int64_t B, int64_t n, const double* zmax,
                        const double* zmin, int64_t bounds_stride, const double* x0,
                        const zmpc_trace* trace, double* hist, int32_t* status);

/*
 * zmpc_herdt_rollout under a trace ("The trace, stated once" above), read in the (walk, axis) lane
 * where the reference applies its impulse (:525-526).  ZMPC_EINVAL before any device call: NULL
 * trace, or NULL dv when B > 0; axes outside 1..3; length < 1 or too large (as
 * zmpc_rollout_traced); zmpc_herdt_rollout's own cases.
 * B = 0 does nothing.  Additive to ABI 7.
 */
int zmpc_herdt_rollout_traced(const zmpc_plan* plan, const zmpc_herdt_params* params, int64_t B,
                              int64_t n, const double* v_ref, int64_t v_stride,
                              const int8_t* states, int64_t s_stride, const int32_t* nb_next,
                              int64_t nb_stride, const double* x0, const zmpc_trace* trace,
                              double* hist, double* foot, int32_t* status);

/*
 * Trace margin: the exact critical scale of a trace, K draws per walk, from one unpushed history of
 * an unconstrained plan.  The closed loop is linear and time-invariant, so under λ times a trace
 * the ZMP of sample i is z0_i + λ·ρ_i, and the largest λ a walk survives is a minimum of quotients
 * over its samples: the argument of zmpc_push_map with a response per row instead of one per batch.
 * No rollout is run per evaluation and no history is written: K random draws of a disturbance per
 * nominal walk cost one unpushed zmpc_rollout of the B walks and this one launch over B·K rows.
 *
 *   hist [B, n, 2, 3] : an unpushed history; read, never written
 *   zmax, zmin, bounds_stride, lengths : as zmpc_walk_metrics and zmpc_push_map (n_b clamped to
 *                       [1, n] the same way)
 *   draws = K >= 1    : the trace describes R = B·K rows, row r belongs to walk b = r / K;
 *                       trace->dv is [R, L, C], trace->steps [R] or NULL.  "The trace, stated once"
 *                       holds per row: where the value acts, the sign, truncation at the walk's end
 *                       (n_b), and entries that reach no sample are never read
 *   scale [R, 2], limit [R, 2] int32 or NULL
 *
 * The trace margin, stated once.  Per row r with start step s and requested axis a,
 *     δ_s = 0,   δ_(i+1) = Ā·δ_i + e1·dv[r, i − s, col(a)]        (Ā = A − B·kxᵀ as zmpc_push_map)
 *     ρ_i^a = −(δ_i^a[0] − (h/g)·δ_i^a[2])                         (uncontracted)
 * z0 is the uncontracted ZMP of hist as in zmpc_walk_metrics, t = max_violation,
 * up_i = (zmax_i − z0_i) + t and dn_i = (z0_i − zmin_i) + t.  Then
 *     scale[r, 0] = min over s < i < n_b and the requested axes of
 *                   up_i/ρ_i where ρ_i > 0,  dn_i/(−ρ_i) where ρ_i < 0,  +inf otherwise
 * and scale[r, 1] is the same with up and dn swapped: the largest multiple of the negated trace.
 * The quotient is an IEEE division; no candidate is formed from ρ = 0 and no 0·inf is formed, so a
 * sample exactly on its bound with t = 0 gives 0.  limit[r, k] = 2·i + a of the smallest (i, a)
 * that attains the minimum (a = 0 for x, 1 for y; i before a), −1 for +inf and NaN entries.
 *   - A walk that fails the nominal test on either axis (zmpc_walk_metrics' test over all i < n_b,
 *     the samples at or before s included; a non-finite state value in a live sample) gives NaN and
 *     −1 in every row of that walk.
 *   - A start step outside [0, n_b − 1), or an all-zero trace, gives +inf and −1 (unless the walk is
 *     NaN by the rule above).
 *   - A non-finite entry of dv gives unspecified values in its own row only and never causes an
 *     out-of-range access.
 *   - Two calls on the same input agree bit for bit; a row's result does not depend on the batch it
 *     sits in; a call with K draws equals the K one-draw calls on the same walk bit for bit.
 * One wavefront per row, the scan of zmpc_rollout_traced in its order of sums, the six propagators
 * per launch from the plan's kx and step constants: O(n) per row, no workspace, no table, and no
 * limit on n from LDS (n <= 2^30: limit holds 2·i + a).  It agrees with the extended-precision
 * statement to 1e-11 relative, the bar of forms that compute the same solution.
 *
 * The call takes no `void* stream`: as for the two traced rollouts above the stream travels in
 * trace->stream, so the stream-contract table (tests/stream_cases.py) does not reach it;
 * tests/test_gpu_trace_margin.py holds it to the same contract.
 * ZMPC_ESTATE before any device call: a strict plan (a clamped response is not affine in the
 * scale; bisect with ZMPController.critical_force).  ZMPC_EINVAL before any device call: NULL plan
 * or trace; with B > 0, NULL dv, hist, zmax, zmin or scale; B < 0 or n < 1; draws < 1; B·draws
 * beyond the batch limit (2^31 − 1); axes outside 1..3; length < 1 or too large (as
 * zmpc_rollout_traced, over B·draws rows); max_violation negative or NaN; a bad bounds_stride.
 * B = 0 does nothing.  Nothing is launched on a refusal.  Additive to ABI 7.
 */
int zmpc_trace_margin(const zmpc_plan* plan, int64_t B, int64_t n, const double* hist,
                      const double* zmax, const double* zmin, int64_t bounds_stride,
                      const int64_t* lengths, int64_t draws, const zmpc_trace* trace,
                      double max_violation, double* scale, int32_t* limit);

/*
 * Per-walk survival metrics of a Herdt rollout, reduced on the device: did the footstep-adapting
 * controller stay up?  zmpc_walk_metrics needs fixed CoP bounds; a Herdt walk has none, its
 * support box follows the footsteps the QP chose.  Here the box is rebuilt from the rollout's own
 * outputs.
 *   hist [B, n, 2, 3], foot [B, n, 2] : what zmpc_herdt_rollout(_pushed) wrote
 *   states [B, n] int8                : what it took (s_stride bytes between walks, 0 = shared)
 *   foot_ref [B, n, 2] or NULL        : the feet of a nominal walk, normally the unpushed one
 *                                       (foot_ref_stride doubles between walks, 0 = shared)
 *   lengths [B] int64 or NULL         : live samples n_b per walk, clamped to [1, n] as in
 *                                       zmpc_walk_metrics; rows from n_b on are never read
 *   count_tol >= 0                    : the excursion above which a sample counts in viol_count
 *   metrics [B, ZMPC_NHERDT_METRICS]
 * The plan supplies h/g only (any plan kind); params supplies foot_length, foot_width,
 * foot_spread, the facets and nfacets, and nothing else of it is read.
 *
 * The support of sample i, stated once.  Let j = max(i − 1, 0), f = foot[b, j], s = states[b, i].
 *   - Row 0 of the QP built at step i − 1 belongs to the current foot of that step, so the
 *     realised ZMP of sample i is held to a box round foot[i − 1], not foot[i]: at a landing
 *     foot[i] has already jumped a step length.
 *   - L_k: states[k] == SINGLE_SUPPORT, states[k+1] != SINGLE_SUPPORT and k + 1 < n_b — a landing
 *     at step k; the rollout flips its side there and writes the new foot to row k + 1.
 *   - side_j: the parity of the number of landings at steps k < j; 0 is left (the rollout's own
 *     rule, :501-502).
 *   - Sample 0 has no box: v_0 = 0.
 *   - i >= 1, s != STANDING: the box is f ± ½(foot_length, foot_width) (:666, :680).
 *   - i >= 1, s == STANDING: x as above; y is held to the hull of both feet, the other foot at
 *     f_y − 2·foot_spread when side_j is left and f_y + 2·foot_spread when it is right, widened by
 *     ½·foot_width on both sides (:716-734).  The reference drops a STANDING row from its QP while
 *     walking rows remain in the window (:682-698); the metric still holds that sample to the
 *     hull, since both feet are on the ground.
 *   - v_i = max(z − hi, lo − z, 0) with z = c − (h/g)·c̈, uncontracted as in zmpc_walk_metrics.
 * The QP is always feasible (its ZMP matrix is triangular with a non-zero diagonal and the jerk
 * is unbounded): under any push the ZMP stays on or inside its box — it sits on the edge by
 * design, so v is rounding noise and viol_count needs count_tol — while the CoM runs away.
 * Whether the robot stayed up is told by dcm_dev_max, never by viol_max.
 *
 * Slot 2k + a holds quantity k of axis a (0: x, 1: y), over 0 <= i < n_b, with fs_i = foot[j]:
 *   0 viol_max        max v_i
 *   1 viol_argmax     the smallest i that attains it, −1 when viol_max is 0
 *   2 viol_count      the number of samples with v_i > count_tol
 *   3 com_dev_max     max |c_i − fs_i|
 *   4 dcm_dev_max     max |c_i + ċ_i·sqrt(h/g) − fs_i|: the survival quantity
 *   5 dcm_end         c + ċ·sqrt(h/g) − fs at i = n_b − 1, signed
 *   6 step_shift_max  max |foot_i − foot_ref_i|: how far the controller stepped aside; 0 when
 *                     foot_ref is NULL
 * Slot 14, reach_slack_min: over the landings k, the minimum over the facets (a_x, a_y, b) of
 * side_k's polytope of b − a·(foot[k+1] − foot[k]) (the sum a_x·d_x + a_y·d_y, uncontracted);
 * +inf with no landing or no facets; zero: the step reached as far as it could.
 * Slot 15, steps_landed: the number of landings.
 * Non-finite rule, as zmpc_walk_metrics: a live sample i of axis a is non-finite when hist[b, i,
 * a, :], foot[b, i, a] or (given) foot_ref[b, i, a] is not finite; such an axis reports viol_max
 * = +inf, viol_argmax = the first such sample and NaN in its other slots, slot 14 is NaN if
 * either axis is flagged, slot 15 and the other walks are unaffected.
 * The reductions run in an order fixed by the lane numbers: two calls on the same input agree bit
 * for bit.  No workspace, no status.  ZMPC_EINVAL before any device call: NULL plan or params;
 * (B > 0) NULL hist, foot, states or metrics; B < 0; n < 1; count_tol negative or NaN; nfacets
 * outside [0, 16]; a non-zero s_stride < n or foot_ref_stride < 2n.  B = 0 does nothing.
 * Additive to ABI 7.
 */
#define ZMPC_NHERDT_METRICS 16
int zmpc_herdt_walk_metrics(const zmpc_plan* plan, const zmpc_herdt_params* params, int64_t B,
                            int64_t n, const double* hist, const double* foot,
                            const int8_t* states, int64_t s_stride, const double* foot_ref,
                            int64_t foot_ref_stride, const int64_t* lengths, double count_tol,
                            double* metrics, void* stream);

/*
 * Footstep bookkeeping of a batch of Herdt walks with different gaits, on the device: the two
 * inputs of zmpc_herdt_rollout(_pushed) that follow from the support states alone — nb_next
 * (zmp_controller.py:203-433, :466-470) and the footstep count that sizes the kernel instance
 * (zmpc_herdt_params.max_footsteps; the phase breaks of :561-573) — which the host otherwise
 * makes one walk at a time.
 *
 * This call takes no stream and is synchronous, like zmpc_plan_counters, zmpc_plan_export and
 * zmpc_plan_destroy: *max_footsteps_host has to reach the host before the rollout it prepares can
 * be sized.  It synchronises the plan's device on entry, so whatever stream produced `states`
 * has finished, and it returns when every output is complete.  The plan supplies N and the device;
 * any plan kind serves.
 *
 * The walk, stated once, in terms of walk b's own sequence, not the batch's:
 *   - n_b = clamp(lengths[b], 1, n), or n with NULL lengths.
 *   - c[i] = states[b, min(i, n_b − 1)] for 0 <= i < L, L = n_b + N: the live walk followed by N
 *     copies of its last live state, what the reference builds for that walk alone (:466-469).
 *     Rows at or past n_b of the input are never read (zmpc_cop_generate's −1 padding lives there),
 *     so a walk padded to the batch's n gives what the walk alone gives.
 *   states     : [B, n] int8 device (s_stride bytes between walks; 0 = one schedule shared by
 *                every walk, only `lengths` can then make the rows differ)
 *   lengths    : [B] int64 device, or NULL
 *   states_out : [B, n] int8 device, or NULL: states_out[b, i] = c[i] for i < n — the states a
 *                rollout of the padded batch reads in walk b's place.  Must not overlap `states`.
 *   nb_next    : [B, n] int32 device.  For i < n_b the first element of find_nb_steps on c[0..L):
 *                with nds the smallest j > i, j < L, with c[j] == DOUBLE_SUPPORT and nss(j) the
 *                same for SINGLE_SUPPORT,
 *                  c[i] == STANDING: L − i with no nds; else with q = nss(nds), L − i with no q,
 *                                    else q − i − 1
 *                  any other code:   nds − i if nds exists, else L − i
 *                (the "next" index may lie in the tail: a walk may end in double or single
 *                support).  nb_next[b, i] = 1 for n_b <= i < n: those rows' windows are constant,
 *                hold no footstep, and the rollout never divides by the value.
 *   max_steps  : [B] int32 device, or NULL: the maximum over 0 <= i < max(n_b − 1, 1) of the
 *                number of t in [i, i + N) with c[t] != c[t+1] and not (c[t] DOUBLE_SUPPORT and
 *                c[t+1] SINGLE_SUPPORT) — the most footsteps in one horizon window of that walk
 *   max_footsteps_host : one int32 in HOST memory, or NULL: the maximum of max_steps over the
 *                batch, 0 for B = 0.  A value above 8 is reported, not refused: the rollout's
 *                parameter check refuses it.
 * Results are integers; two calls on the same input agree.  Workspace: one device word.
 * ZMPC_EINVAL, decided from the arguments before any device call and before the plan is read:
 * NULL plan; B < 0; n < 1; n beyond zmpc_rollout's limit ("walk too long"); (B > 0) NULL states
 * or nb_next; a non-zero s_stride < n.  B = 0 writes the host word and nothing else.  Additive to
 * ABI 7.
 */
int zmpc_herdt_prepare(const zmpc_plan* plan, int64_t B, int64_t n, const int8_t* states,
                       int64_t s_stride, const int64_t* lengths, int8_t* states_out,
                       int32_t* nb_next, int32_t* max_steps, int32_t* max_footsteps_host);

/*
 * Batched predict_herdt_joint (zmp_controller.py:533-826), one QP per instance, cold start:
 *   x [B, 2, 3] (x, y) states; v_win [B, N, 2] window of v_ref; s_win [B, N] window states;
 *   current [B] int8 current support state; foot [B, 2] current foot (x_fc, y_fc);
 *   side [B] int8 (0 left, 1 right)
 *   → x_next [B, 2, 3]; step [B, 2] first planned footstep (NaN when the window holds none,
 *     the reference's None).
 */
int zmpc_herdt_step(const zmpc_plan* plan, const zmpc_herdt_params* params, int64_t B,
                    const double* x, const double* v_win, const int8_t* s_win,
                    const int8_t* current, const double* foot, const int8_t* side,
                    double* x_next, double* step, int32_t* status, void* stream);

/* Message describing the last failure on the calling thread ("" if none). */
const char* zmpc_last_error(void);

/* ZMPC_ABI_VERSION of the loaded library. */
int zmpc_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* ZMPC_H */
