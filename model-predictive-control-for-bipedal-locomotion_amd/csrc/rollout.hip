// Unconstrained Wieber rollout on the device (config.strict == False).
//
// Reference (per walk, sequential, one QP per axis per timestep):
//   generate_com_trajectory_wieber   zmp_controller.py:59-108
//   generate_state_trajectory_wieber zmp_controller.py:110-147
//   predict_wieber_axis (strict=False) zmp_controller.py:196-201
//     X = -inv(PuᵀPu + R/Q·I) Puᵀ (Px x - z_ref);  x⁺ = A x + B X[0]
// Only X[0] is used, so with the plan's gain row k (= row 0 of inv(M) Puᵀ) and kx = k·Px:
//     u_i = f_i - kx·x_i,   f_i = Σ_j k_j z_ref[i+1+j]   (window rows i+1..i+N, :95-104)
// f does not depend on the state, so the N-long dot products of all timesteps are computed
// in parallel (a sliding correlation), and only the 3-dim state recursion is sequential;
// that recursion is run as a lane-parallel affine scan.
//
// This unit holds the kernels of walks of at most 64·8+1 samples (one correlation pass; lane l owns
// timesteps [l·CW, l·CW + CW)) and both launch entries:
//   - the split kernel (split_walk), the default: one 128-thread workgroup per walk, wave 0 the x
//     axis and wave 1 the y axis; z_ref = (z_max + z_min)/2 (:197) staged in LDS and padded with the
//     last row (:81-88), the correlation (sparse-difference, fast-FIR or direct), a DPP affine
//     scan over the 64 lanes with P = Ā^CW (Ā = A - B kxᵀ, powers from the plan), and the replay
//     in the reference form x⁺ = A x + B u with the F_ext kick (:105-106) into the staged history
//     or, in the fused form (zmpc_rollout_metrics), into the walk metrics;
//   - the one-wave kernel (zmpc_rollout_unc_kernel, both axes in one wavefront): the cross-check
//     (ZMPC_OPT_ROLLOUT_KERNEL = 1) and the fallback where the split kernel's LDS passes 64 KiB;
//   - zmpc_shared_f_kernel (shared CoP) and the single-step kernel.
// Longer walks take the wide and chunk kernels of rollout_long.hip; what both units use is in
// rollout_common.h.
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>
#include <vector>

#include "rollout_common.h"

namespace {

// Scan, replay and store of one walk of the one-wave kernel: a0/a1[q] = f of timestep
// lane·CW + q, in registers.  `stage` (>= 2·lzp doubles) is free LDS.
template <int CW>
__device__ __forceinline__ void scan_replay_store(const RolloutArgs& a, int64_t b, int lane,
                                                  const double* a0, const double* a1,
                                                  double* stage, const double* xi0,
                                                  const double* xi1, double kk) {
  const int n = a.n, nsteps = n - 1;
  const LipmConsts lc = a.lc;
  const double kx0 = a.kx[0], kx1 = a.kx[1], kx2 = a.kx[2];
  const double Bv[3] = {lc.T3_6, lc.T2_2, lc.T};
  Mat3 Ab;  // Ā = A - B kxᵀ
  {
    const double A[9] = {1.0, lc.T, lc.T2_2, 0.0, 1.0, lc.T, 0.0, 0.0, 1.0};
    const double kx[3] = {kx0, kx1, kx2};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Ab.m[3 * i + j] = A[3 * i + j] - Bv[i] * kx[j];
  }
  const int mbeg = lane * CW;
  const int64_t kick_step = kick_step_of(a, b);

  // ---- 3. affine scan of x_{i+1} = Ā x_i + B f_i (+ kick) over 64 lane chunks ----------
  double s0[3] = {0.0, 0.0, 0.0}, s1[3] = {0.0, 0.0, 0.0};
  auto scan_step = [&](int m, double fx, double fy) {
    double t[3];
    matvec3(Ab, s0, t);
    s0[0] = fma(Bv[0], fx, t[0]);
    s0[1] = fma(Bv[1], fx, t[1]);
    s0[2] = fma(Bv[2], fx, t[2]);
    matvec3(Ab, s1, t);
    s1[0] = fma(Bv[0], fy, t[0]);
    s1[1] = fma(Bv[1], fy, t[1]);
    s1[2] = fma(Bv[2], fy, t[2]);
    if (m == kick_step) s1[1] -= kk;
  };
#pragma unroll
  for (int q = 0; q < CW; ++q)
    if (mbeg + q < nsteps) scan_step(mbeg + q, a0[q], a1[q]);
  Mat3 P;  // P = Ā^CW (from the plan when it has the table)
  const bool pre = a.scanP != nullptr;
  if (pre) {
#pragma unroll
    for (int q = 0; q < 9; ++q) P.m[q] = a.scanP[(CW - 1) * kScanStride + q];
  } else {
    P = Ab;
    for (int q = 1; q < CW; ++q) P = matmul3(P, Ab);
  }
  if (lane == 0) {
    double t[3];
    matvec3(P, xi0, t);
    for (int i = 0; i < 3; ++i) s0[i] += t[i];
    matvec3(P, xi1, t);
    for (int i = 0; i < 3; ++i) s1[i] += t[i];
  }
  // inclusive Kogge-Stone: T_l += P^d T_{l-d}
  Mat3 Pd = P;
  int r2 = 0;
  for (int d = 1; d < (dbgb(a, 2) ? 1 : 64); d <<= 1, ++r2) {
    double u0[3], u1[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      u0[i] = __shfl_up(s0[i], d, 64);
      u1[i] = __shfl_up(s1[i], d, 64);
    }
    if (lane >= d) {
      double t[3];
      matvec3(Pd, u0, t);
      for (int i = 0; i < 3; ++i) s0[i] += t[i];
      matvec3(Pd, u1, t);
      for (int i = 0; i < 3; ++i) s1[i] += t[i];
    }
    if (pre && r2 < 5) {
#pragma unroll
      for (int q = 0; q < 9; ++q) Pd.m[q] = a.scanP[(CW - 1) * kScanStride + (r2 + 1) * 9 + q];
    } else {
      Pd = matmul3(Pd, Pd);
    }
  }
  double x[3], y[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double p0 = __shfl_up(s0[i], 1, 64);
    const double p1 = __shfl_up(s1[i], 1, 64);
    x[i] = (lane == 0) ? xi0[i] : p0;
    y[i] = (lane == 0) ? xi1[i] : p1;
  }

  // ---- 4. replay in the reference form x⁺ = A x + B u; store through LDS ------------
  // Lane l produces history rows l·CW+1 .. l·CW+CW, i.e. 48-B pieces 48·CW bytes apart across
  // lanes; written directly that is one L2 request per lane per 16 B.  Instead the rows
  // are staged in LDS, `rows_per_round` at a time, and copied out as contiguous 1-KiB wave
  // stores; the cheap replay is recomputed once per round.
  const int rows_per_round = (2 * a.lzp) / 6;
  double* hb = a.hist + b * (int64_t)n * 6;
  const double xs0[3] = {x[0], x[1], x[2]}, ys0[3] = {y[0], y[1], y[2]};
  for (int r0 = 0; r0 < n; r0 += rows_per_round) {
    const int r1 = min(r0 + rows_per_round, n);
    if (lane == 0 && r0 == 0) {
      stage[0] = xi0[0];
      stage[1] = xi0[1];
      stage[2] = xi0[2];
      stage[3] = xi1[0];
      stage[4] = xi1[1];
      stage[5] = xi1[2];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      x[i] = xs0[i];
      y[i] = ys0[i];
    }
    auto replay_step = [&](int m, double fx, double fy) {
      const double ux = fx - (kx0 * x[0] + kx1 * x[1] + kx2 * x[2]);
      const double uy = fy - (kx0 * y[0] + kx1 * y[1] + kx2 * y[2]);
      double xn[3], yn[3];
      lipm_step(lc, x, ux, xn);
      lipm_step(lc, y, uy, yn);
      if (m == kick_step) yn[1] -= kk;
      const int row = m + 1;
      if (row >= r0 && row < r1) {
        double* o = stage + (row - r0) * 6;
        o[0] = xn[0];
        o[1] = xn[1];
        o[2] = xn[2];
        o[3] = yn[0];
        o[4] = yn[1];
        o[5] = yn[2];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        x[i] = xn[i];
        y[i] = yn[i];
      }
    };
#pragma unroll
    for (int q = 0; q < CW; ++q)
      if (mbeg + q < nsteps) replay_step(mbeg + q, a0[q], a1[q]);
    __syncthreads();
    if (!dbgb(a, 4)) {
      const int nd2 = (r1 - r0) * 3;  // double2 items
      const double2* src = reinterpret_cast<const double2*>(stage);
      double2* dst = reinterpret_cast<double2*>(hb + (int64_t)r0 * 6);
      for (int e = lane; e < nd2; e += 64) dst[e] = src[e];
    }
    __syncthreads();
  }
  if (a.status != nullptr) {
    const bool finite = isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]) &&
                        isfinite(y[0]) && isfinite(y[1]) && isfinite(y[2]);
    const unsigned long long bad = __ballot(!finite);
    if (lane == 0) a.status[b] = bad ? ZMPC_ST_NONFINITE : 0;
  }
}

// Walks of at most 64·CW+1 samples (one correlation pass): one wave per walk, f stays in
// registers (lane l's CW outputs are exactly its scan chunk).
template <int CW>
__global__ void __launch_bounds__(64) zmpc_rollout_unc_kernel(RolloutArgs a) {
  constexpr int PF = CW + 1;  // 64·(CW+1) >= n
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  double* ks = smem;
  double* zr0 = smem + a.kcp;
  double* zr1 = zr0 + a.lzp;
  BoundRegs<PF> r;
  if (!dbgb(a, 8)) load_bounds<PF>(a, b, lane, r);
  // everything the tail needs is requested up front, behind the bound loads
  const double* xb = a.x0 + b * 6;
  const double xi0[3] = {xb[0], xb[1], xb[2]};
  const double xi1[3] = {xb[3], xb[4], xb[5]};
  const double kk = (a.kick != nullptr) ? a.kick[b] : 0.0;
  for (int j = lane; j < a.kcp; j += 64) ks[j] = a.k[j];
  store_zref<CW, PF>(a, r, zr0, zr1, lane);
  __syncthreads();
  double a0[CW], a1[CW];
  if (!dbgb(a, 1)) {
    correlate<CW>(a, ks, zr0, zr1, lane * CW, a0, a1);
  } else {
#pragma unroll
    for (int m = 0; m < CW; ++m) a0[m] = a1[m] = 0.0;
  }
  __syncthreads();
  scan_replay_store<CW>(a, b, lane, a0, a1, zr0, xi0, xi1, kk);
}

// Split-axis single-pass kernels: a 128-thread workgroup per walk, wave 0 solves the x axis
// and wave 1 the y axis (half the registers and twice the waves of the one-wave kernel, for
// latency hiding); they share the staged z_ref and the history staging rows, so loads and
// stores stay whole-walk coalesced.
template <int CW>
struct AxisBounds {
  static constexpr int PF2 = (CW + 2) / 2;  // 128·PF2 >= 64·(CW+1) >= n
  double2 hi[PF2], lo[PF2];
};

template <int CW>
__device__ __forceinline__ void axis_load(const RolloutArgs& a, int64_t b, int tid,
                                          AxisBounds<CW>& r) {
  // The walk's two rows as wave-uniform bases (scalar registers) and one 32-bit byte offset per
  // round that both arrays share: `global_load v, v_off, s[base]`, no 64-bit address per load.
  const char* zmx = reinterpret_cast<const char*>(a.zmax + b * a.bstride);
  const char* zmn = reinterpret_cast<const char*>(a.zmin + b * a.bstride);
  const unsigned last = (unsigned)(a.n - 1) * 16u;
#pragma unroll
  for (int u = 0; u < AxisBounds<CW>::PF2; ++u) {
    // clamped rather than predicated (predicated double2 loads here crash the gfx950 backend
    // of ROCm 7.2 in machine copy propagation); dbg bit 8 turns every load into row 0
    const unsigned off = dbgb(a, 8) ? 0u : min((unsigned)(u * 128 + tid) * 16u, last);
    r.hi[u] = *reinterpret_cast<const double2*>(zmx + off);
    r.lo[u] = *reinterpret_cast<const double2*>(zmn + off);
  }
}

// The same correlation in two-parallel fast-FIR form (odd CW).  With g_j = z_ref[s + 1 + j]
// (s = lane·CW), E_m = k_{2m}, O_m = k_{2m+1} and h_j = g_j + g_{j+1}, the half-length sums
//   A(t) = Σ_m E_m g_{t+2m},  Bo(t) = Σ_m O_m g_{t+2m+1},  C(t) = Σ_m (E_m + O_{m−1}) h_{t+2m}
// give f_t = A(t) + Bo(t) and f_{t+1} = C(t) − A(t) − Bo(t+2) (C(t) = A(t) + f_{t+1} + Bo(t+2)).
// The lane's CW outputs are ⌊CW/2⌋ pairs (t = s + 2i) and one single (t = s + CW − 1, which
// reuses the last pair's Bo(t+2)): ⌈CW/2⌉ A, ⌈CW/2⌉ Bo and ⌊CW/2⌋ C sums of ⌈(N+1)/2⌉ taps —
// 11 × 76 FMAs + 76 additions (h) at CW = 7, N = 150, against 7 × 154 for the direct form.
// A window of W = CW + 1 samples slides two per step (ring of W registers, renamed by the U-step
// unroll), the h values a ring of U; one 16-byte pair of samples per step from LDS, the taps
// (E_m, O_m, E_m + O_{m−1}) one wave-uniform row of the plan's table.
template <int CW>
__device__ __forceinline__ void axis_correlate_ffa(const RolloutArgs& a,
                                                   const double* __restrict__ kt,
                                                   const double* zr, int lane, double* f) {
  static_assert(CW & 1, "the fast-FIR correlation takes odd chunk widths (no LDS padding)");
  constexpr int NP = CW / 2, NA = NP + 1, NB = NP + 1, NC = NP, U = NP + 1, W = 2 * U;
  const double* g = zr + lane * CW + 1;
  double w[W], hr[U], A[NA], Bo[NB], C[NC > 0 ? NC : 1];
#pragma unroll
  for (int j = 0; j < W; ++j) w[j] = g[j];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    A[i] = 0.0;
    Bo[i] = 0.0;
  }
#pragma unroll
  for (int i = 0; i < NC; ++i) C[i] = 0.0;
#pragma unroll
  for (int i = 0; i + 1 < NC; ++i) hr[i] = w[2 * i] + w[2 * i + 1];  // h_{s+2i}
  const int mloop = dbgb(a, 1) ? 0 : a.kfm;
  const double* tr = kt;
  for (int m0 = 0; m0 < mloop; m0 += U, tr += 4 * U) {
#pragma unroll
    for (int mm = 0; mm < U; ++mm) {
      const double E = tr[4 * mm], O = tr[4 * mm + 1], EO = tr[4 * mm + 2];
      const int b = 2 * mm;  // ring base (2m mod W: m0 is a multiple of U)
      if (NC > 0) hr[(mm + NC - 1) % U] = w[(b + 2 * NC - 2) % W] + w[(b + 2 * NC - 1) % W];
#pragma unroll
      for (int i = 0; i < NA; ++i) A[i] = fma(E, w[(b + 2 * i) % W], A[i]);
#pragma unroll
      for (int i = 0; i < NB; ++i) Bo[i] = fma(O, w[(b + 2 * i + 1) % W], Bo[i]);
#pragma unroll
      for (int i = 0; i < NC; ++i) C[i] = fma(EO, hr[(mm + i) % U], C[i]);
      w[b % W] = g[2 * (m0 + mm) + W];
      w[(b + 1) % W] = g[2 * (m0 + mm) + W + 1];
    }
  }
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    f[2 * i] = A[i] + Bo[i];
    f[2 * i + 1] = (C[i] - A[i]) - Bo[i + 1];
  }
  f[CW - 1] = A[NP] + Bo[NP];
}

// The correlation by summation by parts over the walk's z_ref changes.  With S_j = Σ_{j'≥j} k_j'
// and d_m = z_ref[m+1] − z_ref[m],
//   f_t = Σ_j k_j z_ref[t+1+j] = S_0 z_ref[t+1] + Σ_{j=1}^{N−1} S_j d_{t+j},
// and the CoP references the footstep generators produce (cop_generator.py:34-115: one box per
// support phase) are piecewise constant, so d is zero except at the support-phase switches —
// ≈16 changes per axis in a 420-sample default.json walk against 150 taps per output.  The wave
// finds its axis's changes with one ballot per chunk column (lane l tests m = l·CW + q), then
// walks the set bits: every lane adds S_{m−t}·d_m to its CW outputs t (Ts = the plan's ksum
// table staged in LDS; entries outside 1 ≤ j ≤ N−1 are zero, so lanes the change does not reach
// read zeros at a clamped offset).  Exact for any input; a wave whose axis changes more than
// kSparseMax times (dense bounds) returns false and takes the dense form instead.  Rounding
// differs from the direct sum by ≈ε·Σ|S_j d_j| (test_sparse_correlation_equals_dense).
constexpr int kSparseMax = 40;

template <int CW>
__device__ __forceinline__ bool axis_correlate_sparse(const RolloutArgs& a, const double* zr,
                                                      const double* Ts, int lane, double* f) {
  using ZL = ZrLayout<CW>;
  const double* z = zr + ZL::idx(lane * CW);
  double gv[CW + 1], d[CW];
  unsigned long long mk[CW];
  int cnt = 0;
#pragma unroll
  for (int j = 0; j <= CW; ++j) gv[j] = z[ZL::idx(j)];
#pragma unroll
  for (int q = 0; q < CW; ++q) {
    d[q] = gv[q + 1] - gv[q];
    mk[q] = __ballot(d[q] != 0.0);
    cnt += __popcll(mk[q]);
  }
  if (cnt > kSparseMax) return false;
  const int N = a.hN, s = lane * CW;
  const double S0 = Ts[ksum_s0(N)];
#pragma unroll
  for (int r = 0; r < CW; ++r) f[r] = S0 * gv[r + 1];
  // the table offset in bytes: the lane's s scaled once per walk
  const unsigned s8 = (unsigned)s * 8u, e8max = (unsigned)(N + CW - 1) * 8u;
#pragma unroll
  for (int q = 0; q < CW; ++q) {
    unsigned long long m = mk[q];
    while (m) {
      const int L = __builtin_ctzll(m);
      m &= m - 1;
      const double dv = readlane_f64(d[q], L);
      // f_{s+r} += S_{e−r} d with e = m − s, S_{e−r} = Ts[e − r + 8]
      // One unsigned minimum clamps both sides: a change before the lane's chunk (e < 0) wraps
      // to a large offset and lands on e = N + CW − 1 with a change out of reach ahead, where the
      // CW entries read are the table's upper zeros, as its lower zeros are at e = 0.
      const unsigned e8 = min(__umul24((unsigned)L, CW * 8u) + (q * 8u - s8), e8max);
      const double* p = reinterpret_cast<const double*>(reinterpret_cast<const char*>(Ts) + e8) +
                        (9 - CW);
#pragma unroll
      for (int r = 0; r < CW; ++r) f[r] = fma(p[CW - 1 - r], dv, f[r]);
    }
  }
  return true;
}

// ---- fused rollout-to-metrics (zmpc_rollout_metrics) ------------------------------------------
// What the metrics form of split_walk needs beside RolloutArgs.
struct MetArgs {
  double* metrics;         // [B, ZMPC_NMETRICS]
  const int64_t* lengths;  // [B] live samples per walk, or null: n
  double hg, sqrt_hg;      // h/g and its root (plan)
};

// One lane's share of one axis of the walk metrics, and the butterfly that combines the 64 lanes:
// the quantities, the strict comparisons, the tie rule and the uncontracted arithmetic of
// metrics.hip AxisAcc (include/zmpc.h zmpc_walk_metrics), here fed from the replay's registers.
struct MetAcc {
  double vmax = 0.0;     // largest violation so far
  int vidx = -1;         // its first sample, −1 while vmax is 0
  int count = 0;         // samples with a violation
  double dev = 0.0;      // largest |c − zr|
  double sq = 0.0;       // Σ (z − zr)²
  int bad = 0x7fffffff;  // first sample with a non-finite state value

  __device__ __forceinline__ void add(int i, double c, double v, double a, double hi, double lo,
                                      double hg) {
#pragma clang fp contract(off)
    if (!(isfinite(c) && isfinite(v) && isfinite(a))) {
      bad = min(bad, i);
      return;
    }
    const double z = c - hg * a;
    const double zr = (hi + lo) * 0.5;
    const double viol = fmax(fmax(z - hi, lo - z), 0.0);
    if (viol > 0.0) ++count;
    if (viol > vmax) {  // strict: a lane's samples ascend, the first one that attains it stays
      vmax = viol;
      vidx = i;
    }
    dev = fmax(dev, fabs(c - zr));
    const double d = z - zr;
    sq += d * d;
  }

  // c + ċ·sqrt(h/g) − zr of one sample (dcm_end)
  __device__ static __forceinline__ double dcm(double c, double v, double hi, double lo,
                                               double sqrt_hg) {
#pragma clang fp contract(off)
    return c + v * sqrt_hg - (hi + lo) * 0.5;
  }

  // xor butterfly over the wave: symmetric in the two lanes, so every lane ends with the same
  // bits in an order fixed by the lane numbers; a tie in the violation goes to the lower index
  __device__ __forceinline__ void reduce() {
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) {
      const double ov = __shfl_xor(vmax, mask);
      const int oi = __shfl_xor(vidx, mask);
      if (ov > vmax || (ov == vmax && oi < vidx)) {
        vmax = ov;
        vidx = oi;
      }
      count += __shfl_xor(count, mask);
      dev = fmax(dev, __shfl_xor(dev, mask));
      sq += __shfl_xor(sq, mask);
      bad = min(bad, __shfl_xor(bad, mask));
    }
  }

  // slot k (viol_max, viol_argmax, viol_count, com_dev_max, zmp_rms, dcm_end) of the axis
  __device__ __forceinline__ double slot(int k, int nb, double dcm_end) const {
#pragma clang fp contract(off)
    if (bad != 0x7fffffff)  // fail safe, as metrics.hip
      return k == 0 ? __builtin_inf() : (k == 1 ? (double)bad : __builtin_nan(""));
    switch (k) {
      case 0: return vmax;
      case 1: return (double)vidx;
      case 2: return (double)count;
      case 3: return dev;
      case 4: return sqrt(sq / (double)nb);
      default: return dcm_end;
    }
  }
};

// Split-axis kernel, one walk per 128-thread workgroup: wave 0 solves the x axis and wave 1 the
// y axis (half the registers and twice the waves of the one-wave kernel, for latency hiding);
// they share the staged z_ref and the history staging rows, so loads and stores stay whole-walk
// coalesced.  The fewest serial steps: every global load (bounds, the last sample for the window
// padding, x0, kick) issued up front, z_ref + padding in one pass, one replay writing the whole
// walk's history rows into the dead z_ref area (LDS sized for it), and one coalesced copy-out —
// three barriers per walk.  The tables read on wave-uniform addresses come in as __restrict__
// pointers so the compiler keeps them on scalar loads even inside a loop that stores the history.
// SHF: shared CoP, f precomputed once per launch (zmpc_shared_f_kernel).
// MET (zmpc_rollout_metrics): phases 1–4 as they are; the replay feeds each state to the walk
// metrics instead of a history row, the two waves' six numbers leave as one 96-byte row, and no
// history exists (hist is null).  The bounds registers of phase 1 stay alive over the correlation
// and go into the dead z_ref area as (z_max, z_min) pairs per axis, where each lane finds the rows
// of its own samples: the metrics see the bounds themselves, not z_ref ± a half width.
// PFB: with the next-dispatch-round prefetch (launch_unc: pf_ahead > 0).
// The dense correlation of odd chunk widths is the two-parallel fast-FIR form (kg = its taps).
template <int CW, bool SHF, bool PFB, bool MET = false>
__device__ __forceinline__ void split_walk(const RolloutArgs& a, int64_t b, double* smem,
                                           int* flag, const double* __restrict__ kg,
                                           const double* __restrict__ scanP,
                                           const double* __restrict__ kxp,
                                           double* __restrict__ hist,
                                           const MetArgs& mo = MetArgs{},
                                           double* mrow = nullptr) {
  using ZL = ZrLayout<CW>;
  const int tid = threadIdx.x, lane = tid & 63, axis = tid >> 6;
  const int n = a.n, nsteps = n - 1;
  const double* Gc = scanP + kScanGOff;  // the chunk-sum columns Ā^p B, Ā^p e1
  double f[CW];
  double pf0 = 0.0, pf1 = 0.0;  // prefetch results (kept alive to the end, never used)
  AxisBounds<CW> r;
  double2 hl, ll;
  double ts0 = 0.0, ts1 = 0.0;  // this thread's two rows of the suffix-sum table
  tl_stamp(a, b, 0);
  // ---- 1. loads ------------------------------------------------------------------------------
  // Every global load of the walk is issued here, before the first wait, as straight-line code
  // (clamped indices, no runtime branch around a load): the compiler then waits with exact
  // partial counts, and the walk's own data is one memory round trip away.  Order: x0 and kick,
  // the bounds, the last sample (wave-uniform: scalar loads), the table rows.
  const double* xb = reinterpret_cast<const double*>(reinterpret_cast<const char*>(a.x0 + b * 6) +
                                                     (unsigned)axis * 24u);
  const double xi[3] = {xb[0], xb[1], xb[2]};
  const double kks = (a.kick != nullptr) ? a.kick[b] : 0.0;  // wave-uniform: a scalar load
  if constexpr (SHF) {
    // shared CoP: f of this lane's timesteps, computed once per launch (zmpc_shared_f_kernel)
    const double* fp = a.fsh + axis * a.fstride + lane * CW;
#pragma unroll
    for (int q = 0; q < CW; ++q) f[q] = fp[q];
    if constexpr (MET) axis_load<CW>(a, b, tid, r);  // the one CoP (stride 0), from the caches
  } else {
    axis_load<CW>(a, b, tid, r);
    hl = reinterpret_cast<const double2*>(a.zmax + b * a.bstride)[n - 1];
    ll = reinterpret_cast<const double2*>(a.zmin + b * a.bstride)[n - 1];
    // rows tid and tid + 128 of the plan's suffix-sum table (sparse-difference correlation), into
    // LDS with the z_ref rows below; without the table (dense plans) the loads read row 0 of k
    {
      const double* tp = a.ksum != nullptr ? a.ksum : kg;
      const int tl = a.ksum != nullptr ? ksum_rows(a.hN) - 1 : 0;
      const char* tb = reinterpret_cast<const char*>(tp);  // uniform base, 32-bit byte offsets
      ts0 = *reinterpret_cast<const double*>(tb + min((unsigned)tid, (unsigned)tl) * 8u);
      ts1 = *reinterpret_cast<const double*>(tb + min((unsigned)tid + 128u, (unsigned)tl) * 8u);
    }
  }
  // The kick, all wave-uniform and on the scalar unit: the lane kl that owns the kick step, the
  // step's place qk in that lane's chunk and the kick's chunk-sum column Ā^(CW−1−qk) e1.  Only the
  // y wave of a walk whose kick step is one of its nsteps steps is `kicked`.
  const bool ywave = __builtin_amdgcn_readfirstlane(axis) != 0;
  const int64_t kick_step = kick_step_of(a, b);
  const bool kicked = ywave && kick_step >= 0 && kick_step < nsteps;
  const int ksi = kicked ? (int)kick_step : 0;
  const int kl = ksi / CW, qk0 = ksi - kl * CW, qk = kicked ? qk0 : -1;
  const double* ekp = Gc + (CW - 1 - qk0) * 6 + 3;
  const double ek[3] = {ekp[0], ekp[1], ekp[2]};
  const double kk = (kicked && lane == kl) ? kks : 0.0;  // the kick on its lane, +0.0 elsewhere
  if constexpr (!SHF) {
    // the suffix-sum table first, at the workgroup's fixed LDS base (the sparse correlation's
    // table reads add a constant to their clamped offset, not the runtime 2·lzp), the two z_ref
    // areas behind it
    double* Ts = smem;
    double* zr0 = smem + (a.ksum != nullptr ? ksum_rows(a.hN) : 0);
    double* zr1 = zr0 + a.lzp;
    // ---- 2. z_ref rows + window padding (zmp_controller.py:81-88), table rows ----------------
    // Branch-free, so that the bound loads stay up front (under `if (t < n)` the compiler sinks
    // a round's loads into the branch, behind a full drain): a thread past the walk's end holds
    // the clamped load of the last sample, which is the padding value of its own row t < lz.
    constexpr int kRows = 128 * AxisBounds<CW>::PF2;  // ≥ n: the rows these stores cover
#pragma unroll
    for (int u = 0; u < AxisBounds<CW>::PF2; ++u) {
      const int t = min(u * 128 + tid, a.lz - 1);
      zr0[ZL::idx_row(t)] = (r.hi[u].x + r.lo[u].x) / 2;
      zr1[ZL::idx_row(t)] = (r.hi[u].y + r.lo[u].y) / 2;
    }
    {
      const double l0 = (hl.x + ll.x) / 2, l1 = (hl.y + ll.y) / 2;
      for (int t = kRows + tid; t < a.lz; t += 128) {
        zr0[ZL::idx_row(t)] = l0;
        zr1[ZL::idx_row(t)] = l1;
      }
    }
    if (a.ksum != nullptr) {
      const int rows = ksum_rows(a.hN);
      if (tid < rows) Ts[tid] = ts0;
      if (tid + 128 < rows) Ts[tid + 128] = ts1;
      for (int i = tid + 256; i < rows; i += 128) Ts[i] = a.ksum[i];  // N > 238 only
    }
    __syncthreads();
    tl_stamp(a, b, 1);
    // ---- 3. correlation (this wave's axis) -------------------------------------------------
    // sparse z_ref differences (piecewise-constant CoP) first, else the dense forms
    const bool sparse = a.ksum != nullptr && !dbgb(a, 1) &&
                        axis_correlate_sparse<CW>(a, axis ? zr1 : zr0, Ts, lane, f);
    if (sparse) {
    } else if constexpr (CW & 1)
      axis_correlate_ffa<CW>(a, kg, axis ? zr1 : zr0, lane, f);  // kg = the fast-FIR taps
    else
      axis_correlate<CW>(a, kg, axis ? zr1 : zr0, lane, f);  // k: wave-uniform scalar loads
    __syncthreads();  // z_ref dead: the area becomes the history staging (n rows of 6)
    tl_stamp(a, b, 2);
    // ---- the next dispatch round's bounds -----------------------------------------------------
    // The bounds of the walk the next dispatch round puts on this slot, one double per 64 B
    // (threads 0..63 z_max, 64..127 z_min; two loads cover n ≤ 512 samples), so that round's
    // loads hit L2 / Infinity Cache instead of HBM.  PFB is the launcher's pf_ahead > 0; the walk
    // index is clamped (the last round's workgroups touch walk B − 1 again), so the loads are
    // straight-line code and no wait before either barrier covers them (the scan's first wait, for
    // its per-lane powers, does: they follow in the in-order counter).  They are issued here,
    // after the correlation: the first round's load phase is bound by HBM bandwidth (all resident
    // workgroups load at once), so prefetch traffic beside the walks' own loads only delays them,
    // while the scan and replay that follow use no global memory (config 2, same box: beside the
    // own loads 27.1–27.3 µs, after the first barrier 25.7–26.2, here 25.0–25.7, before the replay
    // 26.1–26.7, after the third barrier 26.0–26.4; profiles/r7/loadphase/).  Up to round 6 they
    // sat before the first barrier behind a runtime branch and the table loop's drain, so every
    // first-round wave waited for them before its correlation (27.0–27.3 µs).
    if constexpr (PFB) {
      // (the array by wave on the scalar unit: a uniform base and 32-bit byte offsets, as axis_load)
      const char* src = reinterpret_cast<const char*>((ywave ? a.zmin : a.zmax) +
                                                      min(b + a.pf_ahead, a.B - 1) * a.bstride);
      const unsigned l64 = (unsigned)lane * 64u, endb = (unsigned)(2 * n - 1) * 8u;
      pf0 = *reinterpret_cast<const double*>(src + min(l64, endb));
      pf1 = *reinterpret_cast<const double*>(src + min(l64 + 4096u, endb));
    }
  }
  // ---- (MET) the walk's bounds into the dead z_ref area ------------------------------------
  // axis a's pairs (z_max, z_min) of sample t at double2 row a·nbp + ZrLayout row(t); the barrier
  // that publishes them is the one before the replay, so the scan runs in between
  const int nbp = n + ZL::kPad * ((n - 1) / CW);
  if constexpr (MET) {
    double2* bb = reinterpret_cast<double2*>(smem);
#pragma unroll
    for (int u = 0; u < AxisBounds<CW>::PF2; ++u) {
      const int t = u * 128 + tid;
      if (t < n) {
        const int row = ZL::idx_row(t);
        bb[row] = make_double2(r.hi[u].x, r.lo[u].x);
        bb[nbp + row] = make_double2(r.hi[u].y, r.lo[u].y);
      }
    }
  }
  // ---- 4. lane-chunk affine scan -----------------------------------------------------------
  const LipmConsts lc = a.lc;
  const double kx0 = kxp[0], kx1 = kxp[1], kx2 = kxp[2];
  const int mbeg = lane * CW;
  double sv[3] = {0.0, 0.0, 0.0};
  {
    // the chunk's end state from a zero start as one sum, Σ_q Ā^(CW−1−q) B f_q (plan columns;
    // 3 FMAs per step instead of the 12 of the recursion), plus the kick's −kk Ā^(CW−1−q) e1.
    // Steps past nsteps count too: only lanes whose chunk holds no output follow such a lane.
#pragma unroll
    for (int q = 0; q < CW; ++q) {
      const double* gq = Gc + (CW - 1 - q) * 6;
#pragma unroll
      for (int i = 0; i < 3; ++i) sv[i] = fma(gq[i], f[q], sv[i]);
    }
    if (kicked) {
      if (lane == kl) {
#pragma unroll
        for (int i = 0; i < 3; ++i) sv[i] = fma(-kk, ek[i], sv[i]);
      }
    }
  }
  const double* Pp = scanP + (CW - 1) * kScanStride;  // (Ā^CW)^(2^r), r = 0..5, from the plan
  if (lane == 0) {
    double t[3];
    Mat3 P;
#pragma unroll
    for (int q = 0; q < 9; ++q) P.m[q] = Pp[q];
    matvec3(P, xi, t);
    for (int i = 0; i < 3; ++i) sv[i] += t[i];
  }
  if (!dbgb(a, 2)) scan_dpp(sv, lane, Pp, scanP + kScanPowOff + (CW - 1) * 33 * 9);
  double x[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double p = dpp_f64<0x138, 0xF>(sv[i]);  // wave_shr:1
    x[i] = (lane == 0) ? xi[i] : p;
  }
  if constexpr (MET) {
    // ---- 5m. replay (reference form) into the walk metrics ---------------------------------
    // Lane l owns samples l·CW + 1 .. l·CW + CW (the states its steps produce), lane 0 also
    // sample 0; only samples below the walk's live length n_b count.  The rollout itself runs all
    // n − 1 steps: the status is the history launch's.
    int64_t nbl = mo.lengths != nullptr ? mo.lengths[b] : (int64_t)n;  // wave-uniform
    nbl = nbl < 1 ? 1 : (nbl > n ? n : nbl);
    const int nb = (int)nbl;
    __syncthreads();  // the staged bounds
    const double2* bl = reinterpret_cast<const double2*>(smem) + axis * nbp + lane * (CW + ZL::kPad);
    MetAcc acc;
    double dcm = 0.0;  // of the lane that owns sample n_b − 1
    if (lane == 0) {
      const double2 bd = bl[0];
      acc.add(0, xi[0], xi[1], xi[2], bd.x, bd.y, mo.hg);
      if (nb == 1) dcm = MetAcc::dcm(xi[0], xi[1], bd.x, bd.y, mo.sqrt_hg);
    }
    const int live = nsteps - mbeg;
#pragma unroll
    for (int q = 0; q < CW; ++q) {
      if (q < live) {
        const double u = f[q] - (kx0 * x[0] + kx1 * x[1] + kx2 * x[2]);
        double xn[3];
        lipm_step(lc, x, u, xn);
        if (q == qk) xn[1] -= kk;  // force kick (zmp_controller.py:90,105-106)
        const int i = mbeg + q + 1;
        if (i < nb) {
          const double2 bd = bl[ZL::idx(1 + q)];
          acc.add(i, xn[0], xn[1], xn[2], bd.x, bd.y, mo.hg);
          if (i == nb - 1) dcm = MetAcc::dcm(xn[0], xn[1], bd.x, bd.y, mo.sqrt_hg);
        }
#pragma unroll
        for (int i2 = 0; i2 < 3; ++i2) x[i2] = xn[i2];
      }
    }
    acc.reduce();
    const int owner = __builtin_amdgcn_readfirstlane(nb >= 2 ? (nb - 2) / CW : 0);
    const double dcm_end = readlane_f64(dcm, owner);
    const bool finite = isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]);
    const unsigned long long badx = __ballot(!finite);
    if (lane == 0) flag[axis] = badx ? ZMPC_ST_NONFINITE : 0;
    // slot 2k + a: the two waves' six numbers interleave into one row
    if (lane < 6) mrow[2 * lane + axis] = acc.slot(lane, nb, dcm_end);
    __syncthreads();
    if (tid < ZMPC_NMETRICS) mo.metrics[b * ZMPC_NMETRICS + tid] = mrow[tid];
    if (a.status != nullptr && tid == 0) a.status[b] = flag[0] | flag[1];
    if (a.dbg < 0) mo.metrics[tid] = pf0 + pf1;  // never (dbg ≥ 0): keeps the prefetch loads
    return;
  }
  // ---- 5. replay (reference form) straight into the staged history ------------------------
  double* stage = smem;
  if (lane == 0) {
    stage[3 * axis + 0] = xi[0];
    stage[3 * axis + 1] = xi[1];
    stage[3 * axis + 2] = xi[2];
  }
  // The kick is a wave-uniform test on the step's place in the chunk (qk = −1 on a wave without a
  // kick: a scalar compare per step): kk is the kick on lane kl and +0.0 on every other lane,
  // which changes no value.  (A second copy of the replay without the test, taken by waves
  // without a kick, cost the shared-CoP kernel 2 %: config 4 unconstrained 495 vs 486 µs.)
  // The lane's CW staging rows are 48 B apart behind one address: rows l·CW + 1 .. l·CW + CW lie
  // in the pad span (l·CW + q) / (2·CW) = l / 2 for every q < CW (HistLayout::row).
  double* orow = stage + (mbeg + 1) * 6 + HistLayout<CW>::kPad * (lane >> 1) + 3 * axis;
  static_assert(HistLayout<CW>::kSpan == 2 * CW, "a lane's rows share one pad span");
  const int live = nsteps - mbeg;  // the lane's steps q < live exist (one compare per step)
#pragma unroll
  for (int q = 0; q < CW; ++q) {
    if (q < live) {
      const double u = f[q] - (kx0 * x[0] + kx1 * x[1] + kx2 * x[2]);
      double xn[3];
      lipm_step(lc, x, u, xn);
      if (q == qk) xn[1] -= kk;  // force kick (zmp_controller.py:90,105-106)
      double* o = orow + 6 * q;
      o[0] = xn[0];
      o[1] = xn[1];
      o[2] = xn[2];
#pragma unroll
      for (int i = 0; i < 3; ++i) x[i] = xn[i];
    }
  }
  if (a.status != nullptr) {
    const bool finite = isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]);
    const unsigned long long bad = __ballot(!finite);
    if (lane == 0) flag[axis] = bad ? ZMPC_ST_NONFINITE : 0;
  }
  __syncthreads();
  tl_stamp(a, b, 3);
  // ---- 6. coalesced copy-out ---------------------------------------------------------------
  if (!dbgb(a, 4)) {
    const double2* src = reinterpret_cast<const double2*>(stage);
    double2* dst = reinterpret_cast<double2*>(hist + b * (int64_t)n * 6);
    const int ne = n * 3;
    // four rows in flight per thread (LDS reads batched ahead of the stores); the history is
    // written once and never re-read here: non-temporal stores (config 4 unconstrained
    // 0.547 → 0.497 ms in an A/B on one box; config 2 unchanged)
    int e = tid;
    if constexpr (HistLayout<CW>::kPad == 0) {
      for (; e + 3 * 128 < ne; e += 4 * 128) {
        const double2 v0 = src[e], v1 = src[e + 128], v2 = src[e + 256], v3 = src[e + 384];
        st_nt2(&dst[e], v0);
        st_nt2(&dst[e + 128], v1);
        st_nt2(&dst[e + 256], v2);
        st_nt2(&dst[e + 384], v3);
      }
      for (; e < ne; e += 128) st_nt2(&dst[e], src[e]);
    } else {
      // element e (a double2) of row r = e / 3 sits behind (r − 1) / (2·CW) pads of one double2
      auto at = [](int e2) {
        const int r = e2 / 3;
        return e2 + (r >= 1 ? (r - 1) / HistLayout<CW>::kSpan : 0) * (HistLayout<CW>::kPad / 2);
      };
      for (; e + 3 * 128 < ne; e += 4 * 128) {
        const double2 v0 = src[at(e)], v1 = src[at(e + 128)], v2 = src[at(e + 256)],
                      v3 = src[at(e + 384)];
        st_nt2(&dst[e], v0);
        st_nt2(&dst[e + 128], v1);
        st_nt2(&dst[e + 256], v2);
        st_nt2(&dst[e + 384], v3);
      }
      for (; e < ne; e += 128) st_nt2(&dst[e], src[at(e)]);
    }
  }
  tl_stamp(a, b, 4);
  if (a.status != nullptr && tid == 0) a.status[b] = flag[0] | flag[1];
  if (a.dbg < 0) hist[tid] = pf0 + pf1;  // never (dbg ≥ 0): keeps the prefetch loads
}

// Shared CoP (bounds stride 0, e.g. an F_ext sweep over one walk): z_ref, and so f, is the
// same for every walk, so the correlation runs once per launch — one thread per (axis,
// timestep), the taps in the per-walk kernels' order (fma chain from 0 over j = 0..kc−1) — and
// the rollout kernel reads it instead (split_walk<CW, true>); histories equal the per-walk
// kernels' to rounding (≈1e-15 relative: the compiler contracts the two kernels differently).
__global__ void __launch_bounds__(256) zmpc_shared_f_kernel(const double* __restrict__ zmax,
                                                            const double* __restrict__ zmin,
                                                            int n, const double* __restrict__ k,
                                                            int kc, double* fsh, int fstride) {
  const int i = blockIdx.x * 256 + threadIdx.x;  // timestep
  const int axis = blockIdx.y;
  if (i >= fstride) return;
  double acc = 0.0;
  for (int j = 0; j < kc; ++j) {
    const int t = min(i + 1 + j, n - 1);  // window padding with the last row (:81-88)
    const double z = (zmax[2 * t + axis] + zmin[2 * t + axis]) / 2;
    acc = fma(k[j], z, acc);
  }
  fsh[axis * fstride + i] = acc;
}

// One walk per workgroup (the default; odd chunk widths with the fast-FIR dense form), and the
// shared-CoP form (SHF).  (The tables come through the argument struct: as __restrict__ kernel
// arguments they go to SGPRs and the DPP scan's per-lane powers push the kernel into spills.)
template <int CW, bool SHF, bool PFB = false>
__global__ void __launch_bounds__(128, 4) zmpc_rollout_unc_splitd_kernel(RolloutArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ int flag[2];
  split_walk<CW, SHF, PFB>(a, blockIdx.x, smem, flag, (CW & 1) ? a.kffa : a.k, a.scanP, a.kx,
                           a.hist);
}

// The fused rollout-to-metrics kernels: the walk of zmpc_rollout_unc_splitd_kernel<CW, SHF>
// with the metrics replay (split_walk MET), one walk per 128-thread workgroup; no next-round
// prefetch (launch_metrics).
template <int CW, bool SHF>
__global__ void __launch_bounds__(128, 4)
    zmpc_rollout_metrics_splitd_kernel(RolloutArgs a, MetArgs mo) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ int flag[2];
  __shared__ double mrow[ZMPC_NMETRICS];
  split_walk<CW, SHF, false, true>(a, blockIdx.x, smem, flag, (CW & 1) ? a.kffa : a.k, a.scanP,
                                   a.kx, nullptr, mo, mrow);
}

// n = 1: the metrics of the initial state alone (the rollout is a copy of x0, status 0); one
// thread per walk and axis through the same accumulator.
__global__ void __launch_bounds__(256) zmpc_metrics_x0_kernel(RolloutArgs a, MetArgs mo) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= 2 * a.B) return;
  const int64_t b = e >> 1;
  const int axis = (int)(e & 1);
  const double* x = a.x0 + b * 6 + 3 * axis;
  const double hi = a.zmax[b * a.bstride + axis], lo = a.zmin[b * a.bstride + axis];
  MetAcc acc;
  acc.add(0, x[0], x[1], x[2], hi, lo, mo.hg);
  const double dcm_end = MetAcc::dcm(x[0], x[1], hi, lo, mo.sqrt_hg);
#pragma unroll
  for (int k = 0; k < 6; ++k) mo.metrics[b * ZMPC_NMETRICS + 2 * k + axis] = acc.slot(k, 1, dcm_end);
  if (a.status != nullptr && axis == 0) a.status[b] = 0;
}

// Batched predict_wieber_axis (strict=False): one wave per instance.
__global__ void __launch_bounds__(256) zmpc_step_unc_kernel(
    int64_t B, int N, LipmConsts lc, const double* __restrict__ k, const double* __restrict__ kxp,
    const double* __restrict__ x, const double* __restrict__ zmax_win,
    const double* __restrict__ zmin_win, double* __restrict__ x_next,
    int32_t* __restrict__ status) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  const double* zx = zmax_win + b * N;
  const double* zn = zmin_win + b * N;
  double acc = 0.0;
  for (int j = lane; j < N; j += 64) acc = fma(k[j], (zx[j] + zn[j]) / 2, acc);
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) {
    const double* xb = x + b * 3;
    const double xs[3] = {xb[0], xb[1], xb[2]};
    const double u = acc - (kxp[0] * xs[0] + kxp[1] * xs[1] + kxp[2] * xs[2]);
    double y[3];
    lipm_step(lc, xs, u, y);
    x_next[b * 3 + 0] = y[0];
    x_next[b * 3 + 1] = y[1];
    x_next[b * 3 + 2] = y[2];
    if (status != nullptr)
      status[b] = (isfinite(y[0]) && isfinite(y[1]) && isfinite(y[2])) ? 0 : ZMPC_ST_NONFINITE;
  }
}

// Which kernel a call takes, its geometry and its LDS are dispatch.h choose_unc's; the launchers
// below pick the template instance of that choice and add the one rule that needs the runtime,
// the next-dispatch-round prefetch (pf_ahead, from an occupancy query).

// Calls fn(std::integral_constant<int, C>) for the tile width C = cw in 1..8; false: no such width.
template <int... I, class F>
bool with_cw(std::integer_sequence<int, I...>, int cw, F&& fn) {
  return ((cw == I + 1 && (fn(std::integral_constant<int, I + 1>{}), true)) || ...);
}
template <class F>
bool with_cw(int cw, F&& fn) {
  return with_cw(std::make_integer_sequence<int, 8>{}, cw, fn);
}

// The kernel arguments both launches share: the call, the plan's tables and the choice's geometry.
RolloutArgs make_args(const zmpc_plan* p, const RolloutCall& rc, const WalkGeom& g) {
  RolloutArgs a{};
  a.kc = g.kc;
  a.kcp = g.kcp;
  a.lz = g.lz;
  a.lzp = g.lzp;
  a.n = (int)rc.n;
  a.B = rc.B;
  a.lc = p->lc;
  a.k = p->k;
  a.kx = p->kx;
  a.zmax = rc.zmax;
  a.zmin = rc.zmin;
  a.bstride = rc.bstride;
  a.x0 = rc.x0;
  a.kick = rc.kick;
  a.kick_step = rc.kick_step;
  a.status = rc.status;
  a.scanP = p->scanP;
  a.kick_steps = rc.kick_steps;
  a.kffa = p->kffa;
  a.kfm = g.kfm;
  a.ksum = g.sparse ? p->ksum : nullptr;
  a.hN = p->N;
  a.fstride = g.fstride;
  return a;
}

// launch() — the rollout kernel's launch, returning its error — with, for the shared CoP, f of
// both axes computed once into a stream-ordered buffer (a.fsh) that is freed behind the launch.
template <class L>
hipError_t launch_with_shared_f(bool shared, const zmpc_plan* p, const RolloutCall& rc,
                                hipStream_t s, RolloutArgs& a, L&& launch) {
  double* fsh = nullptr;
  if (shared) {
    if (hipMallocAsync((void**)&fsh, 2 * (size_t)a.fstride * sizeof(double), s) != hipSuccess) {
      (void)hipGetLastError();
      return hipErrorOutOfMemory;
    }
    hipLaunchKernelGGL(zmpc_shared_f_kernel, dim3((unsigned)((a.fstride + 255) / 256), 2),
                       dim3(256), 0, s, rc.zmax, rc.zmin, (int)rc.n, p->k, a.kc, fsh, a.fstride);
    a.fsh = fsh;
  }
  hipError_t e = launch();
  if (fsh) {
    const hipError_t ef = hipFreeAsync(fsh, s);
    if (e == hipSuccess) e = ef;
  }
  return e;
}

// Walks of at most 64·8+1 samples (one correlation pass): SplitShared, Generic or Split at tile
// width CW.  Split runs with the next-round prefetch when the batch takes at most two dispatch
// rounds (config 2: 29.6 → 26.9 µs, profiles/r3pf/; with more rounds the touched lines are
// evicted before use, B = 16384: 92 → 117 µs).  Even and odd CW take the same kernel.
template <int CW>
void launch_unc(const UncChoice& c, hipStream_t s, RolloutArgs a, int cus) {
  if (c.kind == UncKind::SplitShared) {
    // shared CoP, f precomputed: scan, replay and the history stores only
    hipLaunchKernelGGL((zmpc_rollout_unc_splitd_kernel<CW, true>), dim3((unsigned)a.B),
                       dim3(128), c.lds, s, a);
    return;
  }
  if (c.kind == UncKind::Generic) {
    hipLaunchKernelGGL(zmpc_rollout_unc_kernel<CW>, dim3((unsigned)a.B), dim3(64), c.lds, s, a);
    return;
  }
  const int occ = occupancy(
      reinterpret_cast<const void*>(zmpc_rollout_unc_splitd_kernel<CW, false, true>), 128, c.lds);
  const int64_t R = (int64_t)std::max(cus, 1) * occ;
  a.pf_ahead = (R > 0 && a.n <= 512 && a.B <= 2 * R) ? R : 0;
  if (a.pf_ahead > 0)
    hipLaunchKernelGGL((zmpc_rollout_unc_splitd_kernel<CW, false, true>), dim3((unsigned)a.B),
                       dim3(128), c.lds, s, a);
  else
    hipLaunchKernelGGL((zmpc_rollout_unc_splitd_kernel<CW, false>), dim3((unsigned)a.B),
                       dim3(128), c.lds, s, a);
}

// The fused launch at tile width CW, per-walk bounds or the shared form.  No next-round prefetch:
// at config 2 the fused launch ran 28.0–28.3 µs without it and 30.9–31.1 µs with it under the
// history launcher's rule (diagnostics build, three alternations, profiles/r9/fused/prefetch_ab.txt)
// — without the history staging ten workgroups fit a CU instead of eight, the batch takes fewer
// dispatch rounds, and the touched lines mostly compete with the walks' own loads.
template <int CW>
void launch_metrics(const MetChoice& c, hipStream_t s, const RolloutArgs& a, const MetArgs& mo) {
  if (c.kind == MetKind::SplitShared)
    hipLaunchKernelGGL((zmpc_rollout_metrics_splitd_kernel<CW, true>), dim3((unsigned)a.B),
                       dim3(128), c.lds, s, a, mo);
  else
    hipLaunchKernelGGL((zmpc_rollout_metrics_splitd_kernel<CW, false>), dim3((unsigned)a.B),
                       dim3(128), c.lds, s, a, mo);
}

#ifdef ZMPC_DIAG
// diagnostics: the phase stamps of the last launch to $ZMPC_ROLLOUT_TL ([B][5] u64)
void tl_write(const unsigned long long* tl, int64_t B, hipStream_t s, hipError_t e) {
  const char* path = getenv("ZMPC_ROLLOUT_TL");
  if (tl == nullptr || path == nullptr || e != hipSuccess) return;
  std::vector<unsigned long long> h((size_t)B * 5);
  (void)hipStreamSynchronize(s);
  (void)hipMemcpy(h.data(), tl, h.size() * 8, hipMemcpyDeviceToHost);
  if (FILE* f = fopen(path, "wb")) {
    fwrite(h.data(), 8, h.size(), f);
    fclose(f);
  }
}
#endif

}  // namespace

hipError_t zmpc_launch_rollout_unc(const zmpc_plan* p, const RolloutCall& rc, hipStream_t s,
                                   std::string* why) {
  const UncChoice c = choose_unc(p->N, rc.n, rc.bstride == 0, p->opt[ZMPC_OPT_ROLLOUT_KERNEL],
                                 p->opt[ZMPC_OPT_LONG_WALK], p->opt[ZMPC_OPT_CORRELATION]);
  if (c.kind == UncKind::Copy) {
    // no QP solve: the history is the initial state only
    hipError_t e = hipMemcpyAsync(rc.hist, rc.x0, 6 * sizeof(double) * (size_t)rc.B,
                                  hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return e;
    if (rc.status) return hipMemsetAsync(rc.status, 0, sizeof(int32_t) * rc.B, s);
    return hipSuccess;
  }
  RolloutArgs a = make_args(p, rc, c);
  a.hist = rc.hist;
  if (c.E) {
    a.fft_tw = reinterpret_cast<const double2*>(p->fft_tw);
    a.fft_g = reinterpret_cast<const double2*>(p->fft_g) + (c.P - kFftPmin);
  }
#ifdef ZMPC_DIAG
  static const int dbg = [] {
    const char* e = getenv("ZMPC_DEBUG_ROLLOUT");  // diagnostics build: ablation bits
    return e ? atoi(e) : 0;
  }();
  a.dbg = dbg;
  // diagnostics: per-walk phase stamps of the split and wide kernels, written to $ZMPC_ROLLOUT_TL after
  // every launch ([B][5] u64, wall_clock64 ticks)
  static unsigned long long* tl_buf = nullptr;
  static int64_t tl_cap = 0;
  if (getenv("ZMPC_ROLLOUT_TL") && rc.B > tl_cap) {
    if (tl_buf) (void)hipFree(tl_buf);
    tl_buf = nullptr;
    tl_cap = hipMalloc((void**)&tl_buf, (size_t)rc.B * 5 * 8) == hipSuccess ? rc.B : 0;
  }
  if (tl_buf && c.kind != UncKind::Chunk) {
    (void)hipMemsetAsync(tl_buf, 0, (size_t)rc.B * 5 * 8, s);
    a.tl = tl_buf;
  }
#endif
  return launch_with_shared_f(c.kind == UncKind::SplitShared, p, rc, s, a, [&] {
    hipError_t e = hipErrorInvalidValue;
    if (c.kind == UncKind::Wide || c.kind == UncKind::Chunk)
      e = zmpc_launch_rollout_long(c, &a, p->cus, s);
    else if (with_cw(c.cw, [&](auto C) { launch_unc<decltype(C)::value>(c, s, a, p->cus); }))
      e = hipGetLastError();
#ifdef ZMPC_DIAG
    tl_write(a.tl, rc.B, s, e);
#endif
    return e;
  });
}

// zmpc_rollout_metrics: the kernel by dispatch.h choose_unc_metrics (the caller has refused the
// shapes it does not take), then the launch.  rc.hist is unused.
hipError_t zmpc_launch_rollout_metrics(const zmpc_plan* p, const RolloutCall& rc,
                                       const int64_t* lengths, double* metrics, hipStream_t s) {
  const MetChoice c = choose_unc_metrics(p->N, rc.n, rc.bstride == 0,
                                         p->opt[ZMPC_OPT_ROLLOUT_KERNEL],
                                         p->opt[ZMPC_OPT_CORRELATION]);
  if (c.kind == MetKind::None) return hipErrorInvalidValue;
  RolloutArgs a = make_args(p, rc, c);
  const MetArgs mo{metrics, lengths, p->hg, sqrt(p->hg)};
  if (c.kind == MetKind::Sample0) {
    hipLaunchKernelGGL(zmpc_metrics_x0_kernel, dim3((unsigned)((2 * rc.B + 255) / 256)), dim3(256),
                       0, s, a, mo);
    return hipGetLastError();
  }
  return launch_with_shared_f(c.kind == MetKind::SplitShared, p, rc, s, a, [&] {
    const bool ok =
        with_cw(c.cw, [&](auto C) { launch_metrics<decltype(C)::value>(c, s, a, mo); });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
  });
}

hipError_t zmpc_launch_step_unc(const zmpc_plan* p, const StepCall& c, hipStream_t s) {
  hipLaunchKernelGGL(zmpc_step_unc_kernel, dim3((unsigned)((c.B + 3) / 4)), dim3(256), 0, s, c.B,
                     p->N, p->lc, p->k, p->kx, c.x, c.zmax_win, c.zmin_win, c.x_next, c.status);
  return hipGetLastError();
}

// The dynamic-LDS ceiling must be raised once per device for > 64 KiB requests: the one-wave
// kernel here, the chunk and 8-wave wide kernels in rollout_long.hip (the split kernels stay
// within the default 64 KiB).
hipError_t zmpc_rollout_unc_set_attrs() {
  hipError_t e = hipSuccess;
#define ZMPC_ATTR(C)                                                                        \
  if (e == hipSuccess)                                                                      \
    e = hipFuncSetAttribute((const void*)zmpc_rollout_unc_kernel<C>,                       \
                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  ZMPC_ATTR(1) ZMPC_ATTR(2) ZMPC_ATTR(3) ZMPC_ATTR(4) ZMPC_ATTR(5) ZMPC_ATTR(6) ZMPC_ATTR(7)
  ZMPC_ATTR(8)
#undef ZMPC_ATTR
  return e == hipSuccess ? zmpc_rollout_long_set_attrs() : e;
}
