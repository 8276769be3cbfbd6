// zmpc_trace_margin: the exact critical scale of a per-walk disturbance trace, K draws per walk
// (include/zmpc.h, "The trace margin, stated once").
//
// The closed loop of the unconstrained controller is linear and time-invariant, so under λ times
// a trace the ZMP of sample i is z0_i + λ·ρ_i with ρ the ZMP image of the trace's state response at
// λ = 1, ρ_i = −(δ_i[0] − (h/g)·δ_i[2]), and δ the recurrence trace.hip scans.  The largest λ that
// keeps every sample inside is a minimum of quotients, zmpc_push_map's argument with a response per
// row instead of one table per batch:
//     scale[r, 0] = min over s < i < n_b and the requested axes of
//                   (ρ > 0 ? up_i/ρ : ρ < 0 ? dn_i/(−ρ) : +inf),   scale[r, 1]: up and dn swapped.
//   - one wavefront per row r = (walk b = r / K, draw), kTraceWaves rows per workgroup: the draws
//     of a walk sit in consecutive waves and re-read its history from cache;
//   - the wave first takes the samples at or before the start step, 64 at a time, for the nominal
//     test alone; then blocks of 64 samples from s + 1 on with trace_scan.h's scan, lane l the
//     sample s + 1 + 64k + l.  A block's state and bound loads and the next block's dv load are
//     issued before the scan, so one memory latency per block hides under its arithmetic;
//   - each lane loads its own sample, three 16-byte pairs and two pairs of bounds: nothing is
//     stored per sample, so trace.hip's pair gather has no use here;
//   - the six powers Ā^(2^r) live in LDS, one copy per workgroup that its first thread writes (432
//     bytes, read at wave-uniform addresses); the lane's Ā^(l+1) stays in registers;
//   - each lane keeps a running (value, index) minimum per column, index 2·i + a, replaced on
//     strict < over ascending (i, a); the wave reduces lexicographically on (value, index), so
//     the result does not depend on the order of the reduction.  Lane 0 writes the row: one
//     16-byte store of the two scales, one 8-byte store of the two indices.
// No candidate is formed from ρ = 0 (an all-zero trace gives ρ = −0), none from a NaN ρ, and the
// quotient is the IEEE division, so a sample on its bound with t = 0 gives exactly 0.  No index
// depends on a value of dv.  Every sum runs in trace_scan.h's order, uncontracted: two calls agree
// bit for bit, and a row gives the same bits alone, in any batch and among any number of draws.
#include "trace_scan.h"

namespace {

#pragma clang fp contract(off)

struct tipair_t {
  int32_t x, y;
};

// (value, index) minimum across two lanes, the lower index on a tie (−1, no sample, loses as
// unsigned): symmetric, so every lane ends with the same pair
__device__ __forceinline__ void margin_min_lanes(double& f, int& i, int mask) {
  const double o = __shfl_xor(f, mask);
  const int j = __shfl_xor(i, mask);
  if (o < f || (o == f && (unsigned)j < (unsigned)i)) {
    f = o;
    i = j;
  }
}

// The two candidates of one (sample, axis): up, dn the margins, rho the response at λ = 1
__device__ __forceinline__ void margin_cand(double up, double dn, double rho, int idx, double f[2],
                                            int ix[2]) {
  if (rho > 0.0 || rho < 0.0) {
    const bool pos = rho > 0.0;
    const double ra = pos ? rho : -rho;
    const double c0 = (pos ? up : dn) / ra;
    const double c1 = (pos ? dn : up) / ra;
    if (c0 < f[0]) {
      f[0] = c0;
      ix[0] = idx;
    }
    if (c1 < f[1]) {
      f[1] = c1;
      ix[1] = idx;
    }
  }
}

// One sample of a walk as the lanes load it: (c, ċ)x (c̈x, cy) (ċ, c̈)y and the bounds (x, y)
struct MSample {
  tpair_t s0, s1, s2, hi, lo;
};

__device__ __forceinline__ MSample margin_load(const tpair_t* __restrict__ h,
                                               const tpair_t* __restrict__ hi,
                                               const tpair_t* __restrict__ lo, int64_t i) {
  MSample m;
  m.s0 = h[3 * i];
  m.s1 = h[3 * i + 1];
  m.s2 = h[3 * i + 2];
  m.hi = hi[i];
  m.lo = lo[i];
  return m;
}

// The nominal test of metrics.hip / pushmap.hip on one sample (a non-finite state value, or a
// violation above t on either axis); z receives the uncontracted ZMP (x, y)
__device__ __forceinline__ bool margin_bad(const MSample& m, double hg, double t, double z[2]) {
  const bool fin = isfinite(m.s0.x) && isfinite(m.s0.y) && isfinite(m.s1.x) && isfinite(m.s1.y) &&
                   isfinite(m.s2.x) && isfinite(m.s2.y);
  z[0] = m.s0.x - hg * m.s1.x;
  z[1] = m.s1.y - hg * m.s2.y;
  const double vx = fmax(fmax(z[0] - m.hi.x, m.lo.x - z[0]), 0.0);
  const double vy = fmax(fmax(z[1] - m.hi.y, m.lo.y - z[1]), 0.0);
  return !fin || vx > t || vy > t;
}

// R = B·K rows; cx, cy: the column of an axis in dv, −1 for an axis that is not requested; L: the
// samples of a row's trace, `cols` doubles each.
__global__ void __launch_bounds__(64 * kTraceWaves)
zmpc_trace_margin_kernel(int64_t R, int64_t K, int64_t n, const double* __restrict__ kx, double T,
                         double T2_2, double T3_6, double hg, double t,
                         const double* __restrict__ hist, const double* __restrict__ zmax,
                         const double* __restrict__ zmin, int64_t bstride,
                         const int64_t* __restrict__ lengths, const double* __restrict__ dv,
                         int cols, int cx, int cy, const int64_t* __restrict__ steps, int64_t step,
                         int64_t L, double* __restrict__ scale, int32_t* __restrict__ limit) {
  __shared__ TMat3 sP[6];  // Ā^(2^r), one copy per workgroup, written by its first thread
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kTraceWaves + (threadIdx.x >> 6);
  TMat3 Q;
  trace_propagators(trace_closed_loop(kx, T, T2_2, T3_6), lane,
                    [&](int k, const TMat3& m) {
                      if (threadIdx.x == 0) sP[k] = m;
                    },
                    Q);
  __syncthreads();
  if (r >= R) return;  // whole waves leave: the shuffles below see 64 live lanes
  const int64_t b = r / K;
  int64_t nb = lengths ? lengths[b] : n;
  nb = nb < 1 ? 1 : (nb > n ? n : nb);
  int64_t s = steps ? steps[r] : step;
  if (s < 0 || s >= nb - 1) s = nb - 1;  // the trace reaches no sample: the nominal test alone

  const tpair_t* h = reinterpret_cast<const tpair_t*>(hist + b * n * 6);
  const tpair_t* hi = reinterpret_cast<const tpair_t*>(zmax + b * bstride);
  const tpair_t* lo = reinterpret_cast<const tpair_t*>(zmin + b * bstride);
  const double inf = __builtin_inf();
  double f[2] = {inf, inf};
  int ix[2] = {-1, -1};
  bool bad = false;

  const int64_t first = s + 1;              // the first sample the trace moves, <= n_b
  const int64_t live = nb - first;          // samples first .. n_b − 1
  const int64_t nin = L < live ? L : live;  // trace entries that reach a sample
  const double* dw = dv + r * L * (int64_t)cols;

  // the input that makes δ of sample first + j out of its predecessor's
  auto input = [&](int64_t j, double& ux, double& uy) {
    ux = 0.0;
    uy = 0.0;
    if (j < nin) {
      if (cols == 2) {
        const tpair_t u = *reinterpret_cast<const tpair_t*>(dw + 2 * j);
        ux = u.x;
        uy = u.y;
      } else if (cx >= 0) {
        ux = dw[j];
      } else {
        uy = dw[j];
      }
    }
  };
  double ux, uy;
  input(lane, ux, uy);  // the first block's, under the loop below

  // samples 0 .. s: the nominal test alone
  for (int64_t i = lane; i < first; i += 64) {
    double z[2];
    bad |= margin_bad(margin_load(h, hi, lo, i), hg, t, z);
  }

  double carry[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};  // δ of the sample before the block
  for (int64_t base = 0; base < live; base += 64) {
    const int64_t j = base + lane;
    const bool on = j < live;
    // the lane's sample (the walk's last one for a lane past the end: loaded, not used), and the
    // next block's input, all in flight under the scan
    const MSample m = margin_load(h, hi, lo, on ? first + j : nb - 1);
    double v[2][3] = {{0.0, ux, 0.0}, {0.0, uy, 0.0}};
    input(j + 64, ux, uy);
    // (the powers are read from LDS in every block: hoisted out of the loop they would take
    // 108 registers, which is what trace.hip pays for them)
    asm volatile("" ::: "memory");
    trace_block_scan(sP, Q, lane, carry, v);
    if (on) {
      double z[2];
      bad |= margin_bad(m, hg, t, z);
      const int idx = 2 * (int)(first + j);  // (n <= 2^24)
      if (cx >= 0) {
        const double rho = -(v[0][0] - hg * v[0][2]);
        margin_cand((m.hi.x - z[0]) + t, (z[0] - m.lo.x) + t, rho, idx, f, ix);
      }
      if (cy >= 0) {
        const double rho = -(v[1][0] - hg * v[1][2]);
        margin_cand((m.hi.y - z[1]) + t, (z[1] - m.lo.y) + t, rho, idx + 1, f, ix);
      }
    }
  }

#pragma unroll
  for (int mask = 1; mask < 64; mask <<= 1) {
    margin_min_lanes(f[0], ix[0], mask);
    margin_min_lanes(f[1], ix[1], mask);
  }
  const bool fail = __any(bad);
  if (lane == 0) {
    const double nan = __builtin_nan("");
    reinterpret_cast<tpair_t*>(scale)[r] = fail ? tpair_t{nan, nan} : tpair_t{f[0], f[1]};
    if (limit) reinterpret_cast<tipair_t*>(limit)[r] = fail ? tipair_t{-1, -1} : tipair_t{ix[0], ix[1]};
  }
}

}  // namespace

hipError_t zmpc_launch_trace_margin(const zmpc_plan* p, const MarginCall& c, hipStream_t s) {
  const int64_t R = c.B * c.draws;
  if (R < 1) return hipSuccess;
  const unsigned grid = (unsigned)((R + kTraceWaves - 1) / kTraceWaves);
  hipLaunchKernelGGL(zmpc_trace_margin_kernel, dim3(grid), dim3(64 * kTraceWaves), 0, s, R, c.draws,
                     c.n, p->kx, p->T, p->T2_2, p->T3_6, p->hg, c.t, c.hist, c.zmax, c.zmin,
                     c.bstride, c.lengths, c.push.amp, c.push.cols, c.push.col[0], c.push.col[1],
                     c.push.steps, c.push.step, c.L, c.scale, c.limit);
  return hipGetLastError();
}
