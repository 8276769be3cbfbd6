// Push-robustness map of an unpushed walk (include/zmpc.h zmpc_push_map): the exact critical push
// of every (walk, push step, direction), from the state history alone.  The closed loop of the
// unconstrained controller is linear and time-invariant, x⁺ = Ā x + B f with Ā = A − B·kxᵀ and f
// independent of the state, so the y-axis ZMP response at sample i to a unit push at step s
// depends on the delay d = i − s alone:
//     r_d = −(dt/m)·C·Ā^(d−1)·e1  (d ≥ 1),  C = (1, 0, −h/g),  r_0 = 0
// (a push of +F at step s lowers the y velocity of sample s + 1 by dt·F/m, zmp_controller.py:
// 105-106; r_1 is exactly 0).  With the margins up_i = (zmax_i − z0_i) + t, dn_i = (z0_i − zmin_i)
// + t of the unpushed ZMP z0 = c − (h/g)·c̈ the largest push that keeps every sample inside is
//     F[b, s, +] = min over s < i < n_b of (r_d > 0 ? up_i/r_d : r_d < 0 ? dn_i/(−r_d) : +inf)
// and F[b, s, −] the same with up and dn swapped: a (min, ×) correlation of the margins with the
// reciprocal response, n_b²/2 (sample, step) pairs per walk and direction.
//
// Three kernels.  zmpc_push_response_kernel (one wave, once per launch) fills the table r_d and
// q_d = 1/|r_d|.  zmpc_push_map_kernel is the hot path: one workgroup per walk streams the history
// once (coalesced 16-byte loads as metrics.hip), runs the nominal test on both axes and leaves
// the (up_i, dn_i) pairs in LDS; then lanes own push steps and the loop runs over the delay d, so
// r_d, q_d and the sign of r_d are wave-uniform (scalar loads, a uniform branch) and consecutive
// lanes read consecutive 16-byte LDS pairs.  A pair costs two multiplies, two compares and six
// 32-bit selects.  64 pairs of +inf behind the walk's samples stand for "no sample": inf·q = inf never
// wins a strict <, so the loop carries no bounds predicate.  The triangular trip count is balanced
// across waves: a wave takes 64-step block k and block K − 1 − k in turn.  The loop visits samples
// in ascending order and replaces on strict <, so a tie keeps the lower sample index, and two
// launches agree bit for bit.  zmpc_push_step_kernel is the single-step form, one wave per walk
// with lanes over samples and a min-butterfly as metrics.hip MetAcc; it forms the same candidates
// (push_cand), and a minimum does not depend on the order it is taken in, so its forces are the
// full map's rows bit for bit.
//
// Guards: a candidate is never formed from r_d = 0; where q_d is not a positive normal number
// (|r_d| denormal or non-finite) the candidate is the division x/|r_d| itself, so no 0·inf is
// formed and a sample exactly on its bound with t = 0 gives F = 0.
//
// zmpc_push_map_shaped (pushshaped.hip) shapes the table for pushes that last several samples and
// adds the x axis; its y-only launches run the map and step kernels here on the shaped table
// (zmpc_push_base_table, zmpc_push_map_on_table below).
#include "push_common.h"
#include "zmpc_internal.h"

namespace {

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------
// Response table: tab[d] = (r_d, q_d = 1/|r_d|) (q_d = 0 where r_d = 0), one 16-byte scalar load
// per delay; resp (may be null) receives r_d.  Lane l holds v = Ā^l e1 (l products), M = Ā^64 comes from six
// squarings, and every further row of 64 delays is one product with M: 63 + 6·3 + n/64 dependent
// 3-vector products instead of n.
struct Mat3 {
  double a[9];
};

__device__ __forceinline__ void matvec(const Mat3& m, double v[3]) {
  const double x = m.a[0] * v[0] + m.a[1] * v[1] + m.a[2] * v[2];
  const double y = m.a[3] * v[0] + m.a[4] * v[1] + m.a[5] * v[2];
  const double z = m.a[6] * v[0] + m.a[7] * v[1] + m.a[8] * v[2];
  v[0] = x;
  v[1] = y;
  v[2] = z;
}

__global__ void __launch_bounds__(64)
zmpc_push_response_kernel(int64_t n, const double* __restrict__ kx, double T, double T2_2,
                          double T3_6, double hg, double dtm, pair_t* __restrict__ tab,
                          double* __restrict__ resp) {
  const int lane = threadIdx.x;
  const double k0 = kx[0], k1 = kx[1], k2 = kx[2];
  Mat3 A;  // Ā = A − B·kxᵀ
  A.a[0] = 1.0 - T3_6 * k0;
  A.a[1] = T - T3_6 * k1;
  A.a[2] = T2_2 - T3_6 * k2;
  A.a[3] = 0.0 - T2_2 * k0;
  A.a[4] = 1.0 - T2_2 * k1;
  A.a[5] = T - T2_2 * k2;
  A.a[6] = 0.0 - T * k0;
  A.a[7] = 0.0 - T * k1;
  A.a[8] = 1.0 - T * k2;
  double v[3] = {0.0, 1.0, 0.0};
  for (int l = 0; l < lane; ++l) matvec(A, v);
  Mat3 M = A;
  for (int r = 0; r < 6; ++r) {
    Mat3 S;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        S.a[3 * i + j] =
            M.a[3 * i] * M.a[j] + M.a[3 * i + 1] * M.a[3 + j] + M.a[3 * i + 2] * M.a[6 + j];
    M = S;
  }
  if (lane == 0) {
    tab[0] = pair_t{0.0, 0.0};
    if (resp) resp[0] = 0.0;
  }
  for (int64_t d = 1 + lane; d < n; d += 64) {
    // d = 1: C·e1 = 0 exactly
    const double r = d == 1 ? 0.0 : -dtm * (v[0] - hg * v[2]);
    tab[d] = pair_t{r, r == 0.0 ? 0.0 : 1.0 / fabs(r)};
    if (resp) resp[d] = r;
    matvec(M, v);
  }
}

// ---------------------------------------------------------------------------------------------
// One sample of a walk: its y-axis margins, and whether it fails the nominal test (a non-finite
// state value, or a violation above t on either axis — the test of metrics.hip AxisAcc::add)
struct Sample {
  double up, dn;
  bool bad;
};

__device__ __forceinline__ Sample push_sample(const pair_t* __restrict__ h,
                                              const pair_t* __restrict__ hi,
                                              const pair_t* __restrict__ lo, int64_t i, double hg,
                                              double t) {
  const pair_t s0 = h[3 * i], s1 = h[3 * i + 1], s2 = h[3 * i + 2];  // (c,ċ | c̈,c | ċ,c̈)
  const pair_t u = hi[i], l = lo[i];
  Sample s;
  s.bad = !(isfinite(s0.x) && isfinite(s0.y) && isfinite(s1.x) && isfinite(s1.y) &&
            isfinite(s2.x) && isfinite(s2.y));
  const double zx = s0.x - hg * s1.x;
  const double zy = s1.y - hg * s2.y;
  const double vx = fmax(fmax(zx - u.x, l.x - zx), 0.0);
  const double vy = fmax(fmax(zy - u.y, l.y - zy), 0.0);
  s.bad = s.bad || vx > t || vy > t;
  s.up = (u.y - zy) + t;
  s.dn = (zy - l.y) + t;
  return s;
}

__global__ void __launch_bounds__(1024)
zmpc_push_map_kernel(int64_t n, const double* __restrict__ hist, const double* __restrict__ zmax,
                     const double* __restrict__ zmin, int64_t bstride,
                     const int64_t* __restrict__ lengths, double hg, double t,
                     const pair_t* __restrict__ tab, double* __restrict__ force,
                     int32_t* __restrict__ limit) {
  extern __shared__ pair_t m[];  // [n + 64]
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  int64_t nb = lengths ? lengths[b] : n;
  nb = nb < 1 ? 1 : (nb > n ? n : nb);
  const pair_t* h = reinterpret_cast<const pair_t*>(hist + b * n * 6);
  const pair_t* hi = reinterpret_cast<const pair_t*>(zmax + b * bstride);
  const pair_t* lo = reinterpret_cast<const pair_t*>(zmin + b * bstride);
  int bad = 0;
  const double inf = __builtin_inf();
  for (int64_t i = threadIdx.x; i < nb + 64; i += blockDim.x) {
    pair_t p{inf, inf};
    if (i < nb) {
      const Sample s = push_sample(h, hi, lo, i, hg, t);
      bad |= s.bad;
      p.x = s.up;
      p.y = s.dn;
    }
    m[i] = p;
  }
  bad = __syncthreads_or(bad);  // (also orders the LDS stores before the reads below)
  pair_t* fo = reinterpret_cast<pair_t*>(force + b * n * 2);
  ipair_t* li = limit ? reinterpret_cast<ipair_t*>(limit + b * n * 2) : nullptr;
  const int nblk = (int)((n + 63) >> 6);
  // a wave takes the blocks k = wave, wave + nwaves, … of the first half, each followed by its
  // mirror nblk − 1 − k: long and short trip counts alternate
  for (int k = wave; 2 * k < nblk; k += nwaves) {
    for (int half = 0; half < 2; ++half) {
      const int blk = half ? nblk - 1 - k : k;
      if (half && blk == k) break;
      const int s0 = blk << 6, s = s0 + lane;
      double f0 = inf, f1 = inf;
      int i0 = -1, i1 = -1;
      if (!bad) {
        // delays 1 … n_b − 1 − s0 (lane 0's; the later lanes run into the +inf pairs), four to
        // a trip so that the scalar loads of the table and the LDS reads go out together
        const int dmax = (int)nb - 1 - s0;
        auto one = [&](int d, const pair_t rq, const pair_t mi) {
          const double r = rq.x, q = rq.y;
          if (r == 0.0) return;
          // wave-uniform branches: the division is only ever issued for a denormal or non-finite
          // response.  (Deciding them on the bit patterns with scalar integer instructions, and
          // tracking the uniform delay instead of the sample, measured 16 % slower.)
          if (q >= 0x1p-1022 && q < inf) {
            if (r > 0.0)
              push_pair<true>(mi, s + d, q, fabs(r), true, f0, f1, i0, i1);
            else
              push_pair<false>(mi, s + d, q, fabs(r), true, f0, f1, i0, i1);
          } else {
            if (r > 0.0)
              push_pair<true>(mi, s + d, q, fabs(r), false, f0, f1, i0, i1);
            else
              push_pair<false>(mi, s + d, q, fabs(r), false, f0, f1, i0, i1);
          }
        };
        int d = 1;
        for (; d + 3 <= dmax; d += 4) {
          const pair_t t0 = tab[d], t1 = tab[d + 1], t2 = tab[d + 2], t3 = tab[d + 3];
          const pair_t m0 = m[s + d], m1 = m[s + d + 1], m2 = m[s + d + 2], m3 = m[s + d + 3];
          one(d, t0, m0);
          one(d + 1, t1, m1);
          one(d + 2, t2, m2);
          one(d + 3, t3, m3);
        }
        for (; d <= dmax; ++d) one(d, tab[d], m[s + d]);
      } else {
        f0 = f1 = __builtin_nan("");
      }
      if (s < n) {
        fo[s] = pair_t{f0, f1};
        if (li) li[s] = ipair_t{i0, i1};
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Single-step form: one wave per walk, four walks per workgroup (kStepWaves), lanes over samples.
__global__ void __launch_bounds__(64 * kStepWaves)
zmpc_push_step_kernel(int64_t B, int64_t n, const double* __restrict__ hist,
                      const double* __restrict__ zmax, const double* __restrict__ zmin,
                      int64_t bstride, const int64_t* __restrict__ lengths,
                      const int64_t* __restrict__ steps, double hg, double t,
                      const pair_t* __restrict__ tab, double* __restrict__ force,
                      int32_t* __restrict__ limit) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * kStepWaves + (threadIdx.x >> 6);
  if (b >= B) return;  // whole waves leave: the shuffles below see 64 live lanes
  int64_t nb = lengths ? lengths[b] : n;
  nb = nb < 1 ? 1 : (nb > n ? n : nb);
  int64_t s = steps[b];
  if (s < 0 || s >= nb - 2) s = nb;  // outside [0, n_b − 2): no sample lies behind it
  const pair_t* h = reinterpret_cast<const pair_t*>(hist + b * n * 6);
  const pair_t* hi = reinterpret_cast<const pair_t*>(zmax + b * bstride);
  const pair_t* lo = reinterpret_cast<const pair_t*>(zmin + b * bstride);
  const double inf = __builtin_inf();
  double f0 = inf, f1 = inf;
  int i0 = -1, i1 = -1;
  int bad = 0;
  for (int64_t i = lane; i < nb; i += 64) {
    const Sample sm = push_sample(h, hi, lo, i, hg, t);
    bad |= sm.bad;
    if (i > s) {
      const pair_t rq = tab[i - s];
      const double r = rq.x;
      if (r != 0.0) {
        const double q = rq.y, ra = fabs(r);
        const bool fast = q >= 0x1p-1022 && q < inf;  // a positive normal number, as the map
        const pair_t mi{sm.up, sm.dn};
        if (r > 0.0)
          push_pair<true>(mi, (int)i, q, ra, fast, f0, f1, i0, i1);
        else
          push_pair<false>(mi, (int)i, q, ra, fast, f0, f1, i0, i1);
      }
    }
  }
  // min-butterfly, the lower index on a tie (symmetric in the two lanes: all end with the same)
#pragma unroll
  for (int mask = 1; mask < 64; mask <<= 1) {
    const double o0 = __shfl_xor(f0, mask), o1 = __shfl_xor(f1, mask);
    const int j0 = __shfl_xor(i0, mask), j1 = __shfl_xor(i1, mask);
    if (o0 < f0 || (o0 == f0 && (unsigned)j0 < (unsigned)i0)) {
      f0 = o0;
      i0 = j0;
    }
    if (o1 < f1 || (o1 == f1 && (unsigned)j1 < (unsigned)i1)) {
      f1 = o1;
      i1 = j1;
    }
    bad |= __shfl_xor(bad, mask);
  }
  if (bad) {
    f0 = f1 = __builtin_nan("");
    i0 = i1 = -1;
  }
  if (lane < 2) {
    force[b * 2 + lane] = lane ? f1 : f0;
    if (limit) limit[b * 2 + lane] = lane ? i1 : i0;
  }
}

}  // namespace

hipError_t zmpc_push_map_set_attrs() {
  const hipError_t e =
      hipFuncSetAttribute((const void*)zmpc_push_map_kernel,
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPushMapLdsCap);
  return e != hipSuccess ? e : zmpc_push_shaped_set_attrs();
}

void zmpc_push_base_table(const zmpc_plan* p, int64_t n, double mass, void* tab, double* response,
                          hipStream_t s) {
  hipLaunchKernelGGL(zmpc_push_response_kernel, dim3(1), dim3(64), 0, s, n, p->kx, p->T, p->T2_2,
                     p->T3_6, p->hg, p->T / mass, static_cast<pair_t*>(tab), response);
}

void zmpc_push_map_on_table(const zmpc_plan* p, int64_t B, int64_t n, const double* hist,
                            const double* zmax, const double* zmin, int64_t bstride,
                            const int64_t* lengths, const int64_t* push_steps, double t,
                            const void* table, double* force, int32_t* limit, hipStream_t s) {
  const PushMapChoice c = choose_push_map(n, push_steps != nullptr);
  const pair_t* tab = static_cast<const pair_t*>(table);
  if (push_steps) {
    const unsigned grid = (unsigned)((B + kStepWaves - 1) / kStepWaves);
    hipLaunchKernelGGL(zmpc_push_step_kernel, dim3(grid), dim3(64 * kStepWaves), 0, s, B, n, hist,
                       zmax, zmin, bstride, lengths, push_steps, p->hg, t, tab, force, limit);
  } else {
    hipLaunchKernelGGL(zmpc_push_map_kernel, dim3((unsigned)B), dim3(64 * c.waves), c.lds, s, n,
                       hist, zmax, zmin, bstride, lengths, p->hg, t, tab, force, limit);
  }
}

hipError_t zmpc_launch_push_map(const zmpc_plan* p, int64_t B, int64_t n, const double* hist,
                                const double* zmax, const double* zmin, int64_t bstride,
                                const int64_t* lengths, const int64_t* push_steps, double t,
                                double mass, double* force, int32_t* limit, double* response,
                                hipStream_t s) {
  // the response table of this n, recomputed per launch into a stream-ordered workspace (a plan
  // is shared by threads and streams, each with an n of its own)
  pair_t* tab = nullptr;
  hipError_t e = hipMallocAsync((void**)&tab, (size_t)n * sizeof(pair_t), s);
  if (e != hipSuccess) return hipErrorOutOfMemory;
  zmpc_push_base_table(p, n, mass, tab, response, s);
  if (B > 0)
    zmpc_push_map_on_table(p, B, n, hist, zmax, zmin, bstride, lengths, push_steps, t, tab, force,
                           limit, s);
  e = hipGetLastError();
  const hipError_t ef = hipFreeAsync(tab, s);
  return e != hipSuccess ? e : ef;
}
