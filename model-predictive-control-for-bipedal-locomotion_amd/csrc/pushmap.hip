// Push-robustness maps of an unpushed walk (include/zmpc.h zmpc_push_map, zmpc_push_map_shaped):
// the exact critical push of every (walk, push step, axis, direction), from the state history
// alone.  The closed loop of the unconstrained controller is linear and time-invariant, x⁺ = Ā x
// + B f with Ā = A − B·kxᵀ and f independent of the state, so the ZMP response at sample i to a
// unit one-sample push at step s depends on the delay d = i − s alone, and is the same on both axes:
//     r_d = −(dt/m)·C·Ā^(d−1)·e1  (d ≥ 1),  C = (1, 0, −h/g),  r_0 = 0
// (a push of +F at step s lowers the velocity of sample s + 1 by dt·F/m, zmp_controller.py:
// 105-106; r_1 is exactly 0).  A push with force profile F·w_j during steps s + j, j < D, is a sum
// of one-sample pushes: R_d = Σ_{j = 0}^{min(D−1, d)} w_j·r_{d−j}.  With the margins up_i = (zmax_i
// − z0_i) + t, dn_i = (z0_i − zmin_i) + t of the unpushed ZMP z0 = c − (h/g)·c̈ of an axis, the
// largest push that keeps every sample inside is
//     F[b, s, +] = min over s < i < n_b of (R_d > 0 ? up_i/R_d : R_d < 0 ? dn_i/(−R_d) : +inf)
// and F[b, s, −] the same with up and dn swapped: a (min, ×) correlation of the margins with the
// reciprocal response, n_b²/2 (sample, step) pairs per walk, axis and direction.
//
// Four kernels.  zmpc_push_response_kernel (one wave, once per launch) fills the table r_d and
// q_d = 1/|r_d|; zmpc_push_shape_kernel turns it into that of a D-sample push (skipped at D = 1
// without a profile).  zmpc_push_map_kernel<NAX> is the hot path, over NAX = 1 or 2 axes: one
// workgroup per walk streams the history (coalesced 16-byte loads as metrics.hip), runs the nominal
// test on both axes and leaves an axis' (up_i, dn_i) pairs in LDS; then lanes own push steps and the
// loop runs over the delay d, so r_d, q_d and the sign of r_d are wave-uniform (scalar loads, a
// uniform branch) and consecutive lanes read consecutive 16-byte LDS pairs.  A pair costs two
// multiplies, two compares and six 32-bit selects.  64 pairs of +inf behind the walk's samples
// stand for "no sample": inf·q = inf never wins a strict <, so the loop carries no bounds predicate.
// The triangular trip count is balanced across waves: a wave takes 64-step block k and block
// K − 1 − k in turn.  Two axes take turns over the same LDS.  zmpc_push_step_kernel<AXES> is the
// single-step form, one wave per walk with lanes over samples and a min-butterfly as metrics.hip
// MetAcc.
//
// The same unit serves zmpc_rollout_pushed on unconstrained plans (the push itself rolled out): the
// response kernel also emits the state response Ā^(d−1)·e1, zmpc_push_state_shape_kernel sums it
// over a push window and zmpc_push_add_kernel streams it onto an unpushed history (further down).
//
// What makes every form agree with every other bit for bit (two axes with one axis column for
// column, the single-step form with the map's rows, a launch with its repetition):
//   - all candidates come from push_cand and push_pair, uncontracted (fp contract off);
//   - a candidate is never formed from r_d = 0, and where q_d is not a positive normal number
//     (|r_d| denormal or non-finite) it is the division x/|r_d| itself, so no 0·inf is formed and a
//     sample exactly on its bound with t = 0 gives F = 0;
//   - the map visits samples in ascending order and replaces on strict <, so a tie keeps the
//     lower sample index; the butterfly keeps the lower index on a tie, and a minimum does not
//     depend on the order it is taken in.
#include "zmpc_internal.h"

namespace {

#pragma clang fp contract(off)

struct pair_t {
  double x, y;
};

struct ipair_t {
  int32_t x, y;
};

// Walks per workgroup of the single-step kernel (one wave each)
constexpr int kStepWaves = 4;
// Delays per workgroup of the shaping kernels
constexpr int kShapeThreads = 256;

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

//
// vec (may be null, as may tab) receives the state response itself for zmpc_rollout_pushed: vec[d]
// = (Ā^(d−1)·e1, 0) as two 16-byte pairs, vec[0] = 0 — the same per-lane powers and squarings.
__global__ void __launch_bounds__(64)
zmpc_push_response_kernel(int64_t n, const double* __restrict__ kx, double T, double T2_2,
                          double T3_6, double hg, double dtm, pair_t* __restrict__ tab,
                          double* __restrict__ resp, pair_t* __restrict__ vec) {
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
    if (tab) tab[0] = pair_t{0.0, 0.0};
    if (resp) resp[0] = 0.0;
    if (vec) vec[0] = vec[1] = pair_t{0.0, 0.0};
  }
  for (int64_t d = 1 + lane; d < n; d += 64) {
    // d = 1: C·e1 = 0 exactly
    const double r = d == 1 ? 0.0 : -dtm * (v[0] - hg * v[2]);
    if (tab) tab[d] = pair_t{r, r == 0.0 ? 0.0 : 1.0 / fabs(r)};
    if (resp) resp[d] = r;
    if (vec) {
      vec[2 * d] = pair_t{v[0], v[1]};
      vec[2 * d + 1] = pair_t{v[2], 0.0};
    }
    matvec(M, v);
  }
}

// ---------------------------------------------------------------------------------------------
// zmpc_rollout_pushed on an unconstrained plan: the closed loop is linear and time-invariant, so
// the pushed history is the unpushed one plus the state response of the window,
//     hist[b, s_b + d, a, :] −= amp[b, a]·S_d,   S_d = Σ_{j = 0}^{min(D−1, d−1)} w_j·Ā^(d−j−1)·e1
// for d >= 1 (the velocity of sample s + j + 1 is lowered by amp·w_j and travels on under Ā).
//
// Shaping: S_d from the table vec of the response kernel, a grid over delays as
// zmpc_push_shape_kernel (the weight wave-uniform, ascending j, no product without a profile).
__global__ void __launch_bounds__(kShapeThreads)
zmpc_push_state_shape_kernel(int64_t n, const pair_t* __restrict__ vec,
                             const double* __restrict__ w, int64_t D, pair_t* __restrict__ out) {
  const int64_t d = (int64_t)blockIdx.x * kShapeThreads + threadIdx.x;
  const int64_t dwave = __builtin_amdgcn_readfirstlane((int)(d | 63));
  const int64_t dlast = dwave < n - 1 ? dwave : n - 1;
  const int64_t jend = D - 1 < dlast - 1 ? D - 1 : dlast - 1;
  const bool live = d < n;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int64_t j = 0; j <= jend; ++j) {
    const double wj = w ? w[j] : 1.0;
    if (live && j < d) {
      const pair_t p = vec[2 * (d - j)], q = vec[2 * (d - j) + 1];
      a0 += w ? wj * p.x : p.x;
      a1 += w ? wj * p.y : p.y;
      a2 += w ? wj * q.x : q.x;
    }
  }
  if (live) {
    out[2 * d] = pair_t{a0, a1};
    out[2 * d + 1] = pair_t{a2, 0.0};
  }
}

// Adding: a walk's history is 3n 16-byte pairs, (c, ċ)x (c̈x, cy) (ċ, c̈)y per sample; consecutive
// lanes take consecutive pairs from the first pushed sample s_b + 1 on (one coalesced 16-byte load
// and store each; the table's 32 bytes per delay come from cache).  The workgroups of a walk
// stride over its pairs; a walk whose start step lies outside [0, n − 1) is left alone, and a pair
// no pushed axis reaches is neither read nor written.  cx, cy: the column of an axis in amp, −1
// for an axis that is not pushed.
constexpr int kAddThreads = 256;

__global__ void __launch_bounds__(kAddThreads)
zmpc_push_add_kernel(int64_t n, int chunks, const double* __restrict__ amp, int cols, int cx,
                     int cy, const int64_t* __restrict__ steps, int64_t step,
                     const pair_t* __restrict__ S, double* __restrict__ hist) {
  const int64_t b = blockIdx.x / (unsigned)chunks;
  const int chunk = (int)(blockIdx.x % (unsigned)chunks);
  const int64_t s = steps ? steps[b] : step;
  if (s < 0 || s >= n - 1) return;
  const double ax = cx >= 0 ? amp[b * cols + cx] : 0.0;
  const double ay = cy >= 0 ? amp[b * cols + cy] : 0.0;
  pair_t* h = reinterpret_cast<pair_t*>(hist + b * n * 6);
  const int p0 = 3 * ((int)s + 1), p1 = 3 * (int)n;  // (n <= 2^24)
  for (int p = p0 + chunk * kAddThreads + (int)threadIdx.x; p < p1; p += chunks * kAddThreads) {
    const int i = p / 3, m = p - 3 * i;
    if ((m == 0 && cx < 0) || (m == 2 && cy < 0)) continue;
    const int d = i - (int)s;
    const pair_t u = S[2 * d], v = S[2 * d + 1];  // (S0, S1), (S2, 0)
    pair_t e = h[p];
    if (m == 0) {
      e.x -= ax * u.x;
      e.y -= ax * u.y;
    } else if (m == 1) {
      if (cx >= 0) e.x -= ax * v.x;
      if (cy >= 0) e.y -= ay * u.x;
    } else {
      e.x -= ay * u.y;
      e.y -= ay * v.x;
    }
    h[p] = e;
  }
}

// ---------------------------------------------------------------------------------------------
// Shaping kernel: R_d from r_d, a grid over delays, one delay per lane, the sum in ascending j.
// The loop runs to the wave's largest delay, so j and the weight w_j are wave-uniform (one scalar
// load) and consecutive lanes read consecutive r; a lane past its own delay skips the term.  A
// term with r = 0 is skipped (no 0·inf from a non-finite weight; R_0 = R_1 = 0 whatever w), and w
// null skips the product.  w is read at j <= min(D, n) − 1 only.
__global__ void __launch_bounds__(kShapeThreads)
zmpc_push_shape_kernel(int64_t n, const double* __restrict__ r, const double* __restrict__ w,
                       int64_t D, pair_t* __restrict__ tab, double* __restrict__ resp) {
  const int64_t d = (int64_t)blockIdx.x * kShapeThreads + threadIdx.x;
  // the last lane's delay, as a value the compiler knows to be wave-uniform (n <= 2^24)
  const int64_t dwave = __builtin_amdgcn_readfirstlane((int)(d | 63));
  const int64_t dlast = dwave < n - 1 ? dwave : n - 1;
  const int64_t jend = D - 1 < dlast ? D - 1 : dlast;
  const bool live = d < n;
  double acc = 0.0;
  for (int64_t j = 0; j <= jend; ++j) {
    const double wj = w ? w[j] : 1.0;
    if (live && j <= d) {
      const double rv = r[d - j];
      if (rv != 0.0) acc += w ? wj * rv : rv;
    }
  }
  if (live) {
    tab[d] = pair_t{acc, acc == 0.0 ? 0.0 : 1.0 / fabs(acc)};
    if (resp) resp[d] = acc;
  }
}

// ---------------------------------------------------------------------------------------------
// The candidate of one margin x >= 0 under a response of magnitude ra with reciprocal q; `fast`:
// q is a positive normal number
__device__ __forceinline__ double push_cand(double x, double q, double ra, bool fast) {
  return fast ? x * q : x / ra;
}

// One (sample, step) pair in both directions: mi = (up_i, dn_i) of sample i.  POS: r_d > 0 (a
// + push raises the ZMP: up limits +, dn limits −).  Strict <: of equal candidates the first one
// met stays.
template <bool POS>
__device__ __forceinline__ void push_pair(const pair_t mi, int i, double q, double ra,
                                          const bool fast, double& f0, double& f1, int& i0,
                                          int& i1) {
  const double c0 = push_cand(POS ? mi.x : mi.y, q, ra, fast);
  const double c1 = push_cand(POS ? mi.y : mi.x, q, ra, fast);
  if (c0 < f0) {
    f0 = c0;
    i0 = i;
  }
  if (c1 < f1) {
    f1 = c1;
    i1 = i;
  }
}

// One sample of a walk: the margins (up, dn) of axis `axis` (0: x, 1: y), and whether it fails the
// nominal test (a non-finite state value, or a violation above t on either axis — the test of
// metrics.hip AxisAcc::add)
struct Sample {
  pair_t m;
  bool bad;
};

__device__ __forceinline__ Sample push_sample(const pair_t* __restrict__ h,
                                              const pair_t* __restrict__ hi,
                                              const pair_t* __restrict__ lo, int64_t i, double hg,
                                              double t, int axis) {
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
  const double z = axis ? zy : zx, ua = axis ? u.y : u.x, la = axis ? l.y : l.x;
  s.m = pair_t{(ua - z) + t, (z - la) + t};
  return s;
}

// A margin pair as the LDS holds it: 16-byte aligned, so that a pair is one 128-bit LDS access
// (two 64-bit ones cost four times the LDS cycles)
struct alignas(16) lds_pair_t {
  double x, y;
};

// Full map of NAX axes, 2·NAX columns per step in the order (+x, −x, +y, −y).  NAX = 1: the axis
// `axis` (0: x, 1: y; wave-uniform); NAX = 2: x then y, in turn over the same n + 64 LDS pairs.  A
// turn fills the margins of its axis, then lanes own push steps over mirrored 64-step blocks, and
// writes its two columns.  The nominal test covers both axes in every fill; the second fill's
// reads of the walk's 48·n bytes come from cache.
template <int NAX>
__global__ void __launch_bounds__(1024)
zmpc_push_map_kernel(int64_t n, const double* __restrict__ hist, const double* __restrict__ zmax,
                     const double* __restrict__ zmin, int64_t bstride,
                     const int64_t* __restrict__ lengths, double hg, double t,
                     const pair_t* __restrict__ tab, int axis, double* __restrict__ force,
                     int32_t* __restrict__ limit) {
  extern __shared__ lds_pair_t m[];  // [n + 64]
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  int64_t nb = lengths ? lengths[b] : n;
  nb = nb < 1 ? 1 : (nb > n ? n : nb);
  const pair_t* h = reinterpret_cast<const pair_t*>(hist + b * n * 6);
  const pair_t* hi = reinterpret_cast<const pair_t*>(zmax + b * bstride);
  const pair_t* lo = reinterpret_cast<const pair_t*>(zmin + b * bstride);
  const double inf = __builtin_inf();
  pair_t* fo = reinterpret_cast<pair_t*>(force) + b * n * NAX;
  ipair_t* li = limit ? reinterpret_cast<ipair_t*>(limit) + b * n * NAX : nullptr;
  const int nblk = (int)((n + 63) >> 6);
  int bad = 0;
  // (one copy of the turn's code: unrolled, the two copies' scalar registers spill)
#pragma clang loop unroll(disable)
  for (int col = 0; col < NAX; ++col) {
    const int a = NAX == 2 ? col : axis;
    if (NAX == 2 && col) __syncthreads();  // the first axis' reads are done
    for (int64_t i = threadIdx.x; i < nb + 64; i += blockDim.x) {
      lds_pair_t p{inf, inf};
      if (i < nb) {
        const Sample s = push_sample(h, hi, lo, i, hg, t, a);
        bad |= s.bad;
        p = lds_pair_t{s.m.x, s.m.y};
      }
      m[i] = p;
    }
    bad = __syncthreads_or(bad);  // (also orders the LDS stores before the reads below)
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
          auto one = [&](int d, const pair_t rq, const lds_pair_t ml) {
            const pair_t mi{ml.x, ml.y};
            const double r = rq.x, q = rq.y;
            if (r == 0.0) return;
            // wave-uniform branches: the division is only ever issued for a denormal or
            // non-finite response.  (Deciding them on the bit patterns with scalar integer
            // instructions, and tracking the uniform delay instead of the sample, measured 16 %
            // slower.)
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
            const lds_pair_t m0 = m[s + d], m1 = m[s + d + 1], m2 = m[s + d + 2],
                             m3 = m[s + d + 3];
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
          fo[(int64_t)s * NAX + col] = pair_t{f0, f1};
          if (li) li[(int64_t)s * NAX + col] = ipair_t{i0, i1};
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// min-butterfly step, the lower index on a tie (symmetric in the two lanes: all end with the same)
__device__ __forceinline__ void push_min_lanes(double& f, int& i, int mask) {
  const double o = __shfl_xor(f, mask);
  const int j = __shfl_xor(i, mask);
  if (o < f || (o == f && (unsigned)j < (unsigned)i)) {
    f = o;
    i = j;
  }
}

// Single-step form of the axes AXES (ZMPC_PUSH_AXIS_X, _Y or both): one wave per walk, kStepWaves
// walks per workgroup, lanes over samples, 2·NAX values per walk in the map's column order.  The
// axes are a compile-time choice, and the two axes are written out, not looped over: with the axis
// in a register, or the samples in an array filled by a loop, the compiler issues the loads of
// the bounds behind the finiteness test's branch, one more memory round trip per sample (2 % of
// a launch at 4096 × 420).
template <int AXES>
__global__ void __launch_bounds__(64 * kStepWaves)
zmpc_push_step_kernel(int64_t B, int64_t n, const double* __restrict__ hist,
                      const double* __restrict__ zmax, const double* __restrict__ zmin,
                      int64_t bstride, const int64_t* __restrict__ lengths,
                      const int64_t* __restrict__ steps, double hg, double t,
                      const pair_t* __restrict__ tab, double* __restrict__ force,
                      int32_t* __restrict__ limit) {
  constexpr int NAX = AXES == 3 ? 2 : 1;
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
  double f[NAX][2];  // [axis][direction]
  int ix[NAX][2];
#pragma unroll
  for (int a = 0; a < NAX; ++a) {
    f[a][0] = f[a][1] = inf;
    ix[a][0] = ix[a][1] = -1;
  }
  int bad = 0;
  for (int64_t i = lane; i < nb; i += 64) {
    // the sample on the first axis and, of two axes, on y (the loads and the nominal test are
    // common to both)
    const Sample sa = push_sample(h, hi, lo, i, hg, t, AXES == ZMPC_PUSH_AXIS_Y);
    const Sample sy = push_sample(h, hi, lo, i, hg, t, 1);
    bad |= sa.bad;
    if (i > s) {
      const pair_t rq = tab[i - s];
      const double r = rq.x;
      if (r != 0.0) {
        const double q = rq.y, ra = fabs(r);
        const bool fast = q >= 0x1p-1022 && q < inf;  // a positive normal number, as the map
        if (r > 0.0) {
          push_pair<true>(sa.m, (int)i, q, ra, fast, f[0][0], f[0][1], ix[0][0], ix[0][1]);
          if (NAX == 2)
            push_pair<true>(sy.m, (int)i, q, ra, fast, f[NAX - 1][0], f[NAX - 1][1],
                            ix[NAX - 1][0], ix[NAX - 1][1]);
        } else {
          push_pair<false>(sa.m, (int)i, q, ra, fast, f[0][0], f[0][1], ix[0][0], ix[0][1]);
          if (NAX == 2)
            push_pair<false>(sy.m, (int)i, q, ra, fast, f[NAX - 1][0], f[NAX - 1][1],
                             ix[NAX - 1][0], ix[NAX - 1][1]);
        }
      }
    }
  }
#pragma unroll
  for (int mask = 1; mask < 64; mask <<= 1) {
#pragma unroll
    for (int c = 0; c < 2 * NAX; ++c) push_min_lanes(f[c >> 1][c & 1], ix[c >> 1][c & 1], mask);
    bad |= __shfl_xor(bad, mask);
  }
  if (lane < 2 * NAX) {
    double fv = f[0][0];
    int iv = ix[0][0];
#pragma unroll
    for (int c = 1; c < 2 * NAX; ++c)
      if (lane == c) {
        fv = f[c >> 1][c & 1];
        iv = ix[c >> 1][c & 1];
      }
    force[b * 2 * NAX + lane] = bad ? __builtin_nan("") : fv;
    if (limit) limit[b * 2 * NAX + lane] = bad ? -1 : iv;
  }
}

}  // namespace

hipError_t zmpc_push_map_set_attrs() {
  const hipError_t e =
      hipFuncSetAttribute((const void*)zmpc_push_map_kernel<1>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPushMapLdsCap);
  return e != hipSuccess ? e
                         : hipFuncSetAttribute((const void*)zmpc_push_map_kernel<2>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)kPushMapLdsCap);
}

hipError_t zmpc_launch_push_map(const zmpc_plan* p, const PushCall& c, hipStream_t s) {
  const int64_t n = c.n;
  const bool shape = c.duration != 1 || c.profile != nullptr;
  // the response table of this n, recomputed per launch into one stream-ordered workspace (a plan
  // is shared by threads and streams, each with an n of its own): the table's pairs [n]; for a
  // shaped push the base table's pairs [n] before them and the base response as plain doubles
  // [n] behind, which the shaping kernel reads at unit stride
  pair_t* ws = nullptr;
  hipError_t e = hipMallocAsync(
      (void**)&ws, (size_t)n * (shape ? 2 * sizeof(pair_t) + sizeof(double) : sizeof(pair_t)), s);
  if (e != hipSuccess) return hipErrorOutOfMemory;
  pair_t* tab = shape ? ws + n : ws;
  double* base = shape ? reinterpret_cast<double*>(ws + 2 * n) : c.response;
  hipLaunchKernelGGL(zmpc_push_response_kernel, dim3(1), dim3(64), 0, s, n, p->kx, p->T, p->T2_2,
                     p->T3_6, p->hg, p->T / c.mass, ws, base, (pair_t*)nullptr);
  if (shape)
    hipLaunchKernelGGL(zmpc_push_shape_kernel,
                       dim3((unsigned)((n + kShapeThreads - 1) / kShapeThreads)),
                       dim3(kShapeThreads), 0, s, n, base, c.profile, c.duration, tab, c.response);
  if (c.B > 0) {
    const bool two = c.axes == (ZMPC_PUSH_AXIS_X | ZMPC_PUSH_AXIS_Y);
    const int axis = c.axes == ZMPC_PUSH_AXIS_Y;  // of a one-axis launch
    if (c.push_steps) {
      const dim3 grid((unsigned)((c.B + kStepWaves - 1) / kStepWaves)), block(64 * kStepWaves);
      auto k = two ? zmpc_push_step_kernel<3>
                   : axis ? zmpc_push_step_kernel<ZMPC_PUSH_AXIS_Y>
                          : zmpc_push_step_kernel<ZMPC_PUSH_AXIS_X>;
      hipLaunchKernelGGL(k, grid, block, 0, s, c.B, n, c.hist, c.zmax, c.zmin, c.bstride,
                         c.lengths, c.push_steps, p->hg, c.t, tab, c.force, c.limit);
    } else {
      const PushMapChoice g = choose_push_shaped(n, false, two ? 2 : 1);
      auto k = two ? zmpc_push_map_kernel<2> : zmpc_push_map_kernel<1>;
      hipLaunchKernelGGL(k, dim3((unsigned)c.B), dim3(64 * g.waves), g.lds, s, n, c.hist, c.zmax,
                         c.zmin, c.bstride, c.lengths, p->hg, c.t, tab, axis, c.force, c.limit);
    }
  }
  e = hipGetLastError();
  const hipError_t ef = hipFreeAsync(ws, s);
  return e != hipSuccess ? e : ef;
}

hipError_t zmpc_launch_push_response(const zmpc_plan* p, const RolloutCall& c, hipStream_t s) {
  const int64_t n = c.n, B = c.B;
  const PushArgs& w = c.push;
  if (n < 2 || B < 1) return hipSuccess;  // no step to push at
  const bool shape = w.dur != 1 || w.w != nullptr;
  // the state response of this n, recomputed per launch into one stream-ordered workspace: two
  // pairs per delay, and as many again for the shaped table
  pair_t* ws = nullptr;
  hipError_t e = hipMallocAsync((void**)&ws, (size_t)n * (shape ? 4 : 2) * sizeof(pair_t), s);
  if (e != hipSuccess) return hipErrorOutOfMemory;
  hipLaunchKernelGGL(zmpc_push_response_kernel, dim3(1), dim3(64), 0, s, n, p->kx, p->T, p->T2_2,
                     p->T3_6, p->hg, 0.0, (pair_t*)nullptr, (double*)nullptr, ws);
  const pair_t* S = ws;
  if (shape) {
    hipLaunchKernelGGL(zmpc_push_state_shape_kernel,
                       dim3((unsigned)((n + kShapeThreads - 1) / kShapeThreads)),
                       dim3(kShapeThreads), 0, s, n, ws, w.w, (int64_t)w.dur, ws + 2 * n);
    S = ws + 2 * n;
  }
  // workgroups per walk: one per 1024 pairs, fewer where the grid would pass 2^31 − 1 blocks
  int64_t chunks = (3 * n + 4 * kAddThreads - 1) / (4 * kAddThreads);
  if (chunks > 0x7fffffff / B) chunks = 0x7fffffff / B;
  if (chunks < 1) chunks = 1;
  hipLaunchKernelGGL(zmpc_push_add_kernel, dim3((unsigned)(B * chunks)), dim3(kAddThreads), 0, s, n,
                     (int)chunks, w.amp, w.cols, w.col[0], w.col[1], w.steps, w.step, S, c.hist);
  e = hipGetLastError();
  const hipError_t ef = hipFreeAsync(ws, s);
  return e != hipSuccess ? e : ef;
}
