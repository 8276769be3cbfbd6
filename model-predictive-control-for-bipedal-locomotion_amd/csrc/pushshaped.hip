// Sustained and shaped pushes on either axis or both (include/zmpc.h zmpc_push_map_shaped), behind
// the push-robustness map of pushmap.hip, whose kernels stay as they are.  Three kernels: the
// shaping kernel turns the one-sample response table into that of a push that lasts D samples;
// zmpc_push_axes_kernel is the full map of the x axis or of both axes, the axes in turn over the
// same LDS; zmpc_push_step_axes_kernel is their single-step form.  A y-only launch runs
// pushmap.hip's own map and step kernels on the shaped table.  Candidates are formed by
// push_common.h's push_cand and push_pair, as there: a two-axis launch equals the one-axis
// launches column for column, and the single-step form the map's rows, bit for bit.
#include "push_common.h"
#include "zmpc_internal.h"

namespace {

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------
// A push with force profile F·w_j during history steps s + j, j < D, is a sum of one-sample
// pushes, so its response by delay is
//     R_d = Σ_{j = 0}^{min(D−1, d)} w_j·r_{d−j}
// and the map kernels run unchanged on the table (R_d, 1/|R_d|).  The x axis runs the same
// closed loop with the same r; a +x push lowers the x velocity.
//
// Shaping kernel: a grid over delays, one delay per lane, the sum in ascending j.  The loop
// runs to the wave's largest delay, so j and the weight w_j are wave-uniform (one scalar load)
// and consecutive lanes read consecutive r; a lane past its own delay skips the term.  A term
// with r = 0 is skipped (no 0·inf from a non-finite weight; R_0 = R_1 = 0 whatever w), and w
// null skips the product, so D = 1 copies r.  w is read at j <= min(D, n) − 1 only.
constexpr int kShapeThreads = 256;

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

// One sample of a walk with the margins of both axes (the arithmetic of push_sample)
struct Sample2 {
  pair_t mx, my;  // (up, dn) of x and of y
  bool bad;
};

__device__ __forceinline__ Sample2 push_sample2(const pair_t* __restrict__ h,
                                                const pair_t* __restrict__ hi,
                                                const pair_t* __restrict__ lo, int64_t i,
                                                double hg, double t) {
  const pair_t s0 = h[3 * i], s1 = h[3 * i + 1], s2 = h[3 * i + 2];  // (c,ċ | c̈,c | ċ,c̈)
  const pair_t u = hi[i], l = lo[i];
  Sample2 s;
  s.bad = !(isfinite(s0.x) && isfinite(s0.y) && isfinite(s1.x) && isfinite(s1.y) &&
            isfinite(s2.x) && isfinite(s2.y));
  const double zx = s0.x - hg * s1.x;
  const double zy = s1.y - hg * s2.y;
  const double vx = fmax(fmax(zx - u.x, l.x - zx), 0.0);
  const double vy = fmax(fmax(zy - u.y, l.y - zy), 0.0);
  s.bad = s.bad || vx > t || vy > t;
  s.mx = pair_t{(u.x - zx) + t, (zx - l.x) + t};
  s.my = pair_t{(u.y - zy) + t, (zy - l.y) + t};
  return s;
}

// A margin pair as the LDS holds it here: 16-byte aligned, so that a pair is one 128-bit LDS
// access (two 64-bit ones cost four times the LDS cycles)
struct alignas(16) lds_pair_t {
  double x, y;
};

// Full map of the axes in `axes` (bit 0: x, bit 1: y), C = 2 or 4 columns per step.  The axes
// take turns over the same n + 64 LDS pairs: each turn is zmpc_push_map_kernel's — fill the
// margins of that axis, then lanes own push steps over mirrored 64-step blocks — and writes its
// two columns.  The nominal test covers both axes in every fill; the second fill's reads of the
// walk's 48·n bytes come from cache.
__global__ void __launch_bounds__(1024)
zmpc_push_axes_kernel(int64_t n, const double* __restrict__ hist, const double* __restrict__ zmax,
                      const double* __restrict__ zmin, int64_t bstride,
                      const int64_t* __restrict__ lengths, double hg, double t,
                      const pair_t* __restrict__ tab, int axes, double* __restrict__ force,
                      int32_t* __restrict__ limit) {
  extern __shared__ lds_pair_t ma[];  // [n + 64]
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  int64_t nb = lengths ? lengths[b] : n;
  nb = nb < 1 ? 1 : (nb > n ? n : nb);
  const pair_t* h = reinterpret_cast<const pair_t*>(hist + b * n * 6);
  const pair_t* hi = reinterpret_cast<const pair_t*>(zmax + b * bstride);
  const pair_t* lo = reinterpret_cast<const pair_t*>(zmin + b * bstride);
  const double inf = __builtin_inf();
  const int cp = axes == 3 ? 2 : 1;  // column pairs per step
  pair_t* fo = reinterpret_cast<pair_t*>(force) + b * n * cp;
  ipair_t* li = limit ? reinterpret_cast<ipair_t*>(limit) + b * n * cp : nullptr;
  const int nblk = (int)((n + 63) >> 6);
  int bad = 0, col = 0;
  // (one copy of the turn's code: unrolled, the two copies' scalar registers spill)
#pragma clang loop unroll(disable)
  for (int a = 0; a < 2; ++a) {
    if (!((axes >> a) & 1)) continue;
    if (col) __syncthreads();  // the first axis' reads are done
    for (int64_t i = threadIdx.x; i < nb + 64; i += blockDim.x) {
      double up = inf, dn = inf;
      if (i < nb) {
        const Sample2 s = push_sample2(h, hi, lo, i, hg, t);
        bad |= s.bad;
        up = a ? s.my.x : s.mx.x;
        dn = a ? s.my.y : s.mx.y;
      }
      ma[i] = lds_pair_t{up, dn};
    }
    bad = __syncthreads_or(bad);  // (also orders the LDS stores before the reads below)
    for (int k = wave; 2 * k < nblk; k += nwaves) {
      for (int half = 0; half < 2; ++half) {
        const int blk = half ? nblk - 1 - k : k;
        if (half && blk == k) break;
        const int s0 = blk << 6, s = s0 + lane;
        double f0 = inf, f1 = inf;
        int i0 = -1, i1 = -1;
        if (!bad) {
          const int dmax = (int)nb - 1 - s0;
          auto one = [&](int d, const pair_t rq, const lds_pair_t ml) {
            const pair_t mi{ml.x, ml.y};
            const double r = rq.x, q = rq.y;
            if (r == 0.0) return;
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
            const lds_pair_t m0 = ma[s + d], m1 = ma[s + d + 1], m2 = ma[s + d + 2],
                             m3 = ma[s + d + 3];
            one(d, t0, m0);
            one(d + 1, t1, m1);
            one(d + 2, t2, m2);
            one(d + 3, t3, m3);
          }
          for (; d <= dmax; ++d) one(d, tab[d], ma[s + d]);
        } else {
          f0 = f1 = __builtin_nan("");
        }
        if (s < n) {
          fo[(int64_t)s * cp + col] = pair_t{f0, f1};
          if (li) li[(int64_t)s * cp + col] = ipair_t{i0, i1};
        }
      }
    }
    ++col;
  }
}

// Single-step form of the axes in `axes`: zmpc_push_step_kernel with the candidates of both axes
// (those of an axis that was not asked for are formed and dropped: the kernel is bound by the
// history it reads), C = 2 or 4 values per walk.
__device__ __forceinline__ void push_min_lanes(double& f, int& i, int mask) {
  const double o = __shfl_xor(f, mask);
  const int j = __shfl_xor(i, mask);
  if (o < f || (o == f && (unsigned)j < (unsigned)i)) {
    f = o;
    i = j;
  }
}

__global__ void __launch_bounds__(64 * kStepWaves)
zmpc_push_step_axes_kernel(int64_t B, int64_t n, const double* __restrict__ hist,
                           const double* __restrict__ zmax, const double* __restrict__ zmin,
                           int64_t bstride, const int64_t* __restrict__ lengths,
                           const int64_t* __restrict__ steps, double hg, double t,
                           const pair_t* __restrict__ tab, int axes, double* __restrict__ force,
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
  double fx0 = inf, fx1 = inf, fy0 = inf, fy1 = inf;
  int ix0 = -1, ix1 = -1, iy0 = -1, iy1 = -1;
  int bad = 0;
  for (int64_t i = lane; i < nb; i += 64) {
    const Sample2 sm = push_sample2(h, hi, lo, i, hg, t);
    bad |= sm.bad;
    if (i > s) {
      const pair_t rq = tab[i - s];
      const double r = rq.x;
      if (r != 0.0) {
        const double q = rq.y, ra = fabs(r);
        const bool fast = q >= 0x1p-1022 && q < inf;  // a positive normal number, as the map
        if (r > 0.0) {
          push_pair<true>(sm.mx, (int)i, q, ra, fast, fx0, fx1, ix0, ix1);
          push_pair<true>(sm.my, (int)i, q, ra, fast, fy0, fy1, iy0, iy1);
        } else {
          push_pair<false>(sm.mx, (int)i, q, ra, fast, fx0, fx1, ix0, ix1);
          push_pair<false>(sm.my, (int)i, q, ra, fast, fy0, fy1, iy0, iy1);
        }
      }
    }
  }
  // min-butterfly, the lower index on a tie (symmetric in the two lanes: all end with the same)
#pragma unroll
  for (int mask = 1; mask < 64; mask <<= 1) {
    push_min_lanes(fx0, ix0, mask);
    push_min_lanes(fx1, ix1, mask);
    push_min_lanes(fy0, iy0, mask);
    push_min_lanes(fy1, iy1, mask);
    bad |= __shfl_xor(bad, mask);
  }
  if (bad) {
    fx0 = fx1 = fy0 = fy1 = __builtin_nan("");
    ix0 = ix1 = iy0 = iy1 = -1;
  }
  const int C = axes == 3 ? 4 : 2;
  if (lane < C) {
    const int k = axes == 2 ? lane + 2 : lane;  // the column among (+x, −x, +y, −y)
    force[b * C + lane] = k == 0 ? fx0 : k == 1 ? fx1 : k == 2 ? fy0 : fy1;
    if (limit) limit[b * C + lane] = k == 0 ? ix0 : k == 1 ? ix1 : k == 2 ? iy0 : iy1;
  }
}

}  // namespace

hipError_t zmpc_push_shaped_set_attrs() {
  return hipFuncSetAttribute((const void*)zmpc_push_axes_kernel,
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPushMapLdsCap);
}

hipError_t zmpc_launch_push_map_shaped(const zmpc_plan* p, int64_t B, int64_t n,
                                       const double* hist, const double* zmax,
                                       const double* zmin, int64_t bstride,
                                       const int64_t* lengths, const int64_t* push_steps,
                                       const double* profile, int64_t duration, int axes, double t,
                                       double mass, double* force, int32_t* limit,
                                       double* response, hipStream_t s) {
  const PushMapChoice c = choose_push_shaped(n, push_steps != nullptr, axes == 3 ? 2 : 1);
  // one stream-ordered workspace: the base table's pairs [n], the shaped table's pairs [n] and
  // the base response as plain doubles [n], which the shaping kernel reads at unit stride
  pair_t* ws = nullptr;
  hipError_t e = hipMallocAsync((void**)&ws, (size_t)n * (2 * sizeof(pair_t) + sizeof(double)), s);
  if (e != hipSuccess) return hipErrorOutOfMemory;
  pair_t* tab = ws + n;
  double* base = reinterpret_cast<double*>(ws + 2 * n);
  zmpc_push_base_table(p, n, mass, ws, base, s);
  hipLaunchKernelGGL(zmpc_push_shape_kernel, dim3((unsigned)((n + kShapeThreads - 1) / kShapeThreads)),
                     dim3(kShapeThreads), 0, s, n, base, profile, duration, tab, response);
  if (B > 0) {
    const unsigned sgrid = (unsigned)((B + kStepWaves - 1) / kStepWaves);
    if (axes == ZMPC_PUSH_AXIS_Y) {  // the y columns alone: the kernels of zmpc_push_map
      zmpc_push_map_on_table(p, B, n, hist, zmax, zmin, bstride, lengths, push_steps, t, tab, force,
                             limit, s);
    } else if (push_steps) {
      hipLaunchKernelGGL(zmpc_push_step_axes_kernel, dim3(sgrid), dim3(64 * kStepWaves), 0, s, B,
                         n, hist, zmax, zmin, bstride, lengths, push_steps, p->hg, t, tab, axes,
                         force, limit);
    } else {
      hipLaunchKernelGGL(zmpc_push_axes_kernel, dim3((unsigned)B), dim3(64 * c.waves), c.lds, s, n,
                         hist, zmax, zmin, bstride, lengths, p->hg, t, tab, axes, force, limit);
    }
  }
  e = hipGetLastError();
  const hipError_t ef = hipFreeAsync(ws, s);
  return e != hipSuccess ? e : ef;
}
