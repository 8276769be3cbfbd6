// Per-walk robustness metrics of a batched rollout (include/zmpc.h zmpc_walk_metrics): the ZMP
// z = c − (h/g)·c̈ of every sample (run_mpc.py:294) against the sample's support box
// (run_compare_resistance.py:173-197 plots exactly this pairing, sample i with bounds row i),
// reduced on the device to ZMPC_NMETRICS doubles per walk, so that a robustness sweep never
// moves its [B, n, 2, 3] state history to the host or through a chain of torch temporaries.
//
// Memory-bound by construction: hist is read once (48 B per sample), each bounds row once (32 B,
// or from cache when every walk shares one CoP), 96 B are written per walk.  One wavefront per
// walk, four walks per 256-thread workgroup.  Lane l takes samples l, l + 64, …: a sample is
// three 16-byte loads per lane, consecutive lanes read consecutive 48-byte samples, so a wave's
// three loads cover 3 KiB of contiguous memory.  The
// per-lane partial results are combined by an xor butterfly (__shfl_xor): every lane ends with
// the same value, the order of the combination is fixed by the lane numbers, and so two launches
// on the same input agree bit for bit.  No LDS, no atomics, no workspace.
//
// The arithmetic of z, the box centre and the violation is evaluated without contraction, as
// NumPy evaluates the statement of mpc_bipedal/analysis.py walk_metrics_reference: the counts
// and indices then follow from the same doubles.
#include "zmpc_internal.h"

namespace {

#pragma clang fp contract(off)

constexpr int kWaves = 4;  // walks per workgroup

// 16-byte pairs of doubles, one global_load_dwordx4 each; only 8-byte alignment is promised (a
// bounds_stride may be odd, and a C caller's arrays are double arrays), which gfx9 global loads
// accept
struct pair_t {
  double x, y;
};

// one axis of one lane's share of a walk
struct AxisAcc {
  double vmax = 0.0;     // largest violation so far
  int vidx = -1;         // its first sample, −1 while vmax is 0
  int count = 0;         // samples with a violation
  double dev = 0.0;      // largest |c − zr|
  double sq = 0.0;       // Σ (z − zr)²
  int bad = 0x7fffffff;  // first sample with a non-finite state value

  __device__ __forceinline__ void add(int i, double c, double v, double a, double hi, double lo,
                                      double hg) {
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

  // butterfly step: combine with the partner lane's partial result (symmetric in the two lanes,
  // so both end with the same bits); a tie in the violation goes to the lower index
  __device__ __forceinline__ void combine(int mask) {
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
};

__global__ void __launch_bounds__(64 * kWaves)
zmpc_walk_metrics_kernel(int64_t B, int64_t n, const double* __restrict__ hist,
                         const double* __restrict__ zmax, const double* __restrict__ zmin,
                         int64_t bstride, const int64_t* __restrict__ lengths, double hg,
                         double sqrt_hg, double* __restrict__ metrics) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (b >= B) return;  // whole waves leave: the shuffles below see 64 live lanes
  // live samples of this walk; a length outside [1, n] is clamped, never followed out of the
  // arrays
  int64_t nb = lengths ? lengths[b] : n;
  nb = nb < 1 ? 1 : (nb > n ? n : nb);
  const pair_t* h = reinterpret_cast<const pair_t*>(hist + b * n * 6);
  const pair_t* hi = reinterpret_cast<const pair_t*>(zmax + b * bstride);
  const pair_t* lo = reinterpret_cast<const pair_t*>(zmin + b * bstride);
  AxisAcc ax, ay;
  double dcm_x = 0.0, dcm_y = 0.0;  // of the lane that holds the last sample
  for (int64_t i = lane; i < nb; i += 64) {
    const pair_t s0 = h[3 * i], s1 = h[3 * i + 1], s2 = h[3 * i + 2];  // (c,ċ | c̈,c | ċ,c̈)
    const pair_t u = hi[i], l = lo[i];
    ax.add((int)i, s0.x, s0.y, s1.x, u.x, l.x, hg);
    ay.add((int)i, s1.y, s2.x, s2.y, u.y, l.y, hg);
    if (i == nb - 1) {
      dcm_x = s0.x + s0.y * sqrt_hg - (u.x + l.x) * 0.5;
      dcm_y = s1.y + s2.x * sqrt_hg - (u.y + l.y) * 0.5;
    }
  }
#pragma unroll
  for (int mask = 1; mask < 64; mask <<= 1) {
    ax.combine(mask);
    ay.combine(mask);
  }
  const int last = (int)((nb - 1) & 63);
  dcm_x = __shfl(dcm_x, last);
  dcm_y = __shfl(dcm_y, last);
  // lanes 0..11 store one slot each (slot 2k + a: quantity k of axis a)
  if (lane < ZMPC_NMETRICS) {
    const bool y = lane & 1;
    const AxisAcc& r = y ? ay : ax;
    const double nan = __builtin_nan("");
    double out;
    if (r.bad != 0x7fffffff) {
      // fail safe: a threshold on viol_max must not pass a walk with a non-finite state
      out = lane < 2 ? __builtin_inf() : (lane < 4 ? (double)r.bad : nan);
    } else {
      switch (lane >> 1) {
        case 0: out = r.vmax; break;
        case 1: out = (double)r.vidx; break;
        case 2: out = (double)r.count; break;
        case 3: out = r.dev; break;
        case 4: out = sqrt(r.sq / (double)nb); break;
        default: out = y ? dcm_y : dcm_x; break;
      }
    }
    metrics[b * ZMPC_NMETRICS + lane] = out;
  }
}

}  // namespace

hipError_t zmpc_launch_walk_metrics(const zmpc_plan* p, int64_t B, int64_t n, const double* hist,
                                    const double* zmax, const double* zmin, int64_t bstride,
                                    const int64_t* lengths, double* metrics, hipStream_t s) {
  if (B == 0) return hipSuccess;
  // one workgroup per four walks, no persistent grid: walks may be ragged, and the hardware
  // dispatcher balances them (B <= 2^31 − 1 is the caller's check, so the grid fits)
  const unsigned grid = (unsigned)((B + kWaves - 1) / kWaves);
  hipLaunchKernelGGL(zmpc_walk_metrics_kernel, dim3(grid), dim3(64 * kWaves), 0, s, B, n, hist,
                     zmax, zmin, bstride, lengths, p->hg, sqrt(p->hg), metrics);
  return hipGetLastError();
}
