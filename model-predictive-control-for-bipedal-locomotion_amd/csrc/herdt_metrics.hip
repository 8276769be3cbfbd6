// Per-walk survival metrics of a batched Herdt rollout (include/zmpc.h zmpc_herdt_walk_metrics).
// A Herdt walk has no fixed CoP bounds: the support box of a sample follows the footsteps the QP
// chose, so the box is rebuilt here from the rollout's own foot history and support states — the
// ZMP z = c − (h/g)·c̈ of sample i against the box round foot[i − 1], the foot that row 0 of the
// QP of step i − 1 belonged to — and the verdict comes from the divergent component of motion
// relative to that foot (the QP is always feasible: the ZMP never leaves its box, the CoM does).
// Reduced on the device to ZMPC_NHERDT_METRICS doubles per walk.
//
// Laid out as metrics.hip: one wavefront per walk, four walks per 256-thread workgroup, lane l
// takes samples l, l + 64, …; a sample is three 16-byte loads of hist, one 16-byte row of foot and
// one byte of state (65 B per sample, 81 B with foot_ref); nothing is loaded twice.  New against
// that kernel is the side of the supporting foot: the parity of the landings before the sample.
// A landing is booked on the sample after it: one __ballot of "this sample is SINGLE_SUPPORT"
// over the 64 samples of a block, shifted by one lane with the bit carried from the block before,
// gives the mask of landings; __popcll of the lower lanes' bits plus the count of the blocks
// before, which is the same in every lane, is what sample i and the landing at step i − 1 both
// need.  Row i − 1 of foot is the neighbouring lane's row (DPP wave_shr:1), for lane 0 the last
// row of the block before (v_readlane).  A second load of rows i − 1 and 86 registers ran at 57 %
// of the copy ceiling where this form (70 registers, 7 waves per SIMD) runs at 85 %.
//
// The per-lane partial results are combined by an xor butterfly in an order fixed by the lane
// numbers: two launches on the same input agree bit for bit.  No LDS, no atomics, no workspace.
// z, the boxes, the deviations and the facet slacks are evaluated without contraction, as NumPy
// evaluates mpc_bipedal/analysis.py herdt_walk_metrics_reference.
#include "zmpc_internal.h"

namespace {

#pragma clang fp contract(off)

constexpr int kWaves = 4;  // walks per workgroup
constexpr int8_t kStanding = 0, kSingleSupport = 2;

// 16-byte pairs of doubles, one global_load_dwordx4 each; only 8-byte alignment is promised (a
// foot_ref_stride may be odd), which gfx9 global loads accept
struct pair_t {
  double x, y;
};

// what the kernel reads of zmpc_herdt_params: wave-uniform, passed by value
struct HerdtBox {
  double half_len, half_wid;  // ½·foot_length, ½·foot_width
  double spread2;             // 2·foot_spread: from the supporting foot to the other one
  int nf[2];                  // facets of the left / right swing polytope
  double facets[2][ZMPC_HERDT_MAX_FACETS][3];
};

// the value of the lane below (DPP wave_shr:1; lane 0 reads 0)
__device__ __forceinline__ double prev_lane(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x138, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x138, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

// the value of lane 63, in scalar registers
__device__ __forceinline__ double last_lane(double v) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63),
                          __builtin_amdgcn_readlane(__double2loint(v), 63));
}

// one axis of one lane's share of a walk
struct HerdtAcc {
  double vmax = 0.0;     // largest violation so far
  int vidx = -1;         // its first sample, −1 while vmax is 0
  int count = 0;         // samples with a violation above count_tol
  double dev = 0.0;      // largest |c − fs|
  double ddev = 0.0;     // largest |c + ċ·√(h/g) − fs|
  double shift = 0.0;    // largest |foot − foot_ref|
  int bad = 0x7fffffff;  // first sample with a non-finite value

  // sample i: state (c, v, a), supporting foot fs = foot[i − 1], own foot row fi, nominal row fr
  // (has_ref), box [lo, hi]; returns the DCM relative to fs
  __device__ __forceinline__ double add(int i, double c, double v, double a, double fs, double fi,
                                        bool has_ref, double fr, double lo, double hi, double hg,
                                        double root, double tol) {
    if (!(isfinite(c) && isfinite(v) && isfinite(a) && isfinite(fi)) ||
        (has_ref && !isfinite(fr))) {
      bad = min(bad, i);
      return 0.0;
    }
    const double z = c - hg * a;
    const double viol = i == 0 ? 0.0 : fmax(fmax(z - hi, lo - z), 0.0);  // sample 0 has no box
    if (viol > tol) ++count;
    if (viol > vmax) {  // strict: a lane's samples ascend, the first one that attains it stays
      vmax = viol;
      vidx = i;
    }
    dev = fmax(dev, fabs(c - fs));
    const double dcm = (c + v * root) - fs;
    ddev = fmax(ddev, fabs(dcm));
    if (has_ref) shift = fmax(shift, fabs(fi - fr));
    return dcm;
  }

  // butterfly step (symmetric in the two lanes, so both end with the same bits); a tie in the
  // violation goes to the lower index
  __device__ __forceinline__ void combine(int mask) {
    const double ov = __shfl_xor(vmax, mask);
    const int oi = __shfl_xor(vidx, mask);
    if (ov > vmax || (ov == vmax && oi < vidx)) {
      vmax = ov;
      vidx = oi;
    }
    count += __shfl_xor(count, mask);
    dev = fmax(dev, __shfl_xor(dev, mask));
    ddev = fmax(ddev, __shfl_xor(ddev, mask));
    shift = fmax(shift, __shfl_xor(shift, mask));
    bad = min(bad, __shfl_xor(bad, mask));
  }
};

__global__ void __launch_bounds__(64 * kWaves)
zmpc_herdt_walk_metrics_kernel(int64_t B, int64_t n, const double* __restrict__ hist,
                               const double* __restrict__ foot,
                               const int8_t* __restrict__ states, int64_t sstride,
                               const double* __restrict__ fref, int64_t rstride,
                               const int64_t* __restrict__ lengths, double tol, double hg,
                               double sqrt_hg, const HerdtBox box, double* __restrict__ metrics) {
  const int lane = threadIdx.x & 63;
  // the walk is the wave's: read through the first lane, so that the compiler keeps the walk's
  // length, pointers and carries in scalar registers
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t b = (int64_t)blockIdx.x * kWaves + wave;
  if (b >= B) return;  // whole waves leave: the cross-lane operations below see 64 live lanes
  // live samples of this walk; a length outside [1, n] is clamped, never followed out of the
  // arrays
  const int64_t len = lengths ? lengths[b] : n;
  const int nb = (int)(len < 1 ? 1 : (len > n ? n : len));  // (n <= 2^24 is the caller's check)
  const pair_t* h = reinterpret_cast<const pair_t*>(hist + b * n * 6);
  const pair_t* ft = reinterpret_cast<const pair_t*>(foot + b * n * 2);
  const pair_t* rf = fref ? reinterpret_cast<const pair_t*>(fref + b * rstride) : nullptr;
  const int8_t* st = states + b * sstride;
  const bool has_ref = rf != nullptr;
  const unsigned long long below = (1ull << lane) - 1;  // the lanes under this one
  HerdtAcc ax, ay;
  double dcm_x = 0.0, dcm_y = 0.0;  // of the lane that holds the last sample
  double slack = __builtin_inf();   // smallest facet slack of this lane's landings
  int landed = 0;                   // landings booked in the blocks before (wave-uniform)
  // carried from the block before (wave-uniform): whether its last sample was SINGLE_SUPPORT
  // (bit 0), and its last foot row
  unsigned long long carry_ss = 0;
  pair_t carry_f{};
  // every lane runs every block: the cross-lane operations need the whole wave
  for (int base = 0; base < nb; base += 64) {
    const int i = base + lane;
    const bool live = i < nb;
    pair_t s0{}, s1{}, s2{}, f{}, r{};
    int8_t sc = kStanding;
    if (live) {
      sc = st[i];  // first: the ballot below waits for this load alone
      f = ft[i];
      s0 = h[3 * i], s1 = h[3 * i + 1], s2 = h[3 * i + 2];  // (c,ċ | c̈,c | ċ,c̈)
      if (has_ref) r = rf[i];
    }
    // the landing at step i − 1 — sample i − 1 SINGLE_SUPPORT, sample i not: the rollout flipped
    // its side there and wrote the new foot to row i — from the bits of one ballot (sample 0 has
    // no sample before it: never a landing)
    const unsigned long long ss = __ballot(live && sc == kSingleSupport);
    const unsigned long long lv = nb - base >= 64 ? ~0ull : (1ull << (nb - base)) - 1;
    const unsigned long long m = ((ss << 1) | carry_ss) & ~ss & lv;
    carry_ss = ss >> 63;
    const bool land = (m >> lane) & 1;
    const int side = (landed + __popcll(m & below)) & 1;  // 0 left: landings at steps < i − 1
    landed += __popcll(m);
    // row i − 1 of foot is the row of the lane below; lane 0 takes the last row of the block
    // before, and at i = 0 row 0 itself
    pair_t fp{prev_lane(f.x), prev_lane(f.y)};
    if (lane == 0) fp = base ? carry_f : f;
    if (base + 64 < nb) carry_f = pair_t{last_lane(f.x), last_lane(f.y)};
    if (!live) continue;
    const double xlo = fp.x - box.half_len, xhi = fp.x + box.half_len;
    double ylo = fp.y - box.half_wid, yhi = fp.y + box.half_wid;
    if (sc == kStanding) {  // both feet on the ground: the hull of the two
      const double other = side ? fp.y + box.spread2 : fp.y - box.spread2;
      ylo = fmin(fp.y, other) - box.half_wid;
      yhi = fmax(fp.y, other) + box.half_wid;
    }
    const double dx = ax.add(i, s0.x, s0.y, s1.x, fp.x, f.x, has_ref, r.x, xlo, xhi, hg,
                             sqrt_hg, tol);
    const double dy = ay.add(i, s1.y, s2.x, s2.y, fp.y, f.y, has_ref, r.y, ylo, yhi, hg,
                             sqrt_hg, tol);
    if (i == nb - 1) {
      dcm_x = dx;
      dcm_y = dy;
    }
    if (land) {  // how much reach the step left: b − a·(foot[k+1] − foot[k]) over side_k's facets
      const double sx = f.x - fp.x, sy = f.y - fp.y;
      // both polytopes in turn, so that every facet is read at a wave-uniform address (scalar
      // loads of the kernel arguments); a lane keeps the slacks of its own side
      for (int sd = 0; sd < 2; ++sd)
        for (int k = 0; k < box.nf[sd]; ++k) {
          const double q = box.facets[sd][k][2] - (box.facets[sd][k][0] * sx +
                                                   box.facets[sd][k][1] * sy);
          if (side == sd) slack = fmin(slack, q);
        }
    }
  }
#pragma unroll
  for (int mask = 1; mask < 64; mask <<= 1) {
    ax.combine(mask);
    ay.combine(mask);
    slack = fmin(slack, __shfl_xor(slack, mask));
  }
  const int last = (nb - 1) & 63;
  dcm_x = __shfl(dcm_x, last);
  dcm_y = __shfl(dcm_y, last);
  // lanes 0..13 store slot 2k + a (quantity k of axis a), lane 14 the reach, lane 15 the landings
  if (lane < ZMPC_NHERDT_METRICS) {
    const bool y = lane & 1;
    const HerdtAcc& q = y ? ay : ax;
    const double nan = __builtin_nan("");
    const bool flagged = ax.bad != 0x7fffffff || ay.bad != 0x7fffffff;
    double out;
    if (lane == 15) {
      out = (double)landed;
    } else if (lane == 14) {
      out = flagged ? nan : slack;
    } else if (q.bad != 0x7fffffff) {
      // fail safe: a threshold on viol_max must not pass a walk with a non-finite value
      out = lane < 2 ? __builtin_inf() : (lane < 4 ? (double)q.bad : nan);
    } else {
      switch (lane >> 1) {
        case 0: out = q.vmax; break;
        case 1: out = (double)q.vidx; break;
        case 2: out = (double)q.count; break;
        case 3: out = q.dev; break;
        case 4: out = q.ddev; break;
        case 5: out = y ? dcm_y : dcm_x; break;
        default: out = q.shift; break;
      }
    }
    metrics[b * ZMPC_NHERDT_METRICS + lane] = out;
  }
}

}  // namespace

hipError_t zmpc_launch_herdt_walk_metrics(const zmpc_plan* p, const zmpc_herdt_params* prm,
                                          int64_t B, int64_t n, const double* hist,
                                          const double* foot, const int8_t* states,
                                          int64_t sstride, const double* foot_ref,
                                          int64_t rstride, const int64_t* lengths, double tol,
                                          double* metrics, hipStream_t s) {
  if (B == 0) return hipSuccess;
  HerdtBox box{};
  box.half_len = 0.5 * prm->foot_length;
  box.half_wid = 0.5 * prm->foot_width;
  box.spread2 = 2.0 * prm->foot_spread;
  for (int sd = 0; sd < 2; ++sd) {
    box.nf[sd] = prm->nfacets[sd];
    for (int k = 0; k < prm->nfacets[sd]; ++k)
      for (int c = 0; c < 3; ++c) box.facets[sd][k][c] = prm->facets[sd][k][c];
  }
  // one workgroup per four walks, as zmpc_launch_walk_metrics (B <= 2^31 − 1 is the caller's
  // check, so the grid fits)
  const unsigned grid = (unsigned)((B + kWaves - 1) / kWaves);
  hipLaunchKernelGGL(zmpc_herdt_walk_metrics_kernel, dim3(grid), dim3(64 * kWaves), 0, s, B, n,
                     hist, foot, states, sstride, foot_ref, rstride, lengths, tol, p->hg,
                     sqrt(p->hg), box, metrics);
  return hipGetLastError();
}
