// The scan of a per-walk trace's state response, shared by zmpc_trace_add_kernel (trace.hip) and
// zmpc_trace_margin_kernel (trace_margin.hip):
//     δ_s = 0,   δ_(i+1) = Ā·δ_i + e1·dv[i − s],   Ā = A − B·kxᵀ
// taken by one wavefront in blocks of 64 consecutive samples from s + 1 on, lane l the sample
// s + 1 + 64k + l.  Order of the sums, fixed by lane and block numbers alone and uncontracted:
//   (1) v_l = e1·dv of the lane's sample;
//   (2) six Kogge-Stone rounds, round r adding Ā^(2^r)·v_(l − 2^r) for l >= 2^r;
//   (3) v_l += Ā^(l+1)·δ(the sample before the block);
//   (4) lane 63's v is carried into the next block.
// The powers Ā^(2^r) come from five squarings and Ā^(l+1) from the products of the set bits of
// l + 1, per launch: no table, no workspace.  The six powers are handed to the kernel as they are
// made and read through a pointer, so a kernel keeps them where it likes (registers in trace.hip,
// LDS in trace_margin.hip).
#pragma once
#include "zmpc_internal.h"

namespace {

#pragma clang fp contract(off)

struct tpair_t {
  double x, y;
};

struct TMat3 {
  double a[9];
};

// Walks (rows) per workgroup, one wave each
constexpr int kTraceWaves = 4;

__device__ __forceinline__ TMat3 tmul(const TMat3& p, const TMat3& q) {
  TMat3 s;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      s.a[3 * i + j] = p.a[3 * i] * q.a[j] + p.a[3 * i + 1] * q.a[3 + j] + p.a[3 * i + 2] * q.a[6 + j];
  return s;
}

// v += m·t
__device__ __forceinline__ void tmac(const TMat3& m, const double t[3], double v[3]) {
  const double x = m.a[0] * t[0] + m.a[1] * t[1] + m.a[2] * t[2];
  const double y = m.a[3] * t[0] + m.a[4] * t[1] + m.a[5] * t[2];
  const double z = m.a[6] * t[0] + m.a[7] * t[1] + m.a[8] * t[2];
  v[0] += x;
  v[1] += y;
  v[2] += z;
}

// Ā of a plan's gain row and step constants
__device__ __forceinline__ TMat3 trace_closed_loop(const double* __restrict__ kx, double T,
                                                   double T2_2, double T3_6) {
  const double k0 = kx[0], k1 = kx[1], k2 = kx[2];
  TMat3 A;
  A.a[0] = 1.0 - T3_6 * k0;
  A.a[1] = T - T3_6 * k1;
  A.a[2] = T2_2 - T3_6 * k2;
  A.a[3] = 0.0 - T2_2 * k0;
  A.a[4] = 1.0 - T2_2 * k1;
  A.a[5] = T - T2_2 * k2;
  A.a[6] = 0.0 - T * k0;
  A.a[7] = 0.0 - T * k1;
  A.a[8] = 1.0 - T * k2;
  return A;
}

// The propagators of a launch: P[r] = Ā^(2^r), r = 0 .. 5, by squaring, and Q = Ā^(l+1), the powers
// of the set bits of l + 1 multiplied on from the low bit up (bit 6: lane 63 alone).  A power is
// used as soon as it exists and handed to put(r, Ā^(2^r)), so only one is live at a time where the
// caller does not keep them in registers.
template <class Put>
__device__ __forceinline__ void trace_propagators(const TMat3& A, int lane, Put put, TMat3& Q) {
  TMat3 cur = A;
  Q = A;
  bool have = false;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    put(r, cur);
    if (((lane + 1) >> r) & 1) {
      Q = have ? tmul(cur, Q) : cur;
      have = true;
    }
    if (r < 5) cur = tmul(cur, cur);
  }
  if (lane == 63) Q = tmul(cur, cur);
}

// One block of the scan, steps (2) to (4): v [axis][3] holds e1·dv of the lane's sample on entry and
// δ of that sample on return; carry is δ of the sample before the block and becomes lane 63's v.
// P: Ā^(2^r), r = 0 .. 5; Q: the lane's Ā^(l+1).  All 64 lanes call it together.
__device__ __forceinline__ void trace_block_scan(const TMat3* P, const TMat3& Q, int lane,
                                                 double carry[2][3], double v[2][3]) {
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const int d = 1 << r;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      double t[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) t[c] = __shfl_up(v[a][c], d);
      if (lane >= d) tmac(P[r], t, v[a]);
    }
  }
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    tmac(Q, carry[a], v[a]);
#pragma unroll
    for (int c = 0; c < 3; ++c) carry[a][c] = __shfl(v[a][c], 63);
  }
}

}  // namespace
