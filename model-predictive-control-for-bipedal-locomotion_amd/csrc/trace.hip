// zmpc_rollout_traced on an unconstrained plan: the state response of a per-walk disturbance
// trace, streamed onto an unpushed history (include/zmpc.h, "The trace, stated once").
//
// The closed loop is linear and time-invariant, so the traced history is the unpushed one minus
//     δ_(s_b) = 0,   δ_(i+1) = Ā·δ_i + e1·dv[b, i − s_b, a],   hist[b, i, a, :] −= δ_i,  s_b < i < n
// with Ā = A − B·kxᵀ (as zmpc_push_response_kernel builds it).  The window form (pushmap.hip)
// shares one shaped table across the batch; a trace per walk has nothing to share, and an n·L
// convolution per walk would cost several times the rollout it decorates.  Here the recurrence is
// a scan, O(n) per walk:
//   - one wavefront per walk, both axes; the wave takes the walk in blocks of 64 consecutive
//     samples from s_b + 1 on, lane l the sample i = s_b + 1 + 64k + l, whose input is dv[b, 64k + l]
//     (zero past the trace's end): dv is read once, samples at or before s_b are never touched;
//   - inside a block an inclusive Kogge-Stone scan, round r adding Ā^(2^r) times the value 2^r
//     lanes below (r = 0 .. 5); then the state that entered the block, δ of the sample before it,
//     comes in through the lane's own power Ā^(l+1), and lane 63's result is carried on;
//   - the powers Ā^(2^r) come from squarings and Ā^(l+1) from the products of the bits of l + 1,
//     per launch and in registers: no table, no workspace;
//   - a walk's history is 3n 16-byte pairs, (c, ċ)x (c̈x, cy) (ċ, c̈)y per sample (pushmap.hip's
//     layout); consecutive lanes load and store consecutive pairs, and a pair fetches the two
//     components it needs from the lane that holds its sample.  A pair no requested axis reaches is
//     neither read nor written; the shared pair of a one-axis call writes its other half back as
//     read.
// Every sum runs in an order fixed by lane and block numbers alone, uncontracted: two calls agree
// bit for bit, a walk gives the same bits alone and inside any batch, and an all-zero trace
// subtracts +0 from every entry.  No index depends on a value of dv.
#include "trace_scan.h"

namespace {

#pragma clang fp contract(off)

// cx, cy: the column of an axis in dv, −1 for an axis that is not requested; L: the samples of a
// walk's trace, `cols` doubles each.
__global__ void __launch_bounds__(64 * kTraceWaves)
zmpc_trace_add_kernel(int64_t B, int64_t n, const double* __restrict__ kx, double T, double T2_2,
                      double T3_6, const double* __restrict__ dv, int cols, int cx, int cy,
                      const int64_t* __restrict__ steps, int64_t step, int64_t L,
                      double* __restrict__ hist) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * kTraceWaves + (threadIdx.x >> 6);
  if (b >= B) return;  // whole waves leave: the shuffles below see 64 live lanes
  const int64_t s = steps ? steps[b] : step;
  if (s < 0 || s >= n - 1) return;  // no disturbance for this walk (wave-uniform)

  TMat3 P[6], Q;  // Ā^(2^r) and the lane's Ā^(l+1) (trace_scan.h)
  trace_propagators(trace_closed_loop(kx, T, T2_2, T3_6), lane,
                    [&](int r, const TMat3& m) { P[r] = m; }, Q);

  const int64_t first = s + 1;              // the first sample the trace moves
  const int64_t live = n - first;           // samples first .. n − 1, >= 1
  const int64_t nin = L < live ? L : live;  // trace entries that reach a sample
  const double* dw = dv + b * L * (int64_t)cols;
  tpair_t* h = reinterpret_cast<tpair_t*>(hist + b * n * 6) + 3 * first;
  const int64_t npairs = 3 * live;
  double carry[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};  // δ of the sample before the block

  for (int64_t base = 0; base < live; base += 64) {
    const int64_t j = base + lane;
    // the input that makes δ of sample first + j out of its predecessor's
    double ux = 0.0, uy = 0.0;
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
    double v[2][3] = {{0.0, ux, 0.0}, {0.0, uy, 0.0}};
    trace_block_scan(P, Q, lane, carry, v);
    // the block's pairs 3·base + 64q + l, q = 0 .. 2: sample (64q + l) / 3 of the block, slot m
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int t = 64 * q + lane;
      const int src = t / 3, m = t - 3 * src;
      double g[2][3];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) g[a][c] = __shfl(v[a][c], src);
      const int64_t p = 3 * base + t;
      if (p >= npairs) continue;
      if ((m == 0 && cx < 0) || (m == 2 && cy < 0)) continue;
      tpair_t e = h[p];
      if (m == 0) {
        e.x -= g[0][0];
        e.y -= g[0][1];
      } else if (m == 1) {
        if (cx >= 0) e.x -= g[0][2];
        if (cy >= 0) e.y -= g[1][0];
      } else {
        e.x -= g[1][1];
        e.y -= g[1][2];
      }
      h[p] = e;
    }
  }
}

}  // namespace

hipError_t zmpc_launch_trace_response(const zmpc_plan* p, const RolloutCall& c, int64_t L,
                                      hipStream_t s) {
  const PushArgs& w = c.push;
  if (c.n < 2 || c.B < 1) return hipSuccess;  // no step to disturb
  const unsigned grid = (unsigned)((c.B + kTraceWaves - 1) / kTraceWaves);
  hipLaunchKernelGGL(zmpc_trace_add_kernel, dim3(grid), dim3(64 * kTraceWaves), 0, s, c.B, c.n,
                     p->kx, p->T, p->T2_2, p->T3_6, w.amp, w.cols, w.col[0], w.col[1], w.steps,
                     w.step, L, c.hist);
  return hipGetLastError();
}
