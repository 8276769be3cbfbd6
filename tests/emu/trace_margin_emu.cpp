// Driver of the host emulation of zmpc_trace_margin_kernel (tests/test_trace_margin_emulation.py):
// scale [R][2] doubles, then limit [R][2] int32 when asked for, to stdout; R = B·K rows from a
// binary input file.  The emulation has one wave, wave 0 of a workgroup.
//   mode 0: every row runs alone as row 0 of a one-row launch on its own slice of the arrays (its
//           walk's history, bounds and length; its own trace, start step and outputs);
//   mode 1: the launch as the library issues it, on the whole arrays with the true K: workgroup q
//           runs its first wave, row 4q; the other rows keep the prefill −7.
// Input: int64 B, n, K, L, cols, cx, cy, has_steps, step, has_lengths, bstride, has_limit, mode;
// f64 T, T²/2, T³/6, kx[3], h/g, t; int64 lengths[B] when has_lengths; int64 steps[R] when
// has_steps; dv[R][L][cols]; hist[B][n][6]; zmax, zmin [B][n][2] (bstride = 2n) or [n][2]
// (bstride = 0).  Test infrastructure only.
#include "hip/hip_runtime.h"

EmuDim3 threadIdx, blockIdx;
uint64_t emu_buf[64];
static ucontext_t g_main, g_lane[64];
static int g_cur;
static bool g_done[64];
void emu_yield() { swapcontext(&g_lane[g_cur], &g_main); }

// the workgroup's LDS is one array for the 64 coroutines: lane 0 runs first and fills it before
// its first lockstep point, as the kernel's first thread does before the barrier
#undef __shared__
#define __shared__ static

#include "trace_margin_kernel_emu.h"  // generated from csrc/trace_margin.hip (kernel part)

#include <cstdio>
#include <vector>

struct Args {
  int64_t R, K, n, bstride, step, L;
  int cols, cx, cy;
  double T, T2_2, T3_6, hg, t;
  const double *kx, *hist, *zmax, *zmin, *dv;
  const int64_t *lengths, *steps;
  double* scale;
  int32_t* limit;
};
static Args g_a;
static void lane_main() {
  emu::zmpc_trace_margin_kernel(g_a.R, g_a.K, g_a.n, g_a.kx, g_a.T, g_a.T2_2, g_a.T3_6, g_a.hg,
                                g_a.t, g_a.hist, g_a.zmax, g_a.zmin, g_a.bstride, g_a.lengths,
                                g_a.dv, g_a.cols, g_a.cx, g_a.cy, g_a.steps, g_a.step, g_a.L,
                                g_a.scale, g_a.limit);
  g_done[g_cur] = true;
}

static void run_wave(std::vector<char>& stacks) {
  for (int l = 0; l < 64; ++l) {
    getcontext(&g_lane[l]);
    g_lane[l].uc_stack.ss_sp = stacks.data() + ((size_t)l << 18);
    g_lane[l].uc_stack.ss_size = (size_t)1 << 18;
    g_lane[l].uc_link = &g_main;
    g_done[l] = false;
    makecontext(&g_lane[l], lane_main, 0);
  }
  for (bool any = true; any;) {
    any = false;
    for (int l = 0; l < 64; ++l) {
      if (g_done[l]) continue;
      g_cur = l;
      threadIdx.x = l;
      swapcontext(&g_main, &g_lane[l]);
      any = true;
    }
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t hd[13];
  double c[8];
  bool ok = fread(hd, 8, 13, f) == 13 && fread(c, 8, 8, f) == 8;
  const int64_t B = hd[0], n = hd[1], K = hd[2], L = hd[3], cols = hd[4], bstride = hd[10];
  if (!ok || B < 1 || n < 1 || K < 1 || L < 1 || cols < 1 || cols > 2) return 2;
  if (bstride != 0 && bstride != 2 * n) return 2;
  const int64_t R = B * K;
  const size_t nbound = (size_t)(bstride ? B * n * 2 : n * 2);
  std::vector<int64_t> lengths(B), steps(R);
  std::vector<double> dv(R * L * cols), hist(B * n * 6), zmax(nbound), zmin(nbound);
  ok = (!hd[9] || fread(lengths.data(), 8, B, f) == (size_t)B) &&
       (!hd[7] || fread(steps.data(), 8, R, f) == (size_t)R) &&
       fread(dv.data(), 8, dv.size(), f) == dv.size() &&
       fread(hist.data(), 8, hist.size(), f) == hist.size() &&
       fread(zmax.data(), 8, nbound, f) == nbound && fread(zmin.data(), 8, nbound, f) == nbound;
  fclose(f);
  if (!ok) return 2;
  std::vector<double> scale(R * 2, -7.0);
  std::vector<int32_t> limit(R * 2, -7);
  std::vector<char> stacks((size_t)64 << 18);
  const Args full{R,    K,    n,     bstride,     hd[8],       L,           (int)cols,
                  (int)hd[5], (int)hd[6], c[0], c[1], c[2], c[6], c[7], c + 3,
                  hist.data(), zmax.data(), zmin.data(), dv.data(),
                  hd[9] ? lengths.data() : nullptr, hd[7] ? steps.data() : nullptr,
                  scale.data(), hd[11] ? limit.data() : nullptr};
  if (hd[12] == 0) {
    blockIdx.x = 0;
    for (int64_t r = 0; r < R; ++r) {
      const int64_t b = r / K;
      g_a = full;
      g_a.R = g_a.K = 1;
      g_a.hist += b * n * 6;
      g_a.zmax += b * bstride;
      g_a.zmin += b * bstride;
      if (g_a.lengths) g_a.lengths += b;
      g_a.dv += r * L * cols;
      if (g_a.steps) g_a.steps += r;
      g_a.scale += 2 * r;
      if (g_a.limit) g_a.limit += 2 * r;
      run_wave(stacks);
    }
  } else {
    g_a = full;
    for (int64_t q = 0; 4 * q < R; ++q) {
      blockIdx.x = (unsigned)q;
      run_wave(stacks);
    }
  }
  fwrite(scale.data(), 8, scale.size(), stdout);
  if (hd[11]) fwrite(limit.data(), 4, limit.size(), stdout);
  return 0;
}
