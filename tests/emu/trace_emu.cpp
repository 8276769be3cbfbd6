// Driver of the host emulation of zmpc_trace_add_kernel (tests/test_trace_emulation.py): the
// histories of B walks after the kernel has subtracted their traces' state responses, from a
// binary input file, [B][n][6] doubles to stdout.  Every walk runs as wave 0 of workgroup 0 on its
// own slice of the arrays (the emulation has one wave).
// Input: int64 B, n, L, cols, cx, cy, has_steps, step; f64 T, T²/2, T³/6, kx[3]; int64 steps[B]
// when has_steps; dv[B][L][cols]; hist[B][n][6].  Test infrastructure only.
#include "hip/hip_runtime.h"

EmuDim3 threadIdx, blockIdx;
uint64_t emu_buf[64];
static ucontext_t g_main, g_lane[64];
static int g_cur;
static bool g_done[64];
void emu_yield() { swapcontext(&g_lane[g_cur], &g_main); }

#include "trace_kernel_emu.h"  // generated from csrc/trace.hip (kernel part)

#include <cstdio>
#include <vector>

struct Args {
  int64_t n, L, step;
  int cols, cx, cy;
  const double *kx, *dv;
  const int64_t* steps;
  double T, T2_2, T3_6, *hist;
};
static Args g_a;
static void lane_main() {
  emu::zmpc_trace_add_kernel(1, g_a.n, g_a.kx, g_a.T, g_a.T2_2, g_a.T3_6, g_a.dv, g_a.cols, g_a.cx,
                             g_a.cy, g_a.steps, g_a.step, g_a.L, g_a.hist);
  g_done[g_cur] = true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t hd[8];
  double c[6];
  bool ok = fread(hd, 8, 8, f) == 8 && fread(c, 8, 6, f) == 6;
  const int64_t B = hd[0], n = hd[1], L = hd[2], cols = hd[3];
  if (!ok || B < 1 || n < 1 || L < 1 || cols < 1 || cols > 2) return 2;
  std::vector<int64_t> steps(B);
  std::vector<double> dv(B * L * cols), hist(B * n * 6);
  ok = (!hd[6] || fread(steps.data(), 8, B, f) == (size_t)B) &&
       fread(dv.data(), 8, dv.size(), f) == dv.size() &&
       fread(hist.data(), 8, hist.size(), f) == hist.size();
  fclose(f);
  if (!ok) return 2;
  std::vector<char> stacks((size_t)64 << 18);
  blockIdx.x = 0;
  for (int64_t b = 0; b < B; ++b) {
    g_a = Args{n, L, hd[7], (int)cols, (int)hd[4], (int)hd[5], c + 3, dv.data() + b * L * cols,
               hd[6] ? steps.data() + b : nullptr, c[0], c[1], c[2], hist.data() + b * n * 6};
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
  fwrite(hist.data(), 8, hist.size(), stdout);
  return 0;
}
