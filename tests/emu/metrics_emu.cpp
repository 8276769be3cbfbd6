// Driver of the host emulation of zmpc_walk_metrics_kernel (tests/test_metrics_emulation.py):
// the metrics of B walks from a binary input file, [B][12] doubles to stdout.  Every walk runs as
// wave 0 of workgroup 0 on its own slice of the arrays (the emulation has one wave).
// Input: int64 B, n, bounds stride, has_lengths; f64 h/g; hist[B][n][6]; zmax, zmin (B·stride
// doubles, or 2n when the stride is 0); int64 lengths[B] when has_lengths.  Test infrastructure
// only.
#include "hip/hip_runtime.h"

EmuDim3 threadIdx, blockIdx;
uint64_t emu_buf[64];
static ucontext_t g_main, g_lane[64];
static int g_cur;
static bool g_done[64];
void emu_yield() { swapcontext(&g_lane[g_cur], &g_main); }

#include "metrics_kernel_emu.h"  // generated from csrc/metrics.hip (kernel part)

#include <cstdio>
#include <vector>

struct Args {
  int64_t n, bstride;
  const double *hist, *zmax, *zmin;
  const int64_t* len;
  double hg, *out;
};
static Args g_a;
static void lane_main() {
  emu::zmpc_walk_metrics_kernel(1, g_a.n, g_a.hist, g_a.zmax, g_a.zmin, g_a.bstride, g_a.len,
                                g_a.hg, std::sqrt(g_a.hg), g_a.out);
  g_done[g_cur] = true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t hd[4];
  double hg = 0;
  bool ok = fread(hd, 8, 4, f) == 4 && fread(&hg, 8, 1, f) == 1;
  const int64_t B = hd[0], n = hd[1], bs = hd[2];
  if (!ok || B < 1 || n < 1 || (bs != 0 && bs < 2 * n)) return 2;
  const size_t nbnd = bs ? (size_t)(B * bs) : (size_t)(2 * n);
  std::vector<double> hist(B * n * 6), zx(nbnd), zn(nbnd), out(B * 12);
  std::vector<int64_t> len(B);
  ok = fread(hist.data(), 8, hist.size(), f) == hist.size() &&
       fread(zx.data(), 8, nbnd, f) == nbnd && fread(zn.data(), 8, nbnd, f) == nbnd &&
       (!hd[3] || fread(len.data(), 8, B, f) == (size_t)B);
  fclose(f);
  if (!ok) return 2;
  std::vector<char> stacks((size_t)64 << 18);
  blockIdx.x = 0;
  for (int64_t b = 0; b < B; ++b) {
    g_a = Args{n, bs, hist.data() + b * n * 6, zx.data() + b * bs, zn.data() + b * bs,
               hd[3] ? len.data() + b : nullptr, hg, out.data() + b * 12};
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
  fwrite(out.data(), 8, out.size(), stdout);
  return 0;
}
