// Driver of the host emulation of zmpc_herdt_walk_metrics_kernel
// (tests/test_herdt_metrics_emulation.py): the metrics of B walks from a binary input file,
// [B][16] doubles to stdout.  Every walk runs as wave 0 of workgroup 0 on its own slice of the
// arrays (the emulation has one wave).
// Input: int64 B, n, states stride (bytes, 0 shared), foot_ref stride (doubles, 0 shared, −1 no
// foot_ref), has_lengths, facets left, facets right; f64 h/g, count_tol, foot_length, foot_width,
// foot_spread, facets[2][16][3]; hist[B][n][6]; foot[B][n][2]; int8 states (B·stride, or n);
// foot_ref (B·stride doubles, or 2n); int64 lengths[B] when has_lengths.  Test infrastructure
// only.
#include "hip/hip_runtime.h"

EmuDim3 threadIdx, blockIdx;
uint64_t emu_buf[64];
static ucontext_t g_main, g_lane[64];
static int g_cur;
static bool g_done[64];
void emu_yield() { swapcontext(&g_lane[g_cur], &g_main); }

// v_readlane_b32: every lane reads lane l (a lockstep point, as the shuffles are)
inline int __builtin_amdgcn_readlane(int v, int l) { return __shfl(v, l); }

#include "herdt_metrics_kernel_emu.h"  // generated from csrc/herdt_metrics.hip (kernel part)

#include <cstdio>
#include <vector>

struct Args {
  int64_t n, sstride, rstride;
  const double *hist, *foot, *ref;
  const int8_t* states;
  const int64_t* len;
  double tol, hg, *out;
  emu::HerdtBox box;
};
static Args g_a;
static void lane_main() {
  emu::zmpc_herdt_walk_metrics_kernel(1, g_a.n, g_a.hist, g_a.foot, g_a.states, g_a.sstride,
                                      g_a.ref, g_a.rstride, g_a.len, g_a.tol, g_a.hg,
                                      std::sqrt(g_a.hg), g_a.box, g_a.out);
  g_done[g_cur] = true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t hd[7];
  double sc[5];
  emu::HerdtBox box{};
  bool ok = fread(hd, 8, 7, f) == 7 && fread(sc, 8, 5, f) == 5 &&
            fread(box.facets, 8, 96, f) == 96;
  const int64_t B = hd[0], n = hd[1], ss = hd[2], rs = hd[3];
  if (!ok || B < 1 || n < 1 || (ss != 0 && ss < n) || (rs > 0 && rs < 2 * n) || hd[5] < 0 ||
      hd[5] > 16 || hd[6] < 0 || hd[6] > 16)
    return 2;
  box.half_len = 0.5 * sc[2];
  box.half_wid = 0.5 * sc[3];
  box.spread2 = 2.0 * sc[4];
  box.nf[0] = (int)hd[5];
  box.nf[1] = (int)hd[6];
  const size_t nst = ss ? (size_t)(B * ss) : (size_t)n;
  const size_t nref = rs < 0 ? 0 : (rs ? (size_t)(B * rs) : (size_t)(2 * n));
  std::vector<double> hist(B * n * 6), foot(B * n * 2), ref(nref), out(B * 16);
  std::vector<int8_t> st(nst);
  std::vector<int64_t> len(B);
  ok = fread(hist.data(), 8, hist.size(), f) == hist.size() &&
       fread(foot.data(), 8, foot.size(), f) == foot.size() &&
       fread(st.data(), 1, nst, f) == nst && fread(ref.data(), 8, nref, f) == nref &&
       (!hd[4] || fread(len.data(), 8, B, f) == (size_t)B);
  fclose(f);
  if (!ok) return 2;
  std::vector<char> stacks((size_t)64 << 18);
  blockIdx.x = 0;
  for (int64_t b = 0; b < B; ++b) {
    g_a = Args{n, ss, rs < 0 ? 0 : rs, hist.data() + b * n * 6, foot.data() + b * n * 2,
               rs < 0 ? nullptr : ref.data() + b * rs, st.data() + b * ss,
               hd[4] ? len.data() + b : nullptr, sc[1], sc[0], out.data() + b * 16, box};
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
