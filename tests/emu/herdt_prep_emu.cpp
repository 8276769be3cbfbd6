// Driver of the host emulation of zmpc_herdt_prepare_kernel
// (tests/test_herdt_prepare_emulation.py): the footstep bookkeeping of B walks from a binary input
// file.  Every walk runs as wave 0 of workgroup 0 on its own slice of the arrays (the emulation has
// one wave); the batch's word is shared, as on the device.
// Input: int64 B, n, N, states stride (bytes, 0 shared), has_lengths; int8 states (B·stride, or
// n); int64 lengths[B] when has_lengths.
// Output to stdout: int32 nb_next[B][n], int32 max_steps[B], int32 batch maximum, int8
// states_out[B][n]; every output is prefilled with −7.  Test infrastructure only.
#include "hip/hip_runtime.h"

EmuDim3 threadIdx, blockIdx;
uint64_t emu_buf[64];
static ucontext_t g_main, g_lane[64];
static int g_cur;
static bool g_done[64];
void emu_yield() { swapcontext(&g_lane[g_cur], &g_main); }

// what the emulation header lacks.  The kernel's fences stand between stores by some lanes of the
// wave and loads of the same words by others: on the host, where a lane runs alone up to its next
// lockstep point, that is a lockstep point itself
inline void __threadfence_block() { (void)__any(false); }
inline int atomicMax(int32_t* p, int v) {
  const int o = *p;
  *p = std::max(*p, v);
  return o;
}

#include "herdt_prep_kernel_emu.h"  // generated from csrc/herdt_prep.hip (kernel part)

#include <cstdio>
#include <vector>

struct Args {
  int64_t n, N, sstride;
  const int8_t* states;
  const int64_t* len;
  int8_t* clean;
  int32_t *nb, *steps, *most;
};
static Args g_a;
static void lane_main() {
  emu::zmpc_herdt_prepare_kernel(1, g_a.n, (int)g_a.N, g_a.states, g_a.sstride, g_a.len,
                                 g_a.clean, g_a.nb, g_a.steps, g_a.most);
  g_done[g_cur] = true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t hd[5];
  if (fread(hd, 8, 5, f) != 5) return 2;
  const int64_t B = hd[0], n = hd[1], N = hd[2], ss = hd[3];
  if (B < 1 || n < 1 || N < 1 || (ss != 0 && ss < n)) return 2;
  const size_t nst = ss ? (size_t)(B * ss) : (size_t)n;
  std::vector<int8_t> st(nst), clean(B * n, -7);
  std::vector<int64_t> len(B);
  std::vector<int32_t> nb(B * n, -7), steps(B, -7);
  int32_t most = 0;
  bool ok = fread(st.data(), 1, nst, f) == nst && (!hd[4] || fread(len.data(), 8, B, f) == (size_t)B);
  fclose(f);
  if (!ok) return 2;
  std::vector<char> stacks((size_t)64 << 18);
  blockIdx.x = 0;
  for (int64_t b = 0; b < B; ++b) {
    g_a = Args{n, N, ss, st.data() + b * ss, hd[4] ? len.data() + b : nullptr,
               clean.data() + b * n, nb.data() + b * n, steps.data() + b, &most};
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
  fwrite(nb.data(), 4, nb.size(), stdout);
  fwrite(steps.data(), 4, steps.size(), stdout);
  fwrite(&most, 4, 1, stdout);
  fwrite(clean.data(), 1, clean.size(), stdout);
  return 0;
}
