// Footstep bookkeeping of a batch of Herdt walks on the device (include/zmpc.h
// zmpc_herdt_prepare): from the support states of B different walks, what a Herdt rollout needs
// beside them — nb_next, the first element of the reference's find_nb_steps
// (zmp_controller.py:203-433) on each walk's own padded sequence (:466-469), and the most
// footsteps any horizon window of a walk holds, which sizes the rollout's kernel instance.  The
// host did both one walk at a time in a Python loop.
//
// Walk b is the sequence c[0 .. L), L = n_b + N: its n_b live states and N copies of the last one
// (the "virtual tail", never stored).  One wavefront per walk, four walks per 256-thread workgroup
// as herdt_metrics.hip; lane l of a chunk takes sample base + l with one byte load.
//
//  - nb_next runs over the chunks from the end of the walk to its start.  One __ballot each of "is
//    DOUBLE_SUPPORT" and "is SINGLE_SUPPORT"; the next such sample after lane l is the lowest set
//    bit above l, and where the chunk has none, the index carried from the later chunks: next DS,
//    next SS, and the next SS after that next DS (what a STANDING sample asks for), all three the
//    same in every lane.  The tail starts the carries: it is a DS or an SS at index n_b, or neither.
//  - The footstep count of window i is the number of phase breaks t in [i, i + N): a state change
//    other than DOUBLE → SINGLE (:561-573).  The tail is constant, so every break has t < n_b − 1
//    and the count is P(min(i + N, n_b − 1)) − P(i) with P(k) the breaks before k.  A forward
//    pass builds P from the ballot of "is a break" and keeps it in the walk's own nb_next row,
//    which the backward pass then overwrites: any n, no workspace beyond the batch's one word.
//
// Results are integers: the order of evaluation is free, two launches agree.  Rows at or past n_b
// of the input are never read.
#include "zmpc_internal.h"

namespace {

constexpr int kPrepWaves = 4;          // walks per workgroup
constexpr int kNone = 0x7fffffff;      // "no such sample"

// the bits above bit l (none for l = 63)
__device__ __forceinline__ unsigned long long bits_above(int l) { return ~((2ull << l) - 1); }

// index of the lowest set bit of m at chunk `base`, `otherwise` for an empty mask
__device__ __forceinline__ int first_at(unsigned long long m, int base, int otherwise) {
  return m ? base + __builtin_ctzll(m) : otherwise;
}

__global__ void __launch_bounds__(64 * kPrepWaves)
zmpc_herdt_prepare_kernel(int64_t B, int64_t n, int N, const int8_t* __restrict__ states,
                          int64_t sstride, const int64_t* __restrict__ lengths,
                          int8_t* __restrict__ states_out, int32_t* nb_next,
                          int32_t* __restrict__ max_steps, int32_t* __restrict__ batch_max) {
  const int lane = threadIdx.x & 63;
  // the walk is the wave's: read through the first lane, so that its length, pointers and carries
  // stay in scalar registers
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t b = (int64_t)blockIdx.x * kPrepWaves + wave;
  if (b >= B) return;  // whole waves leave: the cross-lane operations below see 64 live lanes
  const int64_t len = lengths ? lengths[b] : n;
  const int nb = (int)(len < 1 ? 1 : (len > n ? n : len));  // (n <= 2^24 is the caller's check)
  const int L = nb + N;
  const int8_t* st = states + b * sstride;
  int32_t* out = nb_next + b * n;
  const int8_t last = st[nb - 1];  // the state of the tail
  const unsigned long long below = (1ull << lane) - 1;

  if (max_steps || batch_max) {
    // P(i), the breaks at transitions t < i, into out[i] for i < n_b (every lane runs every
    // chunk: the ballot needs the whole wave)
    int run = 0;
    for (int base = 0; base < nb; base += 64) {
      const int i = base + lane;
      bool brk = false;
      if (i < nb - 1) {
        const int8_t a = st[i], c = st[i + 1];
        brk = a != c && !(a == ZMPC_DOUBLE_SUPPORT && c == ZMPC_SINGLE_SUPPORT);
      }
      const unsigned long long m = __ballot(brk);
      if (i < nb) out[i] = run + __popcll(m & below);
      run += __popcll(m);
    }
    // the counts were stored by other lanes of this wave than the ones that read them next: a
    // fence of workgroup scope orders the two (one wave, one CU, one L1; no L2 write-back)
    __threadfence_block();
    const int windows = nb - 1 > 1 ? nb - 1 : 1;
    int most = 0;
    for (int i = lane; i < windows; i += 64) {
      const int k = i + N < nb - 1 ? i + N : nb - 1;
      most = max(most, out[k] - out[i]);
    }
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) most = max(most, __shfl_xor(most, mask));
    if (lane == 0) {
      if (max_steps) max_steps[b] = most;
      if (batch_max) atomicMax(batch_max, most);
    }
    // ... and are read before the row is overwritten
    __threadfence_block();
  }

  // carried from the later chunks: the next DOUBLE_SUPPORT, the next SINGLE_SUPPORT, and the next
  // SINGLE_SUPPORT after that next DOUBLE_SUPPORT; the tail is one run from n_b on
  int c_nds = last == ZMPC_DOUBLE_SUPPORT ? nb : kNone;
  int c_nss = last == ZMPC_SINGLE_SUPPORT ? nb : kNone;
  int c_q = kNone;
  for (int base = (nb - 1) & ~63; base >= 0; base -= 64) {
    const int i = base + lane;
    const bool live = i < nb;
    const int8_t c = live ? st[i] : (int8_t)-1;
    const unsigned long long ds = __ballot(live && c == ZMPC_DOUBLE_SUPPORT);
    const unsigned long long ss = __ballot(live && c == ZMPC_SINGLE_SUPPORT);
    if (live) {
      const unsigned long long dsa = ds & bits_above(lane);
      int nds = c_nds, q = c_q;
      if (dsa) {
        const int p = __builtin_ctzll(dsa);
        nds = base + p;
        q = first_at(ss & bits_above(p), base, c_nss);
      }
      int v;
      if (c == ZMPC_STANDING)
        v = (nds == kNone || q == kNone) ? L - i : q - i - 1;
      else
        v = nds != kNone ? nds - i : L - i;
      out[i] = v;
      if (states_out) states_out[b * n + i] = c;
    }
    if (ds) {
      const int p = __builtin_ctzll(ds);
      c_q = first_at(ss & bits_above(p), base, c_nss);
      c_nds = base + p;
    }
    c_nss = first_at(ss, base, c_nss);
  }
  // rows past the walk: the window there is constant and holds no footstep
  for (int64_t i = nb + lane; i < n; i += 64) {
    out[i] = 1;
    if (states_out) states_out[b * n + i] = last;
  }
}

}  // namespace

hipError_t zmpc_launch_herdt_prepare(const zmpc_plan* p, int64_t B, int64_t n,
                                     const int8_t* states, int64_t sstride,
                                     const int64_t* lengths, int8_t* states_out,
                                     int32_t* nb_next, int32_t* max_steps, int32_t* batch_max,
                                     hipStream_t s) {
  if (B == 0) return hipSuccess;
  // one workgroup per four walks (B <= 2^31 − 1 is the caller's check, so the grid fits)
  const unsigned grid = (unsigned)((B + kPrepWaves - 1) / kPrepWaves);
  hipLaunchKernelGGL(zmpc_herdt_prepare_kernel, dim3(grid), dim3(64 * kPrepWaves), 0, s, B, n,
                     p->N, states, sstride, lengths, states_out, nb_next, max_steps, batch_max);
  return hipGetLastError();
}
