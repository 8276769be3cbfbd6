// What the two translation units of the unconstrained rollout share (rollout.hip: the one-wave,
// split and fused-metrics kernels; rollout_long.hip: the wide and chunk kernels): 3×3 algebra, the
// DPP affine scan, the LDS layouts, the kernel argument struct, bound staging and the direct
// correlations.  Everything sits in an anonymous namespace, so each unit gets its own copy and the
// kernels' symbols keep the names they had in one unit.
#pragma once

#include <algorithm>
#include <cstdint>

#include "zmpc_internal.h"

namespace {

struct Mat3 {
  double m[9];
};

__device__ __forceinline__ Mat3 matmul3(const Mat3& a, const Mat3& b) {
  Mat3 c;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      c.m[3 * i + j] = fma(a.m[3 * i + 0], b.m[0 + j],
                           fma(a.m[3 * i + 1], b.m[3 + j], a.m[3 * i + 2] * b.m[6 + j]));
  return c;
}

__device__ __forceinline__ void matvec3(const Mat3& a, const double* x, double* y) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
    y[i] = fma(a.m[3 * i + 0], x[0], fma(a.m[3 * i + 1], x[1], a.m[3 * i + 2] * x[2]));
}

// A double moved across lanes by DPP (two 32-bit halves); `ctrl` a DPP control word,
// row_mask the rows written (the others keep 0), out-of-row reads 0 (bound_ctrl).
template <int CTRL, int ROWS>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROWS, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROWS, 0xF, true);
  return __hiloint2double(hi, lo);
}

// Inclusive affine Kogge-Stone scan over the 64 lanes, T_l = Σ_{m≤l} P^(l−m) s_m, on the VALU's
// DPP lane moves instead of LDS-pipe shuffles: four row_shr levels (1, 2, 4, 8) inside each
// 16-lane row with the uniform P^(2^r), then row_bcast:15 (rows 1, 3 take lanes 15, 47) and
// row_bcast:31 (rows 2, 3 take lane 31) with each lane's own power P^k from the plan
// (pw = [33][9], k = its distance to the source lane).
__device__ __forceinline__ void dpp_level(double* sv, const Mat3& M, double u0, double u1,
                                          double u2) {
  const double u[3] = {u0, u1, u2};
  double t[3];
  matvec3(M, u, t);
  sv[0] += t[0];
  sv[1] += t[1];
  sv[2] += t[2];
}

__device__ __forceinline__ void scan_dpp(double* sv, int lane, const double* __restrict__ Pp,
                                         const double* __restrict__ pw) {
#define ZMPC_DPP_ROW(R2, CTRL)                                                             \
  {                                                                                        \
    Mat3 Pd;                                                                               \
    _Pragma("unroll") for (int q = 0; q < 9; ++q) Pd.m[q] = Pp[(R2) * 9 + q];              \
    dpp_level(sv, Pd, dpp_f64<CTRL, 0xF>(sv[0]), dpp_f64<CTRL, 0xF>(sv[1]),                \
              dpp_f64<CTRL, 0xF>(sv[2]));                                                  \
  }
  ZMPC_DPP_ROW(0, 0x111)  // row_shr:1
  ZMPC_DPP_ROW(1, 0x112)  // row_shr:2
  ZMPC_DPP_ROW(2, 0x114)  // row_shr:4
  ZMPC_DPP_ROW(3, 0x118)  // row_shr:8
#undef ZMPC_DPP_ROW
  {  // rows 1 and 3 take lane 15 / 47 at distance (lane & 15) + 1
    const double* m = pw + ((lane & 15) + 1) * 9;
    Mat3 M;
#pragma unroll
    for (int q = 0; q < 9; ++q) M.m[q] = m[q];
    dpp_level(sv, M, dpp_f64<0x142, 0xA>(sv[0]), dpp_f64<0x142, 0xA>(sv[1]),
              dpp_f64<0x142, 0xA>(sv[2]));
  }
  {  // rows 2 and 3 take lane 31 at distance lane − 31
    const double* m = pw + (lane >= 32 ? lane - 31 : 0) * 9;
    Mat3 M;
#pragma unroll
    for (int q = 0; q < 9; ++q) M.m[q] = m[q];
    dpp_level(sv, M, dpp_f64<0x143, 0xC>(sv[0]), dpp_f64<0x143, 0xC>(sv[1]),
              dpp_f64<0x143, 0xC>(sv[2]));
  }
}

// Reference state update x⁺ = A x + B u (zmp_controller.py:199).
__device__ __forceinline__ void lipm_step(const LipmConsts& c, const double* x, double u,
                                          double* y) {
  y[0] = x[0] + c.T * x[1] + c.T2_2 * x[2] + c.T3_6 * u;
  y[1] = x[1] + c.T * x[2] + c.T2_2 * u;
  y[2] = x[2] + c.T * u;
}

// LDS layout of z_ref: lane l's chunk starts at t = l·CW; for even CW one pad double per CW
// keeps the 64 lanes' ds_read_b64 on distinct banks (lane stride CW+1 doubles, odd).
template <int CW>
struct ZrLayout {
  static constexpr int kPad = (CW % 2 == 0) ? 1 : 0;
  __host__ __device__ static constexpr int idx(int t) { return t + kPad * (t / CW); }
  // idx of a runtime row 0 ≤ t < 32768 (the split kernels: two areas of lzp doubles within
  // 64 KiB).  CW = 6 is the one width whose t / CW is no shift: ⌊t·10923 / 2^16⌋ = ⌊t / 6⌋ below
  // 2^16 / (6·10923 − 2^16) = 32768, a 24-bit multiply instead of the quarter-rate v_mul_hi.
  __device__ static __forceinline__ int idx_row(int t) {
    if constexpr (CW == 6)
      return t + (int)(__umul24((unsigned)t, 10923u) >> 16);
    else
      return idx(t);
  }
};

// History staging of the split kernels: row 0 the initial state, row m + 1 the state after
// step m (6 doubles: both axes), written by the lane owning step m.  For even CW the lanes'
// rows are CW·48 bytes apart, a multiple of 128 B, so the 16 lanes of a ds_write_b64 group hit
// one or two banks (16-way at CW = 8); two pad doubles after every 2·CW rows (every second
// lane) spread them over eight bank pairs (2-way, as odd CW) for CW = 2..8, at 2 % more LDS
// (after every CW rows the same 2-way costs twice the pad, which at n = 476 took one of the seven
// workgroups a CU holds).  The copy-out skips the pads.
template <int CW>
struct HistLayout {
  static constexpr int kPad = (CW % 2 == 0) ? 2 : 0;  // doubles after every 2·CW step rows
  static constexpr int kSpan = 2 * CW;
  __host__ __device__ static constexpr int row(int r) {  // first double of staged row r
    return r * 6 + (r >= 1 ? kPad * ((r - 1) / kSpan) : 0);
  }
  __host__ __device__ static constexpr size_t doubles(int n) {
    return hist_doubles(CW, n);  // (dispatch.h: it enters the launch rules' LDS sizes)
  }
};

struct RolloutArgs {
  int kc, kcp, lz, lzp, n;
  int64_t B;
  LipmConsts lc;
  const double* k;
  const double* kx;
  const double* zmax;
  const double* zmin;
  int64_t bstride;
  const double* x0;
  const double* kick;
  int64_t kick_step;
  double* hist;
  int32_t* status;
  const double* scanP;  // [8][kScanLevels][9]: (Ā^C)^(2^r) for C = 1..8 (plan), or null
  int dbg;
  int srows;  // unused; it stays because removing a field moves the argument offsets of every
              // kernel (and with them every kernel's machine code)
  const int64_t* kick_steps;  // [B] per-walk kick steps (ragged walks), or null: kick_step
  const double* fsh;  // shared CoP (bounds stride 0): f of both axes, [2][fstride], or null
  int fstride;
  const double2* fft_tw;  // plan twiddles e^{−2πi m/kFftPT} (FFT correlation, wide kernel)
  const double2* fft_g;   // plan gain spectrum DFT(g)/P for this launch's P
  const double* kffa;     // plan fast-FIR taps [kffa_rows(N)][4] (axis_correlate_ffa)
  int kfm;                // fast-FIR steps per walk, ⌈(N+1)/2⌉ rounded up to the unroll
  const double* ksum;     // plan suffix sums of k [ksum_rows(N)] (axis_correlate_sparse), or null
  int hN;                 // horizon N (ksum layout)
  int64_t pf_ahead;       // one walk per workgroup: touch walk b + pf_ahead's bounds (the next
                          // dispatch round's) into the caches early; 0 = off
  unsigned long long* tl;  // diagnostics build only (ZMPC_ROLLOUT_TL): per-walk phase stamps
};

// Diagnostic ablation bits (ZMPC_DEBUG_ROLLOUT: 1 no correlation, 2 no scan, 4 no history
// stores, 8 bounds from row 0) — compiled only into the diagnostics build (make diag,
// -DZMPC_DIAG); the product library has none of them.
#ifdef ZMPC_DIAG
__device__ __forceinline__ int dbgb(const RolloutArgs& a, int bit) { return a.dbg & bit; }
// phase stamps of walk b (wave 0's view, the 100 MHz constant clock): [0] start, [1] bounds in
// LDS, [2] correlation done, [3] history staged, [4] copy-out issued
__device__ __forceinline__ void tl_stamp(const RolloutArgs& a, int64_t b, int k) {
  if (a.tl != nullptr && threadIdx.x == 0) a.tl[b * 5 + k] = (unsigned long long)wall_clock64();
}
#else
__device__ __forceinline__ constexpr int dbgb(const RolloutArgs&, int) { return 0; }
__device__ __forceinline__ void tl_stamp(const RolloutArgs&, int64_t, int) {}
#endif

// a 16-byte store with the non-temporal hint (streamed past the caches)
__device__ __forceinline__ void st_nt2(double2* p, double2 v) {
  typedef double v2d __attribute__((ext_vector_type(2)));
  const v2d t = {v.x, v.y};
  __builtin_nontemporal_store(t, reinterpret_cast<v2d*>(p));
}

// The kick step of walk b: per walk (ragged batches) or the launch-wide one.
__device__ __forceinline__ int64_t kick_step_of(const RolloutArgs& a, int64_t b) {
  return a.kick_steps != nullptr ? a.kick_steps[b] : a.kick_step;
}


// Bounds of one walk held in registers: PF rounds of 64 samples, one 16-B (x, y) pair of
// each bound array per lane and round.
template <int PF>
struct BoundRegs {
  double2 hi[PF], lo[PF];
};

template <int PF>
__device__ __forceinline__ void load_bounds(const RolloutArgs& a, int64_t b, int lane,
                                            BoundRegs<PF>& r) {
  const double2* zmx = reinterpret_cast<const double2*>(a.zmax + b * a.bstride);
  const double2* zmn = reinterpret_cast<const double2*>(a.zmin + b * a.bstride);
#pragma unroll
  for (int u = 0; u < PF; ++u) {
    const int t = u * 64 + lane;
    if (t < a.n) {
      r.hi[u] = zmx[t];
      r.lo[u] = zmn[t];
    }
  }
}

// z_ref = (z_max + z_min) / 2 into the (padded) LDS layout, then the last row repeated up to
// lz (the window padding of zmp_controller.py:81-88).
template <int CW, int PF>
__device__ __forceinline__ void store_zref(const RolloutArgs& a, const BoundRegs<PF>& r,
                                           double* zr0, double* zr1, int lane) {
  using ZL = ZrLayout<CW>;
#pragma unroll
  for (int u = 0; u < PF; ++u) {
    const int t = u * 64 + lane;
    if (t < a.n) {
      zr0[ZL::idx(t)] = (r.hi[u].x + r.lo[u].x) / 2;
      zr1[ZL::idx(t)] = (r.hi[u].y + r.lo[u].y) / 2;
    }
  }
  // the last sample lives in lane (n-1)%64 of round (n-1)/64: broadcast it
  const int ul = (a.n - 1) >> 6, ll = (a.n - 1) & 63;
  double h0 = 0.0, h1 = 0.0, l0 = 0.0, l1 = 0.0;
#pragma unroll
  for (int u = 0; u < PF; ++u)
    if (u == ul) {
      h0 = r.hi[u].x;
      h1 = r.hi[u].y;
      l0 = r.lo[u].x;
      l1 = r.lo[u].y;
    }
  h0 = __shfl(h0, ll, 64);
  h1 = __shfl(h1, ll, 64);
  l0 = __shfl(l0, ll, 64);
  l1 = __shfl(l1, ll, 64);
  const double last0 = (h0 + l0) / 2, last1 = (h1 + l1) / 2;
  for (int t = a.n + lane; t < a.lz; t += 64) {
    zr0[ZL::idx(t)] = last0;
    zr1[ZL::idx(t)] = last1;
  }
}

// f for lane l's CW timesteps of one pass starting at i0 (both axes).
// k is read from the wave's LDS copy (ks): wave-uniform broadcast reads keep every lgkm
// operation of the loop an in-order LDS access, so waits stay counted (a scalar load here
// would force lgkmcnt(0) drains of the z_ref reads in flight).
template <int CW>
__device__ __forceinline__ void correlate(const RolloutArgs& a, const double* ks,
                                          const double* zr0, const double* zr1, int i0,
                                          double* a0, double* a1) {
  using ZL = ZrLayout<CW>;
  // i0 is a multiple of CW, so idx(i0 + c) = idx(i0) + idx(c): compile-time offsets
  const double* z0 = zr0 + ZL::idx(i0);
  const double* z1 = zr1 + ZL::idx(i0);
  double w0[CW], w1[CW];
#pragma unroll
  for (int m = 0; m < CW; ++m) {
    a0[m] = 0.0;
    a1[m] = 0.0;
    w0[m] = z0[ZL::idx(1 + m)];
    w1[m] = z1[ZL::idx(1 + m)];
  }
  const double* k = ks;
  for (int j = 0; j < a.kc; j += CW) {
#pragma unroll
    for (int jj = 0; jj < CW; ++jj) {
      const double kj = k[j + jj];
#pragma unroll
      for (int m = 0; m < CW; ++m) {
        a0[m] = fma(kj, w0[(jj + m) % CW], a0[m]);
        a1[m] = fma(kj, w1[(jj + m) % CW], a1[m]);
      }
      w0[jj] = z0[ZL::idx(1 + jj + CW)];
      w1[jj] = z1[ZL::idx(1 + jj + CW)];
    }
    z0 += CW + ZL::kPad;
    z1 += CW + ZL::kPad;
  }
}

// One axis of the same correlation for lane l's CW timesteps (the split and wide kernels: a wave
// per axis), k on wave-uniform addresses.
template <int CW>
__device__ __forceinline__ void axis_correlate(const RolloutArgs& a, const double* __restrict__ ks,
                                               const double* zr, int lane, double* f) {
  using ZL = ZrLayout<CW>;
  const double* z = zr + ZL::idx(lane * CW);
  double w[CW];
#pragma unroll
  for (int m = 0; m < CW; ++m) {
    f[m] = 0.0;
    w[m] = z[ZL::idx(1 + m)];
  }
  for (int j = 0; j < (dbgb(a, 1) ? 0 : a.kc); j += CW) {
#pragma unroll
    for (int jj = 0; jj < CW; ++jj) {
      const double kj = ks[j + jj];
#pragma unroll
      for (int m = 0; m < CW; ++m) f[m] = fma(kj, w[(jj + m) % CW], f[m]);
      w[jj] = z[ZL::idx(1 + jj + CW)];
    }
    z += CW + ZL::kPad;
  }
}

// v_readlane of a double at a wave-uniform lane index
__device__ __forceinline__ double readlane_f64(double v, int l) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, l);
  const unsigned hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), l);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// Resident workgroups per CU of a kernel at an LDS size (a small per-host-thread cache keyed by
// kernel, block size and LDS; every device of the pool is the same gfx950 part).
int occupancy(const void* kernel, int threads, size_t lds) {
  struct Entry {
    const void* k;
    size_t lds;
    int threads, occ;
  };
  static thread_local Entry cache[32];
  static thread_local int used = 0;
  const int n = used < 32 ? used : 32;
  for (int i = 0; i < n; ++i)
    if (cache[i].k == kernel && cache[i].lds == lds && cache[i].threads == threads)
      return cache[i].occ;
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, threads, lds) != hipSuccess)
    occ = 0;
  cache[used++ % 32] = Entry{kernel, lds, threads, occ};
  return occ;
}

}  // namespace
