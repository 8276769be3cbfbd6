// Unconstrained Wieber rollout of long walks (more than 64·8+1 samples): the wide kernel (2·W waves
// per walk, direct, sparse-difference or FFT correlation) up to 64·8·8+1 samples and the chunk
// kernel (one wave per walk) for any length.  The arithmetic per step is rollout.hip's; which
// kernel and geometry a call takes is dispatch.h choose_unc's, asked once in rollout.hip, whose
// launcher hands the Wide and Chunk cases to zmpc_launch_rollout_long below.
#include "rollout_common.h"

namespace {

// ---- FFT correlation ---------------------------------------------------------------------------
// f_i =Σ_{d=1..N} g[d] s[i+d] with g[d] = k_{d−1} and s = z_x + i z_y (both axes in one complex
// signal; g is real, so Re and Im stay separate): a circular cross-correlation of period
// P = 2^p ≥ n − 1 + N, so no output i ≤ n − 2 wraps.  Its spectrum is S·conj(DFT g); with
// T = conj(S)·DFT(g)/P (the plan's fft_g) f = conj(DFT(T)): two forward transforms.  O(P log P)
// instead of the direct form's N per output (N = 512: ≈10× fewer FP64 operations).
// Stockham autosort, radix 4 (+ one radix-2 stage when p is odd), in place in LDS: each stage
// reads all of its inputs, barrier, writes, barrier.  NT threads, E = P/NT points each.
__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
  return make_double2(fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x));
}

// 8-point DFT in registers, forward sign (e^{−2πi/8} = (1 − i)/√2).
__device__ __forceinline__ void dft8(double2 (&v)[8]) {
  constexpr double h = 0.70710678118654752440;  // 1/√2
  double2 a[4], c[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    a[r] = make_double2(v[r].x + v[r + 4].x, v[r].y + v[r + 4].y);
    c[r] = make_double2(v[r].x - v[r + 4].x, v[r].y - v[r + 4].y);
  }
  // c1 ·= w8, c2 ·= −i, c3 ·= w8³
  c[1] = make_double2((c[1].x + c[1].y) * h, (c[1].y - c[1].x) * h);
  c[2] = make_double2(c[2].y, -c[2].x);
  c[3] = make_double2((c[3].y - c[3].x) * h, -(c[3].x + c[3].y) * h);
  // 4-point DFTs: evens from a, odds from c
  auto dft4 = [](const double2 (&q)[4], double2& y0, double2& y1, double2& y2, double2& y3) {
    const double2 t0 = make_double2(q[0].x + q[2].x, q[0].y + q[2].y);
    const double2 t1 = make_double2(q[0].x - q[2].x, q[0].y - q[2].y);
    const double2 t2 = make_double2(q[1].x + q[3].x, q[1].y + q[3].y);
    const double2 t3 = make_double2(q[1].y - q[3].y, q[3].x - q[1].x);  // (q1 − q3)·(−i)
    y0 = make_double2(t0.x + t2.x, t0.y + t2.y);
    y2 = make_double2(t0.x - t2.x, t0.y - t2.y);
    y1 = make_double2(t1.x + t3.x, t1.y + t3.y);
    y3 = make_double2(t1.x - t3.x, t1.y - t3.y);
  };
  dft4(a, v[0], v[2], v[4], v[6]);
  dft4(c, v[1], v[3], v[5], v[7]);
}

// In-place-in-registers Stockham FFT of P = 2^p points (forward), radix 8 (+ one radix-2 or
// radix-4 stage when p mod 3 ≠ 0), by the first NF = P/8 threads of the workgroup: thread t
// holds points t + NF·u (u = 0..7) on entry and the transform's points t + NF·u on exit, so
// the first stage reads and the last stage writes registers; between stages the points pass
// through LDS (buf, P complex).  Every thread of the workgroup must call it (barriers).
template <int P>
__device__ __forceinline__ void fft8(double2 (&v)[8], double2* buf,
                                     const double2* __restrict__ tw, int tid) {
  constexpr int NF = P / 8;
  constexpr int LOGP = __builtin_ctz(P);
  constexpr int A8 = LOGP / 3;  // radix-8 stages
  constexpr int RL = LOGP % 3;  // last stage radix 2^RL (0: none)
  constexpr int R = 1 << RL;
  const bool act = tid < NF;
#pragma unroll
  for (int st = 0; st < A8; ++st) {
    const int Ns = 1 << (3 * st);
    const int k = tid & (Ns - 1);
    if (act) {
      if (st > 0) {
        const double2 w1 = tw[k * (kFftPT / (8 * Ns))];
        const double2 w2 = cmul(w1, w1), w3 = cmul(w2, w1), w4 = cmul(w2, w2);
        v[1] = cmul(v[1], w1);
        v[2] = cmul(v[2], w2);
        v[3] = cmul(v[3], w3);
        v[4] = cmul(v[4], w4);
        v[5] = cmul(v[5], cmul(w4, w1));
        v[6] = cmul(v[6], cmul(w4, w2));
        v[7] = cmul(v[7], cmul(w4, w3));
      }
      dft8(v);
    }
    const bool last = (st == A8 - 1) && RL == 0;
    if (!last) {
      if (act) {
        const int base = ((tid - k) << 3) + k;
#pragma unroll
        for (int r = 0; r < 8; ++r) buf[base + r * Ns] = v[r];
      }
      __syncthreads();
      if (act) {
        if (st + 1 < A8) {
#pragma unroll
          for (int r = 0; r < 8; ++r) v[r] = buf[tid + r * NF];
        } else {
          // the radix-R stage: butterflies j = tid + NF·m (m < 8/R), inputs j + r·P/R
#pragma unroll
          for (int m = 0; m < 8 / R; ++m)
#pragma unroll
            for (int r = 0; r < R; ++r) v[m * R + r] = buf[tid + NF * m + r * (P / R)];
        }
      }
      __syncthreads();
    }
  }
  if constexpr (RL > 0) {
    // last stage (Ns = P/R, k = j): twiddles w^{r j}, w = e^{−2πi/P}; outputs j + r·P/R =
    // tid + NF·(m + r·8/R)
    double2 y[8];
    if (act) {
#pragma unroll
      for (int m = 0; m < 8 / R; ++m) {
        const int j = tid + NF * m;
        const double2 w1 = tw[j * (kFftPT / P)];
        double2 q[4];
#pragma unroll
        for (int r = 0; r < R; ++r) q[r] = v[m * R + r];
        if constexpr (R == 2) {
          q[1] = cmul(q[1], w1);
          y[m] = make_double2(q[0].x + q[1].x, q[0].y + q[1].y);
          y[m + 4] = make_double2(q[0].x - q[1].x, q[0].y - q[1].y);
        } else {
          const double2 w2 = cmul(w1, w1), w3 = cmul(w2, w1);
          q[1] = cmul(q[1], w1);
          q[2] = cmul(q[2], w2);
          q[3] = cmul(q[3], w3);
          const double2 t0 = make_double2(q[0].x + q[2].x, q[0].y + q[2].y);
          const double2 t1 = make_double2(q[0].x - q[2].x, q[0].y - q[2].y);
          const double2 t2 = make_double2(q[1].x + q[3].x, q[1].y + q[3].y);
          const double2 t3 = make_double2(q[1].y - q[3].y, q[3].x - q[1].x);
          y[m] = make_double2(t0.x + t2.x, t0.y + t2.y);
          y[m + 2] = make_double2(t1.x + t3.x, t1.y + t3.y);
          y[m + 4] = make_double2(t0.x - t2.x, t0.y - t2.y);
          y[m + 6] = make_double2(t1.x - t3.x, t1.y - t3.y);
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = y[u];
    }
  }
}

// s (points t + NF·u in v, NF = P/8 threads) → f = conj(DFT(conj(DFT s)·G)) into buf (P complex,
// natural order), G = the plan's DFT(g)/P.  Every thread of the workgroup must call it.
template <int P>
__device__ __forceinline__ void fft_correlate8(double2 (&v)[8], double2* buf,
                                               const double2* __restrict__ tw,
                                               const double2* __restrict__ G, int tid) {
  constexpr int NF = P / 8;
  fft8<P>(v, buf, tw, tid);
  if (tid < NF) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const double2 S = v[u], g = G[tid + NF * u];
      v[u] = make_double2(fma(S.x, g.x, S.y * g.y), fma(S.x, g.y, -S.y * g.x));  // conj(S)·g
    }
  }
  __syncthreads();  // the last exchange's reads are done before buf is rewritten
  fft8<P>(v, buf, tw, tid);
  if (tid < NF) {
#pragma unroll
    for (int u = 0; u < 8; ++u) buf[tid + NF * u] = v[u];
  }
  __syncthreads();
}

// The sparse-difference correlation (axis_correlate_sparse) for the wide kernel: the changes a
// lane's outputs need lie up to N − 1 samples ahead, in other waves' ranges, so each axis's
// changes go to an LDS list first (per-wave counts → prefix → positions, deterministic order)
// and every lane walks its axis's list.  Returns false, uniformly over the workgroup, when
// either axis has more than kSparseMaxWide changes (both axes then take the dense form: the FFT
// correlates them together; kSparseMaxWide is in dispatch.h).  Both calls' barriers are reached by
// every thread.

template <int CW, int W>
__device__ __forceinline__ bool wide_correlate_sparse(const RolloutArgs& a, const double* zr,
                                                      const double* Ts, double* ld, int* lm,
                                                      int (*scnt)[W], int axis, int w, int lane,
                                                      double* f) {
  using ZL = ZrLayout<CW>;
  const int s = (w * 64 + lane) * CW;
  const double* z = zr + ZL::idx(s);
  double gv[CW + 1], d[CW];
  unsigned long long mk[CW];
  int cnt = 0;
#pragma unroll
  for (int j = 0; j <= CW; ++j) gv[j] = z[ZL::idx(j)];
#pragma unroll
  for (int q = 0; q < CW; ++q) {
    d[q] = gv[q + 1] - gv[q];
    mk[q] = __ballot(d[q] != 0.0);
    cnt += __popcll(mk[q]);
  }
  if (lane == 0) scnt[axis][w] = cnt;
  __syncthreads();
  int tot0 = 0, tot1 = 0, base = 0;
#pragma unroll
  for (int v = 0; v < W; ++v) {
    tot0 += scnt[0][v];
    tot1 += scnt[1][v];
    if (v < w) base += scnt[axis][v];
  }
  if (tot0 > kSparseMaxWide || tot1 > kSparseMaxWide || dbgb(a, 1)) return false;
  const unsigned long long lt = (1ull << lane) - 1ull;
  double* la = ld + axis * kSparseMaxWide;
  int* lma = lm + axis * kSparseMaxWide;
#pragma unroll
  for (int q = 0; q < CW; ++q) {
    if ((mk[q] >> lane) & 1ull) {
      const int pos = base + __popcll(mk[q] & lt);
      la[pos] = d[q];
      lma[pos] = s + q;
    }
    base += __popcll(mk[q]);
  }
  __syncthreads();
  const int N = a.hN, tot = axis ? tot1 : tot0;
  const double S0 = Ts[ksum_s0(N)];
#pragma unroll
  for (int r = 0; r < CW; ++r) f[r] = S0 * gv[r + 1];
  for (int c = 0; c < tot; ++c) {
    const int e = min(max(lma[c] - s, 0), N + CW - 1);
    const double dv = la[c];
    const double* p = Ts + e + 9 - CW;
#pragma unroll
    for (int r = 0; r < CW; ++r) f[r] = fma(p[CW - 1 - r], dv, f[r]);
  }
  return true;
}

// Long walks (64·8+1 < n ≤ 64·8·8+1): the split-axis structure widened to W waves per axis
// (workgroup = 2·W waves; wave w of an axis owns timesteps [w·64·CW, (w+1)·64·CW)).  Each
// wave scans its range from a zero state; the true start state of wave w is chained over the
// waves' end states with M = (Ā^CW)^64 (plan level 6), and lane l adds (Ā^CW)^(l+1)·x_start by
// binary powering.  History staged through the z_ref area in rounds (replay per round).
template <int CW, int W, int E = 0>
__global__ void __launch_bounds__(128 * W, E == 4 ? 6 : 4) zmpc_rollout_unc_wide_kernel(RolloutArgs a) {
  using ZL = ZrLayout<CW>;
  constexpr int NT = 128 * W;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ int flag[2 * W];
  __shared__ double send[2][W][3];  // zero-start end state of each wave (wave 0: true)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int axis = wv / W, w = wv % W;
  const int64_t b = blockIdx.x;
  const int n = a.n, nsteps = n - 1;
  double* zr0 = smem;
  double* zr1 = zr0 + a.lzp;
  __shared__ int scnt[2][W];  // per-wave z_ref change counts (sparse attempt)
  // (diagnostics timeline: [0] start, [1] correlation inputs staged, [2] correlation done,
  // [3] scan and cross-wave chain done, [4] last copy-out issued)
  tl_stamp(a, b, 0);
  double* Ts = smem + 2 * a.lzp;  // sparse attempt: suffix sums, then the change lists
  double* ld = Ts + ((ksum_rows(a.hN) + 1) & ~1);
  int* lm = reinterpret_cast<int*>(ld + 2 * kSparseMaxWide);
  // ---- 1. z_ref rows + window padding (zmp_controller.py:81-88) ----------------------------
  double f[CW];
  const int mbeg = (w * 64 + lane) * CW;
  // next-dispatch-round prefetch (as split_walk): one double per 64 B of walk b + pf_ahead's
  // bounds, results kept alive to the end and never used
  double pf0 = 0.0, pf1 = 0.0;
  if (a.pf_ahead > 0 && b + a.pf_ahead < a.B) {
    const int nd = 2 * n, half = NT / 2, tl = tid % half;
    const double* src = (tid < half ? a.zmax : a.zmin) + (b + a.pf_ahead) * a.bstride;
    pf0 = src[min(tl * 8, nd - 1)];
    pf1 = src[min((tl + half) * 8, nd - 1)];
  }
  // the sparse-difference correlation first (piecewise-constant CoP), else the dense forms;
  // the FFT form stages only the rows the change scan reads (its transform loads its own)
  bool dense = true;
  if constexpr (E > 0) {
    if (a.ksum != nullptr) {
      const double2* zmx = reinterpret_cast<const double2*>(a.zmax + b * a.bstride);
      const double2* zmn = reinterpret_cast<const double2*>(a.zmin + b * a.bstride);
      // the bound loads issued GB rows per thread at a time ahead of their LDS stores (one HBM
      // round trip per group instead of per row; two-row groups at CW ≥ 7, whose state would
      // spill at four)
      constexpr int lzs = W * 64 * CW + 1, IT = (lzs + NT - 1) / NT, GB = CW >= 7 ? 2 : 4;
#pragma unroll
      for (int u0 = 0; u0 < IT; u0 += GB) {
        double2 hi[GB], lo[GB];
#pragma unroll
        for (int u = 0; u < GB; ++u) {
          const int tc = min(tid + (u0 + u) * NT, n - 1);  // padding = last row
          hi[u] = zmx[tc];
          lo[u] = zmn[tc];
        }
        if (u0 == 0)
          for (int i = tid; i < ksum_rows(a.hN); i += NT) Ts[i] = a.ksum[i];
#pragma unroll
        for (int u = 0; u < GB; ++u) {
          const int t = tid + (u0 + u) * NT;
          if (u0 + u < IT && t < lzs) {
            zr0[ZL::idx(t)] = (hi[u].x + lo[u].x) / 2;
            zr1[ZL::idx(t)] = (hi[u].y + lo[u].y) / 2;
          }
        }
      }
      __syncthreads();
      tl_stamp(a, b, 1);
      dense = !wide_correlate_sparse<CW, W>(a, axis ? zr1 : zr0, Ts, ld, lm, scnt, axis, w, lane,
                                             f);
    }
  }
  if (!dense) {
  } else if constexpr (E > 0) {
    // FFT correlation: s[t] = (z_x, z_y) for t < P (rows past n − 1: the last row)
    double2* buf = reinterpret_cast<double2*>(smem);
    const double2* zmx = reinterpret_cast<const double2*>(a.zmax + b * a.bstride);
    const double2* zmn = reinterpret_cast<const double2*>(a.zmin + b * a.bstride);
    constexpr int P = NT * E, NF = P / 8;  // the first NF threads run the transform
    double2 v[8];
    if (tid < NF) {
      double2 hi[8], lo[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int tc = min(tid + NF * u, n - 1);
        hi[u] = zmx[tc];
        lo[u] = zmn[tc];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        v[u] = make_double2((hi[u].x + lo[u].x) / 2, (hi[u].y + lo[u].y) / 2);
    }
    fft_correlate8<P>(v, buf, a.fft_tw, a.fft_g, tid);
#pragma unroll
    for (int q = 0; q < CW; ++q) {
      const double2 c = buf[min(mbeg + q, NT * E - 1)];
      f[q] = axis ? -c.y : c.x;  // f = conj(DFT T): f_y = −Im
    }
  } else {
    const double2* zmx = reinterpret_cast<const double2*>(a.zmax + b * a.bstride);
    const double2* zmn = reinterpret_cast<const double2*>(a.zmin + b * a.bstride);
    for (int t0 = 0; t0 < a.lz; t0 += 4 * NT) {
      double2 hi[4], lo[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int tc = dbgb(a, 8) ? 0 : min(t0 + u * NT + tid, n - 1);  // padding = last row
        hi[u] = zmx[tc];
        lo[u] = zmn[tc];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = t0 + u * NT + tid;
        if (t < a.lz) {
          zr0[ZL::idx(t)] = (hi[u].x + lo[u].x) / 2;
          zr1[ZL::idx(t)] = (hi[u].y + lo[u].y) / 2;
        }
      }
    }
    if (a.ksum != nullptr)
      for (int i = tid; i < ksum_rows(a.hN); i += NT) Ts[i] = a.ksum[i];
    __syncthreads();
    // ---- 2. correlation ----------------------------------------------------------------------
    if (a.ksum == nullptr ||
        !wide_correlate_sparse<CW, W>(a, axis ? zr1 : zr0, Ts, ld, lm, scnt, axis, w, lane, f))
      axis_correlate<CW>(a, a.k, (axis ? zr1 : zr0) + ZL::idx(w * 64 * CW), lane, f);
  }
  tl_stamp(a, b, 2);
  const double* xb = a.x0 + b * 6 + 3 * axis;
  const double xi[3] = {xb[0], xb[1], xb[2]};
  const double kk = (axis == 1 && a.kick != nullptr) ? a.kick[b] : 0.0;
  // ---- 3. scan: per-wave zero-start Kogge-Stone, then the cross-wave offsets ---------------
  const int64_t kick_step = (axis == 1) ? kick_step_of(a, b) : -1;
  const LipmConsts lc = a.lc;
  const double kx0 = a.kx[0], kx1 = a.kx[1], kx2 = a.kx[2];
  const double Bv[3] = {lc.T3_6, lc.T2_2, lc.T};
  Mat3 Ab;
  {
    const double A[9] = {1.0, lc.T, lc.T2_2, 0.0, 1.0, lc.T, 0.0, 0.0, 1.0};
    const double kx[3] = {kx0, kx1, kx2};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Ab.m[3 * i + j] = A[3 * i + j] - Bv[i] * kx[j];
  }
  double sv[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < CW; ++q) {
    if (mbeg + q < nsteps) {
      double t[3];
      matvec3(Ab, sv, t);
      sv[0] = fma(Bv[0], f[q], t[0]);
      sv[1] = fma(Bv[1], f[q], t[1]);
      sv[2] = fma(Bv[2], f[q], t[2]);
      if (mbeg + q == kick_step) sv[1] -= kk;
    }
  }
  const double* Pp = a.scanP + (CW - 1) * kScanStride;  // (Ā^CW)^(2^r), r = 0..6
  if (lane == 0 && w == 0) {
    double t[3];
    Mat3 P;
#pragma unroll
    for (int q = 0; q < 9; ++q) P.m[q] = Pp[q];
    matvec3(P, xi, t);
    for (int i = 0; i < 3; ++i) sv[i] += t[i];
  }
  // (the 6-waves-per-SIMD FFT instances at CW ≥ 7 keep the shuffle scan and binary powering:
  // the DPP scan's per-lane powers would spill them, 12–36 B)
  constexpr bool kShflScan = E == 4 && CW >= 7;
  if constexpr (kShflScan) {
#pragma unroll
    for (int r2 = 0; r2 < 6; ++r2) {
      const int d = 1 << r2;
      if (dbgb(a, 2)) break;
      double u[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) u[i] = __shfl_up(sv[i], d, 64);
      if (lane >= d) {
        Mat3 Pd;
#pragma unroll
        for (int q = 0; q < 9; ++q) Pd.m[q] = Pp[r2 * 9 + q];
        double t[3];
        matvec3(Pd, u, t);
        for (int i = 0; i < 3; ++i) sv[i] += t[i];
      }
    }
  } else if (!dbgb(a, 2)) {
    scan_dpp(sv, lane, Pp, a.scanP + kScanPowOff + (CW - 1) * 33 * 9);
  }
  if (lane == 63) {
    send[axis][w][0] = sv[0];
    send[axis][w][1] = sv[1];
    send[axis][w][2] = sv[2];
  }
  __syncthreads();  // end states published; z_ref dead (staging from here on)
  double xs[3] = {xi[0], xi[1], xi[2]};  // this wave's start state
  if (w > 0) {
    Mat3 M64;
#pragma unroll
    for (int q = 0; q < 9; ++q) M64.m[q] = Pp[6 * 9 + q];
    for (int i = 0; i < 3; ++i) xs[i] = send[axis][0][i];
    for (int v = 1; v < w; ++v) {
      double t[3];
      matvec3(M64, xs, t);
      for (int i = 0; i < 3; ++i) xs[i] = send[axis][v][i] + t[i];
    }
    // lane l adds (Ā^CW)^(l+1)·x_start: the plan's per-lane powers k ≤ 32, times (Ā^CW)^32
    // (scan level 5) first for lanes 32..63
    double vv[3] = {xs[0], xs[1], xs[2]};
    int e = lane + 1;
    if constexpr (kShflScan) {  // binary powering over the scan levels
#pragma unroll
      for (int r2 = 0; r2 < 7; ++r2) {
        if ((e >> r2) & 1) {
          Mat3 Pd;
#pragma unroll
          for (int q = 0; q < 9; ++q) Pd.m[q] = Pp[r2 * 9 + q];
          double t[3];
          matvec3(Pd, vv, t);
          for (int i = 0; i < 3; ++i) vv[i] = t[i];
        }
      }
      for (int i = 0; i < 3; ++i) sv[i] += vv[i];
    } else {
      if (e > 32) {
        Mat3 P32;
#pragma unroll
        for (int q = 0; q < 9; ++q) P32.m[q] = Pp[5 * 9 + q];
        double t[3];
        matvec3(P32, vv, t);
        for (int i = 0; i < 3; ++i) vv[i] = t[i];
        e -= 32;
      }
      const double* m = a.scanP + kScanPowOff + ((CW - 1) * 33 + e) * 9;
      Mat3 M;
#pragma unroll
      for (int q = 0; q < 9; ++q) M.m[q] = m[q];
      double t[3];
      matvec3(M, vv, t);
      for (int i = 0; i < 3; ++i) sv[i] += t[i];
    }
  }
  double xs0[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double p = kShflScan ? __shfl_up(sv[i], 1, 64) : dpp_f64<0x138, 0xF>(sv[i]);
    xs0[i] = (lane == 0) ? xs[i] : p;
  }
  tl_stamp(a, b, 3);
  // ---- 4. replay (reference form) into the staging rows, coalesced copy-out per round --------
  // staging rows padded as the split kernels' (HistLayout: two doubles after every CW local
  // rows, even CW), so the lanes' ds_write rows are not 128 B multiples apart
  double* stage = smem;
  constexpr int HP = HistLayout<CW>::kPad;
  constexpr int HS = HistLayout<CW>::kSpan;
  const int rows_per_round = (2 * a.lzp) * HS / (6 * HS + HP);
  auto srow = [](int lr) { return lr * 6 + HP * (lr / HS); };
  double* hb = a.hist + b * (int64_t)n * 6;
  double x[3];
  for (int r0 = 0; r0 < n; r0 += rows_per_round) {
    const int r1 = min(r0 + rows_per_round, n);
    if (lane == 0 && w == 0 && r0 == 0) {
      stage[3 * axis + 0] = xi[0];
      stage[3 * axis + 1] = xi[1];
      stage[3 * axis + 2] = xi[2];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = xs0[i];
#pragma unroll
    for (int q = 0; q < CW; ++q) {
      const int m = mbeg + q;
      if (m < nsteps) {
        const double u = f[q] - (kx0 * x[0] + kx1 * x[1] + kx2 * x[2]);
        double xn[3];
        lipm_step(lc, x, u, xn);
        if (m == kick_step) xn[1] -= kk;
        const int row = m + 1;
        if (row >= r0 && row < r1) {
          double* o = stage + srow(row - r0) + 3 * axis;
          o[0] = xn[0];
          o[1] = xn[1];
          o[2] = xn[2];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) x[i] = xn[i];
      }
    }
    __syncthreads();
    if (!dbgb(a, 4)) {
      const int nd2 = (r1 - r0) * 3;
      const double2* src = reinterpret_cast<const double2*>(stage);
      double2* dst = reinterpret_cast<double2*>(hb + (int64_t)r0 * 6);
      for (int e = tid; e < nd2; e += NT)  // written once
        st_nt2(&dst[e], src[e + (HP / 2) * ((e / 3) / HS)]);
    }
    __syncthreads();
  }
  if (a.status != nullptr) {
    const bool finite = isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]);
    const unsigned long long bad = __ballot(!finite);
    if (lane == 0) flag[wv] = bad ? ZMPC_ST_NONFINITE : 0;
    // Sample 0 of the bounds has weight zero in every window: the direct form never reads it,
    // the sparse and FFT forms turn a non-finite one into a non-finite walk.  The status flags
    // it under every form (loads issued ahead of the barrier).
    double2 h0 = make_double2(0.0, 0.0), l0 = h0;
    if (tid == 0) {
      h0 = *reinterpret_cast<const double2*>(a.zmax + b * a.bstride);
      l0 = *reinterpret_cast<const double2*>(a.zmin + b * a.bstride);
    }
    __syncthreads();
    if (tid == 0) {
      int fl = (isfinite(h0.x + l0.x) && isfinite(h0.y + l0.y)) ? 0 : ZMPC_ST_NONFINITE;
      for (int v = 0; v < 2 * W; ++v) fl |= flag[v];
      a.status[b] = fl;
    }
  }
  tl_stamp(a, b, 4);
  if (a.dbg < 0) a.hist[tid] = pf0 + pf1;  // never (dbg ≥ 0): keeps the prefetch loads
}

// Walks of any length (the fallback beyond the wide kernel's 64·8·8 + 1 samples): one wave per
// walk, the walk processed in chunks of `lc` timesteps with the two axes' states carried in
// registers from chunk to chunk, so the LDS footprint does not grow with n.  Per chunk: the
// z_ref rows it reads (t0 .. t0 + lc + kc, clamped to the last sample — the window padding of
// zmp_controller.py:81-88), the correlation passes into f (LDS), the lane-chunk affine scan
// from the carried state, and the replay in the reference form through the dead z_ref area.
template <int CW>
__device__ __forceinline__ void chunk_scan_replay(const RolloutArgs& a, int lane, const double* f0,
                                                  const double* f1, double* stage, int rows_pr,
                                                  double* xs, double* ys, double kk,
                                                  int64_t kstep, int64_t t0, int ns,
                                                  double* hb) {
  const LipmConsts lc = a.lc;
  const double kx0 = a.kx[0], kx1 = a.kx[1], kx2 = a.kx[2];
  const double Bv[3] = {lc.T3_6, lc.T2_2, lc.T};
  Mat3 Ab;  // Ā = A − B kxᵀ
  {
    const double A[9] = {1.0, lc.T, lc.T2_2, 0.0, 1.0, lc.T, 0.0, 0.0, 1.0};
    const double kx[3] = {kx0, kx1, kx2};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Ab.m[3 * i + j] = A[3 * i + j] - Bv[i] * kx[j];
  }
  const int C = (ns + 63) / 64;  // steps per lane chunk
  const int mbeg = lane * C, mend = min(mbeg + C, ns);
  // zero-start composition of the lane's steps, then Kogge-Stone with P = Ā^C
  double s0[3] = {0.0, 0.0, 0.0}, s1[3] = {0.0, 0.0, 0.0};
  for (int m = mbeg; m < mend; ++m) {
    double t[3];
    matvec3(Ab, s0, t);
    for (int i = 0; i < 3; ++i) s0[i] = fma(Bv[i], f0[m], t[i]);
    matvec3(Ab, s1, t);
    for (int i = 0; i < 3; ++i) s1[i] = fma(Bv[i], f1[m], t[i]);
    if (t0 + m == kstep) s1[1] -= kk;
  }
  Mat3 P = Ab;
  for (int q = 1; q < C; ++q) P = matmul3(P, Ab);
  if (lane == 0) {
    double t[3];
    matvec3(P, xs, t);
    for (int i = 0; i < 3; ++i) s0[i] += t[i];
    matvec3(P, ys, t);
    for (int i = 0; i < 3; ++i) s1[i] += t[i];
  }
  Mat3 Pd = P;
  for (int d = 1; d < 64; d <<= 1) {
    double u0[3], u1[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      u0[i] = __shfl_up(s0[i], d, 64);
      u1[i] = __shfl_up(s1[i], d, 64);
    }
    if (lane >= d) {
      double t[3];
      matvec3(Pd, u0, t);
      for (int i = 0; i < 3; ++i) s0[i] += t[i];
      matvec3(Pd, u1, t);
      for (int i = 0; i < 3; ++i) s1[i] += t[i];
    }
    Pd = matmul3(Pd, Pd);
  }
  double xb0[3], yb0[3];  // state at the start of this lane's steps
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double p0 = __shfl_up(s0[i], 1, 64);
    const double p1 = __shfl_up(s1[i], 1, 64);
    xb0[i] = (lane == 0) ? xs[i] : p0;
    yb0[i] = (lane == 0) ? ys[i] : p1;
  }
  // replay x⁺ = A x + B u (zmp_controller.py:199) in rounds of staged rows t0+1 .. t0+ns
  double x[3], y[3];
  for (int r0 = 0; r0 < ns; r0 += rows_pr) {
    const int r1 = min(r0 + rows_pr, ns);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      x[i] = xb0[i];
      y[i] = yb0[i];
    }
    for (int m = mbeg; m < mend; ++m) {
      const double ux = f0[m] - (kx0 * x[0] + kx1 * x[1] + kx2 * x[2]);
      const double uy = f1[m] - (kx0 * y[0] + kx1 * y[1] + kx2 * y[2]);
      double xn[3], yn[3];
      lipm_step(lc, x, ux, xn);
      lipm_step(lc, y, uy, yn);
      if (t0 + m == kstep) yn[1] -= kk;  // F_ext impulse (:105-106)
      if (m >= r0 && m < r1) {
        double* o = stage + (m - r0) * 6;
        o[0] = xn[0];
        o[1] = xn[1];
        o[2] = xn[2];
        o[3] = yn[0];
        o[4] = yn[1];
        o[5] = yn[2];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        x[i] = xn[i];
        y[i] = yn[i];
      }
    }
    __syncthreads();
    const double2* src = reinterpret_cast<const double2*>(stage);
    double2* dst = reinterpret_cast<double2*>(hb + (t0 + r0 + 1) * 6);
    for (int e = lane; e < (r1 - r0) * 3; e += 64) st_nt2(&dst[e], src[e]);
    __syncthreads();
  }
  // carry the chunk's end state: the lane that ran step ns − 1
  const int last = (ns - 1) / C;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    xs[i] = __shfl(x[i], last, 64);
    ys[i] = __shfl(y[i], last, 64);
  }
}

template <int CW>
__global__ void __launch_bounds__(64) zmpc_rollout_unc_chunk_kernel(RolloutArgs a, int lc) {
  using ZL = ZrLayout<CW>;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const int n = a.n;
  const int64_t nsteps = n - 1;
  double* ks = smem;
  double* zr0 = smem + a.kcp;
  double* zr1 = zr0 + a.lzp;
  double* f0 = zr1 + a.lzp;
  double* f1 = f0 + lc;
  const int rows_pr = (2 * a.lzp) / 6;  // history rows per staging round (z_ref area)
  for (int j = lane; j < a.kcp; j += 64) ks[j] = a.k[j];
  const double2* zmx = reinterpret_cast<const double2*>(a.zmax + b * a.bstride);
  const double2* zmn = reinterpret_cast<const double2*>(a.zmin + b * a.bstride);
  const double* xb = a.x0 + b * 6;
  double xs[3] = {xb[0], xb[1], xb[2]}, ys[3] = {xb[3], xb[4], xb[5]};
  const double kk = (a.kick != nullptr) ? a.kick[b] : 0.0;
  const int64_t kstep = kick_step_of(a, b);
  double* hb = a.hist + b * (int64_t)n * 6;
  if (lane < 6) hb[lane] = xb[lane];  // row 0 = x0
  for (int64_t t0 = 0; t0 < nsteps; t0 += lc) {
    const int ns = (int)min((int64_t)lc, nsteps - t0);
    const int passes = (ns + 64 * CW - 1) / (64 * CW);
    const int lz = passes * 64 * CW + a.kc + 1;
    __syncthreads();  // the previous chunk's staging rows are out
    for (int t = lane; t < lz; t += 64) {
      const int64_t row = min(t0 + t, (int64_t)n - 1);
      const double2 h = zmx[row], l = zmn[row];
      zr0[ZL::idx(t)] = (h.x + l.x) / 2;
      zr1[ZL::idx(t)] = (h.y + l.y) / 2;
    }
    __syncthreads();
    for (int pass = 0; pass < passes; ++pass) {
      const int i0 = pass * 64 * CW + lane * CW;
      double a0[CW], a1[CW];
      correlate<CW>(a, ks, zr0, zr1, i0, a0, a1);
#pragma unroll
      for (int m = 0; m < CW; ++m) {
        if (i0 + m < ns) {
          f0[i0 + m] = a0[m];
          f1[i0 + m] = a1[m];
        }
      }
    }
    __syncthreads();  // f complete; the z_ref area becomes the history staging
    chunk_scan_replay<CW>(a, lane, f0, f1, zr0, rows_pr, xs, ys, kk, kstep, t0, ns, hb);
  }
  if (a.status != nullptr) {
    // (sample 0 of the bounds, which no window reads, is flagged as the wide kernel flags it)
    const double2 h0 = zmx[0], l0 = zmn[0];
    const bool finite = isfinite(xs[0]) && isfinite(xs[1]) && isfinite(xs[2]) &&
                        isfinite(ys[0]) && isfinite(ys[1]) && isfinite(ys[2]) &&
                        isfinite(h0.x + l0.x) && isfinite(h0.y + l0.y);
    if (lane == 0) a.status[b] = finite ? 0 : ZMPC_ST_NONFINITE;
  }
}

// The wide kernel, with the next-dispatch-round prefetch when the batch takes at most two
// rounds of resident workgroups (config 5 at ≈2.7 rounds: 64.4 vs 54.3 µs with it, so off there;
// profiles/r3pfw/).
template <int C, int W, int E>
void launch_wide(const UncChoice& c, hipStream_t s, RolloutArgs q, int cus) {
  const int occ = occupancy(reinterpret_cast<const void*>(zmpc_rollout_unc_wide_kernel<C, W, E>),
                            128 * W, c.lds);
  const int64_t R = (int64_t)std::max(cus, 1) * occ;
  q.pf_ahead = (R > 0 && q.n <= 512 * W && q.B <= 2 * R) ? R : 0;
  hipLaunchKernelGGL((zmpc_rollout_unc_wide_kernel<C, W, E>), dim3((unsigned)q.B), dim3(128 * W),
                     c.lds, s, q);
}

// The wide kernel's instance for E points per thread.  E = 8 exists only where its transform
// (P = 8·128·W points of 16 B) fits the 64 KiB LDS ceiling choose_unc enforces, i.e. W ≤ 4:
// an 8-wave E = 8 instance could never launch.
template <int C, int W>
void launch_wide_e(const UncChoice& c, hipStream_t s, const RolloutArgs& q, int cus) {
  if (c.E == 4) return launch_wide<C, W, 4>(c, s, q, cus);
  if constexpr (8 * 128 * W * 16 <= 64 * 1024) {
    if (c.E == 8) return launch_wide<C, W, 8>(c, s, q, cus);
  }
  launch_wide<C, W, 0>(c, s, q, cus);
}

}  // namespace

// The Wide and Chunk launches of a choice made by the caller; rollout_args is the caller's
// RolloutArgs (rollout_common.h: the type is local to each unit, so it crosses as a pointer).
hipError_t zmpc_launch_rollout_long(const UncChoice& c, const void* rollout_args, int cus,
                                    hipStream_t s) {
  const RolloutArgs& a = *static_cast<const RolloutArgs*>(rollout_args);
  if (c.kind == UncKind::Chunk) {
    hipLaunchKernelGGL(zmpc_rollout_unc_chunk_kernel<8>, dim3((unsigned)a.B), dim3(64), c.lds, s,
                       a, c.lc);
    return hipGetLastError();
  }
  // (the twelve shapes choose_unc can return: W = 2, 4, 8 at CW = 5..8)
  switch (c.kind == UncKind::Wide ? c.w * 16 + c.cw : 0) {
#define ZMPC_WCASE(W, C)                \
  case W * 16 + C:                      \
    launch_wide_e<C, W>(c, s, a, cus);  \
    break;
    ZMPC_WCASE(2, 5) ZMPC_WCASE(2, 6) ZMPC_WCASE(2, 7) ZMPC_WCASE(2, 8)
    ZMPC_WCASE(4, 5) ZMPC_WCASE(4, 6) ZMPC_WCASE(4, 7) ZMPC_WCASE(4, 8)
    ZMPC_WCASE(8, 5) ZMPC_WCASE(8, 6) ZMPC_WCASE(8, 7) ZMPC_WCASE(8, 8)
#undef ZMPC_WCASE
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// The chunk kernel's dynamic LDS passes the default 64 KiB ceiling at long horizons; the 8-wave
// wide kernel runs up to wide_lds_cap(8): its instances are CW = 5..8 with E = 0 or 4
// (launch_wide_e: E = 8 has no 8-wave instance).
hipError_t zmpc_rollout_long_set_attrs() {
  hipError_t e = hipFuncSetAttribute((const void*)zmpc_rollout_unc_chunk_kernel<8>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
#define ZMPC_WATTR(C, E)                                                                      \
  if (e == hipSuccess)                                                                        \
    e = hipFuncSetAttribute((const void*)zmpc_rollout_unc_wide_kernel<C, 8, E>,              \
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)wide_lds_cap(8));
  ZMPC_WATTR(5, 0) ZMPC_WATTR(6, 0) ZMPC_WATTR(7, 0) ZMPC_WATTR(8, 0)
  ZMPC_WATTR(5, 4) ZMPC_WATTR(6, 4) ZMPC_WATTR(7, 4) ZMPC_WATTR(8, 4)
#undef ZMPC_WATTR
  return e;
}
