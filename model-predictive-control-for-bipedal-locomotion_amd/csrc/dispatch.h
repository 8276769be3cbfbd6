// The launch rules of libzmpc.so, stated once: which kernel, with which geometry and how much
// dynamic LDS, a call of a given shape takes.  Plain host C++17 — integers and option values in,
// POD structs out; no HIP call, no plan pointer, no environment, no allocation — so that the
// rules compile and run without a GPU (tests/test_dispatch_host.py pins them).  The launchers
// (rollout.hip with rollout_long.hip, strict_dispatch.hip, strict_lq.hip, strict_scan.hip,
// herdt.hip, capi.hip) ask here and only launch; the device code reads the layout constants below.
#pragma once

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>

// ---------------------------------------------------------------------------------------------
// Plan tables whose sizes enter the LDS budgets

// suffix sums S_j = Σ_{j' ≥ j} k_{j'} of the gain row: entry i = S_{i−8} for 1 ≤ i − 8 ≤ N − 1,
// zero elsewhere in [0, N + 16) (so a lane's 8-wide read at any clamped offset stays inside),
// S_0 at N + 16
constexpr int ksum_rows(int N) { return N + 18; }
constexpr int ksum_s0(int N) { return N + 16; }

constexpr int kFftPT = 8192;    // largest transform (twiddle table size)
constexpr int kFftPmin = 256;   // smallest transform with a gain spectrum
constexpr int kFftGComplex = 2 * kFftPT - kFftPmin;  // Σ_P P over P = kFftPmin..kFftPT

// ---------------------------------------------------------------------------------------------
// Unconstrained rollout (rollout.hip; the wide and chunk kernels: rollout_long.hip)

// Correlation tile width: outputs per lane per pass, chosen per walk length so that
// passes·64·CW barely covers the n−1 timesteps (n = 420 → CW = 7: 448 outputs, 1 pass).
inline int pick_cw(int64_t nsteps) {
  int best = 8;
  int64_t best_cost = INT64_MAX;
  for (int cw = 8; cw >= 1; --cw) {
    const int64_t cost = ((nsteps + 64 * cw - 1) / (64 * cw)) * cw;
    if (cost < best_cost) {
      best_cost = cost;
      best = cw;
    }
  }
  return best;
}

// Doubles of the split kernels' history staging for n rows at tile width cw (rollout_common.h
// HistLayout: two pad doubles after every 2·cw step rows for even cw).
constexpr size_t hist_doubles(int cw, int n) {
  return (size_t)n * 6 + (size_t)((cw % 2 == 0) ? 2 : 0) * ((n + 2 * cw - 1) / (2 * cw));
}

struct RolloutGeom {
  int cw, passes, kc, lz, lzp, nf;
  int kfm;  // fast-FIR steps (odd CW; axis_correlate_ffa), 0 otherwise
  int kcp;  // doubles of LDS for the staged gain row (kc rounded up to even)
};

inline RolloutGeom rollout_geom(int N, int64_t n) {
  RolloutGeom g;
  const int64_t nsteps = n - 1;
  g.cw = pick_cw(nsteps);
  g.passes = (int)((nsteps + 64 * g.cw - 1) / (64 * g.cw));
  g.kc = (N + g.cw - 1) / g.cw * g.cw;           // k loop bound (k zero-padded)
  g.lz = g.passes * 64 * g.cw + g.kc + 1;         // z_ref samples staged (padded with last)
  g.kfm = 0;
  if (g.cw & 1) {
    // the fast-FIR form (odd CW) reads up to sample 64·CW + 2·kfm + W of the walk
    const int U = g.cw / 2 + 1, mm = (N + 2) / 2;
    g.kfm = (mm + U - 1) / U * U;
    g.lz = std::max(g.lz, g.passes * 64 * g.cw + 2 * g.kfm + 2 * U + 2);
  }
  const int pad = (g.cw % 2 == 0) ? 1 : 0;
  g.lzp = g.lz + pad * (g.lz / g.cw) + 1;         // LDS doubles per axis
  // the z_ref area doubles as the history staging buffer: at least a third of a walk of rows
  const int64_t stage_min = ((n + 2) / 3 * 6 + 1) / 2;
  if (g.lzp < stage_min) g.lzp = (int)stage_min;
  g.lzp = (g.lzp + 1) & ~1;
  g.nf = g.passes == 1 ? 0 : (int)((nsteps + 2) & ~1LL);  // f lives in LDS only if passes > 1
  g.kcp = (g.kc + 1) & ~1;
  return g;
}

inline size_t lds_bytes(const RolloutGeom& g) {
  return (size_t)(g.kcp + 2 * g.lzp + 2 * g.nf) * sizeof(double);
}

// The wide kernel's sparse attempt (wide_correlate_sparse) gives up, uniformly over the
// workgroup, when either axis has more than this many changes.
constexpr int kSparseMaxWide = 64;

// LDS doubles the wide kernel's sparse attempt adds behind the two z_ref areas: the suffix-sum
// table, the two change lists (values, then int positions)
constexpr int wide_sparse_doubles(int N) {
  return ((ksum_rows(N) + 1) & ~1) + 2 * kSparseMaxWide + kSparseMaxWide;
}

// Geometry of the wide kernel: W waves per axis (2, 4 or 8), CW = ceil((n−1)/(64·W)) ≤ 8.
struct WideGeom {
  int w, cw, kc, lz, lzp;
};

// The wide kernel's dynamic-LDS ceiling: 64 KiB (the 4-waves-per-SIMD bound leaves no room above
// it for W = 2 and 4), but 159 KiB for W = 8 — a 16-wave workgroup fills a CU's wave slots at that
// bound alone, so its LDS costs no occupancy (walks of 2561..4096 samples at N >= 920 took the
// chunk kernel at 8x the time, profiles/r6fin/configs/sweep_full.jsonl).  The kernel's static LDS
// (≈0.5 KiB) comes on top: hipFuncSetAttribute refuses a dynamic limit of the full 160 KiB.
inline size_t wide_lds_cap(int w) { return (size_t)(w == 8 ? 159 : 64) * 1024; }

// (Up to 64·8 timesteps are one pass of the split kernel, so the wide kernel starts at CW = 5.)
inline bool wide_geom(int N, int64_t n, WideGeom* g) {
  const int64_t ns = n - 1;
  if (ns > 64 * 8 * 8) return false;
  g->w = ns <= 64 * 8 * 2 ? 2 : (ns <= 64 * 8 * 4 ? 4 : 8);
  g->cw = (int)((ns + 64 * g->w - 1) / (64 * g->w));
  g->kc = (N + g->cw - 1) / g->cw * g->cw;
  g->lz = g->w * 64 * g->cw + g->kc + 1;
  const int pad = (g->cw % 2 == 0) ? 1 : 0;
  g->lzp = ((g->lz + pad * (g->lz / g->cw) + 1) + 1) & ~1;
  return (size_t)2 * g->lzp * sizeof(double) <= wide_lds_cap(g->w);
}

// Chunk geometry: CW = 8, chunks of lc = 2·64·CW timesteps (two correlation passes), LDS =
// k + z_ref (2 axes, lc + kc + 1 padded rows) + f (2 axes × lc): ≈ 45 KB at N = 512.
struct ChunkGeom {
  int lc, kc, kcp, lz, lzp;
};

inline ChunkGeom chunk_geom(int N) {
  constexpr int CW = 8;
  ChunkGeom g;
  g.lc = 2 * 64 * CW;
  g.kc = (N + CW - 1) / CW * CW;
  g.kcp = (g.kc + CW + 1) & ~1;  // the correlation's sliding window reads one group past kc
  g.lz = g.lc + g.kc + 1;
  g.lzp = ((g.lz + g.lz / CW + 1) + 1) & ~1;
  return g;
}

inline size_t chunk_lds_bytes(const ChunkGeom& g) {
  return (size_t)(g.kcp + 2 * g.lzp + 2 * g.lc) * sizeof(double);
}

// The kernel of an unconstrained rollout:
//   Copy         n = 1: the history is the initial state, no kernel;
//   SplitShared  one pass, shared CoP: zmpc_shared_f_kernel once, then
//                zmpc_rollout_unc_splitd_kernel<CW, true> (scan, replay, history stores);
//   Split        one pass, per-walk bounds: zmpc_rollout_unc_splitd_kernel<CW, false>, a
//                128-thread workgroup per walk (odd CW: the fast-FIR dense form);
//   Generic      one pass whose split LDS passes 64 KiB (very long horizons), or
//                ZMPC_OPT_ROLLOUT_KERNEL = 1 (the cross-check): zmpc_rollout_unc_kernel<CW>, one
//                wave per walk;
//   Wide         64·8 < n − 1 ≤ 64·8·8: zmpc_rollout_unc_wide_kernel<CW, W, E>, 2·W waves per walk;
//   Chunk        any length: zmpc_rollout_unc_chunk_kernel<8>, one wave per walk.
enum class UncKind { Copy, SplitShared, Split, Generic, Wide, Chunk };

// What a choice puts into the kernel arguments (rollout_common.h RolloutArgs), shared by the
// history launch and the fused rollout-to-metrics launch.
struct WalkGeom {
  int cw;       // correlation tile width (the kernel's CW), 0 for Copy
  bool sparse;  // the kernel stages the plan's suffix sums and tries the sparse-difference
                // correlation first (the split and wide kernels only)
  int kc, kcp, lz, lzp, kfm;  // geometry fields of the kernel arguments
  int fstride;  // SplitShared: doubles per axis of the precomputed f, 0 otherwise
};

struct UncChoice : WalkGeom {
  UncKind kind;
  int w;        // Wide: waves per axis (2, 4 or 8), 0 otherwise
  int E, P;     // Wide with the FFT correlation: points per thread (4 or 8) and transform size;
                // 0, 0 for the direct form and every other kind
  size_t lds;   // dynamic LDS bytes of the launch
  int lc;       // Chunk: timesteps per chunk, 0 otherwise
};

// (N, n): horizon and walk samples; shared_cop: bounds stride 0; the three options as
// include/zmpc.h (ZMPC_OPT_ROLLOUT_KERNEL, ZMPC_OPT_LONG_WALK, ZMPC_OPT_CORRELATION).
inline UncChoice choose_unc(int N, int64_t n, bool shared_cop, int opt_rollout_kernel,
                            int opt_long_walk, int opt_correlation) {
  UncChoice c{};
  if (n == 1) {
    c.kind = UncKind::Copy;
    return c;
  }
  const RolloutGeom g = rollout_geom(N, n);
  const size_t lds = lds_bytes(g);
  c.kfm = g.kfm;
  // ZMPC_OPT_CORRELATION = 1: the dense correlation forms only (cross-checks, and bench.py's
  // dense-form timing beside the default)
  const bool want_sparse = opt_correlation != 1;
  const int long_form = opt_long_walk;  // 0 auto, 1 direct, 2 FFT, 3 chunk kernel
  WideGeom wg;
  // any length (the whole walk does not fit one pass, and the wide kernel does not take it), or
  // a single-pass geometry beyond LDS (very long horizon N)
  if ((g.passes > 1 && (long_form == 3 || !wide_geom(N, n, &wg))) || lds > 160 * 1024) {
    const ChunkGeom cg = chunk_geom(N);
    c.kind = UncKind::Chunk;
    c.cw = 8;
    c.kc = cg.kc;
    c.kcp = cg.kcp;
    c.lz = cg.lz;
    c.lzp = cg.lzp;
    c.lc = cg.lc;
    c.lds = chunk_lds_bytes(cg);
    return c;
  }
  if (g.passes > 1) {
    c.kind = UncKind::Wide;
    c.cw = wg.cw;
    c.w = wg.w;
    c.kc = wg.kc;
    c.kcp = g.kcp;
    c.lz = wg.lz;
    c.lzp = wg.lzp;
    size_t lds_w = 2 * (size_t)wg.lzp * sizeof(double);
    // FFT correlation when the transform maps onto the workgroup (E = P/NT points per thread,
    // 4 or 8), fits the default LDS ceiling and costs less than the direct form: measured
    // crossover (n − 1)·N ≥ 9·P·log2 P — N = 150 walks of 1000/2000 samples
    // are faster direct, N ≥ 200 faster by FFT.  ZMPC_OPT_LONG_WALK 1 / 2 forces the direct
    // form / the FFT wherever it fits.
    int P = kFftPmin;
    while (P < n - 1 + N) P *= 2;
    const int NT = 128 * wg.w;
    int E = (P % NT == 0) ? P / NT : 0;
    if (long_form == 1 || (E != 4 && E != 8) || P > kFftPT || (size_t)P * 16 > 64 * 1024) E = 0;
    if (long_form == 0 && (double)(n - 1) * N < 9.0 * P * __builtin_ctz((unsigned)P)) E = 0;
    if (E) {
      c.E = E;
      c.P = P;
      lds_w = std::max(lds_w, (size_t)P * 16);
    }
    // the sparse attempt's table and change lists behind the z_ref areas (within the kernel's
    // dynamic-LDS ceiling, else dense only)
    const size_t lds_sp = (2 * (size_t)wg.lzp + wide_sparse_doubles(N)) * sizeof(double);
    if (want_sparse && lds_sp <= wide_lds_cap(wg.w)) {
      c.sparse = true;
      lds_w = std::max(lds_w, lds_sp);
    }
    c.lds = lds_w;
    return c;
  }
  // Walks of at most 64·8+1 samples (one correlation pass).
  c.cw = g.cw;
  c.kc = g.kc;
  c.kcp = g.kcp;
  c.lz = g.lz;
  c.lzp = g.lzp;
  const bool generic = opt_rollout_kernel == 1;
  const size_t lds_axis = lds - (size_t)g.kcp * sizeof(double);  // no staged gain row
  size_t lds_split = std::max<size_t>(lds_axis, hist_doubles(g.cw, (int)n) * sizeof(double));
  // the sparse-difference correlation stages the plan's suffix sums in front of the z_ref areas
  const size_t lds_sparse = std::max(lds_axis + (size_t)ksum_rows(N) * sizeof(double), lds_split);
  const bool sparse = want_sparse && lds_sparse <= 64 * 1024;
  if (sparse) lds_split = lds_sparse;
  // shared CoP (bounds stride 0): f once per launch, when a walk's history and f fit the
  // default 64 KiB
  if (shared_cop && !generic && (6 * (size_t)n + 2 * (size_t)n) * sizeof(double) <= 64 * 1024) {
    c.kind = UncKind::SplitShared;
    c.fstride = ((64 * g.cw) + 63) & ~63;  // every lane's CW values, padded
    c.lds = hist_doubles(g.cw, (int)n) * sizeof(double);
    return c;
  }
  if (generic || lds_split > 64 * 1024) {
    c.kind = UncKind::Generic;
    c.lds = lds;
    return c;
  }
  c.kind = UncKind::Split;
  c.sparse = sparse;
  c.lds = lds_split;
  return c;
}

// The fused rollout-to-metrics launch (zmpc_rollout_metrics; rollout.hip split_walk with MET):
// the split kernels' walk with the replay feeding the metrics reduction instead of a history.
//   Sample0      n = 1 (choose_unc: Copy): the metrics of x0 alone, zmpc_metrics_x0_kernel;
//   Split        zmpc_rollout_metrics_splitd_kernel<CW, false>, where choose_unc answers Split;
//   SplitShared  zmpc_shared_f_kernel, then zmpc_rollout_metrics_splitd_kernel<CW, true>, where
//                choose_unc answers SplitShared;
//   None         every other shape (Generic, Wide, Chunk): no fused form, `why` names the reason.
// CW, the geometry fields and the sparse attempt are choose_unc's, so the fused walk takes the
// history walk's arithmetic up to the replay.  The LDS holds no history staging: the z_ref areas
// (with the suffix sums in front), reused after the correlation for the walk's bounds — per axis
// one (z_max, z_min) pair of doubles per sample in the z_ref row layout, from which each lane
// reads the rows of its own CW samples.
enum class MetKind { None, Sample0, Split, SplitShared };

// Doubles of the bounds staging: two axes of 16-byte (z_max, z_min) pairs, rows as ZrLayout
// (one pad row per cw rows for even cw).
constexpr size_t metrics_bound_doubles(int cw, int n) {
  return 4 * (size_t)(n + ((cw % 2 == 0) ? (n - 1) / cw : 0));
}

struct MetChoice : WalkGeom {
  MetKind kind;
  const char* why;  // None: the reason, for the caller's message
  size_t lds;
};

inline MetChoice choose_unc_metrics(int N, int64_t n, bool shared_cop, int opt_rollout_kernel,
                                    int opt_correlation) {
  MetChoice m{};
  if (opt_rollout_kernel == 1) {
    m.why = "the one-wave cross-check kernel (rollout kernel option 1) has no fused form";
    return m;
  }
  // (the long-walk option only chooses among the forms of walks that take several passes)
  const UncChoice c = choose_unc(N, n, shared_cop, opt_rollout_kernel, 0, opt_correlation);
  switch (c.kind) {
    case UncKind::Copy:
      m.kind = MetKind::Sample0;
      return m;
    case UncKind::Split:
    case UncKind::SplitShared:
      break;
    case UncKind::Generic:
      m.why = "the horizon's split-kernel LDS passes 64 KiB (one-wave kernel): no fused form";
      return m;
    default:
      m.why = "walks of more than 513 samples (wide and chunk kernels) have no fused form";
      return m;
  }
  m.kind = c.kind == UncKind::Split ? MetKind::Split : MetKind::SplitShared;
  static_cast<WalkGeom&>(m) = c;
  const size_t bounds = metrics_bound_doubles(c.cw, (int)n) * sizeof(double);
  m.lds = bounds;
  if (m.kind == MetKind::Split)
    m.lds = std::max(bounds, ((size_t)2 * c.lzp + (c.sparse ? ksum_rows(N) : 0)) * sizeof(double));
  if (m.lds > 64 * 1024) {  // (cannot happen where choose_unc's own 64 KiB rule passed)
    m = MetChoice{};
    m.why = "the fused form's LDS passes 64 KiB";
  }
  return m;
}

// ---------------------------------------------------------------------------------------------
// Push-robustness maps (zmpc_push_map, zmpc_push_map_shaped; pushmap.hip)

// The full map keeps a walk's (up, dn) margin pairs in LDS, 16 bytes per sample plus 64 pairs of
// +inf behind them, one workgroup per walk.  Its dynamic-LDS ceiling is the wide kernel's 159 KiB
// (hipFuncSetAttribute refuses the full 160), so the longest walk has 159·64 − 64 samples.
constexpr size_t kPushMapLdsCap = (size_t)159 * 1024;
constexpr int64_t kPushMapMaxN = (int64_t)(kPushMapLdsCap / 16) - 64;  // 10112

// The geometry of a zmpc_push_map launch of n-sample walks:
//   full map     `waves` waves per walk (one per pair of 64-step blocks, 16 at the most) and `lds`
//                bytes of dynamic LDS; ok = false past kPushMapMaxN, `why` states the limit;
//   single step  one wave per walk, no LDS, any n the history entries take.
struct PushMapChoice {
  bool ok;
  int waves;
  size_t lds;
  const char* why;
};

inline PushMapChoice choose_push_map(int64_t n, bool single_step) {
  if (single_step) return PushMapChoice{true, 1, 0, nullptr};
  if (n > kPushMapMaxN)
    return PushMapChoice{false, 0, 0,
                         "the full map keeps a walk's margins in LDS: at most 10112 samples per "
                         "walk (the single-step form, push_steps, has no such limit)"};
  const int64_t nblk = (n + 63) / 64;
  const int waves = (int)std::min<int64_t>(16, std::max<int64_t>(1, (nblk + 1) / 2));
  return PushMapChoice{true, waves, (size_t)(n + 64) * 16, nullptr};
}
static_assert(kPushMapMaxN == 10112 && kPushMapMaxN >= 4096, "the message states the limit");

// The geometry of a zmpc_push_map_shaped launch over naxes = 1 or 2 axes.  Two axes take turns
// over the same 16 bytes per sample (the second fill re-reads the walk's 48·n bytes from cache:
// n samples against the n²/2 pairs of the map loop), so the LDS, the waves and the longest walk
// are choose_push_map's for either count.  Both axes' margins in LDS at once (32 bytes per
// sample) would halve the longest walk to 5024 samples and double the loop's LDS bytes and live
// accumulators to save the second, cached pass and half the scalar table loads.
inline PushMapChoice choose_push_shaped(int64_t n, bool single_step, int naxes) {
  if (naxes != 1 && naxes != 2) return PushMapChoice{false, 0, 0, "one or two axes"};
  PushMapChoice c = choose_push_map(n, single_step);
  if (!c.ok)
    c.why = "the full map keeps a walk's margins in LDS, one axis at a time: at most 10112 "
            "samples per walk for one axis or two (the single-step form, push_steps, has no "
            "such limit)";
  return c;
}

// ---------------------------------------------------------------------------------------------
// Strict box-QP (strict_dispatch.hip and its backends)

// Horizons of the reduced-Cholesky kernels (strict.hip: eight 64-slot column blocks).
constexpr int kStrictCholMaxN = 512;

// Longest strict horizon of the LQ kernel (lq_shape: its per-wave LDS — slot flags, 2 bits per
// slot and lane, and the parked V and state — fits a CU at two waves per workgroup, checked below
// by a static_assert).
constexpr int ZMPC_STRICT_MAX_N = 2464;

// Active-set pass cap of every strict kernel (strict.hip, strict_lq.hip, strict_scan.hip).  64 was
// too few: at (Q, R, h) = (0.1, 1e-3, 0.5) and N = 400 the reference's exact answer takes 150
// primal-dual passes from a cold start and 212 after an 800 N kick (strict_weights_long_ref.npz);
// the cap only bounds a cycling iteration
constexpr int kStrictMaxPasses = 1024;

// horizons of the parallel-in-time kernel (strict_scan.hip): 32-lane instances to N = 512 (C ≤ 16
// slots per lane: 256 VGPRs + 248 AGPRs), whole-wave ones to 960 (C ≤ 15: 256 + 236; C = 16 of 64
// lanes spills 12 B to scratch)
constexpr int kScan32MaxN = 512;
constexpr int kScanMaxN = 960;

// Auto: the parallel-in-time kernel up to this many instances, the LQ kernel beyond.  Crossover
// measured at N = 150, n = 420 (profiles/r4/r4h_crossover.jsonl): 4096 walks 19.9 vs 55.2 ms
// (LQ), 8192 walks 35.6 vs 56.8, 16384 walks 65.2 vs 57.8 — the LQ kernel won from ≈14 000
// walks.  Round 5 (profiles/r5r/cross.jsonl; both kernels faster): 8192 walks 45.0 vs 47.0 ms,
// 12288 walks 64.9 vs 47.6 — the LQ kernel wins from ≈8 600 walks.
constexpr int64_t kScanMaxInst = 16384;

// LQ kernel (strict_lq.hip): timesteps per segment (one flag word per segment), and the most
// working-set checkpoints a wave keeps in LDS (LqArgs::nlck)
constexpr int LQ_S = 8;
constexpr int kLdsCk = 2;
constexpr size_t kLdsCap = 160 * 1024;

// dwords of a lane's slot flags for NS segments (2 bits per slot: 16 bits per segment)
constexpr int flag_dwords(int NS) { return (NS + 1) / 2; }

// LDS of one workgroup: the G waves' slot flags (2 bits per slot and lane), parked V and state
// ([12][64] doubles each) and nlck LDS checkpoints ([9][64] doubles each).
constexpr size_t lq_lds_bytes(int G, int N, int nlck = 0) {
  const size_t segs = (size_t)(N + LQ_S - 1) / LQ_S;
  return (size_t)G * ((size_t)flag_dwords((int)segs) * 64 * 4 +
                      (12 + 9 * (size_t)nlck) * 64 * sizeof(double));
}

static_assert(lq_lds_bytes(2, ZMPC_STRICT_MAX_N) <= kLdsCap, "ZMPC_STRICT_MAX_N past the LDS");

// Workgroup shape of the LQ kernel: G waves per workgroup — the largest of 8, 4, 2 whose slot
// flags and parks fit a CU (N ≤ 896, 2176, ZMPC_STRICT_MAX_N; G = 0: none) — with the nlck LDS
// checkpoints per wave that fit beside them (config 3, N = 150: 2 at G = 8).
struct LqShape {
  int G, nlck;
  size_t lds;
};

inline LqShape lq_shape(int N) {
  if (N > ZMPC_STRICT_MAX_N) return LqShape{0, 0, 0};  // (no strict plan exists past it)
  for (int G : {8, 4, 2}) {
    if (lq_lds_bytes(G, N) > kLdsCap) continue;
    int c = kLdsCk;
    while (c > 0 && lq_lds_bytes(G, N, c) > 160 * 1024) --c;
    return LqShape{G, c, lq_lds_bytes(G, N, c)};
  }
  return LqShape{0, 0, 0};
}

inline bool strict_lq_supported(int N, bool has_lq_table) {
  return N >= 1 && N <= ZMPC_STRICT_MAX_N && has_lq_table && lq_shape(N).G != 0;
}

inline bool strict_scan_supported(int N) { return N >= 1 && N <= kScanMaxN; }

// Lanes per instance of the parallel-in-time kernel, and its slots per lane C (the kernel's
// template arguments): a whole wave while the instances fit one wave per SIMD (the latency of
// one pass is what counts), 32 beyond (two instances per wave; chunks of up to 16 slots,
// N ≤ 512; whole-wave instances beyond, to N = 960: N = 330–510 at 1024 walks 8.3e7–9.1e7 →
// 1.26e8–1.40e8 solves/s, profiles/r5aa/).  cus: compute units of the device (0: unknown, 256).
struct ScanShape {
  int lanes, C;
};

inline ScanShape scan_shape(int N, int64_t ninst, int cus_of_device) {
  const int64_t cus = cus_of_device > 0 ? cus_of_device : 256;
  // (one instance per SIMD: at N ≤ 128 the whole-wave instances would fit two waves per SIMD,
  // but two instances per wave already run 1.6–1.8× faster there, profiles/r5t/)
  const int lanes = (ninst > cus * 4 && N <= kScan32MaxN) ? 32 : 64;
  return ScanShape{lanes, (N + lanes - 1) / lanes};
}

// The strict solver of a launch over `ninst` instances (ZMPC_OPT_STRICT_SOLVER: 1 the tile
// kernel of strict.hip, 2 its reduced-Cholesky one-instance-per-wave kernel, 3 the LQ
// lane-per-instance kernel of strict_lq.hip, 4 the parallel-in-time one-instance-per-wave kernel
// of strict_scan.hip, 0 = auto): small batches take the parallel-in-time kernel and large ones
// the LQ kernel, whose per-pass work is O(N) per lane but serial within it.  The reduced-Cholesky
// wave kernel is a cross-check (profiles/r4/r4e_strict_small_batch.jsonl, N = 150, n = 420: 1
// walk 27.6 ms vs the LQ kernel's 29.0, 8 walks 92.8 vs 46.4 — its passes are long when a
// kicked walk pins many slots).
enum class StrictKind { Tile = 1, Wave = 2, Lq = 3, Scan = 4 };

inline StrictKind choose_strict(int N, int64_t ninst, int opt_strict_solver, bool has_lq_table) {
  const bool lq_ok = strict_lq_supported(N, has_lq_table);
  const bool scan_ok = strict_scan_supported(N);
  if (opt_strict_solver == 1) return StrictKind::Tile;
  if (opt_strict_solver == 2) return StrictKind::Wave;
  if (opt_strict_solver == 3) return StrictKind::Lq;  // (zmpc_plan_set_option accepts 3 and 4
  if (opt_strict_solver == 4) return StrictKind::Scan;  //  only where they run)
  if (scan_ok && (ninst <= kScanMaxInst || !lq_ok)) return StrictKind::Scan;
  return lq_ok ? StrictKind::Lq : StrictKind::Tile;
}

// ---------------------------------------------------------------------------------------------
// Herdt joint footstep QP (herdt.hip)

// Most footsteps inside one horizon window (zmpc_herdt_params.max_footsteps), and the footstep
// capacities MM the kernel is instantiated at: a launch takes the smallest that holds its count.
constexpr int kHerdtMaxFootsteps = 8;
constexpr int kHerdtMM[] = {2, 4, 6, 7, 8};
// facets per swing polygon (ZMPC_HERDT_MAX_FACETS of include/zmpc.h; herdt.hip asserts both)
constexpr int kHerdtMaxFacets = 16;
// the swing polygons in LDS (herdt.hip PolyLds): per side and facet 3 doubles of a half-space
// and 4 of its boundary segment
constexpr int kHerdtPolyBytes = 2 * kHerdtMaxFacets * (3 + 4) * (int)sizeof(double);

// Dynamic LDS of the kernel's one-wave workgroup at horizon N, byte offsets: per row and lane
// one byte each of support segment, constraint kind and working-set flag ([N][64] planes), then
// from a 16-byte boundary the swing polygons, the free-tail feedback ktab [N][4] doubles and the
// ZMP centres cen [kHerdtMaxFootsteps + 1][64] doubles.  (int: the kernel indexes LDS in 32 bits)
struct HerdtLds {
  int segb, kind, wset, poly, ktab, cen, bytes;
};

constexpr HerdtLds herdt_lds(int N) {
  HerdtLds l{};
  l.segb = 0;
  l.kind = N * 64;
  l.wset = 2 * N * 64;
  l.poly = (3 * N * 64 + 15) & ~15;
  l.ktab = l.poly + kHerdtPolyBytes;
  l.cen = l.ktab + N * 4 * (int)sizeof(double);
  l.bytes = l.cen + (kHerdtMaxFootsteps + 1) * 64 * (int)sizeof(double);
  return l;
}

// The kernel instance (MM = 0: none, more footsteps than kHerdtMaxFootsteps) and the dynamic LDS
// of a launch; the launcher refuses lds > kLdsCap (N > 702).
struct HerdtShape {
  int MM;
  size_t lds;
};

inline HerdtShape herdt_shape(int N, int max_footsteps) {
  int MM = 0;
  for (int mm : kHerdtMM)
    if (MM == 0 && max_footsteps <= mm) MM = mm;
  return HerdtShape{MM, (size_t)herdt_lds(N).bytes};
}
