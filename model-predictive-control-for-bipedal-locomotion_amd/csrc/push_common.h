// What the push-map units share (pushmap.hip: zmpc_push_map; pushshaped.hip:
// zmpc_push_map_shaped): the 16-byte pairs and the candidate arithmetic.  Both units form their
// candidates with push_cand and push_pair, uncontracted, which is what makes their results agree
// bit for bit.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace {

#pragma clang fp contract(off)

struct pair_t {
  double x, y;
};

struct ipair_t {
  int32_t x, y;
};

// The candidate of one margin x >= 0 under a response of magnitude ra with reciprocal q; `fast`:
// q is a positive normal number
__device__ __forceinline__ double push_cand(double x, double q, double ra, bool fast) {
  return fast ? x * q : x / ra;
}

// One (sample, step) pair in both directions: mi = (up_i, dn_i) of sample i.  POS: r_d > 0 (a +y push raises the ZMP: up limits
// +, dn limits −).  Strict <: of equal candidates the first one met stays.
template <bool POS>
__device__ __forceinline__ void push_pair(const pair_t mi, int i, double q, double ra,
                                          const bool fast, double& f0, double& f1, int& i0,
                                          int& i1) {
  const double c0 = push_cand(POS ? mi.x : mi.y, q, ra, fast);
  const double c1 = push_cand(POS ? mi.y : mi.x, q, ra, fast);
  if (c0 < f0) {
    f0 = c0;
    i0 = i;
  }
  if (c1 < f1) {
    f1 = c1;
    i1 = i;
  }
}

// Walks per workgroup of the single-step kernels (one wave each)
constexpr int kStepWaves = 4;

}  // namespace
