// The strict box-QP entry points of the C-ABI layer: the solver of a launch is dispatch.h
// choose_strict's, the launch its backend's (strict_scan.hip, strict_lq.hip, strict.hip).  Host
// code only.
#include "zmpc_internal.h"

namespace {

StrictKind kind_for(const zmpc_plan* p, int64_t ninst) {
  return choose_strict(p->N, ninst, p->opt[ZMPC_OPT_STRICT_SOLVER], p->lqtab != nullptr);
}

}  // namespace

hipError_t zmpc_launch_rollout_strict(const zmpc_plan* p, const RolloutCall& c, hipStream_t s,
                                      std::string* why) {
  if (c.n == 1) {  // no QP solve, whatever the solver: the history is the initial state
    hipError_t e = hipMemcpyAsync(c.hist, c.x0, 6 * sizeof(double) * (size_t)c.B,
                                  hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && c.status) e = hipMemsetAsync(c.status, 0, sizeof(int32_t) * c.B, s);
    return e;
  }
  switch (kind_for(p, 2 * c.B)) {  // an instance per walk and axis
    case StrictKind::Scan: return zmpc_launch_rollout_strict_scan(p, c, s, why);
    case StrictKind::Lq: return zmpc_launch_rollout_strict_lq(p, c, s, why);
    case StrictKind::Wave: return zmpc_launch_rollout_strict_wave(p, c, s, why);
    case StrictKind::Tile: break;
  }
  return zmpc_launch_rollout_strict_tile(p, c, s, why);
}

hipError_t zmpc_launch_step_strict(const zmpc_plan* p, const StepCall& c, hipStream_t s,
                                   std::string* why) {
  switch (kind_for(p, c.B)) {
    case StrictKind::Scan: return zmpc_launch_step_strict_scan(p, c, s, why);
    case StrictKind::Lq: return zmpc_launch_step_strict_lq(p, c, s, why);
    case StrictKind::Wave: return zmpc_launch_step_strict_wave(p, c, s, why);
    case StrictKind::Tile: break;
  }
  return zmpc_launch_step_strict_tile(p, c, s, why);
}
