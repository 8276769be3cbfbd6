// The fused rollout-to-metrics launch rule of csrc/dispatch.h beside the rollout's own, as a
// stand-alone host program (tests/test_dispatch_metrics_host.py): one query per line of standard
// input, one answer per line of standard output.
//   N n shared_cop opt_rollout_kernel opt_correlation
//       -> unc_kind unc_cw unc_sparse unc_kc unc_kcp unc_lz unc_lzp unc_kfm unc_fstride unc_lds
//          met_kind met_cw met_sparse met_kc met_kcp met_lz met_lzp met_kfm met_fstride met_lds
//          has_reason
#include <cstdio>

#include "dispatch.h"

int main() {
  static const char* unc_names[] = {"Copy", "SplitShared", "Split", "Generic", "Wide", "Chunk"};
  static const char* met_names[] = {"None", "Sample0", "Split", "SplitShared"};
  long long a[5];
  while (scanf("%lld %lld %lld %lld %lld", &a[0], &a[1], &a[2], &a[3], &a[4]) == 5) {
    const UncChoice c = choose_unc((int)a[0], a[1], a[2] != 0, (int)a[3], 0, (int)a[4]);
    const MetChoice m = choose_unc_metrics((int)a[0], a[1], a[2] != 0, (int)a[3], (int)a[4]);
    printf("%s %d %d %d %d %d %d %d %d %zu %s %d %d %d %d %d %d %d %d %zu %d\n",
           unc_names[(int)c.kind], c.cw, (int)c.sparse, c.kc, c.kcp, c.lz, c.lzp, c.kfm, c.fstride,
           c.lds, met_names[(int)m.kind], m.cw, (int)m.sparse, m.kc, m.kcp, m.lz, m.lzp, m.kfm,
           m.fstride, m.lds, (int)(m.why != nullptr && m.why[0] != '\0'));
  }
  return 0;
}
