// The launch rules of csrc/dispatch.h as a stand-alone host program (tests/test_dispatch_host.py):
// one query per line of standard input, one answer per line of standard output.
//   unc N n shared_cop opt_rollout_kernel opt_long_walk opt_correlation
//       -> kind cw w E P sparse lds kc kcp lz lzp kfm fstride lc
//   lq N                                   -> G nlck lds
//   strict N ninst opt_strict_solver has_lq_table -> kind
//   scan N ninst cus                       -> lanes C
//   caps                                   -> wide_lds_cap(2) wide_lds_cap(4) wide_lds_cap(8)
//   herdt N max_footsteps                  -> MM lds fits(lds <= kLdsCap) poly ktab cen
#include <cstdio>
#include <cstring>

#include "dispatch.h"

int main() {
  static const char* unc_names[] = {"Copy", "SplitShared", "Split", "Generic", "Wide", "Chunk"};
  static const char* strict_names[] = {"", "Tile", "Wave", "Lq", "Scan"};
  char tag[16];
  long long a[6];
  while (scanf("%15s", tag) == 1) {
    const int want = !strcmp(tag, "unc") ? 6 : !strcmp(tag, "lq") ? 1 : !strcmp(tag, "strict") ? 4
                     : !strcmp(tag, "scan") ? 3 : !strcmp(tag, "caps") ? 0
                     : !strcmp(tag, "herdt") ? 2 : -1;
    if (want < 0) return 2;
    for (int i = 0; i < want; ++i)
      if (scanf("%lld", &a[i]) != 1) return 2;
    if (!strcmp(tag, "unc")) {
      const UncChoice c = choose_unc((int)a[0], a[1], a[2] != 0, (int)a[3], (int)a[4], (int)a[5]);
      printf("%s %d %d %d %d %d %zu %d %d %d %d %d %d %d\n", unc_names[(int)c.kind], c.cw, c.w, c.E,
             c.P, (int)c.sparse, c.lds, c.kc, c.kcp, c.lz, c.lzp, c.kfm, c.fstride, c.lc);
    } else if (!strcmp(tag, "lq")) {
      const LqShape s = lq_shape((int)a[0]);
      printf("%d %d %zu\n", s.G, s.nlck, s.lds);
    } else if (!strcmp(tag, "strict")) {
      printf("%s\n", strict_names[(int)choose_strict((int)a[0], a[1], (int)a[2], a[3] != 0)]);
    } else if (!strcmp(tag, "scan")) {
      const ScanShape s = scan_shape((int)a[0], a[1], (int)a[2]);
      printf("%d %d\n", s.lanes, s.C);
    } else if (!strcmp(tag, "herdt")) {
      const HerdtShape s = herdt_shape((int)a[0], (int)a[1]);
      const HerdtLds l = herdt_lds((int)a[0]);
      printf("%d %zu %d %d %d %d\n", s.MM, s.lds, (int)(s.lds <= kLdsCap), l.poly, l.ktab, l.cen);
    } else {
      printf("%zu %zu %zu\n", wide_lds_cap(2), wide_lds_cap(4), wide_lds_cap(8));
    }
  }
  return 0;
}
