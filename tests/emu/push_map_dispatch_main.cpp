// The push-map launch rule of csrc/dispatch.h (choose_push_map) as a stand-alone host program
// (tests/test_push_map_host.py): one query per line of standard input, one answer per line of
// standard output.
//   n single_step -> ok waves lds max_n has_reason
#include <cstdio>

#include "dispatch.h"

int main() {
  long long n, single;
  while (scanf("%lld %lld", &n, &single) == 2) {
    const PushMapChoice c = choose_push_map(n, single != 0);
    printf("%d %d %zu %lld %d\n", (int)c.ok, c.waves, c.lds, (long long)kPushMapMaxN,
           (int)(c.why != nullptr && c.why[0] != '\0'));
  }
  return 0;
}
