// The launch rule of zmpc_push_map_shaped (csrc/dispatch.h choose_push_shaped) as a stand-alone
// host program (tests/test_push_shaped_host.py): one query per line of standard input, one
// answer per line of standard output.
//   n single_step naxes -> ok waves lds | reason (empty where the shape is taken)
#include <cstdio>

#include "dispatch.h"

int main() {
  long long n, single, naxes;
  while (scanf("%lld %lld %lld", &n, &single, &naxes) == 3) {
    const PushMapChoice c = choose_push_shaped(n, single != 0, (int)naxes);
    printf("%d %d %zu | %s\n", (int)c.ok, c.waves, c.lds, c.why ? c.why : "");
  }
  return 0;
}
