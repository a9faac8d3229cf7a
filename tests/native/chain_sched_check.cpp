// Host check of ops/csrc/chain_sched.h (tests/test_chain_sched.py): for every tile count 0..2000 and
// every grid 1..520, the blocks of the persistent conv_chain form take every tile exactly once.
#include <cstdio>
#include <cstring>

#include "chain_sched.h"

int main() {
  static unsigned char taken[2048];
  for (int G = 1; G <= 520; ++G) {
    for (int T = 0; T <= 2000; ++T) {
      std::memset(taken, 0, sizeof(taken));
      for (int b = 0; b < G; ++b)
        for (int t = chain_first_tile(b, G); t < T; t = chain_next_tile(t, G)) {
          if (t < 0) {
            std::printf("NEGATIVE tile G=%d T=%d block=%d tile=%d\n", G, T, b, t);
            return 1;
          }
          ++taken[t];
        }
      for (int t = 0; t < T; ++t)
        if (taken[t] != 1) {
          std::printf("MISMATCH G=%d T=%d tile=%d taken %d times\n", G, T, t, (int)taken[t]);
          return 1;
        }
    }
  }
  std::printf("chain_sched: ok\n");
  return 0;
}
