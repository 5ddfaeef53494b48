// Host check of 2s-agcn_amd/csrc/dadj_plan.h (no HIP): the channel of dy that gcn_dadj_chain_kernel stages into element
// e of group og of stage s, against the channel whose weight dadj_pack_kernel puts at the same position of the image.
// Swept over every Cout in 1..300 and every stage.  Checked: a staged channel is never negative and never reaches Cout;
// wherever the weight image holds a weight (channel < Cout), the staged element is live and comes from that very
// channel; wherever an element is staged as zero or the weight is zero, nothing reaches the sum; every channel of dy
// is met exactly once, so that the staged contraction, done in integers, equals sum_o w[o] dy[o].
#include <stdio.h>
#include <vector>

#include "dadj_plan.h"

static long cases = 0, failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    ++cases;                                                                         \
    if (!(cond)) {                                                                   \
      if (++failures <= 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                                \
  } while (0)

int main() {
  for (int Cout = 1; Cout <= 300; ++Cout) {
    const int S = dadj_stages(Cout);
    CHECK(S * DADJ_KC >= Cout && (S - 1) * DADJ_KC < Cout);
    std::vector<int> met(Cout, 0);
    long staged = 0, direct = 0;
    for (int o = 0; o < Cout; ++o) direct += (long)(3 * o + 1) * (7 * o + 5);      // w[o] = 3o + 1, dy[o] = 7o + 5
    for (int s = 0; s < S; ++s)
      for (int og = 0; og < 4; ++og) {
        const int ks = og >> 1, h = og & 1;
        const int o0 = dadj_stage_first(s, og);
        const int nv = dadj_stage_count(o0, Cout);
        CHECK(nv >= 0 && nv <= 8);
        for (int e = 0; e < 8; ++e) {
          const int src = dadj_stage_channel(o0, e, Cout);
          const bool live = dadj_stage_live(o0, e, Cout);
          const int wo = dadj_pack_channel(s, ks, h, e);
          const bool wlive = dadj_pack_live(wo, Cout);
          CHECK(src >= 0);
          CHECK(src < Cout);
          CHECK(live == (e < nv));
          CHECK(!wlive || (live && src == wo));       // a weight meets its own channel
          CHECK(!live || wlive);                      // nothing is staged against a position the image zeroes
          if (live && src >= 0 && src < Cout) ++met[src];
          const long w = wlive ? 3L * wo + 1 : 0, d = (live && src >= 0 && src < Cout) ? 7L * src + 5 : 0;
          staged += w * d;
        }
      }
    for (int o = 0; o < Cout; ++o) CHECK(met[o] == 1);
    CHECK(staged == direct);
  }
  printf("%ld cases, %ld failures\n", cases, failures);
  return failures ? 1 : 0;
}
