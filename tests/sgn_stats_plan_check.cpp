// Host check of 2s-agcn_amd/csrc/sgn_stats_plan.h (no HIP): the partial buffers of the SGN batch-statistics passes.  For
// V 2..32, seg across the 32-frame tile boundary and N 1..3: every (group, sum | M2, channel) has its own offset below the
// size, the count the finalize takes for a group is what the pass reduced, the counts add up to the samples a BatchNorm
// sees, and a batch cut into chunks of whole clips has the same groups with the same counts in the same order.
#include <stdio.h>

#include "sgn_stats_plan.h"

static long cases = 0, failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    ++cases;                                                                         \
    if (!(cond)) {                                                                   \
      if (++failures <= 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                                \
  } while (0)

int main() {
  const int segs[] = {1, 2, 12, 20, 31, 32, 33, 34, 63, 64, 65, 100};
  const int passes[][2] = {{SGN_STATS_INPUT, 0}, {SGN_STATS_FRAMES, 1}, {SGN_STATS_FRAMES, 2},
                           {SGN_STATS_FRAMES, 3}, {SGN_STATS_CLIP, 1},   {SGN_STATS_CLIP, 2}};
  for (int V = 2; V <= SGN_MAX_V; ++V)
    for (int seg : segs)
      for (int N = 1; N <= 3; ++N)
        for (const auto& p : passes) {
          const int kind = p[0], layer = p[1];
          CHECK(sgn_stats_domain(kind, layer, N, seg, V));
          const int C = sgn_stats_channels(kind, layer, V);
          const long groups = sgn_stats_groups(kind, N, seg), total = sgn_stats_part_floats(kind, layer, N, seg, V);
          CHECK(C == (kind == SGN_STATS_INPUT ? 6 * V : kind == SGN_STATS_FRAMES ? (layer == 1 ? 128 : 256) : layer == 1 ? 256 : 512));
          CHECK(C <= (kind == SGN_STATS_INPUT ? SGN_THREADS : SGN_C4));
          CHECK(total == groups * 2 * C);
          CHECK(sgn_stats_state_doubles(kind, layer, V) == 3L * C);
          // the finalize's workspace: a (count, mean, M2) state per clip, dense, and the clip of a group
          CHECK(sgn_stats_workspace_doubles(kind, layer, N, V) == 3L * C * N);
          CHECK(sgn_stats_clip_state_index(N - 1, 2, C - 1, C) == sgn_stats_workspace_doubles(kind, layer, N, V) - 1);
          CHECK(sgn_stats_clip_state_index(0, 0, 0, C) == 0 && sgn_stats_clip_state_index(0, 1, 0, C) == C);
          CHECK(groups == (long)N * sgn_stats_groups_per_clip(kind, seg));
          CHECK(sgn_stats_groups_per_clip(kind, seg) == (kind == SGN_STATS_INPUT ? 1 : kind == SGN_STATS_FRAMES ? seg : (seg + 31) / 32));
          // offsets: dense, ascending in (group, which, channel), the last one is the size minus one
          long next = 0, samples = 0;
          for (long g = 0; g < groups; ++g) {
            for (int which = 0; which < 2; ++which) {
              CHECK(sgn_stats_part_index(g, which, 0, C) == next);
              CHECK(sgn_stats_part_index(g, which, C - 1, C) == next + C - 1);
              next += C;
            }
            // the count the finalize assumes = what the pass reduced for this group
            const int cnt = sgn_stats_group_count(kind, g, seg, V);
            if (kind == SGN_STATS_INPUT) CHECK(cnt == seg);                      // the seg frames of clip g, t = 0 included
            if (kind == SGN_STATS_FRAMES) CHECK(cnt == V);                       // the real joint rows of frame g
            if (kind == SGN_STATS_CLIP) {                                        // the valid rows of tile g % tiles
              const int tiles = sgn_clip_tiles(seg), tile = (int)(g % tiles);
              CHECK(cnt == sgn_tile_rows(tile, seg) && cnt >= 1 && cnt <= SGN_VP);
              int real = 0;
              for (int row = 1; row <= SGN_VP; ++row) real += sgn_tile_frame(tile, row, seg) >= 0;
              CHECK(cnt == real);
            }
            samples += cnt;
          }
          CHECK(next == total);
          CHECK(samples == (kind == SGN_STATS_FRAMES ? (long)N * seg * V : (long)N * seg));
          // chunks of whole clips: the groups of a chunk that starts at clip n0 are the batch's groups from
          // sgn_stats_groups(n0) on, with the same counts
          for (int n0 = 1; n0 < N; ++n0) {
            const long g0 = sgn_stats_groups(kind, n0, seg);
            CHECK(g0 + sgn_stats_groups(kind, N - n0, seg) == groups);
            for (long g = 0; g < groups - g0; ++g)
              CHECK(sgn_stats_group_count(kind, g, seg, V) == sgn_stats_group_count(kind, g0 + g, seg, V));
          }
        }
  // layers and domains
  CHECK(!sgn_stats_layer_ok(SGN_STATS_FRAMES, 0) && !sgn_stats_layer_ok(SGN_STATS_FRAMES, 4));
  CHECK(!sgn_stats_layer_ok(SGN_STATS_CLIP, 0) && !sgn_stats_layer_ok(SGN_STATS_CLIP, 3));
  CHECK(!sgn_stats_layer_ok(SGN_STATS_INPUT, 1) && !sgn_stats_layer_ok(3, 1) && !sgn_stats_layer_ok(-1, 0));
  CHECK(!sgn_stats_domain(SGN_STATS_FRAMES, 1, 5, 20, 33) && !sgn_stats_domain(SGN_STATS_FRAMES, 1, 5, 20, 1));
  CHECK(!sgn_stats_domain(SGN_STATS_INPUT, 0, 0, 20, 15) && !sgn_stats_domain(SGN_STATS_CLIP, 2, 5, 0, 15));
  CHECK(!sgn_stats_domain(SGN_STATS_FRAMES, 3, 1L << 30, 20, 15));
  // the largest partial buffers of the two domains, computed in long
  CHECK(sgn_stats_part_floats(SGN_STATS_FRAMES, 3, 0x7fffffffL / (SGN_MAX_V * SGN_MAX_V), 1, 32) ==
        (0x7fffffffL / 1024) * 512);
  CHECK(sgn_stats_part_floats(SGN_STATS_CLIP, 2, 0x7fffffffL / SGN_MAX_CLASS, 1 << 20, 2) ==
        (0x7fffffffL / 4096) * (1L << 15) * 1024);
  printf("%ld cases, %ld failures\n", cases, failures);
  return failures ? 1 : 0;
}
