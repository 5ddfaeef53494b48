// Host check of 2s-agcn_amd/csrc/sgn_v15_stats_plan.h (no HIP), at the ten geometries of tests/sgn_v15_grad_util.py::CASES
// (the table of tests/sgn_v15_wgrad_plan_check.cpp): the partial indices of a pass are disjoint, dense and inside
// part_floats, the counts of its groups sum to N * seg * V (frames) and N * seg (clip), the workspace holds one state per
// clip, invalid kinds and layers are refused, and the domain of a pass is that of the forward launch it is cut from.
#include <stdio.h>
#include <vector>

#include "sgn_v15_stats_plan.h"

static long cases = 0, failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    ++cases;                                                                         \
    if (!(cond)) {                                                                   \
      if (++failures <= 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                                \
  } while (0)

struct Geo { int heads, d_head, ff; };
struct Case { int V, seg; Geo sp, tp; int num_class, N; };
// tests/sgn_v15_grad_util.py::CASES
static const Case CASES[] = {
    {3, 2, {8, 16, 128}, {8, 32, 256}, 60, 2},      {15, 4, {8, 16, 128}, {8, 32, 256}, 60, 1},
    {17, 3, {16, 16, 256}, {16, 16, 128}, 33, 1},   {32, 2, {4, 64, 128}, {2, 64, 384}, 257, 1},
    {2, 32, {1, 128, 128}, {4, 64, 128}, 60, 1},    {5, 3, {2, 128, 256}, {3, 128, 256}, 60, 1},
    {9, 5, {2, 256, 128}, {2, 256, 384}, 60, 1},    {4, 7, {1, 384, 384}, {1, 1024, 1024}, 60, 1},
    {3, 2, {1, 1024, 1024}, {2, 512, 128}, 4096, 1}, {7, 1, {4, 32, 128}, {8, 32, 128}, 60, 2},
};

int main() {
  CHECK(SGN15_STATS_FRAMES == 1 && SGN15_STATS_CLIP == 2);
  CHECK(sgn15_stats_channels(SGN15_STATS_FRAMES) == 128 && sgn15_stats_channels(SGN15_STATS_CLIP) == 256);
  for (const Case& c : CASES) {
    for (int kind : {SGN15_STATS_FRAMES, SGN15_STATS_CLIP}) {
      const Geo& g = kind == SGN15_STATS_FRAMES ? c.sp : c.tp;
      const int C = sgn15_stats_channels(kind);
      const int per = sgn15_stats_groups_per_clip(kind, c.seg);
      CHECK(per == (kind == SGN15_STATS_FRAMES ? c.seg : 1));
      const long groups = sgn15_stats_groups(kind, c.N, c.seg);
      CHECK(groups == (long)c.N * per);
      const long floats = sgn15_stats_part_floats(kind, c.N, c.seg);
      CHECK(floats == groups * 2 * C);
      // every (group, which, channel) has a float of its own, inside the buffer, and together they fill it
      std::vector<char> hit((size_t)floats, 0);
      long samples = 0;
      for (long gi = 0; gi < groups; ++gi) {
        samples += sgn15_stats_group_count(kind, c.seg, c.V);
        for (int which = 0; which < 2; ++which)
          for (int ch = 0; ch < C; ++ch) {
            const long i = sgn_stats_part_index(gi, which, ch, C);
            CHECK(i >= 0 && i < floats);
            if (i >= 0 && i < floats) {
              CHECK(!hit[(size_t)i]);
              hit[(size_t)i] = 1;
            }
          }
      }
      long filled = 0;
      for (char h : hit) filled += h;
      CHECK(filled == floats);
      CHECK(samples == (kind == SGN15_STATS_FRAMES ? (long)c.N * c.seg * c.V : (long)c.N * c.seg));
      // the finalize's workspace: one (3, C) state per clip, and the carry state
      CHECK(sgn15_stats_state_doubles(kind) == 3L * C);
      CHECK(sgn15_stats_workspace_doubles(kind, c.N) == (long)c.N * 3 * C);
      CHECK(sgn_stats_clip_state_index(c.N - 1, 2, C - 1, C) == sgn15_stats_workspace_doubles(kind, c.N) - 1);
      for (int layer = -1; layer <= 4; ++layer) {
        const bool ok = layer == 1 || layer == 2;
        CHECK(sgn15_stats_layer_ok(kind, layer) == ok);
        // the domain is the forward's, for the valid layers only
        const bool fwd = kind == SGN15_STATS_FRAMES ? sgn15_frames_domain(c.N, c.seg, c.V, g.heads, g.d_head, g.ff)
                                                    : sgn15_clip_domain(c.N, c.seg, c.num_class, g.heads, g.d_head, g.ff);
        CHECK(fwd);
        CHECK(sgn15_stats_domain(kind, layer, c.N, c.seg, c.V, g.heads, g.d_head, g.ff) == (ok && fwd));
        CHECK(sgn15_stats_shape_domain(kind, layer, c.N, c.seg, c.V) == ok);
      }
    }
    for (int kind : {-1, 0, 3, 4})
      for (int layer = 0; layer <= 3; ++layer) {
        CHECK(!sgn15_stats_layer_ok(kind, layer));
        CHECK(!sgn15_stats_domain(kind, layer, c.N, c.seg, c.V, c.sp.heads, c.sp.d_head, c.sp.ff));
        CHECK(!sgn15_stats_shape_domain(kind, layer, c.N, c.seg, c.V));
      }
  }
  // the edges of the domain follow the forward: V and the block for a frames pass, seg and the block for a clip pass
  for (int V : {1, 2, 32, 33})
    CHECK(sgn15_stats_domain(SGN15_STATS_FRAMES, 1, 2, 20, V, 8, 16, 128) == sgn15_frames_domain(2, 20, V, 8, 16, 128));
  for (int seg : {0, 1, 32, 33}) {
    CHECK(sgn15_stats_domain(SGN15_STATS_CLIP, 2, 2, seg, 15, 8, 32, 256) == sgn15_clip_domain(2, seg, 60, 8, 32, 256));
    CHECK(sgn15_stats_shape_domain(SGN15_STATS_CLIP, 2, 2, seg, 2) == (seg >= 1 && seg <= 32));
  }
  CHECK(!sgn15_stats_domain(SGN15_STATS_FRAMES, 1, 2, 20, 15, 8, 24, 128));       // a head width outside the block's domain
  CHECK(!sgn15_stats_domain(SGN15_STATS_CLIP, 1, 2, 20, 15, 8, 32, 100));
  CHECK(!sgn15_stats_domain(SGN15_STATS_CLIP, 1, 0, 20, 15, 8, 32, 256));
  printf("%ld cases, %ld failures\n", cases, failures);
  return failures ? 1 : 0;
}
