// Geometry of the SGN batch-statistics passes (sgn_stats.hip): which BatchNorm a pass measures, how many channels and
// groups its partial buffer has, where a group's numbers lie and how many samples the group stands for.  A group is what
// one workgroup (or one row tile of it) reduces on its own: a clip of the input pass, a frame of a frames pass, a
// (clip, tile) of a clip pass.  The finalize merges the groups of a clip in ascending group index and then the clips in
// ascending clip index (so the order is a function of the group index alone and a chunk of whole clips merges as it does
// inside the whole batch), and takes every count from here: the kernels emit no counts.  Plain C++17 without HIP, like
// sgn_plan.h: tests/sgn_stats_plan_check.cpp compiles it with the host compiler.
#pragma once
#include "sgn_plan.h"

#define SGN_STATS_INPUT 0      // joint_embed.cnn.0.bn and dif_embed.cnn.0.bn: 2 * 3V features [which][v*3 + c]
#define SGN_STATS_FRAMES 1     // gcn<layer>.bn, layer 1..3
#define SGN_STATS_CLIP 2       // cnn.bn<layer>, layer 1..2
#define SGN_STATS_THREADS 64   // finalize: one thread per channel

SGN_HD bool sgn_stats_layer_ok(int kind, int layer) {
  return kind == SGN_STATS_INPUT ? layer == 0
         : kind == SGN_STATS_FRAMES ? layer >= 1 && layer <= 3
         : kind == SGN_STATS_CLIP   ? layer >= 1 && layer <= 2
                                    : false;
}
// the domain of a pass: that of the forward launch it is cut from (V is not read by a clip pass)
SGN_HD bool sgn_stats_domain(int kind, int layer, long N, int seg, int V) {
  if (!sgn_stats_layer_ok(kind, layer)) return false;
  return kind == SGN_STATS_CLIP ? sgn_clip_domain(N, seg, 1) : sgn_frames_domain(N, seg, V);
}
SGN_HD int sgn_stats_channels(int kind, int layer, int V) {
  return kind == SGN_STATS_INPUT ? 2 * 3 * V
         : kind == SGN_STATS_FRAMES ? (layer == 1 ? SGN_C2 : SGN_C3)
                                    : (layer == 1 ? SGN_C3 : SGN_C4);
}
SGN_HD int sgn_stats_groups_per_clip(int kind, int seg) {
  return kind == SGN_STATS_INPUT ? 1 : kind == SGN_STATS_FRAMES ? seg : sgn_clip_tiles(seg);
}
SGN_HD long sgn_stats_groups(int kind, long N, int seg) { return N * sgn_stats_groups_per_clip(kind, seg); }
// samples of group g: seg frames of a clip, V joints of a frame, the valid rows of a tile
SGN_HD int sgn_stats_group_count(int kind, long g, int seg, int V) {
  return kind == SGN_STATS_INPUT ? seg
         : kind == SGN_STATS_FRAMES ? V
                                    : sgn_tile_rows((int)(g % sgn_clip_tiles(seg)), seg);
}
// partial buffer (groups, 2, C) floats: the sum, then M2 = the sum of squares about the group's own mean
SGN_HD long sgn_stats_part_index(long g, int which, int c, int C) { return (g * 2 + which) * C + c; }
SGN_HD long sgn_stats_part_floats(int kind, int layer, long N, int seg, int V) {
  return sgn_stats_groups(kind, N, seg) * 2 * sgn_stats_channels(kind, layer, V);
}
// carry state of the finalize (doubles): (3, C) = count, mean, M2 of everything merged so far; its workspace holds one
// such state per clip, (N, 3, C)
SGN_HD long sgn_stats_state_doubles(int kind, int layer, int V) { return 3L * sgn_stats_channels(kind, layer, V); }
SGN_HD long sgn_stats_clip_state_index(long n, int which, int c, int C) { return (n * 3 + which) * C + c; }
SGN_HD long sgn_stats_workspace_doubles(int kind, int layer, long N, int V) {
  return N * sgn_stats_state_doubles(kind, layer, V);
}
