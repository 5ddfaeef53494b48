// Geometry of the SGN v15 batch-statistics passes (sgn_v15_stats.hip): which of the four block BatchNorms a pass
// measures, how many channels and groups its partial buffer has and how many samples a group stands for.  The two input
// BatchNorms (the DataNorms) are measured by the base SGN's input pass (sgn_stats_plan.h: SGN_STATS_INPUT), the same
// [v*3 + c] computation.  A group is what one workgroup reduces on its own: a frame of a frames pass (its V joints), a
// clip of a clip pass (its seg frames).  Partial and state indexing are the base's (sgn_stats_part_index,
// sgn_stats_clip_state_index); the finalize merges the groups of a clip in ascending group index and then the clips in
// ascending clip index, and takes every count from here: the kernels emit no counts.
//
// A pass is the fused forward cut off at one BatchNorm and never reads a section that depends on the BatchNorm it
// measures: the n_a passes (layer 1) read no block section at all -- the frames pass stops at the complete token tile
// X = [pos + vel | spa], the clip pass at feat + tem -- and the n_f passes (layer 2) read qkv_w, qkv_b, o_w, o_b and never
// f1_* or f2_* (nor fc_*).  So, unlike the base model's passes, no "identity" fold is needed: the images of a pass only
// need the EARLIER BatchNorms on their batch statistics, and whatever the later sections hold is not looked at.
// Plain C++17 without HIP: tests/sgn_v15_stats_plan_check.cpp compiles it with the host compiler.
#pragma once
#include "sgn_stats_plan.h"
#include "sgn_v15_plan.h"

#define SGN15_STATS_FRAMES 1   // spatial block: layer 1 = layers.l1.attn.norm.fn (n_a, on x), 2 = layers.l1.ffn.norm.fn (n_f, on x1)
#define SGN15_STATS_CLIP 2     // temporal block: the same two layers

SGN_HD bool sgn15_stats_layer_ok(int kind, int layer) {
  return (kind == SGN15_STATS_FRAMES || kind == SGN15_STATS_CLIP) && layer >= 1 && layer <= 2;
}
// both BatchNorms of a block see its input width: x and x1 = attention + bo + x
SGN_HD int sgn15_stats_channels(int kind) { return kind == SGN15_STATS_FRAMES ? SGN15_SPA_IN : SGN15_SPA_OUT; }
SGN_HD int sgn15_stats_groups_per_clip(int kind, int seg) { return kind == SGN15_STATS_FRAMES ? seg : 1; }
SGN_HD long sgn15_stats_groups(int kind, long N, int seg) { return N * sgn15_stats_groups_per_clip(kind, seg); }
// samples of a group: the V joints of a frame, the seg frames of a clip (padded rows take no part)
SGN_HD int sgn15_stats_group_count(int kind, int seg, int V) { return kind == SGN15_STATS_FRAMES ? V : seg; }
// partial buffer (groups, 2, C) floats, finalize workspace (N, 3, C) doubles, carry state (3, C) doubles
SGN_HD long sgn15_stats_part_floats(int kind, long N, int seg) {
  return sgn15_stats_groups(kind, N, seg) * 2 * sgn15_stats_channels(kind);
}
SGN_HD long sgn15_stats_state_doubles(int kind) { return 3L * sgn15_stats_channels(kind); }
SGN_HD long sgn15_stats_workspace_doubles(int kind, long N) { return N * sgn15_stats_state_doubles(kind); }
// the domain of a pass: that of the forward launch it is cut from (V is not read by a clip pass, num_class by neither)
SGN_HD bool sgn15_stats_domain(int kind, int layer, long N, int seg, int V, int heads, int d_head, int ff) {
  if (!sgn15_stats_layer_ok(kind, layer)) return false;
  return kind == SGN15_STATS_FRAMES ? sgn15_frames_domain(N, seg, V, heads, d_head, ff)
                                    : sgn15_clip_domain(N, seg, 1, heads, d_head, ff);
}
// ... of the size queries and the finalize, which do not depend on the block's heads: any block inside its domain
SGN_HD bool sgn15_stats_shape_domain(int kind, int layer, long N, int seg, int V) {
  return sgn15_stats_domain(kind, layer, N, seg, V, SGN15_GROUP / SGN15_MIN_HEAD, SGN15_MIN_HEAD, SGN15_GROUP);
}
