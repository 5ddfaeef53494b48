// Geometry and index arithmetic of the SGN v15 input-gradient kernels (sgn_v15_bwd.hip, the block backward in
// sgn_v15_device.h): the transposed weight images, the LDS carve with the lifetime of every band, and the workspace of
// the dif coupling.  Plain C++17 without HIP, like sgn_v15_plan.h which it builds on: the kernels and launchers include
// it, tests/sgn_v15_bwd_plan_check.cpp compiles it with the host compiler.
//
// With the forward's notation (sgn_v15_plan.h) and dy (R rows x DOUT) holding one non-zero per column, at the arg-max
// row of that column:
//   dx1  = dy Wr^T + sum_c (dy W2_c^T * [hidden_c > 0]) W1_c^T         over the 128-column FFN chunks c, ascending
//   per 128-column group g, ascending:   do = dx1 Wo_g^T;   per head dP = do_h v_h^T, dv_h = P^T do_h,
//        dS = P * (dP - rowsum(dP * P)), dq = dS k, dk = dS^T q;   dX += [dq | dk | dv]_g (Wqkv_g)^T
//   dX starts from dx1, the attention residual.  d_head^-1/2 and both BatchNorms are folded into the images.
//
// Where it can go wrong:
//   padded rows   The arg-max runs over the real rows only, from -inf.  The recomputed hidden rows >= R hold bias garbage;
//                 they meet rows of dy that are zero, so dh and dx1 are zero there.  P's padded rows and columns are zero,
//                 hence dS's: dk = dS^T q and dv = P^T do take nothing from the padded query rows, whose q is garbage.
//   d_head 16     Two heads share a 32-column MFMA block: dv, dq and dk of the block are formed with both heads' P / dS
//                 and selected per lane (r >= 16), as a . v in the forward.  dP has K = 16.
//   sliced heads  (d_head = k * 128) pass 1: the scores of all slices -> P, the forward's code.  pass 2: dP = sum over
//                 the slices of do_s v_s^T, each wave its own 32-column quarter of every slice, the four partials added in
//                 wave order, then dS.  pass 3: dq_s, dk_s, dv_s and the product with (Wqkv_s)^T slice by slice.  [q | k | v]
//                 of a slice is recomputed up to three times, do_s twice.
#pragma once
#include "sgn_v15_plan.h"

// ---- transposed sections of one block (floats).  The backward products are dZ . W^T; every matrix is stored (N, K)
// row-major = W^T of the forward image's section, so the 32 lanes of an MFMA B operand read 32 consecutive floats.
// Biases, the 3 -> 64 layers, aff, tem and fc are read from the forward image. ----
struct Sgn15BlockWT {
  long qkv;                    // (3 inner, DIN)
  long o;                      // (DIN, inner)
  long f1;                     // (ff, DIN)
  long f2;                     // (DOUT, ff + DIN) = [W2 ; Wr]^T
  long end;
};
SGN_HD Sgn15BlockWT sgn15_block_wt(long base, int din, int dout, int heads, int d_head, int ff) {
  Sgn15BlockWT w;
  const long inner = (long)heads * d_head;
  long o = base;
  w.qkv = o; o += 3 * inner * din;
  w.o = o;   o += din * inner;
  w.f1 = o;  o += (long)ff * din;
  w.f2 = o;  o += (long)dout * (ff + din);
  w.end = o;
  return w;
}
// frames: the second layers of the two embeddings, (64, 64) each, then the block
struct Sgn15FramesWT {
  long je2, de2;
  Sgn15BlockWT blk;
  long total;
};
SGN_HD Sgn15FramesWT sgn15_frames_wt(int heads, int d_head, int ff) {
  Sgn15FramesWT w;
  w.je2 = 0;
  w.de2 = SGN_C1 * SGN_C1;
  w.blk = sgn15_block_wt(2 * SGN_C1 * SGN_C1, SGN15_SPA_IN, SGN15_SPA_OUT, heads, d_head, ff);
  w.total = w.blk.end;
  return w;
}
// clip: the block alone
struct Sgn15ClipWT {
  Sgn15BlockWT blk;
  long total;
};
SGN_HD Sgn15ClipWT sgn15_clip_wt(int heads, int d_head, int ff) {
  Sgn15ClipWT w;
  w.blk = sgn15_block_wt(0, SGN15_SPA_OUT, SGN15_TEM_OUT, heads, d_head, ff);
  w.total = w.blk.end;
  return w;
}

// ---- the dif coupling: as in the base SGN, frame f writes dj[f] and dd[f] (V * 3 floats each) to the workspace and a
// second launch combines dx[t] = dj[t] + dd[t] [t > 0] - dd[t + 1] [t + 1 < seg] (sgn_plan.h: sgn_dif_*) ----
SGN_HD size_t sgn15_frames_bwd_ws_floats(long N, int seg, int V) {
  return (size_t)2 * (size_t)N * (size_t)seg * (size_t)(V * 3);
}

// ---- LDS (floats).  The forward's carve would need x AND dx1 resident at DIN = 256 next to [q | k | v], a do band and
// eight P slots: 2 * 8224 + 12320 + 4128 + 8448 = 41344 > 40960.  What gives: dx1 and dX never live in LDS.  dx1 stays in
// the accumulators it was summed in (wave w owns the column blocks w, w + 4, ... of all 32 rows), dX starts as a copy of
// them, and for do = dx1 Wo_g^T each 128-column half of dx1 is staged through the DO band, which do then takes.
//   X      (32, DIN + 1)       x -> x1 in place (forward) -> x again for the group walk (the frames kernel copies it back
//                              from X0, the clip kernel reloads feat + tem)
//   QKV    (32, 385)           forward: as there.  Then, together with DO: the dense dy (32, DOUT + 1).  Group walk:
//                              [q | k | v] of a group, overwritten by [dq | dk | dv].  Frames kernel, at the end: the
//                              second embedding layers' activations / gradients [0, 128), d(first layers) [128, 256)
//   DO     (32, 129)           directly behind QKV.  a 128-column half of dx1, then do of the group
//   P      (8, 32, 33)         forward: as there.  FFN backward: the masked dh chunk (32, 129).  Group walk: the P of the
//                              group's heads, each overwritten by its dS; for a sliced head slot 0 = P, 1..4 = the waves'
//                              K-split partials (scores, then dP), slot 5 = dS
//   MISC   512                 frames: xin (2, 32, 4); clip: d pooled (512)
//   X0, E1 (32, 129) each      frames kernel only: the copy of x0 = [pos + vel | spa] and the first embedding layers'
//                              activations (masks, and the operand of the recomputed second layers) ----
#define SGN15_BWD_DO_STRIDE (SGN15_GROUP + 1)   // 129
#define SGN15_BWD_DS_SLOT 5
#define SGN15_BWD_LDS_X 0
#define SGN15_BWD_LDS_QKV(DIN) (SGN15_BWD_LDS_X + SGN_VP * SGN15_X_STRIDE(DIN))
#define SGN15_BWD_LDS_DO(DIN) (SGN15_BWD_LDS_QKV(DIN) + SGN_VP * SGN15_QKV_STRIDE)
#define SGN15_BWD_LDS_P(DIN) (SGN15_BWD_LDS_DO(DIN) + SGN_VP * SGN15_BWD_DO_STRIDE)
#define SGN15_BWD_LDS_MISC(DIN) (SGN15_BWD_LDS_P(DIN) + SGN15_P_SLOTS * SGN15_P_SLOT)
#define SGN15_BWD_LDS_BLOCK(DIN) (SGN15_BWD_LDS_MISC(DIN) + 512)
#define SGN15_BWD_LDS_X0 SGN15_BWD_LDS_BLOCK(SGN15_SPA_IN)
#define SGN15_BWD_LDS_E1 (SGN15_BWD_LDS_X0 + SGN_VP * SGN15_X_STRIDE(SGN15_SPA_IN))
#define SGN15_FRAMES_BWD_LDS_FLOATS (SGN15_BWD_LDS_E1 + SGN_VP * SGN15_BWD_DO_STRIDE)
#define SGN15_CLIP_BWD_LDS_FLOATS SGN15_BWD_LDS_BLOCK(SGN15_SPA_OUT)
#define SGN15_BWD_DY_STRIDE(DOUT) ((DOUT) + 1)
static_assert(SGN15_FRAMES_BWD_LDS_FLOATS * 4 <= SGN_LDS_LIMIT, "agcn_sgn15_frames_bwd: LDS");
static_assert(SGN15_CLIP_BWD_LDS_FLOATS * 4 <= SGN_LDS_LIMIT, "agcn_sgn15_clip_bwd: LDS");
static_assert((2 * SGN_VP * SGN15_X_STRIDE(SGN15_SPA_OUT) + SGN_VP * SGN15_QKV_STRIDE + SGN_VP * SGN15_BWD_DO_STRIDE +
               SGN15_P_SLOTS * SGN15_P_SLOT) * 4 > SGN_LDS_LIMIT,
              "x and dx1 would both fit at DIN = 256: no staging of dx1 needed");
static_assert(SGN_VP * SGN15_BWD_DY_STRIDE(SGN15_TEM_OUT) <= SGN_VP * (SGN15_QKV_STRIDE + SGN15_BWD_DO_STRIDE),
              "the dense dy fits QKV + DO");
static_assert(SGN_VP * SGN15_BWD_DO_STRIDE <= SGN15_P_SLOTS * SGN15_P_SLOT, "the dh chunk fits P");
static_assert(SGN15_BWD_DS_SLOT > SGN_WAVES && SGN15_BWD_DS_SLOT < SGN15_P_SLOTS, "a sliced head: P, four partials, dS");
static_assert(SGN15_GROUP / SGN15_MIN_HEAD == 2 * SGN_WAVES, "a wave owns at most two heads of a group");
static_assert(2 * SGN_C2 <= SGN15_QKV_STRIDE - 1, "the embedding backward's two bands fit QKV");

// The lifetimes above as data, for the host check: band, first float, floats, first and last step it is live in.
// Steps: 0 the tokens (frames: embeddings), 1 the forward (x -> x1), 2 dy routed to the arg-max rows, 3 FFN backward,
// 4 x again, 5 the group walk, 6 the embeddings' backward (frames).
struct Sgn15BwdLife { const char* name; int first_float, floats, first, last; };
#define SGN15_BWD_BLOCK_LIVES(DIN, DOUT)                                                                             \
  {"x -> x1 in place", SGN15_BWD_LDS_X, SGN_VP * SGN15_X_STRIDE(DIN), 0, 3},                                         \
  {"x again", SGN15_BWD_LDS_X, SGN_VP * SGN15_X_STRIDE(DIN), 4, 5},                                                  \
  {"forward q|k|v, hidden", SGN15_BWD_LDS_QKV(DIN), SGN_VP * SGN15_QKV_STRIDE, 1, 1},                                \
  {"forward P", SGN15_BWD_LDS_P(DIN), SGN15_P_SLOTS * SGN15_P_SLOT, 1, 1},                                           \
  {"dy", SGN15_BWD_LDS_QKV(DIN), SGN_VP * SGN15_BWD_DY_STRIDE(DOUT), 2, 3},                                          \
  {"dh chunk", SGN15_BWD_LDS_P(DIN), SGN_VP * SGN15_BWD_DO_STRIDE, 3, 3},                                            \
  {"q|k|v -> dq|dk|dv", SGN15_BWD_LDS_QKV(DIN), SGN_VP * SGN15_QKV_STRIDE, 5, 5},                                    \
  {"dx1 half -> do", SGN15_BWD_LDS_DO(DIN), SGN_VP * SGN15_BWD_DO_STRIDE, 5, 5},                                     \
  {"P -> dS", SGN15_BWD_LDS_P(DIN), SGN15_P_SLOTS * SGN15_P_SLOT, 5, 5}
static const Sgn15BwdLife SGN15_FRAMES_BWD_LIVES[] = {
    SGN15_BWD_BLOCK_LIVES(SGN15_SPA_IN, SGN15_SPA_OUT),
    {"xin", SGN15_BWD_LDS_MISC(SGN15_SPA_IN), 2 * SGN_VP * 4, 0, 0},
    {"x0 copy", SGN15_BWD_LDS_X0, SGN_VP * SGN15_X_STRIDE(SGN15_SPA_IN), 0, 4},
    {"E1", SGN15_BWD_LDS_E1, SGN_VP * SGN15_BWD_DO_STRIDE, 0, 6},
    {"d embed", SGN15_BWD_LDS_QKV(SGN15_SPA_IN), SGN_VP * SGN15_QKV_STRIDE, 6, 6},
};
static const Sgn15BwdLife SGN15_CLIP_BWD_LIVES[] = {
    SGN15_BWD_BLOCK_LIVES(SGN15_SPA_OUT, SGN15_TEM_OUT),
    {"d pooled", SGN15_BWD_LDS_MISC(SGN15_SPA_OUT), SGN15_TEM_OUT, 0, 2},
};
