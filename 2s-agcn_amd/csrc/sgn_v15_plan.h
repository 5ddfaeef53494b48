// Geometry and index arithmetic of the SGN v15 inference kernels (sgn_v15.hip): the layout of the two folded weight
// images, the column-group walk of the attention block, the chunk walk of its feed-forward, and the LDS carve.
// Plain C++17 without HIP: sgn_v15.hip and sgn_v15_device.h include it for the launchers AND the kernels (SGN_HD), and
// tests/sgn_v15_plan_check.cpp compiles it with the host compiler.
//
// One block (reference model/layers/attention/crossattention.py::Transformer, pre-norm, one layer) maps R <= 32 token
// rows of width DIN to width DOUT:
//   a  = softmax_j((n_a(x) Wq)(n_a(x) Wk)^T d_head^-1/2) per head,   x1 = concat_h(a . n_a(x) Wv) Wo + bo + x,
//   y  = relu(n_f(x1) W1 + b1) W2 + b2 + (x1 Wr + br)
// with the two BatchNorms n_a, n_f folded into [Wq | Wk | Wv] (+ a bias row) and W1, b1 by the caller.
#pragma once
#include "sgn_plan.h"

#define SGN15_GROUP 128        // inner columns (of q, of k and of v) resident in LDS at a time; also the FFN chunk
#define SGN15_MAX_INNER 1024   // heads * d_head and dim_feedforward: multiples of SGN15_GROUP up to this
#define SGN15_MIN_HEAD 16      // the narrowest head: two of them share one 32-column MFMA block
#define SGN15_SPA_IN SGN_C2    // 128 = [pos + vel | spa]
#define SGN15_SPA_OUT SGN_C3   // 256
#define SGN15_TEM_OUT SGN_C4   // 512

// heads, d_head, ff of one block.  A group of 128 inner columns holds whole heads (d_head 16, 32, 64) or is a K-slice of
// one head (d_head a multiple of 128); other head widths would straddle a group and take the tensor-code composition.
SGN_HD bool sgn15_block_domain(int heads, int d_head, int ff) {
  if (heads < 1 || d_head < SGN15_MIN_HEAD || d_head > SGN15_MAX_INNER || heads > SGN15_MAX_INNER / SGN15_MIN_HEAD) return false;
  const int inner = heads * d_head;
  if (inner % SGN15_GROUP || inner > SGN15_MAX_INNER) return false;
  if (ff < SGN15_GROUP || ff % SGN15_GROUP || ff > SGN15_MAX_INNER) return false;
  return d_head == SGN15_MIN_HEAD || d_head == 32 || d_head == 64 || d_head % SGN15_GROUP == 0;
}
SGN_HD bool sgn15_frames_domain(long N, int seg, int V, int heads, int d_head, int ff) {
  // the batch limit is the base SGN's (about 2M frames: the grid); every offset in the kernels is computed in long
  return sgn_frames_domain(N, seg, V) && sgn15_block_domain(heads, d_head, ff);
}
SGN_HD bool sgn15_clip_domain(long N, int seg, int num_class, int heads, int d_head, int ff) {
  return N >= 1 && N <= 0x7fffffffL / SGN_MAX_CLASS && seg >= 1 && seg <= SGN_VP && num_class >= 1 &&
         num_class <= SGN_MAX_CLASS && sgn15_block_domain(heads, d_head, ff);
}

// ---- the walks ----
SGN_HD int sgn15_groups(int heads, int d_head) { return heads * d_head / SGN15_GROUP; }
SGN_HD int sgn15_group_col(int g) { return g * SGN15_GROUP; }                 // first inner column of group g
SGN_HD bool sgn15_sliced(int d_head) { return d_head >= SGN15_GROUP; }        // a head is one or more whole groups
SGN_HD int sgn15_head_groups(int d_head) { return sgn15_sliced(d_head) ? d_head / SGN15_GROUP : 1; }
SGN_HD int sgn15_group_heads(int d_head) { return sgn15_sliced(d_head) ? 1 : SGN15_GROUP / d_head; }   // 1, 2, 4, 8
SGN_HD int sgn15_group_first_head(int g, int d_head) {
  return sgn15_sliced(d_head) ? g / sgn15_head_groups(d_head) : g * sgn15_group_heads(d_head);
}
SGN_HD int sgn15_chunks(int ff) { return ff / SGN15_GROUP; }
SGN_HD int sgn15_chunk_col(int c) { return c * SGN15_GROUP; }
// element (i, j) of head h of token set b in an attention output (B, heads, rows, rows)
SGN_HD long sgn15_attn_index(long b, int heads, int h, int rows, int i, int j) {
  return ((b * heads + h) * rows + i) * (long)rows + j;
}

// ---- the sections of one block in a weight image (floats).  Every matrix is stored (K, N) row-major. ----
struct Sgn15BlockW {
  long qkv_w, qkv_b;           // (DIN, 3 inner) = [Wq d^-1/2 | Wk | Wv] with n_a folded, (3 inner)
  long o_w, o_b;               // (inner, DIN), (DIN)
  long f1_w, f1_b;             // (DIN, ff) with n_f folded, (ff)
  long f2_w, f2_b;             // ([W2 ; Wr]: (ff + DIN, DOUT)), (DOUT) = b2 + br
  long end;
};
SGN_HD Sgn15BlockW sgn15_block_w(long base, int din, int dout, int heads, int d_head, int ff) {
  Sgn15BlockW w;
  const long inner = (long)heads * d_head;
  long o = base;
  w.qkv_w = o; o += din * 3 * inner;
  w.qkv_b = o; o += 3 * inner;
  w.o_w = o;   o += inner * din;
  w.o_b = o;   o += din;
  w.f1_w = o;  o += (long)din * ff;
  w.f1_b = o;  o += ff;
  w.f2_w = o;  o += ((long)ff + din) * dout;
  w.f2_b = o;  o += dout;
  w.end = o;
  return w;
}
// frames image: the base image's input sections (SgnFramesW up to spa1: aff, the two embeddings, spa1), then the block
SGN_HD long sgn15_frames_block_base(int V) { return sgn_frames_w(V).g_w; }
SGN_HD long sgn15_frames_floats(int V, int heads, int d_head, int ff) {
  return sgn15_block_w(sgn15_frames_block_base(V), SGN15_SPA_IN, SGN15_SPA_OUT, heads, d_head, ff).end;
}
// clip image: tem (seg, 256), the block, fc_w (512, num_class), fc_b (num_class)
struct Sgn15ClipW {
  long tem;
  Sgn15BlockW blk;
  long fc_w, fc_b, total;
};
SGN_HD Sgn15ClipW sgn15_clip_w(int seg, int num_class, int heads, int d_head, int ff) {
  Sgn15ClipW w;
  w.tem = 0;
  w.blk = sgn15_block_w((long)seg * SGN15_SPA_OUT, SGN15_SPA_OUT, SGN15_TEM_OUT, heads, d_head, ff);
  w.fc_w = w.blk.end;
  w.fc_b = w.fc_w + (long)SGN15_TEM_OUT * num_class;
  w.total = w.fc_b + num_class;
  return w;
}

// ---- LDS (floats).  Row strides are odd (see sgn_plan.h).
//   X     (32, DIN + 1)        the token rows: x, then x1 in place
//   QKV   (32, 3 * 128 + 1)    [q | k | v] of one group; a . v overwrites q; the FFN's hidden chunk; the embeddings' E
//   P     (8, 32, 33)          the probabilities of the (up to 8) heads of a group; for a sliced head slot 0 holds the
//                              probabilities and slots 1..4 the four waves' K-split partial scores
//   MISC  512                  xin (2, 32, 4) of the frames kernel / the pooled maximum (512) of the clip kernel
// Three things do NOT fit and are walked instead: [q | k | v] of all heads at inner = 1024 (3 * 32 * 1024 floats =
// 384 KB), the FFN hidden tile at ff = 1024 next to it, and the 8 * 4 = 32 score tiles of 16-wide heads at once.
#define SGN15_QKV_STRIDE (3 * SGN15_GROUP + 1)   // 385
#define SGN15_P_STRIDE (SGN_VP + 1)              // 33
#define SGN15_P_SLOT (SGN_VP * SGN15_P_STRIDE)   // 1056
#define SGN15_P_SLOTS 8
#define SGN15_X_STRIDE(DIN) ((DIN) + 1)
#define SGN15_LDS_X 0
#define SGN15_LDS_QKV(DIN) (SGN15_LDS_X + SGN_VP * SGN15_X_STRIDE(DIN))
#define SGN15_LDS_P(DIN) (SGN15_LDS_QKV(DIN) + SGN_VP * SGN15_QKV_STRIDE)
#define SGN15_LDS_MISC(DIN) (SGN15_LDS_P(DIN) + SGN15_P_SLOTS * SGN15_P_SLOT)
#define SGN15_LDS_FLOATS(DIN) (SGN15_LDS_MISC(DIN) + 512)
static_assert(3 * SGN_VP * SGN15_MAX_INNER * 4 > SGN_LDS_LIMIT, "q, k, v of every head would fit: no group walk needed");
static_assert((SGN15_LDS_FLOATS(SGN15_SPA_OUT) + SGN_VP * SGN15_MAX_INNER) * 4 > SGN_LDS_LIMIT,
              "the whole FFN hidden tile at ff = 1024 would fit next to the carve: no chunk walk needed");
static_assert(32 / SGN15_MIN_HEAD == 2, "sgn15_block selects between the products of exactly TWO heads per MFMA block");
static_assert(SGN15_LDS_FLOATS(SGN15_SPA_IN) * 4 <= SGN_LDS_LIMIT, "agcn_sgn15_frames: LDS");
static_assert(SGN15_LDS_FLOATS(SGN15_SPA_OUT) * 4 <= SGN_LDS_LIMIT, "agcn_sgn15_clip: LDS");
static_assert(SGN15_GROUP / SGN15_MIN_HEAD <= SGN15_P_SLOTS && 1 + SGN_WAVES <= SGN15_P_SLOTS, "P slots");
static_assert(2 * SGN_VP * 4 <= 512 && SGN15_TEM_OUT <= 512, "MISC");
static_assert(SGN_C2 + 1 <= SGN15_QKV_STRIDE, "the embeddings' E (32, 128) lives in QKV");
static_assert(SGN15_GROUP == SGN_WAVES * 32, "one 32-column MFMA block of a group per wave");
