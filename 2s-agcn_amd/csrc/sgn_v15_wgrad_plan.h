// Geometry of the SGN v15 parameter-gradient kernels: the tapes that the taping instantiations of sgn15_frames_bwd_kernel /
// sgn15_clip_bwd_kernel write (sgn_v15_bwd.hip, sgn15_block_bwd in sgn_v15_device.h), and the workspace of the reductions
// of sgn_v15_wgrad.hip, which are the base SGN's (sgn_wgrad_device.h; row splits, strips: sgn_wgrad_plan.h).  Plain C++17
// without HIP, like sgn_v15_bwd_plan.h and sgn_wgrad_plan.h which it builds on: the kernels and launchers include it,
// tests/sgn_v15_wgrad_plan_check.cpp compiles it with the host compiler.
//
// A tape holds one row per REAL token, never a padded one: joint v < V of frame f at row f * V + v (frames tape), frame
// t < seg of clip n at row n * seg + t (clip tape).  As in SgnFramesTape no reduction needs a row mask.  A row holds, for
// the block (inner = heads * d_head), the operand pairs of the image's sections in the layout of Sgn15BlockW:
//   qkv_w (DIN, 3 inner)     X = x, the block's input tokens        Z = [dq | dk | dv], the image's column order
//   o_w   (inner, DIN)       X = o = concat_h(P v)                  Z = dx1
//   f1_w  (DIN, ff)          X = x1                                 Z = d(hidden pre-activation), masked
//   f2_w  (ff + DIN, DOUT)   X = [relu(hidden) | x1], adjacent      Z = dy, dense, one non-zero per column
//   every bias = the column sums of its matrix's Z.
// The frames tape adds what SgnFramesTape holds for the input side (e1, de2, de1, xn, dxn) and columns 64..127 of the
// block's dX (summed over the frames: d spa).  The clip tape adds the block's dX per frame row (summed over the clips,
// per frame: d tem) and, behind the rows, the pooled maxima (N, 512): the X of fc_w, whose Z is the caller's dlogits.
//
// Where it can go wrong:
//   o is transient   In the forward walk o exists per 128-column group only between P v and the product with Wo, inside
//                    sgn15_block_y, which the forward kernels share and which therefore stays untouched.  The taping
//                    backward recomputes P v_g in its own group walk at the one step where P and v of the group are both
//                    live: behind the softmax, before P is overwritten by dS and [q | k | v] by [dq | dk | dv].  It is the
//                    forward's product (same operands, same K order), so the taped o is the forward's o bit for bit.
//   d_head 16        Two heads share a 32-column block.  o, dq, dk and dv of the block are formed with both heads' P / dS
//                    and selected per lane (r >= 16); the tape takes them BEHIND the select, from the accumulators that go
//                    on to finish(): never one head's product for all 32 columns.
//   sliced heads     (d_head = k * 128) [q | k | v] of a slice is recomputed up to three times and do twice (passes 1 - 3).
//                    Only pass 3 tapes, where finish() is called once per slice: o_g and [dq | dk | dv]_g are written
//                    exactly once.  x, x1, hidden, d hidden, dy and dx1 are taped outside the walk, once.
//   the qkv fold     The qkv_w image carries d_head^-1/2 and the BatchNorm scale.  The image gradient is the plain
//                    x^T [dq | dk | dv] with the q, k, v the kernel computed from that image; torch takes it through the
//                    fold.  Nothing is unscaled here.
//   seg = 1, dS = 0  A single row has the 1 x 1 map [1]: dS, dq and dk are exact zeros and are taped as zeros (the q and k
//                    columns of d qkv_w come out zero, as autograd's); dv = do.  Rows of V whose dS is zero are the same.
//                    With R = 1 row the row pair of the reduction has a zero second row (sgn_wgrad_device.h).
//   padded rows      hold bias garbage in x1, hidden and q; the lanes of rows >= R store nothing, and the band copies
//                    stop at R.  A bias summed over the padded rows too would be off by (32 - R) garbage terms.
//   num_class        up to 4096: fc_w's partial is 512 * 4096 floats per split of the CLIPS; the strips of the reduction
//                    guard a num_class that is no multiple of 32.
//   alignment        every section that feeds the matrix cores starts at a multiple of 32 floats and cols is one; every K
//                    (128, 256, inner, ff + DIN) is a multiple of 32.  [relu(hidden) | x1] must stay adjacent.
//
// Size at the widest geometry (inner = ff = 1024): a frames row is 7264 floats (28.4 KiB per joint), a clip row 7680
// (30 KiB per frame); of the clip block f2_w is (1280, 512) = 655 360 floats and qkv_w (256, 3072) = 786 432, the largest
// partial per split.  Deployed (8 x 16, ff 128 / 8 x 32, ff 256; V 15, seg 20): 1888 floats per joint and 3072 per frame,
// 2.5 MB of tape per clip.
#pragma once
#include "sgn_v15_bwd_plan.h"
#include "sgn_wgrad_plan.h"

// ---- the block's sections of a tape row (column offsets) ----
struct Sgn15BlockTape {
  int x;                       // (DIN): X of qkv_w
  int dqkv;                    // (3 inner): Z of qkv_w, column s * inner + c for s = q, k, v; sums = qkv_b
  int o;                       // (inner): X of o_w
  int dx1;                     // (DIN): Z of o_w; sums = o_b
  int hid, x1;                 // [relu(hidden) | x1] (ff + DIN): X of f2_w; x1 alone is X of f1_w
  int dhid;                    // (ff): Z of f1_w; sums = f1_b
  int dy;                      // (DOUT): Z of f2_w; sums = f2_b
  int end;
};
SGN_HD Sgn15BlockTape sgn15_block_tape(int base, int din, int dout, int heads, int d_head, int ff) {
  Sgn15BlockTape t;
  const int inner = heads * d_head;
  int o = base;
  t.x = o;    o += din;
  t.dqkv = o; o += 3 * inner;
  t.o = o;    o += inner;
  t.dx1 = o;  o += din;
  t.hid = o;  o += ff;
  t.x1 = o;   o += din;
  t.dhid = o; o += ff;
  t.dy = o;   o += dout;
  t.end = o;
  return t;
}

// ---- the frames tape: the block, then the input side as in SgnFramesTape ----
struct Sgn15FramesTape {
  Sgn15BlockTape blk;
  int e1;                      // first embedding layers' activations [position | velocity] (128): X of je2_w / de2_w
  int de2;                     // d(second layers' pre-activations) (128): Z of je2_w / de2_w, sums = je2_b / de2_b
  int de1;                     // d(first layers' pre-activations) (128): Z of je1_w / de1_w, sums = je1_b / de1_b
  int dspa;                    // columns 64..127 of the block's dX (64): summed over the frames = d spa
  int xn;                      // the normalised input (2, 4): position c0..c2, 0, velocity c0..c2, 0
  int dxn;                     // d xn before the folded scale (2, 3)
  int cols;
};
SGN_HD Sgn15FramesTape sgn15_frames_tape(int heads, int d_head, int ff) {
  Sgn15FramesTape t;
  t.blk = sgn15_block_tape(0, SGN15_SPA_IN, SGN15_SPA_OUT, heads, d_head, ff);
  int o = t.blk.end;
  t.e1 = o;   o += SGN_C2;
  t.de2 = o;  o += SGN_C2;
  t.de1 = o;  o += SGN_C2;
  t.dspa = o; o += SGN_C1;
  t.xn = o;   o += 8;
  t.dxn = o;  o += 6;
  t.cols = (o + 31) & ~31;
  return t;
}
// closed form of cols: 3 DIN + 4 inner + 2 ff + DOUT + 448 + 14 rounded up = 4 inner + 2 ff + 1120
SGN_HD int sgn15_frames_tape_cols(int heads, int d_head, int ff) { return 4 * heads * d_head + 2 * ff + 1120; }
SGN_HD size_t sgn15_frames_tape_row(long f, int v, int V) { return (size_t)f * (size_t)V + (size_t)v; }
SGN_HD size_t sgn15_frames_tape_floats(long N, int seg, int V, int heads, int d_head, int ff) {
  return (size_t)N * (size_t)seg * (size_t)V * (size_t)sgn15_frames_tape(heads, d_head, ff).cols;
}

// ---- the clip tape: N * seg rows of `cols` floats, then the pooled maxima (N, 512) ----
struct Sgn15ClipTape {
  Sgn15BlockTape blk;
  int dx;                      // the block's dX (256) of the frame row: summed over the clips, per frame = d tem
  int cols;
  size_t ymax;                 // float offset of the (N, 512) maxima = fc's input
  size_t total;
};
SGN_HD Sgn15ClipTape sgn15_clip_tape(long N, int seg, int heads, int d_head, int ff) {
  Sgn15ClipTape t;
  t.blk = sgn15_block_tape(0, SGN15_SPA_OUT, SGN15_TEM_OUT, heads, d_head, ff);
  t.dx = t.blk.end;
  t.cols = t.dx + SGN15_SPA_OUT;
  t.ymax = (size_t)N * (size_t)seg * (size_t)t.cols;
  t.total = t.ymax + (size_t)N * SGN15_TEM_OUT;
  return t;
}
// closed form: 3 DIN + 4 inner + 2 ff + DOUT + 256 = 4 inner + 2 ff + 1536
SGN_HD int sgn15_clip_tape_cols(int heads, int d_head, int ff) { return 4 * heads * d_head + 2 * ff + 1536; }
SGN_HD size_t sgn15_clip_tape_row(long n, int t, int seg) { return (size_t)n * (size_t)seg + (size_t)t; }

// ---- workspace (floats) of one image's reductions, as sgn_wgrad_ws_floats: the launches run one after the other on the
// stream and share it, so it is the largest partial: a section's elements times the splits of ITS row count.  Biases are
// smaller than their matrices at the same row count and need no entry. ----
SGN_HD size_t sgn15_block_wgrad_part(int din, int dout, int heads, int d_head, int ff, long R, int rows_per_split) {
  const size_t inner = (size_t)heads * d_head;
  const size_t secs[] = {(size_t)din * 3 * inner, inner * din, (size_t)din * ff, ((size_t)ff + din) * dout};
  size_t m = 0;
  for (size_t e : secs) if (e > m) m = e;
  return sgn_wgrad_part(m, R, rows_per_split);
}
SGN_HD size_t sgn15_frames_wgrad_ws_floats(long N, int seg, int V, int heads, int d_head, int ff, int rows_per_split) {
  const long frames = N * seg, rows = frames * V;
  size_t m = sgn15_block_wgrad_part(SGN15_SPA_IN, SGN15_SPA_OUT, heads, d_head, ff, rows, rows_per_split), c;
  const size_t per_row[] = {(size_t)SGN_C1 * SGN_C1, (size_t)2 * 3 * SGN_C1};                    // je2_w / de2_w, je1_w | de1_w
  for (size_t e : per_row) if ((c = sgn_wgrad_part(e, rows, rows_per_split)) > m) m = c;
  const size_t per_frame[] = {(size_t)V * SGN_C1, (size_t)4 * V * 3};                           // spa, aff
  for (size_t e : per_frame) if ((c = sgn_wgrad_part(e, frames, rows_per_split)) > m) m = c;
  return m;
}
SGN_HD size_t sgn15_clip_wgrad_ws_floats(long N, int seg, int num_class, int heads, int d_head, int ff, int rows_per_split) {
  size_t m = sgn15_block_wgrad_part(SGN15_SPA_OUT, SGN15_TEM_OUT, heads, d_head, ff, N * seg, rows_per_split), c;
  const size_t per_clip[] = {(size_t)seg * SGN15_SPA_OUT, (size_t)SGN15_TEM_OUT * (size_t)num_class};   // tem, fc_w
  for (size_t e : per_clip) if ((c = sgn_wgrad_part(e, N, rows_per_split)) > m) m = c;
  return m;
}
