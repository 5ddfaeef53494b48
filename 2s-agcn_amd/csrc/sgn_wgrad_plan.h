// Geometry of the SGN parameter-gradient kernels (sgn_wgrad.hip): the tapes the taping backward kernels write, the row
// splits of the deterministic reduction and its workspace.  Plain C++17 without HIP, like sgn_bwd_plan.h which it builds
// on: sgn_wgrad.hip includes it for launchers and kernels, tests/sgn_wgrad_plan_check.cpp compiles it with the host compiler.
//
// What is taped and what is recomputed.  The taping instantiations of sgn_frames_bwd_kernel / sgn_clip_bwd_kernel recompute
// the forward exactly as the untaped ones do and copy every operand pair of a weight gradient from LDS to the tape at the
// step it is live (SGN_BWD_LIVES): nothing is computed twice for the reduction, and the reduction reads plain row-major
// matrices.  The tape holds the V real joint rows of a frame, never the padded ones, so no reduction needs a row mask.
#pragma once
#include "sgn_bwd_plan.h"

// ---- the frames tape: one row of `cols` floats per (frame f, joint v < V), row index f * V + v.  Column offsets of the
// sections; operands that one product reads side by side are adjacent ([g.x_l | x_l]).  Every section that feeds the
// matrix cores starts at a multiple of 32 floats and cols is one, so a lane group's 32 consecutive floats stay aligned. ----
struct SgnFramesTape {
  int gx3, x2;                 // [g.x2 | x2] (512): X of c3_w
  int dz3;                     // (256): Z of c3_w, column sums = c3_b
  int gx2, x1;                 // [g.x1 | x1] (256): X of c2_w
  int dz2;                     // (256)
  int gx1, x0;                 // [g.x0 | x0] (256): X of c1_w; x0 (128) alone is X of g_w
  int dz1;                     // (128)
  int dg;                      // [d g1 | d g2] (512): Z of g_w, column sums = g_b
  int e1;                      // first embedding layers' activations [joint | dif] (128): X of je2_w / de2_w
  int de2;                     // d(second layers' pre-activations) [joint | dif] (128): Z of je2_w / de2_w, sums = je2_b / de2_b
  int de1;                     // d(first layers' pre-activations) [joint | dif] (128): Z of je1_w / de1_w, sums = je1_b / de1_b
  int dspa;                    // columns 64..127 of d x0 (64): summed over the frames = d spa1
  int xn;                      // the normalised input (2, 4): joint c0..c2, 0, dif c0..c2, 0: X of je1_w / de1_w
  int dxn;                     // d xn before the folded scale (2, 3): joint, dif
  int cols;
};
SGN_HD SgnFramesTape sgn_frames_tape() {
  SgnFramesTape t;
  int o = 0;
  t.gx3 = o;  o += SGN_C3;
  t.x2 = o;   o += SGN_C3;
  t.dz3 = o;  o += SGN_C3;
  t.gx2 = o;  o += SGN_C2;
  t.x1 = o;   o += SGN_C2;
  t.dz2 = o;  o += SGN_C3;
  t.gx1 = o;  o += SGN_C2;
  t.x0 = o;   o += SGN_C2;
  t.dz1 = o;  o += SGN_C2;
  t.dg = o;   o += 2 * SGN_C3;
  t.e1 = o;   o += SGN_C2;
  t.de2 = o;  o += SGN_C2;
  t.de1 = o;  o += SGN_C2;
  t.dspa = o; o += SGN_C1;
  t.xn = o;   o += 8;
  t.dxn = o;  o += 6;
  t.cols = (o + 31) & ~31;
  return t;
}
SGN_HD size_t sgn_frames_tape_row(long f, int v, int V) { return (size_t)f * (size_t)V + (size_t)v; }
SGN_HD size_t sgn_frames_tape_floats(long N, int seg, int V) {
  return (size_t)N * (size_t)seg * (size_t)V * (size_t)sgn_frames_tape().cols;
}

// ---- the clip tape: five row-major matrices one after the other (float offsets).  H keeps the conv's zero padding as
// two zero rows per clip, so the 3-tap weight gradient reads row clip * (seg + 2) + u + dt for tap dt of frame u. ----
struct SgnClipTape {
  size_t h;                    // (N * (seg + 2), 256): H = feat + tem1, frame t of a clip at row t + 1, rows 0 and seg + 1 zero
  size_t y1;                   // (N * seg, 256): relu(conv1)
  size_t dy1;                  // (N * seg, 256): d(conv1's pre-activation)
  size_t dy2;                  // (N * seg, 512): d(conv2's pre-activation), dense: column k is d ymax[k] at its arg-max frame
  size_t ymax;                 // (N, 512): the maximum over the frames = fc's input
  size_t total;
};
SGN_HD SgnClipTape sgn_clip_tape(long N, int seg) {
  SgnClipTape t;
  size_t o = 0;
  const size_t n = (size_t)N, s = (size_t)seg;
  t.h = o;    o += n * (s + 2) * SGN_C3;
  t.y1 = o;   o += n * s * SGN_C3;
  t.dy1 = o;  o += n * s * SGN_C3;
  t.dy2 = o;  o += n * s * SGN_C4;
  t.ymax = o; o += n * SGN_C4;
  t.total = o;
  return t;
}
// row of frame t (-1 and seg: the zero padding) of a clip in the H section
SGN_HD size_t sgn_clip_tape_h_row(long clip, int t, int seg) { return (size_t)clip * (size_t)(seg + 2) + (size_t)(t + 1); }

SGN_HD bool sgn_wgrad_domain(long N, int seg, int V, int num_class) {
  return sgn_frames_domain(N, seg, V) && sgn_clip_domain(N, seg, num_class);
}

// ---- the reduction dW (K, N) = sum over rows r < R of X[xrow(r), k] * Z[zrow(r), n].  One wave owns 32 rows of dW by a
// strip of up to four 32-column tiles (below) and walks its rows two at a time (v_mfma_f32_32x32x2_f32 consumes two): lanes 0..31 read row r, lanes 32..63 row r + 1,
// each 32 consecutive floats of X and of Z straight from the tape (an operand of X^T . Z is read along its rows, so no
// transposed copy and no LDS staging is needed; the tape of a chunk is re-read from L2 by the tiles that share it).  The
// rows are cut into splits of `rows` rows; split s covers [s * rows, min(R, (s + 1) * rows)) and writes a (K, N) partial
// to the workspace; a second kernel adds the partials in ascending split order.  No atomics.
// rows_per_split = 0 is the default: at least SGN_WGRAD_MIN_ROWS rows (below that a split is launch overhead), and at most
// SGN_WGRAD_MAX_SPLITS splits (32 splits x 32 workgroups of four tiles for the 512 x 256 matrix fill the 256 CUs four
// times, and bound the partials to 32 images). ----
#define SGN_WGRAD_MIN_ROWS 256
#define SGN_WGRAD_MAX_SPLITS 32
#define SGN_WGRAD_TILE 32
SGN_HD long sgn_wgrad_split_rows(long R, int rows_per_split) {
  if (rows_per_split > 0) return rows_per_split;
  long rows = (R + SGN_WGRAD_MAX_SPLITS - 1) / SGN_WGRAD_MAX_SPLITS;
  rows = (rows + 1) & ~1L;
  return rows < SGN_WGRAD_MIN_ROWS ? SGN_WGRAD_MIN_ROWS : rows;
}
SGN_HD long sgn_wgrad_splits(long R, int rows_per_split) {
  const long rows = sgn_wgrad_split_rows(R, rows_per_split);
  return R < 1 ? 1 : (R + rows - 1) / rows;
}
SGN_HD long sgn_wgrad_split_begin(long s, long R, int rows_per_split) { return s * sgn_wgrad_split_rows(R, rows_per_split); }
SGN_HD long sgn_wgrad_split_end(long s, long R, int rows_per_split) {
  const long e = (s + 1) * sgn_wgrad_split_rows(R, rows_per_split);
  return e < R ? e : R;
}
// the splits are blockIdx.x of the reduction's grid
SGN_HD bool sgn_wgrad_splits_ok(long R, int rows_per_split) {
  return rows_per_split >= 0 && sgn_wgrad_splits(R, rows_per_split) <= 0x7fffffffL;
}

// Grouped row addressing: reduction row r = group * group_rows + u reads X row group * x_group_stride + u + x_off and Z row
// group * z_group_stride + u.  Plain sections are one group of R rows.  Tap dt of the 3-tap convolution: group = clip,
// group_rows = seg, X = H with x_group_stride = seg + 2 and x_off = dt, Z = dY1 with z_group_stride = seg.
struct SgnWgradRows { long group_rows, x_group_stride, z_group_stride, x_off; };
SGN_HD SgnWgradRows sgn_wgrad_plain_rows(long R) { return SgnWgradRows{R < 1 ? 1 : R, 0, 0, 0}; }
SGN_HD SgnWgradRows sgn_wgrad_tap_rows(int seg, int dt) { return SgnWgradRows{seg, seg + 2, seg, dt}; }
SGN_HD long sgn_wgrad_xrow(long r, const SgnWgradRows& g) { return r / g.group_rows * g.x_group_stride + r % g.group_rows + g.x_off; }
SGN_HD long sgn_wgrad_zrow(long r, const SgnWgradRows& g) { return r / g.group_rows * g.z_group_stride + r % g.group_rows; }

// column tiles of an N that is no multiple of 32 (num_class = 60): the last tile's lanes with n0 + lane >= N read and write
// nothing.  A wave owns a strip of `sgn_wgrad_strip(N)` column tiles next to each other (4 from N = 97 on, else 2 or 1): one
// load of X feeds that many matrix instructions, which cuts the re-reads of the X half of the tape by that factor; column
// tiles of a strip that start at or behind N are guarded like a tail.
SGN_HD int sgn_wgrad_col_tiles(int N) { return (N + SGN_WGRAD_TILE - 1) / SGN_WGRAD_TILE; }
SGN_HD int sgn_wgrad_strip(int N) { const int ct = sgn_wgrad_col_tiles(N); return ct >= 4 ? 4 : ct >= 2 ? 2 : 1; }
SGN_HD int sgn_wgrad_strips(int N) { return (sgn_wgrad_col_tiles(N) + sgn_wgrad_strip(N) - 1) / sgn_wgrad_strip(N); }
SGN_HD int sgn_wgrad_tiles(int K, int N) { return K / SGN_WGRAD_TILE * sgn_wgrad_strips(N); }     // wave-owned strips of dW
// column sums: a workgroup owns SGN_WGRAD_SUM_COLS columns of one split, its SGN_WGRAD_SUM_PHASES row phases (rows begin +
// phase, + 8, ...) are added in ascending phase order
#define SGN_WGRAD_SUM_COLS 32
#define SGN_WGRAD_SUM_PHASES (SGN_THREADS / SGN_WGRAD_SUM_COLS)
#define SGN_WGRAD_FIRST_PHASES (SGN_THREADS / SGN_C1)
static_assert(SGN_WGRAD_FIRST_PHASES >= 3, "sgn_wgrad_first_kernel: one thread row per input coordinate adds the phases");

// ---- workspace (floats): the launches of one image run one after the other on the stream and share it, so it is the
// largest partial: elements of the section times the splits of ITS row count ----
SGN_HD size_t sgn_wgrad_part(size_t elems, long R, int rows_per_split) { return elems * (size_t)sgn_wgrad_splits(R, rows_per_split); }
SGN_HD size_t sgn_wgrad_ws_floats(long N, int seg, int V, int num_class, int rows_per_split) {
  const long frames = N * seg, rows = frames * V;
  size_t m = 0, c;
  const size_t per_row[] = {(size_t)2 * SGN_C3 * SGN_C3, (size_t)SGN_C2 * 2 * SGN_C3, (size_t)2 * 3 * SGN_C1};   // c3_w, g_w, je1_w | de1_w
  for (size_t e : per_row) if ((c = sgn_wgrad_part(e, rows, rows_per_split)) > m) m = c;
  const size_t per_frame[] = {(size_t)V * SGN_C1, (size_t)4 * V * 3, (size_t)SGN_C3 * SGN_C4};   // spa1, aff; t2_w (rows = frames)
  for (size_t e : per_frame) if ((c = sgn_wgrad_part(e, frames, rows_per_split)) > m) m = c;
  const size_t per_clip[] = {(size_t)seg * SGN_C3, (size_t)SGN_C4 * (size_t)num_class};          // tem1, fc_w
  for (size_t e : per_clip) if ((c = sgn_wgrad_part(e, N, rows_per_split)) > m) m = c;
  return m;
}
