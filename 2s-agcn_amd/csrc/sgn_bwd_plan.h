// Geometry and index arithmetic of the SGN input-gradient kernels (sgn_bwd.hip): the transposed weight images, the LDS
// carve of the joint-level backward with the lifetime of every band, the workspace of the dif coupling, and the guarded
// neighbour indices (t - 1, t + 1, tile halos, the picks of the sampler adjoint).  Plain C++17 without HIP, like sgn_plan.h which it builds on:
// sgn_bwd.hip includes it for launchers and kernels, tests/sgn_bwd_plan_check.cpp compiles it with the host compiler.
#pragma once
#include "sgn_plan.h"

// ---- transposed weight image of agcn_sgn_frames_bwd (floats).  The backward products are dZ . W^T; every matrix is
// stored (N, K) row-major = W^T, so that the 32 lanes of an MFMA B operand again read 32 consecutive floats.  The 3 -> 64
// first layers and the bias / affine vectors are read from the forward image. ----
struct SgnFramesWT {
  int je2, de2;                // (64, 64): second layers of the two embeddings
  int g;                       // (512, 128): rows 0..255 g1^T, rows 256..511 g2^T
  int c1, c2, c3;              // gcn l: (Cout, 2 Cin), columns [0, Cin) the g.x part, [Cin, 2 Cin) the x part
  int total;
};
SGN_HD SgnFramesWT sgn_frames_wt() {
  SgnFramesWT w;
  int o = 0;
  w.je2 = o; o += SGN_C1 * SGN_C1;
  w.de2 = o; o += SGN_C1 * SGN_C1;
  w.g = o;   o += 2 * SGN_C3 * SGN_C2;
  w.c1 = o;  o += SGN_C2 * 2 * SGN_C2;
  w.c2 = o;  o += SGN_C3 * 2 * SGN_C2;
  w.c3 = o;  o += SGN_C3 * 2 * SGN_C3;
  w.total = o;
  return w;
}

// ---- transposed weight image of agcn_sgn_clip_bwd: the two convolutions; fc is read from the forward image (row k of
// its (512, num_class) matrix is already the contiguous run d ymax[k] sums over) ----
struct SgnClipWT {
  int t1;                      // (3, 256, 256): tap dt, row = output channel, column = input channel
  int t2;                      // (512, 256)
  int total;
};
SGN_HD SgnClipWT sgn_clip_wt() {
  SgnClipWT w;
  int o = 0;
  w.t1 = o; o += 3 * SGN_C3 * SGN_C3;
  w.t2 = o; o += SGN_C4 * SGN_C3;
  w.total = o;
  return w;
}

// ---- LDS of agcn_sgn_frames_bwd (floats).  One tile of SGN_VP rows x SGN_BWD_STRIDE holds five column bands:
//   P  [0, 256)     forward: g1.  backward: d z3 (layer 3) -> g1 again (adjacency projections) -> the second embedding
//                   layers' activations, masked in place to their gradients
//   T  [256, 512)   forward: g2, then g.x of each layer.  backward: d(g.x) of each layer -> g2 -> d(first embedding layers)
//   X2 [512, 768)   forward: the four K-split partials of g1 . g2^T (before x2 exists), then x2.  backward: d z2 in place
//                   -> [640, 768) the partial d x0 of gcn1
//   X1 [768, 896)   x1 -> d z1 in place -> left half of d g1 / d g2
//   X0 [896, 1024)  x0 (live until g1 | g2 are recomputed) -> right half of d g1 / d g2
// The partials of dG are written to P [0, 132) after layer 1, when d z3 is dead and g1 is not yet recomputed.  The stride
// is odd, as in the forward.  Outside the tile: G, dG (dS after the softmax backward), the first embedding layers'
// activations E1 (their masks, and the operand of the recomputed second layers), and the normalised input. ----
#define SGN_BWD_STRIDE (4 * SGN_C3 + 1)        // 1025
#define SGN_BWD_P 0
#define SGN_BWD_T (SGN_BWD_P + SGN_C3)
#define SGN_BWD_X2 (SGN_BWD_T + SGN_C3)
#define SGN_BWD_X1 (SGN_BWD_X2 + SGN_C3)
#define SGN_BWD_X0 (SGN_BWD_X1 + SGN_C2)
#define SGN_BWD_DX0 (SGN_BWD_X2 + SGN_C2)      // partial d x0 of gcn1: the right half of the X2 band
#define SGN_BWD_DG12 SGN_BWD_X1                // d g1 / d g2, 256 columns over the X1 and X0 bands
#define SGN_BWD_PART_STRIDE SGN_G_STRIDE       // partial p of row i, column j: band + p * 33 + j in row i of the tile
#define SGN_BWD_E1_STRIDE (SGN_C2 + 1)         // 129
#define SGN_BWD_LDS_TILE 0
#define SGN_BWD_LDS_G (SGN_BWD_LDS_TILE + SGN_VP * SGN_BWD_STRIDE)
#define SGN_BWD_LDS_DG (SGN_BWD_LDS_G + SGN_VP * SGN_G_STRIDE)
#define SGN_BWD_LDS_E1 (SGN_BWD_LDS_DG + SGN_VP * SGN_G_STRIDE)
#define SGN_BWD_LDS_XIN (SGN_BWD_LDS_E1 + SGN_VP * SGN_BWD_E1_STRIDE)
#define SGN_FRAMES_BWD_LDS_FLOATS (SGN_BWD_LDS_XIN + 2 * SGN_VP * 4)
static_assert(SGN_BWD_X0 + SGN_C2 == SGN_BWD_STRIDE - 1, "agcn_sgn_frames_bwd: the bands fill the tile row");
static_assert(SGN_WAVES * SGN_BWD_PART_STRIDE <= SGN_C3, "agcn_sgn_frames_bwd: the partials fit a band");
static_assert(SGN_FRAMES_BWD_LDS_FLOATS * 4 <= SGN_LDS_LIMIT, "agcn_sgn_frames_bwd: LDS");

// The lifetimes above as data, for the host check: buffer, first column, width, first and last step it is live in.
// Steps: 0 embeddings, 1 g1|g2, 2 g3 partials + softmax, 3..5 gcn1..3 forward (5 ends with d z3), 6..8 backward of
// gcn3..1, 9 dG partials + softmax backward, 10 g1|g2 again, 11 d g1, 12 d g2, 13 second embedding layers, 14 first.
struct SgnBwdLife { const char* name; int col, width, first, last; };
static const SgnBwdLife SGN_BWD_LIVES[] = {
    {"x0", SGN_BWD_X0, SGN_C2, 0, 10},       {"g1|g2", SGN_BWD_P, 2 * SGN_C3, 1, 2},
    {"g3 partials", SGN_BWD_X2, SGN_WAVES * SGN_BWD_PART_STRIDE, 2, 2},
    {"g.x", SGN_BWD_T, SGN_C3, 3, 5},        {"x1", SGN_BWD_X1, SGN_C2, 3, 8},
    {"x2", SGN_BWD_X2, SGN_C3, 4, 7},        {"dz3", SGN_BWD_P, SGN_C3, 5, 6},
    {"d(g.x)", SGN_BWD_T, SGN_C3, 6, 8},     {"dx0 partial", SGN_BWD_DX0, SGN_C2, 8, 12},
    {"dG partials", SGN_BWD_P, SGN_WAVES * SGN_BWD_PART_STRIDE, 9, 9},
    {"g1|g2 again", SGN_BWD_P, 2 * SGN_C3, 10, 12},
    {"dg1", SGN_BWD_DG12, SGN_C3, 11, 11},   {"dg2", SGN_BWD_DG12, SGN_C3, 12, 12},
    {"d embed 2", SGN_BWD_P, SGN_C2, 13, 14}, {"d embed 1", SGN_BWD_T, SGN_C2, 14, 14},
};
// x0 is read for the last time when g1 | g2 are recomputed (step 10) and d g1 is written from step 11 on; d g1 is consumed
// (into registers) before d g2 overwrites it.

// ---- the dif coupling: frame f = n * seg + t writes dj[f] and dd[f] (V * 3 floats each) to the workspace, a second
// kernel combines dx[t] = dj[t] + dd[t] [t > 0] - dd[t + 1] [t + 1 < seg], with the guarded neighbours sgn_dif_* of
// sgn_plan.h. ----
SGN_HD size_t sgn_frames_bwd_ws_floats(long N, int seg, int V) { return (size_t)2 * (size_t)N * (size_t)seg * (size_t)(V * 3); }

// ---- the sampler's adjoint: the kept row that pick (k, r) of a sequence of L rows reads, as an index into the kept-row
// table (0 <= index < kept <= SGN_SAMPLE_MAX_ROWS), or -1 where the pick falls into the zero padding behind the kept rows
// (or the window is empty): such a pick has no source row and its gradient goes nowhere ----
SGN_HD int sgn_pick_source(int k, int L, int seg, unsigned r, int kept) {
  if (L < 1 || kept < 1) return -1;
  const int idx = sgn_pick(k, L, seg, r);
  return idx < kept ? idx : -1;
}

// ---- the clip kernel's tiles (sgn_plan.h: sgn_tile_rows, sgn_tile_frame).  A tile's conv gradient also reaches frame
// 32 k - 1 (through tap 0 of its first frame) and frame 32 k + 32 (through tap 2 of its last): halo frames, owned by
// the neighbouring tiles.  -1 = the halo is the conv's zero padding (or does not exist) and receives nothing. ----
SGN_HD int sgn_halo_lo(int tile, int seg) { return tile > 0 && tile * SGN_VP - 1 < seg ? tile * SGN_VP - 1 : -1; }
SGN_HD int sgn_halo_hi(int tile, int seg) { return (tile + 1) * SGN_VP < seg ? (tile + 1) * SGN_VP : -1; }
// LDS of agcn_sgn_clip_bwd: the forward's H / Y / maximum, where d Y1 (with a zero row on either side) takes the place
// of H once Y1 exists, plus the arg-max frame of every column
#define SGN_CLIP_BWD_LDS_ARG SGN_CLIP_LDS_FLOATS                       // (512) ints
#define SGN_CLIP_BWD_LDS_FLOATS (SGN_CLIP_BWD_LDS_ARG + SGN_C4)
static_assert(SGN_CLIP_BWD_LDS_FLOATS * 4 <= SGN_LDS_LIMIT, "agcn_sgn_clip_bwd: LDS");
