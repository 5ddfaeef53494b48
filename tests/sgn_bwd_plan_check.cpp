// Host check of 2s-agcn_amd/csrc/sgn_bwd_plan.h (no HIP): the transposed weight images tile without overlap, no two
// buffers of the joint-level backward's LDS tile that are live in the same step share a column, workspace sizes, the
// guarded neighbour indices of the dif coupling and of the clip kernel's tile halos over every t, and the guarded source
// row of the sampler adjoint's picks.
#include <stdio.h>
#include <initializer_list>

#include "sgn_bwd_plan.h"

static long cases = 0, failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    ++cases;                                                                         \
    if (!(cond)) {                                                                   \
      if (++failures <= 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                                \
  } while (0)

int main() {
  // transposed images: regions in order, each exactly as long as its matrix, the total as the queries report it
  {
    const SgnFramesWT w = sgn_frames_wt();
    CHECK(w.je2 == 0 && w.de2 == w.je2 + 64 * 64 && w.g == w.de2 + 64 * 64 && w.c1 == w.g + 512 * 128);
    CHECK(w.c2 == w.c1 + 128 * 256 && w.c3 == w.c2 + 256 * 256 && w.total == w.c3 + 256 * 512);
    // the same matrices as the forward image holds
    const SgnFramesW f = sgn_frames_w(15);
    CHECK(w.de2 - w.je2 == f.je2_b - f.je2_w && w.c1 - w.g == f.g_b - f.g_w && w.c2 - w.c1 == f.c1_b - f.c1_w);
    CHECK(w.c3 - w.c2 == f.c2_b - f.c2_w && w.total - w.c3 == f.c3_b - f.c3_w);
    const SgnClipWT c = sgn_clip_wt();
    const SgnClipW cf = sgn_clip_w(20, 60);
    CHECK(c.t1 == 0 && c.t2 == 3 * 256 * 256 && c.total == c.t2 + 512 * 256);
    CHECK(c.t2 - c.t1 == cf.t1_b - cf.t1_w && c.total - c.t2 == cf.t2_b - cf.t2_w);
  }
  // the LDS tile: bands in order and inside the row; buffers outside the tile in order and inside the limit
  CHECK(SGN_BWD_P == 0 && SGN_BWD_T == 256 && SGN_BWD_X2 == 512 && SGN_BWD_X1 == 768 && SGN_BWD_X0 == 896);
  CHECK(SGN_BWD_X0 + SGN_C2 <= SGN_BWD_STRIDE && SGN_BWD_STRIDE % 2 == 1 && SGN_BWD_E1_STRIDE % 2 == 1);
  CHECK(SGN_BWD_DX0 + SGN_C2 == SGN_BWD_X1 && SGN_BWD_DG12 + SGN_C3 == SGN_BWD_X0 + SGN_C2);
  CHECK(SGN_BWD_LDS_G == SGN_VP * SGN_BWD_STRIDE && SGN_BWD_LDS_DG == SGN_BWD_LDS_G + SGN_VP * SGN_G_STRIDE);
  CHECK(SGN_BWD_LDS_E1 == SGN_BWD_LDS_DG + SGN_VP * SGN_G_STRIDE);
  CHECK(SGN_BWD_LDS_XIN == SGN_BWD_LDS_E1 + SGN_VP * SGN_BWD_E1_STRIDE);
  CHECK((long)SGN_FRAMES_BWD_LDS_FLOATS * 4 <= SGN_LDS_LIMIT && (long)SGN_CLIP_BWD_LDS_FLOATS * 4 <= SGN_LDS_LIMIT);
  CHECK(SGN_CLIP_BWD_LDS_ARG >= SGN_CLIP_LDS_MAX + SGN_C4);
  // lifetimes: two buffers that are live in the same step never share a column, and every buffer is inside the row
  {
    const int n = (int)(sizeof(SGN_BWD_LIVES) / sizeof(SGN_BWD_LIVES[0]));
    for (int a = 0; a < n; ++a) {
      const SgnBwdLife& A = SGN_BWD_LIVES[a];
      CHECK(A.col >= 0 && A.width > 0 && A.col + A.width <= SGN_BWD_STRIDE - 1 && A.first <= A.last);
      for (int b = a + 1; b < n; ++b) {
        const SgnBwdLife& B = SGN_BWD_LIVES[b];
        const bool time = A.first <= B.last && B.first <= A.last;
        const bool space = A.col < B.col + B.width && B.col < A.col + A.width;
        ++cases;
        if (time && space) {
          ++failures;
          printf("FAILED: %s and %s overlap in columns and in steps\n", A.name, B.name);
        }
      }
    }
  }
  // workspace: dj and dd, V * 3 floats per frame each
  CHECK(sgn_frames_bwd_ws_floats(1, 1, 2) == 12 && sgn_frames_bwd_ws_floats(5, 20, 15) == 2u * 5 * 20 * 45);
  CHECK(sgn_frames_bwd_ws_floats(1L << 20, 64, 32) == (size_t)2 * (1L << 20) * 64 * 96);
  // the dif coupling and the tile halos over all t
  const int segs[] = {1, 2, 32, 33, 40, 64};
  for (int seg : segs) {
    for (int V = 2; V <= SGN_MAX_V; ++V) {
      const int F = V * 3;
      for (long n = 0; n < 3; ++n) {
        long terms = 0;
        for (int t = 0; t < seg; ++t) {
          const long f = n * seg + t;
          const long prev = sgn_dif_prev(f, seg), own = sgn_dif_own(f, seg), next = sgn_dif_next(f, seg);
          // every index a kernel forms from them stays inside this clip's rows of x / dd
          for (long idx : {prev, own, next})
            if (idx >= 0) CHECK(idx >= n * seg && idx < (n + 1) * seg && (idx + 1) * F <= 3L * seg * F);
          CHECK((prev >= 0) == (t > 0) && (prev < 0 || prev == f - 1));
          CHECK((own >= 0) == (t > 0) && (own < 0 || own == f));
          CHECK((next >= 0) == (t + 1 < seg) && (next < 0 || next == f + 1));
          // adjointness: dd[u] reaches x[u] (+) and x[u - 1] (-) exactly when the forward's dif[u] read them
          terms += (own >= 0) + (next >= 0);
        }
        CHECK(terms == 2L * (seg - 1));
      }
    }
    // tiles: the rows of all tiles partition [0, seg); halos are the neighbours' edge frames or absent
    const int tiles = sgn_clip_tiles(seg);
    int covered = 0;
    for (int k = 0; k < tiles; ++k) {
      const int rows = sgn_tile_rows(k, seg), lo = sgn_halo_lo(k, seg), hi = sgn_halo_hi(k, seg);
      CHECK(rows >= 1 && rows <= SGN_VP && k * SGN_VP + rows <= seg);
      covered += rows;
      CHECK((lo >= 0) == (k > 0) && (lo < 0 || (lo == k * SGN_VP - 1 && lo < seg)));
      CHECK((hi >= 0) == (k + 1 < tiles) && (hi < 0 || (hi == (k + 1) * SGN_VP && hi < seg)));
      if (hi >= 0) CHECK(rows == SGN_VP);            // the halo product reads the tile's last row: it must be a real frame
      // the 34 rows of H: the tile's frames with one on either side, -1 exactly where that leaves the clip
      for (int row = 0; row < SGN_VP + 2; ++row) {
        const int t = sgn_tile_frame(k, row, seg), want = k * SGN_VP - 1 + row;
        CHECK(t == (want >= 0 && want < seg ? want : -1));
      }
      CHECK(sgn_tile_frame(k, 0, seg) == lo && (hi < 0 || sgn_tile_frame(k, SGN_VP + 1, seg) == hi));
      // the padded d Y1 rows the main product reads: r + 2 - dt for r < 32, dt < 3 stays inside the 34 rows
      for (int r = 0; r < SGN_VP; ++r)
        for (int dt = 0; dt < 3; ++dt) CHECK(r + 2 - dt >= 0 && r + 2 - dt < SGN_VP + 2);
    }
    CHECK(covered == seg);
    CHECK(sgn_tile_rows(tiles, seg) == 0 && sgn_halo_lo(tiles + 1, seg) == -1);
  }
  // the sampler's adjoint: a pick's source is a kept row or -1, never a row of the padding or outside the table
  for (int seg : {1, 20, 30, 64})
    for (int kept = 0; kept <= 3 * seg + 7; ++kept) {
      const int L = kept > 0 ? sgn_sample_rows(kept, seg) : 0;
      for (int k = 0; k < seg; ++k)
        for (unsigned r : {0u, 1u, 7u, 12345u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu}) {
          const int src = sgn_pick_source(k, L, seg, r, kept);
          CHECK(src >= -1 && src < kept && src < SGN_SAMPLE_MAX_ROWS);
          if (kept == 0) CHECK(src == -1);
          if (kept > 0) CHECK(src == (sgn_pick(k, L, seg, r) < kept ? sgn_pick(k, L, seg, r) : -1));
          if (kept > 0 && kept < seg) CHECK(src == (k < kept ? k : -1));      // padded to seg rows: interval k = row k
          if (kept >= seg) CHECK(src >= 0);                                  // nothing padded: every pick has a source
        }
    }
  for (int kept : {SGN_SAMPLE_MAX_ROWS - 1, SGN_SAMPLE_MAX_ROWS})
    for (int k = 0; k < 20; ++k) {
      const int src = sgn_pick_source(k, kept, 20, 0xFFFFFFFFu, kept);
      CHECK(src >= 0 && src < kept);
    }
  printf("%ld cases, %ld failures\n", cases, failures);
  return failures ? 1 : 0;
}
