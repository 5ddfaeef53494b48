// Host check of 2s-agcn_amd/csrc/sgn_wgrad_plan.h (no HIP): the sections of the two tapes neither overlap nor leave the
// tape, every row split covers [0, R) exactly once (walked two rows at a time, as the reduction kernel walks them, odd
// tails included), guarded column tiles cover [0, N) exactly once, the grouped addressing of the 3-tap convolution stays
// inside a clip's seg + 2 rows, the workspace holds every section's partials, and no size overflows at the domain's edge.
#include <stdio.h>
#include <initializer_list>
#include <vector>

#include "sgn_wgrad_plan.h"

static long cases = 0, failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    ++cases;                                                                         \
    if (!(cond)) {                                                                   \
      if (++failures <= 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                                \
  } while (0)

typedef unsigned __int128 u128;

int main() {
  // ---- the frames tape: sections in order, each as wide as its operand, inside the row; matrix-core sections aligned ----
  {
    const SgnFramesTape t = sgn_frames_tape();
    const int off[] = {t.gx3, t.x2, t.dz3, t.gx2, t.x1, t.dz2, t.gx1, t.x0, t.dz1, t.dg, t.e1, t.de2, t.de1, t.dspa, t.xn, t.dxn};
    const int wid[] = {256, 256, 256, 128, 128, 256, 128, 128, 128, 512, 128, 128, 128, 64, 8, 6};
    int o = 0;
    for (int i = 0; i < 16; ++i) {
      CHECK(off[i] == o && wid[i] > 0);
      if (i < 14) CHECK(off[i] % 32 == 0);
      o += wid[i];
    }
    CHECK(o <= t.cols && t.cols % 32 == 0 && t.cols - o < 32);
    CHECK(t.x2 == t.gx3 + 256 && t.x1 == t.gx2 + 128 && t.x0 == t.gx1 + 128);      // [g.x | x] side by side
  }
  const int classes[] = {1, 31, 32, 60, 4096};
  const int splits_set[] = {0, 1, 2, 3, 7, 32, 33, 255, 1000};
  for (int V = 2; V <= 32; ++V)
    for (int seg = 1; seg <= 64; ++seg)
      for (int N = 1; N <= 8; ++N) {
        CHECK(sgn_wgrad_domain(N, seg, V, 60));
        const SgnFramesTape t = sgn_frames_tape();
        const size_t total = sgn_frames_tape_floats(N, seg, V);
        const long frames = (long)N * seg;
        // rows: (f, v) -> f * V + v, strictly ascending, the last row ends the tape
        CHECK(sgn_frames_tape_row(0, 0, V) == 0 && sgn_frames_tape_row(1, 0, V) == sgn_frames_tape_row(0, V - 1, V) + 1);
        CHECK((sgn_frames_tape_row(frames - 1, V - 1, V) + 1) * (size_t)t.cols == total);
        // the clip tape: sections in order and of their matrices' sizes
        const SgnClipTape c = sgn_clip_tape(N, seg);
        CHECK(c.h == 0 && c.y1 == (size_t)N * (seg + 2) * 256 && c.dy1 == c.y1 + (size_t)frames * 256);
        CHECK(c.dy2 == c.dy1 + (size_t)frames * 256 && c.ymax == c.dy2 + (size_t)frames * 512 && c.total == c.ymax + (size_t)N * 512);
        for (long clip = 0; clip < N; ++clip) {
          CHECK(sgn_clip_tape_h_row(clip, -1, seg) == (size_t)clip * (seg + 2));
          CHECK(sgn_clip_tape_h_row(clip, seg, seg) + 1 == (size_t)(clip + 1) * (seg + 2));
          CHECK((sgn_clip_tape_h_row(clip, seg, seg) + 1) * 256 <= c.y1);
        }
        // the three taps: X rows inside the clip's seg + 2 rows of H, Z rows the clip's own frames; the kernel's
        // incremental (group, u) walk from any start agrees with the division
        for (int dt = 0; dt < 3; ++dt) {
          const SgnWgradRows g = sgn_wgrad_tap_rows(seg, dt);
          long grp = 0, u = 0;
          for (long r = 0; r < frames; ++r) {
            const long clip = r / seg, xr = sgn_wgrad_xrow(r, g), zr = sgn_wgrad_zrow(r, g);
            CHECK(xr >= clip * (seg + 2) && xr < (clip + 1) * (seg + 2) && xr == clip * (seg + 2) + r % seg + dt);
            CHECK(zr == r && zr < frames);
            CHECK(grp * g.x_group_stride + u + g.x_off == xr && grp * g.z_group_stride + u == zr);
            u += 1;
            while (u >= g.group_rows) { u -= g.group_rows; ++grp; }
          }
        }
        {
          const SgnWgradRows g = sgn_wgrad_plain_rows(frames);
          CHECK(sgn_wgrad_xrow(frames - 1, g) == frames - 1 && sgn_wgrad_zrow(frames - 1, g) == frames - 1);
        }
        // the workspace holds the partials of every section as it is launched
        for (int nc : classes)
          for (int rps : splits_set) {
            if ((V + seg + N) % 4 && rps > 3) continue;          // thin the sweep
            const size_t ws = sgn_wgrad_ws_floats(N, seg, V, nc, rps);
            const long rows = frames * V;
            const size_t per_row[] = {512 * 256, 256 * 256, 256 * 128, 128 * 512, 64 * 64, 512, 2 * 3 * 64};
            for (size_t e : per_row) CHECK(ws >= e * (size_t)sgn_wgrad_splits(rows, rps));
            const size_t per_frame[] = {(size_t)V * 64, (size_t)12 * V, 256 * 256, 256 * 512, 512};
            for (size_t e : per_frame) CHECK(ws >= e * (size_t)sgn_wgrad_splits(frames, rps));
            const size_t per_clip[] = {(size_t)seg * 256, (size_t)512 * nc, (size_t)nc};
            for (size_t e : per_clip) CHECK(ws >= e * (size_t)sgn_wgrad_splits(N, rps));
          }
      }
  // ---- the splits: [0, R) exactly once, walked in pairs with the second row of the last pair guarded ----
  {
    std::vector<int> seen;
    for (long R = 1; R <= 1200; R += (R < 140 ? 1 : 53))
      for (int rps : splits_set) {
        CHECK(sgn_wgrad_splits_ok(R, rps));
        const long rows = sgn_wgrad_split_rows(R, rps), splits = sgn_wgrad_splits(R, rps);
        CHECK(rows >= 1 && splits >= 1 && (splits - 1) * rows < R && splits * rows >= R);
        if (rps == 0) CHECK(rows % 2 == 0 && rows >= SGN_WGRAD_MIN_ROWS && splits <= SGN_WGRAD_MAX_SPLITS);
        seen.assign((size_t)R, 0);
        long prev = 0;
        for (long s = 0; s < splits; ++s) {
          const long b = sgn_wgrad_split_begin(s, R, rps), e = sgn_wgrad_split_end(s, R, rps);
          CHECK(b == prev && b < e && e <= R);
          prev = e;
          for (long r0 = b; r0 < e; r0 += 2)
            for (int h = 0; h < 2; ++h)
              if (r0 + h < e) ++seen[(size_t)(r0 + h)];
        }
        CHECK(prev == R);
        bool once = true;
        for (int v : seen) once = once && v == 1;
        CHECK(once);
      }
    CHECK(sgn_wgrad_splits(96000, 0) <= SGN_WGRAD_MAX_SPLITS && sgn_wgrad_split_rows(96000, 0) == 3000);
    CHECK(!sgn_wgrad_splits_ok(10, -1));
  }
  // ---- guarded column tiles: every column of an N that is no multiple of 32 is owned by exactly one (tile, lane) ----
  for (int N = 1; N <= 4096; N += (N < 130 ? 1 : 61)) {
    const int ct = sgn_wgrad_col_tiles(N);
    CHECK(ct * 32 >= N && (ct - 1) * 32 < N);
    const int nb = sgn_wgrad_strip(N), strips = sgn_wgrad_strips(N);
    CHECK((nb == 1 || nb == 2 || nb == 4) && strips * nb >= ct && (strips - 1) * nb < ct);
    long owned = 0, last = -1;
    bool ascending = true;
    for (int strip = 0; strip < strips; ++strip)
      for (int i = 0; i < nb; ++i)
        for (int lane = 0; lane < 32; ++lane) {
          const int n = strip * nb * 32 + i * 32 + lane;         // the kernel's n0 + i * 32 + r
          if (n < N) {
            ++owned;
            ascending = ascending && n == last + 1;
            last = n;
          }
        }
    CHECK(owned == N && ascending);
    for (int K : {64, 128, 256, 512}) CHECK(sgn_wgrad_tiles(K, N) == K / 32 * strips);
  }
  // ---- sizes at the edge of the domain: computed in size_t as in 128 bits ----
  {
    const long clips = 0x7fffffffL / SGN_MAX_CLASS, frames = clips * 4;      // the most clips, of four frames each
    CHECK(frames <= 0x7fffffffL / (SGN_MAX_V * SGN_MAX_V) && frames + 4 > 0x7fffffffL / (SGN_MAX_V * SGN_MAX_V));
    CHECK(sgn_wgrad_domain(clips, 4, 32, 4096) && !sgn_wgrad_domain(clips + 1, 4, 32, 4096) && !sgn_wgrad_domain(clips, 5, 32, 60));
    CHECK(!sgn_wgrad_domain(1, 1, 33, 60) && !sgn_wgrad_domain(1, 1, 1, 60) && !sgn_wgrad_domain(1, 1, 2, 0));
    CHECK(!sgn_wgrad_domain(1, 1, 2, 4097) && !sgn_wgrad_domain(0, 1, 2, 60) && !sgn_wgrad_domain(1, 0, 2, 60));
    const u128 want = (u128)frames * 32 * (u128)sgn_frames_tape().cols;
    CHECK((u128)sgn_frames_tape_floats(frames, 1, 32) == want && want < ((u128)1 << 62));
    const long N = 2047, seg = 1024;                                   // N * seg = the most frames of a long clip
    CHECK(sgn_wgrad_domain(N, (int)seg, 32, 4096));
    CHECK((u128)sgn_clip_tape(N, (int)seg).total == (u128)N * (seg + 2) * 256 + (u128)N * seg * 1024 + (u128)N * 512);
    const u128 ws = (u128)512 * 4096 * (u128)frames;                  // fc_w with one clip per split
    CHECK((u128)sgn_wgrad_ws_floats(frames, 1, 2, 4096, 1) >= ws && ws * 4 < ((u128)1 << 63));
    CHECK((u128)sgn_wgrad_ws_floats(frames, 1, 32, 60, 1) == (u128)512 * 256 * (u128)(frames * 32));
  }
  printf("%ld cases, %ld failures\n", cases, failures);
  return failures ? 1 : 0;
}
