// Host check of 2s-agcn_amd/csrc/sgn_v15_wgrad_plan.h (no HIP), at the ten geometries of tests/sgn_v15_grad_util.py::CASES:
// the sections of a tape row are disjoint, in order and start at multiples of 32 floats, [relu(hidden) | x1] is adjacent,
// cols equals the closed formula, the row indexing is dense over the real tokens, the tape sizes, and the workspace is the
// maximum of every section's partial by brute force.  Also the widest geometry's sizes the header states.
#include <stdio.h>
#include <algorithm>

#include "sgn_v15_wgrad_plan.h"

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

// the block's sections: in order from `base`, each a multiple of 32 wide and 32-aligned, hid and x1 adjacent
static void block(const Sgn15BlockTape& t, int base, int din, int dout, const Geo& g) {
  const int inner = g.heads * g.d_head;
  const int start[] = {t.x, t.dqkv, t.o, t.dx1, t.hid, t.x1, t.dhid, t.dy, t.end};
  const int width[] = {din, 3 * inner, inner, din, g.ff, din, g.ff, dout};
  CHECK(t.x == base);
  for (int i = 0; i < 8; ++i) {
    CHECK(start[i] % 32 == 0 && width[i] % 32 == 0 && width[i] > 0);
    CHECK(start[i + 1] == start[i] + width[i]);                      // disjoint and without a gap
  }
  CHECK(t.x1 == t.hid + g.ff);                                       // X of f2_w is one (ff + DIN)-wide operand
  CHECK(din % 32 == 0 && inner % 32 == 0 && (g.ff + din) % 32 == 0); // every K of a reduction
}

static size_t brute_ws(size_t m, size_t elems, long R, int rps) { return std::max(m, elems * (size_t)sgn_wgrad_splits(R, rps)); }

int main() {
  for (const Case& c : CASES) {
    CHECK(sgn15_frames_domain(c.N, c.seg, c.V, c.sp.heads, c.sp.d_head, c.sp.ff));
    CHECK(sgn15_clip_domain(c.N, c.seg, c.num_class, c.tp.heads, c.tp.d_head, c.tp.ff));
    // ---- frames tape ----
    const Sgn15FramesTape f = sgn15_frames_tape(c.sp.heads, c.sp.d_head, c.sp.ff);
    block(f.blk, 0, SGN15_SPA_IN, SGN15_SPA_OUT, c.sp);
    CHECK(f.e1 == f.blk.end && f.de2 == f.e1 + 128 && f.de1 == f.de2 + 128 && f.dspa == f.de1 + 128);
    CHECK(f.xn == f.dspa + 64 && f.dxn == f.xn + 8 && f.dxn + 6 <= f.cols && f.cols - (f.dxn + 6) < 32);
    CHECK(f.e1 % 32 == 0 && f.de2 % 32 == 0 && f.de1 % 32 == 0 && f.dspa % 32 == 0 && f.cols % 32 == 0);
    CHECK(f.cols == sgn15_frames_tape_cols(c.sp.heads, c.sp.d_head, c.sp.ff));
    CHECK(f.cols == 4 * c.sp.heads * c.sp.d_head + 2 * c.sp.ff + 1120);
    // rows: dense over (frame, joint < V), the last row ends the tape
    const long frames = (long)c.N * c.seg;
    size_t next = 0;
    for (long fr = 0; fr < frames; ++fr)
      for (int v = 0; v < c.V; ++v) CHECK(sgn15_frames_tape_row(fr, v, c.V) == next++);
    CHECK(sgn15_frames_tape_floats(c.N, c.seg, c.V, c.sp.heads, c.sp.d_head, c.sp.ff) == next * (size_t)f.cols);
    // ---- clip tape ----
    const Sgn15ClipTape t = sgn15_clip_tape(c.N, c.seg, c.tp.heads, c.tp.d_head, c.tp.ff);
    block(t.blk, 0, SGN15_SPA_OUT, SGN15_TEM_OUT, c.tp);
    CHECK(t.dx == t.blk.end && t.dx % 32 == 0 && t.cols == t.dx + 256 && t.cols % 32 == 0);
    CHECK(t.cols == sgn15_clip_tape_cols(c.tp.heads, c.tp.d_head, c.tp.ff));
    CHECK(t.cols == 4 * c.tp.heads * c.tp.d_head + 2 * c.tp.ff + 1536);
    next = 0;
    for (long n = 0; n < c.N; ++n)
      for (int s = 0; s < c.seg; ++s) CHECK(sgn15_clip_tape_row(n, s, c.seg) == next++);
    CHECK(t.ymax == next * (size_t)t.cols && t.ymax % 32 == 0 && t.total == t.ymax + (size_t)c.N * 512);
    // ---- workspace: the maximum over every section of elements x the splits of its rows ----
    for (int rps : {0, 2, 7, 32}) {
      {
        const Geo& g = c.sp;
        const long inner = (long)g.heads * g.d_head, R = frames * c.V;
        size_t m = 0;
        for (size_t e : {(size_t)(128 * 3 * inner), (size_t)(3 * inner), (size_t)(inner * 128), (size_t)128,
                         (size_t)(128 * g.ff), (size_t)g.ff, (size_t)((g.ff + 128) * 256), (size_t)256, (size_t)64 * 64,
                         (size_t)64, (size_t)2 * 3 * 64})
          m = brute_ws(m, e, R, rps);
        m = brute_ws(m, (size_t)c.V * 64, frames, rps);
        m = brute_ws(m, (size_t)4 * c.V * 3, frames, rps);
        CHECK(sgn15_frames_wgrad_ws_floats(c.N, c.seg, c.V, g.heads, g.d_head, g.ff, rps) == m);
      }
      {
        const Geo& g = c.tp;
        const long inner = (long)g.heads * g.d_head, R = frames;
        size_t m = 0;
        for (size_t e : {(size_t)(256 * 3 * inner), (size_t)(3 * inner), (size_t)(inner * 256), (size_t)256,
                         (size_t)(256 * g.ff), (size_t)g.ff, (size_t)((g.ff + 256) * 512), (size_t)512})
          m = brute_ws(m, e, R, rps);
        m = brute_ws(m, (size_t)c.seg * 256, c.N, rps);
        m = brute_ws(m, (size_t)512 * c.num_class, c.N, rps);
        m = brute_ws(m, (size_t)c.num_class, c.N, rps);
        CHECK(sgn15_clip_wgrad_ws_floats(c.N, c.seg, c.num_class, g.heads, g.d_head, g.ff, rps) == m);
      }
    }
  }
  // the sizes the header states: the widest geometry and the deployed one
  CHECK(sgn15_frames_tape(1, 1024, 1024).cols == 7264 && sgn15_clip_tape(1, 1, 1, 1024, 1024).cols == 7680);
  CHECK(sgn15_block_wgrad_part(256, 512, 1, 1024, 1024, 1, 0) == (size_t)256 * 3072 && 256 * 3072 > 1280 * 512);
  CHECK(sgn15_frames_tape(8, 16, 128).cols == 1888 && sgn15_clip_tape(1, 20, 8, 32, 256).cols == 3072);
  // num_class up to the limit: fc_w's partial per split of the clips
  CHECK(sgn15_clip_wgrad_ws_floats(64, 20, 4096, 8, 32, 256, 0) >= (size_t)512 * 4096);
  CHECK(sgn15_clip_wgrad_ws_floats(64, 1, 4096, 8, 32, 128, 2) == (size_t)512 * 4096 * 32);       // 64 clips in splits of 2
  printf("%ld cases, %ld failures\n", cases, failures);
  return failures ? 1 : 0;
}
