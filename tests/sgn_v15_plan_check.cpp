// Host check of 2s-agcn_amd/csrc/sgn_v15_plan.h (no HIP): the domain, the column-group and chunk walks of the attention
// block, the layouts of the two weight images and the LDS carves, at every corner of the domain.
#include <stdio.h>
#include <vector>

#include "sgn_v15_plan.h"

static long cases = 0, failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    ++cases;                                                                         \
    if (!(cond)) {                                                                   \
      if (++failures <= 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                                \
  } while (0)

// the order in which sgn15_block visits the inner columns [q | k | v share them]: whole-head groups ascending, or per
// head its slices ascending; every column exactly once, ascending
static void check_walk(int heads, int d_head) {
  const int inner = heads * d_head;
  std::vector<int> seen(inner, 0);
  int last = -1;
  auto visit = [&](int g, int head_lo, int head_hi) {
    CHECK(g >= 0 && g < sgn15_groups(heads, d_head));
    for (int c = sgn15_group_col(g); c < sgn15_group_col(g) + SGN15_GROUP; ++c) {
      CHECK(c < inner && c == last + 1);
      CHECK(c / d_head >= head_lo && c / d_head <= head_hi);       // the column belongs to a head the group claims
      if (c < inner) ++seen[c];
      last = c;
    }
  };
  if (!sgn15_sliced(d_head)) {
    const int hg = sgn15_group_heads(d_head);
    CHECK(hg * d_head == SGN15_GROUP && hg <= SGN15_P_SLOTS);
    for (int g = 0; g < sgn15_groups(heads, d_head); ++g) {
      const int first = sgn15_group_first_head(g, d_head);
      CHECK(first * d_head == sgn15_group_col(g));
      visit(g, first, first + hg - 1);
    }
  } else {
    const int hs = sgn15_head_groups(d_head);
    CHECK(hs * SGN15_GROUP == d_head);
    for (int head = 0; head < heads; ++head)
      for (int sl = 0; sl < hs; ++sl) {
        CHECK(sgn15_group_first_head(head * hs + sl, d_head) == head);
        visit(head * hs + sl, head, head);
      }
  }
  for (int c = 0; c < inner; ++c) CHECK(seen[c] == 1);
}

static void check_block(long base, int din, int dout, int heads, int d_head, int ff) {
  const Sgn15BlockW w = sgn15_block_w(base, din, dout, heads, d_head, ff);
  const long inner = (long)heads * d_head;
  const long sizes[] = {din * 3 * inner, 3 * inner, inner * din, din, (long)din * ff, ff, ((long)ff + din) * dout, dout};
  const long offs[] = {w.qkv_w, w.qkv_b, w.o_w, w.o_b, w.f1_w, w.f1_b, w.f2_w, w.f2_b, w.end};
  CHECK(offs[0] == base);
  for (int i = 0; i < 8; ++i) CHECK(offs[i + 1] == offs[i] + sizes[i]);       // the sections tile the block: no gaps
}

int main() {
  const int d_heads[] = {16, 32, 64, 128, 256, 384, 512, 640, 768, 896, 1024};
  int configs = 0;
  for (int d_head : d_heads)
    for (int heads = 1; heads <= 64; ++heads)
      for (int ff = 128; ff <= 1024; ff += 128) {
        if (!sgn15_block_domain(heads, d_head, ff)) continue;
        ++configs;
        CHECK(heads * d_head % SGN15_GROUP == 0 && heads * d_head <= SGN15_MAX_INNER);
        if (ff == 128) check_walk(heads, d_head);
        // the FFN chunks cover the hidden columns exactly once, ascending
        int last = -1;
        for (int c = 0; c < sgn15_chunks(ff); ++c) {
          CHECK(sgn15_chunk_col(c) == last + 1);
          last = sgn15_chunk_col(c) + SGN15_GROUP - 1;
        }
        CHECK(last == ff - 1);
        for (int V : {2, 15, 32}) {
          check_block(sgn15_frames_block_base(V), SGN15_SPA_IN, SGN15_SPA_OUT, heads, d_head, ff);
          CHECK(sgn15_frames_floats(V, heads, d_head, ff) ==
                12 * V + 2 * (3 * 64 + 64 + 64 * 64 + 64) + 64 * V +
                    sgn15_block_w(0, SGN15_SPA_IN, SGN15_SPA_OUT, heads, d_head, ff).end);
          CHECK(sgn15_frames_domain(5, 20, V, heads, d_head, ff));
        }
        for (int seg : {1, 20, 32}) {
          const Sgn15ClipW w = sgn15_clip_w(seg, 60, heads, d_head, ff);
          CHECK(w.tem == 0 && w.blk.qkv_w == (long)seg * 256 && w.fc_w == w.blk.end && w.fc_b == w.fc_w + 512 * 60 &&
                w.total == w.fc_b + 60);
          check_block((long)seg * 256, SGN15_SPA_OUT, SGN15_TEM_OUT, heads, d_head, ff);
          CHECK(sgn15_clip_domain(5, seg, 60, heads, d_head, ff));
        }
      }
  CHECK(configs > 100);
  // the corners: both the yaml's single wide heads and the deployed narrow ones are inside
  CHECK(sgn15_block_domain(1, 512, 512) && sgn15_block_domain(1, 1024, 1024) && sgn15_block_domain(8, 16, 128) &&
        sgn15_block_domain(8, 32, 256) && sgn15_block_domain(64, 16, 1024) && sgn15_block_domain(2, 64, 128));
  CHECK(!sgn15_block_domain(8, 8, 128) && !sgn15_block_domain(9, 128, 128) && !sgn15_block_domain(1, 1152, 128) &&
        !sgn15_block_domain(8, 16, 64) && !sgn15_block_domain(8, 16, 1152) && !sgn15_block_domain(8, 16, 192) &&
        !sgn15_block_domain(0, 128, 128) && !sgn15_block_domain(8, 48, 128) && !sgn15_block_domain(3, 32, 128));
  CHECK(!sgn15_frames_domain(5, 20, 1, 8, 16, 128) && !sgn15_frames_domain(5, 20, 33, 8, 16, 128) &&
        !sgn15_frames_domain(0, 20, 15, 8, 16, 128) && !sgn15_frames_domain(5, 0, 15, 8, 16, 128));
  // the batch limit is the base SGN's: evaluation batches of thousands of clips are one launch
  CHECK(sgn15_frames_domain(1639, 20, 15, 8, 16, 128) && sgn15_frames_domain(2560, 20, 25, 1, 512, 512) &&
        sgn15_frames_domain(1L << 15, 32, 32, 64, 16, 1024) && sgn15_clip_domain(1L << 15, 32, 60, 8, 32, 256));
  CHECK(sgn15_frames_domain(100000, 20, 15, 8, 16, 128) == sgn_frames_domain(100000, 20, 15));
  CHECK(!sgn15_frames_domain(1L << 30, 20, 15, 8, 16, 128) && !sgn15_clip_domain(1L << 30, 20, 60, 8, 32, 256));
  // the last attention element of the largest launch is addressed in long, far beyond 2^31
  CHECK(sgn15_attn_index((1L << 15) * 32 - 1, 64, 63, 32, 31, 31) == (1L << 15) * 32 * 64 * 32 * 32 - 1);
  CHECK(!sgn15_clip_domain(5, 33, 60, 8, 32, 256) && !sgn15_clip_domain(5, 0, 60, 8, 32, 256) &&
        !sgn15_clip_domain(5, 20, 0, 8, 32, 256) && !sgn15_clip_domain(5, 20, SGN_MAX_CLASS + 1, 8, 32, 256));
  // LDS carves: regions in order, inside the limit at both widths, odd row strides; what is walked would not fit
  for (int din : {SGN15_SPA_IN, SGN15_SPA_OUT}) {
    CHECK(SGN15_LDS_QKV(din) == SGN_VP * (din + 1) && SGN15_LDS_P(din) == SGN15_LDS_QKV(din) + SGN_VP * SGN15_QKV_STRIDE);
    CHECK(SGN15_LDS_MISC(din) == SGN15_LDS_P(din) + SGN15_P_SLOTS * SGN15_P_SLOT);
    CHECK((long)SGN15_LDS_FLOATS(din) * 4 <= SGN_LDS_LIMIT);
    CHECK(SGN15_X_STRIDE(din) % 2 == 1);
  }
  CHECK(SGN15_QKV_STRIDE % 2 == 1 && SGN15_P_STRIDE % 2 == 1 && SGN15_QKV_STRIDE > 3 * SGN15_GROUP);
  CHECK(3L * SGN_VP * SGN15_MAX_INNER * 4 > SGN_LDS_LIMIT);                       // [q | k | v] of all heads at 1024
  CHECK((long)(SGN15_LDS_FLOATS(SGN15_SPA_OUT) + SGN_VP * SGN15_MAX_INNER) * 4 > SGN_LDS_LIMIT);   // + a whole hidden tile
  CHECK(sgn15_attn_index(0, 8, 0, 15, 0, 0) == 0 && sgn15_attn_index(2, 8, 3, 15, 4, 5) == ((2L * 8 + 3) * 15 + 4) * 15 + 5);

  printf("%ld cases, %ld failures\n", cases, failures);
  return failures ? 1 : 0;
}
