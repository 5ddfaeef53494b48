// Host check of 2s-agcn_amd/csrc/sgn_plan.h (no HIP): the sampler's interval plan over its whole domain, the padding
// rule, the clamps of sgn_pick, and the layouts of the weight images and the LDS carves.  With a file name as its
// argument it also writes the boundaries b_0..b_seg of every (seg, L) it swept, as int32, for the comparison with
// numpy in tests/test_sgn_cpu.py.
#include <stdio.h>
#include <vector>

#include "sgn_plan.h"

static long cases = 0, failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    ++cases;                                                                         \
    if (!(cond)) {                                                                   \
      if (++failures <= 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                                \
  } while (0)

int main(int argc, char** argv) {
  const int segs[] = {20, 30, 64, 100};
  std::vector<int> table;
  for (int seg : segs) {
    for (int L = seg; L <= SGN_SAMPLE_MAX_ROWS; ++L) {
      CHECK(sgn_interval(0, L, seg) == 0);
      CHECK(sgn_interval(seg, L, seg) == L);
      for (int k = 0; k <= seg; ++k) table.push_back(sgn_interval(k, L, seg));
      for (int k = 0; k < seg; ++k) {
        const int lo = sgn_interval(k, L, seg), hi = sgn_interval(k + 1, L, seg);
        CHECK(hi > lo);
        CHECK(sgn_pick(k, L, seg, 0u) == lo);
        CHECK(sgn_pick(k, L, seg, 0xFFFFFFFFu) >= lo && sgn_pick(k, L, seg, 0xFFFFFFFFu) < hi);
        CHECK(sgn_pick(k, L, seg, (unsigned)(hi - lo)) == lo);
      }
    }
    // fewer kept rows than intervals: the sequence is padded to seg rows, every interval is one row wide
    for (int kept = 1; kept < seg; ++kept) {
      CHECK(sgn_sample_rows(kept, seg) == seg);
      for (int k = 0; k < seg; ++k) CHECK(sgn_pick(k, sgn_sample_rows(kept, seg), seg, 12345u * k) == k);
    }
    CHECK(sgn_sample_rows(seg, seg) == seg && sgn_sample_rows(seg + 1, seg) == seg + 1);
  }
  // any plan stays in range, also outside the swept domain (L < seg never reaches the kernel's gather unpadded)
  for (int seg = 1; seg <= 130; ++seg)
    for (int L = 1; L <= 300; ++L)
      for (int k = 0; k < seg; ++k)
        for (unsigned r : {0u, 1u, 7u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu}) {
          const int idx = sgn_pick(k, L, seg, r);
          CHECK(idx >= 0 && idx < L);
        }
  // domains
  CHECK(sgn_sample_domain(1, 300, 15, 2, 5, 20) && sgn_sample_domain(64, SGN_SAMPLE_MAX_T, 32, 2, 5, 20));
  CHECK(!sgn_sample_domain(1, 300, 15, 1, 5, 20) && !sgn_sample_domain(1, 300, 15, 3, 5, 20));
  CHECK(!sgn_sample_domain(1, SGN_SAMPLE_MAX_T + 1, 15, 2, 5, 20) && !sgn_sample_domain(1, 300, 33, 2, 5, 20));
  CHECK(!sgn_sample_domain(0, 300, 15, 2, 5, 20) && !sgn_sample_domain(1, 300, 15, 2, 0, 20));
  CHECK(SGN_SAMPLE_CHUNK * SGN_THREADS == SGN_SAMPLE_MAX_ROWS && SGN_SAMPLE_MAX_ROWS <= 65536);
  CHECK(sgn_frames_domain(5, 20, 15) && !sgn_frames_domain(5, 20, 33) && !sgn_frames_domain(5, 20, 1));
  CHECK(!sgn_frames_domain(1L << 30, 20, 15));
  // weight images: regions in order, nothing overlapping, totals as documented
  for (int V = 2; V <= SGN_MAX_V; ++V) {
    const SgnFramesW w = sgn_frames_w(V);
    const int offs[] = {w.aff,  w.je1_w, w.je1_b, w.je2_w, w.je2_b, w.de1_w, w.de1_b, w.de2_w, w.de2_b, w.spa1, w.g_w,
                        w.g_b,  w.c1_w,  w.c1_b,  w.c2_w,  w.c2_b,  w.c3_w,  w.c3_b,  w.total};
    for (size_t i = 1; i < sizeof(offs) / sizeof(offs[0]); ++i) CHECK(offs[i] > offs[i - 1]);
    CHECK(w.total == 12 * V + 2 * (3 * 64 + 64 + 64 * 64 + 64) + 64 * V + 2 * (128 * 256 + 256) + 256 * 128 + 128 +
                         256 * 256 + 256 + 512 * 256 + 256);
  }
  {
    const SgnClipW w = sgn_clip_w(20, 60);
    CHECK(w.tem1 == 0 && w.t1_w == 20 * 256 && w.t1_b == w.t1_w + 3 * 256 * 256 && w.t2_w == w.t1_b + 256);
    CHECK(w.t2_b == w.t2_w + 256 * 512 && w.fc_w == w.t2_b + 512 && w.fc_b == w.fc_w + 512 * 60 && w.total == w.fc_b + 60);
    CHECK(sgn_clip_tiles(1) == 1 && sgn_clip_tiles(32) == 1 && sgn_clip_tiles(33) == 2);
  }
  // LDS carves: regions in order, inside the limit, row strides odd (bank-conflict-free A operands)
  CHECK(SGN_LDS_BUF_B == SGN_VP * SGN_BUF_STRIDE && SGN_LDS_PART == 2 * SGN_VP * SGN_BUF_STRIDE);
  CHECK(SGN_LDS_G == SGN_LDS_PART + SGN_WAVES * SGN_VP * SGN_G_STRIDE && SGN_LDS_XIN == SGN_LDS_G + SGN_VP * SGN_G_STRIDE);
  CHECK((long)SGN_FRAMES_LDS_FLOATS * 4 <= SGN_LDS_LIMIT && (long)SGN_CLIP_LDS_FLOATS * 4 <= SGN_LDS_LIMIT);
  CHECK(SGN_BUF_STRIDE % 2 == 1 && SGN_G_STRIDE % 2 == 1 && SGN_CLIP_STRIDE % 2 == 1);
  CHECK(SGN_BUF_STRIDE > 2 * SGN_C3 && SGN_CLIP_STRIDE > SGN_C3);

  if (argc > 1) {
    FILE* f = fopen(argv[1], "wb");
    if (!f || fwrite(table.data(), sizeof(int), table.size(), f) != table.size()) {
      printf("cannot write %s\n", argv[1]);
      return 2;
    }
    fclose(f);
  }
  printf("%ld cases, %ld failures\n", cases, failures);
  return failures ? 1 : 0;
}
