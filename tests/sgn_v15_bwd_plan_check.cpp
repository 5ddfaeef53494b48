// Host check of 2s-agcn_amd/csrc/sgn_v15_bwd_plan.h (no HIP): the transposed weight images tile without overlap and hold
// the forward image's matrices over the whole domain of block geometries, no two LDS bands of either backward kernel that
// are live in the same step share a float, every band is inside the 160 KB, the dense dy and the dh chunk fit the bands
// they overlay, and the workspace of the dif coupling.
#include <stdio.h>
#include <initializer_list>

#include "sgn_v15_bwd_plan.h"

static long cases = 0, failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    ++cases;                                                                         \
    if (!(cond)) {                                                                   \
      if (++failures <= 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                                \
  } while (0)

static void lives(const char* kernel, const Sgn15BwdLife* L, int n, long total) {
  for (int a = 0; a < n; ++a) {
    const Sgn15BwdLife& A = L[a];
    CHECK(A.first_float >= 0 && A.floats > 0 && A.first_float + A.floats <= total && A.first <= A.last);
    CHECK(((long)A.first_float + A.floats) * 4 <= SGN_LDS_LIMIT);
    for (int b = a + 1; b < n; ++b) {
      const Sgn15BwdLife& B = L[b];
      const bool time = A.first <= B.last && B.first <= A.last;
      const bool space = A.first_float < B.first_float + B.floats && B.first_float < A.first_float + A.floats;
      ++cases;
      if (time && space) {
        ++failures;
        printf("FAILED: %s: %s and %s overlap in floats and in steps\n", kernel, A.name, B.name);
      }
    }
  }
}

static void block(const Sgn15BlockWT& t, const Sgn15BlockW& f, long base, int din, int dout, int heads, int d_head, int ff) {
  const long inner = (long)heads * d_head;
  CHECK(t.qkv == base && t.o == t.qkv + 3 * inner * din && t.f1 == t.o + inner * din && t.f2 == t.f1 + (long)ff * din);
  CHECK(t.end == t.f2 + (long)dout * (ff + din));
  // the same matrices as the forward image holds
  CHECK(t.o - t.qkv == f.qkv_b - f.qkv_w && t.f1 - t.o == f.o_b - f.o_w && t.f2 - t.f1 == f.f1_b - f.f1_w);
  CHECK(t.end - t.f2 == f.f2_b - f.f2_w);
  // the last float every product of the block backward reads from each section (sgn_v15_device.h) is inside it
  const long ldf2 = ff + din;
  CHECK(t.f2 + (long)(dout - 1) * ldf2 + ff + din - 1 < t.end);                       // dy Wr^T
  CHECK(t.f2 + (long)(dout - 1) * ldf2 + ff - 1 < t.end);                             // dy W2_c^T, the last chunk
  CHECK(t.f1 + (long)(ff - 1) * din + din - 1 < t.f2);                                // dh W1_c^T
  CHECK(t.o + (long)(din - 1) * inner + inner - 1 < t.f1);                            // dx1 Wo_g^T, the last group
  CHECK(t.qkv + (3 * inner - 1) * din + din - 1 < t.o);                               // [dq | dk | dv] Wqkv_g^T
}

int main() {
  // every block geometry of the domain, and a few outside it
  long in_domain = 0;
  for (int d_head = 8; d_head <= 1152; d_head += 8)
    for (int heads = 1; heads <= 66; ++heads)
      for (int ff = 128; ff <= 1024; ff += 128) {
        const bool ok = sgn15_block_domain(heads, d_head, ff);
        if (!ok) continue;
        ++in_domain;
        const Sgn15FramesWT fw = sgn15_frames_wt(heads, d_head, ff);
        CHECK(fw.je2 == 0 && fw.de2 == 64 * 64 && fw.blk.qkv == 2 * 64 * 64 && fw.total == fw.blk.end);
        block(fw.blk, sgn15_block_w(sgn15_frames_block_base(15), 128, 256, heads, d_head, ff), 2 * 64 * 64, 128, 256, heads,
              d_head, ff);
        const Sgn15ClipWT cw = sgn15_clip_wt(heads, d_head, ff);
        CHECK(cw.blk.qkv == 0 && cw.total == cw.blk.end);
        block(cw.blk, sgn15_clip_w(20, 60, heads, d_head, ff).blk, 0, 256, 512, heads, d_head, ff);
        // the walks the backward shares with the forward
        const int groups = sgn15_groups(heads, d_head);
        CHECK(groups >= 1 && groups * SGN15_GROUP == heads * d_head);
        if (sgn15_sliced(d_head)) {
          CHECK(sgn15_head_groups(d_head) * heads == groups && SGN15_BWD_DS_SLOT < SGN15_P_SLOTS);
        } else {
          const int hg = sgn15_group_heads(d_head);
          CHECK(hg * d_head == SGN15_GROUP && hg <= SGN15_P_SLOTS && hg <= 2 * SGN_WAVES);
          for (int wave = 0; wave < SGN_WAVES; ++wave) {
            const int lh0 = wave * 32 / d_head;                                     // the head(s) of the wave's block
            CHECK(lh0 < hg && (d_head != SGN15_MIN_HEAD || lh0 + 1 < hg));
            CHECK(d_head == SGN15_MIN_HEAD ? lh0 * d_head == wave * 32 : lh0 * d_head <= wave * 32);
          }
        }
      }
  CHECK(in_domain > 100);
  SgnFramesW fw15 = sgn_frames_w(15);
  CHECK(sgn15_frames_block_base(15) == fw15.g_w);
  // the carve: bands in order, odd strides, dy over QKV + DO, dh in P
  CHECK(SGN15_BWD_DO_STRIDE % 2 == 1 && SGN15_QKV_STRIDE % 2 == 1 && SGN15_P_STRIDE % 2 == 1);
  for (int din : {SGN15_SPA_IN, SGN15_SPA_OUT}) {
    const int dout = 2 * din;
    CHECK(SGN15_X_STRIDE(din) % 2 == 1 && SGN15_BWD_DY_STRIDE(dout) % 2 == 1);
    CHECK(SGN15_BWD_LDS_QKV(din) == SGN_VP * SGN15_X_STRIDE(din));
    CHECK(SGN15_BWD_LDS_DO(din) == SGN15_BWD_LDS_QKV(din) + SGN_VP * SGN15_QKV_STRIDE);
    CHECK(SGN15_BWD_LDS_P(din) == SGN15_BWD_LDS_DO(din) + SGN_VP * SGN15_BWD_DO_STRIDE);
    CHECK(SGN15_BWD_LDS_MISC(din) == SGN15_BWD_LDS_P(din) + SGN15_P_SLOTS * SGN15_P_SLOT);
    CHECK(SGN15_BWD_LDS_QKV(din) + SGN_VP * SGN15_BWD_DY_STRIDE(dout) <= SGN15_BWD_LDS_P(din));
    CHECK(SGN_VP * SGN15_BWD_DO_STRIDE <= SGN15_P_SLOTS * SGN15_P_SLOT);
    CHECK((long)SGN15_BWD_LDS_BLOCK(din) * 4 <= SGN_LDS_LIMIT);
  }
  CHECK(SGN15_BWD_LDS_X0 == SGN15_BWD_LDS_BLOCK(SGN15_SPA_IN) && SGN15_BWD_LDS_E1 > SGN15_BWD_LDS_X0);
  CHECK((long)SGN15_FRAMES_BWD_LDS_FLOATS * 4 <= SGN_LDS_LIMIT && (long)SGN15_CLIP_BWD_LDS_FLOATS * 4 <= SGN_LDS_LIMIT);
  // the issue's count: x and dx1 both resident at DIN = 256 do not fit, which is why dx1 stays in registers
  CHECK(2 * 8224 + 12320 + 4128 + 8448 == 41344 && 41344 * 4 > SGN_LDS_LIMIT);
  lives("frames", SGN15_FRAMES_BWD_LIVES, (int)(sizeof(SGN15_FRAMES_BWD_LIVES) / sizeof(SGN15_FRAMES_BWD_LIVES[0])),
        SGN15_FRAMES_BWD_LDS_FLOATS);
  lives("clip", SGN15_CLIP_BWD_LIVES, (int)(sizeof(SGN15_CLIP_BWD_LIVES) / sizeof(SGN15_CLIP_BWD_LIVES[0])),
        SGN15_CLIP_BWD_LDS_FLOATS);
  // workspace: dj and dd, V * 3 floats per frame each
  CHECK(sgn15_frames_bwd_ws_floats(1, 1, 2) == 12 && sgn15_frames_bwd_ws_floats(5, 20, 15) == 2u * 5 * 20 * 45);
  CHECK(sgn15_frames_bwd_ws_floats(1L << 15, 32, 32) == (size_t)2 * (1L << 15) * 32 * 96);
  printf("%ld cases, %ld failures\n", cases, failures);
  return failures ? 1 : 0;
}
