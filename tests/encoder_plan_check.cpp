// Host check of 2s-agcn_amd/csrc/encoder_plan.h: the geometry and the index arithmetic the encoder kernels use, swept
// over the whole domain with the host compiler (no HIP, no GPU).
//   * attention: every (L, dh) of the domain: LDS <= 160 KiB, the three LDS regions disjoint and inside it, the extreme
//     LDS offset of every loop inside its region, row blocks and key blocks covering [0, L) exactly once, the per-thread
//     tile elements covering (ENC_ROWS x dh) exactly once; for a set of (N, H): the tensor offsets of every loop inside
//     the extents the entry points are given, and (small shapes, by enumeration) hitting every element exactly once;
//   * LayerNorm: the waves' row ranges cover [0, R) exactly once, the partial slab fits its workspace;
//   * tokens: the tile fits its LDS, frame blocks cover [0, T'), every x and tok element is touched exactly once with
//     an offset inside the tensor.
#include <cstdio>
#include <vector>

#include "encoder_plan.h"

static long cases = 0, failures = 0;
#define CHECK(cond, ...)                                                                   \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      if (failures < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
      ++failures;                                                                          \
    }                                                                                      \
  } while (0)

static void check_mha_plan(int L, int dh) {
  ++cases;
  const EncMhaPlan p = enc_mha_plan(L, dh);
  CHECK(enc_mha_lds_bytes(p) <= ENC_LDS_LIMIT, "L %d dh %d lds %ld", L, dh, enc_mha_lds_bytes(p));
  CHECK(p.dhp >= dh && p.dhp % 4 == 0 && p.dhp < dh + 4, "L %d dh %d dhp %d", L, dh, p.dhp);
  // regions: A [a_off, b_off), B [b_off, s_off), S [s_off, lds_floats)
  CHECK(p.a_off == 0 && p.b_off >= p.a_off + ENC_ROWS * p.ap && p.s_off >= p.b_off + ENC_KB * p.bp &&
            p.lds_floats >= p.s_off + ENC_ROWS * p.sp, "L %d dh %d regions", L, dh);
  // extreme offsets of stage_rows (rows < ENC_ROWS / ENC_KB, d < dhp), tile_scores, the softmax rows and tile_apply
  CHECK(enc_lds_a(p, ENC_ROWS - 1, p.dhp - 1) < p.b_off, "L %d dh %d A", L, dh);
  CHECK(enc_lds_b(p, ENC_KB - 1, p.dhp - 1) < p.s_off, "L %d dh %d B", L, dh);
  CHECK(enc_lds_s(p, ENC_ROWS - 1, (p.nkb - 1) * ENC_KB + ENC_KB - 1) < p.lds_floats, "L %d dh %d S scores", L, dh);
  CHECK(enc_lds_s(p, ENC_ROWS - 1, L - 1) < p.lds_floats && p.sp - 4 >= L, "L %d dh %d S rows", L, dh);
  CHECK(enc_lds_s(p, 0, 0) >= p.s_off && enc_lds_b(p, 0, 0) >= p.b_off, "L %d dh %d region starts", L, dh);
  // the transposed fill of backward B writes S[r][i], i < nkb*ENC_KB; tile_apply reads 4 floats at S[r][j], j % 4 == 0,
  // j < nkb*ENC_KB
  CHECK(enc_lds_s(p, ENC_ROWS - 1, p.nkb * ENC_KB - 1) < p.lds_floats, "L %d dh %d S transposed", L, dh);
  CHECK(enc_lds_s(p, ENC_ROWS - 1, p.nkb * ENC_KB - 4) + 3 < p.lds_floats, "L %d dh %d S 16-byte reads", L, dh);
  // 16-byte alignment of every row the kernels read or write with 16-byte accesses
  CHECK(p.ap % 4 == 0 && p.bp % 4 == 0 && p.sp % 4 == 0 && p.a_off % 4 == 0 && p.b_off % 4 == 0 && p.s_off % 4 == 0,
        "L %d dh %d alignment", L, dh);
  CHECK(((p.bp / 4) & 1) == 1 && p.bp >= p.dhp + 4, "dh %d bp %d", dh, p.bp);
  // blocks cover [0, L) exactly once
  CHECK(p.nrb * ENC_ROWS >= L && (p.nrb - 1) * ENC_ROWS < L, "L %d nrb %d", L, p.nrb);
  CHECK(p.nkb * ENC_KB >= L && (p.nkb - 1) * ENC_KB < L, "L %d nkb %d", L, p.nkb);
  long keys = 0;
  for (int kb = 0; kb < p.nkb; ++kb) {
    const int jn = ENC_KB < L - kb * ENC_KB ? ENC_KB : L - kb * ENC_KB;
    CHECK(jn >= 1, "L %d kb %d jn %d", L, kb, jn);
    keys += jn;
  }
  CHECK(keys == L, "L %d keys %ld", L, keys);
  // tile elements: thread t owns column t % dw of rows (t / dw)*rpt + k, k < rpt: each (r < ENC_ROWS, d < dh) once
  CHECK(p.dw >= dh && (p.dw & (p.dw - 1)) == 0 && (p.dw == 1 || p.dw / 2 < dh) && p.dw <= ENC_THREADS, "dh %d dw %d", dh, p.dw);
  CHECK(p.ngroups >= 1 && p.ngroups * p.dw <= ENC_THREADS && p.ngroups * p.rpt == ENC_ROWS && p.rpt <= ENC_NI,
        "dh %d groups %d rpt %d", dh, p.ngroups, p.rpt);
  // the score threads: j = tid % ENC_KB, rows tid / ENC_KB and + ENC_ROWS/2 cover (ENC_ROWS x ENC_KB) once
  CHECK(ENC_THREADS / ENC_KB * 2 == ENC_ROWS && ENC_THREADS % ENC_KB == 0, "score thread map");
}

// all tensor offsets of the attention kernels for one (N, L, H, dh): inside the extents, every element exactly once
static void check_mha_tensors(int N, int L, int H, int dh, bool enumerate) {
  ++cases;
  const long D = (long)H * dh;
  const long qkv_n = (long)N * L * 3 * D, ctx_n = (long)N * L * D, prob_n = (long)N * H * L * L, avg_n = (long)N * L * L;
  CHECK(enc_qkv_index(N - 1, L - 1, 2, H - 1, dh - 1, L, H, dh) == qkv_n - 1, "qkv last %d %d %d %d", N, L, H, dh);
  CHECK(enc_ctx_index(N - 1, L - 1, H - 1, dh - 1, L, H, dh) == ctx_n - 1, "ctx last");
  CHECK(enc_prob_index(N - 1, H - 1, L - 1, L - 1, L, H) == prob_n - 1, "prob last");
  CHECK(enc_avg_index(N - 1, L - 1, L - 1, L) == avg_n - 1, "avg last");
  CHECK(enc_null_index(N - 1, L - 1, L) == (long)N * L - 1, "null last");
  CHECK(enc_mha_bwd_ws_bytes(N, L, H) == prob_n * 4, "ws bytes");
  if (!enumerate) return;
  const EncMhaPlan p = enc_mha_plan(L, dh);
  std::vector<int> qkv(qkv_n, 0), ctx(ctx_n, 0), prob(prob_n, 0);
  // stage_rows + tile_store as the kernels walk them: per (n, h, row block): rows via base + row*ld + d
  for (int n = 0; n < N; ++n)
    for (int h = 0; h < H; ++h) {
      for (int part = 0; part < 3; ++part) {
        const long base = enc_qkv_index(n, 0, part, h, 0, L, H, dh);
        for (int kb = 0; kb < p.nkb; ++kb)
          for (int e = 0; e < ENC_KB * p.dhp; ++e) {
            const int j = e / p.dhp, d = e - j * p.dhp, row = kb * ENC_KB + j;
            CHECK(enc_lds_b(p, j, d) < p.s_off, "stage B");
            if (row < L && d < dh) {
              const long idx = base + (long)row * 3 * D + d;
              CHECK(idx >= 0 && idx < qkv_n, "qkv idx %ld", idx);
              if (idx >= 0 && idx < qkv_n) ++qkv[idx];
            }
          }
      }
      const long cbase = enc_ctx_index(n, 0, h, 0, L, H, dh);
      for (int rb = 0; rb < p.nrb; ++rb) {
        for (int tid = 0; tid < ENC_THREADS; ++tid)
          for (int k = 0; k < p.rpt; ++k) {
            const int d = tid & (p.dw - 1), rg = tid / p.dw;
            if (d >= dh || rg >= p.ngroups) continue;
            const int r = rg * p.rpt + k;
            CHECK(r < ENC_ROWS && enc_lds_s(p, r, L - 1) < p.lds_floats && enc_lds_b(p, ENC_KB - 1, d) < p.s_off, "apply lds");
            if (rb * ENC_ROWS + r < L) {
              const long idx = cbase + (long)(rb * ENC_ROWS + r) * D + d;
              CHECK(idx >= 0 && idx < ctx_n, "ctx idx %ld", idx);
              if (idx >= 0 && idx < ctx_n) ++ctx[idx];
            }
          }
        for (int r = 0; r < ENC_ROWS; ++r)
          for (int j = 0; j < L; ++j)
            if (rb * ENC_ROWS + r < L) {
              const long idx = enc_prob_index(n, h, rb * ENC_ROWS + r, j, L, H);
              CHECK(idx >= 0 && idx < prob_n, "prob idx %ld", idx);
              if (idx >= 0 && idx < prob_n) ++prob[idx];
            }
      }
    }
  for (long i = 0; i < qkv_n; ++i) CHECK(qkv[i] == 1, "qkv[%ld] staged %d times (N %d L %d H %d dh %d)", i, qkv[i], N, L, H, dh);
  for (long i = 0; i < ctx_n; ++i) CHECK(ctx[i] == 1, "ctx[%ld] stored %d times", i, ctx[i]);
  for (long i = 0; i < prob_n; ++i) CHECK(prob[i] == 1, "prob[%ld] stored %d times", i, prob[i]);
}

static void check_mask() {
  ++cases;
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < 5; ++j) {
      CHECK(enc_allowed(i, j, 0, false, true) && enc_allowed(i, j, 0, true, false) && !enc_allowed(i, j, 0, true, true), "null");
      CHECK(enc_allowed(i, j, 1, false, false) == (j <= i), "forward");
      CHECK(enc_allowed(i, j, 2, false, false) == (j >= i), "backward");
      CHECK(!enc_allowed(i, j, 1, true, true), "both");
    }
}

static void check_ln(long R, int D) {
  ++cases;
  CHECK(enc_ln_domain(R, D), "ln domain %ld %d", R, D);
  const EncLnPlan p = enc_ln_plan(R);
  CHECK(p.nblocks >= 1 && p.nslots == p.nblocks * ENC_LN_WAVES && p.nslots <= ENC_LN_MAX_WAVES + ENC_LN_WAVES - 1 &&
            p.rows_per_wave >= 1, "R %ld blocks %d", R, p.nblocks);
  // the waves that own rows cover [0, R) exactly once; the slab has a slot for every wave of the grid
  CHECK((long)p.nslots * p.rows_per_wave >= R && (long)(p.nslots - ENC_LN_WAVES) * p.rows_per_wave < R, "R %ld cover", R);
  CHECK(enc_ln_bwd_ws_bytes(R, D) == (long)p.nslots * 2 * D * 4, "R %ld ws", R);
  CHECK(enc_ln_bwd_ws_bytes(R, D) <= (long)((R < 1024 ? R : 1024) + 3) * 2 * D * 4, "R %ld ws bound", R);
  CHECK(ENC_LN_PER_LANE * 64 >= D, "D %d per lane", D);
  CHECK(ENC_LN_PER_THREAD * ENC_THREADS >= D, "D %d per thread", D);
  CHECK((R - 1) * D + D - 1 < 0x7fffffffL, "R %ld D %d int rows", R, D);
}

static void check_tokens(int N, int M, int C, int Tp, int V, int has_cls, bool enumerate) {
  ++cases;
  CHECK(enc_tok_domain(N, M, C, Tp, V, has_cls), "tok domain");
  const EncTokPlan p = enc_tok_plan(C, Tp, V);
  const int D = V * C, L = M * Tp + has_cls;
  CHECK(p.lds_floats <= ENC_TOK_LDS, "C %d T' %d V %d lds %d", C, Tp, V, p.lds_floats);
  CHECK(p.tt >= 1 && p.tt <= Tp && p.ntb * p.tt >= Tp && (p.ntb - 1) * p.tt < Tp, "C %d T' %d V %d frames", C, Tp, V);
  CHECK(p.w >= p.tt * V && (C - 1) * p.w + p.tt * V - 1 < p.lds_floats, "C %d T' %d V %d tile", C, Tp, V);
  CHECK(enc_x_index(N * M - 1, C - 1, Tp - 1, V - 1, C, Tp, V) == (long)N * M * C * Tp * V - 1, "x last");
  CHECK(enc_tok_index(N - 1, L - 1, D - 1, L, D) == (long)N * L * D - 1, "tok last");
  if (!enumerate) return;
  const long xn = (long)N * M * C * Tp * V, tn = (long)N * L * D;
  std::vector<int> xs(xn, 0), ts(tn, 0);
  for (int nm = 0; nm < N * M; ++nm)
    for (int tb = 0; tb < p.ntb; ++tb) {
      const int n = nm / M, m = nm - n * M;
      const int t0 = tb * p.tt, nt = p.tt < Tp - t0 ? p.tt : Tp - t0, run = nt * V;
      for (int e = 0; e < C * run; ++e) {
        const int c = e / run, q = e - c * run;
        const long idx = enc_x_index(nm, c, t0, 0, C, Tp, V) + q;
        CHECK(c * p.w + q < p.lds_floats && idx >= 0 && idx < xn, "x idx");
        if (idx >= 0 && idx < xn) ++xs[idx];
      }
      for (int e = 0; e < nt * D; ++e) {
        const int tt = e / D, f = e - tt * D, v = f / C, c = f - v * C;
        const int l = has_cls + m * Tp + t0 + tt;
        const long idx = enc_tok_index(n, l, f, L, D);
        CHECK(c * p.w + tt * V + v < p.lds_floats && l < L && idx >= 0 && idx < tn, "tok idx");
        if (idx >= 0 && idx < tn) ++ts[idx];
      }
      if (has_cls && m == 0 && tb == 0)
        for (int f = 0; f < D; ++f) ++ts[enc_tok_index(n, 0, f, L, D)];
    }
  for (long i = 0; i < xn; ++i) CHECK(xs[i] == 1, "x[%ld] read %d times", i, xs[i]);
  for (long i = 0; i < tn; ++i) CHECK(ts[i] == 1, "tok[%ld] written %d times", i, ts[i]);
}

int main() {
  for (int L = 1; L <= ENC_MAX_L; ++L)
    for (int dh = 1; dh <= ENC_MAX_DH; ++dh) check_mha_plan(L, dh);
  CHECK(!enc_mha_domain(1, 0, 1, 1) && !enc_mha_domain(1, ENC_MAX_L + 1, 1, 1) && !enc_mha_domain(1, 1, 1, ENC_MAX_DH + 1) &&
            !enc_mha_domain(1, 1, 9, 256) && !enc_mha_domain(0, 1, 1, 1) && enc_mha_domain(1, 640, 8, 256), "domain edges");
  // tensor extents for every L and a spread of widths; enumeration at the shapes the GPU tests run and around the tiles
  const int dhs[] = {1, 2, 3, 4, 5, 8, 16, 25, 50, 63, 64, 65, 144, 200, 255, 256};
  for (int L = 1; L <= ENC_MAX_L; ++L)
    for (int dh : dhs)
      for (int H : {1, 2, 3, 8})
        for (int N : {1, 3}) check_mha_tensors(N, L, H, dh, false);
  const int shapes[][4] = {{1, 2, 1, 1},   {2, 21, 2, 200}, {2, 21, 16, 25}, {2, 6, 2, 144},  {1, 64, 2, 16}, {1, 65, 2, 16},
                           {1, 201, 2, 200}, {1, 601, 1, 8},  {1, 640, 1, 256}, {2, 1, 1, 1},    {1, 15, 3, 5},  {1, 16, 1, 17},
                           {1, 17, 2, 3},  {2, 31, 1, 1},   {1, 32, 1, 2},   {1, 33, 2, 7},   {3, 47, 2, 33}, {1, 129, 1, 31}};
  for (auto& s : shapes) check_mha_tensors(s[0], s[1], s[2], s[3], true);
  check_mask();
  for (long R = 1; R <= 6000; ++R) check_ln(R, R % 2048 + 1);
  for (long R : {12864L, 65536L, 100000L, 1048575L}) check_ln(R, 2048);
  CHECK(!enc_ln_domain(0, 1) && !enc_ln_domain(1, 0) && !enc_ln_domain(1, ENC_MAX_D + 1), "ln domain edges");
  // tokens: every (C, V) with V*C <= 2048 on a coarse grid, every T' with M*T' + cls <= 640 on a coarse grid
  for (int V = 1; V <= 32; ++V)
    for (int C = 1; C * V <= ENC_MAX_D; C += (C < 32 ? 1 : 37))
      for (int M = 1; M <= 3; ++M)
        for (int Tp = 1; M * Tp + 1 <= ENC_MAX_L; Tp += (Tp < 12 ? 1 : 41))
          for (int cls = 0; cls < 2; ++cls) check_tokens(2, M, C, Tp, V, cls, false);
  const int toks[][5] = {{2, 2, 16, 10, 25}, {2, 2, 16, 3, 18}, {1, 1, 1, 1, 1}, {2, 2, 16, 100, 25}, {1, 3, 7, 11, 5},
                         {1, 1, 2048, 3, 1}, {1, 2, 64, 9, 32}, {2, 1, 1, 13, 3}};
  for (auto& t : toks)
    for (int cls = 0; cls < 2; ++cls) check_tokens(t[0], t[1], t[2], t[3], t[4], cls, true);
  CHECK(!enc_tok_domain(1, 2, 16, 320, 25, 1) && enc_tok_domain(1, 2, 16, 320, 25, 0) && !enc_tok_domain(1, 1, 2049, 1, 1, 0),
        "tok domain edges");
  printf("%ld cases, %ld failures\n", cases, failures);
  return failures ? 1 : 0;
}
