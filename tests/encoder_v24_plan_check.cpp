// Host check of the aagcn_v24 part of 2s-agcn_amd/csrc/encoder_plan.h: the index functions of the attention bias, of the
// two-stage sums over sequences and of the spatial tokens, swept over their domain with the host compiler (no HIP, no GPU).
//   * bias: every (L, H, Hb in {1, H}): the last offset is the extent - 1; by enumeration every (hb, i, j) has an offset of
//     its own inside (Hb, L, L), and with Hb = 1 every head reads slice 0;
//   * sums over sequences: the slots' ranges cover [0, S) exactly once, every slab offset is inside the queried workspace,
//     stage 1 of the bias gradient reads every element of dS exactly once, with an offset inside (N, H, L, L);
//   * spatial tokens: the tile fits its LDS over the whole (C, V) domain (V*C above 2048 included), frame blocks cover
//     [0, T'); by enumeration the map x -> tok is a bijection onto the token tensor (CLS rows written once each), every
//     offset inside its tensor, every positional offset inside (L, C).
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

static void check_bias(int L, int H, int Hb, bool enumerate) {
  ++cases;
  CHECK(enc_bias_heads_ok(Hb, H), "Hb %d H %d", Hb, H);
  const long n = (long)Hb * L * L;
  CHECK(enc_bias_index(H - 1, L - 1, L - 1, L, Hb) == n - 1, "bias last L %d H %d Hb %d", L, H, Hb);
  CHECK(enc_bias_index(0, 0, 0, L, Hb) == 0, "bias first");
  if (!enumerate) return;
  std::vector<int> hit(n, 0);
  for (int h = 0; h < H; ++h)
    for (int i = 0; i < L; ++i)
      for (int j = 0; j < L; ++j) {
        const long idx = enc_bias_index(h, i, j, L, Hb);
        CHECK(idx >= 0 && idx < n, "bias idx %ld", idx);
        if (Hb == 1) CHECK(idx == (long)i * L + j, "shared slice h %d", h);
        if (idx >= 0 && idx < n) ++hit[idx];
      }
  for (long e = 0; e < n; ++e) CHECK(hit[e] == (Hb == 1 ? H : 1), "bias[%ld] read %d times", e, hit[e]);
}

static void check_slots(long S) {
  ++cases;
  const long slots = enc_seq_slots(S);
  CHECK(slots >= 1 && slots * ENC_SEQ_CHUNK >= S && (slots - 1) * ENC_SEQ_CHUNK < S, "S %ld slots %ld", S, slots);
  long covered = 0;
  for (long b = 0; b < slots; ++b) {
    const long s0 = b * ENC_SEQ_CHUNK, s1 = s0 + ENC_SEQ_CHUNK < S ? s0 + ENC_SEQ_CHUNK : S;
    CHECK(s0 == covered && s1 > s0, "S %ld slot %ld", S, b);
    covered = s1;
  }
  CHECK(covered == S, "S %ld covered %ld", S, covered);
}

// stage 1 of the bias gradient as bias_partial_kernel walks it
static void check_bias_grad(int N, int L, int H, int Hb, bool enumerate) {
  ++cases;
  CHECK(enc_bias_grad_domain(N, L, H, Hb), "bias grad domain %d %d %d %d", N, L, H, Hb);
  const long LL = (long)L * L, W = (long)Hb * LL, slots = enc_seq_slots(N), dsn = (long)N * H * LL;
  const long ws = enc_bias_grad_ws_bytes(N, L, H, Hb);
  CHECK(ws == slots * W * 4, "bias grad ws");
  CHECK(enc_seq_slab_index(slots - 1, W - 1, W) * 4 + 4 == ws, "slab last");
  CHECK(enc_prob_index(N - 1, H - 1, 0, 0, L, H) + LL - 1 == dsn - 1, "dS last");
  CHECK(W <= ENC_SEQ_MAX_W && W + 16 < 0x7fffffffL && slots <= ENC_SEQ_MAX_SLOTS, "grid");
  if (!enumerate) return;
  std::vector<int> hit(dsn, 0), slab(slots * W, 0);
  for (long slot = 0; slot < slots; ++slot)
    for (long col = 0; col < W; ++col) {
      const int hb = (int)(col / LL);
      const long ij = col - (long)hb * LL;
      const int h0 = Hb == 1 ? 0 : hb, h1 = Hb == 1 ? H : hb + 1;
      const long n0 = slot * ENC_SEQ_CHUNK, n1 = n0 + ENC_SEQ_CHUNK < N ? n0 + ENC_SEQ_CHUNK : N;
      for (long n = n0; n < n1; ++n)
        for (int h = h0; h < h1; ++h) {
          const long idx = enc_prob_index((int)n, h, 0, 0, L, H) + ij;
          CHECK(idx >= 0 && idx < dsn, "dS idx %ld", idx);
          if (idx >= 0 && idx < dsn) ++hit[idx];
        }
      const long si = enc_seq_slab_index(slot, col, W);
      CHECK(si >= 0 && si < slots * W, "slab idx %ld", si);
      if (si >= 0 && si < slots * W) ++slab[si];
    }
  for (long e = 0; e < dsn; ++e) CHECK(hit[e] == 1, "dS[%ld] read %d times (N %d L %d H %d Hb %d)", e, hit[e], N, L, H, Hb);
  for (long e = 0; e < slots * W; ++e) CHECK(slab[e] == 1, "slab[%ld] written %d times", e, slab[e]);
}

static void check_stokens(int N, int M, int C, int Tp, int V, int has_cls, bool enumerate) {
  ++cases;
  CHECK(enc_stok_domain(N, M, C, Tp, V, has_cls), "stok domain %d %d %d %d %d", N, M, C, Tp, V);
  const EncTokPlan p = enc_tok_plan(C, Tp, V);
  const int D = V * C, L = M * V + has_cls;
  CHECK(p.lds_floats <= ENC_TOK_LDS, "C %d T' %d V %d lds %d", C, Tp, V, p.lds_floats);
  CHECK(p.tt >= 1 && p.tt <= Tp && p.ntb * p.tt >= Tp && (p.ntb - 1) * p.tt < Tp, "C %d T' %d V %d frames", C, Tp, V);
  CHECK(p.w >= p.tt * V && (C - 1) * p.w + p.tt * V - 1 < p.lds_floats, "C %d T' %d V %d tile", C, Tp, V);
  CHECK(enc_stok_index(N - 1, Tp - 1, L - 1, C - 1, Tp, L, C) == (long)N * Tp * L * C - 1, "stok last");
  CHECK(enc_stok_bwd_ws_bytes(N, M, C, Tp, V, has_cls) == enc_seq_slots((long)N * Tp) * L * C * 4, "stok ws");
  CHECK((long)p.ntb * N * M <= 0x7fffffffL && enc_seq_slots((long)N * Tp) <= ENC_SEQ_MAX_SLOTS, "stok grids");
  if (!enumerate) return;
  const long xn = (long)N * M * C * Tp * V, tn = (long)N * Tp * L * C;
  std::vector<int> xs(xn, 0), ts(tn, 0);
  for (int nm = 0; nm < N * M; ++nm)
    for (int tb = 0; tb < p.ntb; ++tb) {
      const int n = nm / M, m = nm - n * M;
      const int t0 = tb * p.tt, nt = p.tt < Tp - t0 ? p.tt : Tp - t0, run = nt * V;
      const int l0 = has_cls + m * V;
      for (int e = 0; e < C * run; ++e) {
        const int c = e / run, q = e - c * run;
        const long idx = enc_x_index(nm, c, t0, 0, C, Tp, V) + q;
        CHECK(c * p.w + q < p.lds_floats && idx >= 0 && idx < xn, "x idx");
        if (idx >= 0 && idx < xn) ++xs[idx];
      }
      for (int e = 0; e < nt * D; ++e) {
        const int tt = e / D, f = e - tt * D, v = f / C, c = f - v * C;
        const long idx = enc_stok_index(n, t0 + tt, l0, 0, Tp, L, C) + f;
        CHECK(idx == enc_stok_index(n, t0 + tt, l0 + v, c, Tp, L, C), "token l0 + v, feature c");
        CHECK(c * p.w + tt * V + v < p.lds_floats && l0 + v < L && idx >= 0 && idx < tn, "tok idx");
        CHECK((long)l0 * C + f < (long)L * C, "pe idx");
        if (idx >= 0 && idx < tn) ++ts[idx];
      }
      if (has_cls && m == 0)
        for (int e = 0; e < nt * C; ++e) {
          const int tt = e / C, c = e - tt * C;
          const long idx = enc_stok_index(n, t0 + tt, 0, c, Tp, L, C);
          CHECK(idx >= 0 && idx < tn, "cls idx");
          if (idx >= 0 && idx < tn) ++ts[idx];
        }
    }
  for (long i = 0; i < xn; ++i) CHECK(xs[i] == 1, "x[%ld] read %d times", i, xs[i]);
  for (long i = 0; i < tn; ++i) CHECK(ts[i] == 1, "tok[%ld] written %d times (C %d T' %d V %d M %d)", i, ts[i], C, Tp, V, M);
  // the sums: stage 1 reads column col < L*C (dpe) or < C (dcls) of every sequence
  const long S = (long)N * Tp, LC = (long)L * C;
  CHECK((S - 1) * LC + LC - 1 == tn - 1, "last column of the last sequence");
}

int main() {
  for (int L = 1; L <= ENC_MAX_L; ++L)
    for (int H : {1, 2, 3, 8, 2048}) {
      check_bias(L, H, 1, false);
      check_bias(L, H, H, false);
    }
  for (int L : {1, 2, 7, 37, 51})
    for (int H : {1, 2, 3}) {
      check_bias(L, H, 1, true);
      check_bias(L, H, H, true);
    }
  CHECK(!enc_bias_heads_ok(2, 3) && !enc_bias_heads_ok(0, 3) && !enc_bias_heads_ok(4, 3) && enc_bias_heads_ok(1, 1), "Hb edges");
  for (long S = 1; S <= 5000; ++S) check_slots(S);
  for (long S : {6400L, 65535L, 2097119L, 2097120L}) check_slots(S);
  for (int L = 1; L <= ENC_MAX_L; L += 3)
    for (int H : {1, 3, 8})
      for (int N : {1, 31, 32, 33, 300, 6400, 2097120}) {
        check_bias_grad(N, L, H, 1, false);
        check_bias_grad(N, L, H, H, false);
      }
  const int grads[][3] = {{3, 51, 3}, {2, 51, 3}, {5, 37, 1}, {1, 1, 2}, {300, 51, 3}, {33, 7, 2}, {64, 5, 3}, {65, 3, 2}};
  for (auto& g : grads) {
    check_bias_grad(g[0], g[1], g[2], 1, true);
    check_bias_grad(g[0], g[1], g[2], g[2], true);
  }
  CHECK(!enc_bias_grad_domain(0, 5, 3, 1) && !enc_bias_grad_domain(1, ENC_MAX_L + 1, 3, 1) && !enc_bias_grad_domain(1, 5, 3, 2) &&
            !enc_bias_grad_domain(2097121, 5, 3, 1) && enc_bias_grad_domain(2097120, 5, 3, 3), "bias grad domain edges");
  CHECK(enc_bias_grad_ws_bytes(6400, 51, 3, 1) == 200L * 2601 * 4, "ws at the workload's shape");
  // spatial tokens: every (C, V) whose frame fits the tile, on a coarse grid; M*V + cls <= 640
  for (int V = 1; V <= 64; ++V)
    for (int C = 1; C <= ENC_MAX_D && (long)C * (V | 1) <= ENC_TOK_LDS; C += (C < 32 ? 1 : 37))
      for (int M = 1; M <= 3; ++M)
        for (int Tp = 1; Tp <= 300; Tp += (Tp < 12 ? 1 : 41))
          for (int cls = 0; cls < 2; ++cls)
            if (M * V + cls <= ENC_MAX_L) check_stokens(2, M, C, Tp, V, cls, false);
  check_stokens(64, 2, 144, 100, 25, 1, false);                  // the shipped shape: V*C = 3600, one frame per workgroup
  const int toks[][5] = {{1, 2, 3, 1, 18}, {2, 2, 24, 10, 25}, {2, 2, 25, 3, 25}, {11, 1, 3, 3, 18}, {1, 1, 1, 1, 1},
                         {1, 2, 144, 4, 25}, {2, 3, 7, 11, 5}, {1, 1, 2048, 2, 1}, {1, 2, 64, 9, 32}, {2, 1, 327, 2, 24}};
  for (auto& t : toks)
    for (int cls = 0; cls < 2; ++cls) check_stokens(t[0], t[1], t[2], t[3], t[4], cls, true);
  CHECK(!enc_stok_domain(1, 2, 16, 10, 320, 1) && enc_stok_domain(1, 2, 16, 10, 320, 0) && !enc_stok_domain(1, 1, 2049, 1, 1, 0) &&
            !enc_stok_domain(1, 1, 328, 1, 24, 0) && !enc_stok_domain(0, 1, 1, 1, 1, 0) &&
            !enc_stok_domain(2097121, 1, 1, 1, 1, 0) && enc_stok_domain(64, 2, 144, 100, 25, 1), "stok domain edges");
  printf("%ld cases, %ld failures\n", cases, failures);
  return failures ? 1 : 0;
}
