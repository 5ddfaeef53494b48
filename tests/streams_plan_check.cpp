// Host check of 2s-agcn_amd/csrc/streams_plan.h (no HIP): the per-item functions the stream kernels run are run here
// behind bounds-checking views, over V 1..32, M 1..4, T 1..6, C 1..4 and the parent tables of the three graphs, chains
// and stars.  Checked: every index a kernel would form stays inside the tensor (and inside its own (n, c) row); the
// forward, as a dense matrix, equals the definition written out with five nested loops; the backward, as a dense matrix,
// is the transpose of that forward, stream by stream and in the weighted sum.
#include <stdio.h>
#include <vector>

#include "streams_plan.h"

static long cases = 0, failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    ++cases;                                                                         \
    if (!(cond)) {                                                                   \
      if (++failures <= 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                                \
  } while (0)

static long out_of_range = 0, out_of_row = 0;

// an item-indexed view that refuses what a raw pointer would let through; `row` items belong to one (n, c) row, and an
// access made for item `home` must stay inside the row of `home`
struct View {
  float* p = nullptr;
  long n = 0, row = 1;
  const long* home = nullptr;
  explicit operator bool() const { return p != nullptr; }
  float& operator[](long j) const {
    static float sink;
    if (j < 0 || j >= n) {
      ++out_of_range;
      sink = 0.f;
      return sink;
    }
    if (home && j / row != *home / row) ++out_of_row;
    return p[j];
  }
};

static const int NTU[25] = {1, 20, 20, 2, 20, 4, 5, 6, 20, 8, 9, 10, 0, 12, 13, 14, 0, 16, 17, 18, 20, 22, 7, 24, 11};
static const int KINETICS[18] = {0, 0, 1, 2, 3, 1, 5, 6, 2, 8, 9, 5, 11, 12, 0, 0, 14, 15};
static const int B25_J15[15] = {1, 1, 1, 2, 3, 1, 5, 6, 1, 8, 9, 10, 8, 12, 13};

static std::vector<std::vector<int>> tables(int V) {
  std::vector<std::vector<int>> t;
  std::vector<int> chain(V), back(V), star(V), last(V), self(V);
  for (int v = 0; v < V; ++v) {
    chain[v] = v > 0 ? v - 1 : 0;        // towards joint 0
    back[v] = v + 1 < V ? v + 1 : v;     // towards the last joint: every parent offset positive
    star[v] = 0;                         // V - 1 children of one joint
    last[v] = V - 1;
    self[v] = v;                         // every bone exactly zero
  }
  t.push_back(chain);
  t.push_back(back);
  t.push_back(star);
  t.push_back(last);
  t.push_back(self);
  if (V == 25) t.push_back(std::vector<int>(NTU, NTU + 25));
  if (V == 18) t.push_back(std::vector<int>(KINETICS, KINETICS + 18));
  if (V == 15) t.push_back(std::vector<int>(B25_J15, B25_J15 + 15));
  return t;
}

// the definition, element by element: rows of F[s] (s = 0 bone, 1 joint_motion, 2 bone_motion) over the E elements of x
static void definition(std::vector<std::vector<int>>* F, const std::vector<int>& parent, int NC, int T, int V, int M) {
  const long E = (long)NC * T * V * M;
  for (int s = 0; s < 3; ++s) F[s].assign(E, std::vector<int>(E, 0));
  auto at = [&](int r, int t, int v, int m) { return (((long)r * T + t) * V + v) * M + m; };
  for (int r = 0; r < NC; ++r)
    for (int t = 0; t < T; ++t)
      for (int v = 0; v < V; ++v)
        for (int m = 0; m < M; ++m) {
          const long e = at(r, t, v, m);
          F[0][e][e] += 1;
          F[0][e][at(r, t, parent[v], m)] -= 1;
          if (t + 1 < T) {
            F[1][e][at(r, t + 1, v, m)] += 1;
            F[1][e][e] -= 1;
            F[2][e][at(r, t + 1, v, m)] += 1;
            F[2][e][at(r, t + 1, parent[v], m)] -= 1;
            F[2][e][e] -= 1;
            F[2][e][at(r, t, parent[v], m)] += 1;
          }
        }
}

// W = 1: the scalar path (items are elements, Mw = M); W = M: the vector path (items are joints, Mw = 1, the M lanes of an
// item never mix, so one lane stands for all: the item tensor is the element tensor of M = 1)
static void check_case(const std::vector<int>& parent, int NC, int T, int V, int M, int W, bool dense) {
  const int Mw = M / W, Mi = Mw;                 // persons per joint at item level
  const long items = (long)NC * T * V * Mi, row = (long)T * V * Mi;
  CHECK(agcn_stream_table_ok(parent.data(), V));
  AgcnStreamTable tab;
  for (int v = 0; v < AGCN_STREAM_MAX_V; ++v) tab.parent[v] = v < V ? parent[v] : 0;
  for (int v = 0; v < V; ++v) CHECK(agcn_stream_parent(tab, v, V) == parent[v]);

  long home = 0;
  std::vector<float> x(items), o[3], d[4], dx(items);
  for (auto& a : o) a.assign(items, 0.f);
  for (auto& a : d) a.assign(items, 0.f);
  auto view = [&](std::vector<float>& a) {
    View w;
    w.p = a.data(), w.n = items, w.row = row, w.home = &home;
    return w;
  };
  const View none;
  const long range0 = out_of_range, row0 = out_of_row;

  // positions
  for (long i = 0; i < items; ++i) {
    const AgcnStreamPos pos = agcn_stream_pos((unsigned)i, T, V, Mw);
    CHECK(pos.v == (int)((i / Mi) % V) && pos.t == (int)((i / ((long)Mi * V)) % T));
  }
  // bounds: every subset of outputs / cotangents, every item, values irrelevant
  // (every subset on one and two channel rows; beyond that the rows only repeat, and the full set is enough)
  for (int mask = NC <= 2 ? 1 : 7; mask < 8; ++mask)
    for (home = 0; home < items; ++home)
      agcn_stream_fwd_item<float>(view(x), (mask & 1) ? view(o[0]) : none, (mask & 2) ? view(o[1]) : none,
                                  (mask & 4) ? view(o[2]) : none, tab, (unsigned)home, T, V, Mw);
  for (int mask = NC <= 2 ? 1 : 15; mask < 16; ++mask)
    for (home = 0; home < items; ++home)
      agcn_stream_bwd_item<float>((mask & 1) ? view(d[0]) : none, (mask & 2) ? view(d[1]) : none,
                                  (mask & 4) ? view(d[2]) : none, (mask & 8) ? view(d[3]) : none, view(dx), tab, 1.f, 1.f,
                                  1.f, 1.f, (unsigned)home, T, V, Mw);
  CHECK(out_of_range == range0);
  CHECK(out_of_row == row0);
  if (!dense) return;

  // dense matrices at item level against the definition at the same level (M = Mi)
  std::vector<std::vector<int>> F[3];
  definition(F, parent, NC, T, V, Mi);
  long fwd_bad = 0, bwd_bad = 0, sum_bad = 0;
  for (long k = 0; k < items; ++k) {            // column k of the forward: x = e_k
    x.assign(items, 0.f);
    x[k] = 1.f;
    for (home = 0; home < items; ++home)
      agcn_stream_fwd_item<float>(view(x), view(o[0]), view(o[1]), view(o[2]), tab, (unsigned)home, T, V, Mw);
    for (int s = 0; s < 3; ++s)
      for (long e = 0; e < items; ++e) fwd_bad += (o[s][e] != (float)F[s][e][k]);
  }
  const float w[4] = {1.f, 0.5f, -2.f, 3.f};
  for (long k = 0; k < items; ++k) {            // column k of each backward: d_s = e_k -> dx = row k of F[s], i.e. F[s]^T e_k
    for (int s = 0; s < 4; ++s) {
      d[s].assign(items, 0.f);
      d[s][k] = 1.f;
      for (home = 0; home < items; ++home)
        agcn_stream_bwd_item<float>(s == 0 ? view(d[0]) : none, s == 1 ? view(d[1]) : none, s == 2 ? view(d[2]) : none,
                                    s == 3 ? view(d[3]) : none, view(dx), tab, 1.f, 1.f, 1.f, 1.f, (unsigned)home, T, V,
                                    Mw);
      for (long e = 0; e < items; ++e) bwd_bad += (dx[e] != (s == 0 ? (float)(e == k) : (float)F[s - 1][k][e]));
    }
    for (home = 0; home < items; ++home)      // all four at once with weights: small integers and halves, exact in fp32
      agcn_stream_bwd_item<float>(view(d[0]), view(d[1]), view(d[2]), view(d[3]), view(dx), tab, w[0], w[1], w[2], w[3],
                                  (unsigned)home, T, V, Mw);
    for (long e = 0; e < items; ++e)
      sum_bad += (dx[e] != w[0] * (e == k) + w[1] * F[0][k][e] + w[2] * F[1][k][e] + w[3] * F[2][k][e]);
  }
  CHECK(fwd_bad == 0);
  CHECK(bwd_bad == 0);
  CHECK(sum_bad == 0);
}

int main() {
  // the table check the C entries run before they copy the table into the kernel arguments
  const int ok[3] = {0, 0, 1}, high[3] = {0, 3, 1}, neg[3] = {0, -1, 1};
  CHECK(agcn_stream_table_ok(ok, 3) && agcn_stream_table_ok(ok, 1));
  CHECK(!agcn_stream_table_ok(high, 3) && !agcn_stream_table_ok(neg, 3));
  CHECK(!agcn_stream_table_ok(nullptr, 3) && !agcn_stream_table_ok(ok, 0) && !agcn_stream_table_ok(ok, -1));
  std::vector<int> wide(AGCN_STREAM_MAX_V + 1, 0);
  CHECK(agcn_stream_table_ok(wide.data(), AGCN_STREAM_MAX_V) && !agcn_stream_table_ok(wide.data(), AGCN_STREAM_MAX_V + 1));
  // a table that slipped through would still be clamped into the frame
  AgcnStreamTable bad;
  for (int v = 0; v < AGCN_STREAM_MAX_V; ++v) bad.parent[v] = v % 2 ? 1000 : -1000;
  for (int V = 1; V <= AGCN_STREAM_MAX_V; ++V)
    for (int v = 0; v < V; ++v) CHECK(agcn_stream_parent(bad, v, V) >= 0 && agcn_stream_parent(bad, v, V) < V);

  // width, item count and grid
  CHECK(agcn_stream_width(2, 0x1000) == 2 && agcn_stream_width(2, 0x1008) == 2 && agcn_stream_width(2, 0x1004) == 1);
  CHECK(agcn_stream_width(4, 0x1010) == 4 && agcn_stream_width(4, 0x1008) == 1 && agcn_stream_width(4, 0x1004) == 1);
  CHECK(agcn_stream_width(1, 0x1000) == 1 && agcn_stream_width(3, 0x1000) == 1 && agcn_stream_width(8, 0x1000) == 1);
  CHECK(agcn_stream_items(64, 3, 300, 25, 2, 2) == 64L * 3 * 300 * 25 && agcn_stream_items(64, 3, 300, 25, 2, 1) == 2880000);
  CHECK(agcn_stream_items(1 << 15, 1 << 10, 64, 1, 1, 1) == -1);                      // 2^31 elements
  CHECK(agcn_stream_items(0x7fffffff, 1, 1, 1, 1, 1) == 0x7fffffffLL);
  CHECK(agcn_stream_grid(1) == 1 && agcn_stream_grid(256) == 1 && agcn_stream_grid(257) == 2);
  CHECK(agcn_stream_grid(2048L * 256) == 2048 && agcn_stream_grid(0x7fffffffLL) == 2048);
  // the grid-stride loop's counter is unsigned: the last item plus one whole stride does not wrap
  CHECK(0x7fffffffULL + 2048ULL * 256ULL < 0xffffffffULL);

  for (int V = 1; V <= AGCN_STREAM_MAX_V; ++V) {
    const std::vector<std::vector<int>> tabs = tables(V);
    for (size_t k = 0; k < tabs.size(); ++k)
      for (int M = 1; M <= 4; ++M)
        for (int T = 1; T <= 6; ++T)
          for (int C = 1; C <= 4; ++C) {
            // The dense comparison costs items^2 per case, so it runs where the tensor is small (one channel row and
            // two: rows are independent, two show that nothing crosses them), on single-person rows of any V up to two
            // frames, and on the three graphs' own tables up to six frames.  The vector path at item level is the scalar
            // path of M = 1 whatever M is: compared once, at M = 2.
            const bool graph_table = k >= 5;
            auto dense = [&](int Mi) {
              const long items = (long)C * T * V * Mi;
              return (C <= 2 && items <= 48) || (C == 1 && Mi == 1 && (T <= 2 || graph_table));
            };
            check_case(tabs[k], C, T, V, M, 1, dense(M));
            if (M == 2 || M == 4) check_case(tabs[k], C, T, V, M, M, M == 2 && dense(1));
          }
  }
  printf("%ld cases, %ld failures\n", cases, failures);
  return failures ? 1 : 0;
}
