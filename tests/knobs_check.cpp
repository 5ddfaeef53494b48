// The switch table of 2s-agcn_amd/csrc/knobs.h against the values the hand-written reads it replaced gave.  One child
// process per scenario (a latched switch can be read once per process): the parent re-executes itself with
// "--child <switch index> <text or @unset>", the child prints what its accessor returns and what it returns after the
// variable is changed behind its back.  Host only: no GPU, no HIP.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "knobs.h"

namespace {

const char* const TEXTS[] = {"@unset", "0", "1", "", "8", "-1"};
constexpr int NTEXT = 6;
constexpr int U = AGCN_KNOB_UNSET;

// the expected values, written out from the code the table replaced; columns as TEXTS
struct Expect { AgcnKnob k; AgcnKnobKind kind; int v[NTEXT]; };
const Expect EXPECT[] = {
    //                                               unset  "0" "1"  ""  "8" "-1"
    // strcmp against f32 / bf16x3 / bf16, else 3 (more spellings below)
    {AGCN_GEMM,         AGCN_KNOB_LATCHED,  {3, 3, 3, 3, 3, 3}},
    // nw = (e && atoi(e) == 8) ? 8 : 4
    {AGCN_CHAIN_WAVES,  AGCN_KNOB_LATCHED,  {4, 4, 4, 4, 8, 4}},
    // static const int on = getenv(..) ? atoi(getenv(..)) : 1
    {AGCN_CHAIN_F16X3,  AGCN_KNOB_LATCHED,  {1, 0, 1, 0, 8, -1}},
    {AGCN_CHAIN_WS,     AGCN_KNOB_LATCHED,  {1, 0, 1, 0, 8, -1}},
    {AGCN_WS_K128,      AGCN_KNOB_LATCHED,  {1, 0, 1, 0, 8, -1}},
    // ... : 0
    {AGCN_CHAIN_F32,    AGCN_KNOB_LATCHED,  {0, 0, 1, 0, 8, -1}},
    {AGCN_GC_DBG,       AGCN_KNOB_LATCHED,  {0, 0, 1, 0, 8, -1}},
    {AGCN_DADJ_F16X3,   AGCN_KNOB_LATCHED,  {1, 0, 1, 0, 8, -1}},
    {AGCN_DADJ_RED16,   AGCN_KNOB_LATCHED,  {1, 0, 1, 0, 8, -1}},
    // v = (e && atoi(e) == 8) ? 0 : 1 (four waves): 8, or the default 4
    {AGCN_WGRAD_NW,     AGCN_KNOB_LATCHED,  {4, 4, 4, 4, 8, 4}},
    {AGCN_WGRAD_F16X3,  AGCN_KNOB_LATCHED,  {1, 0, 1, 0, 8, -1}},
    {AGCN_WC_BCH,       AGCN_KNOB_LATCHED,  {0, 0, 1, 0, 8, -1}},
    {AGCN_WC_AGG16,     AGCN_KNOB_LATCHED,  {1, 0, 1, 0, 8, -1}},
    // v = (e && atoi(e) == 0) ? 0 : 1
    {AGCN_WC_PC,        AGCN_KNOB_LATCHED,  {1, 0, 1, 0, 1, 1}},
    // ... : -1 (three states)
    {AGCN_WC_NWP8,      AGCN_KNOB_LATCHED,  {-1, 0, 1, 0, 8, -1}},
    {AGCN_CB_DBG,       AGCN_KNOB_LATCHED,  {0, 0, 1, 0, 8, -1}},
    {AGCN_CONV_PC,      AGCN_KNOB_LATCHED,  {1, 0, 1, 0, 1, 1}},
    {AGCN_CONV_NWP2,    AGCN_KNOB_LATCHED,  {0, 0, 1, 0, 8, -1}},
    {AGCN_CONV_WIDE,    AGCN_KNOB_LATCHED,  {1, 0, 1, 0, 1, 1}},
    {AGCN_CONV_F16X3,   AGCN_KNOB_LATCHED,  {1, 0, 1, 0, 8, -1}},
    {AGCN_WGRAD9_F16X3, AGCN_KNOB_LATCHED,  {1, 0, 1, 0, 8, -1}},
    {AGCN_WGRAD9_BF16,  AGCN_KNOB_LATCHED,  {1, 0, 1, 0, 1, 1}},
    {AGCN_WGRAD_BF16,   AGCN_KNOB_LATCHED,  {1, 0, 1, 0, 1, 1}},
    {AGCN_ADJ_WS,       AGCN_KNOB_LATCHED,  {1, 0, 1, 0, 8, -1}},
    {AGCN_SCORES_ROWS,  AGCN_KNOB_LATCHED,  {1, 0, 1, 0, 8, -1}},
    // if (const char* e = getenv(..)) want = atoi(e): unset leaves the launcher's own value
    {AGCN_WS_SPLIT,     AGCN_KNOB_PER_CALL, {U, 0, 1, 0, 8, -1}},
    {AGCN_AW_SPLIT,     AGCN_KNOB_PER_CALL, {U, 0, 1, 0, 8, -1}},
    // if (!dry) if (const char* e = getenv(..)) a.dbg = atoi(e): unset keeps AGCN_GC_DBG's value
    {AGCN_WS_DBG,       AGCN_KNOB_PROBE,    {U, 0, 1, 0, 8, -1}},
    {AGCN_DADJ_DBG,     AGCN_KNOB_PROBE,    {0, 0, 1, 0, 8, -1}},
    // a.dbg = e ? atoi(e) : 0
    {AGCN_WC_DBG,       AGCN_KNOB_PROBE,    {0, 0, 1, 0, 8, -1}},
    // a.pad = (e && atoi(e) == 0) ? 0 : 1
    {AGCN_WC_PAD,       AGCN_KNOB_PROBE,    {1, 0, 1, 0, 1, 1}},
    {AGCN_AF_DBG,       AGCN_KNOB_PROBE,    {0, 0, 1, 0, 8, -1}},
};
struct GemmExpect { const char* text; int v; };
const GemmExpect GEMM_EXPECT[] = {{"f32", 0}, {"bf16", 1}, {"bf16x3", 2}, {"bf16x6", 3}, {"F32", 3}, {"bf16x", 3}};

int read_by_kind(AgcnKnob k, const AgcnDryRun* dry) {
  switch (agcn_knob_row(k).kind) {
    case AGCN_KNOB_LATCHED: return agcn_knob(k);
    case AGCN_KNOB_PER_CALL: return agcn_knob_now(k);
    default: return agcn_probe(k, dry);
  }
}

// child: "<first read> <read after the variable changed> <the same with a dry-run record>"; the variable changes to "1"
// after a first read of 0 and to "0" otherwise (AGCN_GEMM: to another mode), so a fresh read always differs
int child(int idx, const char* text) {
  const AgcnKnob k = (AgcnKnob)idx;
  const char* name = agcn_knob_row(k).name;
  if (strcmp(text, "@unset")) setenv(name, text, 1); else unsetenv(name);
  const AgcnDryRun* dry = reinterpret_cast<const AgcnDryRun*>(name);      // (non-null is all a PROBE read looks at)
  const int first = read_by_kind(k, nullptr);
  setenv(name, k == AGCN_GEMM ? (first == 0 ? "bf16" : "f32") : (first == 0 ? "1" : "0"), 1);
  printf("%d %d %d\n", first, read_by_kind(k, nullptr), read_by_kind(k, dry));
  return 0;
}

bool run_child(const char* self, int idx, const char* text, int out[3]) {
  const std::string cmd = std::string("'") + self + "' --child " + std::to_string(idx) + " '" + text + "'";
  FILE* f = popen(cmd.c_str(), "r");
  if (!f) return false;
  const int n = fscanf(f, "%d %d %d", &out[0], &out[1], &out[2]);
  return pclose(f) == 0 && n == 3;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "--child")) return child(atoi(argv[2]), argv[3]);
  int cases = 0, failures = 0;
  auto check = [&](bool ok, const char* name, const char* text, const char* what, int got, int want) {
    ++cases;
    if (ok) return;
    ++failures;
    printf("FAIL %s=%s: %s: got %d, expected %d\n", name, text, what, got, want);
  };
  if (sizeof(EXPECT) / sizeof(EXPECT[0]) != AGCN_KNOB_COUNT) {
    printf("FAIL: %zu rows expected, the table has %d\n", sizeof(EXPECT) / sizeof(EXPECT[0]), (int)AGCN_KNOB_COUNT);
    return 1;
  }
  for (int i = 0; i < AGCN_KNOB_COUNT; ++i) {
    const Expect& e = EXPECT[i];
    const AgcnKnobRow& r = agcn_knob_row(e.k);
    check(e.k == i, r.name, "", "row order", e.k, i);
    check(r.kind == e.kind, r.name, "", "kind", r.kind, e.kind);
    check(r.def == e.v[0], r.name, "", "default", r.def, e.v[0]);
    for (int t = 0; t < NTEXT; ++t) {
      int got[3];
      if (!run_child(argv[0], i, TEXTS[t], got)) { check(false, r.name, TEXTS[t], "child failed", 0, 0); continue; }
      check(got[0] == e.v[t], r.name, TEXTS[t], "value", got[0], e.v[t]);
      if (e.kind == AGCN_KNOB_LATCHED) {
        check(got[1] == e.v[t], r.name, TEXTS[t], "latched value after setenv", got[1], e.v[t]);
      } else {
        const int changed = e.v[t] == 0 ? 1 : 0;      // what a fresh read gives once the child has changed the variable
        check(got[1] == changed, r.name, TEXTS[t], "fresh value after setenv", got[1], changed);
      }
      if (e.kind == AGCN_KNOB_PROBE) check(got[2] == r.def, r.name, TEXTS[t], "value in a dry run", got[2], r.def);
    }
  }
  for (const GemmExpect& g : GEMM_EXPECT) {
    int got[3];
    const bool ran = run_child(argv[0], AGCN_GEMM, g.text, got);
    check(ran && got[0] == g.v && got[1] == g.v, "AGCN_GEMM", g.text, "mode", ran ? got[0] : -99, g.v);
  }
  printf("%d switches, %d cases, %d failures\n", (int)AGCN_KNOB_COUNT, cases, failures);
  return failures ? 1 : 0;
}
