// Every AGCN_* environment switch the library reads, in one table.  Host-only C++17 (no HIP header: the host compiler
// builds tests/knobs_check.cpp from it).  Nothing else in csrc/ calls getenv.
//
// Kinds:
//   LATCHED   read once per process (the first agcn_knob call latches them all, thread-safely, one copy per library)
//   PER_CALL  read at every launch AND every dry run: it steers the routing / geometry a size query must reproduce
//   PROBE     kernel profiling switch, read at every real launch and NEVER in a dry run (agcn_probe returns the default)
// Parses (what the variable's text becomes; unset gives the default):
//   INT       atoi(text)
//   BOOL      0 when atoi(text) == 0, else 1
//   EIGHT     8 when atoi(text) == 8, else the default
//   GEMM      f32 -> 0, bf16 -> 1, bf16x3 -> 2, anything else -> 3 (bf16x6)
// A switch read as a condition (`agcn_knob(K) != 0`, `&&`) is therefore off only when it is set and atoi gives 0.
// AGCN_KNOB_UNSET as a default marks a switch whose absence means "computed by the launcher".
#pragma once
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#define AGCN_KNOB_UNSET INT_MIN

//  X(name, default, kind, parse, meaning)
#define AGCN_KNOBS(X)                                                                                                   \
  X(AGCN_GEMM, 3, LATCHED, GEMM, "GEMM arithmetic: bf16x6 (default) | f32 | bf16x3 | bf16")                             \
  X(AGCN_CHAIN_WAVES, 4, LATCHED, EIGHT, "waves (= frames) per graph-chain workgroup: 4, or 8")                         \
  X(AGCN_CHAIN_F16X3, 1, LATCHED, INT, "0: graph chain forward / backward-data on bf16x6 instead of f16x3")             \
  X(AGCN_CHAIN_WS, 1, LATCHED, INT, "0: no persistent weight-stationary graph-chain kernel")                            \
  X(AGCN_WS_K128, 1, LATCHED, INT, "0: weight-stationary kernel only up to 64 streamed channels")                       \
  X(AGCN_CHAIN_F32, 0, LATCHED, INT, "1: exact-f32 MFMA aggregation in the graph chain")                                \
  X(AGCN_GC_DBG, 0, LATCHED, INT, "graph-chain profiling bits; non-zero also keeps the weight-stationary kernel out")   \
  X(AGCN_DADJ_F16X3, 1, LATCHED, INT, "0: adjacency gradient on bf16x6 (A/B)")                                          \
  X(AGCN_DADJ_RED16, 1, LATCHED, INT, "0: exact-f32 reduction MFMA in the adjacency gradient (A/B)")                    \
  X(AGCN_WGRAD_NW, 4, LATCHED, EIGHT, "waves per tap-free weight-gradient workgroup: 4 where it pays, or 8 everywhere") \
  X(AGCN_WGRAD_F16X3, 1, LATCHED, INT, "0: tap-free weight gradients on bf16x6 (A/B)")                                  \
  X(AGCN_WC_BCH, 0, LATCHED, INT, "1: split-bf16 aggregation in the producer/consumer weight gradient")                 \
  X(AGCN_WC_AGG16, 1, LATCHED, INT, "0: exact-f32 aggregation chain in the f16x3 weight gradient")                      \
  X(AGCN_WC_PC, 1, LATCHED, BOOL, "0: single-role weight-gradient kernel (A/B)")                                        \
  X(AGCN_WC_NWP8, -1, LATCHED, INT, "plain 1x1 weight gradient: 1 forces / 0 forbids 8 producer waves, -1 by shape")    \
  X(AGCN_CB_DBG, 0, LATCHED, INT, "temporal-convolution profiling bits")                                                \
  X(AGCN_CONV_PC, 1, LATCHED, BOOL, "0: single-role temporal-convolution kernel (A/B)")                                 \
  X(AGCN_CONV_NWP2, 0, LATCHED, INT, "1: two producer waves in the producer/consumer temporal convolution")             \
  X(AGCN_CONV_WIDE, 1, LATCHED, BOOL, "0: no 512-position tiles for 64-row temporal convolutions")                      \
  X(AGCN_CONV_F16X3, 1, LATCHED, INT, "0: temporal convolutions on bf16x6 instead of f16x3")                            \
  X(AGCN_WGRAD9_F16X3, 1, LATCHED, INT, "0: tap weight gradient on bf16x6 (A/B)")                                       \
  X(AGCN_WGRAD9_BF16, 1, LATCHED, BOOL, "0: tap weight gradient on the exact-f32 kernel")                               \
  X(AGCN_WGRAD_BF16, 1, LATCHED, BOOL, "0: tap-free weight gradients on the exact-f32 kernel")                          \
  X(AGCN_ADJ_WS, 1, LATCHED, INT, "0: no weight-stationary adjacency-score kernel")                                     \
  X(AGCN_SCORES_ROWS, 1, LATCHED, INT, "0: LDS-staged adjacency-score kernel (A/B)")                                    \
  X(AGCN_WS_SPLIT, AGCN_KNOB_UNSET, PER_CALL, INT, "frame splits per sample of the weight-stationary graph chain")      \
  X(AGCN_AW_SPLIT, AGCN_KNOB_UNSET, PER_CALL, INT, "frame splits per sample of the weight-stationary adjacency scores") \
  X(AGCN_WS_DBG, AGCN_KNOB_UNSET, PROBE, INT, "weight-stationary graph-chain profiling bits")                           \
  X(AGCN_DADJ_DBG, 0, PROBE, INT, "adjacency-gradient profiling (1: no reduction phase, 2: no projection MFMAs)")       \
  X(AGCN_WC_DBG, 0, PROBE, INT, "tap-free weight-gradient profiling bits")                                              \
  X(AGCN_WC_PAD, 1, PROBE, BOOL, "0: unpadded LDS rows in the tap-free weight gradient")                                \
  X(AGCN_AF_DBG, 0, PROBE, INT, "fused adjacency kernel profiling bits")

enum AgcnKnob {
#define X(name, def, kind, parse, text) name,
  AGCN_KNOBS(X)
#undef X
  AGCN_KNOB_COUNT
};
enum AgcnKnobKind { AGCN_KNOB_LATCHED, AGCN_KNOB_PER_CALL, AGCN_KNOB_PROBE };
enum AgcnKnobParse { AGCN_KNOB_INT, AGCN_KNOB_BOOL, AGCN_KNOB_EIGHT, AGCN_KNOB_GEMM };
struct AgcnKnobRow { const char* name; int def; AgcnKnobKind kind; AgcnKnobParse parse; const char* text; };

inline const AgcnKnobRow& agcn_knob_row(AgcnKnob k) {
  static const AgcnKnobRow rows[AGCN_KNOB_COUNT] = {
#define X(name, def, kind, parse, text) {#name, def, AGCN_KNOB_##kind, AGCN_KNOB_##parse, text},
      AGCN_KNOBS(X)
#undef X
  };
  return rows[k];
}

// the switch's value as the environment holds it NOW
inline int agcn_knob_read(AgcnKnob k) {
  const AgcnKnobRow& r = agcn_knob_row(k);
  const char* e = getenv(r.name);
  if (!e) return r.def;
  switch (r.parse) {
    case AGCN_KNOB_BOOL: return atoi(e) == 0 ? 0 : 1;
    case AGCN_KNOB_EIGHT: return atoi(e) == 8 ? 8 : r.def;
    case AGCN_KNOB_GEMM: return !strcmp(e, "f32") ? 0 : !strcmp(e, "bf16x3") ? 2 : !strcmp(e, "bf16") ? 1 : 3;
    default: return atoi(e);
  }
}

struct AgcnKnobs {
  int v[AGCN_KNOB_COUNT];
  AgcnKnobs() {
    for (int k = 0; k < AGCN_KNOB_COUNT; ++k) v[k] = agcn_knob_read((AgcnKnob)k);
  }
};

struct AgcnDryRun;
// LATCHED switches (an inline function's local static: initialised once, thread-safely, one object per library)
inline int agcn_knob(AgcnKnob k) {
  static const AgcnKnobs latched;
  return latched.v[k];
}
// PER_CALL switches
inline int agcn_knob_now(AgcnKnob k) { return agcn_knob_read(k); }
// PROBE switches: a dry run sees the default
inline int agcn_probe(AgcnKnob k, const AgcnDryRun* dry) { return dry ? agcn_knob_row(k).def : agcn_knob_read(k); }
