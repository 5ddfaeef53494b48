// On-load attention gates of the folded inference convolution (agcn_tconv_infer): the streamed operand is
//   x[n][c][t][v] * a_s[n][v] * a_t[n][t] * a_c[n][c]          (reference aagcn.py:264-271, the three "x * se + x" passes)
// and the product is formed where the operand tile goes from registers to LDS, so the gated tensor never exists in HBM.
// The three vectors of a workgroup's sample are a few hundred floats: they are staged in LDS once per workgroup (ones
// where a factor is absent) and every later use is an LDS read -- no global load per element.
// LDS image `gl`:  [0, KP) a_c by input channel (0 beyond C) | [KP, KP+32) a_s by joint | [KP+32, KP+32+FW) a_t by WINDOW
// frame (0 outside the sample).  KP is a multiple of 16, so a K chunk's channel factors are aligned 16-byte reads.
#pragma once
#include "agcn_common.h"

struct GateArgs {
  const float* gs;   // (N, V) or null
  const float* gt;   // (N, T) or null
  const float* gc;   // (N, C) or null
};

static inline int gate_lds_floats(int FW, int KP) { return KP + 32 + ((FW + 3) & ~3); }

template <int NTH>
__device__ __forceinline__ void gate_stage(float* gl, const GateArgs& g, int n, int V, int T, int C, int f0, int FW,
                                           int KP) {
  for (int e = threadIdx.x; e < KP + 32 + FW; e += NTH) {
    float v = 0.f;
    if (e < KP) {
      if (e < C) v = g.gc ? g.gc[(long)n * C + e] : 1.f;
    } else if (e < KP + 32) {
      const int j = e - KP;
      if (j < V) v = g.gs ? g.gs[(long)n * V + j] : 1.f;
    } else {
      const int f = f0 + (e - KP - 32);
      if (f >= 0 && f < T) v = g.gt ? g.gt[(long)n * T + f] : 1.f;
    }
    gl[e] = v;
  }
}

// gate factor of window position r (frame r / V, joint r % V of the staged window); 0 beyond the window
__device__ __forceinline__ float gate_pos(const float* gl, int KP, int r, int V, int WL) {
  if (r >= WL) return 0.f;
  const int f = r / V;
  return gl[KP + (r - f * V)] * gl[KP + 32 + f];
}

// max |a_c| * max |a_s| * max |a_t (window)| of the staged vectors, by every wave for itself (fixed order)
__device__ __forceinline__ float gate_bound(const float* gl, int KP, int FW, int lane) {
  float mc = 0.f, ms = 0.f, mt = 0.f;
  for (int i = lane; i < KP; i += 64) mc = fmaxf(mc, fabsf(gl[i]));
  if (lane < 32) ms = fabsf(gl[KP + lane]);
  for (int i = lane; i < FW; i += 64) mt = fmaxf(mt, fabsf(gl[KP + 32 + i]));
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) {
    mc = fmaxf(mc, __shfl_xor(mc, k));
    ms = fmaxf(ms, __shfl_xor(ms, k));
    mt = fmaxf(mt, __shfl_xor(mt, k));
  }
  return mc * ms * mt;
}
