// Channel arithmetic of the chained adjacency gradient (gcn_chain.hip: dadj_pack_kernel, gcn_dadj_chain_kernel), shared
// with the host so that tests/dadj_plan_check.cpp can sweep it without a device.
//
// The projection H = Wd^T dy streams the Cout channels of dy in stages of DADJ_KC.  A stage is four 8-channel groups
// og = ks*2 + h (ks: 16-deep MFMA step, h: half of the wave); element e of group og multiplies slot e of the weight
// image's (ks, h) lane.  Both sides must name the same channel of dy, or the weight there must be zero.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AGCN_DADJ_HD __host__ __device__ __forceinline__
#else
#define AGCN_DADJ_HD inline
#endif

constexpr int DADJ_KC = 32;          // dy channels per stage (two 16-deep MFMA steps)

AGCN_DADJ_HD int dadj_stages(int Cout) { return (Cout + DADJ_KC - 1) / DADJ_KC; }

// channel of dy whose weight sits in slot e (0..7) of lane half h, step ks, of stage kc's image (zero where >= Cout)
AGCN_DADJ_HD int dadj_pack_channel(int kc, int ks, int h, int e) { return kc * DADJ_KC + ks * 16 + h * 8 + e; }
AGCN_DADJ_HD bool dadj_pack_live(int o, int Cout) { return o < Cout; }

// first channel of staging group og (0..3) of stage s, and how many of its eight channels exist (0..8)
AGCN_DADJ_HD int dadj_stage_first(int s, int og) { return s * DADJ_KC + og * 8; }
AGCN_DADJ_HD int dadj_stage_count(int o0, int Cout) {
  const int n = Cout - o0;
  return n < 0 ? 0 : (n > 8 ? 8 : n);
}
// channel element e of the group is staged from: o0 + e where it exists.  Elements beyond the tensor's last channel are
// staged as zeros; the channel returned for them only keeps a (never issued) address inside the tensor.
AGCN_DADJ_HD bool dadj_stage_live(int o0, int e, int Cout) { return o0 + e < Cout; }
AGCN_DADJ_HD int dadj_stage_channel(int o0, int e, int Cout) {
  const int o = o0 + e;
  return o < Cout ? o : Cout - 1;
}
