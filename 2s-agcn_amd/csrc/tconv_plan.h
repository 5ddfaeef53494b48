// The one description of a temporal convolution  y[t] = sum_k w[k] x[t*stride + k - pad]  that every launch ladder
// consumes (conv_gemm.hip, conv_gemm_bf16.hip, conv_wgrad.hip): its domain, its output-frame count, and the PASSES its
// forward and its backward-data are launched as.  Host only, plain C++17, no HIP: tests/tconv_plan_check.cpp compiles it
// with the host compiler and holds it against the definition.
#pragma once
#include <type_traits>

#ifndef AGCN_ERR_UNSUPPORTED
#define AGCN_ERR_UNSUPPORTED (-3)        // as in include/agcn_hip.h, for the host-only check that includes this file alone
#endif

// the supported domain (agcn_tconv_*), and the shapes the agcn_conv_* entry points cover: rows of the same plan that keep
// the kernel instantiations they were tuned with (the rung table of DESIGN.md)
static inline bool agcn_tconv_domain(int T, int taps, int stride, int pad) {
  return taps >= 1 && taps <= 9 && stride >= 1 && stride <= 9 && pad >= 0 && pad <= (taps - 1) / 2 && T + 2 * pad >= taps;
}
static inline bool agcn_tconv_legacy(int taps, int stride, int pad) {
  return pad == (taps - 1) / 2 && (taps == 1 || taps == 9) && (stride == 1 || stride == 2);
}
static inline int tconv_out_frames(int T, int taps, int stride, int pad) { return (T + 2 * pad - taps) / stride + 1; }

// One launch: output frame slot tau < T_out is frame tau*out_fs + out_fo of the output tensor and contracts the source
// frames tau*src_stride + f_off + j, j < taps (frames outside [0, T_src) read as zero), with the weight tap
// tap_flip_from >= 0 ? tap_flip_from - (j*tap_mul + tap_add) : j.
struct TconvPass {
  int taps;                              // J, the kernel's TAPS; an empty pass launches with 1 tap and Kinner = 0
  int T_out;
  int out_fs, out_fo;
  int src_stride, f_off;
  int tap_mul, tap_add, tap_flip_from;
  bool empty;                            // no tap reaches these output frames: the epilogue writes 0 (+ addends)
};

struct TconvPlan {
  int taps;                              // of the convolution (the weight tensor's last extent)
  bool bwd;                              // backward-data: the contraction runs over Cout and writes Cin rows
  int T_src, T_full;                     // frames of the tensor read / of the tensor written
  int npasses;
  TconvPass pass[9];
};

inline TconvPlan tconv_plan_fwd(int T, int taps, int stride, int pad) {
  TconvPlan pl = {};
  pl.taps = taps;
  pl.T_src = T; pl.T_full = tconv_out_frames(T, taps, stride, pad);
  pl.npasses = 1;
  pl.pass[0] = {taps, pl.T_full, 1, 0, stride, -pad, 0, 0, -1, false};
  return pl;
}

// dx[t] = sum_{k, tau: stride*tau + k - pad = t} w[k] dy[tau].  The output frames t = stride*tau + r of one residue r form
// a stride-1 problem over tau: only the taps k = k0 + stride*i (k0 = (r + pad) mod stride) reach them,
//   dx[stride*tau + r] = sum_{j<J} w[k0 + stride*(J-1-j)] dy[tau + (r + pad - k0)/stride - (J-1) + j],
// J = number of such taps (0: the residue receives no signal), so no matrix-core work is spent on structural zeros.
inline TconvPlan tconv_plan_bwd_data(int T, int taps, int stride, int pad) {
  TconvPlan pl = {};
  pl.taps = taps; pl.bwd = true;
  pl.T_src = tconv_out_frames(T, taps, stride, pad); pl.T_full = T;
  for (int r = 0; r < stride && r < T; ++r) {
    const int k0 = (r + pad) % stride;
    const int J = k0 < taps ? (taps - k0 + stride - 1) / stride : 0;
    const int T_out = (T - r + stride - 1) / stride;
    if (J > 0) pl.pass[r] = {J, T_out, stride, r, 1, (r + pad - k0) / stride - (J - 1), stride, 0, k0 + stride * (J - 1), false};
    else pl.pass[r] = {1, T_out, stride, r, 1, 0, stride, 0, 0, true};
  }
  pl.npasses = stride < T ? stride : T;
  return pl;
}

// Copies one pass into the argument and problem structs of a launch ladder (ConvGemmArgs/Problem of conv_gemm.hip,
// BfArgs/BfProblem of conv_gemm_bf16.hip: the field names agree), with the rows, the contraction length and the strides
// of the (Cout, Cin, taps) weight tensor as the direction reads it.
template <class P>
void tconv_fill(P& p, const TconvPlan& pl, const TconvPass& ps, int Cin, int Cout) {
  auto& a = p.a;
  a.M = pl.bwd ? Cin : Cout; a.in_rows = pl.bwd ? Cout : Cin; a.Kinner = ps.empty ? 0 : a.in_rows;
  a.T_src = pl.T_src; a.T_full = pl.T_full; a.T_out = ps.T_out;
  a.src_stride = ps.src_stride; a.f_off = ps.f_off; a.out_fs = ps.out_fs; a.out_fo = ps.out_fo;
  p.sa_m = pl.bwd ? pl.taps : (long)Cin * pl.taps; p.sa_c = pl.bwd ? (long)Cin * pl.taps : pl.taps;
  p.tap_mul = ps.tap_mul; p.tap_add = ps.tap_add; p.tap_flip_from = ps.tap_flip_from;
}

// a runtime tap count 1..9 as a compile-time constant: f(std::integral_constant<int, TAPS>) -> int
template <class F>
int dispatch_taps(int taps, F&& f) {
  switch (taps) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
    case 5: return f(std::integral_constant<int, 5>());
    case 6: return f(std::integral_constant<int, 6>());
    case 7: return f(std::integral_constant<int, 7>());
    case 8: return f(std::integral_constant<int, 8>());
    case 9: return f(std::integral_constant<int, 9>());
    default: return AGCN_ERR_UNSUPPORTED;
  }
}
