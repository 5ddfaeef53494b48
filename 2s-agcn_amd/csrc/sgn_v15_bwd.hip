// The input gradient of SGN v15 in eval mode: the backward of sgn_v15.hip.  Three kernels:
//   sgn15_clip_bwd_kernel    d logits -> d feat, one workgroup per clip: d pooled = fc_w . d logits, the clip's forward
//                            again (feat + tem, the block), d pooled routed to the arg-max frame of every column, the
//                            block backward.  tem is a constant: the block's dX is d feat.
//   sgn15_frames_bwd_kernel  d feat -> dj, dd (gradients of the position and the velocity branch, workspace), one workgroup
//                            per frame: the embeddings and the block again, d feat routed to the arg-max joint of every
//                            column, the block backward (columns 64..127 of its dX are spa and go nowhere), the two
//                            embeddings' layers and the DataNorm affine.
//   sgn15_dif_combine_kernel dx[t] = dj[t] + dd[t] [t > 0] - dd[t + 1] [t + 1 < seg]: the dif coupling, inside a clip.
// Nothing of the forward is stored.  The recomputed forward is the forward's own device code (sgn_device.h,
// sgn_v15_device.h), so the arg-max rows are the forward's.  Arithmetic as there: exact-f32 MFMA in every AGCN_GEMM mode,
// every sum in a fixed order, no atomics; a workgroup reads no other clip's or frame's intermediates (the dif coupling
// through the workspace excepted), so a clip's dx is the same bits alone and in any batch.  ReLU's derivative at 0 is 0;
// a maximum routes to its lowest index.  Formulas, the LDS carve and its lifetimes: sgn_v15_bwd_plan.h.
// The first two are templates on bool TAPE.  TAPE = false gives the input gradients alone.  A taping instantiation computes
// what the untaped one computes in the same order (dfeat and dx are the same bits) and copies every operand pair of a
// weight gradient from LDS or the accumulators to a caller-owned tape at the step it is live, for the reductions of
// sgn_v15_wgrad.hip: global stores only, the LDS carve is the untaped one.  Layout: sgn_v15_wgrad_plan.h.
#include "agcn_common.h"
#include "sgn_v15_bwd_plan.h"
#include "sgn_v15_wgrad_plan.h"
#include "sgn_v15_device.h"

template <bool TAPE>
__global__ __launch_bounds__(SGN_THREADS) void sgn15_clip_bwd_kernel(const float* __restrict__ feat,
                                                                     const float* __restrict__ w,
                                                                     const float* __restrict__ wt,
                                                                     const float* __restrict__ dlogits,
                                                                     float* __restrict__ dfeat,
                                                                     float* __restrict__ tape, int seg, int num_class,
                                                                     int heads, int d_head, int ff) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int DIN = SGN15_SPA_OUT, DOUT = SGN15_TEM_OUT, XS = SGN15_X_STRIDE(DIN);
  float* X = lds + SGN15_BWD_LDS_X;
  float* QKV = lds + SGN15_BWD_LDS_QKV(DIN);
  float* DO = lds + SGN15_BWD_LDS_DO(DIN);
  float* P = lds + SGN15_BWD_LDS_P(DIN);
  float* dpool = lds + SGN15_BWD_LDS_MISC(DIN);
  const Sgn15ClipW o = sgn15_clip_w(seg, num_class, heads, d_head, ff);
  const Sgn15ClipWT ot = sgn15_clip_wt(heads, d_head, ff);
  const long n = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  // the taping instantiation: this clip's seg rows of the tape and its row of the pooled maxima
  const Sgn15ClipTape tp = sgn15_clip_tape(TAPE ? (long)gridDim.x : 0, seg, heads, d_head, ff);
  const size_t TC = (size_t)tp.cols;
  float* trow = TAPE ? tape + sgn15_clip_tape_row(n, 0, seg) * TC : nullptr;
  // d pooled[k] = sum over the classes, ascending, of d logits[c] fc_w[k, c]
  for (int k = tid; k < DOUT; k += SGN_THREADS) {
    float s = 0.f;
    for (int c = 0; c < num_class; ++c) s = fmaf(dlogits[n * num_class + c], w[o.fc_w + (long)k * num_class + c], s);
    dpool[k] = s;
  }
  // the frames of the clip with tem added, as the forward loads them
  auto load = [&]() {
    for (int i = tid; i < SGN_VP * DIN; i += SGN_THREADS) {
      const int t = i / DIN, c = i % DIN;
      X[t * XS + c] = t < seg ? feat[(n * seg + t) * DIN + c] + w[o.tem + (long)t * DIN + c] : 0.f;
    }
  };
  load();
  __syncthreads();
  float d[DOUT / SGN15_GROUP];
#pragma unroll
  for (int i = 0; i < DOUT / SGN15_GROUP; ++i) d[i] = dpool[(wave + SGN_WAVES * i) * 32 + r];
  f32x16 dX[DIN / SGN15_GROUP];
  sgn15_block_bwd<DIN, DOUT, TAPE>(X, QKV, DO, P, w, o.blk, wt, ot.blk, seg, heads, d_head, ff, d, load, dX, trow, TC, tp.blk,
                                   TAPE ? tape + tp.ymax + (size_t)n * DOUT : nullptr);
#pragma unroll
  for (int i = 0; i < DIN / SGN15_GROUP; ++i) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int row = mfma_row(j, h);
      if (row < seg) dfeat[(n * seg + row) * DIN + (wave + SGN_WAVES * i) * 32 + r] = dX[i][j];
    }
    if constexpr (TAPE) sgn15_tape_tile(dX[i], seg, trow, TC, tp.dx + (wave + SGN_WAVES * i) * 32);
  }
}

template <bool TAPE>
__global__ __launch_bounds__(SGN_THREADS) void sgn15_frames_bwd_kernel(const float* __restrict__ x,
                                                                       const float* __restrict__ w,
                                                                       const float* __restrict__ wt,
                                                                       const float* __restrict__ dfeat,
                                                                       float* __restrict__ dj, float* __restrict__ dd,
                                                                       float* __restrict__ tape, int seg, int V, int heads,
                                                                       int d_head, int ff) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int DIN = SGN15_SPA_IN, DOUT = SGN15_SPA_OUT, XS = SGN15_X_STRIDE(DIN);
  constexpr int QS = SGN15_QKV_STRIDE, ES = SGN15_BWD_DO_STRIDE;
  float* X = lds + SGN15_BWD_LDS_X;
  float* QKV = lds + SGN15_BWD_LDS_QKV(DIN);
  float* DO = lds + SGN15_BWD_LDS_DO(DIN);
  float* P = lds + SGN15_BWD_LDS_P(DIN);
  float* xin = lds + SGN15_BWD_LDS_MISC(DIN);
  float* X0 = lds + SGN15_BWD_LDS_X0;
  float* E1 = lds + SGN15_BWD_LDS_E1;
  const SgnFramesW o = sgn_frames_w(V);          // only the input sections (aff .. spa1) exist in this image
  const Sgn15BlockW b = sgn15_block_w(sgn15_frames_block_base(V), DIN, DOUT, heads, d_head, ff);
  const Sgn15FramesWT ot = sgn15_frames_wt(heads, d_head, ff);
  const long f = blockIdx.x;                     // frame n * seg + t
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int F = V * 3;
  // the taping instantiation: this frame's V rows of the tape and the column offsets of its sections
  const Sgn15FramesTape tp = sgn15_frames_tape(heads, d_head, ff);
  const size_t TC = (size_t)tp.cols;
  float* trow = TAPE ? tape + sgn15_frames_tape_row(f, 0, V) * TC : nullptr;

  // ---- the frame's tokens: the stages of sgn15_frames_kernel, with E1 and a copy of x0 kept ----
  sgn_norm_input(x, w, o, f, seg, V, xin);
  __syncthreads();
  sgn_embed_first(xin, w, o, E1, ES);
  sgn_fill_spa1(w, o, V, X, XS);
  __syncthreads();
  sgn_embed_second(E1, ES, w, o, X, XS);
  __syncthreads();
  for (int i = tid; i < SGN_VP * DIN; i += SGN_THREADS) X0[i / DIN * XS + i % DIN] = X[i / DIN * XS + i % DIN];
  auto reload = [&]() {
    for (int i = tid; i < SGN_VP * DIN; i += SGN_THREADS) X[i / DIN * XS + i % DIN] = X0[i / DIN * XS + i % DIN];
  };
  float d[DOUT / SGN15_GROUP];
#pragma unroll
  for (int i = 0; i < DOUT / SGN15_GROUP; ++i) d[i] = dfeat[f * DOUT + (wave + SGN_WAVES * i) * 32 + r];
  f32x16 dX[1];
  sgn15_block_bwd<DIN, DOUT, TAPE>(X, QKV, DO, P, w, b, wt, ot.blk, V, heads, d_head, ff, d, reload, dX, trow, TC, tp.blk,
                                   nullptr);

  // ---- the embeddings.  x0[:, 0:64] = pos + vel: waves 0 and 1 hold its gradient, and both second layers take it ----
  float* A2 = QKV;                               // the second layers' activations, masked in place to d(pre-activations)
  float* T = QKV + SGN_C2;                       // d(the first layers' pre-activations)
  gemm_w<1, 0>(E1, ES, SGN_C1, w + o.je2_w, w + o.je2_b, SGN_C1, A2, QS);
  gemm_w<1, 0>(E1 + SGN_C1, ES, SGN_C1, w + o.de2_w, w + o.de2_b, SGN_C1, A2 + SGN_C1, QS);
  if (wave < 2) {
    const int col = wave * 32 + r;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int row = mfma_row(j, h);
      float* p = A2 + row * QS + col;
      p[0] = (row < V && p[0] > 0.f) ? dX[0][j] : 0.f;
      p[SGN_C1] = (row < V && p[SGN_C1] > 0.f) ? dX[0][j] : 0.f;
    }
  } else if constexpr (TAPE) {                     // waves 2, 3: columns 64..127 of dX, the spa half, straight to the tape
    sgn15_tape_tile(dX[0], V, trow, TC, tp.dspa + wave * 32 - SGN_C1);
  }
  __syncthreads();
  if constexpr (TAPE) {
    sgn15_tape_band(E1, ES, V, SGN_C2, trow + tp.e1, TC);
    sgn15_tape_band(A2, QS, V, SGN_C2, trow + tp.de2, TC);
  }
  {
    const int br = wave >> 1, cb = wave & 1;       // waves 0, 1: position branch, waves 2, 3: velocity branch
    f32x16 acc = {};
    const float* a = A2 + br * SGN_C1 + r * QS + h;
    const float* bt = wt + (br ? ot.de2 : ot.je2) + h * SGN_C1 + cb * 32 + r;
#pragma unroll 16
    for (int k = 0; k < SGN_C1; k += 2) acc = mfma32(a[k], bt[k * SGN_C1], acc);
    const int col = br * SGN_C1 + cb * 32 + r;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int row = mfma_row(j, h);
      T[row * QS + col] = E1[row * ES + col] > 0.f ? acc[j] : 0.f;
    }
  }
  __syncthreads();
  if constexpr (TAPE) {
    sgn15_tape_band(T, QS, V, SGN_C2, trow + tp.de1, TC);
    for (int i = tid; i < V * 8; i += SGN_THREADS)           // xn: (position c0..c2, 0, velocity c0..c2, 0) of joint i / 8
      trow[(size_t)(i >> 3) * TC + tp.xn + (i & 7)] = xin[((i >> 2) & 1) * SGN_VP * 4 + (i >> 3) * 4 + (i & 3)];
  }
  // 64 -> 3 and the folded DataNorm scale; one thread per (branch, joint, coordinate), k ascending
  if (tid < 2 * SGN_VP * 3) {
    const int which = tid / (SGN_VP * 3), v = (tid / 3) % SGN_VP, c = tid % 3;
    if (v < V) {
      const float* wi = w + (which ? o.de1_w : o.je1_w) + c * SGN_C1;
      const float* dz = T + v * QS + which * SGN_C1;
      float s = 0.f;
      for (int k = 0; k < SGN_C1; ++k) s = fmaf(dz[k], wi[k], s);
      const int e = v * 3 + c;
      if constexpr (TAPE) trow[(size_t)v * TC + tp.dxn + which * 3 + c] = s;      // d xn, before the folded scale
      (which ? dd : dj)[f * F + e] = s * w[o.aff + (which ? 2 : 0) * F + e];
    }
  }
}

__global__ __launch_bounds__(SGN_THREADS) void sgn15_dif_combine_kernel(const float* __restrict__ dj,
                                                                        const float* __restrict__ dd,
                                                                        float* __restrict__ dx, long total, int seg, int F) {
  const long i = (long)blockIdx.x * SGN_THREADS + threadIdx.x;
  if (i >= total) return;
  const long f = i / F;
  const int e = (int)(i % F);
  float v = dj[i];
  const long own = sgn_dif_own(f, seg), next = sgn_dif_next(f, seg);
  if (own >= 0) v += dd[own * F + e];
  if (next >= 0) v -= dd[next * F + e];
  dx[i] = v;
}

extern "C" size_t agcn_sgn15_frames_bwd_weights(int V, int heads, int d_head, int ff) {
  return sgn15_frames_domain(1, 1, V, heads, d_head, ff) ? (size_t)sgn15_frames_wt(heads, d_head, ff).total : 0;
}
extern "C" size_t agcn_sgn15_clip_bwd_weights(int seg, int num_class, int heads, int d_head, int ff) {
  return sgn15_clip_domain(1, seg, num_class, heads, d_head, ff) ? (size_t)sgn15_clip_wt(heads, d_head, ff).total : 0;
}
extern "C" size_t agcn_sgn15_frames_bwd_workspace(int N, int seg, int V) {
  return sgn_frames_domain(N, seg, V) ? sgn15_frames_bwd_ws_floats(N, seg, V) * sizeof(float) : 0;
}

// ---- the two backward launches: with a tape (of tape_floats floats) the taping instantiation, without one (null) the
// plain one.  The *_tape entries refuse a null tape themselves. ----
static int sgn15_clip_bwd_launch(const float* feat, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                                 const float* dlogits, float* dfeat, int N, int seg, int num_class, int heads, int d_head,
                                 int ff, float* tape, size_t tape_floats, void* stream) {
  if (!feat || !w || !wt || !dlogits || !dfeat) return AGCN_ERR_ARG;
  if (!sgn15_clip_domain(N, seg, num_class, heads, d_head, ff)) return AGCN_ERR_ARG;
  if (w_floats != (size_t)sgn15_clip_w(seg, num_class, heads, d_head, ff).total ||
      wt_floats != (size_t)sgn15_clip_wt(heads, d_head, ff).total)
    return AGCN_ERR_ARG;
  if (tape && tape_floats < sgn15_clip_tape(N, seg, heads, d_head, ff).total) return AGCN_ERR_WORKSPACE;
  const dim3 grid((unsigned)N), block(SGN_THREADS);
  const size_t lds = (size_t)SGN15_CLIP_BWD_LDS_FLOATS * 4;
  if (tape) {
    AGCN_NOTE_KERNEL("sgn15_clip_bwd_kernel<f32 mfma, tape> seg=%d heads=%dx%d ff=%d clips=%d", seg, heads, d_head, ff, N);
    return agcn_launch_big<sgn15_clip_bwd_kernel<true>>(grid, block, lds, (hipStream_t)stream, feat, w, wt, dlogits, dfeat,
                                                        tape, seg, num_class, heads, d_head, ff);
  }
  AGCN_NOTE_KERNEL("sgn15_clip_bwd_kernel<f32 mfma> seg=%d heads=%dx%d ff=%d clips=%d", seg, heads, d_head, ff, N);
  return agcn_launch_big<sgn15_clip_bwd_kernel<false>>(grid, block, lds, (hipStream_t)stream, feat, w, wt, dlogits, dfeat,
                                                       tape, seg, num_class, heads, d_head, ff);
}

static int sgn15_frames_bwd_launch(const float* x, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                                   const float* dfeat, float* dx, void* ws, size_t ws_bytes, int N, int seg, int V, int heads,
                                   int d_head, int ff, float* tape, size_t tape_floats, void* stream) {
  if (!x || !w || !wt || !dfeat || !dx || !ws) return AGCN_ERR_ARG;
  if (!sgn15_frames_domain(N, seg, V, heads, d_head, ff)) return AGCN_ERR_ARG;
  if (w_floats != (size_t)sgn15_frames_floats(V, heads, d_head, ff) ||
      wt_floats != (size_t)sgn15_frames_wt(heads, d_head, ff).total)
    return AGCN_ERR_ARG;
  if (ws_bytes != sgn15_frames_bwd_ws_floats(N, seg, V) * sizeof(float)) return AGCN_ERR_ARG;
  if (tape && tape_floats < sgn15_frames_tape_floats(N, seg, V, heads, d_head, ff)) return AGCN_ERR_WORKSPACE;
  const long frames = (long)N * seg, total = frames * (V * 3);
  float* dj = (float*)ws;
  float* dd = dj + total;
  const dim3 grid((unsigned)frames), block(SGN_THREADS);
  const size_t lds = (size_t)SGN15_FRAMES_BWD_LDS_FLOATS * 4;
  int rc;
  if (tape) {
    AGCN_NOTE_KERNEL("sgn15_frames_bwd_kernel<f32 mfma, tape> V=%d heads=%dx%d ff=%d frames=%ld", V, heads, d_head, ff, frames);
    rc = agcn_launch_big<sgn15_frames_bwd_kernel<true>>(grid, block, lds, (hipStream_t)stream, x, w, wt, dfeat, dj, dd, tape,
                                                        seg, V, heads, d_head, ff);
  } else {
    AGCN_NOTE_KERNEL("sgn15_frames_bwd_kernel<f32 mfma> V=%d heads=%dx%d ff=%d frames=%ld", V, heads, d_head, ff, frames);
    rc = agcn_launch_big<sgn15_frames_bwd_kernel<false>>(grid, block, lds, (hipStream_t)stream, x, w, wt, dfeat, dj, dd, tape,
                                                         seg, V, heads, d_head, ff);
  }
  if (rc != AGCN_OK) return rc;
  hipLaunchKernelGGL(sgn15_dif_combine_kernel, dim3((unsigned)((total + SGN_THREADS - 1) / SGN_THREADS)), dim3(SGN_THREADS),
                     0, (hipStream_t)stream, (const float*)dj, (const float*)dd, dx, total, seg, V * 3);
  return agcn_check_launch();
}

extern "C" int agcn_sgn15_clip_bwd(const float* feat, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                                   const float* dlogits, float* dfeat, int N, int seg, int num_class, int heads, int d_head,
                                   int ff, void* stream) {
  return sgn15_clip_bwd_launch(feat, w, w_floats, wt, wt_floats, dlogits, dfeat, N, seg, num_class, heads, d_head, ff, nullptr,
                               0, stream);
}

extern "C" int agcn_sgn15_frames_bwd(const float* x, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                                     const float* dfeat, float* dx, void* ws, size_t ws_bytes, int N, int seg, int V,
                                     int heads, int d_head, int ff, void* stream) {
  return sgn15_frames_bwd_launch(x, w, w_floats, wt, wt_floats, dfeat, dx, ws, ws_bytes, N, seg, V, heads, d_head, ff, nullptr,
                                 0, stream);
}

extern "C" int agcn_sgn15_clip_bwd_tape(const float* feat, const float* w, size_t w_floats, const float* wt,
                                        size_t wt_floats, const float* dlogits, float* dfeat, int N, int seg, int num_class,
                                        int heads, int d_head, int ff, float* tape, size_t tape_floats, void* stream) {
  if (!tape) return AGCN_ERR_ARG;
  return sgn15_clip_bwd_launch(feat, w, w_floats, wt, wt_floats, dlogits, dfeat, N, seg, num_class, heads, d_head, ff, tape,
                               tape_floats, stream);
}

extern "C" int agcn_sgn15_frames_bwd_tape(const float* x, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                                          const float* dfeat, float* dx, void* ws, size_t ws_bytes, int N, int seg, int V,
                                          int heads, int d_head, int ff, float* tape, size_t tape_floats, void* stream) {
  if (!tape) return AGCN_ERR_ARG;
  return sgn15_frames_bwd_launch(x, w, w_floats, wt, wt_floats, dfeat, dx, ws, ws_bytes, N, seg, V, heads, d_head, ff, tape,
                                 tape_floats, stream);
}
