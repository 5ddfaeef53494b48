// Input gradients of the base SGN in eval mode (the backward of sgn.hip with respect to x; the parameter gradients are
// sgn_wgrad.hip, on taping instantiations of the same kernels) and the adjoint of the sampler.  Four kernels, the first
// three in sgn_bwd_kernels.h (instantiated here without a tape):
//   sgn_clip_bwd_kernel     d logits -> d feat, one workgroup per clip: recomputes H = feat + tem1, Y1, y2 and the arg-max
//                           frame of every column (pass 1), then goes back tile by tile through fc, the maximum, the 1x1
//                           conv and the 3-tap conv (pass 2).
//   sgn_frames_bwd_kernel   d feat -> dj, dd (gradients of the joint and the dif branch, workspace), one workgroup per
//                           frame: recomputes the frame's forward with the forward's own operation order, then the
//                           maximum over joints, the three gcn_spa, the softmax, g1 / g2 and the two embeddings.
//   sgn_dif_combine_kernel  dx[t] = dj[t] + dd[t] [t > 0] - dd[t + 1] [t + 1 < seg]: the dif coupling, inside a clip.
//   sgn_sample_bwd_kernel   d out -> d win, the adjoint of the gather, one workgroup per window.
// Arithmetic as in the forward: exact-f32 MFMA (v_mfma_f32_32x32x2_f32) in every AGCN_GEMM mode, every sum in a fixed
// order, no atomics, no launch reads another clip's intermediates: a clip's dx is the same bits alone and in any batch.
// ReLU's derivative at 0 is 0; a maximum routes to its lowest index (ties only happen at 0, where nothing flows).
// Geometry, the LDS carve and every guarded index: sgn_bwd_plan.h.
#include "agcn_common.h"
#include "sgn_bwd_plan.h"
#include "sgn_bwd_kernels.h"

__global__ __launch_bounds__(SGN_THREADS) void sgn_sample_bwd_kernel(const float* __restrict__ win,
                                                                     const unsigned* __restrict__ r,
                                                                     const float* __restrict__ dout, float* dwin, int T,
                                                                     int V, int S, int seg) {
  __shared__ unsigned short rows[SGN_SAMPLE_MAX_ROWS];       // the kept-row table of sgn_sample_kernel
  __shared__ int scan[SGN_THREADS];
  __shared__ unsigned char flag[SGN_SAMPLE_MAX_ROWS];
  const long n = blockIdx.x;
  const int tid = threadIdx.x;
  const int nrows = 2 * T;
  for (int row = tid; row < nrows; row += SGN_THREADS) {
    const int t = row >> 1, m = row & 1;
    bool any = false;
    for (int c = 0; c < 3; ++c)
      for (int v = 0; v < V; ++v) any |= win[sgn_win_index(n, c, t, v, m, T, V)] != 0.f;
    flag[row] = any ? 1 : 0;
  }
  const long per = (long)3 * T * V * 2;
  for (long e = tid; e < per; e += SGN_THREADS) dwin[n * per + e] = 0.f;
  __syncthreads();
  unsigned keep = 0;
  for (int i = 0; i < SGN_SAMPLE_CHUNK; ++i) {
    const int row = tid * SGN_SAMPLE_CHUNK + i;
    if (row < nrows && flag[row]) keep |= 1u << i;
  }
  const int mine = __popc(keep);
  scan[tid] = mine;
  __syncthreads();
  for (int d = 1; d < SGN_THREADS; d <<= 1) {
    const int add = tid >= d ? scan[tid - d] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  const int kept = scan[SGN_THREADS - 1];
  int pos = scan[tid] - mine;
  for (int i = 0; i < SGN_SAMPLE_CHUNK; ++i)
    if (keep >> i & 1u) rows[pos++] = (unsigned short)(tid * SGN_SAMPLE_CHUNK + i);
  __syncthreads();
  const int L = kept > 0 ? sgn_sample_rows(kept, seg) : 0;
  const int F = V * 3;
  // thread fcol owns feature column (v, c) of every row of the window: the adds come in the order s major, k minor
  if (tid < F) {
    const int v = tid / 3, c = tid % 3;
    for (int s = 0; s < S; ++s)
      for (int k = 0; k < seg; ++k) {
        const int idx = sgn_pick_source(k, L, seg, r[(n * S + s) * seg + k], kept);
        if (idx >= 0) {                           // -1: the zero padding or an empty window, no source row
          const int row = rows[idx];
          dwin[sgn_win_index(n, c, row >> 1, v, row & 1, T, V)] += dout[sgn_sample_out_index(n, s, k, tid, S, seg, V)];
        }
      }
  }
}

extern "C" size_t agcn_sgn_frames_bwd_weights(int V) {
  return V >= 2 && V <= SGN_MAX_V ? (size_t)sgn_frames_wt().total : 0;
}
extern "C" size_t agcn_sgn_clip_bwd_weights(int seg, int num_class) {
  return sgn_clip_domain(1, seg, num_class) ? (size_t)sgn_clip_wt().total : 0;
}
extern "C" size_t agcn_sgn_frames_bwd_workspace(int N, int seg, int V) {
  return sgn_frames_domain(N, seg, V) ? sgn_frames_bwd_ws_floats(N, seg, V) * sizeof(float) : 0;
}

extern "C" int agcn_sgn_clip_bwd(const float* feat, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                                 const float* dlogits, float* dfeat, int N, int seg, int num_class, void* stream) {
  if (!feat || !w || !wt || !dlogits || !dfeat) return AGCN_ERR_ARG;
  if (N < 1 || seg < 1 || num_class < 1) return AGCN_ERR_ARG;
  if (!sgn_clip_domain(N, seg, num_class)) return AGCN_ERR_UNSUPPORTED;
  if (w_floats != (size_t)sgn_clip_w(seg, num_class).total || wt_floats != (size_t)sgn_clip_wt().total) return AGCN_ERR_ARG;
  AGCN_NOTE_KERNEL("sgn_clip_bwd_kernel<f32 mfma> seg=%d clips=%d", seg, N);
  return agcn_launch_big<sgn_clip_bwd_kernel<false>>(dim3((unsigned)N), dim3(SGN_THREADS),
                                                     (size_t)SGN_CLIP_BWD_LDS_FLOATS * 4, (hipStream_t)stream, feat, w, wt,
                                                     dlogits, dfeat, (float*)nullptr, seg, num_class);
}

extern "C" int agcn_sgn_frames_bwd(const float* x, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                                   const float* dfeat, float* dx, void* ws, size_t ws_bytes, int N, int seg, int V,
                                   void* stream) {
  if (!x || !w || !wt || !dfeat || !dx || !ws) return AGCN_ERR_ARG;
  if (N < 1 || seg < 1 || V < 2 || V > SGN_MAX_V) return AGCN_ERR_ARG;
  if (!sgn_frames_domain(N, seg, V)) return AGCN_ERR_UNSUPPORTED;
  if (w_floats != (size_t)sgn_frames_w(V).total || wt_floats != (size_t)sgn_frames_wt().total) return AGCN_ERR_ARG;
  if (ws_bytes < agcn_sgn_frames_bwd_workspace(N, seg, V)) return AGCN_ERR_WORKSPACE;
  const long frames = (long)N * seg, total = frames * (V * 3);
  float* dj = (float*)ws;
  float* dd = dj + total;
  AGCN_NOTE_KERNEL("sgn_frames_bwd_kernel<f32 mfma> V=%d frames=%ld", V, frames);
  int rc = agcn_launch_big<sgn_frames_bwd_kernel<false>>(dim3((unsigned)frames), dim3(SGN_THREADS),
                                                         (size_t)SGN_FRAMES_BWD_LDS_FLOATS * 4, (hipStream_t)stream, x, w, wt,
                                                         dfeat, dj, dd, (float*)nullptr, seg, V);
  if (rc != AGCN_OK) return rc;
  hipLaunchKernelGGL(sgn_dif_combine_kernel, dim3((unsigned)((total + SGN_THREADS - 1) / SGN_THREADS)), dim3(SGN_THREADS), 0,
                     (hipStream_t)stream, (const float*)dj, (const float*)dd, dx, total, seg, V * 3);
  return agcn_check_launch();
}

extern "C" int agcn_sgn_sample_bwd(const float* win, const unsigned* r, const float* dout, float* dwin, int N, int T, int V,
                                   int K, int S, int seg, void* stream) {
  if (!win || !r || !dout || !dwin) return AGCN_ERR_ARG;
  if (!sgn_sample_domain(N, T, V, K, S, seg)) return AGCN_ERR_ARG;
  hipLaunchKernelGGL(sgn_sample_bwd_kernel, dim3((unsigned)N), dim3(SGN_THREADS), 0, (hipStream_t)stream, win, r, dout, dwin,
                     T, V, S, seg);
  return agcn_check_launch();
}
