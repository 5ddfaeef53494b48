// Fused eval-mode inference of the base SGN (reference model/architecture/sgn/archiv/sgn.py) and the sampler in front
// of it (reference feeders/loader.py::NTUDataLoaders.to_fix_length, equal-interval branch).  Four kernels:
//   sgn_frames_kernel   joint-level module, one workgroup per frame: dif, the two embeddings + spa1, the adaptive
//                       adjacency g = softmax(g1(x)^T g2(x)), three gcn_spa layers with their BatchNorm folded, the
//                       maximum over joints.  Activations stay in LDS, weights stream from global / L2.
//   sgn_clip_kernel     frame-level module + classifier, one workgroup per clip: + tem1, k = 3 temporal conv, 1x1 conv,
//                       maximum over frames, fc.
//   sgn_sample_kernel   null-row removal, two-body interleave, padding and the S interval draws as one gather.
//   sgn_collate_kernel  the same gather by sample index from a device-resident dataset, with the subject flags and the
//                       training rotation (reference feeders/loader.py::collate_fn_fix_{train,val,test}).
// All products are exact-f32 MFMA (v_mfma_f32_32x32x2_f32) in every AGCN_GEMM mode: the work is launch- and latency-
// bound, the split modes would add range-scaling passes and buy nothing.  Every sum has a fixed order and no launch
// reads another frame's or clip's intermediate, so the outputs are bitwise reproducible and independent of the batch.
// Geometry and every offset: sgn_plan.h.  The stages themselves: sgn_device.h, shared with the backward (sgn_bwd.hip).
#include "agcn_common.h"
#include "sgn_plan.h"
#include "sgn_device.h"

__global__ __launch_bounds__(SGN_THREADS) void sgn_frames_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ w, float* __restrict__ feat,
                                                                 float* __restrict__ gout, int seg, int V) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* bufA = lds + SGN_LDS_BUF_A;
  float* bufB = lds + SGN_LDS_BUF_B;
  float* part = lds + SGN_LDS_PART;
  float* G = lds + SGN_LDS_G;
  float* xin = lds + SGN_LDS_XIN;
  const SgnFramesW o = sgn_frames_w(V);
  const long f = blockIdx.x;                     // frame n * seg + t
  const int tid = threadIdx.x;
  const int BS = SGN_BUF_STRIDE;
  float* X0 = bufA + SGN_C2;                     // x0 = [pos + dif | spa1] = bufA[:, 128:256]

  sgn_norm_input(x, w, o, f, seg, V, xin);
  __syncthreads();
  sgn_embed_first(xin, w, o, bufB, BS);          // bufB[:, 0:64] joint, bufB[:, 64:128] dif
  sgn_fill_spa1(w, o, V, X0, BS);
  __syncthreads();
  sgn_embed_second(bufB, BS, w, o, X0, BS);
  __syncthreads();
  // [g1 | g2] into bufB, the K-split partials of g1 . g2^T as (wave, row) rows of `part`
  sgn_adjacency(X0, BS, w, o, bufB, BS, part, SGN_VP * SGN_G_STRIDE, SGN_G_STRIDE, G, gout ? gout + f * V * V : nullptr, V);
  __syncthreads();
  const int Kg = (V + 1) & ~1;
  // gcn1 (128 -> 128): [g . x0 | x0] = bufA[:, 0:256] -> x1 = bufB[:, 128:256]
  gemm_g(G, Kg, X0, BS, SGN_C2, bufA, BS);
  __syncthreads();
  gemm_w<1, 0>(bufA, BS, 2 * SGN_C2, w + o.c1_w, w + o.c1_b, SGN_C2, bufB + SGN_C2, BS);
  __syncthreads();
  // gcn2 (128 -> 256): [g . x1 | x1] = bufB[:, 0:256] -> x2 = bufA[:, 256:512]
  gemm_g(G, Kg, bufB + SGN_C2, BS, SGN_C2, bufB, BS);
  __syncthreads();
  gemm_w<2, 0>(bufB, BS, 2 * SGN_C2, w + o.c2_w, w + o.c2_b, SGN_C3, bufA + SGN_C3, BS);
  __syncthreads();
  // gcn3 (256 -> 256): [g . x2 | x2] = bufA[:, 0:512] -> maximum over the real joints (local.maxpool at step == seg)
  gemm_g(G, Kg, bufA + SGN_C3, BS, SGN_C3, bufA, BS);
  __syncthreads();
  {
    const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    f32x16 acc[2] = {};
    float m[2];
    mma_w<2>(bufA + r * BS + h, w + o.c3_w + (long)h * SGN_C3 + wave * 32 + r, SGN_C3, 2 * SGN_C3, acc);
    rowmax<2>(acc, w + o.c3_b, V, m);
    if (h == 0)
      for (int i = 0; i < 2; ++i) feat[f * SGN_C3 + (wave + SGN_WAVES * i) * 32 + r] = m[i];
  }
}

__global__ __launch_bounds__(SGN_THREADS) void sgn_clip_kernel(const float* __restrict__ feat,
                                                               const float* __restrict__ w, float* __restrict__ logits,
                                                               int seg, int num_class) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* H = lds + SGN_CLIP_LDS_H;
  float* Y = lds + SGN_CLIP_LDS_Y;
  float* ymax = lds + SGN_CLIP_LDS_MAX;
  const SgnClipW o = sgn_clip_w(seg, num_class);
  const long n = blockIdx.x;
  const int tid = threadIdx.x;
  const int CS = SGN_CLIP_STRIDE;
  for (int i = tid; i < SGN_C4; i += SGN_THREADS) ymax[i] = 0.f;      // values after a ReLU: 0 is the neutral element
  for (int tile = 0; tile < sgn_clip_tiles(seg); ++tile) {
    __syncthreads();
    sgn_clip_load_tile(feat, w, o, n, tile, seg, H);
    __syncthreads();
    sgn_clip_cnn1(H, w, o, Y);
    __syncthreads();
    // local.cnn2 + bn2 + relu and the running maximum over the frames of the clip
    {
      const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
      f32x16 acc[4] = {};
      float m[4];
      mma_w<4>(Y + r * CS + h, w + o.t2_w + (long)h * SGN_C4 + wave * 32 + r, SGN_C4, SGN_C3, acc);
      rowmax<4>(acc, w + o.t2_b, sgn_tile_rows(tile, seg), m);
      if (h == 0)
        for (int i = 0; i < 4; ++i) {                       // a column is owned by the same lane in every tile
          const int col = (wave + SGN_WAVES * i) * 32 + r;
          ymax[col] = fmaxf(ymax[col], m[i]);
        }
    }
  }
  __syncthreads();
  for (int c = tid; c < num_class; c += SGN_THREADS) {
    float s = w[o.fc_b + c];
    for (int k = 0; k < SGN_C4; ++k) s = fmaf(ymax[k], w[o.fc_w + (long)k * num_class + c], s);
    logits[n * num_class + c] = s;
  }
}

__global__ __launch_bounds__(SGN_THREADS) void sgn_sample_kernel(const float* __restrict__ win,
                                                                 const unsigned* __restrict__ r, float* __restrict__ out,
                                                                 int* __restrict__ Lout, int T, int V, int S, int seg) {
  __shared__ unsigned short rows[SGN_SAMPLE_MAX_ROWS];
  __shared__ int scan[SGN_THREADS];
  __shared__ unsigned char flag[SGN_SAMPLE_MAX_ROWS];
  const long n = blockIdx.x;
  const int tid = threadIdx.x;
  const int kept = sgn_kept_rows(win, n, T, V, flag, scan, rows);
  const int L = kept > 0 ? sgn_sample_rows(kept, seg) : 0;
  if (tid == 0) Lout[n] = L;
  const int F = V * 3;
  const long total = (long)S * seg * F;
  for (long e = tid; e < total; e += SGN_THREADS) {
    const int fcol = (int)(e % F), k = (int)(e / F % seg), s = (int)(e / F / seg);
    float val = 0.f;
    if (L > 0) {
      const int idx = sgn_pick(k, L, seg, r[(n * S + s) * seg + k]);
      if (idx < kept) {                           // rows from `kept` on are the zero padding
        const int row = rows[idx], v = fcol / 3, c = fcol % 3;
        val = win[sgn_win_index(n, c, row >> 1, v, row & 1, T, V)];
      }
    }
    out[sgn_sample_out_index(n, s, k, fcol, S, seg, V)] = val;
  }
}

// The training / evaluation collate: sgn_sample_kernel's gather on sample index[n] of a device-resident pool, with the
// subject flag of every picked row and one rotation per sample.  A thread owns whole joints, so that it holds the
// (x, y, z) the rotation mixes.  Without angles no arithmetic touches the values: the same bits as sgn_sample_kernel.
__global__ __launch_bounds__(SGN_THREADS) void sgn_collate_kernel(const float* __restrict__ pool,
                                                                  const long long* __restrict__ index,
                                                                  const unsigned* __restrict__ r,
                                                                  const float* __restrict__ angles,
                                                                  float* __restrict__ out, float* __restrict__ subj,
                                                                  int* __restrict__ Lout, long P, int T, int V, int S,
                                                                  int seg) {
  __shared__ unsigned short rows[SGN_SAMPLE_MAX_ROWS];
  __shared__ int scan[SGN_THREADS];
  __shared__ unsigned char flag[SGN_SAMPLE_MAX_ROWS];
  __shared__ float R[9];
  const long n = blockIdx.x;
  const int tid = threadIdx.x;
  const long src = sgn_collate_source(index, n, P);       // the same for every thread: the branch below is uniform
  const int kept = src >= 0 ? sgn_kept_rows(pool, src, T, V, flag, scan, rows) : 0;
  const int L = kept > 0 ? sgn_sample_rows(kept, seg) : 0;
  if (tid == 0) {
    Lout[n] = L;
    if (angles) sgn_rotation(angles + n * 3, R);
  }
  __syncthreads();
  const long total = (long)S * seg * V;
  for (long e = tid; e < total; e += SGN_THREADS) {
    const int v = (int)(e % V), k = (int)(e / V % seg), s = (int)(e / V / seg);
    float x = 0.f, y = 0.f, z = 0.f, body = 0.f;
    if (L > 0) {
      const int idx = sgn_pick(k, L, seg, r[(n * S + s) * seg + k]);
      if (idx < kept) {                           // rows from `kept` on are the zero padding
        const int row = rows[idx], t = row >> 1, m = row & 1;
        x = pool[sgn_win_index(src, 0, t, v, m, T, V)];
        y = pool[sgn_win_index(src, 1, t, v, m, T, V)];
        z = pool[sgn_win_index(src, 2, t, v, m, T, V)];
        body = (float)m;
        if (angles) {
          const float rx = sgn_rotate(R, 0, x, y, z), ry = sgn_rotate(R, 1, x, y, z), rz = sgn_rotate(R, 2, x, y, z);
          x = rx, y = ry, z = rz;
        }
      }
    }
    const long o = sgn_sample_out_index(n, s, k, v * 3, S, seg, V);
    out[o] = x;
    out[o + 1] = y;
    out[o + 2] = z;
    if (subj && v == 0) subj[sgn_subject_index(n, s, k, S, seg)] = body;
  }
}

extern "C" size_t agcn_sgn_frames_weights(int V) { return V >= 2 && V <= SGN_MAX_V ? (size_t)sgn_frames_w(V).total : 0; }
extern "C" size_t agcn_sgn_clip_weights(int seg, int num_class) {
  return sgn_clip_domain(1, seg, num_class) ? (size_t)sgn_clip_w(seg, num_class).total : 0;
}

extern "C" int agcn_sgn_frames(const float* x, const float* w, size_t w_floats, float* feat, float* g, int N, int seg,
                               int V, void* stream) {
  if (!x || !w || !feat) return AGCN_ERR_ARG;
  if (N < 1 || seg < 1 || V < 2 || V > SGN_MAX_V) return AGCN_ERR_ARG;
  if (!sgn_frames_domain(N, seg, V)) return AGCN_ERR_UNSUPPORTED;
  if (w_floats != (size_t)sgn_frames_w(V).total) return AGCN_ERR_ARG;
  AGCN_NOTE_KERNEL("sgn_frames_kernel<f32 mfma> V=%d frames=%ld", V, (long)N * seg);
  return agcn_launch_big<sgn_frames_kernel>(dim3((unsigned)((long)N * seg)), dim3(SGN_THREADS),
                                            (size_t)SGN_FRAMES_LDS_FLOATS * 4, (hipStream_t)stream, x, w, feat, g, seg, V);
}

extern "C" int agcn_sgn_clip(const float* feat, const float* w, size_t w_floats, float* logits, int N, int seg,
                             int num_class, void* stream) {
  if (!feat || !w || !logits) return AGCN_ERR_ARG;
  if (N < 1 || seg < 1 || num_class < 1) return AGCN_ERR_ARG;
  if (!sgn_clip_domain(N, seg, num_class)) return AGCN_ERR_UNSUPPORTED;
  if (w_floats != (size_t)sgn_clip_w(seg, num_class).total) return AGCN_ERR_ARG;
  AGCN_NOTE_KERNEL("sgn_clip_kernel<f32 mfma> seg=%d clips=%d", seg, N);
  return agcn_launch_big<sgn_clip_kernel>(dim3((unsigned)N), dim3(SGN_THREADS), (size_t)SGN_CLIP_LDS_FLOATS * 4,
                                          (hipStream_t)stream, feat, w, logits, seg, num_class);
}

extern "C" int agcn_sgn_sample(const float* win, const unsigned* r, float* out, int* L, int N, int T, int V, int K, int S,
                               int seg, void* stream) {
  if (!win || !r || !out || !L) return AGCN_ERR_ARG;
  if (!sgn_sample_domain(N, T, V, K, S, seg)) return AGCN_ERR_ARG;
  hipLaunchKernelGGL(sgn_sample_kernel, dim3((unsigned)N), dim3(SGN_THREADS), 0, (hipStream_t)stream, win, r, out, L, T,
                     V, S, seg);
  return agcn_check_launch();
}

extern "C" int agcn_sgn_collate(const float* pool, const long long* index, const unsigned* r, const float* angles,
                                float* out, float* subj, int* L, long P, int N, int T, int V, int K, int S, int seg,
                                void* stream) {
  if (!pool || !r || !out || !L) return AGCN_ERR_ARG;
  if (!sgn_collate_domain(P, N, T, V, K, S, seg)) return AGCN_ERR_ARG;
  if (!index && N > P) return AGCN_ERR_ARG;
  hipLaunchKernelGGL(sgn_collate_kernel, dim3((unsigned)N), dim3(SGN_THREADS), 0, (hipStream_t)stream, pool, index, r,
                     angles, out, subj, L, P, T, V, S, seg);
  return agcn_check_launch();
}
