// Fused eval-mode inference of SGN v15, the attention SGN (reference model/architecture/sgn/sgn_v15.py in the structure
// of config/nturgbd-cross-view/train_sgn_v15.yaml).  Two kernels:
//   sgn15_frames_kernel  one workgroup per frame: dif, the two DataNorm + 1x1 embeddings + spa (the base SGN's input
//                        stages, sgn_device.h), the attention block 128 -> 256 over the joints, the maximum over the
//                        real joints -> feat (N, seg, 256).  tem is added by the clip kernel when it loads feat:
//                        max_v(y[v] + tem[t]) = max_v(y[v]) + tem[t] bit for bit, rounding being monotone.
//   sgn15_clip_kernel    one workgroup per clip: feat + tem, the attention block 256 -> 512 over the frames, the maximum
//                        over the real frames, fc.
// The block is one device function template (sgn_v15_device.h).  All products are exact-f32 MFMA in every AGCN_GEMM
// mode; every sum has a fixed order and no launch reads another frame's or clip's intermediate, so a clip's result is
// the same bits alone and inside any batch.  Geometry and every offset: sgn_v15_plan.h.
#include "agcn_common.h"
#include "sgn_v15_plan.h"
#include "sgn_v15_device.h"

__global__ __launch_bounds__(SGN_THREADS) void sgn15_frames_kernel(const float* __restrict__ x,
                                                                   const float* __restrict__ w, float* __restrict__ feat,
                                                                   float* __restrict__ attn, int seg, int V, int heads,
                                                                   int d_head, int ff) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int DIN = SGN15_SPA_IN, DOUT = SGN15_SPA_OUT, XS = SGN15_X_STRIDE(DIN);
  float* X = lds + SGN15_LDS_X;
  float* QKV = lds + SGN15_LDS_QKV(DIN);
  float* P = lds + SGN15_LDS_P(DIN);
  float* xin = lds + SGN15_LDS_MISC(DIN);
  const SgnFramesW o = sgn_frames_w(V);          // only the input sections (aff .. spa1) exist in this image
  const Sgn15BlockW b = sgn15_block_w(sgn15_frames_block_base(V), DIN, DOUT, heads, d_head, ff);
  const long f = blockIdx.x;                     // frame n * seg + t

  sgn_norm_input(x, w, o, f, seg, V, xin);
  __syncthreads();
  sgn_embed_first(xin, w, o, QKV, SGN15_QKV_STRIDE);      // E[:, 0:64] pos, E[:, 64:128] vel
  sgn_fill_spa1(w, o, V, X, XS);                          // X = [pos + vel | spa]
  __syncthreads();
  sgn_embed_second(QKV, SGN15_QKV_STRIDE, w, o, X, XS);
  __syncthreads();
  float m[DOUT / SGN15_GROUP];
  sgn15_block<DIN, DOUT>(X, QKV, P, w, b, V, heads, d_head, ff,
                         attn ? attn + sgn15_attn_index(f, heads, 0, V, 0, 0) : nullptr, m);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  if (h == 0)
    for (int i = 0; i < DOUT / SGN15_GROUP; ++i) feat[f * DOUT + (wave + SGN_WAVES * i) * 32 + r] = m[i];
}

__global__ __launch_bounds__(SGN_THREADS) void sgn15_clip_kernel(const float* __restrict__ feat,
                                                                 const float* __restrict__ w, float* __restrict__ logits,
                                                                 float* __restrict__ attn, int seg, int num_class,
                                                                 int heads, int d_head, int ff) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int DIN = SGN15_SPA_OUT, DOUT = SGN15_TEM_OUT, XS = SGN15_X_STRIDE(DIN);
  float* X = lds + SGN15_LDS_X;
  float* QKV = lds + SGN15_LDS_QKV(DIN);
  float* P = lds + SGN15_LDS_P(DIN);
  float* ymax = lds + SGN15_LDS_MISC(DIN);
  const Sgn15ClipW o = sgn15_clip_w(seg, num_class, heads, d_head, ff);
  const long n = blockIdx.x;
  const int tid = threadIdx.x;
  // the frames of the clip with tem added; padded frame rows (seg < 32) are zero and excluded from softmax and maximum
  for (int i = tid; i < SGN_VP * DIN; i += SGN_THREADS) {
    const int t = i / DIN, c = i % DIN;
    X[t * XS + c] = t < seg ? feat[(n * seg + t) * DIN + c] + w[o.tem + (long)t * DIN + c] : 0.f;
  }
  __syncthreads();
  float m[DOUT / SGN15_GROUP];
  sgn15_block<DIN, DOUT>(X, QKV, P, w, o.blk, seg, heads, d_head, ff,
                         attn ? attn + sgn15_attn_index(n, heads, 0, seg, 0, 0) : nullptr, m);
  const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  if (h == 0)
    for (int i = 0; i < DOUT / SGN15_GROUP; ++i) ymax[(wave + SGN_WAVES * i) * 32 + r] = m[i];
  __syncthreads();
  for (int c = tid; c < num_class; c += SGN_THREADS) {
    float s = w[o.fc_b + c];
    for (int k = 0; k < DOUT; ++k) s = fmaf(ymax[k], w[o.fc_w + (long)k * num_class + c], s);
    logits[n * num_class + c] = s;
  }
}

extern "C" size_t agcn_sgn15_frames_weights(int V, int heads, int d_head, int ff) {
  return sgn15_frames_domain(1, 1, V, heads, d_head, ff) ? (size_t)sgn15_frames_floats(V, heads, d_head, ff) : 0;
}
extern "C" size_t agcn_sgn15_clip_weights(int seg, int num_class, int heads, int d_head, int ff) {
  return sgn15_clip_domain(1, seg, num_class, heads, d_head, ff)
             ? (size_t)sgn15_clip_w(seg, num_class, heads, d_head, ff).total : 0;
}

extern "C" int agcn_sgn15_frames(const float* x, const float* w, size_t w_floats, float* feat, float* attn, int N, int seg,
                                 int V, int heads, int d_head, int ff, void* stream) {
  if (!x || !w || !feat) return AGCN_ERR_ARG;
  if (!sgn15_frames_domain(N, seg, V, heads, d_head, ff)) return AGCN_ERR_ARG;
  if (w_floats != (size_t)sgn15_frames_floats(V, heads, d_head, ff)) return AGCN_ERR_ARG;
  AGCN_NOTE_KERNEL("sgn15_frames_kernel<f32 mfma> V=%d heads=%dx%d ff=%d frames=%ld", V, heads, d_head, ff, (long)N * seg);
  return agcn_launch_big<sgn15_frames_kernel>(dim3((unsigned)((long)N * seg)), dim3(SGN_THREADS),
                                              (size_t)SGN15_LDS_FLOATS(SGN15_SPA_IN) * 4, (hipStream_t)stream, x, w, feat,
                                              attn, seg, V, heads, d_head, ff);
}

extern "C" int agcn_sgn15_clip(const float* feat, const float* w, size_t w_floats, float* logits, float* attn, int N,
                               int seg, int num_class, int heads, int d_head, int ff, void* stream) {
  if (!feat || !w || !logits) return AGCN_ERR_ARG;
  if (!sgn15_clip_domain(N, seg, num_class, heads, d_head, ff)) return AGCN_ERR_ARG;
  if (w_floats != (size_t)sgn15_clip_w(seg, num_class, heads, d_head, ff).total) return AGCN_ERR_ARG;
  AGCN_NOTE_KERNEL("sgn15_clip_kernel<f32 mfma> seg=%d heads=%dx%d ff=%d clips=%d", seg, heads, d_head, ff, N);
  return agcn_launch_big<sgn15_clip_kernel>(dim3((unsigned)N), dim3(SGN_THREADS),
                                            (size_t)SGN15_LDS_FLOATS(SGN15_SPA_OUT) * 4, (hipStream_t)stream, feat, w,
                                            logits, attn, seg, num_class, heads, d_head, ff);
}
