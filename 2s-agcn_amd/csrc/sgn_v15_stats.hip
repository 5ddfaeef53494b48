// Batch statistics of the four block BatchNorms of SGN v15 (the forward half of train-mode BatchNorm; reference
// model/layers/attention/crossattention.py::Transformer, pre-norm: PreNorm.norm of the attention, on the block's input x,
// and of the feed-forward, on x1 = attention + bo + x).  The two DataNorms in front are the base SGN's input pass
// (sgn_stats.hip::sgn_input_stats_kernel), the same [v*3 + c] computation.  BatchNorm k sees activations normalised by the
// batch statistics of every BatchNorm in front of it, so the statistics come from sequential passes.  A pass is the fused
// forward of sgn_v15.hip cut off at one BatchNorm, on a folded weight image in which every EARLIER BatchNorm carries its
// batch statistics; a pass never reads a section that depends on the BatchNorm it measures (sgn_v15_stats_plan.h).
//   sgn15_frames_stats_kernel<L>  one workgroup per frame, sgn15_frames_kernel's LDS carve and stages, call for call, up
//                                 to the complete token tile X = [pos + vel | spa] (L = 1, n_a) and on through the
//                                 attention half of the block (sgn15_block_x1) to x1 in place in X (L = 2, n_f)
//   sgn15_clip_stats_kernel<L>    one workgroup per clip, sgn15_clip_kernel's load of feat + tem (L = 1) and the attention
//                                 half (L = 2)
// The measured values are the LDS tile itself: thread c owns column c (colstats_lds, sgn_device.h), over the REAL rows
// only -- padded rows hold bias garbage in the frames kernel and zeros in the clip kernel -- and the tile is never stored.
// Every group emits (sum, M2 about its own mean); E[z^2] - mean^2 is never formed.  Exact-f32 MFMA in every AGCN_GEMM mode,
// fixed summation orders, no atomics, no launch reads another launch's LDS: a group's partials are the same bits alone
// and inside any batch, and a batch merged chunk by chunk through the carry state equals one launch bit for bit.  The
// merge is the base model's (sgn_stats_device.h) with this model's group rule.
#include "agcn_common.h"
#include "sgn_v15_plan.h"
#include "sgn_v15_stats_plan.h"
#include "sgn_v15_device.h"
#include "sgn_stats_device.h"

// column threadIdx.x of the (32, DIN + 1) tile over its rows < nrows -> the group's two rows of the partial buffer
template <int DIN>
__device__ __forceinline__ void sgn15_stats_store(const float* X, int nrows, float* __restrict__ part, long g) {
  static_assert(DIN <= SGN_THREADS, "one thread per column");
  const int c = threadIdx.x;
  if (c >= DIN) return;
  float s, q;
  colstats_lds(X, SGN15_X_STRIDE(DIN), c, nrows, s, q);
  part[sgn_stats_part_index(g, 0, c, DIN)] = s;
  part[sgn_stats_part_index(g, 1, c, DIN)] = q;
}

template <int LAYER>
__global__ __launch_bounds__(SGN_THREADS) void sgn15_frames_stats_kernel(const float* __restrict__ x,
                                                                         const float* __restrict__ w,
                                                                         float* __restrict__ part, int seg, int V,
                                                                         int heads, int d_head, int ff) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int DIN = SGN15_SPA_IN, DOUT = SGN15_SPA_OUT, XS = SGN15_X_STRIDE(DIN);
  float* X = lds + SGN15_LDS_X;
  float* QKV = lds + SGN15_LDS_QKV(DIN);
  float* P = lds + SGN15_LDS_P(DIN);
  float* xin = lds + SGN15_LDS_MISC(DIN);
  const SgnFramesW o = sgn_frames_w(V);
  const long f = blockIdx.x;                     // frame n * seg + t = the group

  // sgn15_frames_kernel up to the block, call for call
  sgn_norm_input(x, w, o, f, seg, V, xin);
  __syncthreads();
  sgn_embed_first(xin, w, o, QKV, SGN15_QKV_STRIDE);
  sgn_fill_spa1(w, o, V, X, XS);
  __syncthreads();
  sgn_embed_second(QKV, SGN15_QKV_STRIDE, w, o, X, XS);
  __syncthreads();
  if constexpr (LAYER == 2) {
    const Sgn15BlockW b = sgn15_block_w(sgn15_frames_block_base(V), DIN, DOUT, heads, d_head, ff);
    sgn15_block_x1<DIN, DOUT>(X, QKV, P, w, b, V, heads, d_head);        // leaves a barrier behind x1
  }
  sgn15_stats_store<DIN>(X, V, part, f);
}

template <int LAYER>
__global__ __launch_bounds__(SGN_THREADS) void sgn15_clip_stats_kernel(const float* __restrict__ feat,
                                                                       const float* __restrict__ w,
                                                                       float* __restrict__ part, int seg, int num_class,
                                                                       int heads, int d_head, int ff) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int DIN = SGN15_SPA_OUT, DOUT = SGN15_TEM_OUT, XS = SGN15_X_STRIDE(DIN);
  float* X = lds + SGN15_LDS_X;
  float* QKV = lds + SGN15_LDS_QKV(DIN);
  float* P = lds + SGN15_LDS_P(DIN);
  const Sgn15ClipW o = sgn15_clip_w(seg, num_class, heads, d_head, ff);
  const long n = blockIdx.x;                     // the clip = the group
  const int tid = threadIdx.x;
  // sgn15_clip_kernel's load: the frames of the clip with tem added, padded frame rows zero
  for (int i = tid; i < SGN_VP * DIN; i += SGN_THREADS) {
    const int t = i / DIN, c = i % DIN;
    X[t * XS + c] = t < seg ? feat[(n * seg + t) * DIN + c] + w[o.tem + (long)t * DIN + c] : 0.f;
  }
  __syncthreads();
  if constexpr (LAYER == 2) sgn15_block_x1<DIN, DOUT>(X, QKV, P, w, o.blk, seg, heads, d_head);
  sgn15_stats_store<DIN>(X, seg, part, n);
}

// this model's merge rule (sgn_stats_device.h): every group of a pass stands for the same number of samples
struct Sgn15StatsRule {
  int per, cnt;
  __device__ int count(long) const { return cnt; }
};

extern "C" size_t agcn_sgn15_stats_part_floats(int kind, int layer, int N, int seg, int V) {
  if (kind == SGN15_STATS_CLIP) V = 2;           // a clip pass does not depend on V
  return sgn15_stats_shape_domain(kind, layer, N, seg, V) ? (size_t)sgn15_stats_part_floats(kind, N, seg) : 0;
}
extern "C" size_t agcn_sgn15_stats_channels(int kind, int layer) {
  return sgn15_stats_layer_ok(kind, layer) ? (size_t)sgn15_stats_channels(kind) : 0;
}
extern "C" size_t agcn_sgn15_stats_finalize_workspace(int kind, int layer, int N, int seg, int V) {
  if (kind == SGN15_STATS_CLIP) V = 2;
  return sgn15_stats_shape_domain(kind, layer, N, seg, V) ? (size_t)sgn15_stats_workspace_doubles(kind, N) * 8 : 0;
}

extern "C" int agcn_sgn15_frames_stats(const float* x, const float* w, size_t w_floats, float* part, size_t part_floats,
                                       int layer, int N, int seg, int V, int heads, int d_head, int ff, void* stream) {
  if (!x || !w || !part) return AGCN_ERR_ARG;
  if (N < 1 || seg < 1 || V < 2 || V > SGN_MAX_V || !sgn15_stats_layer_ok(SGN15_STATS_FRAMES, layer)) return AGCN_ERR_ARG;
  if (!sgn15_stats_domain(SGN15_STATS_FRAMES, layer, N, seg, V, heads, d_head, ff)) return AGCN_ERR_UNSUPPORTED;
  if (w_floats != (size_t)sgn15_frames_floats(V, heads, d_head, ff)) return AGCN_ERR_ARG;
  if (part_floats < (size_t)sgn15_stats_part_floats(SGN15_STATS_FRAMES, N, seg)) return AGCN_ERR_WORKSPACE;
  AGCN_NOTE_KERNEL("sgn15_frames_stats_kernel<n%c, f32 mfma> V=%d heads=%dx%d frames=%ld", layer == 1 ? 'a' : 'f', V, heads,
                   d_head, (long)N * seg);
  const dim3 grid((unsigned)((long)N * seg)), block(SGN_THREADS);
  const size_t lds = (size_t)SGN15_LDS_FLOATS(SGN15_SPA_IN) * 4;
  hipStream_t s = (hipStream_t)stream;
  if (layer == 1) return agcn_launch_big<sgn15_frames_stats_kernel<1>>(grid, block, lds, s, x, w, part, seg, V, heads, d_head, ff);
  return agcn_launch_big<sgn15_frames_stats_kernel<2>>(grid, block, lds, s, x, w, part, seg, V, heads, d_head, ff);
}

extern "C" int agcn_sgn15_clip_stats(const float* feat, const float* w, size_t w_floats, float* part, size_t part_floats,
                                     int layer, int N, int seg, int num_class, int heads, int d_head, int ff, void* stream) {
  if (!feat || !w || !part) return AGCN_ERR_ARG;
  if (N < 1 || seg < 1 || num_class < 1 || !sgn15_stats_layer_ok(SGN15_STATS_CLIP, layer)) return AGCN_ERR_ARG;
  if (!sgn15_clip_domain(N, seg, num_class, heads, d_head, ff)) return AGCN_ERR_UNSUPPORTED;
  if (w_floats != (size_t)sgn15_clip_w(seg, num_class, heads, d_head, ff).total) return AGCN_ERR_ARG;
  if (part_floats < (size_t)sgn15_stats_part_floats(SGN15_STATS_CLIP, N, seg)) return AGCN_ERR_WORKSPACE;
  AGCN_NOTE_KERNEL("sgn15_clip_stats_kernel<n%c, f32 mfma> seg=%d heads=%dx%d clips=%d", layer == 1 ? 'a' : 'f', seg, heads,
                   d_head, N);
  const dim3 grid((unsigned)N), block(SGN_THREADS);
  const size_t lds = (size_t)SGN15_LDS_FLOATS(SGN15_SPA_OUT) * 4;
  hipStream_t s = (hipStream_t)stream;
  if (layer == 1)
    return agcn_launch_big<sgn15_clip_stats_kernel<1>>(grid, block, lds, s, feat, w, part, seg, num_class, heads, d_head, ff);
  return agcn_launch_big<sgn15_clip_stats_kernel<2>>(grid, block, lds, s, feat, w, part, seg, num_class, heads, d_head, ff);
}

extern "C" int agcn_sgn15_stats_finalize(const float* part, size_t part_floats, int kind, int layer, int N, int seg, int V,
                                         const double* carry_in, double* carry_out, float* mean, float* var, void* ws,
                                         size_t ws_bytes, void* stream) {
  if (!part || !ws || (!carry_out && !(mean && var))) return AGCN_ERR_ARG;
  if (kind == SGN15_STATS_CLIP) V = 2;
  if (N < 1 || seg < 1 || V < 2 || V > SGN_MAX_V || !sgn15_stats_layer_ok(kind, layer)) return AGCN_ERR_ARG;
  if (!sgn15_stats_shape_domain(kind, layer, N, seg, V)) return AGCN_ERR_UNSUPPORTED;
  if (part_floats < (size_t)sgn15_stats_part_floats(kind, N, seg)) return AGCN_ERR_WORKSPACE;
  if (ws_bytes < (size_t)sgn15_stats_workspace_doubles(kind, N) * 8) return AGCN_ERR_WORKSPACE;
  const Sgn15StatsRule rule{sgn15_stats_groups_per_clip(kind, seg), sgn15_stats_group_count(kind, seg, V)};
  return sgn_stats_merge(part, (double*)ws, rule, sgn15_stats_channels(kind), (long)N, carry_in, carry_out, mean, var,
                         (hipStream_t)stream);
}
