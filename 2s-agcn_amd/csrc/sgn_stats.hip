// Batch statistics of SGN's seven BatchNorms (the forward half of train-mode BatchNorm; reference sgn.py:110-117 norm_data,
// 183-194 gcn_spa, 161-175 local, each nn.BatchNorm in training mode).  BatchNorm k sees activations normalised by the
// batch statistics of every BatchNorm in front of it, so the statistics come from sequential passes.  A pass is the fused
// forward of sgn.hip cut off at one BatchNorm: it runs on a folded weight image in which every earlier BatchNorm carries
// its batch statistics and the one under measurement is the identity, and its epilogue (colstats, sgn_device.h) reduces
// the pre-BatchNorm values straight from the accumulators.
//   sgn_input_stats_kernel       one workgroup per clip: x and dif per feature over the seg frames
//   sgn_frames_stats_kernel<L>   one workgroup per frame, sgn_frames_kernel's LDS carve and stages up to gcn<L>'s product
//   sgn_clip_stats_kernel<L>     one workgroup per clip, sgn_clip_kernel's tile loop up to cnn<L>'s product
//   sgn_stats_clip_merge_kernel  one thread per (clip, channel) merges the clip's groups in ascending order (fp64 state)
//   sgn_stats_finalize_kernel    one thread per channel merges the clips in ascending order on top of the carry state
//                                (both in sgn_stats_device.h, shared with sgn_v15_stats.hip)
// Every group emits (sum, M2 about its own mean); E[z^2] - mean^2 is never formed.  Exact-f32 MFMA in every AGCN_GEMM mode,
// fixed summation orders, no atomics, no launch reads another launch's LDS: a group's partials are the same bits alone
// and inside any batch, and a batch merged chunk by chunk through the carry state equals one launch bit for bit.
// Geometry: sgn_stats_plan.h.  The stages: sgn_device.h, shared with sgn.hip and sgn_bwd.hip.
#include "agcn_common.h"
#include "sgn_plan.h"
#include "sgn_stats_plan.h"
#include "sgn_device.h"
#include "sgn_stats_device.h"

__global__ __launch_bounds__(SGN_THREADS) void sgn_input_stats_kernel(const float* __restrict__ x, float* __restrict__ part,
                                                                      int seg, int V) {
  const int F = V * 3, C = 2 * F;
  const long n = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid >= C) return;
  const int which = tid >= F, e = which ? tid - F : tid;
  // two sweeps over the seg frames of the clip: the sum, then the squares about the clip's own mean
  float s = 0.f;
  for (int t = 0; t < seg; ++t) {
    const long f = n * seg + t, prev = sgn_dif_prev(f, seg);
    const float cur = x[f * F + e];
    s += which ? (prev >= 0 ? cur - x[prev * F + e] : 0.f) : cur;
  }
  const float mean = s / (float)seg;
  float q = 0.f;
  for (int t = 0; t < seg; ++t) {
    const long f = n * seg + t, prev = sgn_dif_prev(f, seg);
    const float cur = x[f * F + e];
    const float d = (which ? (prev >= 0 ? cur - x[prev * F + e] : 0.f) : cur) - mean;
    q = fmaf(d, d, q);
  }
  part[sgn_stats_part_index(n, 0, tid, C)] = s;
  part[sgn_stats_part_index(n, 1, tid, C)] = q;
}

// the columns this lane owns of an NB-block product -> the group's two rows of the partial buffer
template <int NB>
__device__ __forceinline__ void stats_store(const float (&sum)[NB], const float (&m2)[NB], float* __restrict__ part, long g,
                                            int C) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  if (h == 0)
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int col = (wave + SGN_WAVES * i) * 32 + r;
      part[sgn_stats_part_index(g, 0, col, C)] = sum[i];
      part[sgn_stats_part_index(g, 1, col, C)] = m2[i];
    }
}

template <int LAYER>
__global__ __launch_bounds__(SGN_THREADS) void sgn_frames_stats_kernel(const float* __restrict__ x,
                                                                       const float* __restrict__ w,
                                                                       float* __restrict__ part, int seg, int V) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* bufA = lds + SGN_LDS_BUF_A;
  float* bufB = lds + SGN_LDS_BUF_B;
  float* pr = lds + SGN_LDS_PART;
  float* G = lds + SGN_LDS_G;
  float* xin = lds + SGN_LDS_XIN;
  const SgnFramesW o = sgn_frames_w(V);
  const long f = blockIdx.x;                     // frame n * seg + t = the group
  const int tid = threadIdx.x;
  const int BS = SGN_BUF_STRIDE;
  const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  float* X0 = bufA + SGN_C2;

  // sgn_frames_kernel up to gcn<LAYER>'s product, call for call
  sgn_norm_input(x, w, o, f, seg, V, xin);
  __syncthreads();
  sgn_embed_first(xin, w, o, bufB, BS);
  sgn_fill_spa1(w, o, V, X0, BS);
  __syncthreads();
  sgn_embed_second(bufB, BS, w, o, X0, BS);
  __syncthreads();
  sgn_adjacency(X0, BS, w, o, bufB, BS, pr, SGN_VP * SGN_G_STRIDE, SGN_G_STRIDE, G, nullptr, V);
  __syncthreads();
  const int Kg = (V + 1) & ~1;
  gemm_g(G, Kg, X0, BS, SGN_C2, bufA, BS);
  __syncthreads();
  if constexpr (LAYER == 1) {
    // gemm_w<1, .>'s product (128 columns: one block per wave), the statistics instead of the store
    f32x16 acc[1] = {};
    float s[1], q[1];
    mma_w<1>(bufA + r * BS + h, w + o.c1_w + (long)h * SGN_C2 + wave * 32 + r, SGN_C2, 2 * SGN_C2, acc);
    colstats<1>(acc, w + o.c1_b, V, s, q);
    stats_store<1>(s, q, part, f, SGN_C2);
    return;
  }
  gemm_w<1, 0>(bufA, BS, 2 * SGN_C2, w + o.c1_w, w + o.c1_b, SGN_C2, bufB + SGN_C2, BS);
  __syncthreads();
  gemm_g(G, Kg, bufB + SGN_C2, BS, SGN_C2, bufB, BS);
  __syncthreads();
  if constexpr (LAYER == 2) {
    f32x16 acc[2] = {};
    float s[2], q[2];
    mma_w<2>(bufB + r * BS + h, w + o.c2_w + (long)h * SGN_C3 + wave * 32 + r, SGN_C3, 2 * SGN_C2, acc);
    colstats<2>(acc, w + o.c2_b, V, s, q);
    stats_store<2>(s, q, part, f, SGN_C3);
    return;
  }
  gemm_w<2, 0>(bufB, BS, 2 * SGN_C2, w + o.c2_w, w + o.c2_b, SGN_C3, bufA + SGN_C3, BS);
  __syncthreads();
  gemm_g(G, Kg, bufA + SGN_C3, BS, SGN_C3, bufA, BS);
  __syncthreads();
  {
    f32x16 acc[2] = {};
    float s[2], q[2];
    mma_w<2>(bufA + r * BS + h, w + o.c3_w + (long)h * SGN_C3 + wave * 32 + r, SGN_C3, 2 * SGN_C3, acc);
    colstats<2>(acc, w + o.c3_b, V, s, q);
    stats_store<2>(s, q, part, f, SGN_C3);
  }
}

template <int LAYER>
__global__ __launch_bounds__(SGN_THREADS) void sgn_clip_stats_kernel(const float* __restrict__ feat,
                                                                     const float* __restrict__ w,
                                                                     float* __restrict__ part, int seg, int num_class) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* H = lds + SGN_CLIP_LDS_H;
  float* Y = lds + SGN_CLIP_LDS_Y;
  const SgnClipW o = sgn_clip_w(seg, num_class);
  const long n = blockIdx.x;
  const int tid = threadIdx.x;
  const int CS = SGN_CLIP_STRIDE;
  const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int tiles = sgn_clip_tiles(seg);
  for (int tile = 0; tile < tiles; ++tile) {
    const int rows = sgn_tile_rows(tile, seg);
    const long g = n * tiles + tile;
    __syncthreads();
    sgn_clip_load_tile(feat, w, o, n, tile, seg, H);
    __syncthreads();
    if constexpr (LAYER == 1) {
      // sgn_clip_cnn1's product, the statistics instead of the store
      f32x16 acc[2] = {};
      float s[2], q[2];
      for (int dt = 0; dt < 3; ++dt)
        mma_w<2>(H + (r + dt) * CS + h, w + o.t1_w + ((long)dt * SGN_C3 + h) * SGN_C3 + wave * 32 + r, SGN_C3, SGN_C3, acc);
      colstats<2>(acc, w + o.t1_b, rows, s, q);
      stats_store<2>(s, q, part, g, SGN_C3);
    } else {
      sgn_clip_cnn1(H, w, o, Y);
      __syncthreads();
      f32x16 acc[4] = {};
      float s[4], q[4];
      mma_w<4>(Y + r * CS + h, w + o.t2_w + (long)h * SGN_C4 + wave * 32 + r, SGN_C4, SGN_C3, acc);
      colstats<4>(acc, w + o.t2_b, rows, s, q);
      stats_store<4>(s, q, part, g, SGN_C4);
    }
  }
}

// the base model's merge rule (sgn_stats_device.h): groups per clip and samples per group by the pass's kind
struct SgnStatsRule {
  int per, kind, seg, V;
  __device__ int count(long g) const { return sgn_stats_group_count(kind, g, seg, V); }
};

extern "C" size_t agcn_sgn_stats_part_floats(int kind, int layer, int N, int seg, int V) {
  if (kind == SGN_STATS_CLIP) V = 2;             // a clip pass does not depend on V
  return sgn_stats_domain(kind, layer, N, seg, V) ? (size_t)sgn_stats_part_floats(kind, layer, N, seg, V) : 0;
}
extern "C" size_t agcn_sgn_stats_channels(int kind, int layer, int V) {
  if (kind == SGN_STATS_CLIP) V = 2;
  return sgn_stats_domain(kind, layer, 1, 1, V) ? (size_t)sgn_stats_channels(kind, layer, V) : 0;
}

extern "C" int agcn_sgn_input_stats(const float* x, float* part, size_t part_floats, int N, int seg, int V, void* stream) {
  if (!x || !part) return AGCN_ERR_ARG;
  if (N < 1 || seg < 1 || V < 2 || V > SGN_MAX_V) return AGCN_ERR_ARG;
  if (!sgn_stats_domain(SGN_STATS_INPUT, 0, N, seg, V)) return AGCN_ERR_UNSUPPORTED;
  if (part_floats < (size_t)sgn_stats_part_floats(SGN_STATS_INPUT, 0, N, seg, V)) return AGCN_ERR_WORKSPACE;
  static_assert(2 * 3 * SGN_MAX_V <= SGN_THREADS, "agcn_sgn_input_stats: one thread per feature");
  AGCN_NOTE_KERNEL("sgn_input_stats_kernel V=%d clips=%d", V, N);
  hipLaunchKernelGGL(sgn_input_stats_kernel, dim3((unsigned)N), dim3(SGN_THREADS), 0, (hipStream_t)stream, x, part, seg, V);
  return agcn_check_launch();
}

extern "C" int agcn_sgn_frames_stats(const float* x, const float* w, size_t w_floats, float* part, size_t part_floats,
                                     int layer, int N, int seg, int V, void* stream) {
  if (!x || !w || !part) return AGCN_ERR_ARG;
  if (N < 1 || seg < 1 || V < 2 || V > SGN_MAX_V || !sgn_stats_layer_ok(SGN_STATS_FRAMES, layer)) return AGCN_ERR_ARG;
  if (!sgn_frames_domain(N, seg, V)) return AGCN_ERR_UNSUPPORTED;
  if (w_floats != (size_t)sgn_frames_w(V).total) return AGCN_ERR_ARG;
  if (part_floats < (size_t)sgn_stats_part_floats(SGN_STATS_FRAMES, layer, N, seg, V)) return AGCN_ERR_WORKSPACE;
  AGCN_NOTE_KERNEL("sgn_frames_stats_kernel<gcn%d, f32 mfma> V=%d frames=%ld", layer, V, (long)N * seg);
  const dim3 grid((unsigned)((long)N * seg)), block(SGN_THREADS);
  const size_t lds = (size_t)SGN_FRAMES_LDS_FLOATS * 4;
  hipStream_t s = (hipStream_t)stream;
  if (layer == 1) return agcn_launch_big<sgn_frames_stats_kernel<1>>(grid, block, lds, s, x, w, part, seg, V);
  if (layer == 2) return agcn_launch_big<sgn_frames_stats_kernel<2>>(grid, block, lds, s, x, w, part, seg, V);
  return agcn_launch_big<sgn_frames_stats_kernel<3>>(grid, block, lds, s, x, w, part, seg, V);
}

extern "C" int agcn_sgn_clip_stats(const float* feat, const float* w, size_t w_floats, float* part, size_t part_floats,
                                   int layer, int N, int seg, int num_class, void* stream) {
  if (!feat || !w || !part) return AGCN_ERR_ARG;
  if (N < 1 || seg < 1 || num_class < 1 || !sgn_stats_layer_ok(SGN_STATS_CLIP, layer)) return AGCN_ERR_ARG;
  if (!sgn_clip_domain(N, seg, num_class)) return AGCN_ERR_UNSUPPORTED;
  if (w_floats != (size_t)sgn_clip_w(seg, num_class).total) return AGCN_ERR_ARG;
  if (part_floats < (size_t)sgn_stats_part_floats(SGN_STATS_CLIP, layer, N, seg, 2)) return AGCN_ERR_WORKSPACE;
  AGCN_NOTE_KERNEL("sgn_clip_stats_kernel<cnn%d, f32 mfma> seg=%d clips=%d", layer, seg, N);
  const dim3 grid((unsigned)N), block(SGN_THREADS);
  const size_t lds = (size_t)SGN_CLIP_LDS_FLOATS * 4;
  hipStream_t s = (hipStream_t)stream;
  if (layer == 1) return agcn_launch_big<sgn_clip_stats_kernel<1>>(grid, block, lds, s, feat, w, part, seg, num_class);
  return agcn_launch_big<sgn_clip_stats_kernel<2>>(grid, block, lds, s, feat, w, part, seg, num_class);
}

extern "C" size_t agcn_sgn_stats_finalize_workspace(int kind, int layer, int N, int seg, int V) {
  if (kind == SGN_STATS_CLIP) V = 2;
  return sgn_stats_domain(kind, layer, N, seg, V) ? (size_t)sgn_stats_workspace_doubles(kind, layer, N, V) * 8 : 0;
}

extern "C" int agcn_sgn_stats_finalize(const float* part, size_t part_floats, int kind, int layer, int N, int seg, int V,
                                       const double* carry_in, double* carry_out, float* mean, float* var, void* ws,
                                       size_t ws_bytes, void* stream) {
  if (!part || !ws || (!carry_out && !(mean && var))) return AGCN_ERR_ARG;
  if (kind == SGN_STATS_CLIP) V = 2;
  if (N < 1 || seg < 1 || V < 2 || V > SGN_MAX_V || !sgn_stats_layer_ok(kind, layer)) return AGCN_ERR_ARG;
  if (!sgn_stats_domain(kind, layer, N, seg, V)) return AGCN_ERR_UNSUPPORTED;
  if (part_floats < (size_t)sgn_stats_part_floats(kind, layer, N, seg, V)) return AGCN_ERR_WORKSPACE;
  if (ws_bytes < (size_t)sgn_stats_workspace_doubles(kind, layer, N, V) * 8) return AGCN_ERR_WORKSPACE;
  const int C = sgn_stats_channels(kind, layer, V);
  const SgnStatsRule rule{sgn_stats_groups_per_clip(kind, seg), kind, seg, V};
  return sgn_stats_merge(part, (double*)ws, rule, C, (long)N, carry_in, carry_out, mean, var, (hipStream_t)stream);
}
