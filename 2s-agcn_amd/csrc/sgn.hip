// Fused eval-mode inference of the base SGN (reference model/architecture/sgn/archiv/sgn.py) and the sampler in front
// of it (reference feeders/loader.py::NTUDataLoaders.to_fix_length, equal-interval branch).  Three kernels:
//   sgn_frames_kernel   joint-level module, one workgroup per frame: dif, the two embeddings + spa1, the adaptive
//                       adjacency g = softmax(g1(x)^T g2(x)), three gcn_spa layers with their BatchNorm folded, the
//                       maximum over joints.  Activations stay in LDS, weights stream from global / L2.
//   sgn_clip_kernel     frame-level module + classifier, one workgroup per clip: + tem1, k = 3 temporal conv, 1x1 conv,
//                       maximum over frames, fc.
//   sgn_sample_kernel   null-row removal, two-body interleave, padding and the S interval draws as one gather.
// All products are exact-f32 MFMA (v_mfma_f32_32x32x2_f32) in every AGCN_GEMM mode: the work is launch- and latency-
// bound, the split modes would add range-scaling passes and buy nothing.  Every sum has a fixed order and no launch
// reads another frame's or clip's intermediate, so the outputs are bitwise reproducible and independent of the batch.
// Geometry and every offset: sgn_plan.h.
#include "agcn_common.h"
#include "sgn_plan.h"

// acc[i] += X (32 x K) . W[:, block wave + SGN_WAVES * i], i < NB: X in LDS (a = the lane's row and k parity), W in global
// memory with leading dimension ldb (b = the lane's column in block `wave`).  One A read feeds NB matrix products, and
// 16 weight loads are in flight per step whatever NB is.
template <int NB>
__device__ __forceinline__ void mma_w(const float* a, const float* __restrict__ b, int ldb, int K, f32x16 (&acc)[NB]) {
#pragma unroll 16 / NB
  for (int k = 0; k < K; k += 2) {
    const float av = a[k];
#pragma unroll
    for (int i = 0; i < NB; ++i) acc[i] = mfma32(av, b[(long)k * ldb + i * (SGN_WAVES * 32)], acc[i]);
  }
}

// Y (32 x N) = act(bias + X (32 x K) . W (K x N)); X in LDS (row stride xs), W in global memory, Y to LDS (row stride
// ys).  N = 32 * SGN_WAVES * NB (or 64 with NB = 1: two waves idle); wave w owns the 32-column blocks w, w + 4, ...
// MODE 0: Y = relu(.), 1: Y += relu(.), 2: Y = . (no activation)
template <int NB, int MODE>
__device__ __forceinline__ void gemm_w(const float* X, int xs, int K, const float* __restrict__ W,
                                       const float* __restrict__ bias, int N, float* Y, int ys) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  if (wave * 32 >= N) return;
  f32x16 acc[NB] = {};
  mma_w<NB>(X + r * xs + h, W + (long)h * N + wave * 32 + r, N, K, acc);
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int col = (wave + SGN_WAVES * i) * 32 + r;
    const float bv = bias[col];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      float* y = Y + mfma_row(j, h) * ys + col;
      const float v = MODE == 2 ? acc[i][j] + bv : fmaxf(acc[i][j] + bv, 0.f);
      *y = MODE == 1 ? *y + v : v;
    }
  }
}

// Y (32 x N) = G (32 x Kg) . X (Kg x N), all in LDS; G has row stride SGN_G_STRIDE and zero columns from V on
__device__ __forceinline__ void gemm_g(const float* G, int Kg, const float* X, int xs, int N, float* Y, int ys) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  for (int nb = wave; nb < N / 32; nb += SGN_WAVES) {
    const float* a = G + r * SGN_G_STRIDE + h;
    const float* b = X + h * xs + nb * 32 + r;
    f32x16 acc = {};
    for (int k = 0; k < Kg; k += 2) acc = mfma32(a[k], b[k * xs], acc);
#pragma unroll
    for (int j = 0; j < 16; ++j) Y[mfma_row(j, h) * ys + nb * 32 + r] = acc[j];
  }
}

// out[col] = max over the rows < nrows of relu(bias + acc): the tile is never stored.  Every candidate is >= 0 after the
// ReLU and row 0 is always a real row, so 0 is the neutral element.
template <int NB>
__device__ __forceinline__ void rowmax(const f32x16 (&acc)[NB], const float* __restrict__ bias, int nrows, float (&m)[NB]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const float bv = bias[(wave + SGN_WAVES * i) * 32 + r];
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (mfma_row(j, h) < nrows) v = fmaxf(v, acc[i][j] + bv);
    m[i] = fmaxf(v, __shfl_xor(v, 32));
  }
}

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
  const int t = (int)(f % seg);
  const int tid = threadIdx.x;
  const int BS = SGN_BUF_STRIDE;

  // norm_data of the joints and of dif (reference sgn.py:73-75: dif is zero at t = 0, it never reads the clip before);
  // padded joint rows are zero
  if (tid < SGN_VP * 4) {
    const int v = tid >> 2, c = tid & 3;
    float a = 0.f, d = 0.f;
    if (v < V && c < 3) {
      const int e = v * 3 + c;
      const float cur = x[f * (V * 3) + e];
      const float dif = t > 0 ? cur - x[(f - 1) * (V * 3) + e] : 0.f;
      a = cur * w[o.aff + e] + w[o.aff + V * 3 + e];
      d = dif * w[o.aff + 2 * V * 3 + e] + w[o.aff + 3 * V * 3 + e];
    }
    xin[tid] = a;
    xin[SGN_VP * 4 + tid] = d;
  }
  __syncthreads();
  // first layers of the two embeddings (3 -> 64): bufB[:, 0:64] joint, bufB[:, 64:128] dif
  for (int i = tid; i < 2 * SGN_VP * SGN_C1; i += SGN_THREADS) {
    const int which = i / (SGN_VP * SGN_C1), v = (i / SGN_C1) % SGN_VP, c = i % SGN_C1;
    const float* wi = w + (which ? o.de1_w : o.je1_w);
    const float* xi = xin + which * SGN_VP * 4 + v * 4;
    float s = w[(which ? o.de1_b : o.je1_b) + c];
    s = fmaf(xi[0], wi[c], s);
    s = fmaf(xi[1], wi[SGN_C1 + c], s);
    s = fmaf(xi[2], wi[2 * SGN_C1 + c], s);
    bufB[v * BS + which * SGN_C1 + c] = fmaxf(s, 0.f);
  }
  // spa1 into the last 64 columns of x0 = [pos + dif | spa1] = bufA[:, 128:256]
  for (int i = tid; i < SGN_VP * SGN_C1; i += SGN_THREADS) {
    const int v = i / SGN_C1, c = i % SGN_C1;
    bufA[v * BS + SGN_C2 + SGN_C1 + c] = v < V ? w[o.spa1 + v * SGN_C1 + c] : 0.f;
  }
  __syncthreads();
  gemm_w<1, 0>(bufB, BS, SGN_C1, w + o.je2_w, w + o.je2_b, SGN_C1, bufA + SGN_C2, BS);
  __syncthreads();
  gemm_w<1, 1>(bufB + SGN_C1, BS, SGN_C1, w + o.de2_w, w + o.de2_b, SGN_C1, bufA + SGN_C2, BS);
  __syncthreads();

  // compute_g1 (reference sgn.py:206-211): [g1 | g2] (32 x 512) into bufB as one product, then g3 = g1 . g2^T with K
  // split over the waves
  gemm_w<4, 2>(bufA + SGN_C2, BS, SGN_C2, w + o.g_w, w + o.g_b, 2 * SGN_C3, bufB, BS);
  __syncthreads();
  {
    const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int k0 = wave * (SGN_C3 / SGN_WAVES);
    const float* a = bufB + r * BS + k0 + h;                 // g1[i = r][k]
    const float* b = bufB + SGN_C3 + r * BS + k0 + h;        // g2[j = r][k]
    f32x16 acc = {};
#pragma unroll 16
    for (int k = 0; k < SGN_C3 / SGN_WAVES; k += 2) acc = mfma32(a[k], b[k], acc);
#pragma unroll
    for (int j = 0; j < 16; ++j) part[(wave * SGN_VP + mfma_row(j, h)) * SGN_G_STRIDE + r] = acc[j];
  }
  __syncthreads();
  // softmax over the real joints j < V of every real row i < V, the row maximum subtracted; padded rows and columns of G
  // are zero, so they add nothing to g . x
  if (tid < SGN_VP) {
    const int i = tid;
    float s[SGN_VP];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < SGN_VP; ++j) {
      float v = part[i * SGN_G_STRIDE + j];
#pragma unroll
      for (int p = 1; p < SGN_WAVES; ++p) v += part[(p * SGN_VP + i) * SGN_G_STRIDE + j];
      s[j] = v;
      if (j < V) mx = fmaxf(mx, v);
    }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < SGN_VP; ++j) {
      s[j] = j < V ? expf(s[j] - mx) : 0.f;
      sum += s[j];
    }
    const float inv = 1.f / sum;
#pragma unroll
    for (int j = 0; j < SGN_VP; ++j) {
      const float p = i < V ? s[j] * inv : 0.f;
      G[i * SGN_G_STRIDE + j] = p;
      if (gout && i < V && j < V) gout[(f * V + i) * V + j] = p;
    }
  }
  __syncthreads();
  const int Kg = (V + 1) & ~1;
  // gcn1 (128 -> 128): [g . x0 | x0] = bufA[:, 0:256] -> x1 = bufB[:, 128:256]
  gemm_g(G, Kg, bufA + SGN_C2, BS, SGN_C2, bufA, BS);
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
    const int t0 = tile * SGN_VP;
    __syncthreads();
    // frames t0 - 1 .. t0 + 32 with tem1 added (reference sgn.py:89); frames outside the clip are the conv's zero padding
    for (int i = tid; i < (SGN_VP + 2) * SGN_C3; i += SGN_THREADS) {
      const int row = i / SGN_C3, c = i % SGN_C3, t = t0 - 1 + row;
      H[row * CS + c] = (t >= 0 && t < seg) ? feat[(n * seg + t) * SGN_C3 + c] + w[o.tem1 + t * SGN_C3 + c] : 0.f;
    }
    __syncthreads();
    // local.cnn1 + bn1 + relu (reference sgn.py:169-171): output row r reads rows r, r + 1, r + 2 of H
    const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    {
      f32x16 acc[2] = {};
      for (int dt = 0; dt < 3; ++dt)
        mma_w<2>(H + (r + dt) * CS + h, w + o.t1_w + ((long)dt * SGN_C3 + h) * SGN_C3 + wave * 32 + r, SGN_C3, SGN_C3, acc);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int col = (wave + SGN_WAVES * i) * 32 + r;
        const float bv = w[o.t1_b + col];
#pragma unroll
        for (int j = 0; j < 16; ++j) Y[mfma_row(j, h) * CS + col] = fmaxf(acc[i][j] + bv, 0.f);
      }
    }
    __syncthreads();
    // local.cnn2 + bn2 + relu and the running maximum over the frames of the clip
    {
      const int nrows = seg - t0 < SGN_VP ? seg - t0 : SGN_VP;
      f32x16 acc[4] = {};
      float m[4];
      mma_w<4>(Y + r * CS + h, w + o.t2_w + (long)h * SGN_C4 + wave * 32 + r, SGN_C4, SGN_C3, acc);
      rowmax<4>(acc, w + o.t2_b, nrows, m);
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
  __shared__ unsigned short rows[SGN_SAMPLE_MAX_ROWS];       // kept rows, (t << 1) | m, in (t, m) order
  __shared__ int scan[SGN_THREADS];
  __shared__ unsigned char flag[SGN_SAMPLE_MAX_ROWS];
  const long n = blockIdx.x;
  const int tid = threadIdx.x;
  const int nrows = 2 * T;
  // null flags: row (t, m) is kept iff any of its 3 V values is nonzero; rows dealt round-robin so that neighbouring
  // threads read neighbouring addresses
  for (int row = tid; row < nrows; row += SGN_THREADS) {
    const int t = row >> 1, m = row & 1;
    bool any = false;
    for (int c = 0; c < 3; ++c)
      for (int v = 0; v < V; ++v) any |= win[sgn_win_index(n, c, t, v, m, T, V)] != 0.f;
    flag[row] = any ? 1 : 0;
  }
  __syncthreads();
  // this thread compacts the SGN_SAMPLE_CHUNK consecutive rows from tid * SGN_SAMPLE_CHUNK on
  unsigned keep = 0;
  for (int i = 0; i < SGN_SAMPLE_CHUNK; ++i) {
    const int row = tid * SGN_SAMPLE_CHUNK + i;
    if (row < nrows && flag[row]) keep |= 1u << i;
  }
  // exclusive prefix sum of the kept counts over the threads (Hillis-Steele in LDS)
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
