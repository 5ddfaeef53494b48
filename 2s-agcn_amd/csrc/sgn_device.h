// Device stages of the base SGN, written once: sgn.hip (inference) and sgn_bwd.hip (the backward, which recomputes the
// forward) call the same functions, so the recomputed forward is the forward by construction: same operation order on
// every accumulator, same bits, down to the arg-max that routes a gradient.  Each stage takes buffer pointers and row
// strides, so that the LDS carves of sgn_plan.h and sgn_bwd_plan.h both fit.  A stage holds a barrier only where its
// comment says so; the barrier behind a stage belongs to the caller.
#pragma once
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

// acc += A (32 x K) . B (K x 32), both in LDS with any strides: element (row, k) of A at a[row * ars + k * aks], element
// (k, col) of B at b[k * bks + col * bcs].  Transposed operands are a choice of strides.
__device__ __forceinline__ f32x16 mma_l(const float* a, int ars, int aks, const float* b, int bks, int bcs, int K,
                                        f32x16 acc) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  a += r * ars + h * aks;
  b += h * bks + r * bcs;
  for (int k = 0; k < K; k += 2) acc = mfma32(a[k * aks], b[k * bks], acc);
  return acc;
}

// Y[:, block wave + SGN_WAVES * i] = act(bias + acc[i]), Y in LDS (row stride ys).
// MODE 0: Y = relu(.), 1: Y += relu(.), 2: Y = . (no activation)
template <int NB, int MODE>
__device__ __forceinline__ void store_act(const f32x16 (&acc)[NB], const float* __restrict__ bias, float* Y, int ys) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
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

// Y (32 x N) = act(bias + X (32 x K) . W (K x N)); X in LDS (row stride xs), W in global memory, Y to LDS (row stride
// ys).  N = 32 * SGN_WAVES * NB (or 64 with NB = 1: two waves idle); wave w owns the 32-column blocks w, w + 4, ...
template <int NB, int MODE>
__device__ __forceinline__ void gemm_w(const float* X, int xs, int K, const float* __restrict__ W,
                                       const float* __restrict__ bias, int N, float* Y, int ys) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  if (wave * 32 >= N) return;
  f32x16 acc[NB] = {};
  mma_w<NB>(X + r * xs + h, W + (long)h * N + wave * 32 + r, N, K, acc);
  store_act<NB, MODE>(acc, bias, Y, ys);
}

// acc = [XA | XB] (32 x 2 Kh) . W (2 Kh x N): one product over [g.x | x] with its two halves in separate bands.  With
// XB = XA + Kh this is gemm_w's MFMA sequence on acc (k ascending), so the bits are.
template <int NB>
__device__ __forceinline__ void mma_cat(const float* XA, const float* XB, int xs, int Kh, const float* __restrict__ W,
                                        int N, f32x16 (&acc)[NB]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  mma_w<NB>(XA + r * xs + h, W + (long)h * N + wave * 32 + r, N, Kh, acc);
  mma_w<NB>(XB + r * xs + h, W + (long)(Kh + h) * N + wave * 32 + r, N, Kh, acc);
}

// Y (32 x N) = G (32 x Kg) . X (Kg x N), all in LDS; G has row stride SGN_G_STRIDE and zero columns from V on
__device__ __forceinline__ void gemm_g(const float* G, int Kg, const float* X, int xs, int N, float* Y, int ys) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  for (int nb = wave; nb < N / 32; nb += SGN_WAVES) {
    f32x16 acc = {};
    acc = mma_l(G, SGN_G_STRIDE, 1, X + nb * 32, xs, 1, Kg, acc);
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

// The batch-statistics epilogue, on the accumulators like rowmax: per column the sum over the rows < nrows (>= 1) of
// z = bias + acc and M2 = the sum of (z - sum / nrows)^2, in both lanes of the column; the tile is never stored.  Each
// half-wave adds its rows in ascending j, and the two halves combine as (rows of h = 0) + (rows of h = 1) in either lane.
template <int NB>
__device__ __forceinline__ void colstats(const f32x16 (&acc)[NB], const float* __restrict__ bias, int nrows, float (&sum)[NB],
                                         float (&m2)[NB]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const float bv = bias[(wave + SGN_WAVES * i) * 32 + r];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (mfma_row(j, h) < nrows) s += acc[i][j] + bv;
    const float so = __shfl_xor(s, 32);
    s = h == 0 ? s + so : so + s;
    const float mean = s / (float)nrows;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (mfma_row(j, h) < nrows) {
        const float d = acc[i][j] + bv - mean;
        q = fmaf(d, d, q);
      }
    const float qo = __shfl_xor(q, 32);
    sum[i] = s;
    m2[i] = h == 0 ? q + qo : qo + q;
  }
}

// colstats of a tile that sits in LDS (32 rows, odd row stride) instead of in accumulators: the calling thread owns
// column c and walks its rows < nrows (>= 1) in ascending order, twice, in fp32 -- the sum, then with mean = sum / nrows
// M2 = the sum of fmaf(d, d, .) about that mean; E[z^2] - mean^2 is formed nowhere.  Consecutive threads on consecutive
// columns read consecutive banks of one row.  Rows >= nrows are not read; the tile is not written.
__device__ __forceinline__ void colstats_lds(const float* tile, int stride, int c, int nrows, float& sum, float& m2) {
  float s = 0.f;
  for (int i = 0; i < nrows; ++i) s += tile[i * stride + c];
  const float mean = s / (float)nrows;
  float q = 0.f;
  for (int i = 0; i < nrows; ++i) {
    const float d = tile[i * stride + c] - mean;
    q = fmaf(d, d, q);
  }
  sum = s;
  m2 = q;
}

// rowmax with the index: best = the column's maximum of bv + acc over the rows < nrows where that is positive (else 0),
// arg = its row (else -1), in both lanes of the column.  Rows ascend with j and a strict > keeps the lowest index; the
// merge of the two half-waves keeps the lower row at a tie.
__device__ __forceinline__ void col_argmax(const f32x16& acc, float bv, int nrows, float& best, int& arg) {
  const int h = (threadIdx.x & 63) >> 5;
  best = 0.f;
  arg = -1;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int row = mfma_row(j, h);
    const float v = acc[j] + bv;
    if (row < nrows && v > best) {
      best = v;
      arg = row;
    }
  }
  const float ob = __shfl_xor(best, 32);
  const int oa = __shfl_xor(arg, 32);
  if (ob > best || (ob == best && oa >= 0 && oa < arg)) {
    best = ob;
    arg = oa;
  }
}

// ---- the joint-level module, frame f = n * seg + t ----

// norm_data of the joints and of dif (reference sgn.py:73-75: dif is zero at t = 0, it never reads the clip before) ->
// xin (2, SGN_VP, 4); padded joint rows are zero
__device__ __forceinline__ void sgn_norm_input(const float* __restrict__ x, const float* __restrict__ w,
                                               const SgnFramesW& o, long f, int seg, int V, float* xin) {
  const int tid = threadIdx.x, F = V * 3;
  if (tid < SGN_VP * 4) {
    const int v = tid >> 2, c = tid & 3;
    float a = 0.f, d = 0.f;
    if (v < V && c < 3) {
      const int e = v * 3 + c;
      const float cur = x[f * F + e];
      const long prev = sgn_dif_prev(f, seg);
      const float dif = prev >= 0 ? cur - x[prev * F + e] : 0.f;
      a = cur * w[o.aff + e] + w[o.aff + F + e];
      d = dif * w[o.aff + 2 * F + e] + w[o.aff + 3 * F + e];
    }
    xin[tid] = a;
    xin[SGN_VP * 4 + tid] = d;
  }
}

// first layers of the two embeddings (3 -> 64): E[:, 0:64] joint, E[:, 64:128] dif
__device__ __forceinline__ void sgn_embed_first(const float* xin, const float* __restrict__ w, const SgnFramesW& o, float* E,
                                                int es) {
  for (int i = threadIdx.x; i < 2 * SGN_VP * SGN_C1; i += SGN_THREADS) {
    const int which = i / (SGN_VP * SGN_C1), v = (i / SGN_C1) % SGN_VP, c = i % SGN_C1;
    const float* wi = w + (which ? o.de1_w : o.je1_w);
    const float* xi = xin + which * SGN_VP * 4 + v * 4;
    float s = w[(which ? o.de1_b : o.je1_b) + c];
    s = fmaf(xi[0], wi[c], s);
    s = fmaf(xi[1], wi[SGN_C1 + c], s);
    s = fmaf(xi[2], wi[2 * SGN_C1 + c], s);
    E[v * es + which * SGN_C1 + c] = fmaxf(s, 0.f);
  }
}

// spa1 into the last 64 columns of x0 = [pos + dif | spa1] (32 x 128)
__device__ __forceinline__ void sgn_fill_spa1(const float* __restrict__ w, const SgnFramesW& o, int V, float* X0, int xs) {
  for (int i = threadIdx.x; i < SGN_VP * SGN_C1; i += SGN_THREADS) {
    const int v = i / SGN_C1, c = i % SGN_C1;
    X0[v * xs + SGN_C1 + c] = v < V ? w[o.spa1 + v * SGN_C1 + c] : 0.f;
  }
}

// second layers of the two embeddings, added into the first 64 columns of x0; one barrier between the two
__device__ __forceinline__ void sgn_embed_second(const float* E, int es, const float* __restrict__ w, const SgnFramesW& o,
                                                 float* X0, int xs) {
  gemm_w<1, 0>(E, es, SGN_C1, w + o.je2_w, w + o.je2_b, SGN_C1, X0, xs);
  __syncthreads();
  gemm_w<1, 1>(E + SGN_C1, es, SGN_C1, w + o.de2_w, w + o.de2_b, SGN_C1, X0, xs);
}

// compute_g1 (reference sgn.py:206-211): [g1 | g2] (32 x 512) into GG as one product
__device__ __forceinline__ void sgn_g12(const float* X0, int xs, const float* __restrict__ w, const SgnFramesW& o, float* GG,
                                        int ggs) {
  gemm_w<4, 2>(X0, xs, SGN_C2, w + o.g_w, w + o.g_b, 2 * SGN_C3, GG, ggs);
}

// the adaptive adjacency G = softmax(g1 . g2^T): sgn_g12, the product with K split over the waves (the partial of wave p,
// row i, column j at part[p * pstride + i * rstride + j]), and the softmax over the real joints j < V of every real row
// i < V, the row maximum subtracted; padded rows and columns of G are zero, so they add nothing to g . x.  Two barriers
// inside.  gout: this frame's (V, V) block of the g output, or null.
__device__ __forceinline__ void sgn_adjacency(const float* X0, int xs, const float* __restrict__ w, const SgnFramesW& o,
                                              float* GG, int ggs, float* part, int pstride, int rstride, float* G,
                                              float* __restrict__ gout, int V) {
  const int tid = threadIdx.x;
  sgn_g12(X0, xs, w, o, GG, ggs);
  __syncthreads();
  {
    const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int k0 = wave * (SGN_C3 / SGN_WAVES);
    const float* a = GG + r * ggs + k0 + h;                  // g1[i = r][k]
    const float* b = GG + SGN_C3 + r * ggs + k0 + h;         // g2[j = r][k]
    f32x16 acc = {};
#pragma unroll 16
    for (int k = 0; k < SGN_C3 / SGN_WAVES; k += 2) acc = mfma32(a[k], b[k], acc);
#pragma unroll
    for (int j = 0; j < 16; ++j) part[wave * pstride + mfma_row(j, h) * rstride + r] = acc[j];
  }
  __syncthreads();
  if (tid < SGN_VP) {
    const int i = tid;
    float s[SGN_VP];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < SGN_VP; ++j) {
      float v = part[i * rstride + j];
#pragma unroll
      for (int p = 1; p < SGN_WAVES; ++p) v += part[p * pstride + i * rstride + j];
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
      if (gout && i < V && j < V) gout[i * V + j] = p;
    }
  }
}

// ---- the frame-level module, clip n ----

// rows 0..33 of H = frames 32 tile - 1 .. 32 tile + 32 with tem1 added (reference sgn.py:89); frames outside the clip
// are the conv's zero padding
__device__ __forceinline__ void sgn_clip_load_tile(const float* __restrict__ feat, const float* __restrict__ w,
                                                   const SgnClipW& o, long n, int tile, int seg, float* H) {
  for (int i = threadIdx.x; i < (SGN_VP + 2) * SGN_C3; i += SGN_THREADS) {
    const int row = i / SGN_C3, c = i % SGN_C3, t = sgn_tile_frame(tile, row, seg);
    H[row * SGN_CLIP_STRIDE + c] = t >= 0 ? feat[(n * seg + t) * SGN_C3 + c] + w[o.tem1 + t * SGN_C3 + c] : 0.f;
  }
}

// local.cnn1 + bn1 + relu (reference sgn.py:169-171): row r of Y reads rows r, r + 1, r + 2 of H
__device__ __forceinline__ void sgn_clip_cnn1(const float* H, const float* __restrict__ w, const SgnClipW& o, float* Y) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  f32x16 acc[2] = {};
  for (int dt = 0; dt < 3; ++dt)
    mma_w<2>(H + (r + dt) * SGN_CLIP_STRIDE + h, w + o.t1_w + ((long)dt * SGN_C3 + h) * SGN_C3 + wave * 32 + r, SGN_C3,
             SGN_C3, acc);
  store_act<2, 0>(acc, w + o.t1_b, Y, SGN_CLIP_STRIDE);
}

// ---- the sampler: the kept-row table of window n.  flag[row] = row (t, m) has a nonzero among its 3 V values; rows[] =
// the kept rows, (t << 1) | m, in (t, m) order; -> their number.  scan: SGN_THREADS ints.  Barriers inside, the last one
// behind the writes of rows[]. ----
__device__ __forceinline__ int sgn_kept_rows(const float* __restrict__ win, long n, int T, int V, unsigned char* flag,
                                             int* scan, unsigned short* rows) {
  const int tid = threadIdx.x;
  const int nrows = 2 * T;
  // rows dealt round-robin so that neighbouring threads read neighbouring addresses
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
  return kept;
}
