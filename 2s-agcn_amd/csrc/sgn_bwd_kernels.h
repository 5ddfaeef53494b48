// Device code of the SGN eval-mode backward, shared by sgn_bwd.hip (input gradients: the TAPE = false instantiations) and
// sgn_wgrad.hip (parameter gradients: TAPE = true).  A taping instantiation computes what the untaped one computes, with
// the same operation order (dx and dfeat are the same bits), and copies every operand pair of a weight gradient from LDS
// to a caller-owned tape at the step it is live (sgn_bwd_plan.h: SGN_BWD_LIVES, layout: sgn_wgrad_plan.h); it also
// finishes columns 64..127 of d x0 (the spa1 half), which the input gradient does not need.
#pragma once
#include "agcn_common.h"
#include "sgn_wgrad_plan.h"

// rows [0, nrows) x width columns of an LDS band -> the tape, consecutive threads on consecutive columns.  Only reads LDS:
// it may run next to readers of the band, between the barrier behind its producer and the one in front of its next writer.
__device__ __forceinline__ void tape_band(const float* band, int stride, int nrows, int width, float* dst, size_t ld) {
  for (int i = threadIdx.x; i < nrows * width; i += SGN_THREADS) {
    const int row = i / width, c = i - row * width;
    dst[(size_t)row * ld + c] = band[row * stride + c];
  }
}

// acc[i] += X (32 x K) . W[:, block wave + SGN_WAVES * i]: X in LDS, W in global memory (sgn.hip::mma_w)
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

// Y (32 x N) = act(bias + X . W), sgn.hip::gemm_w with its operation order.  MODE 0: relu, 1: += relu, 2: no activation
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

// acc = [XA | XB] (32 x 2 Kh) . W (2 Kh x N): the forward's one product over [g.x | x], its two halves in separate bands;
// the MFMA sequence on acc is the forward's (k ascending), so the bits are
template <int NB>
__device__ __forceinline__ void mma_cat(const float* XA, const float* XB, int xs, int Kh, const float* __restrict__ W,
                                        int N, f32x16 (&acc)[NB]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  mma_w<NB>(XA + r * xs + h, W + (long)h * N + wave * 32 + r, N, Kh, acc);
  mma_w<NB>(XB + r * xs + h, W + (long)(Kh + h) * N + wave * 32 + r, N, Kh, acc);
}

// Y (32 x N) = G (32 x Kg) . X (Kg x N), all in LDS (sgn.hip::gemm_g)
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

// One layer of the gcn_spa backward.  dZ (32 x Cout, rows >= V zero) and x_l (32 x Cin) in LDS, WT = Wcat^T (Cout, 2 Cin):
//   T = dZ . WT[:, 0:Cin]  (= d(g.x));   dgacc += T[:, this wave's K quarter] . x_l^T;   acc = dZ . WT[:, Cin:] + G^T . T
// Two barriers inside; the caller stores acc (masked) after another one.  NB = Cin / 128.
template <int NB>
__device__ __forceinline__ void gcn_bwd(const float* dZ, int Cout, const float* xl, int Cin, const float* __restrict__ WT,
                                        const float* G, int Kg, float* T, f32x16& dgacc, f32x16 (&acc)[NB]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int BS = SGN_BWD_STRIDE;
  {
    f32x16 t[NB] = {};
    mma_w<NB>(dZ + r * BS + h, WT + (long)h * 2 * Cin + wave * 32 + r, 2 * Cin, Cout, t);
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int j = 0; j < 16; ++j) T[mfma_row(j, h) * BS + (wave + SGN_WAVES * i) * 32 + r] = t[i][j];
  }
  __syncthreads();
  const int kq = Cin / SGN_WAVES;
  dgacc = mma_l(T + wave * kq, BS, 1, xl + wave * kq, 1, BS, kq, dgacc);
  mma_w<NB>(dZ + r * BS + h, WT + (long)h * 2 * Cin + Cin + wave * 32 + r, 2 * Cin, Cout, acc);
#pragma unroll
  for (int i = 0; i < NB; ++i) acc[i] = mma_l(G, 1, SGN_G_STRIDE, T + (wave + SGN_WAVES * i) * 32, BS, 1, Kg, acc[i]);
  __syncthreads();
}

template <bool TAPE>
__global__ __launch_bounds__(SGN_THREADS) void sgn_frames_bwd_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ w,
                                                                     const float* __restrict__ wt,
                                                                     const float* __restrict__ dfeat,
                                                                     float* __restrict__ dj, float* __restrict__ dd,
                                                                     float* __restrict__ tape, int seg, int V) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* tile = lds + SGN_BWD_LDS_TILE;
  float* P = tile + SGN_BWD_P;
  float* T = tile + SGN_BWD_T;
  float* X2 = tile + SGN_BWD_X2;
  float* X1 = tile + SGN_BWD_X1;
  float* X0 = tile + SGN_BWD_X0;
  float* G = lds + SGN_BWD_LDS_G;
  float* DG = lds + SGN_BWD_LDS_DG;
  float* E1 = lds + SGN_BWD_LDS_E1;
  float* xin = lds + SGN_BWD_LDS_XIN;
  const SgnFramesW o = sgn_frames_w(V);
  const SgnFramesWT ot = sgn_frames_wt();
  const long f = blockIdx.x;                     // frame n * seg + t
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int BS = SGN_BWD_STRIDE, ES = SGN_BWD_E1_STRIDE, GS = SGN_G_STRIDE;
  const int F = V * 3;
  const int Kg = (V + 1) & ~1;
  // the taping instantiation: this frame's V rows of the tape and the column offsets of its sections
  const SgnFramesTape tp = sgn_frames_tape();
  const size_t TC = (size_t)tp.cols;
  float* trow = TAPE ? tape + sgn_frames_tape_row(f, 0, V) * TC : nullptr;

  // ---- the frame's forward, as sgn_frames_kernel computes it ----
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
  __syncthreads();
  for (int i = tid; i < 2 * SGN_VP * SGN_C1; i += SGN_THREADS) {
    const int which = i / (SGN_VP * SGN_C1), v = (i / SGN_C1) % SGN_VP, c = i % SGN_C1;
    const float* wi = w + (which ? o.de1_w : o.je1_w);
    const float* xi = xin + which * SGN_VP * 4 + v * 4;
    float s = w[(which ? o.de1_b : o.je1_b) + c];
    s = fmaf(xi[0], wi[c], s);
    s = fmaf(xi[1], wi[SGN_C1 + c], s);
    s = fmaf(xi[2], wi[2 * SGN_C1 + c], s);
    E1[v * ES + which * SGN_C1 + c] = fmaxf(s, 0.f);
  }
  for (int i = tid; i < SGN_VP * SGN_C1; i += SGN_THREADS) {
    const int v = i / SGN_C1, c = i % SGN_C1;
    X0[v * BS + SGN_C1 + c] = v < V ? w[o.spa1 + v * SGN_C1 + c] : 0.f;
  }
  __syncthreads();
  gemm_w<1, 0>(E1, ES, SGN_C1, w + o.je2_w, w + o.je2_b, SGN_C1, X0, BS);
  __syncthreads();
  gemm_w<1, 1>(E1 + SGN_C1, ES, SGN_C1, w + o.de2_w, w + o.de2_b, SGN_C1, X0, BS);
  __syncthreads();
  gemm_w<4, 2>(X0, BS, SGN_C2, w + o.g_w, w + o.g_b, 2 * SGN_C3, P, BS);          // [g1 | g2] = the P and T bands
  __syncthreads();
  {
    const int k0 = wave * (SGN_C3 / SGN_WAVES);
    f32x16 acc = {};
    const float* a = P + r * BS + k0 + h;
    const float* b = T + r * BS + k0 + h;
#pragma unroll 16
    for (int k = 0; k < SGN_C3 / SGN_WAVES; k += 2) acc = mfma32(a[k], b[k], acc);
#pragma unroll
    for (int j = 0; j < 16; ++j) X2[mfma_row(j, h) * BS + wave * SGN_BWD_PART_STRIDE + r] = acc[j];
  }
  __syncthreads();
  if (tid < SGN_VP) {
    const int i = tid;
    float s[SGN_VP];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < SGN_VP; ++j) {
      float v = X2[i * BS + j];
#pragma unroll
      for (int p = 1; p < SGN_WAVES; ++p) v += X2[i * BS + p * SGN_BWD_PART_STRIDE + j];
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
    for (int j = 0; j < SGN_VP; ++j) G[i * GS + j] = i < V ? s[j] * inv : 0.f;
  }
  __syncthreads();
  // gcn1: x1 = X1
  gemm_g(G, Kg, X0, BS, SGN_C2, T, BS);
  __syncthreads();
  if constexpr (TAPE) {
    tape_band(T, BS, V, SGN_C2, trow + tp.gx1, TC);
    tape_band(X0, BS, V, SGN_C2, trow + tp.x0, TC);
  }
  {
    f32x16 acc[1] = {};
    mma_cat<1>(T, X0, BS, SGN_C2, w + o.c1_w, SGN_C2, acc);
    const int col = wave * 32 + r;
    const float bv = w[o.c1_b + col];
#pragma unroll
    for (int j = 0; j < 16; ++j) X1[mfma_row(j, h) * BS + col] = fmaxf(acc[0][j] + bv, 0.f);
  }
  __syncthreads();
  // gcn2: x2 = X2
  gemm_g(G, Kg, X1, BS, SGN_C2, T, BS);
  __syncthreads();
  if constexpr (TAPE) {
    tape_band(T, BS, V, SGN_C2, trow + tp.gx2, TC);
    tape_band(X1, BS, V, SGN_C2, trow + tp.x1, TC);
  }
  {
    f32x16 acc[2] = {};
    mma_cat<2>(T, X1, BS, SGN_C2, w + o.c2_w, SGN_C3, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int col = (wave + SGN_WAVES * i) * 32 + r;
      const float bv = w[o.c2_b + col];
#pragma unroll
      for (int j = 0; j < 16; ++j) X2[mfma_row(j, h) * BS + col] = fmaxf(acc[i][j] + bv, 0.f);
    }
  }
  __syncthreads();
  // gcn3 and the maximum over the real joints: d z3 = d feat at the arg-max joint of a column whose maximum is positive
  gemm_g(G, Kg, X2, BS, SGN_C3, T, BS);
  __syncthreads();
  if constexpr (TAPE) {
    tape_band(T, BS, V, SGN_C3, trow + tp.gx3, TC);
    tape_band(X2, BS, V, SGN_C3, trow + tp.x2, TC);
  }
  {
    f32x16 acc[2] = {};
    mma_cat<2>(T, X2, BS, SGN_C3, w + o.c3_w, SGN_C3, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int col = (wave + SGN_WAVES * i) * 32 + r;
      const float bv = w[o.c3_b + col];
      float best = 0.f;
      int arg = -1;
#pragma unroll
      for (int j = 0; j < 16; ++j) {               // rows ascend with j: a strict > keeps the lowest index
        const int row = mfma_row(j, h);
        const float v = acc[i][j] + bv;
        if (row < V && v > best) {
          best = v;
          arg = row;
        }
      }
      const float ob = __shfl_xor(best, 32);
      const int oa = __shfl_xor(arg, 32);
      if (ob > best || (ob == best && oa >= 0 && oa < arg)) arg = oa;
      const float d = dfeat[f * SGN_C3 + col];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int row = mfma_row(j, h);
        P[row * BS + col] = row == arg ? d : 0.f;
      }
    }
  }
  __syncthreads();

  // ---- backward through gcn3, gcn2, gcn1; dG accumulates in registers, K split over the waves ----
  f32x16 dgacc = {};
  if constexpr (TAPE) tape_band(P, BS, V, SGN_C3, trow + tp.dz3, TC);
  {
    f32x16 acc[2] = {};
    gcn_bwd<2>(P, SGN_C3, X2, SGN_C3, wt + ot.c3, G, Kg, T, dgacc, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int row = mfma_row(j, h);
        float* p = X2 + row * BS + (wave + SGN_WAVES * i) * 32 + r;
        *p = (row < V && *p > 0.f) ? acc[i][j] : 0.f;
      }
  }
  __syncthreads();
  if constexpr (TAPE) tape_band(X2, BS, V, SGN_C3, trow + tp.dz2, TC);
  {
    f32x16 acc[1] = {};
    gcn_bwd<1>(X2, SGN_C3, X1, SGN_C2, wt + ot.c2, G, Kg, T, dgacc, acc);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int row = mfma_row(j, h);
      float* p = X1 + row * BS + wave * 32 + r;
      *p = (row < V && *p > 0.f) ? acc[0][j] : 0.f;
    }
  }
  __syncthreads();
  if constexpr (TAPE) tape_band(X1, BS, V, SGN_C2, trow + tp.dz1, TC);
  {
    f32x16 acc[1] = {};
    gcn_bwd<1>(X1, SGN_C2, X0, SGN_C2, wt + ot.c1, G, Kg, T, dgacc, acc);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int row = mfma_row(j, h);
      tile[row * BS + SGN_BWD_DX0 + wave * 32 + r] = row < V ? acc[0][j] : 0.f;
      P[row * BS + wave * SGN_BWD_PART_STRIDE + r] = dgacc[j];
    }
  }
  __syncthreads();
  // softmax backward over the real columns: dS = G * (dG - rowsum(G * dG)); padded rows and columns are zero
  if (tid < SGN_VP) {
    const int i = tid;
    float dg[SGN_VP];
    float rs = 0.f;
#pragma unroll
    for (int j = 0; j < SGN_VP; ++j) {
      float v = P[i * BS + j];
#pragma unroll
      for (int p = 1; p < SGN_WAVES; ++p) v += P[i * BS + p * SGN_BWD_PART_STRIDE + j];
      dg[j] = v;
      if (j < V) rs = fmaf(G[i * GS + j], v, rs);
    }
#pragma unroll
    for (int j = 0; j < SGN_VP; ++j) DG[i * GS + j] = (i < V && j < V) ? G[i * GS + j] * (dg[j] - rs) : 0.f;
  }
  __syncthreads();
  // g1 | g2 again, then d g1 = dS . g2 and d g2 = dS^T . g1, each taken to d x0 (its first 64 columns: the spa1 half is
  // input independent) before the next one overwrites it
  gemm_w<4, 2>(X0, BS, SGN_C2, w + o.g_w, w + o.g_b, 2 * SGN_C3, P, BS);
  __syncthreads();
  float* D12 = tile + SGN_BWD_DG12;
  f32x16 dx0[1] = {};
  for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c0 = (wave + SGN_WAVES * i) * 32;
      f32x16 acc = {};
      acc = pass == 0 ? mma_l(DG, GS, 1, T + c0, BS, 1, Kg, acc) : mma_l(DG, 1, GS, P + c0, BS, 1, Kg, acc);
#pragma unroll
      for (int j = 0; j < 16; ++j) D12[mfma_row(j, h) * BS + c0 + r] = acc[j];
    }
    __syncthreads();
    if constexpr (TAPE) tape_band(D12, BS, V, SGN_C3, trow + tp.dg + pass * SGN_C3, TC);
    if (TAPE || wave < 2)                          // waves 2, 3: columns 64..127 of d x0, the spa1 half
      mma_w<1>(D12 + r * BS + h, wt + ot.g + (long)(pass * SGN_C3 + h) * SGN_C2 + wave * 32 + r, SGN_C2, SGN_C3, dx0);
    __syncthreads();
  }
  // the second embedding layers again (P band), masked in place to d(their pre-activations)
  gemm_w<1, 0>(E1, ES, SGN_C1, w + o.je2_w, w + o.je2_b, SGN_C1, P, BS);
  gemm_w<1, 0>(E1 + SGN_C1, ES, SGN_C1, w + o.de2_w, w + o.de2_b, SGN_C1, P + SGN_C1, BS);
  if (wave < 2) {
    const int col = wave * 32 + r;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int row = mfma_row(j, h);
      const float d = dx0[0][j] + tile[row * BS + SGN_BWD_DX0 + col];
      float* p = P + row * BS + col;
      p[0] = (row < V && p[0] > 0.f) ? d : 0.f;
      p[SGN_C1] = (row < V && p[SGN_C1] > 0.f) ? d : 0.f;
    }
  } else if constexpr (TAPE) {
    const int col = wave * 32 + r;                 // 64..127: d x0 of the spa1 half, straight to the tape
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int row = mfma_row(j, h);
      if (row < V) trow[(size_t)row * TC + tp.dspa + col - SGN_C1] = dx0[0][j] + tile[row * BS + SGN_BWD_DX0 + col];
    }
  }
  __syncthreads();
  if constexpr (TAPE) {
    tape_band(E1, ES, V, SGN_C2, trow + tp.e1, TC);
    tape_band(P, BS, V, SGN_C2, trow + tp.de2, TC);
  }
  {
    const int br = wave >> 1, cb = wave & 1;       // waves 0, 1: joint branch, waves 2, 3: dif branch
    f32x16 acc = {};
    const float* a = P + br * SGN_C1 + r * BS + h;
    const float* b = wt + (br ? ot.de2 : ot.je2) + h * SGN_C1 + cb * 32 + r;
#pragma unroll 16
    for (int k = 0; k < SGN_C1; k += 2) acc = mfma32(a[k], b[k * SGN_C1], acc);
    const int col = br * SGN_C1 + cb * 32 + r;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int row = mfma_row(j, h);
      T[row * BS + col] = E1[row * ES + col] > 0.f ? acc[j] : 0.f;
    }
  }
  __syncthreads();
  if constexpr (TAPE) {
    tape_band(T, BS, V, SGN_C2, trow + tp.de1, TC);
    for (int i = tid; i < V * 8; i += SGN_THREADS)           // xn: (joint c0..c2, 0, dif c0..c2, 0) of joint i / 8
      trow[(size_t)(i >> 3) * TC + tp.xn + (i & 7)] = xin[((i >> 2) & 1) * SGN_VP * 4 + (i >> 3) * 4 + (i & 3)];
  }
  // 64 -> 3 and the folded norm_data scale; one thread per (branch, joint, coordinate), k ascending
  if (tid < 2 * SGN_VP * 3) {
    const int which = tid / (SGN_VP * 3), v = (tid / 3) % SGN_VP, c = tid % 3;
    if (v < V) {
      const float* wi = w + (which ? o.de1_w : o.je1_w) + c * SGN_C1;
      const float* d = T + v * BS + which * SGN_C1;
      float s = 0.f;
      for (int k = 0; k < SGN_C1; ++k) s = fmaf(d[k], wi[k], s);
      const int e = v * 3 + c;
      if constexpr (TAPE) trow[(size_t)v * TC + tp.dxn + which * 3 + c] = s;      // d xn, before the folded scale
      (which ? dd : dj)[f * F + e] = s * w[o.aff + (which ? 2 : 0) * F + e];
    }
  }
}

static __global__ __launch_bounds__(SGN_THREADS) void sgn_dif_combine_kernel(const float* __restrict__ dj,
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

template <bool TAPE>
__global__ __launch_bounds__(SGN_THREADS) void sgn_clip_bwd_kernel(const float* __restrict__ feat,
                                                                   const float* __restrict__ w,
                                                                   const float* __restrict__ wt,
                                                                   const float* __restrict__ dlogits, float* dfeat,
                                                                   float* __restrict__ tape, int seg, int num_class) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* H = lds + SGN_CLIP_LDS_H;               // pass 2: d Y1 with a zero row on either side, once Y1 exists
  float* Y = lds + SGN_CLIP_LDS_Y;
  float* ymax = lds + SGN_CLIP_LDS_MAX;          // the running maximum, then d ymax
  int* arg = reinterpret_cast<int*>(lds + SGN_CLIP_BWD_LDS_ARG);
  const SgnClipW o = sgn_clip_w(seg, num_class);
  const SgnClipWT ot = sgn_clip_wt();
  const long n = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int CS = SGN_CLIP_STRIDE;
  const int tiles = sgn_clip_tiles(seg);
  for (int i = tid; i < SGN_C4; i += SGN_THREADS) {
    ymax[i] = 0.f;
    arg[i] = -1;
  }
  const SgnClipTape tp = sgn_clip_tape(TAPE ? (long)gridDim.x : 0, seg);
  if constexpr (TAPE) {                            // the conv's zero padding: rows t = -1 and t = seg of this clip's H
    tape[tp.h + sgn_clip_tape_h_row(n, -1, seg) * SGN_C3 + tid] = 0.f;
    tape[tp.h + sgn_clip_tape_h_row(n, seg, seg) * SGN_C3 + tid] = 0.f;
  }
  for (int pass = 0; pass < 2; ++pass) {
    for (int tile = 0; tile < tiles; ++tile) {
      const int t0 = tile * SGN_VP, nrows = sgn_tile_rows(tile, seg);
      __syncthreads();
      for (int i = tid; i < (SGN_VP + 2) * SGN_C3; i += SGN_THREADS) {
        const int row = i / SGN_C3, c = i % SGN_C3, t = sgn_tile_frame(tile, row, seg);
        H[row * CS + c] = t >= 0 ? feat[(n * seg + t) * SGN_C3 + c] + w[o.tem1 + t * SGN_C3 + c] : 0.f;
      }
      __syncthreads();
      if constexpr (TAPE)
        if (pass == 1) {                           // the tile's own frames of H (rows 1..nrows), and d y2 of those frames
          tape_band(H + CS, CS, nrows, SGN_C3, tape + tp.h + sgn_clip_tape_h_row(n, t0, seg) * SGN_C3, SGN_C3);
          float* d2 = tape + tp.dy2 + (size_t)(n * seg + t0) * SGN_C4;
          for (int i = tid; i < nrows * SGN_C4; i += SGN_THREADS) {
            const int row = i / SGN_C4, k = i % SGN_C4;
            d2[i] = arg[k] == t0 + row ? ymax[k] : 0.f;
          }
        }
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
      if (pass == 0) {
        // y2 and the arg-max frame of every column: a strict > keeps the first frame, 0 is what a ReLU leaves
        f32x16 acc[4] = {};
        mma_w<4>(Y + r * CS + h, w + o.t2_w + (long)h * SGN_C4 + wave * 32 + r, SGN_C4, SGN_C3, acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int col = (wave + SGN_WAVES * i) * 32 + r;
          const float bv = w[o.t2_b + col];
          float best = 0.f;
          int a = -1;
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const int row = mfma_row(j, h);
            const float v = acc[i][j] + bv;
            if (row < nrows && v > best) {
              best = v;
              a = row;
            }
          }
          const float ob = __shfl_xor(best, 32);
          const int oa = __shfl_xor(a, 32);
          if (ob > best || (ob == best && oa >= 0 && oa < a)) {
            best = ob;
            a = oa;
          }
          if (h == 0 && best > ymax[col]) {         // a column is owned by the same lane in every tile
            ymax[col] = best;
            arg[col] = t0 + a;
          }
        }
        continue;
      }
      // d Y1 = (d y2 . W2^T) masked by Y1 > 0, where d y2 has one entry per column k, at its arg-max frame: thread c owns
      // column c of d Y1 and adds the rows of W2^T in the order of k
      if constexpr (TAPE) tape_band(Y, CS, nrows, SGN_C3, tape + tp.y1 + (size_t)(n * seg + t0) * SGN_C3, SGN_C3);
      {
        const int c = tid;
        for (int row = 0; row < SGN_VP + 2; ++row) H[row * CS + c] = 0.f;
        for (int k0 = 0; k0 < SGN_C4; k0 += 8) {       // eight rows of W2^T requested at once, used in the order of k
          float wv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) wv[u] = wt[ot.t2 + (k0 + u) * SGN_C3 + c];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int a = arg[k0 + u] - t0;
            if (a >= 0 && a < nrows) H[(a + 1) * CS + c] = fmaf(ymax[k0 + u], wv[u], H[(a + 1) * CS + c]);
          }
        }
        for (int row = 0; row < SGN_VP; ++row)
          if (!(Y[row * CS + c] > 0.f)) H[(row + 1) * CS + c] = 0.f;
      }
      __syncthreads();
      // d H[u] = sum over dt of d Y1[u + 1 - dt] . W1[dt]^T for the tile's own frames u: row u + 2 - dt of the padded d Y1
      if constexpr (TAPE) tape_band(H + CS, CS, nrows, SGN_C3, tape + tp.dy1 + (size_t)(n * seg + t0) * SGN_C3, SGN_C3);
      {
        f32x16 acc[2] = {};
        for (int dt = 0; dt < 3; ++dt)
          mma_w<2>(H + (r + 2 - dt) * CS + h, wt + ot.t1 + ((long)dt * SGN_C3 + h) * SGN_C3 + wave * 32 + r, SGN_C3, SGN_C3,
                   acc);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int col = (wave + SGN_WAVES * i) * 32 + r;
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const int row = mfma_row(j, h);
            if (row < nrows) {
              float* p = dfeat + (n * seg + t0 + row) * SGN_C3 + col;
              // the first frame of a later tile already holds what the tile before sent through its last frame's tap 2
              *p = (row == 0 && tile > 0) ? *p + acc[i][j] : acc[i][j];
            }
          }
        }
      }
      __syncthreads();
      // the two halo frames: owned by the neighbouring tiles, added in the order of the tiles
      {
        const int c = tid;
        const int lo = sgn_halo_lo(tile, seg), hi = sgn_halo_hi(tile, seg);
        if (lo >= 0) {
          float s = 0.f;
          for (int k = 0; k < SGN_C3; ++k) s = fmaf(H[1 * CS + k], wt[ot.t1 + (long)k * SGN_C3 + c], s);
          dfeat[(n * seg + lo) * SGN_C3 + c] += s;
        }
        if (hi >= 0) {
          float s = 0.f;
          for (int k = 0; k < SGN_C3; ++k)
            s = fmaf(H[SGN_VP * CS + k], wt[ot.t1 + ((long)2 * SGN_C3 + k) * SGN_C3 + c], s);
          dfeat[(n * seg + hi) * SGN_C3 + c] = s;
        }
      }
    }
    if (pass == 0) {
      // d ymax = d logits . Wfc^T, only where a frame was chosen (a maximum of 0 passes nothing)
      __syncthreads();
      for (int k = tid; k < SGN_C4; k += SGN_THREADS) {
        if constexpr (TAPE) tape[tp.ymax + (size_t)n * SGN_C4 + k] = ymax[k];      // the forward's maximum, before d ymax
        float s = 0.f;
        for (int c = 0; c < num_class; ++c) s = fmaf(dlogits[n * num_class + c], w[o.fc_w + (long)k * num_class + c], s);
        ymax[k] = arg[k] >= 0 ? s : 0.f;
      }
    }
  }
}
