// The backward of the base SGN in eval mode (the backward of sgn.hip) and the adjoint of the sampler.  Four kernels:
//   sgn_clip_bwd_kernel     d logits -> d feat, one workgroup per clip: recomputes H = feat + tem1, Y1, y2 and the arg-max
//                           frame of every column (pass 1), then goes back tile by tile through fc, the maximum, the 1x1
//                           conv and the 3-tap conv (pass 2).
//   sgn_frames_bwd_kernel   d feat -> dj, dd (gradients of the joint and the dif branch, workspace), one workgroup per
//                           frame: recomputes the frame's forward, then the maximum over joints, the three gcn_spa, the
//                           softmax, g1 / g2 and the two embeddings.
//   sgn_dif_combine_kernel  dx[t] = dj[t] + dd[t] [t > 0] - dd[t + 1] [t + 1 < seg]: the dif coupling, inside a clip.
//   sgn_sample_bwd_kernel   d out -> d win, the adjoint of the gather, one workgroup per window.
// The first two are templates on bool TAPE.  TAPE = false gives the input gradients alone.  A taping instantiation
// computes what the untaped one computes, with the same operation order (dx and dfeat are the same bits), and copies
// every operand pair of a weight gradient from LDS to a caller-owned tape at the step it is live (sgn_bwd_plan.h:
// SGN_BWD_LIVES, layout: sgn_wgrad_plan.h) for the reductions of sgn_wgrad.hip; it also finishes columns 64..127 of d x0
// (the spa1 half), which the input gradient does not need.
// The recomputed forward is the forward's own code: the stages of sgn_device.h, which sgn.hip calls too.
// Arithmetic as in the forward: exact-f32 MFMA (v_mfma_f32_32x32x2_f32) in every AGCN_GEMM mode, every sum in a fixed
// order, no atomics, no launch reads another clip's intermediates: a clip's dx is the same bits alone and in any batch.
// ReLU's derivative at 0 is 0; a maximum routes to its lowest index (ties only happen at 0, where nothing flows).
// Geometry, the LDS carve and every guarded index: sgn_bwd_plan.h.
#include "agcn_common.h"
#include "sgn_wgrad_plan.h"
#include "sgn_device.h"

// rows [0, nrows) x width columns of an LDS band -> the tape, consecutive threads on consecutive columns.  Only reads LDS:
// it may run next to readers of the band, between the barrier behind its producer and the one in front of its next writer.
__device__ __forceinline__ void tape_band(const float* band, int stride, int nrows, int width, float* dst, size_t ld) {
  for (int i = threadIdx.x; i < nrows * width; i += SGN_THREADS) {
    const int row = i / width, c = i - row * width;
    dst[(size_t)row * ld + c] = band[row * stride + c];
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

  // ---- the frame's forward: the stages of sgn_frames_kernel on this carve.  [g1 | g2] = the P and T bands, the K-split
  // partials of g1 . g2^T in the X2 band of their row ----
  sgn_norm_input(x, w, o, f, seg, V, xin);
  __syncthreads();
  sgn_embed_first(xin, w, o, E1, ES);
  sgn_fill_spa1(w, o, V, X0, BS);
  __syncthreads();
  sgn_embed_second(E1, ES, w, o, X0, BS);
  __syncthreads();
  sgn_adjacency(X0, BS, w, o, P, BS, X2, SGN_BWD_PART_STRIDE, BS, G, nullptr, V);
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
    store_act<1, 0>(acc, w + o.c1_b, X1, BS);
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
    store_act<2, 0>(acc, w + o.c2_b, X2, BS);
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
      float best;
      int arg;
      col_argmax(acc[i], w[o.c3_b + col], V, best, arg);
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
  sgn_g12(X0, BS, w, o, P, BS);
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

__global__ __launch_bounds__(SGN_THREADS) void sgn_dif_combine_kernel(const float* __restrict__ dj,
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
      sgn_clip_load_tile(feat, w, o, n, tile, seg, H);
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
      sgn_clip_cnn1(H, w, o, Y);
      __syncthreads();
      if (pass == 0) {
        // y2 and the arg-max frame of every column: the first frame wins a tie, 0 is what a ReLU leaves
        f32x16 acc[4] = {};
        mma_w<4>(Y + r * CS + h, w + o.t2_w + (long)h * SGN_C4 + wave * 32 + r, SGN_C4, SGN_C3, acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int col = (wave + SGN_WAVES * i) * 32 + r;
          float best;
          int a;
          col_argmax(acc[i], w[o.t2_b + col], nrows, best, a);
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

__global__ __launch_bounds__(SGN_THREADS) void sgn_sample_bwd_kernel(const float* __restrict__ win,
                                                                     const unsigned* __restrict__ r,
                                                                     const float* __restrict__ dout, float* dwin, int T,
                                                                     int V, int S, int seg) {
  __shared__ unsigned short rows[SGN_SAMPLE_MAX_ROWS];
  __shared__ int scan[SGN_THREADS];
  __shared__ unsigned char flag[SGN_SAMPLE_MAX_ROWS];
  const long n = blockIdx.x;
  const int tid = threadIdx.x;
  const long per = (long)3 * T * V * 2;
  for (long e = tid; e < per; e += SGN_THREADS) dwin[n * per + e] = 0.f;     // in front of the table's first barrier
  const int kept = sgn_kept_rows(win, n, T, V, flag, scan, rows);
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

// ---- the two backward launches: with a tape (of tape_floats floats) the taping instantiation, without one (null) the
// plain one.  The *_tape entries refuse a null tape themselves. ----
static int sgn_clip_bwd_launch(const float* feat, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                               const float* dlogits, float* dfeat, int N, int seg, int num_class, float* tape,
                               size_t tape_floats, void* stream) {
  if (!feat || !w || !wt || !dlogits || !dfeat) return AGCN_ERR_ARG;
  if (N < 1 || seg < 1 || num_class < 1) return AGCN_ERR_ARG;
  if (!sgn_clip_domain(N, seg, num_class)) return AGCN_ERR_UNSUPPORTED;
  if (w_floats != (size_t)sgn_clip_w(seg, num_class).total || wt_floats != (size_t)sgn_clip_wt().total) return AGCN_ERR_ARG;
  if (tape && tape_floats < sgn_clip_tape(N, seg).total) return AGCN_ERR_WORKSPACE;
  const dim3 grid((unsigned)N), block(SGN_THREADS);
  const size_t lds = (size_t)SGN_CLIP_BWD_LDS_FLOATS * 4;
  if (tape) {
    AGCN_NOTE_KERNEL("sgn_clip_bwd_kernel<f32 mfma, tape> seg=%d clips=%d", seg, N);
    return agcn_launch_big<sgn_clip_bwd_kernel<true>>(grid, block, lds, (hipStream_t)stream, feat, w, wt, dlogits, dfeat,
                                                      tape, seg, num_class);
  }
  AGCN_NOTE_KERNEL("sgn_clip_bwd_kernel<f32 mfma> seg=%d clips=%d", seg, N);
  return agcn_launch_big<sgn_clip_bwd_kernel<false>>(grid, block, lds, (hipStream_t)stream, feat, w, wt, dlogits, dfeat,
                                                     (float*)nullptr, seg, num_class);
}

static int sgn_frames_bwd_launch(const float* x, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                                 const float* dfeat, float* dx, void* ws, size_t ws_bytes, int N, int seg, int V, float* tape,
                                 size_t tape_floats, void* stream) {
  if (!x || !w || !wt || !dfeat || !dx || !ws) return AGCN_ERR_ARG;
  if (N < 1 || seg < 1 || V < 2 || V > SGN_MAX_V) return AGCN_ERR_ARG;
  if (!sgn_frames_domain(N, seg, V)) return AGCN_ERR_UNSUPPORTED;
  if (w_floats != (size_t)sgn_frames_w(V).total || wt_floats != (size_t)sgn_frames_wt().total) return AGCN_ERR_ARG;
  if (ws_bytes < sgn_frames_bwd_ws_floats(N, seg, V) * sizeof(float)) return AGCN_ERR_WORKSPACE;
  if (tape && tape_floats < sgn_frames_tape_floats(N, seg, V)) return AGCN_ERR_WORKSPACE;
  const long frames = (long)N * seg, total = frames * (V * 3);
  float* dj = (float*)ws;
  float* dd = dj + total;
  const dim3 grid((unsigned)frames), block(SGN_THREADS);
  const size_t lds = (size_t)SGN_FRAMES_BWD_LDS_FLOATS * 4;
  int rc;
  if (tape) {
    AGCN_NOTE_KERNEL("sgn_frames_bwd_kernel<f32 mfma, tape> V=%d frames=%ld", V, frames);
    rc = agcn_launch_big<sgn_frames_bwd_kernel<true>>(grid, block, lds, (hipStream_t)stream, x, w, wt, dfeat, dj, dd, tape,
                                                      seg, V);
  } else {
    AGCN_NOTE_KERNEL("sgn_frames_bwd_kernel<f32 mfma> V=%d frames=%ld", V, frames);
    rc = agcn_launch_big<sgn_frames_bwd_kernel<false>>(grid, block, lds, (hipStream_t)stream, x, w, wt, dfeat, dj, dd,
                                                       (float*)nullptr, seg, V);
  }
  if (rc != AGCN_OK) return rc;
  hipLaunchKernelGGL(sgn_dif_combine_kernel, dim3((unsigned)((total + SGN_THREADS - 1) / SGN_THREADS)), dim3(SGN_THREADS), 0,
                     (hipStream_t)stream, (const float*)dj, (const float*)dd, dx, total, seg, V * 3);
  return agcn_check_launch();
}

extern "C" int agcn_sgn_clip_bwd(const float* feat, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                                 const float* dlogits, float* dfeat, int N, int seg, int num_class, void* stream) {
  return sgn_clip_bwd_launch(feat, w, w_floats, wt, wt_floats, dlogits, dfeat, N, seg, num_class, nullptr, 0, stream);
}
extern "C" int agcn_sgn_clip_bwd_tape(const float* feat, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                                      const float* dlogits, float* dfeat, int N, int seg, int num_class, float* tape,
                                      size_t tape_floats, void* stream) {
  if (!tape) return AGCN_ERR_ARG;
  return sgn_clip_bwd_launch(feat, w, w_floats, wt, wt_floats, dlogits, dfeat, N, seg, num_class, tape, tape_floats, stream);
}

extern "C" int agcn_sgn_frames_bwd(const float* x, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                                   const float* dfeat, float* dx, void* ws, size_t ws_bytes, int N, int seg, int V,
                                   void* stream) {
  return sgn_frames_bwd_launch(x, w, w_floats, wt, wt_floats, dfeat, dx, ws, ws_bytes, N, seg, V, nullptr, 0, stream);
}
extern "C" int agcn_sgn_frames_bwd_tape(const float* x, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                                        const float* dfeat, float* dx, void* ws, size_t ws_bytes, int N, int seg, int V,
                                        float* tape, size_t tape_floats, void* stream) {
  if (!tape) return AGCN_ERR_ARG;
  return sgn_frames_bwd_launch(x, w, w_floats, wt, wt_floats, dfeat, dx, ws, ws_bytes, N, seg, V, tape, tape_floats, stream);
}

extern "C" int agcn_sgn_sample_bwd(const float* win, const unsigned* r, const float* dout, float* dwin, int N, int T, int V,
                                   int K, int S, int seg, void* stream) {
  if (!win || !r || !dout || !dwin) return AGCN_ERR_ARG;
  if (!sgn_sample_domain(N, T, V, K, S, seg)) return AGCN_ERR_ARG;
  hipLaunchKernelGGL(sgn_sample_bwd_kernel, dim3((unsigned)N), dim3(SGN_THREADS), 0, (hipStream_t)stream, win, r, dout, dwin,
                     T, V, S, seg);
  return agcn_check_launch();
}
