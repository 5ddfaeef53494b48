// The attention block of SGN v15, written once as a device function template over (input width, output width): the
// joint-level kernel calls it at 128 -> 256 over the joints of a frame, the frame-level kernel at 256 -> 512 over the
// frames of a clip (sgn_v15.hip).  Geometry, walks and the LDS carve: sgn_v15_plan.h; the MFMA helpers: sgn_device.h.
// Everything is exact-f32 MFMA with a fixed summation order; no atomics.
#pragma once
#include "sgn_device.h"
#include "sgn_v15_plan.h"

// mma_w with the column step between a wave's blocks as a parameter: block i of the wave sits cstep columns after
// block i - 1 (the q, k and v sections of one group are `inner` columns apart in [Wq | Wk | Wv]).  As there, 16 weight
// loads (15 at NB = 3) are in flight per step.
template <int NB>
__device__ __forceinline__ void mma_ws(const float* a, const float* __restrict__ b, long ldb, long cstep, int K,
                                       f32x16 (&acc)[NB]) {
#pragma unroll 16 / NB
  for (int k = 0; k < K; k += 2) {
    const float av = a[k];
#pragma unroll
    for (int i = 0; i < NB; ++i) acc[i] = mfma32(av, b[(long)k * ldb + i * cstep], acc[i]);
  }
}

__device__ __forceinline__ float half_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  v = fmaxf(v, __shfl_xor(v, 8));
  v = fmaxf(v, __shfl_xor(v, 4));
  v = fmaxf(v, __shfl_xor(v, 2));
  v = fmaxf(v, __shfl_xor(v, 1));
  return v;
}

// Softmax of a 32 x 32 score tile held in the MFMA accumulator layout (register j of lane (r, h): row mfma_row(j, h),
// column r) over the real columns j < rows only; padded query rows (>= rows) give zeros, never NaN: their scores are
// finite garbage, the row is computed like any other and then dropped.  -> P (LDS, stride SGN15_P_STRIDE) and, unless
// null, the (rows, rows) map `out` of one head in global memory (element (i, j) at sgn15_attn_index(0, 1, 0, rows, i, j)).
__device__ __forceinline__ void sgn15_softmax_store(const f32x16& s, int rows, float* P, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const bool col_ok = r < rows;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int row = mfma_row(j, h);
    const float v = col_ok ? s[j] : -INFINITY;
    const float mx = half_max(v);                    // column 0 is always real: finite
    const float e = col_ok ? expf(v - mx) : 0.f;
    const float sum = half_sum(e);                   // >= 1
    const float p = row < rows ? e / sum : 0.f;
    P[row * SGN15_P_STRIDE + r] = p;
    if (out && row < rows && col_ok) out[sgn15_attn_index(0, 1, 0, rows, row, r)] = p;
  }
}

// [section `first` ...] of group g of [q | k | v] = X . W + b into QKV: NB sections from `first` on (0 = q, 1 = k, 2 = v)
template <int DIN, int NB>
__device__ __forceinline__ void sgn15_qkv(const float* X, const float* __restrict__ w, const Sgn15BlockW& o, int inner,
                                          int g, int first, float* QKV) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const long col = (long)first * inner + sgn15_group_col(g) + wave * 32 + r;
  f32x16 acc[NB] = {};
  mma_ws<NB>(X + r * SGN15_X_STRIDE(DIN) + h, w + o.qkv_w + (long)h * 3 * inner + col, 3L * inner, inner, DIN, acc);
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const float bv = w[o.qkv_b + col + (long)i * inner];
#pragma unroll
    for (int j = 0; j < 16; ++j)
      QKV[mfma_row(j, h) * SGN15_QKV_STRIDE + (first + i) * SGN15_GROUP + wave * 32 + r] = acc[i][j] + bv;
  }
}

// The block on `rows` real token rows (1..32) of X (LDS, 32 x DIN, stride DIN + 1; padded rows hold finite garbage).
// -> m[i]: the maximum over the REAL rows of output column (wave + SGN_WAVES * i) * 32 + r, in both lanes of the
// column.  There is no ReLU in front of the reference's pooling, so the maximum starts from -inf and skips the padded
// rows, which hold bias garbage, not zeros.  attn: this token set's (heads, rows, rows) maps (the caller's
// sgn15_attn_index(b, heads, 0, rows, 0, 0) into the output), or null.
// The per-head output pointer is formed at the call of sgn15_softmax_store, not inside it: with the (token set, head)
// index carried into the store the compiler put a full vmcnt(0) wait behind every batch of weight loads of the product
// loops (measured: 1.76 instead of 1.21 ms for one window with 1 x 1024 heads).
// Barriers inside; the caller puts one in front (X complete) and needs none behind for m.
template <int DIN, int DOUT>
__device__ __forceinline__ void sgn15_block(float* X, float* QKV, float* P, const float* __restrict__ w,
                                            const Sgn15BlockW& o, int rows, int heads, int d_head, int ff,
                                            float* __restrict__ attn, float (&m)[DOUT / SGN15_GROUP]) {
  constexpr int XS = SGN15_X_STRIDE(DIN), QS = SGN15_QKV_STRIDE, NBO = DIN / SGN15_GROUP, NBY = DOUT / SGN15_GROUP;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int inner = heads * d_head, groups = sgn15_groups(heads, d_head);
  const int Kp = (rows + 1) & ~1;                  // P's columns >= rows are zero: the odd column adds nothing
  float* Q = QKV;
  float* Kk = QKV + SGN15_GROUP;
  float* Vv = QKV + 2 * SGN15_GROUP;
  f32x16 accO[NBO] = {};                           // concat_h(a . v) . Wo, accumulated over the groups in ascending order

  // the output projection of group g, whose a . v (32 x 128) sits in the q section, onto accO
  auto project = [&](int g) {
    mma_w<NBO>(Q + r * QS + h, w + o.o_w + (long)(sgn15_group_col(g) + h) * DIN + wave * 32 + r, DIN, SGN15_GROUP, accO);
  };

  if (!sgn15_sliced(d_head)) {
    const int hg = sgn15_group_heads(d_head);      // 2, 4 or 8 whole heads per group
    for (int g = 0; g < groups; ++g) {
      sgn15_qkv<DIN, 3>(X, w, o, inner, g, 0, QKV);
      __syncthreads();
      for (int lh = wave; lh < hg; lh += SGN_WAVES) {
        const f32x16 s = mma_l(Q + lh * d_head, QS, 1, Kk + lh * d_head, 1, QS, d_head, f32x16{});
        const int head = sgn15_group_first_head(g, d_head) + lh;
        sgn15_softmax_store(s, rows, P + lh * SGN15_P_SLOT, attn ? attn + sgn15_attn_index(0, heads, head, rows, 0, 0) : nullptr);
      }
      __syncthreads();
      {
        // the wave's block holds one head (d_head >= 32) or two (d_head = 16): each column takes the product with its
        // own head's probabilities
        const int lh0 = wave * 32 / d_head;
        f32x16 av = mma_l(P + lh0 * SGN15_P_SLOT, SGN15_P_STRIDE, 1, Vv + wave * 32, QS, 1, Kp, f32x16{});
        if (d_head == 16) {
          const f32x16 av1 = mma_l(P + (lh0 + 1) * SGN15_P_SLOT, SGN15_P_STRIDE, 1, Vv + wave * 32, QS, 1, Kp, f32x16{});
          if (r >= 16) av = av1;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) Q[mfma_row(j, h) * QS + wave * 32 + r] = av[j];
      }
      __syncthreads();
      project(g);
      __syncthreads();
    }
  } else {
    const int hs = sgn15_head_groups(d_head);      // the head's K-slices
    for (int head = 0; head < heads; ++head) {
      // pass 1: the scores.  NOT one accumulator over the head's columns in ascending order: each wave accumulates its
      // own 32-column quarter of every slice over the slices in ascending order, and the four waves' partials are then
      // added in wave order, all before the softmax.  The order is fixed, so the bits are reproducible.
      f32x16 s = {};
      for (int sl = 0; sl < hs; ++sl) {
        sgn15_qkv<DIN, 2>(X, w, o, inner, head * hs + sl, 0, QKV);
        __syncthreads();
        s = mma_l(Q + wave * 32, QS, 1, Kk + wave * 32, 1, QS, 32, s);
        __syncthreads();
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) P[(1 + wave) * SGN15_P_SLOT + mfma_row(j, h) * SGN15_P_STRIDE + r] = s[j];
      __syncthreads();
      if (wave == 0) {
        f32x16 t;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int e = mfma_row(j, h) * SGN15_P_STRIDE + r;
          t[j] = ((P[SGN15_P_SLOT + e] + P[2 * SGN15_P_SLOT + e]) + P[3 * SGN15_P_SLOT + e]) + P[4 * SGN15_P_SLOT + e];
        }
        sgn15_softmax_store(t, rows, P, attn ? attn + sgn15_attn_index(0, heads, head, rows, 0, 0) : nullptr);
      }
      __syncthreads();
      // pass 2: per slice v, a . v and the projection
      for (int sl = 0; sl < hs; ++sl) {
        const int g = head * hs + sl;
        sgn15_qkv<DIN, 1>(X, w, o, inner, g, 2, QKV);
        __syncthreads();
        const f32x16 av = mma_l(P, SGN15_P_STRIDE, 1, Vv + wave * 32, QS, 1, Kp, f32x16{});
#pragma unroll
        for (int j = 0; j < 16; ++j) Q[mfma_row(j, h) * QS + wave * 32 + r] = av[j];
        __syncthreads();
        project(g);
        __syncthreads();
      }
    }
  }

  // x1 = attention + bo + x, in place: every element is read and written by the one lane that owns it
#pragma unroll
  for (int i = 0; i < NBO; ++i) {
    const int col = (wave + SGN_WAVES * i) * 32 + r;
    const float bv = w[o.o_b + col];
#pragma unroll
    for (int j = 0; j < 16; ++j) X[mfma_row(j, h) * XS + col] += accO[i][j] + bv;
  }
  __syncthreads();

  // y = [relu(x1 W1 + b1) | x1] . [W2 ; Wr] + (b2 + br): the hidden tile in chunks of 128 columns, ascending, then x1
  f32x16 accY[NBY] = {};
  for (int c = 0; c < sgn15_chunks(ff); ++c) {
    const int col = sgn15_chunk_col(c) + wave * 32 + r;
    f32x16 hid[1] = {};
    mma_ws<1>(X + r * XS + h, w + o.f1_w + (long)h * ff + col, ff, 0, DIN, hid);
    const float bv = w[o.f1_b + col];
#pragma unroll
    for (int j = 0; j < 16; ++j) QKV[mfma_row(j, h) * QS + wave * 32 + r] = fmaxf(hid[0][j] + bv, 0.f);
    __syncthreads();
    mma_w<NBY>(QKV + r * QS + h, w + o.f2_w + (long)(sgn15_chunk_col(c) + h) * DOUT + wave * 32 + r, DOUT, SGN15_GROUP, accY);
    __syncthreads();
  }
  mma_w<NBY>(X + r * XS + h, w + o.f2_w + (long)(ff + h) * DOUT + wave * 32 + r, DOUT, DIN, accY);
#pragma unroll
  for (int i = 0; i < NBY; ++i) {
    const float bv = w[o.f2_b + (wave + SGN_WAVES * i) * 32 + r];
    float v = -INFINITY;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (mfma_row(j, h) < rows) v = fmaxf(v, accY[i][j] + bv);
    m[i] = fmaxf(v, __shfl_xor(v, 32));
  }
}
