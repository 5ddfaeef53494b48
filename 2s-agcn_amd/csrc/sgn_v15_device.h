// The attention block of SGN v15, written once as a device function template over (input width, output width): the
// joint-level kernel calls it at 128 -> 256 over the joints of a frame, the frame-level kernel at 256 -> 512 over the
// frames of a clip (sgn_v15.hip).  Geometry, walks and the LDS carve: sgn_v15_plan.h; the MFMA helpers: sgn_device.h.
// Behind it its backward, sgn15_block_bwd (sgn_v15_bwd.hip; formulas and carve: sgn_v15_bwd_plan.h).
// Everything is exact-f32 MFMA with a fixed summation order; no atomics.
#pragma once
#include "sgn_device.h"
#include "sgn_v15_plan.h"
#include "sgn_v15_bwd_plan.h"
#include "sgn_v15_wgrad_plan.h"

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
// sgn15_block_y is the block up to the accumulators of y (without b2 + br), which the backward takes the arg-max rows
// from; it leaves x1 in X and a barrier behind the last read of QKV and P.  sgn15_block adds the maximum.
// X1_ONLY (compile time): stop behind the barrier that follows "x1 = attention + bo + x, in place" -- the attention half,
// which reads qkv_w, qkv_b, o_w, o_b and nothing else of the block; ff, f1_*, f2_* and accY are then not touched (the
// batch-statistics pass of n_f, sgn_v15_stats.hip, through sgn15_block_x1 below).  A flag and not a second function: the
// group walk is written once, and the instantiations without the flag are the code they were.
template <int DIN, int DOUT, bool X1_ONLY = false>
__device__ __forceinline__ void sgn15_block_y(float* X, float* QKV, float* P, const float* __restrict__ w,
                                              const Sgn15BlockW& o, int rows, int heads, int d_head, int ff,
                                              float* __restrict__ attn, f32x16 (&accY)[DOUT / SGN15_GROUP]) {
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
  if constexpr (X1_ONLY) return;

  // y = [relu(x1 W1 + b1) | x1] . [W2 ; Wr] + (b2 + br): the hidden tile in chunks of 128 columns, ascending, then x1
#pragma unroll
  for (int i = 0; i < NBY; ++i) accY[i] = f32x16{};
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
}

// the attention half alone: x -> x1 in place in X, a barrier behind it
template <int DIN, int DOUT>
__device__ __forceinline__ void sgn15_block_x1(float* X, float* QKV, float* P, const float* __restrict__ w,
                                               const Sgn15BlockW& o, int rows, int heads, int d_head) {
  f32x16 unused[DOUT / SGN15_GROUP];
  sgn15_block_y<DIN, DOUT, true>(X, QKV, P, w, o, rows, heads, d_head, SGN15_GROUP, nullptr, unused);
}

template <int DIN, int DOUT>
__device__ __forceinline__ void sgn15_block(float* X, float* QKV, float* P, const float* __restrict__ w,
                                            const Sgn15BlockW& o, int rows, int heads, int d_head, int ff,
                                            float* __restrict__ attn, float (&m)[DOUT / SGN15_GROUP]) {
  constexpr int NBY = DOUT / SGN15_GROUP;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  f32x16 accY[NBY];
  sgn15_block_y<DIN, DOUT>(X, QKV, P, w, o, rows, heads, d_head, ff, attn, accY);
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

// ---- the backward of the block (sgn_v15_bwd_plan.h: the formulas, the carve, where it can go wrong) ----

// The arg-max row of acc + bv over the rows < nrows of the lane's column, in both lanes of the column.  Unlike col_argmax
// it starts from -inf: there is no ReLU in front of v15's maxima, so a maximum may be negative and always has a row.
// Rows ascend with j and a strict > keeps the lowest index; the merge of the two half-waves keeps the lower row at a tie.
__device__ __forceinline__ int sgn15_col_argmax(const f32x16& acc, float bv, int nrows) {
  const int h = (threadIdx.x & 63) >> 5;
  float best = -INFINITY;
  int arg = -1;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int row = mfma_row(j, h);
    const float v = acc[j] + bv;
    if (row < nrows && (arg < 0 || v > best)) {
      best = v;
      arg = row;
    }
  }
  const float ob = __shfl_xor(best, 32);
  const int oa = __shfl_xor(arg, 32);
  if (oa >= 0 && (arg < 0 || ob > best || (ob == best && oa < arg))) arg = oa;
  return arg;
}

// an accumulator tile -> 32 columns of an LDS band from column `col` on
__device__ __forceinline__ void sgn15_store_tile(const f32x16& a, float* band, int stride, int col) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int j = 0; j < 16; ++j) band[mfma_row(j, h) * stride + col + r] = a[j];
}
// ... -> the wave's own 32-column block of a 128-column band
__device__ __forceinline__ void sgn15_store_block(const f32x16& a, float* band, int stride) {
  sgn15_store_tile(a, band, stride, (threadIdx.x >> 6) * 32);
}

// ---- the taping instantiations (sgn_v15_wgrad_plan.h): global stores only, from the lanes that hold the values; trow is
// row 0 of this token set in the tape, TC the tape's row stride.  Lanes of padded rows store nothing. ----
// the real rows of an accumulator tile -> 32 columns of the tape from column `col` on
__device__ __forceinline__ void sgn15_tape_tile(const f32x16& a, int rows, float* trow, size_t TC, int col) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int row = mfma_row(j, h);
    if (row < rows) trow[(size_t)row * TC + col + r] = a[j];
  }
}
// rows [0, nrows) x width columns of an LDS band -> the tape, consecutive threads on consecutive columns.  Only reads LDS:
// it may run next to readers of the band, between the barrier behind its producer and the one in front of its next writer.
__device__ __forceinline__ void sgn15_tape_band(const float* band, int stride, int nrows, int width, float* dst, size_t ld) {
  for (int i = threadIdx.x; i < nrows * width; i += SGN_THREADS) {
    const int row = i / width, c = i - row * width;
    dst[(size_t)row * ld + c] = band[row * stride + c];
  }
}

// dS = P * (dP - rowsum(dP * P)) of one head, dP in the accumulator layout, P in its slot -> dS in registers.  The row sum
// runs over the 32 lanes of the half-wave that holds the row; P is zero in padded rows and columns, and so is dS.
__device__ __forceinline__ f32x16 sgn15_softmax_bwd(const f32x16& dp, const float* Pslot) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  f32x16 ds;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float p = Pslot[mfma_row(j, h) * SGN15_P_STRIDE + r];
    const float rs = half_sum(dp[j] * p);
    ds[j] = p * (dp[j] - rs);
  }
  return ds;
}

// X holds the `rows` real token rows x (as for sgn15_block, one barrier in front).  d[i]: the gradient of the pooled
// column (wave + SGN_WAVES * i) * 32 + r, which goes to the column's arg-max row.  reload(): writes x into X again (the
// forward leaves x1 there).  -> dX[i]: d x of the column blocks wave + SGN_WAVES * i, all 32 rows (padded rows: zero).
// w / o the forward image, wt / ot the transposed one.  Barriers inside, the last one behind every read of LDS.
// TAPE: the same arithmetic in the same order (dX is the same bits), and every operand pair of the block's weight
// gradients copied to the tape rows trow (sections bt, row stride TC) at the step it is live; o = concat_h(P v), which only
// the forward holds, is formed again in the group walk while P and v are live.  ymax, unless null: the pooled maxima of
// the DOUT columns, the forward's values.  With TAPE off trow, TC, bt and ymax are not read.
template <int DIN, int DOUT, bool TAPE, class Reload>
__device__ __forceinline__ void sgn15_block_bwd(float* X, float* QKV, float* DO, float* P, const float* __restrict__ w,
                                                const Sgn15BlockW& o, const float* __restrict__ wt, const Sgn15BlockWT& ot,
                                                int rows, int heads, int d_head, int ff,
                                                const float (&d)[DOUT / SGN15_GROUP], Reload reload,
                                                f32x16 (&dX)[DIN / SGN15_GROUP], float* __restrict__ trow, size_t TC,
                                                const Sgn15BlockTape& bt, float* __restrict__ ymax) {
  constexpr int XS = SGN15_X_STRIDE(DIN), QS = SGN15_QKV_STRIDE, DS = SGN15_BWD_DO_STRIDE, PS = SGN15_P_STRIDE;
  constexpr int DYS = SGN15_BWD_DY_STRIDE(DOUT), NBO = DIN / SGN15_GROUP, NBY = DOUT / SGN15_GROUP;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int inner = heads * d_head, groups = sgn15_groups(heads, d_head);
  const int Kp = (rows + 1) & ~1;
  float* Q = QKV;
  float* Kk = QKV + SGN15_GROUP;
  float* Vv = QKV + 2 * SGN15_GROUP;
  float* DY = QKV;                                 // (32, DOUT + 1) over QKV and DO
  float* DH = P;                                   // (32, 129)

  // ---- the forward and the arg-max row of every column; dy dense, one non-zero per column ----
  {
    f32x16 accY[NBY];
    sgn15_block_y<DIN, DOUT>(X, QKV, P, w, o, rows, heads, d_head, ff, nullptr, accY);
#pragma unroll
    for (int i = 0; i < NBY; ++i) {
      const int col = (wave + SGN_WAVES * i) * 32 + r;
      const int arg = sgn15_col_argmax(accY[i], w[o.f2_b + col], rows);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int row = mfma_row(j, h);
        DY[row * DYS + col] = row == arg ? d[i] : 0.f;
        if constexpr (TAPE)
          if (row < rows) trow[(size_t)row * TC + bt.dy + col] = row == arg ? d[i] : 0.f;
      }
      if constexpr (TAPE)
        if (ymax) {                                // the maximum as sgn15_block forms it
          const float bv = w[o.f2_b + col];
          float v = -INFINITY;
#pragma unroll
          for (int j = 0; j < 16; ++j)
            if (mfma_row(j, h) < rows) v = fmaxf(v, accY[i][j] + bv);
          v = fmaxf(v, __shfl_xor(v, 32));
          if (h == 0) ymax[col] = v;
        }
    }
  }
  __syncthreads();
  if constexpr (TAPE) sgn15_tape_band(X, XS, rows, DIN, trow + bt.x1, TC);       // x1: X is not written before reload()

  // ---- the feed-forward: dx1 = dy Wr^T + sum_c (dy W2_c^T * [hidden_c > 0]) W1_c^T, in registers ----
  const int ldf2 = ff + DIN;
  f32x16 dx1[NBO] = {};
  mma_w<NBO>(DY + r * DYS + h, wt + ot.f2 + (long)h * ldf2 + ff + wave * 32 + r, ldf2, DOUT, dx1);
  for (int c = 0; c < sgn15_chunks(ff); ++c) {
    const int col = sgn15_chunk_col(c) + wave * 32 + r;
    f32x16 hid[1] = {};
    mma_ws<1>(X + r * XS + h, w + o.f1_w + (long)h * ff + col, ff, 0, DIN, hid);      // the forward's sequence
    f32x16 dh[1] = {};
    mma_w<1>(DY + r * DYS + h, wt + ot.f2 + (long)h * ldf2 + col, ldf2, DOUT, dh);
    const float bv = w[o.f1_b + col];
#pragma unroll
    for (int j = 0; j < 16; ++j) DH[mfma_row(j, h) * DS + wave * 32 + r] = hid[0][j] + bv > 0.f ? dh[0][j] : 0.f;
    if constexpr (TAPE) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int row = mfma_row(j, h);
        if (row < rows) {
          trow[(size_t)row * TC + bt.hid + col] = fmaxf(hid[0][j] + bv, 0.f);
          trow[(size_t)row * TC + bt.dhid + col] = hid[0][j] + bv > 0.f ? dh[0][j] : 0.f;
        }
      }
    }
    __syncthreads();
    mma_w<NBO>(DH + r * DS + h, wt + ot.f1 + (long)(sgn15_chunk_col(c) + h) * DIN + wave * 32 + r, DIN, SGN15_GROUP, dx1);
    __syncthreads();
  }
  reload();
#pragma unroll
  for (int i = 0; i < NBO; ++i) dX[i] = dx1[i];    // the attention residual
  __syncthreads();
  if constexpr (TAPE) {
#pragma unroll
    for (int i = 0; i < NBO; ++i) sgn15_tape_tile(dx1[i], rows, trow, TC, bt.dx1 + (wave + SGN_WAVES * i) * 32);
    sgn15_tape_band(X, XS, rows, DIN, trow + bt.x, TC);                           // x again: only read from here on
  }
  // o of group g = P v (both live), the forward's product: the taping instantiation only
  auto tape_o = [&](int g, const f32x16& av) { sgn15_tape_tile(av, rows, trow, TC, bt.o + sgn15_group_col(g) + wave * 32); };

  // do = dx1 Wo_g^T into DO: each 128-column half of dx1 is staged through DO from the registers that hold it
  auto make_do = [&](int g) {
    f32x16 a[1] = {};
#pragma unroll
    for (int i = 0; i < NBO; ++i) {
      sgn15_store_block(dx1[i], DO, DS);
      __syncthreads();
      mma_w<1>(DO + r * DS + h, wt + ot.o + (long)(i * SGN15_GROUP + h) * inner + sgn15_group_col(g) + wave * 32 + r, inner,
               SGN15_GROUP, a);
      __syncthreads();
    }
    sgn15_store_block(a[0], DO, DS);
    __syncthreads();
  };
  // [dq | dk | dv] of group g over [q | k | v], then dX += [dq | dk | dv] (Wqkv_g)^T; a barrier in front and behind
  auto finish = [&](int g, const f32x16& dq, const f32x16& dk, const f32x16& dv) {
    __syncthreads();
    sgn15_store_block(dq, Q, QS);
    sgn15_store_block(dk, Kk, QS);
    sgn15_store_block(dv, Vv, QS);
    if constexpr (TAPE) {                          // behind the pair select, once per group
      const int col = bt.dqkv + sgn15_group_col(g) + wave * 32;
      sgn15_tape_tile(dq, rows, trow, TC, col);
      sgn15_tape_tile(dk, rows, trow, TC, col + inner);
      sgn15_tape_tile(dv, rows, trow, TC, col + 2 * inner);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 3; ++s)
      mma_w<NBO>(QKV + s * SGN15_GROUP + r * QS + h,
                 wt + ot.qkv + ((long)s * inner + sgn15_group_col(g) + h) * DIN + wave * 32 + r, DIN, SGN15_GROUP, dX);
    __syncthreads();
  };

  if (!sgn15_sliced(d_head)) {
    const int hg = sgn15_group_heads(d_head);
    const int lh0 = wave * 32 / d_head;            // the (first) head of the wave's 32-column block
    const bool pair = d_head == SGN15_MIN_HEAD;
    for (int g = 0; g < groups; ++g) {
      sgn15_qkv<DIN, 3>(X, w, o, inner, g, 0, QKV);
      make_do(g);
      for (int lh = wave; lh < hg; lh += SGN_WAVES) {
        const f32x16 s = mma_l(Q + lh * d_head, QS, 1, Kk + lh * d_head, 1, QS, d_head, f32x16{});
        sgn15_softmax_store(s, rows, P + lh * SGN15_P_SLOT, nullptr);
      }
      __syncthreads();
      if constexpr (TAPE) {
        f32x16 av = mma_l(P + lh0 * SGN15_P_SLOT, PS, 1, Vv + wave * 32, QS, 1, Kp, f32x16{});
        if (pair) {
          const f32x16 av1 = mma_l(P + (lh0 + 1) * SGN15_P_SLOT, PS, 1, Vv + wave * 32, QS, 1, Kp, f32x16{});
          if (r >= 16) av = av1;
        }
        tape_o(g, av);
      }
      // dv = P^T do of the wave's block; dP = do_h v_h^T and dS of the wave's heads
      f32x16 dv = mma_l(P + lh0 * SGN15_P_SLOT, 1, PS, DO + wave * 32, DS, 1, Kp, f32x16{});
      if (pair) {
        const f32x16 dv1 = mma_l(P + (lh0 + 1) * SGN15_P_SLOT, 1, PS, DO + wave * 32, DS, 1, Kp, f32x16{});
        if (r >= 16) dv = dv1;
      }
      f32x16 ds[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int lh = wave + SGN_WAVES * u;
        if (lh < hg) {
          const f32x16 dp = mma_l(DO + lh * d_head, DS, 1, Vv + lh * d_head, 1, QS, d_head, f32x16{});
          ds[u] = sgn15_softmax_bwd(dp, P + lh * SGN15_P_SLOT);
        }
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int lh = wave + SGN_WAVES * u;
        if (lh < hg) {
#pragma unroll
          for (int j = 0; j < 16; ++j) P[lh * SGN15_P_SLOT + mfma_row(j, h) * PS + r] = ds[u][j];
        }
      }
      __syncthreads();
      // dq = dS k, dk = dS^T q of the wave's block
      f32x16 dq = mma_l(P + lh0 * SGN15_P_SLOT, PS, 1, Kk + wave * 32, QS, 1, Kp, f32x16{});
      f32x16 dk = mma_l(P + lh0 * SGN15_P_SLOT, 1, PS, Q + wave * 32, QS, 1, Kp, f32x16{});
      if (pair) {
        const f32x16 dq1 = mma_l(P + (lh0 + 1) * SGN15_P_SLOT, PS, 1, Kk + wave * 32, QS, 1, Kp, f32x16{});
        const f32x16 dk1 = mma_l(P + (lh0 + 1) * SGN15_P_SLOT, 1, PS, Q + wave * 32, QS, 1, Kp, f32x16{});
        if (r >= 16) {
          dq = dq1;
          dk = dk1;
        }
      }
      finish(g, dq, dk, dv);
    }
  } else {
    const int hs = sgn15_head_groups(d_head);
    float* dS = P + SGN15_BWD_DS_SLOT * SGN15_P_SLOT;
    for (int head = 0; head < heads; ++head) {
      // pass 1: the scores and P, the forward's sequence
      f32x16 s = {};
      for (int sl = 0; sl < hs; ++sl) {
        sgn15_qkv<DIN, 2>(X, w, o, inner, head * hs + sl, 0, QKV);
        __syncthreads();
        s = mma_l(Q + wave * 32, QS, 1, Kk + wave * 32, 1, QS, 32, s);
        __syncthreads();
      }
      sgn15_store_tile(s, P + (1 + wave) * SGN15_P_SLOT, PS, 0);
      __syncthreads();
      if (wave == 0) {
        f32x16 t;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int e = mfma_row(j, h) * PS + r;
          t[j] = ((P[SGN15_P_SLOT + e] + P[2 * SGN15_P_SLOT + e]) + P[3 * SGN15_P_SLOT + e]) + P[4 * SGN15_P_SLOT + e];
        }
        sgn15_softmax_store(t, rows, P, nullptr);
      }
      __syncthreads();
      // pass 2: dP = sum over the slices of do_s v_s^T, K split over the waves, partials added in wave order; dS
      f32x16 dp = {};
      for (int sl = 0; sl < hs; ++sl) {
        sgn15_qkv<DIN, 1>(X, w, o, inner, head * hs + sl, 2, QKV);
        make_do(head * hs + sl);
        dp = mma_l(DO + wave * 32, DS, 1, Vv + wave * 32, 1, QS, 32, dp);
        __syncthreads();
      }
      sgn15_store_tile(dp, P + (1 + wave) * SGN15_P_SLOT, PS, 0);
      __syncthreads();
      if (wave == 0) {
        f32x16 t;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int e = mfma_row(j, h) * PS + r;
          t[j] = ((P[SGN15_P_SLOT + e] + P[2 * SGN15_P_SLOT + e]) + P[3 * SGN15_P_SLOT + e]) + P[4 * SGN15_P_SLOT + e];
        }
        const f32x16 v = sgn15_softmax_bwd(t, P);
#pragma unroll
        for (int j = 0; j < 16; ++j) dS[mfma_row(j, h) * PS + r] = v[j];
      }
      __syncthreads();
      // pass 3: dq_s, dk_s, dv_s slice by slice
      for (int sl = 0; sl < hs; ++sl) {
        const int g = head * hs + sl;
        sgn15_qkv<DIN, 3>(X, w, o, inner, g, 0, QKV);
        make_do(g);
        if constexpr (TAPE) tape_o(g, mma_l(P, PS, 1, Vv + wave * 32, QS, 1, Kp, f32x16{}));
        const f32x16 dv = mma_l(P, 1, PS, DO + wave * 32, DS, 1, Kp, f32x16{});
        const f32x16 dq = mma_l(dS, PS, 1, Kk + wave * 32, QS, 1, Kp, f32x16{});
        const f32x16 dk = mma_l(dS, 1, PS, Q + wave * 32, QS, 1, Kp, f32x16{});
        finish(g, dq, dk, dv);
      }
    }
  }
}
