// Transformer-encoder head of aagcn_v17 (reference model/architecture/aagcn/aagcn_v17.py): the parts between the four
// projections of a layer, which stay vendor GEMMs:
//
//   * tokens: backbone output (N*M, C, T', V) -> (N, [CLS +] M*T', V*C) with the positional table added, and back;
//   * the attention core of one layer: softmax(q k^T / sqrt(dh) + mask) [dropout] v for all heads from the packed
//     in_proj output, the head-averaged weights, and its backward;
//   * LayerNorm of (a + b) over rows of D, and its backward;
//   * for the spatial head of aagcn_v24 (reference model/architecture/aagcn/aagcn_v24.py): tokens over joints, one sequence
//     per frame window, (N*M, C, T', V) -> (N*T', [CLS +] M*V, C); an additive bias (Hb, L, L) on the logits of the
//     attention core; its gradient, the score gradient summed over the sequences.
//
// Arithmetic is fp32 FMA in every AGCN_GEMM mode: the core is ~10 % of the layer's FLOPs and latency-bound at L = 201.
// No float atomics: every sum over rows / samples / heads is taken by one thread or one workgroup in a fixed order, so
// the results are bitwise reproducible.  All geometry and index arithmetic is in encoder_plan.h (swept on the host by
// tests/encoder_plan_check.cpp); rows are staged with 16-byte loads where their starts are aligned (dh % 4 == 0), with
// scalar loads otherwise (dh = 25 is legal).
#include "agcn_common.h"
#include "encoder_plan.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// shared device pieces of the attention kernels
// ---------------------------------------------------------------------------------------------------------------------
// rows [row0, row0 + nrows) x columns [0, dh) of a row-major matrix (leading dimension ld) -> LDS rows of stride lp, padded
// with zeros up to dhp columns and for rows >= L
// (lp % 4 == 0: the LDS rows are 16-byte aligned).  Row starts in memory are 16-byte aligned only when dh % 4 == 0,
// ld % 4 == 0 and the base pointer is: then 16-byte loads, else scalar ones (dh = 25 is legal).
__device__ __forceinline__ void stage_rows(float* __restrict__ dst, int lp, const float* __restrict__ src, long ld, int row0,
                                           int nrows, int L, int dh, int dhp) {
  if ((dh & 3) == 0 && (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
    const int q = dhp >> 2, total = nrows * q;           // dhp == dh
    for (int e = threadIdx.x; e < total; e += ENC_THREADS) {
      const int j = e / q, d4 = e - j * q;
      const int row = row0 + j;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (row < L) v = *reinterpret_cast<const f32x4*>(src + (long)row * ld + 4 * d4);
      *reinterpret_cast<f32x4*>(dst + j * lp + 4 * d4) = v;
    }
    return;
  }
  const int total = nrows * dhp;
  for (int e = threadIdx.x; e < total; e += ENC_THREADS) {
    const int j = e / dhp, d = e - j * dhp;
    const int row = row0 + j;
    dst[j * lp + d] = (row < L && d < dh) ? src[(long)row * ld + d] : 0.f;
  }
}

// S[r][j] = sum_d A[r][d] * B[j][d] for r < ENC_ROWS, j < L: A is staged in LDS by the caller (covered by the barrier
// after the first block is staged), B (L rows, leading dimension ldb) is walked in blocks of ENC_KB rows.
__device__ __forceinline__ void tile_scores(float* lds, const EncMhaPlan& p, const float* __restrict__ B, long ldb) {
  const int j = threadIdx.x & (ENC_KB - 1), rg = threadIdx.x / ENC_KB;      // rg < 8: rows rg and rg + 8
  for (int kb = 0; kb < p.nkb; ++kb) {
    stage_rows(lds + p.b_off, p.bp, B, ldb, kb * ENC_KB, ENC_KB, p.L, p.dh, p.dhp);
    __syncthreads();
    const f32x4* a0 = reinterpret_cast<const f32x4*>(lds + enc_lds_a(p, rg, 0));
    const f32x4* a1 = reinterpret_cast<const f32x4*>(lds + enc_lds_a(p, rg + ENC_ROWS / 2, 0));
    const f32x4* b = reinterpret_cast<const f32x4*>(lds + enc_lds_b(p, j, 0));
    float s0 = 0.f, s1 = 0.f;
    for (int d4 = 0; d4 < (p.dhp >> 2); ++d4) {          // d ascending: one fixed order of the sum
      const f32x4 k = b[d4], x = a0[d4], y = a1[d4];
      s0 = fmaf(x[0], k[0], s0); s0 = fmaf(x[1], k[1], s0); s0 = fmaf(x[2], k[2], s0); s0 = fmaf(x[3], k[3], s0);
      s1 = fmaf(y[0], k[0], s1); s1 = fmaf(y[1], k[1], s1); s1 = fmaf(y[2], k[2], s1); s1 = fmaf(y[3], k[3], s1);
    }
    lds[enc_lds_s(p, rg, kb * ENC_KB + j)] = s0;
    lds[enc_lds_s(p, rg + ENC_ROWS / 2, kb * ENC_KB + j)] = s1;
    __syncthreads();
  }
}

// acc[k] = sum_{j} S[r][j] * X[j][d], j ascending over all nkb*ENC_KB columns (S and the staged X hold zeros past L), for
// this thread's column d = threadIdx.x % dw and rows r = rg*rpt + k, k < rpt (encoder_plan.h): per 4 keys one 16-byte
// read of each S row (the same address in every lane of a row group) and 4 reads of X shared by the rpt rows.  X (L rows,
// leading dimension ldx) is walked in blocks of ENC_KB rows.  S must be complete (barrier) on entry.
__device__ __forceinline__ void tile_apply(float* lds, const EncMhaPlan& p, const float* __restrict__ X, long ldx,
                                           float (&acc)[ENC_NI]) {
  const int d = threadIdx.x & (p.dw - 1), rg = threadIdx.x / p.dw;
  const bool on = d < p.dh && rg < p.ngroups;
#pragma unroll
  for (int k = 0; k < ENC_NI; ++k) acc[k] = 0.f;
  const float* x = lds + enc_lds_b(p, 0, on ? d : 0);
  const float* s = lds + enc_lds_s(p, on ? rg * p.rpt : 0, 0);
  for (int kb = 0; kb < p.nkb; ++kb) {
    stage_rows(lds + p.b_off, p.bp, X, ldx, kb * ENC_KB, ENC_KB, p.L, p.dh, p.dhp);
    __syncthreads();
    if (on) {
      const int j0 = kb * ENC_KB;
      for (int j = 0; j < ENC_KB; j += 4) {
        const float x0 = x[j * p.bp], x1 = x[(j + 1) * p.bp], x2 = x[(j + 2) * p.bp], x3 = x[(j + 3) * p.bp];
#pragma unroll
        for (int k = 0; k < ENC_NI; ++k) {
          if (k < p.rpt) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(s + k * p.sp + j0 + j);
            float a = acc[k];
            a = fmaf(v[0], x0, a); a = fmaf(v[1], x1, a); a = fmaf(v[2], x2, a); a = fmaf(v[3], x3, a);
            acc[k] = a;
          }
        }
      }
    }
    __syncthreads();
  }
}

// the (ENC_ROWS x dh) tile in `acc` -> rows [row0, ...) of a row-major matrix, scaled
__device__ __forceinline__ void tile_store(const EncMhaPlan& p, const float (&acc)[ENC_NI], float* __restrict__ out, long ld,
                                           int row0, float scale) {
  const int d = threadIdx.x & (p.dw - 1), rg = threadIdx.x / p.dw;
  if (d >= p.dh || rg >= p.ngroups) return;
#pragma unroll
  for (int k = 0; k < ENC_NI; ++k) {
    const int r = rg * p.rpt + k;
    if (k < p.rpt && row0 + r < p.L) out[(long)(row0 + r) * ld + d] = acc[k] * scale;
  }
}

__device__ __forceinline__ float wave_sum(float v) {
  for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  for (int k = 32; k >= 1; k >>= 1) v = fmaxf(v, __shfl_xor(v, k));
  return v;
}

struct MhaArgs {
  const float* qkv;
  const unsigned char* null_tok;
  const unsigned char* keep;
  float keep_scale;
  int causal;
  float* ctx;
  float* prob;
  float* avg;
  int N, L, H, dh;
  int heads_per_wg;            // H where avg is written (one workgroup sums the heads in order), else 1
  const float* bias;           // (Hb, L, L) added to the scaled logits (mha_fwd_kernel<true>), else null
  int Hb;
};

// the logit of (i, j): the scaled score, plus the bias where the kernel has one
template <bool BIAS>
__device__ __forceinline__ float mha_logit(const MhaArgs& a, float s, float scale, int h, int i, int j) {
  if (BIAS) return s * scale + a.bias[enc_bias_index(h, i, j, a.L, a.Hb)];
  return s * scale;
}

// one workgroup: ENC_ROWS query rows of sample n, head h (or all heads in turn)
template <bool BIAS>
__global__ void __launch_bounds__(ENC_THREADS) mha_fwd_kernel(MhaArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const EncMhaPlan p = enc_mha_plan(a.L, a.dh);
  const int rb = blockIdx.x % p.nrb, g = blockIdx.x / p.nrb;
  const int groups = a.H / a.heads_per_wg;
  const int n = g / groups, h_first = (g - n * groups) * a.heads_per_wg;
  if (n >= a.N) return;
  const int i0 = rb * ENC_ROWS;
  const long ld = 3L * a.H * a.dh;
  const float scale = 1.0f / sqrtf((float)a.dh);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int h = h_first; h < h_first + a.heads_per_wg; ++h) {
    stage_rows(lds + p.a_off, p.ap, a.qkv + enc_qkv_index(n, 0, 0, h, 0, a.L, a.H, a.dh), ld, i0, ENC_ROWS, a.L, a.dh, p.dhp);
    tile_scores(lds, p, a.qkv + enc_qkv_index(n, 0, 1, h, 0, a.L, a.H, a.dh), ld);
    // masked, max-subtracted softmax of each row; one wave per row, lanes stride the keys
    for (int r = wave; r < ENC_ROWS; r += ENC_THREADS / 64) {
      const int i = i0 + r;
      float* s = lds + enc_lds_s(p, r, 0);
      if (i >= a.L) {
        for (int j = lane; j < a.L; j += 64) s[j] = 0.f;
        continue;
      }
      const bool null_i = a.null_tok != nullptr && a.null_tok[enc_null_index(n, i, a.L)] != 0;
      float m = -INFINITY;
      for (int j = lane; j < a.L; j += 64) {
        const bool null_j = a.null_tok != nullptr && a.null_tok[enc_null_index(n, j, a.L)] != 0;
        if (enc_allowed(i, j, a.causal, null_i, null_j)) m = fmaxf(m, mha_logit<BIAS>(a, s[j], scale, h, i, j));
      }
      m = wave_max(m);
      float sum = 0.f;
      for (int j = lane; j < a.L; j += 64) {
        const bool null_j = a.null_tok != nullptr && a.null_tok[enc_null_index(n, j, a.L)] != 0;
        const float e =
            enc_allowed(i, j, a.causal, null_i, null_j) ? expf(mha_logit<BIAS>(a, s[j], scale, h, i, j) - m) : 0.f;
        s[j] = e;
        sum += e;
      }
      sum = wave_sum(sum);
      const float inv = sum > 0.f ? 1.0f / sum : 0.f;           // a fully masked row: all-zero probabilities
      for (int j = lane; j < a.L; j += 64) {
        const float pr = s[j] * inv;
        if (a.prob != nullptr) a.prob[enc_prob_index(n, h, i, j, a.L, a.H)] = pr;
        float pd = pr;
        if (a.keep != nullptr) pd = a.keep[enc_prob_index(n, h, i, j, a.L, a.H)] != 0 ? pr * a.keep_scale : 0.f;
        s[j] = pd;
        if (a.avg != nullptr) {                                  // heads in order 0..H-1, by this thread alone
          const long ai = enc_avg_index(n, i, j, a.L);
          float v = (h == 0 ? 0.f : a.avg[ai]) + pd;
          if (h == a.H - 1) v *= 1.0f / (float)a.H;
          a.avg[ai] = v;
        }
      }
    }
    __syncthreads();
    float acc[ENC_NI];
    tile_apply(lds, p, a.qkv + enc_qkv_index(n, 0, 2, h, 0, a.L, a.H, a.dh), ld, acc);
    tile_store(p, acc, a.ctx + enc_ctx_index(n, 0, h, 0, a.L, a.H, a.dh), (long)a.H * a.dh, i0, 1.0f);
  }
}

struct MhaBwdArgs {
  const float* dctx;
  const float* qkv;
  const float* prob;
  const unsigned char* keep;
  float keep_scale;
  float* ds;                   // scratch (N, H, L, L)
  float* dqkv;
  int N, L, H, dh;
};

// A: per block of query rows: dP = (dctx V^T) * keep * scale, dS = P o (dP - rowsum(dP o P)), dQ = dS K / sqrt(dh)
__global__ void __launch_bounds__(ENC_THREADS) mha_bwd_rows_kernel(MhaBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const EncMhaPlan p = enc_mha_plan(a.L, a.dh);
  const int rb = blockIdx.x % p.nrb, g = blockIdx.x / p.nrb;
  const int n = g / a.H, h = g - n * a.H;
  if (n >= a.N) return;
  const int i0 = rb * ENC_ROWS;
  const long ld = 3L * a.H * a.dh, ldc = (long)a.H * a.dh;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  stage_rows(lds + p.a_off, p.ap, a.dctx + enc_ctx_index(n, 0, h, 0, a.L, a.H, a.dh), ldc, i0, ENC_ROWS, a.L, a.dh, p.dhp);
  tile_scores(lds, p, a.qkv + enc_qkv_index(n, 0, 2, h, 0, a.L, a.H, a.dh), ld);
  for (int r = wave; r < ENC_ROWS; r += ENC_THREADS / 64) {
    const int i = i0 + r;
    float* s = lds + enc_lds_s(p, r, 0);
    if (i >= a.L) {
      for (int j = lane; j < a.L; j += 64) s[j] = 0.f;
      continue;
    }
    float dot = 0.f;
    for (int j = lane; j < a.L; j += 64) {
      const long pi = enc_prob_index(n, h, i, j, a.L, a.H);
      float dp = s[j];
      if (a.keep != nullptr) dp = a.keep[pi] != 0 ? dp * a.keep_scale : 0.f;
      s[j] = dp;
      dot = fmaf(dp, a.prob[pi], dot);
    }
    dot = wave_sum(dot);
    for (int j = lane; j < a.L; j += 64) {
      const long pi = enc_prob_index(n, h, i, j, a.L, a.H);
      const float d = a.prob[pi] * (s[j] - dot);
      s[j] = d;
      a.ds[pi] = d;
    }
  }
  __syncthreads();
  float acc[ENC_NI];
  tile_apply(lds, p, a.qkv + enc_qkv_index(n, 0, 1, h, 0, a.L, a.H, a.dh), ld, acc);
  tile_store(p, acc, a.dqkv + enc_qkv_index(n, 0, 0, h, 0, a.L, a.H, a.dh), ld, i0, 1.0f / sqrtf((float)a.dh));
}

// B: per block of key rows j: dK[j] = sum_i dS[i][j] Q[i] / sqrt(dh), dV[j] = sum_i P_d[i][j] dctx[i], i ascending: the sum
// over the query rows stays inside one workgroup
__global__ void __launch_bounds__(ENC_THREADS) mha_bwd_cols_kernel(MhaBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const EncMhaPlan p = enc_mha_plan(a.L, a.dh);
  const int rb = blockIdx.x % p.nrb, g = blockIdx.x / p.nrb;
  const int n = g / a.H, h = g - n * a.H;
  if (n >= a.N) return;
  const int j0 = rb * ENC_ROWS;
  const long ld = 3L * a.H * a.dh, ldc = (long)a.H * a.dh;
  const int total = ENC_ROWS * p.nkb * ENC_KB;            // every column tile_apply reads, zeros past L
  for (int pass = 0; pass < 2; ++pass) {
    // S[r][i] = M[i][j0 + r], M = dS (pass 0) or the dropped-out probabilities (pass 1)
    for (int e = threadIdx.x; e < total; e += ENC_THREADS) {
      const int r = e % ENC_ROWS, i = e / ENC_ROWS;
      float v = 0.f;
      if (i < a.L && j0 + r < a.L) {
        const long pi = enc_prob_index(n, h, i, j0 + r, a.L, a.H);
        if (pass == 0) v = a.ds[pi];
        else {
          v = a.prob[pi];
          if (a.keep != nullptr) v = a.keep[pi] != 0 ? v * a.keep_scale : 0.f;
        }
      }
      lds[enc_lds_s(p, r, i)] = v;
    }
    __syncthreads();
    float acc[ENC_NI];
    if (pass == 0) {
      tile_apply(lds, p, a.qkv + enc_qkv_index(n, 0, 0, h, 0, a.L, a.H, a.dh), ld, acc);
      tile_store(p, acc, a.dqkv + enc_qkv_index(n, 0, 1, h, 0, a.L, a.H, a.dh), ld, j0, 1.0f / sqrtf((float)a.dh));
    } else {
      tile_apply(lds, p, a.dctx + enc_ctx_index(n, 0, h, 0, a.L, a.H, a.dh), ldc, acc);
      tile_store(p, acc, a.dqkv + enc_qkv_index(n, 0, 2, h, 0, a.L, a.H, a.dh), ld, j0, 1.0f);
    }
    // (tile_apply ends with a barrier: S may be rewritten)
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// LayerNorm
// ---------------------------------------------------------------------------------------------------------------------
// sum over the workgroup, the same value in every thread: lanes by butterfly, then the 4 wave sums in order
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();                                   // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ void __launch_bounds__(ENC_THREADS) ln_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             float eps, float* __restrict__ out, float* __restrict__ mean,
                                                             float* __restrict__ rstd, int R, int D) {
  __shared__ float red[4];
  for (int row = blockIdx.x; row < R; row += gridDim.x) {
    const long base = (long)row * D;
    float x[ENC_LN_PER_THREAD];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < ENC_LN_PER_THREAD; ++k) {
      const int c = threadIdx.x + k * ENC_THREADS;
      x[k] = 0.f;
      if (c < D) x[k] = b != nullptr ? a[base + c] + b[base + c] : a[base + c];
      s += x[k];
    }
    const float mu = block_sum(s, red) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < ENC_LN_PER_THREAD; ++k) {
      const int c = threadIdx.x + k * ENC_THREADS;
      const float d = c < D ? x[k] - mu : 0.f;
      q = fmaf(d, d, q);
    }
    const float rs = 1.0f / sqrtf(block_sum(q, red) / (float)D + eps);
#pragma unroll
    for (int k = 0; k < ENC_LN_PER_THREAD; ++k) {
      const int c = threadIdx.x + k * ENC_THREADS;
      if (c < D) out[base + c] = (x[k] - mu) * rs * gamma[c] + beta[c];
    }
    if (threadIdx.x == 0) { mean[row] = mu; rstd[row] = rs; }
  }
}

// wave w of the grid: rows [w*rpw, min(R, (w+1)*rpw)): dx of each, and its partial sums of dgamma / dbeta (rows ascending)
// in slot w of the slab.  A row lives in the registers of one wave (lane l: columns l + 64*k), so nothing waits at a
// workgroup barrier.
__global__ void __launch_bounds__(ENC_THREADS) ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ a,
                                                             const float* __restrict__ b, const float* __restrict__ gamma,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd,
                                                             float* __restrict__ dx, float* __restrict__ part, int R, int D,
                                                             int rpw) {
  const int lane = threadIdx.x & 63, w = blockIdx.x * ENC_LN_WAVES + (threadIdx.x >> 6);
  const int kmax = (D + 63) >> 6;
  float dg[ENC_LN_PER_LANE], db[ENC_LN_PER_LANE];
#pragma unroll
  for (int k = 0; k < ENC_LN_PER_LANE; ++k) { dg[k] = 0.f; db[k] = 0.f; }
  const long r0 = (long)w * rpw, r1 = r0 + rpw < R ? r0 + rpw : R;
  for (long row = r0; row < r1; ++row) {
    const long base = row * D;
    const float mu = mean[row], rs = rstd[row];
    float xh[ENC_LN_PER_LANE], g[ENC_LN_PER_LANE];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < ENC_LN_PER_LANE; ++k) {
      xh[k] = 0.f; g[k] = 0.f;
      const int c = lane + 64 * k;
      if (k < kmax && c < D) {
        const float x = b != nullptr ? a[base + c] + b[base + c] : a[base + c];
        const float d = dy[base + c];
        xh[k] = (x - mu) * rs;
        g[k] = d * gamma[c];
        dg[k] = fmaf(d, xh[k], dg[k]);
        db[k] += d;
        s1 += g[k];
        s2 = fmaf(g[k], xh[k], s2);
      }
    }
    const float m1 = wave_sum(s1) / (float)D;
    const float m2 = wave_sum(s2) / (float)D;
#pragma unroll
    for (int k = 0; k < ENC_LN_PER_LANE; ++k) {
      const int c = lane + 64 * k;
      if (k < kmax && c < D) dx[base + c] = rs * (g[k] - m1 - xh[k] * m2);
    }
  }
#pragma unroll
  for (int k = 0; k < ENC_LN_PER_LANE; ++k) {
    const int c = lane + 64 * k;
    if (k < kmax && c < D) {
      part[((long)w * 2 + 0) * D + c] = dg[k];
      part[((long)w * 2 + 1) * D + c] = db[k];
    }
  }
}

// out[c] = sum_b part[b][c] over the slots b < nslots, c < W (the first `split` columns to out0, the rest to out1)
__global__ void __launch_bounds__(ENC_THREADS) enc_slab_sum_kernel(const float* __restrict__ part, int nslots, int W,
                                                                   float* __restrict__ out0, float* __restrict__ out1,
                                                                   int split) {
  // 16 columns per workgroup; thread group g = tid / 16 adds the slots g, g + 16, ... in order, then thread g = 0 adds
  // the 16 group sums in order: a fixed order, 1/16 of the serial chain
  __shared__ float red[16][17];
  const int cl = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  float s = 0.f;
  if (c < W)
    for (int b = g; b < nslots; b += 16) s += part[(long)b * W + c];
  red[g][cl] = s;
  __syncthreads();
  if (g == 0 && c < W) {
    float t = red[0][cl];
    for (int k = 1; k < 16; ++k) t += red[k][cl];
    if (c < split) out0[c] = t;
    else out1[c - split] = t;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// tokens
// ---------------------------------------------------------------------------------------------------------------------
// fwd: tok[n, cls + m*T' + t, v*C + c] = x[n*M + m, c, t, v] + pe[l, v*C + c]; bwd (x = dx written, tok = dtok read)
template <bool BWD>
__global__ void __launch_bounds__(ENC_THREADS) tokens_kernel(float* __restrict__ x, const float* __restrict__ cls,
                                                             const float* __restrict__ pe, float* __restrict__ tok,
                                                             int N, int M, int C, int Tp, int V, int has_cls) {
  __shared__ float tile[ENC_TOK_LDS];
  const EncTokPlan p = enc_tok_plan(C, Tp, V);
  const int tb = blockIdx.x % p.ntb, nm = blockIdx.x / p.ntb;
  if (nm >= N * M) return;
  const int n = nm / M, m = nm - n * M;
  const int D = V * C, L = M * Tp + has_cls;
  const int t0 = tb * p.tt, nt = min(p.tt, Tp - t0);
  const int run = nt * V;                                       // contiguous floats of one channel
  if (!BWD) {
    for (int e = threadIdx.x; e < C * run; e += ENC_THREADS) {
      const int c = e / run, q = e - c * run;
      tile[c * p.w + q] = x[enc_x_index(nm, c, t0, 0, C, Tp, V) + q];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nt * D; e += ENC_THREADS) {
      const int tt = e / D, f = e - tt * D;
      const int v = f / C, c = f - v * C;
      const int l = has_cls + m * Tp + t0 + tt;
      float val = tile[c * p.w + tt * V + v];
      if (pe != nullptr) val += pe[(long)l * D + f];
      tok[enc_tok_index(n, l, f, L, D)] = val;
    }
    if (has_cls && m == 0 && tb == 0) {
      for (int f = threadIdx.x; f < D; f += ENC_THREADS)
        tok[enc_tok_index(n, 0, f, L, D)] = pe != nullptr ? cls[f] + pe[f] : cls[f];
    }
  } else {
    for (int e = threadIdx.x; e < nt * D; e += ENC_THREADS) {
      const int tt = e / D, f = e - tt * D;
      const int v = f / C, c = f - v * C;
      const int l = has_cls + m * Tp + t0 + tt;
      tile[c * p.w + tt * V + v] = tok[enc_tok_index(n, l, f, L, D)];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < C * run; e += ENC_THREADS) {
      const int c = e / run, q = e - c * run;
      x[enc_x_index(nm, c, t0, 0, C, Tp, V) + q] = tile[c * p.w + q];
    }
  }
}

// dpe[l, f] = sum_n dtok[n, l, f] (n ascending) for l < L, 0 for L <= l < pe_rows; dcls[f] = sum_n dtok[n, 0, f]
__global__ void __launch_bounds__(ENC_THREADS) tokens_bwd_sums_kernel(const float* __restrict__ dtok, float* __restrict__ dcls,
                                                                      float* __restrict__ dpe, int N, int L, int D,
                                                                      int rows) {
  const long e = (long)blockIdx.x * ENC_THREADS + threadIdx.x;
  if (e >= (long)rows * D) return;
  const int l = (int)(e / D), f = (int)(e - (long)l * D);
  float s = 0.f;
  if (l < L)
    for (int n = 0; n < N; ++n) s += dtok[enc_tok_index(n, l, f, L, D)];
  if (dpe != nullptr) dpe[e] = s;
  if (dcls != nullptr && l == 0) dcls[f] = s;
}

// spatial tokens of aagcn_v24, fwd: tok[n*T' + t, cls + m*V + v, c] = x[n*M + m, c, t, v] + pe[cls + m*V + v, c]; bwd
// (x = dx written, tok = dtok read).  The tile and its two walks are tokens_kernel's; the outer index differs.
template <bool BWD>
__global__ void __launch_bounds__(ENC_THREADS) stokens_kernel(float* __restrict__ x, const float* __restrict__ cls,
                                                              const float* __restrict__ pe, float* __restrict__ tok,
                                                              int N, int M, int C, int Tp, int V, int has_cls) {
  __shared__ float tile[ENC_TOK_LDS];
  const EncTokPlan p = enc_tok_plan(C, Tp, V);
  const int tb = blockIdx.x % p.ntb, nm = blockIdx.x / p.ntb;
  if (nm >= N * M) return;
  const int n = nm / M, m = nm - n * M;
  const int D = V * C, L = M * V + has_cls;
  const int t0 = tb * p.tt, nt = min(p.tt, Tp - t0);
  const int run = nt * V;                                       // contiguous floats of one channel
  const int l0 = has_cls + m * V;                               // first token of person m
  if (!BWD) {
    for (int e = threadIdx.x; e < C * run; e += ENC_THREADS) {
      const int c = e / run, q = e - c * run;
      tile[c * p.w + q] = x[enc_x_index(nm, c, t0, 0, C, Tp, V) + q];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nt * D; e += ENC_THREADS) {
      const int tt = e / D, f = e - tt * D;                     // f = v*C + c: token l0 + v, feature c
      const int v = f / C, c = f - v * C;
      float val = tile[c * p.w + tt * V + v];
      if (pe != nullptr) val += pe[(long)l0 * C + f];
      tok[enc_stok_index(n, t0 + tt, l0, 0, Tp, L, C) + f] = val;
    }
    if (has_cls && m == 0) {
      for (int e = threadIdx.x; e < nt * C; e += ENC_THREADS) {
        const int tt = e / C, c = e - tt * C;
        tok[enc_stok_index(n, t0 + tt, 0, c, Tp, L, C)] = pe != nullptr ? cls[c] + pe[c] : cls[c];
      }
    }
  } else {
    for (int e = threadIdx.x; e < nt * D; e += ENC_THREADS) {
      const int tt = e / D, f = e - tt * D;
      const int v = f / C, c = f - v * C;
      tile[c * p.w + tt * V + v] = tok[enc_stok_index(n, t0 + tt, l0, 0, Tp, L, C) + f];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < C * run; e += ENC_THREADS) {
      const int c = e / run, q = e - c * run;
      x[enc_x_index(nm, c, t0, 0, C, Tp, V) + q] = tile[c * p.w + q];
    }
  }
}

// stage 1 of a sum over sequences: part[slot, col] = sum of src[s, col] over the slot's sequences s (ascending), col < W;
// a sequence of src is `stride` floats long (W <= stride: the first W columns are summed)
__global__ void __launch_bounds__(ENC_THREADS) seq_partial_kernel(const float* __restrict__ src, float* __restrict__ part,
                                                                  long S, long stride, long W) {
  const long col = (long)blockIdx.x * ENC_THREADS + threadIdx.x;
  const long slot = blockIdx.y;
  if (col >= W) return;
  const long s0 = slot * ENC_SEQ_CHUNK, s1 = s0 + ENC_SEQ_CHUNK < S ? s0 + ENC_SEQ_CHUNK : S;
  float acc = 0.f;
  for (long s = s0; s < s1; ++s) acc += src[s * stride + col];
  part[enc_seq_slab_index(slot, col, W)] = acc;
}

// stage 1 of the bias gradient: part[slot, (hb, i, j)] = sum over the slot's sequences n (ascending) and, when Hb = 1,
// over the heads h (ascending inside n) of dS[n, h, i, j]
__global__ void __launch_bounds__(ENC_THREADS) bias_partial_kernel(const float* __restrict__ ds, float* __restrict__ part,
                                                                   int N, int L, int H, int Hb) {
  const long LL = (long)L * L, W = (long)Hb * LL;
  const long col = (long)blockIdx.x * ENC_THREADS + threadIdx.x;
  const long slot = blockIdx.y;
  if (col >= W) return;
  const int hb = (int)(col / LL);
  const long ij = col - (long)hb * LL;
  const int h0 = Hb == 1 ? 0 : hb, h1 = Hb == 1 ? H : hb + 1;
  const long n0 = slot * ENC_SEQ_CHUNK, n1 = n0 + ENC_SEQ_CHUNK < N ? n0 + ENC_SEQ_CHUNK : N;
  float acc = 0.f;
  for (long n = n0; n < n1; ++n)
    for (int h = h0; h < h1; ++h) acc += ds[enc_prob_index((int)n, h, 0, 0, L, H) + ij];
  part[enc_seq_slab_index(slot, col, W)] = acc;
}

__global__ void __launch_bounds__(ENC_THREADS) enc_zero_kernel(float* __restrict__ out, long count) {
  const long e = (long)blockIdx.x * ENC_THREADS + threadIdx.x;
  if (e < count) out[e] = 0.f;
}

// out[col] = sum over the S sequences of src[s, col], col < W, through the slab `part` (enc_seq_slots(S) x W floats)
int seq_sum(const float* src, float* part, float* out, long S, long stride, long W, hipStream_t stream) {
  const long slots = enc_seq_slots(S);          // <= ENC_SEQ_MAX_SLOTS: the y dimension of the grid
  hipLaunchKernelGGL(seq_partial_kernel, dim3((unsigned)((W + ENC_THREADS - 1) / ENC_THREADS), (unsigned)slots),
                     dim3(ENC_THREADS), 0, stream, src, part, S, stride, W);
  int rc = agcn_check_launch();
  if (rc != AGCN_OK) return rc;
  hipLaunchKernelGGL(enc_slab_sum_kernel, dim3((unsigned)((W + 15) / 16)), dim3(ENC_THREADS), 0, stream,
                     (const float*)part, (int)slots, (int)W, out, out, (int)W);
  return agcn_check_launch();
}

int mha_grid(int N, int L, int H, int dh, int groups_per_sample, long* grid) {
  const EncMhaPlan p = enc_mha_plan(L, dh);
  if (enc_mha_lds_bytes(p) > ENC_LDS_LIMIT) return AGCN_ERR_UNSUPPORTED;
  *grid = (long)p.nrb * N * groups_per_sample;
  if (*grid > 0x7fffffffL || (long)N * H * L * L > (1L << 40)) return AGCN_ERR_UNSUPPORTED;
  return AGCN_OK;
}

// agcn_mha_fwd (bias null) and agcn_mha_bias_fwd: one launcher, the bias in the instantiation of its own
int mha_fwd_launch(const float* qkv, const float* bias, int Hb, const unsigned char* null_tok, int causal,
                   const unsigned char* keep, float keep_scale, float* ctx, float* prob, float* avg, int N, int L, int H,
                   int dh, hipStream_t stream) {
  if (!enc_mha_domain(N, L, H, dh)) return AGCN_ERR_UNSUPPORTED;
  long grid;
  const int per_wg = avg != nullptr ? H : 1;
  int rc = mha_grid(N, L, H, dh, H / per_wg, &grid);
  if (rc != AGCN_OK) return rc;
  const EncMhaPlan p = enc_mha_plan(L, dh);
  MhaArgs a = {qkv, null_tok, keep, keep_scale, causal, ctx, prob, avg, N, L, H, dh, per_wg, bias, Hb};
  AGCN_NOTE_KERNEL("mha_fwd_kernel L=%d dh=%d rows=%d kb=%d lds=%ld heads/wg=%d%s", L, dh, ENC_ROWS, ENC_KB,
                   enc_mha_lds_bytes(p), per_wg, bias != nullptr ? (Hb == 1 ? " bias=1" : " bias=H") : "");
  if (bias != nullptr)
    return agcn_launch_big<mha_fwd_kernel<true>>(dim3((unsigned)grid), dim3(ENC_THREADS), (size_t)enc_mha_lds_bytes(p),
                                                 stream, a);
  return agcn_launch_big<mha_fwd_kernel<false>>(dim3((unsigned)grid), dim3(ENC_THREADS), (size_t)enc_mha_lds_bytes(p),
                                                stream, a);
}

}  // namespace

extern "C" int agcn_mha_fwd(const float* qkv, const unsigned char* null_tok, int causal, const unsigned char* keep,
                            float keep_scale, float* ctx, float* prob, float* avg, int N, int L, int H, int dh,
                            void* stream) {
  if (!qkv || !ctx || N < 1 || L < 1 || H < 1 || dh < 1 || causal < 0 || causal > 2) return AGCN_ERR_ARG;
  return mha_fwd_launch(qkv, nullptr, 1, null_tok, causal, keep, keep_scale, ctx, prob, avg, N, L, H, dh,
                        (hipStream_t)stream);
}

extern "C" int agcn_mha_bias_fwd(const float* qkv, const float* bias, int Hb, const unsigned char* null_tok, int causal,
                                 const unsigned char* keep, float keep_scale, float* ctx, float* prob, float* avg, int N,
                                 int L, int H, int dh, void* stream) {
  if (!qkv || !bias || !ctx || N < 1 || L < 1 || H < 1 || dh < 1 || causal < 0 || causal > 2) return AGCN_ERR_ARG;
  if (!enc_bias_heads_ok(Hb, H)) return AGCN_ERR_ARG;
  return mha_fwd_launch(qkv, bias, Hb, null_tok, causal, keep, keep_scale, ctx, prob, avg, N, L, H, dh,
                        (hipStream_t)stream);
}

extern "C" size_t agcn_mha_bias_grad_workspace(int N, int L, int H, int Hb) {
  return enc_bias_grad_domain(N, L, H, Hb) ? (size_t)enc_bias_grad_ws_bytes(N, L, H, Hb) : 0;
}

extern "C" int agcn_mha_bias_grad(const float* ds, float* dbias, void* ws, size_t ws_bytes, int N, int L, int H, int Hb,
                                  void* stream) {
  if (!ds || !dbias || !ws || N < 1 || L < 1 || H < 1 || !enc_bias_heads_ok(Hb, H)) return AGCN_ERR_ARG;
  if (!enc_bias_grad_domain(N, L, H, Hb)) return AGCN_ERR_UNSUPPORTED;
  if ((long)ws_bytes < enc_bias_grad_ws_bytes(N, L, H, Hb)) return AGCN_ERR_WORKSPACE;
  const long W = (long)Hb * L * L, slots = enc_seq_slots(N);
  AGCN_NOTE_KERNEL("bias_partial_kernel+enc_slab_sum_kernel N=%d L=%d H=%d Hb=%d slots=%ld", N, L, H, Hb, slots);
  hipLaunchKernelGGL(bias_partial_kernel, dim3((unsigned)((W + ENC_THREADS - 1) / ENC_THREADS), (unsigned)slots),
                     dim3(ENC_THREADS), 0, (hipStream_t)stream, ds, (float*)ws, N, L, H, Hb);
  int rc = agcn_check_launch();
  if (rc != AGCN_OK) return rc;
  hipLaunchKernelGGL(enc_slab_sum_kernel, dim3((unsigned)((W + 15) / 16)), dim3(ENC_THREADS), 0, (hipStream_t)stream,
                     (const float*)ws, (int)slots, (int)W, dbias, dbias, (int)W);
  return agcn_check_launch();
}

extern "C" int agcn_mha_bwd(const float* dctx, const float* qkv, const float* prob, const unsigned char* keep,
                            float keep_scale, float* dqkv, void* ws, size_t ws_bytes, int N, int L, int H, int dh,
                            void* stream) {
  if (!dctx || !qkv || !prob || !dqkv || !ws || N < 1 || L < 1 || H < 1 || dh < 1) return AGCN_ERR_ARG;
  if (!enc_mha_domain(N, L, H, dh)) return AGCN_ERR_UNSUPPORTED;
  if ((long)ws_bytes < enc_mha_bwd_ws_bytes(N, L, H)) return AGCN_ERR_WORKSPACE;
  long grid;
  int rc = mha_grid(N, L, H, dh, H, &grid);
  if (rc != AGCN_OK) return rc;
  const EncMhaPlan p = enc_mha_plan(L, dh);
  MhaBwdArgs a = {dctx, qkv, prob, keep, keep_scale, (float*)ws, dqkv, N, L, H, dh};
  AGCN_NOTE_KERNEL("mha_bwd_rows_kernel+mha_bwd_cols_kernel L=%d dh=%d lds=%ld", L, dh, enc_mha_lds_bytes(p));
  rc = agcn_launch_big<mha_bwd_rows_kernel>(dim3((unsigned)grid), dim3(ENC_THREADS), (size_t)enc_mha_lds_bytes(p),
                                            (hipStream_t)stream, a);
  if (rc != AGCN_OK) return rc;
  return agcn_launch_big<mha_bwd_cols_kernel>(dim3((unsigned)grid), dim3(ENC_THREADS), (size_t)enc_mha_lds_bytes(p),
                                              (hipStream_t)stream, a);
}

extern "C" int agcn_ln_fwd(const float* a, const float* b, const float* gamma, const float* beta, float eps, float* out,
                           float* mean, float* rstd, long R, int D, void* stream) {
  if (!a || !gamma || !beta || !out || !mean || !rstd || R < 1 || D < 1 || !(eps >= 0.f)) return AGCN_ERR_ARG;
  if (!enc_ln_domain(R, D)) return AGCN_ERR_UNSUPPORTED;
  const int grid = (int)(R < 4096 ? R : 4096);
  AGCN_NOTE_KERNEL("ln_fwd_kernel R=%ld D=%d", R, D);
  hipLaunchKernelGGL(ln_fwd_kernel, dim3(grid), dim3(ENC_THREADS), 0, (hipStream_t)stream, a, b, gamma, beta, eps, out,
                     mean, rstd, (int)R, D);
  return agcn_check_launch();
}

extern "C" int agcn_ln_bwd(const float* dy, const float* a, const float* b, const float* gamma, const float* mean,
                           const float* rstd, float* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, long R,
                           int D, void* stream) {
  if (!dy || !a || !gamma || !mean || !rstd || !dx || !dgamma || !dbeta || !ws || R < 1 || D < 1) return AGCN_ERR_ARG;
  if (!enc_ln_domain(R, D)) return AGCN_ERR_UNSUPPORTED;
  if ((long)ws_bytes < enc_ln_bwd_ws_bytes(R, D)) return AGCN_ERR_WORKSPACE;
  const EncLnPlan p = enc_ln_plan(R);
  AGCN_NOTE_KERNEL("ln_bwd_kernel R=%ld D=%d blocks=%d rows/wave=%d", R, D, p.nblocks, p.rows_per_wave);
  hipLaunchKernelGGL(ln_bwd_kernel, dim3(p.nblocks), dim3(ENC_THREADS), 0, (hipStream_t)stream, dy, a, b, gamma, mean, rstd,
                     dx, (float*)ws, (int)R, D, p.rows_per_wave);
  int rc = agcn_check_launch();
  if (rc != AGCN_OK) return rc;
  hipLaunchKernelGGL(enc_slab_sum_kernel, dim3((2 * D + 15) / 16), dim3(ENC_THREADS), 0,
                     (hipStream_t)stream, (const float*)ws, p.nslots, 2 * D, dgamma, dbeta, D);
  return agcn_check_launch();
}

extern "C" int agcn_tokens_fwd(const float* x, const float* cls, const float* pe, int pe_rows, float* tok, int N, int M,
                               int C, int Tp, int V, void* stream) {
  if (!x || !tok || N < 1 || M < 1 || C < 1 || Tp < 1 || V < 1) return AGCN_ERR_ARG;
  const int has_cls = cls != nullptr;
  if (!enc_tok_domain(N, M, C, Tp, V, has_cls)) return AGCN_ERR_UNSUPPORTED;
  if (pe != nullptr && pe_rows < M * Tp + has_cls) return AGCN_ERR_ARG;
  const EncTokPlan p = enc_tok_plan(C, Tp, V);
  if (p.lds_floats > ENC_TOK_LDS) return AGCN_ERR_UNSUPPORTED;
  AGCN_NOTE_KERNEL("tokens_kernel<fwd> C=%d T'=%d V=%d tt=%d", C, Tp, V, p.tt);
  hipLaunchKernelGGL(tokens_kernel<false>, dim3((unsigned)((long)p.ntb * N * M)), dim3(ENC_THREADS), 0, (hipStream_t)stream,
                     const_cast<float*>(x), cls, pe, tok, N, M, C, Tp, V, has_cls);
  return agcn_check_launch();
}

extern "C" int agcn_tokens_bwd(const float* dtok, float* dx, float* dcls, float* dpe, int has_cls, int pe_rows, int N,
                               int M, int C, int Tp, int V, void* stream) {
  if (!dtok || N < 1 || M < 1 || C < 1 || Tp < 1 || V < 1 || (has_cls != 0 && has_cls != 1)) return AGCN_ERR_ARG;
  if (dcls != nullptr && !has_cls) return AGCN_ERR_ARG;
  if (!enc_tok_domain(N, M, C, Tp, V, has_cls)) return AGCN_ERR_UNSUPPORTED;
  const int L = M * Tp + has_cls, D = V * C;
  if (dpe != nullptr && (pe_rows < L || pe_rows > 65536)) return AGCN_ERR_ARG;
  const EncTokPlan p = enc_tok_plan(C, Tp, V);
  if (p.lds_floats > ENC_TOK_LDS) return AGCN_ERR_UNSUPPORTED;
  AGCN_NOTE_KERNEL("tokens_kernel<bwd> C=%d T'=%d V=%d tt=%d", C, Tp, V, p.tt);
  if (dx != nullptr) {
    hipLaunchKernelGGL(tokens_kernel<true>, dim3((unsigned)((long)p.ntb * N * M)), dim3(ENC_THREADS), 0,
                       (hipStream_t)stream, dx, (const float*)nullptr, (const float*)nullptr, const_cast<float*>(dtok), N, M,
                       C, Tp, V, has_cls);
    int rc = agcn_check_launch();
    if (rc != AGCN_OK) return rc;
  }
  if (dcls != nullptr || dpe != nullptr) {
    const int rows = dpe != nullptr ? pe_rows : 1;
    const long total = (long)rows * D;
    hipLaunchKernelGGL(tokens_bwd_sums_kernel, dim3((unsigned)((total + ENC_THREADS - 1) / ENC_THREADS)), dim3(ENC_THREADS),
                       0, (hipStream_t)stream, dtok, dcls, dpe, N, L, D, rows);
    return agcn_check_launch();
  }
  return AGCN_OK;
}

extern "C" int agcn_tokens_spatial_fwd(const float* x, const float* cls, const float* pe, int pe_rows, float* tok, int N,
                                       int M, int C, int Tp, int V, void* stream) {
  if (!x || !tok || N < 1 || M < 1 || C < 1 || Tp < 1 || V < 1) return AGCN_ERR_ARG;
  const int has_cls = cls != nullptr;
  if (!enc_stok_domain(N, M, C, Tp, V, has_cls)) return AGCN_ERR_UNSUPPORTED;
  if (pe != nullptr && pe_rows < M * V + has_cls) return AGCN_ERR_ARG;
  const EncTokPlan p = enc_tok_plan(C, Tp, V);
  if (p.lds_floats > ENC_TOK_LDS) return AGCN_ERR_UNSUPPORTED;
  AGCN_NOTE_KERNEL("stokens_kernel<fwd> C=%d T'=%d V=%d tt=%d", C, Tp, V, p.tt);
  hipLaunchKernelGGL(stokens_kernel<false>, dim3((unsigned)((long)p.ntb * N * M)), dim3(ENC_THREADS), 0,
                     (hipStream_t)stream, const_cast<float*>(x), cls, pe, tok, N, M, C, Tp, V, has_cls);
  return agcn_check_launch();
}

extern "C" size_t agcn_tokens_spatial_bwd_workspace(int N, int M, int C, int Tp, int V, int has_cls) {
  return enc_stok_domain(N, M, C, Tp, V, has_cls) ? (size_t)enc_stok_bwd_ws_bytes(N, M, C, Tp, V, has_cls) : 0;
}

extern "C" int agcn_tokens_spatial_bwd(const float* dtok, float* dx, float* dcls, float* dpe, int has_cls, int pe_rows,
                                       void* ws, size_t ws_bytes, int N, int M, int C, int Tp, int V, void* stream) {
  if (!dtok || N < 1 || M < 1 || C < 1 || Tp < 1 || V < 1 || (has_cls != 0 && has_cls != 1)) return AGCN_ERR_ARG;
  if (dcls != nullptr && !has_cls) return AGCN_ERR_ARG;
  if ((dcls != nullptr || dpe != nullptr) && !ws) return AGCN_ERR_ARG;
  if (!enc_stok_domain(N, M, C, Tp, V, has_cls)) return AGCN_ERR_UNSUPPORTED;
  const int L = M * V + has_cls;
  if (dpe != nullptr && (pe_rows < L || pe_rows > 65536)) return AGCN_ERR_ARG;
  if ((dcls != nullptr || dpe != nullptr) && (long)ws_bytes < enc_stok_bwd_ws_bytes(N, M, C, Tp, V, has_cls))
    return AGCN_ERR_WORKSPACE;
  const EncTokPlan p = enc_tok_plan(C, Tp, V);
  if (p.lds_floats > ENC_TOK_LDS) return AGCN_ERR_UNSUPPORTED;
  AGCN_NOTE_KERNEL("stokens_kernel<bwd> C=%d T'=%d V=%d tt=%d", C, Tp, V, p.tt);
  hipStream_t st = (hipStream_t)stream;
  if (dx != nullptr) {
    hipLaunchKernelGGL(stokens_kernel<true>, dim3((unsigned)((long)p.ntb * N * M)), dim3(ENC_THREADS), 0, st, dx,
                       (const float*)nullptr, (const float*)nullptr, const_cast<float*>(dtok), N, M, C, Tp, V, has_cls);
    int rc = agcn_check_launch();
    if (rc != AGCN_OK) return rc;
  }
  const long S = (long)N * Tp, LC = (long)L * C;
  if (dpe != nullptr) {
    // rows < L: the sum over the sequences; the table rows behind them: zeros; dcls is row 0 summed once more, the
    // same additions in the same order
    int rc = seq_sum(dtok, (float*)ws, dpe, S, LC, LC, st);
    if (rc != AGCN_OK) return rc;
    const long tail = ((long)pe_rows - L) * C;
    if (tail > 0) {
      hipLaunchKernelGGL(enc_zero_kernel, dim3((unsigned)((tail + ENC_THREADS - 1) / ENC_THREADS)), dim3(ENC_THREADS), 0,
                         st, dpe + LC, tail);
      rc = agcn_check_launch();
      if (rc != AGCN_OK) return rc;
    }
  }
  if (dcls != nullptr) return seq_sum(dtok, (float*)ws, dcls, S, LC, C, st);
  return AGCN_OK;
}
