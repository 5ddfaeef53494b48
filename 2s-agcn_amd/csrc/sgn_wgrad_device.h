// The reduction kernels of the SGN parameter gradients and their host launch helpers, shared by sgn_wgrad.hip (base SGN)
// and sgn_v15_wgrad.hip (SGN v15): a tape of row-major operand pairs -> X^T . Z and column sums, over row splits into
// partials and then the ascending-order add.
//   sgn_wgrad_gemm_kernel   dW (K, N) = X^T . Z over the rows of one split, one wave per 32 x (32..128) strip of dW,
//                           exact-f32 MFMA (v_mfma_f32_32x32x2_f32), both operands read along their rows straight from
//                           the tape; plain or grouped rows (the three taps of the temporal convolution).
//   sgn_wgrad_colsum_kernel column sums over the rows of one split (32 columns x 8 row phases per workgroup, the phases
//                           added in ascending order): biases, and tables summed over frames / clips as strided views.
//   sgn_wgrad_first_kernel  the 3 x 64 first embedding layers (K = 3: VALU);  sgn_wgrad_aff_kernel  the folded norm_data.
//   sgn_wgrad_finalize_kernel  adds the partials of the splits in ascending order into the image.
// Every sum runs in a fixed order (rows ascending inside a split, splits ascending), no atomics: the same inputs give the
// same bits.  Splits, strips and every guarded index: sgn_wgrad_plan.h.  The kernels are static or templates: each of
// the two sources that include this header carries its own copy.
#pragma once
#include "agcn_common.h"
#include "sgn_wgrad_plan.h"

struct SgnWgradGemm {
  const float* X;
  const float* Z;
  float* part;                 // (splits, K, N)
  long ldx, ldz;
  int K, N;                    // K a multiple of 32; any N >= 1
  int tile_blocks;             // workgroups of SGN_WAVES tiles per split
  long R, rows;                // rows in all, rows per split
  SgnWgradRows g;
};

template <int NB>
__global__ __launch_bounds__(SGN_THREADS) void sgn_wgrad_gemm_kernel(SgnWgradGemm p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int strips = sgn_wgrad_strips(p.N);
  const long s = blockIdx.x / p.tile_blocks;
  const int tile = (int)(blockIdx.x % p.tile_blocks) * SGN_WAVES + wave;
  if (tile >= sgn_wgrad_tiles(p.K, p.N)) return;                 // the same for a whole wave
  const int k0 = tile / strips * SGN_WGRAD_TILE, n0 = tile % strips * (NB * SGN_WGRAD_TILE);
  bool col[NB];                                                  // N is no multiple of the strip: these lanes read and write nothing
#pragma unroll
  for (int i = 0; i < NB; ++i) col[i] = n0 + i * SGN_WGRAD_TILE + r < p.N;
  const long begin = s * p.rows;
  const long end = begin + p.rows < p.R ? begin + p.rows : p.R;
  long row = begin + h;                                          // lanes 0..31: the even row of a pair, lanes 32..63: the odd one
  long grp = row / p.g.group_rows, u = row % p.g.group_rows;
  f32x16 acc[NB] = {};
  for (long r0 = begin; r0 < end; r0 += 2) {
    float a = 0.f, b[NB] = {};
    if (row < end) {                                             // an odd number of rows: the last pair's second row is zero
      a = p.X[(grp * p.g.x_group_stride + u + p.g.x_off) * p.ldx + k0 + r];
      const float* z = p.Z + (grp * p.g.z_group_stride + u) * p.ldz + n0 + r;
#pragma unroll
      for (int i = 0; i < NB; ++i)
        if (col[i]) b[i] = z[i * SGN_WGRAD_TILE];
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) acc[i] = mfma32(a, b[i], acc[i]);
    row += 2;
    u += 2;
    while (u >= p.g.group_rows) {
      u -= p.g.group_rows;
      ++grp;
    }
  }
  float* o = p.part + (size_t)s * p.K * p.N;
#pragma unroll
  for (int i = 0; i < NB; ++i)
    if (col[i]) {
#pragma unroll
      for (int j = 0; j < 16; ++j) o[(size_t)(k0 + mfma_row(j, h)) * p.N + n0 + i * SGN_WGRAD_TILE + r] = acc[i][j];
    }
}

// column n of a (R, N) view: element (row, n) at Z[row * ld + (n / w) * ld2 + n % w]
struct SgnWgradColsum {
  const float* Z;
  float* part;                 // (splits, N)
  long ld, ld2;
  int w, N, col_blocks;          // workgroups of SGN_WGRAD_SUM_COLS columns per split
  long R, rows;
};

static __global__ __launch_bounds__(SGN_THREADS) void sgn_wgrad_colsum_kernel(SgnWgradColsum p) {
  __shared__ float ph_sum[SGN_WGRAD_SUM_PHASES][SGN_WGRAD_SUM_COLS + 1];
  const int cl = threadIdx.x % SGN_WGRAD_SUM_COLS, ph = threadIdx.x / SGN_WGRAD_SUM_COLS;
  const long s = blockIdx.x / p.col_blocks;
  const int n = (int)(blockIdx.x % p.col_blocks) * SGN_WGRAD_SUM_COLS + cl;
  const long begin = s * p.rows;
  const long end = begin + p.rows < p.R ? begin + p.rows : p.R;
  float acc = 0.f;
  if (n < p.N) {
    const float* z = p.Z + (long)(n / p.w) * p.ld2 + n % p.w;
    for (long row = begin + ph; row < end; row += SGN_WGRAD_SUM_PHASES) acc += z[row * p.ld];
  }
  ph_sum[ph][cl] = acc;
  __syncthreads();
  if (ph == 0 && n < p.N) {
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < SGN_WGRAD_SUM_PHASES; ++q) t += ph_sum[q][cl];
    p.part[(size_t)s * p.N + n] = t;
  }
}

// where the input side sits in a frames tape row (SgnFramesTape / Sgn15FramesTape): de1 (128), xn (2, 4), dxn (2, 3)
struct SgnWgradInputCols { int de1, xn, dxn; long cols; };

// je1_w | de1_w (3, 64) each: workgroup (split, branch), thread (row phase, n) owns column n; the phases are added in
// ascending order; part (splits, 2, 3, 64)
static __global__ __launch_bounds__(SGN_THREADS) void sgn_wgrad_first_kernel(const float* __restrict__ tape,
                                                                             SgnWgradInputCols tp, float* part, long R,
                                                                             long rows) {
  __shared__ float ph_sum[SGN_WGRAD_FIRST_PHASES][3][SGN_C1];
  const int n = threadIdx.x % SGN_C1, ph = threadIdx.x / SGN_C1, which = blockIdx.y;
  const long s = blockIdx.x, begin = s * rows;
  const long end = begin + rows < R ? begin + rows : R;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (long row = begin + ph; row < end; row += SGN_WGRAD_FIRST_PHASES) {
    const float* t = tape + (size_t)row * tp.cols;
    const float d = t[tp.de1 + which * SGN_C1 + n];
    a0 = fmaf(t[tp.xn + which * 4 + 0], d, a0);
    a1 = fmaf(t[tp.xn + which * 4 + 1], d, a1);
    a2 = fmaf(t[tp.xn + which * 4 + 2], d, a2);
  }
  ph_sum[ph][0][n] = a0;
  ph_sum[ph][1][n] = a1;
  ph_sum[ph][2][n] = a2;
  __syncthreads();
  if (ph < 3) {                                    // phase index re-used as the coordinate c
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < SGN_WGRAD_FIRST_PHASES; ++q) t += ph_sum[q][ph][n];
    part[(size_t)s * (2 * 3 * SGN_C1) + which * 3 * SGN_C1 + ph * SGN_C1 + n] = t;
  }
}

// aff (4, V, 3): d scale = sum over the frames of d xn * raw (raw = x, or dif = x[t] - x[t - 1], 0 at t = 0), d shift = sum of
// d xn; part (splits, 4 * V * 3), the splits over the frames; joint v of frame f at tape row f * V + v
static __global__ __launch_bounds__(SGN_THREADS) void sgn_wgrad_aff_kernel(const float* __restrict__ x,
                                                                           const float* __restrict__ tape,
                                                                           SgnWgradInputCols tp, float* part, long frames,
                                                                           long rows, int seg, int V) {
  const int F = V * 3;
  const long s = blockIdx.x, begin = s * rows;
  const long end = begin + rows < frames ? begin + rows : frames;
  for (int i = threadIdx.x; i < 4 * F; i += SGN_THREADS) {
    const int kind = i / F, e = i % F, v = e / 3, c = e % 3;       // 0 joint scale, 1 joint shift, 2 dif scale, 3 dif shift
    float acc = 0.f;
    for (long f = begin; f < end; ++f) {
      const float d = tape[sgn_frames_tape_row(f, v, V) * tp.cols + tp.dxn + (kind >> 1) * 3 + c];
      float raw = 1.f;
      if (kind == 0) raw = x[f * F + e];
      if (kind == 2) {
        const long prev = sgn_dif_prev(f, seg);
        raw = prev >= 0 ? x[f * F + e] - x[prev * F + e] : 0.f;
      }
      acc = fmaf(d, raw, acc);
    }
    part[(size_t)s * (4 * F) + i] = acc;
  }
}

static __global__ __launch_bounds__(SGN_THREADS) void sgn_wgrad_finalize_kernel(const float* __restrict__ part, long stride,
                                                                                long splits, float* out, long count) {
  const long i = (long)blockIdx.x * SGN_THREADS + threadIdx.x;
  if (i >= count) return;
  float acc = 0.f;
  for (long s = 0; s < splits; ++s) acc += part[s * stride + i];
  out[i] = acc;
}

// ---- host: one section = a partial launch and the finalize ----
static bool wgrad_grid_ok(long splits, long blocks) { return splits >= 1 && blocks >= 1 && splits <= 0x7fffffffL / blocks; }

static int wgrad_finalize(const float* part, long stride, long splits, float* out, long count, hipStream_t st) {
  const long blocks = (count + SGN_THREADS - 1) / SGN_THREADS;
  if (blocks > 0x7fffffffL) return AGCN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(sgn_wgrad_finalize_kernel, dim3((unsigned)blocks), dim3(SGN_THREADS), 0, st, part, stride, splits, out,
                     count);
  return agcn_check_launch();
}

static int wgrad_gemm(const float* X, long ldx, const float* Z, long ldz, int K, int N, long R, SgnWgradRows g, float* out,
                      float* ws, int rps, hipStream_t st) {
  SgnWgradGemm p;
  p.X = X; p.Z = Z; p.part = ws; p.ldx = ldx; p.ldz = ldz; p.K = K; p.N = N;
  p.tile_blocks = (sgn_wgrad_tiles(K, N) + SGN_WAVES - 1) / SGN_WAVES;
  p.R = R; p.rows = sgn_wgrad_split_rows(R, rps); p.g = g;
  const long splits = sgn_wgrad_splits(R, rps);
  if (K % SGN_WGRAD_TILE || !wgrad_grid_ok(splits, p.tile_blocks)) return AGCN_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(splits * p.tile_blocks));
  switch (sgn_wgrad_strip(N)) {
    case 4: hipLaunchKernelGGL(sgn_wgrad_gemm_kernel<4>, grid, dim3(SGN_THREADS), 0, st, p); break;
    case 2: hipLaunchKernelGGL(sgn_wgrad_gemm_kernel<2>, grid, dim3(SGN_THREADS), 0, st, p); break;
    default: hipLaunchKernelGGL(sgn_wgrad_gemm_kernel<1>, grid, dim3(SGN_THREADS), 0, st, p); break;
  }
  int rc = agcn_check_launch();
  if (rc != AGCN_OK) return rc;
  return wgrad_finalize(ws, (long)K * N, splits, out, (long)K * N, st);
}

static int wgrad_colsum(const float* Z, long ld, int w, long ld2, int N, long R, float* out, float* ws, int rps,
                        hipStream_t st) {
  SgnWgradColsum p;
  p.Z = Z; p.part = ws; p.ld = ld; p.ld2 = ld2; p.w = w; p.N = N;
  p.col_blocks = (N + SGN_WGRAD_SUM_COLS - 1) / SGN_WGRAD_SUM_COLS;
  p.R = R; p.rows = sgn_wgrad_split_rows(R, rps);
  const long splits = sgn_wgrad_splits(R, rps);
  if (!wgrad_grid_ok(splits, p.col_blocks)) return AGCN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(sgn_wgrad_colsum_kernel, dim3((unsigned)(splits * p.col_blocks)), dim3(SGN_THREADS), 0, st, p);
  int rc = agcn_check_launch();
  if (rc != AGCN_OK) return rc;
  return wgrad_finalize(ws, N, splits, out, N, st);
}

// the input side of a frames image, shared by both models (SgnFramesW up to spa1): the second and the first layers of the
// two embeddings from e1 / de2 / de1 / xn, spa1 (V, 64) from the tape as a (frames, V * 64) view, aff from d xn and x
static int wgrad_input_side(const float* x, const float* tape, int e1, int de2, int dspa, SgnWgradInputCols tp,
                            const SgnFramesW& o, float* d_w, float* part, long frames, int seg, int V, int rps,
                            hipStream_t st) {
  const long R = frames * V, C = tp.cols;
  const SgnWgradRows plain = sgn_wgrad_plain_rows(R);
  int rc;
#define WGRAD_STEP(call) if ((rc = (call)) != AGCN_OK) return rc
  WGRAD_STEP(wgrad_gemm(tape + e1, C, tape + de2, C, SGN_C1, SGN_C1, R, plain, d_w + o.je2_w, part, rps, st));
  WGRAD_STEP(wgrad_colsum(tape + de2, C, SGN_C1, 0, SGN_C1, R, d_w + o.je2_b, part, rps, st));
  WGRAD_STEP(wgrad_gemm(tape + e1 + SGN_C1, C, tape + de2 + SGN_C1, C, SGN_C1, SGN_C1, R, plain, d_w + o.de2_w, part, rps,
                        st));
  WGRAD_STEP(wgrad_colsum(tape + de2 + SGN_C1, C, SGN_C1, 0, SGN_C1, R, d_w + o.de2_b, part, rps, st));
  {
    const long splits = sgn_wgrad_splits(R, rps);
    hipLaunchKernelGGL(sgn_wgrad_first_kernel, dim3((unsigned)splits, 2), dim3(SGN_THREADS), 0, st, tape, tp, part, R,
                       sgn_wgrad_split_rows(R, rps));
    WGRAD_STEP(agcn_check_launch());
    WGRAD_STEP(wgrad_finalize(part, 2 * 3 * SGN_C1, splits, d_w + o.je1_w, 3 * SGN_C1, st));
    WGRAD_STEP(wgrad_finalize(part + 3 * SGN_C1, 2 * 3 * SGN_C1, splits, d_w + o.de1_w, 3 * SGN_C1, st));
  }
  WGRAD_STEP(wgrad_colsum(tape + tp.de1, C, SGN_C1, 0, SGN_C1, R, d_w + o.je1_b, part, rps, st));
  WGRAD_STEP(wgrad_colsum(tape + tp.de1 + SGN_C1, C, SGN_C1, 0, SGN_C1, R, d_w + o.de1_b, part, rps, st));
  WGRAD_STEP(wgrad_colsum(tape + dspa, (long)V * C, SGN_C1, C, V * SGN_C1, frames, d_w + o.spa1, part, rps, st));
  {
    const long splits = sgn_wgrad_splits(frames, rps);
    hipLaunchKernelGGL(sgn_wgrad_aff_kernel, dim3((unsigned)splits), dim3(SGN_THREADS), 0, st, x, tape, tp, part, frames,
                       sgn_wgrad_split_rows(frames, rps), seg, V);
    WGRAD_STEP(agcn_check_launch());
    WGRAD_STEP(wgrad_finalize(part, 4 * V * 3, splits, d_w + o.aff, 4 * V * 3, st));
  }
#undef WGRAD_STEP
  return AGCN_OK;
}

#define WGRAD_TRY(call)            \
  do {                             \
    const int rc_ = (call);        \
    if (rc_ != AGCN_OK) return rc_; \
  } while (0)
