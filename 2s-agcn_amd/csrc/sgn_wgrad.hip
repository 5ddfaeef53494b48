// Parameter gradients of the base SGN in eval mode (frozen-BatchNorm fine-tuning): the gradient of a loss on the logits
// with respect to the two folded weight images of sgn.hip, each in its image's own layout (sgn_plan.h: SgnFramesW,
// SgnClipW).  torch autograd carries them through the fold to the parameters (model/sgn.py::SGN._folded).
// The operands come from the two tapes that the taping backward kernels of sgn_bwd.hip write (agcn_sgn_clip_bwd_tape,
// agcn_sgn_frames_bwd_tape; V real joint rows per frame; layout in sgn_wgrad_plan.h).  The reduction kernels here:
//   sgn_wgrad_gemm_kernel   dW (K, N) = X^T . Z over the rows of one split, one wave per 32 x (32..128) strip of dW,
//                           exact-f32 MFMA (v_mfma_f32_32x32x2_f32), both operands read along their rows straight from
//                           the tape; plain or grouped rows (the three taps of the temporal convolution).
//   sgn_wgrad_colsum_kernel column sums over the rows of one split (32 columns x 8 row phases per workgroup, the phases
//                           added in ascending order): biases, and tem1 / spa1 as (clips, seg * 256) / (frames, V * 64).
//   sgn_wgrad_first_kernel  the 3 x 64 first embedding layers (K = 3: VALU);  sgn_wgrad_aff_kernel  the folded norm_data.
//   sgn_wgrad_finalize_kernel  adds the partials of the splits in ascending order into the image.
// Every sum runs in a fixed order (rows ascending inside a split, splits ascending), no atomics: the same inputs give the
// same bits.  Geometry, splits, workspace and every guarded index: sgn_wgrad_plan.h.
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

__global__ __launch_bounds__(SGN_THREADS) void sgn_wgrad_colsum_kernel(SgnWgradColsum p) {
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

// je1_w | de1_w (3, 64) each: workgroup (split, branch), thread (row phase, n) owns column n; the phases are added in
// ascending order; part (splits, 2, 3, 64)
__global__ __launch_bounds__(SGN_THREADS) void sgn_wgrad_first_kernel(const float* __restrict__ tape, float* part, long R,
                                                                      long rows) {
  __shared__ float ph_sum[SGN_WGRAD_FIRST_PHASES][3][SGN_C1];
  const SgnFramesTape tp = sgn_frames_tape();
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
// d xn; part (splits, 4 * V * 3), the splits over the frames
__global__ __launch_bounds__(SGN_THREADS) void sgn_wgrad_aff_kernel(const float* __restrict__ x,
                                                                    const float* __restrict__ tape, float* part,
                                                                    long frames, long rows, int seg, int V) {
  const SgnFramesTape tp = sgn_frames_tape();
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

__global__ __launch_bounds__(SGN_THREADS) void sgn_wgrad_finalize_kernel(const float* __restrict__ part, long stride,
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

#define WGRAD_TRY(call)            \
  do {                             \
    const int rc_ = (call);        \
    if (rc_ != AGCN_OK) return rc_; \
  } while (0)

extern "C" size_t agcn_sgn_frames_tape_floats(int N, int seg, int V) {
  return sgn_frames_domain(N, seg, V) ? sgn_frames_tape_floats(N, seg, V) : 0;
}
extern "C" size_t agcn_sgn_clip_tape_floats(int N, int seg, int num_class) {
  return sgn_clip_domain(N, seg, num_class) ? sgn_clip_tape(N, seg).total : 0;
}
extern "C" size_t agcn_sgn_wgrad_workspace(int N, int seg, int V, int num_class, int rows_per_split) {
  if (!sgn_wgrad_domain(N, seg, V, num_class) || rows_per_split < 0) return 0;
  return sgn_wgrad_ws_floats(N, seg, V, num_class, rows_per_split) * sizeof(float);
}

extern "C" int agcn_sgn_frames_wgrad(const float* x, const float* w, const float* tape, float* d_w, void* ws,
                                     size_t ws_bytes, int N, int seg, int V, int rows_per_split, void* stream) {
  if (!x || !w || !tape || !d_w || !ws) return AGCN_ERR_ARG;
  if (N < 1 || seg < 1 || V < 2 || V > SGN_MAX_V || rows_per_split < 0) return AGCN_ERR_ARG;
  if (!sgn_frames_domain(N, seg, V)) return AGCN_ERR_UNSUPPORTED;
  const long frames = (long)N * seg, R = frames * V;
  if (!sgn_wgrad_splits_ok(R, rows_per_split)) return AGCN_ERR_UNSUPPORTED;
  if (ws_bytes < sgn_wgrad_ws_floats(N, seg, V, 1, rows_per_split) * sizeof(float)) return AGCN_ERR_WORKSPACE;
  const SgnFramesW o = sgn_frames_w(V);
  const SgnFramesTape tp = sgn_frames_tape();
  const long C = tp.cols;
  const int rps = rows_per_split;
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)ws;
  const SgnWgradRows plain = sgn_wgrad_plain_rows(R);
  AGCN_NOTE_KERNEL("sgn_wgrad_gemm_kernel<f32 mfma> frames image V=%d rows=%ld splits=%ld", V, R, sgn_wgrad_splits(R, rps));
  // the three gcn_spa: [g.x_l | x_l]^T . d z_l and the column sums of d z_l
  WGRAD_TRY(wgrad_gemm(tape + tp.gx3, C, tape + tp.dz3, C, 2 * SGN_C3, SGN_C3, R, plain, d_w + o.c3_w, part, rps, st));
  WGRAD_TRY(wgrad_colsum(tape + tp.dz3, C, SGN_C3, 0, SGN_C3, R, d_w + o.c3_b, part, rps, st));
  WGRAD_TRY(wgrad_gemm(tape + tp.gx2, C, tape + tp.dz2, C, 2 * SGN_C2, SGN_C3, R, plain, d_w + o.c2_w, part, rps, st));
  WGRAD_TRY(wgrad_colsum(tape + tp.dz2, C, SGN_C3, 0, SGN_C3, R, d_w + o.c2_b, part, rps, st));
  WGRAD_TRY(wgrad_gemm(tape + tp.gx1, C, tape + tp.dz1, C, 2 * SGN_C2, SGN_C2, R, plain, d_w + o.c1_w, part, rps, st));
  WGRAD_TRY(wgrad_colsum(tape + tp.dz1, C, SGN_C2, 0, SGN_C2, R, d_w + o.c1_b, part, rps, st));
  // [g1 | g2]
  WGRAD_TRY(wgrad_gemm(tape + tp.x0, C, tape + tp.dg, C, SGN_C2, 2 * SGN_C3, R, plain, d_w + o.g_w, part, rps, st));
  WGRAD_TRY(wgrad_colsum(tape + tp.dg, C, 2 * SGN_C3, 0, 2 * SGN_C3, R, d_w + o.g_b, part, rps, st));
  // the second and the first layers of the two embeddings
  WGRAD_TRY(wgrad_gemm(tape + tp.e1, C, tape + tp.de2, C, SGN_C1, SGN_C1, R, plain, d_w + o.je2_w, part, rps, st));
  WGRAD_TRY(wgrad_colsum(tape + tp.de2, C, SGN_C1, 0, SGN_C1, R, d_w + o.je2_b, part, rps, st));
  WGRAD_TRY(wgrad_gemm(tape + tp.e1 + SGN_C1, C, tape + tp.de2 + SGN_C1, C, SGN_C1, SGN_C1, R, plain, d_w + o.de2_w, part,
                       rps, st));
  WGRAD_TRY(wgrad_colsum(tape + tp.de2 + SGN_C1, C, SGN_C1, 0, SGN_C1, R, d_w + o.de2_b, part, rps, st));
  {
    const long splits = sgn_wgrad_splits(R, rps);
    hipLaunchKernelGGL(sgn_wgrad_first_kernel, dim3((unsigned)splits, 2), dim3(SGN_THREADS), 0, st, tape, part, R,
                       sgn_wgrad_split_rows(R, rps));
    WGRAD_TRY(agcn_check_launch());
    WGRAD_TRY(wgrad_finalize(part, 2 * 3 * SGN_C1, splits, d_w + o.je1_w, 3 * SGN_C1, st));
    WGRAD_TRY(wgrad_finalize(part + 3 * SGN_C1, 2 * 3 * SGN_C1, splits, d_w + o.de1_w, 3 * SGN_C1, st));
  }
  WGRAD_TRY(wgrad_colsum(tape + tp.de1, C, SGN_C1, 0, SGN_C1, R, d_w + o.je1_b, part, rps, st));
  WGRAD_TRY(wgrad_colsum(tape + tp.de1 + SGN_C1, C, SGN_C1, 0, SGN_C1, R, d_w + o.de1_b, part, rps, st));
  // spa1 (V, 64): the frames tape as a (frames, V * 64) view; aff: the folded norm_data, from d xn and x
  WGRAD_TRY(wgrad_colsum(tape + tp.dspa, (long)V * C, SGN_C1, C, V * SGN_C1, frames, d_w + o.spa1, part, rps, st));
  {
    const long splits = sgn_wgrad_splits(frames, rps);
    hipLaunchKernelGGL(sgn_wgrad_aff_kernel, dim3((unsigned)splits), dim3(SGN_THREADS), 0, st, x, tape, part, frames,
                       sgn_wgrad_split_rows(frames, rps), seg, V);
    WGRAD_TRY(agcn_check_launch());
    WGRAD_TRY(wgrad_finalize(part, 4 * V * 3, splits, d_w + o.aff, 4 * V * 3, st));
  }
  return AGCN_OK;
}

extern "C" int agcn_sgn_clip_wgrad(const float* tape, const float* dfeat, const float* dlogits, float* d_w, void* ws,
                                   size_t ws_bytes, int N, int seg, int num_class, int rows_per_split, void* stream) {
  if (!tape || !dfeat || !dlogits || !d_w || !ws) return AGCN_ERR_ARG;
  if (N < 1 || seg < 1 || num_class < 1 || rows_per_split < 0) return AGCN_ERR_ARG;
  if (!sgn_clip_domain(N, seg, num_class)) return AGCN_ERR_UNSUPPORTED;
  const long R = (long)N * seg;
  if (!sgn_wgrad_splits_ok(R, rows_per_split)) return AGCN_ERR_UNSUPPORTED;
  if (ws_bytes < sgn_wgrad_ws_floats(N, seg, 2, num_class, rows_per_split) * sizeof(float)) return AGCN_ERR_WORKSPACE;
  const SgnClipW o = sgn_clip_w(seg, num_class);
  const SgnClipTape tp = sgn_clip_tape(N, seg);
  const int rps = rows_per_split;
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)ws;
  AGCN_NOTE_KERNEL("sgn_wgrad_gemm_kernel<f32 mfma> clip image seg=%d clips=%d splits=%ld", seg, N, sgn_wgrad_splits(R, rps));
  // tem1 (seg, 256): d feat summed over the clips
  WGRAD_TRY(wgrad_colsum(dfeat, (long)seg * SGN_C3, seg * SGN_C3, 0, seg * SGN_C3, N, d_w + o.tem1, part, rps, st));
  // the 3-tap convolution: tap dt reads H one row further, inside the clip's seg + 2 rows
  for (int dt = 0; dt < 3; ++dt)
    WGRAD_TRY(wgrad_gemm(tape + tp.h, SGN_C3, tape + tp.dy1, SGN_C3, SGN_C3, SGN_C3, R, sgn_wgrad_tap_rows(seg, dt),
                         d_w + o.t1_w + (long)dt * SGN_C3 * SGN_C3, part, rps, st));
  WGRAD_TRY(wgrad_colsum(tape + tp.dy1, SGN_C3, SGN_C3, 0, SGN_C3, R, d_w + o.t1_b, part, rps, st));
  WGRAD_TRY(wgrad_gemm(tape + tp.y1, SGN_C3, tape + tp.dy2, SGN_C4, SGN_C3, SGN_C4, R, sgn_wgrad_plain_rows(R), d_w + o.t2_w,
                       part, rps, st));
  WGRAD_TRY(wgrad_colsum(tape + tp.dy2, SGN_C4, SGN_C4, 0, SGN_C4, R, d_w + o.t2_b, part, rps, st));
  WGRAD_TRY(wgrad_gemm(tape + tp.ymax, SGN_C4, dlogits, num_class, SGN_C4, num_class, N, sgn_wgrad_plain_rows(N),
                       d_w + o.fc_w, part, rps, st));
  WGRAD_TRY(wgrad_colsum(dlogits, num_class, num_class, 0, num_class, N, d_w + o.fc_b, part, rps, st));
  return AGCN_OK;
}
