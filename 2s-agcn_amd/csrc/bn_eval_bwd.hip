// Backward through the eval-mode (frozen statistics) BatchNorm + residual + ReLU stage of bn.hip:
//   out = act(s1[c]*y1 + b1[c] [+ s2[c]*y2 + b2[c] | + r]),  s = gamma * rsqrt(running_var + eps)
// The mean / variance terms of the train-mode backward vanish, so the whole stage is ONE streaming pass
//   dz = dout * mask ; dy1 = s1[c]*dz ; dy2 = s2[c]*dz ; per-row (sum dz, sum dz*y1, sum dz*y2) ; max |dy1|
// (train: reduce reads 2 tensors, apply reads 2 and writes 1; here: reads 2, writes 1, or reads 1 and writes 1 when no
// parameter gradient is wanted) and a per-channel finalize in double.  No float atomics: the row partials go through
// the same (N*C, 3) slab as agcn_bn_bwd_reduce and are added in a fixed order.
#include "agcn_common.h"

namespace {

typedef f32x4 f32x4_u __attribute__((aligned(4)));     // rows of P % 4 != 0 floats start 4- or 8-byte aligned only

// one workgroup per (n, c) row at a time, rows dealt round-robin to a grid of at most MAX_WG resident workgroups
// (measured on MI355X at C=256, P=1875: with a workgroup -- and so an atomicMax on the one scalar -- per row, 32768 of
// them, the pass took 0.41 ms against 0.25 ms for the two train-mode passes).
// HAS2: second (down / residual) BatchNorm branch; SUMS: the row partials are wanted (y1 / y2 are read only then)
constexpr int MAX_WG = 2048;             // 256 CUs x 8 workgroups of 4 waves

template <bool HAS2, bool SUMS>
__global__ void __launch_bounds__(256)
bn_bwd_eval_kernel(const float* __restrict__ dout, const float* __restrict__ mask, int mask_bits,
                   const float* __restrict__ y1, const float* __restrict__ y2, const float* __restrict__ scale1,
                   const float* __restrict__ scale2, float* __restrict__ part, float* __restrict__ dy1,
                   float* __restrict__ dy2, int rows, int P, int C, unsigned* __restrict__ amax1) {
  __shared__ float red[2][3][4];         // double-buffered by row parity: one barrier per row is enough
  __shared__ unsigned wmax[4];
  const int wave = threadIdx.x >> 6;
  unsigned tmax = 0;                     // max |dy1| of this thread (bit pattern: unsigned order = float order)
  int it = 0;
  for (long row = blockIdx.x; row < rows; row += gridDim.x, it ^= 1) {
    const int c = (int)(row % C);
    const long e_row = row * P;
    const float k1 = scale1[c];
    const float k2 = HAS2 ? scale2[c] : 0.f;
    const float* d = dout + e_row;
    const float* mk = (mask && !mask_bits) ? mask + e_row : nullptr;
    const unsigned* mb = (mask && mask_bits) ? reinterpret_cast<const unsigned*>(mask) : nullptr;
    const float* a = SUMS ? y1 + e_row : nullptr;
    const float* b = (SUMS && HAS2) ? y2 + e_row : nullptr;
    float* o1 = dy1 + e_row;
    float* o2 = HAS2 ? dy2 + e_row : nullptr;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    const int P4 = P >> 2;
    for (int q4 = threadIdx.x; q4 < P4; q4 += 256) {
      const f32x4 d4 = reinterpret_cast<const f32x4_u*>(d)[q4];
      f32x4 a4 = {0.f, 0.f, 0.f, 0.f}, b4 = a4;
      if (SUMS) a4 = reinterpret_cast<const f32x4_u*>(a)[q4];
      if (SUMS && HAS2) b4 = reinterpret_cast<const f32x4_u*>(b)[q4];
      float dv[4] = {d4.x, d4.y, d4.z, d4.w};
      if (mk) {
        const f32x4 m4 = reinterpret_cast<const f32x4_u*>(mk)[q4];
        const float mv[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) dv[k] = (mv[k] > 0.f) ? dv[k] : 0.f;
      }
      if (mb) {
        const long e = e_row + 4L * q4;
        const int sh = (int)(e & 31);
        unsigned nib = mb[e >> 5] >> sh;
        if (sh > 28) nib |= mb[(e >> 5) + 1] << (32 - sh);   // the 4 bits straddle two words (rows not a multiple of 4)
#pragma unroll
        for (int k = 0; k < 4; ++k) dv[k] = ((nib >> k) & 1u) ? dv[k] : 0.f;
      }
      const float av[4] = {a4.x, a4.y, a4.z, a4.w};
      const float bv[4] = {b4.x, b4.y, b4.z, b4.w};
      float r1[4], r2[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        r1[k] = k1 * dv[k];
        if (HAS2) r2[k] = k2 * dv[k];
        if (SUMS) {
          s0 += dv[k];
          s1 += dv[k] * av[k];
          if (HAS2) s2 += dv[k] * bv[k];
        }
        tmax = max(tmax, __float_as_uint(r1[k]) & 0x7fffffffu);
      }
      reinterpret_cast<f32x4_u*>(o1)[q4] = f32x4{r1[0], r1[1], r1[2], r1[3]};
      if (HAS2) reinterpret_cast<f32x4_u*>(o2)[q4] = f32x4{r2[0], r2[1], r2[2], r2[3]};
    }
    for (int q = 4 * P4 + threadIdx.x; q < P; q += 256) {    // the last P % 4 elements of the row
      float dz = d[q];
      if (mk) dz = (mk[q] > 0.f) ? dz : 0.f;
      if (mb) {
        const long e = e_row + q;
        dz = ((mb[e >> 5] >> (e & 31)) & 1u) ? dz : 0.f;
      }
      const float r1 = k1 * dz;
      o1[q] = r1;
      if (HAS2) o2[q] = k2 * dz;
      if (SUMS) {
        s0 += dz;
        s1 += dz * a[q];
        if (HAS2) s2 += dz * b[q];
      }
      tmax = max(tmax, __float_as_uint(r1) & 0x7fffffffu);
    }
    if (SUMS) {                            // fixed-order tree: lanes, half-waves, the four waves
      s0 = half_sum(s0); s1 = half_sum(s1); s2 = half_sum(s2);
      s0 += __shfl_xor(s0, 32); s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
      if ((threadIdx.x & 63) == 0) { red[it][0][wave] = s0; red[it][1][wave] = s1; red[it][2][wave] = s2; }
      __syncthreads();
      if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        part[row * 3 + k] = red[it][k][0] + red[it][k][1] + red[it][k][2] + red[it][k][3];
      }
    }
  }
  if (amax1) {
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) tmax = max(tmax, (unsigned)__shfl_xor((int)tmax, k));
    if ((threadIdx.x & 63) == 0) wmax[wave] = tmax;
    __syncthreads();
  }
  if (amax1 && threadIdx.x == 0) {       // one atomic per workgroup; max is order-independent, so the result is exact
    const unsigned m = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
    if (m) atomicMax(amax1, m);
  }
}

// per channel, in double and in row order: dbeta = S0, dgamma = invstd*(S1 - mean*S0), and the gradient of the bias of
// the convolution in front of the BatchNorm, scale*S0 (NOT zero in eval mode: the frozen mean does not cancel it)
__global__ void bn_bwd_eval_finalize_kernel(const float* __restrict__ part, int N, int C,
                                            const float* __restrict__ scale1, const float* __restrict__ mean1,
                                            const float* __restrict__ invstd1, const float* __restrict__ scale2,
                                            const float* __restrict__ mean2, const float* __restrict__ invstd2,
                                            float* __restrict__ dgamma1, float* __restrict__ dbeta1,
                                            float* __restrict__ dbias1, float* __restrict__ dgamma2,
                                            float* __restrict__ dbeta2, float* __restrict__ dbias2) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll 8
  for (int n = 0; n < N; ++n) {
    const float* p = part + ((long)n * C + c) * 3;
    s0 += (double)p[0]; s1 += (double)p[1]; s2 += (double)p[2];
  }
  dgamma1[c] = (float)((double)invstd1[c] * (s1 - (double)mean1[c] * s0));
  dbeta1[c] = (float)s0;
  if (dbias1) dbias1[c] = (float)((double)scale1[c] * s0);
  if (scale2) {
    dgamma2[c] = (float)((double)invstd2[c] * (s2 - (double)mean2[c] * s0));
    dbeta2[c] = (float)s0;
    if (dbias2) dbias2[c] = (float)((double)scale2[c] * s0);
  }
}

// the forward coefficients of bn.hip's bn_eval_coeff_kernel (same expressions, same bits) plus the frozen mean / invstd
// the backward needs, copied out so that a later in-place update of the running statistics cannot reach the graph
__global__ void bn_eval_coeff_ex_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                        const float* __restrict__ rmean, const float* __restrict__ rvar, float eps, int C,
                                        float* __restrict__ scale_out, float* __restrict__ shift_out,
                                        float* __restrict__ mean_out, float* __restrict__ invstd_out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float sd = sqrtf(rvar[c] + eps);
  const float sc = gamma[c] / sd;
  scale_out[c] = sc;
  shift_out[c] = beta[c] - rmean[c] * sc;
  mean_out[c] = rmean[c];
  invstd_out[c] = 1.f / sd;
}

}  // namespace

extern "C" {

int agcn_bn_eval_coeff_ex(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                          float eps, int C, float* scale, float* shift, float* mean, float* invstd, void* stream) {
  if (!gamma || !beta || !running_mean || !running_var || !scale || !shift || !mean || !invstd || C <= 0)
    return AGCN_ERR_ARG;
  hipLaunchKernelGGL(bn_eval_coeff_ex_kernel, dim3((C + 63) / 64), dim3(64), 0, (hipStream_t)stream, gamma, beta,
                     running_mean, running_var, eps, C, scale, shift, mean, invstd);
  return agcn_check_launch();
}

// dz = dout*(mask>0) (mask NULL: no ReLU; fp32 tensor or sign bit words as in agcn_bn_bwd_reduce); dy1 = scale1[c]*dz,
// dy2 = scale2[c]*dz (branch 2 exists iff scale2 != NULL).  want_sums: also part[(n*C + c)*3 + k] = per-row
// (sum dz, sum dz*y1, sum dz*y2) for agcn_bn_bwd_eval_finalize; with want_sums = 0 neither y1, y2 nor part is touched
// (they may be NULL).  absmax1_out (optional, 4 bytes): max |dy1|.  Any N*C*P (no multiple-of-4 requirement).
int agcn_bn_bwd_eval(const float* dout, const void* mask, int mask_bits, const float* y1, const float* scale1,
                     const float* y2, const float* scale2, int want_sums, float* part, float* dy1, float* dy2,
                     float* absmax1_out, int N, int C, int P, void* stream) {
  if (!dout || !scale1 || !dy1 || N <= 0 || C <= 0 || P <= 0) return AGCN_ERR_ARG;
  if (scale2 && !dy2) return AGCN_ERR_ARG;
  if (want_sums && (!y1 || !part || (scale2 && !y2))) return AGCN_ERR_ARG;
  if ((long)N * C > 0x7fffffffL) return AGCN_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (absmax1_out && hipMemsetAsync(absmax1_out, 0, 4, s) != hipSuccess) return AGCN_ERR_ARG;
  const int rows = N * C;
  const dim3 g((unsigned)(rows < MAX_WG ? rows : MAX_WG)), b(256);
#define LAUNCH_EVAL(H, S)                                                                                          \
  hipLaunchKernelGGL((bn_bwd_eval_kernel<H, S>), g, b, 0, s, dout, (const float*)mask, mask_bits, y1, y2, scale1, \
                     scale2, part, dy1, dy2, rows, P, C, (unsigned*)absmax1_out)
  if (scale2) { if (want_sums) LAUNCH_EVAL(true, true); else LAUNCH_EVAL(true, false); }
  else { if (want_sums) LAUNCH_EVAL(false, true); else LAUNCH_EVAL(false, false); }
#undef LAUNCH_EVAL
  return agcn_check_launch();
}

// part: the slab of agcn_bn_bwd_eval(want_sums = 1), nrows = N rows per channel; mean / invstd: the frozen statistics
// (agcn_bn_eval_coeff_ex).  dbias1 / dbias2 (optional): gradient of the bias of the convolution in front of each BN.
int agcn_bn_bwd_eval_finalize(const float* part, int nrows, int C, const float* scale1, const float* mean1,
                              const float* invstd1, const float* scale2, const float* mean2, const float* invstd2,
                              float* dgamma1, float* dbeta1, float* dbias1, float* dgamma2, float* dbeta2,
                              float* dbias2, void* stream) {
  if (!part || !scale1 || !mean1 || !invstd1 || !dgamma1 || !dbeta1 || nrows <= 0 || C <= 0) return AGCN_ERR_ARG;
  if (scale2 && (!mean2 || !invstd2 || !dgamma2 || !dbeta2)) return AGCN_ERR_ARG;
  hipLaunchKernelGGL(bn_bwd_eval_finalize_kernel, dim3((C + 63) / 64), dim3(64), 0, (hipStream_t)stream, part, nrows, C,
                     scale1, mean1, invstd1, scale2, mean2, invstd2, dgamma1, dbeta1, dbias1, dgamma2, dbeta2, dbias2);
  return agcn_check_launch();
}

}  // extern "C"
