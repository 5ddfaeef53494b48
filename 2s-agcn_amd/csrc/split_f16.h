// "f16x3" split arithmetic shared by the temporal-convolution and graph-convolution kernels: two fp16 pieces per
// operand, x = h1 + h2 (11 + 11 significand bits), and the three products h1*h1 + h1*h2 + h2*h1 on
// v_mfma_f32_32x32x16_f16: dropped terms below 2^-22 |a*b|.  Emulated on the CPU against fp64
// (tools/split_numerics.py): 9e-7 of the result scale for O(1) operands, the same as an fp32 GEMM's own rounding (7e-7);
// half the matrix work, half the split arithmetic and two thirds of the LDS bytes of bf16x6.
#pragma once
#include "agcn_common.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float sf_f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void split_pair_f16(float a, float b, unsigned& p1, unsigned& p2) {
  const sf_f32x2 v = {a, b};
  const f16x2 h = __builtin_convertvector(v, f16x2);            // v_cvt_pk_f16_f32 (round to nearest even)
  const sf_f32x2 r = v - __builtin_convertvector(h, sf_f32x2);
  p1 = __builtin_bit_cast(unsigned, h);
  p2 = __builtin_bit_cast(unsigned, __builtin_convertvector(r, f16x2));
}

// The same split in three instructions per pair instead of five: the residual x - float(h) is formed by v_fma_mix*_f16
// (fp16 and fp32 sources in one fma, result rounded to fp16 once), bit-identical to split_pair_f16: x - float(h) is exact
// in fp32 either way.  (hipcc does not select the mixed-precision fma from the plain expression.)
__device__ __forceinline__ void split_pair_f16_mix(float a, float b, unsigned& p1, unsigned& p2) {
  const sf_f32x2 v = {a, b};
  const f16x2 h = __builtin_convertvector(v, f16x2);            // v_cvt_pk_f16_f32
  p1 = __builtin_bit_cast(unsigned, h);
  unsigned lo;
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(lo) : "v"(p1), "v"(a));
  asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lo) : "v"(p1), "v"(b));
  p2 = lo;
}

// fp16 holds 6e-5 < |x| < 65504 with full precision: the f16x3 kernels multiply the streamed operand by the power of two
// (exact) that brings the TENSOR's maximum m into [2^TARGET, 2^(TARGET+1)) and undo it on the accumulators (exact).  That
// covers activations that grew past 2^15 as well as gradients of 1e-6; elements far below the maximum lose bits only
// below 2^-25 * 2^(14-TARGET) of it, which is what an fp32 accumulation of the same sum loses too.
// TARGET = 14: the operand itself is split (temporal convolutions).  TARGET = F16_ADJ_TARGET = 2: what is split next is the
// operand times an adjacency (graph chain: G = x . A^), so the scale leaves headroom for the adjacency's column (backward:
// row) sums: |G| <= 2^(TARGET+1) * sum |A^| stays inside fp16 up to sums of 2^13 = 8192 (V <= 32 entries averaging 256).
// The reference's A^ = A (column-normalised, <= 1) + PA (a trained parameter, initialised 1e-6 / A) + softmax (<= 1) sits
// three orders of magnitude below that; round 2 used TARGET = 8 (headroom 2^7).  A smaller TARGET costs no accuracy: the
// split is invariant under powers of two, and the absolute error floor (half an fp16 subnormal step, 2^-25 in scaled
// units) is 2^-(26+TARGET) of the tensor maximum -- 2^-28 here, far below fp32's own rounding.  Beyond 2^13 the products
// overflow to Inf and the loss turns NaN (visible, not silent); tests/test_gpu_kernels.py::test_f16x3_adjacency_headroom.
constexpr int F16_ADJ_TARGET = 2;

// WEIGHTS are split after a multiplication by the fixed power of two F16_W_SCALE, undone on the accumulators (both exact):
// the residual plane of a weight w is (w - fp16(w)) ~ 2^-11 |w|, a normal fp16 only for |w| >= 2^-3 -- below that its
// absolute error is half a subnormal step (2^-25), e.g. 5e-6 RELATIVE at the reference's conv_d initialisation of l8..l10
// (std 0.0032), ten times an fp32 GEMM's own rounding (emulated: tools/split_numerics.py).  With the pre-scale the
// threshold drops to |w| >= 2^-11 and the floor to 2^-33; weights up to 255 fit (|w| >= 256 -> Inf -> NaN loss, visible).
// No measurement pass: trained convolution weights of this network sit between 1e-4 and O(1).
constexpr float F16_W_SCALE = 256.f, F16_W_INV = 1.f / 256.f;

template <int TARGET = 14>
__device__ __forceinline__ void f16_range_scale_of(float m, float& s, float& inv) {
  s = 1.f; inv = 1.f;
  if (m > 0.f) {
    int e = (int)((__builtin_bit_cast(unsigned, m) >> 23) & 0xffu) - 127;   // floor(log2 m); inf / nan: 128
    e = max(e, -100);
    s = __builtin_bit_cast(float, (unsigned)(127 - (e - TARGET)) << 23);
    inv = __builtin_bit_cast(float, (unsigned)(127 + (e - TARGET)) << 23);
  }
}
// (s, 1/s) from the device scalar max |x|
__device__ __forceinline__ void f16_range_scale(const float* absmax, float& s, float& inv) {
  s = 1.f; inv = 1.f;
  if (absmax) f16_range_scale_of<14>(*absmax, s, inv);
}

// max |x| of a tensor -> *out (as the bit pattern of a non-negative float: unsigned order = float order); *out zeroed first
static __global__ void __launch_bounds__(256) absmax_kernel(const float* __restrict__ x, long n, unsigned* __restrict__ out) {
  __shared__ unsigned red[4];
  unsigned m = 0;
  // 16-byte loads from the first aligned element on; the (up to 3) floats in front of it and the tail go one by one
  long head = (long)(((16 - (reinterpret_cast<unsigned long>(x) & 15)) & 15) >> 2);
  if (head > n) head = n;
  const float* xa = x + head;
  const long na = n - head, n4 = na >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const f32x4 v = reinterpret_cast<const f32x4*>(xa)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {          // (through a float: __builtin_bit_cast on a vector ELEMENT read element 0 four times)
      const float f = v[k];
      m = max(m, __float_as_uint(f) & 0x7fffffffu);
    }
  }
  for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < na; i += (long)gridDim.x * 256)
    m = max(m, __float_as_uint(xa[i]) & 0x7fffffffu);
  if (blockIdx.x == 0 && (long)threadIdx.x < head) m = max(m, __float_as_uint(x[threadIdx.x]) & 0x7fffffffu);
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, k));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(out, max(max(red[0], red[1]), max(red[2], red[3])));
}

// *out = max |x| over n floats, on `stream`
static inline int agcn_launch_absmax(const float* x, long n, unsigned* out, hipStream_t stream) {
  if (hipMemsetAsync(out, 0, 4, stream) != hipSuccess) return AGCN_ERR_ARG;
  hipLaunchKernelGGL(absmax_kernel, dim3(2048), dim3(256), 0, stream, x, n, out);
  return agcn_check_launch();
}

// The range-scale maximum of an f16x3 operand: the one its producer left behind (`given`; nothing is launched), else a
// streaming pass of our own into `slot`.  Where a launcher keeps its slots (each size query carries the matching slack):
//   graph chain, adjacency gradient:         the 16 bytes behind the weight images (query: +16)
//   temporal convolutions (bf16_in_absmax):  the last 16 bytes of the workspace (query: +256)
//   tap weight gradients (w9_run):           two words behind the transposed copies (query: +512, alignment included)
//   fused adjacency forward:                 the caller's output slot, else behind the weight images (query: +256)
static inline int agcn_operand_max(const float* given, const float* tensor, long n, void* slot, hipStream_t stream,
                                   const float** out) {
  if (given) { *out = given; return AGCN_OK; }
  if (int rc = agcn_launch_absmax(tensor, n, static_cast<unsigned*>(slot), stream)) return rc;
  *out = static_cast<const float*>(slot);
  return AGCN_OK;
}
