// Common device/host helpers for the agcn_hip kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "knobs.h"
// the C ABI: every exported prototype and the AGCN_OK / AGCN_ERR_* codes.  Each definition is compiled against its
// declaration, so a definition that drifts from the header is a "conflicting types" error, not a wild pointer at run time.
#include "../../include/agcn_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// exact-f32 matrix core op: D(32x32) += A(32x2) * B(2x32); lane l holds A[l&31][l>>5], B[l>>5][l&31];
// D register j of lane l is D[row = (j&3) + 8*(j>>2) + 4*(l>>5)][col = l&31].
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int mfma_row(int j, int h) { return (j & 3) + 8 * (j >> 2) + 4 * h; }

// ReLU masks reach the kernels either as the fp32 activation tensor (positive = pass) or as its sign bit mask
// (agcn_bn_act_fwd: bit e of word w <-> element 32*w + e); the raw 32-bit load of either kind and the test:
__device__ __forceinline__ float mask_load(const float* m, long idx, int bits) {
  return bits ? m[idx >> 5] : m[idx];            // bit-mask words are fetched as raw 32-bit patterns
}
__device__ __forceinline__ bool mask_pass(float raw, long idx, int bits) {
  return bits ? ((__builtin_bit_cast(unsigned, raw) >> (idx & 31)) & 1u) != 0u : raw > 0.f;
}

// sum over the 32 lanes of a half-wave (lanes l and l^k stay inside the half for k<32)
__device__ __forceinline__ float half_sum(float v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 1);
  return v;
}

// Bijective XCD-aware remap of a 1-D block id (guide T1): blocks b and b+8 share an XCD, so give
// every XCD a contiguous range of logical ids (neighbouring tiles share halos / rows in its L2).
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, x = bid & 7, k = bid >> 3;
  const int base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
  return base + k;
}

// adjacency.hip: slab sum + 1/K + column softmax + graph terms (also the tail of adj_fused.hip's forward)
int agcn_adj_finalize(const float* spart, const float* A, const float* PA, const float* alpha, float* P, float* adj,
                      int N, int Ci, int T, int V, hipStream_t s, int nused = -1);

// persistent weight-stationary forward of the adjacency scores (adj_ws.hip)
bool agcn_adj_ws_supported(int N, int C, int Ci, int T, int V);
size_t agcn_adj_ws_workspace(int C, int Ci);
int agcn_adj_ws_scores(const float* x, const float* wab, const float* bab, float* tp_out, float* spart, int slots,
                       int* nslots_used, const float* x_absmax, void* ws, size_t ws_bytes, int N, int C, int Ci, int T, int V,
                       hipStream_t s);

// A size query is a dry run of the launch: it builds the same problem with null pointers and walks the same ladder
// with this record attached.  A leaf launcher that is handed one runs its geometry and feasibility checks as always,
// notes what it WOULD write and returns before its first HIP call.  Host only: reached through the host-side problem
// structs or a launcher parameter, never a member of a struct a kernel takes by value.
struct AgcnDryRun {
  long slab_slots;     // slots the launch writes to its partial slab (BatchNorm partials, adjacency-gradient partials)
  size_t ws_bytes;     // workspace bytes it touches, the absmax scalars parked behind the weight images included
};
// an operation of several launches reports the largest workspace and the slot count of the slab it writes
static inline int agcn_dry_note(AgcnDryRun* d, long slab_slots, size_t ws_bytes) {
  if (slab_slots > d->slab_slots) d->slab_slots = slab_slots;
  if (ws_bytes > d->ws_bytes) d->ws_bytes = ws_bytes;
  return AGCN_OK;
}

// What a dry run passes for an operand whose PRESENCE steers the routing (the slab to account for, a fused second
// source, the gate vectors, the operand maxima): non-null, and host code never dereferences a tensor pointer.  The route
// functions of the entry points may therefore be handed placeholders instead of tensors.
static inline float* agcn_dry_present() { static float placeholder; return &placeholder; }

// the size arguments every contraction entry point and size query checks first
static inline bool agcn_sizes_ok(int N, int a, int b, int T, int V) {
  return N > 0 && a > 0 && b > 0 && T > 0 && V > 0 && V <= 32;
}

// temporal convolutions (agcn_tconv_*, and agcn_conv_* as the 1- and 9-tap "same"-padded rows of it): the domain, the
// output-frame count and the launch plan every ladder consumes
#include "tconv_plan.h"

// split-bf16 / f16x3 temporal convolution (conv_gemm_bf16.hip); npl: 3 = bf16x6 (fp32-equivalent), 2 = bf16x3, 1 = bf16.
// Shapes these kernels are tuned for: 9 taps with padding 4 at stride 1 or 2, stride-1 3/5/7 taps with any padding, and
// the stride-1 1x1 backward-data.  The callers add the arithmetic mode (and, for the 1x1, the channel counts).
bool agcn_bf16_conv_wide(int taps, int M);
enum AgcnTconvOp { AGCN_TCONV_FWD, AGCN_TCONV_BWD_DATA };
bool agcn_bf16_tconv_supported(AgcnTconvOp op, int taps, int stride, int pad);
// y = act( bias + tconv(x * gate) [+ add] ): the training forward (stats_part; add, gate null) and the BN-folded inference
// form (agcn_tconv_infer, agcn_conv9_infer), the attention gates of gate.h applied while the operand is staged.  A window
// too long for these kernels' LDS is refused (AGCN_ERR_UNSUPPORTED) before anything is launched.
struct GateArgs;
int agcn_bf16_tconv_fwd(const float* x, const float* w, const float* bias, float* y, float* stats_part, void* ws,
                        size_t ws_bytes, int N, int Cin, int Cout, int T, int V, int taps, int stride, int pad, int npl,
                        hipStream_t s, const float* add, int relu, const float* x_absmax, const GateArgs* gate,
                        AgcnDryRun* dry);
int agcn_bf16_tconv_bwd_data(const float* dy, const float* w, float* dx, int accumulate, const float* add1,
                             const float* mask1, const float* add2, const float* mask2, void* ws, size_t ws_bytes,
                             int N, int Cin, int Cout, int T, int V, int taps, int stride, int pad, int npl,
                             hipStream_t s, const float* dy_absmax, AgcnDryRun* dry);

// register-chained aggregate+project (gcn_chain.hip); mode 0 = forward, 1 = backward-data
bool agcn_gcn_chain_supported(int M, int K, int V);
int agcn_chain_f16x3();                       // 1: the chain runs on f16x3 (split_f16.h), 0: bf16x6 / AGCN_GEMM's mode
int agcn_gcn_chain_tiles(int T);
struct GcnChainCall {
  int mode = 0;                                  // 0: in = x, K = C, M = Cout; 1: in = dy, K = Cout, M = C
  const float *in = nullptr, *adj = nullptr, *wcat = nullptr, *bias = nullptr;
  float *out = nullptr, *stats_part = nullptr;   // stats_part: BatchNorm partials of the forward
  int accumulate = 0, relu = 0;
  const float *add1 = nullptr, *mask1 = nullptr, *add2 = nullptr, *mask2 = nullptr;   // masked addends of the row store
  int mask_bits = 0;
  const float *in2 = nullptr, *w2 = nullptr;     // fused 1x1 term: out += W2 . in2, w2 (K2, M) row-major, or
  int K2 = 0, w2_rows_are_outputs = 0;           //   (M, K2) with w2_rows_are_outputs
  const float *in_absmax = nullptr, *in2_absmax = nullptr;   // f16x3: maxima the producers left behind
  void* ws = nullptr;
  size_t ws_bytes = 0;
  int N = 0, C = 0, Cout = 0, T = 0, V = 0;
  AgcnDryRun* dry = nullptr;
};
int agcn_gcn_chain(const GcnChainCall& c, hipStream_t stream);

bool agcn_gcn_dadj_chain_supported(int C, int V);
int agcn_gcn_dadj_chain(const float* dy, const float* wcat, const float* x, float* dadj_part, void* ws, size_t ws_bytes,
                        int N, int C, int Cout, int T, int V, hipStream_t stream, const float* dy_absmax = nullptr,
                        const float* x_absmax = nullptr, AgcnDryRun* dry = nullptr);

// split-bf16 weight gradients of the tap-free contractions (wgrad_chain.hip): partial slabs only, reduced by the caller
bool agcn_wgrad_chain_supported(int M, int C, int V);
int agcn_wgrad_chain(int agg, const float* dy, const float* x, const float* adj, void* ws, size_t ws_bytes, int* nslabs,
                     int N, int M, int C, int V, int T_src, int T_out, int stride, hipStream_t s,
                     const float* dy_absmax = nullptr, const float* x_absmax = nullptr, AgcnDryRun* dry = nullptr);

// split-bf16 weight gradient of the 9-tap temporal convolution (wgrad9_bf16.hip): slabs [nslabs][9][M][C] at ws; T = frames
// of x
bool agcn_wgrad9_bf16_supported(int M, int C, int V, int stride);
int agcn_wgrad9_bf16(const float* dy, const float* x, void* ws, size_t ws_bytes, int* nslabs, int N, int M, int C, int V,
                     int T, int stride, hipStream_t s, const float* dy_absmax, const float* x_absmax, AgcnDryRun* dry);

// the same f16x3 kernel for stride-1 3/5/7-tap gradients with taps - pad <= 5 (agcn_tconv_bwd_weight): slabs [taps][M][C]
bool agcn_wgrad_tconv_f16_supported(int M, int C, int V, int taps, int stride, int pad);
int agcn_wgrad_tconv_f16(const float* dy, const float* x, void* ws, size_t ws_bytes, int* nslabs, int N, int M, int C,
                         int V, int T, int taps, int pad, hipStream_t s, const float* dy_absmax, const float* x_absmax,
                         AgcnDryRun* dry);

// GEMM arithmetic of the channel contractions: 3 = bf16x6 (default: fp32-equivalent accuracy, measured), 0 = f32 MFMA,
// 2 = bf16x3 (~5e-6 per GEMM; does NOT hold the 1e-4 parity bar end to end), 1 = bf16 (plain bf16 MFMA operands, ONE
// product per fp32 product, fp32 accumulate and fp32 storage: BASELINE configs[3], ~2^-9 relative per product).
// Chosen once per process from the environment variable AGCN_GEMM (knobs.h).
static inline int agcn_gemm_precision() { return agcn_knob(AGCN_GEMM); }
// the register-chained / split-plane kernel family serves bf16x6 (3 planes, 6 products) and bf16 (hi plane, 1 product)
static inline bool agcn_chained() { const int m = agcn_gemm_precision(); return m == 3 || m == 1; }
static inline int agcn_npl() { return agcn_gemm_precision() == 1 ? 1 : 3; }

// Diagnostic only: the contraction launchers note which kernel instantiation they enqueued last ON THIS THREAD, so that
// a benchmark can name the kernel it actually timed (agcn_last_kernel()).  Never read by any compute path.
#include <stdio.h>
inline thread_local char agcn_last_kernel_buf[192] = "";
#define AGCN_NOTE_KERNEL(...) snprintf(agcn_last_kernel_buf, sizeof(agcn_last_kernel_buf), __VA_ARGS__)

static inline int agcn_check_launch() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? AGCN_OK : (int)e;
}

// Launch a kernel that needs more than the default 64 KB of dynamic LDS: raise its limit to 160 KB on the CURRENT
// device once per (kernel, device), launch, return agcn_check_launch().  Keyed by the kernel itself (instantiations of
// one template share a function TYPE).  hipFuncSetAttribute is per device, and forward / autograd-backward threads may
// reach a first launch together: the flags are atomics and a lost race only repeats the idempotent call.
#define AGCN_MAX_DEVICES 64
template <auto KERN, class... Args>
static inline int agcn_launch_big(dim3 grid, dim3 block, size_t smem_bytes, hipStream_t stream, const Args&... args) {
  static unsigned char done[AGCN_MAX_DEVICES] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= AGCN_MAX_DEVICES) dev = -1;
  if (dev < 0 || !__atomic_load_n(&done[dev], __ATOMIC_ACQUIRE)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       160 * 1024);
    if (e != hipSuccess) return (int)e;
    if (dev >= 0) __atomic_store_n(&done[dev], (unsigned char)1, __ATOMIC_RELEASE);
  }
  hipLaunchKernelGGL(KERN, grid, block, smem_bytes, stream, args...);
  return agcn_check_launch();
}
