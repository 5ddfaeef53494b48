/* agcn_hip.h -- C ABI of libagcn_hip.so: the 2s-AGCN hot path (unit_gcn / unit_tcn / TCN_GCN_unit forward and
 * backward, and the clip+SGD tail of the training step) as hand-written gfx950 (MI355X, CDNA4) HIP kernels.
 *
 * The reference (cheneeheng/2s-AGCN) is pure Python/PyTorch and has no FFI for this path; every entry point below
 * replaces the stock ATen operators that one line range of the reference launches (cited per function as
 * agcn.py:<lines> = model/architecture/aagcn/agcn.py, processor.py = utils/processor.py).  INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to contiguous fp32 owned by the caller (PyTorch's caching allocator in our
 *    host code), with one exception by name: a `const int* host_<name>` parameter is a HOST array (the parent table of
 *    agcn_streams_*); the library never allocates, frees or keeps device memory; scratch/workspace is passed in and its
 *    size is given by the matching *_workspace / *_scratch_bytes / *_num_* query;
 *  - activations are (N, C, T, V) row-major ("NCHW"), N = batch*persons, V <= 32 joints, P = T*V;
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises the device, the
 *    functions are re-entrant and hold no mutable global state (forward and autograd-backward threads may call
 *    concurrently).  What the library does keep is set-once and idempotent: the AGCN_* environment switches are read
 *    on first use and never change afterwards, and the per-(kernel, device) "dynamic LDS limit raised" flags are
 *    atomics whose lost race only repeats an idempotent hipFuncSetAttribute;
 *  - return value: 0 = ok, AGCN_ERR_* (negative) = argument/shape problem detected on the host before any launch,
 *    positive = hipError_t of a failed launch.  Nothing throws or aborts.
 *  - results are bitwise reproducible run to run (no float atomics; all cross-workgroup sums go through slabs that
 *    are added in a fixed order).
 */
#ifndef AGCN_HIP_H
#define AGCN_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGCN_OK 0
#define AGCN_ERR_ARG (-1)         /* null pointer / non-positive size / V > 32 */
#define AGCN_ERR_WORKSPACE (-2)   /* workspace smaller than the query says */
#define AGCN_ERR_UNSUPPORTED (-3) /* taps not in {1,9}, stride not in {1,2}, element count not a multiple of 4 ... */

/* load-time checks */
int agcn_version(void);          /* 100 = 0.1.0 */
const char* agcn_arch(void);     /* "gfx950" */

/* diagnostics (never used by a compute path): the kernel instantiation the calling thread's last contraction launch
 * enqueued, and the arithmetic mode of the channel contractions ("bf16x6" = fp32-equivalent 6-product bf16 split,
 * "f32" = exact-f32 MFMA, "bf16x3"), read once per process from the environment variable AGCN_GEMM */
const char* agcn_last_kernel(void);
const char* agcn_gemm_mode(void);
/* arithmetic of the aggregate+project chain: "f16x3" (two fp16 pieces per operand, three products, operands range-scaled
 * by the tensor maximum) in the default mode, "bf16x6" with AGCN_CHAIN_F16X3=0, else agcn_gemm_mode() */
const char* agcn_chain_mode(void);

/* ---- tile geometry queries (sizes of the partial slabs below) ---------------------------------------------------- */
int agcn_conv_tile_frames(int V, int T_out);     /* frames per position tile of the contraction kernels (256/V) */
int agcn_conv_num_tiles(int V, int T_out);       /* default tiles per sample */
int agcn_conv_stats_tiles(int Cin, int Cout, int T_out, int V, int taps, int stride);   /* agcn_conv_fwd: stats_part has N * this many slots */
int agcn_scores_num_tiles(int V, int T);         /* tiles per sample of the adjacency-score kernels */
int agcn_dadj_num_slots(int C, int V, int T);    /* slots per (sample, subset) of the adjacency-gradient slab */

/* ---- channel contractions: unit_tcn's Conv2d((k,1), stride (s,1), pad ((k-1)/2,0)) and every 1x1 Conv2d ------------
 * replaces: nn.Conv2d forward/backward at agcn.py:40-41,49 (unit_tcn.conv), :66-68,99-100 (conv_a/conv_b),
 *           :73 (down conv), and the kernel_size=1 residual unit_tcn at :125.   taps in {1,9}, stride in {1,2}.
 * w: (Cout, Cin, taps, 1) as in the reference state_dict.  stats_part (optional, may be NULL): per-channel partial
 * (sum, sum of squares) of y, layout [N*agcn_conv_num_tiles][2][Cout], consumed by agcn_bn_stats_finalize. */
size_t agcn_conv_workspace(int Cin, int Cout, int T, int V, int taps, int stride); /* fwd and bwd_data (packed weights) */
int agcn_conv_fwd(const float* x, const float* w, const float* bias, float* y, float* stats_part, void* workspace,
                  size_t workspace_bytes, int N, int Cin, int Cout, int T, int V, int taps, int stride, void* stream);
/* dx (+)= conv^T(dy) [+ add1*(mask1>0)] [+ add2*(mask2>0)]; add/mask are dx-shaped or NULL (mask NULL = no masking);
 * they fold the ReLU-masked identity-residual gradients (agcn.py:108-109,128-129) into the epilogue. */
int agcn_conv_bwd_data(const float* dy, const float* w, float* dx, int accumulate, const float* add1,
                       const float* mask1, const float* add2, const float* mask2, void* workspace,
                       size_t workspace_bytes, int N, int Cin, int Cout, int T, int V, int taps, int stride,
                       void* stream);
size_t agcn_conv_bwd_weight_workspace(int N, int Cin, int Cout, int T, int V, int taps, int stride);
int agcn_conv_bwd_weight(const float* dy, const float* x, float* dw, void* workspace, size_t workspace_bytes, int N,
                         int Cin, int Cout, int T, int V, int taps, int stride, void* stream);

/* ---- unit_gcn: graph aggregation fused with the conv_d projection --------------------------------------------------
 * replaces agcn.py:103-105:  y = sum_i conv_d[i]( matmul(x.view(N,C*T,V), A^_i) )   (three bmm + three 1x1 convs + adds)
 * adj: (N,3,V,V) = A^ from agcn_adjacency_fwd ; wcat: (Cout, 3*C) = [Wd_0 | Wd_1 | Wd_2] ; bias: sum of the three
 * conv_d biases (or NULL). */
size_t agcn_gcn_workspace(int C, int Cout, int T, int V);   /* aggregate fwd / bwd_data / dadj (packed weights) */
int agcn_gcn_stats_tiles(int C, int Cout, int T, int V);    /* stats_part slots per sample of the tile-per-workgroup kernels */
int agcn_gcn_stats_slots(int N, int C, int Cout, int T, int V);   /* TOTAL stats_part slots agcn_gcn_aggregate_project_fwd writes (what the caller allocates: the persistent kernel's count depends on N) */
int agcn_gcn_aggregate_project_fwd(const float* x, const float* adj, const float* wcat, const float* bias, float* y,
                                   float* stats_part, void* workspace, size_t workspace_bytes, int N, int C, int Cout,
                                   int T, int V, void* stream);
/* ---- operand maxima for the split-fp16 ("f16x3") temporal convolutions ------------------------------------------------
 * The f16x3 kernels scale their streamed operand by a power of two derived from the tensor's max |x|.  The
 * _ex variants let the kernel that PRODUCES a tensor leave that maximum behind (4-byte device scalar) and the kernel that
 * consumes it skip its own pass over the tensor; with NULL they behave exactly like the plain entry points. */
int agcn_bn_act_fwd_ex(const float* y1, const float* scale1, const float* shift1, const float* r, const float* scale2,
                       const float* shift2, float* out, unsigned* sign_bits, float* absmax_out, int N, int C, int P,
                       int res_mode, int relu, void* stream);
int agcn_bn_bwd_apply_ex(const float* part, int nrows, double count, float param_grad_scale, const float* dout,
                         const void* mask, int mask_bits, const float* y1, const float* gamma1, const float* mean1,
                         const float* invstd1, const float* y2, const float* gamma2, const float* mean2,
                         const float* invstd2, float* coef, float* dy1, float* dgamma1, float* dbeta1, float* dy2,
                         float* dgamma2, float* dbeta2, float* absmax1_out, int N, int C, int P, void* stream);
/* the aggregate+project chain runs on f16x3 too (agcn_chain_mode): x_absmax = max |x| (agcn_bn_act_fwd_ex of the previous
 * unit), dy_absmax = max |dy| (agcn_bn_bwd_apply_ex), dtp_absmax = max |dtp|; any of them NULL: a streaming pass inside.
 * agcn_gcn_aggregate_project_bwd_data_ex covers both backward-data forms: dtp NULL = the plain one, else the fused one.
 * agcn_gcn_dadj_ex: dy_absmax for the projection H = Wd^T dy, x_absmax (the forward's max |x|) for the reduction of H
 * against x, both on f16x3; NULL: a streaming pass inside (same bits either way). */
int agcn_gcn_aggregate_project_fwd_ex(const float* x, const float* adj, const float* wcat, const float* bias, float* y,
                                      float* stats_part, void* workspace, size_t workspace_bytes, int N, int C, int Cout,
                                      int T, int V, const float* x_absmax, void* stream);
int agcn_gcn_aggregate_project_bwd_data_ex(const float* dy, const float* adj, const float* wcat, const float* dtp,
                                           const float* w2, int K2, float* dx, int accumulate, const float* add1,
                                           const float* mask1, const float* add2, const float* mask2, int mask_bits,
                                           void* workspace, size_t workspace_bytes, int N, int C, int Cout, int T, int V,
                                           const float* dy_absmax, const float* dtp_absmax, void* stream);
int agcn_gcn_dadj_ex(const float* dy, const float* wcat, const float* x, float* dadj_part, void* workspace,
                     size_t workspace_bytes, int N, int C, int Cout, int T, int V, const float* dy_absmax,
                     const float* x_absmax, void* stream);
int agcn_adjacency_bwd_scores_ex(const float* tp, const float* dS, float* dtp, float* dbpart, void* scratch, float* db,
                                 float* dtp_absmax_out, int N, int Ci, int T, int V, void* stream);
/* weight gradients: with BOTH operand maxima given the tap-free gradients (1x1, stride 1, Cin a multiple of 64; the
 * projection gradient with C a multiple of 64, its aggregation included) run on f16x3; NULL: bf16x6 as the plain entry
 * points (no pass inside).  The 9-tap gradient (rows and channels multiples of 64) runs on f16x3 either way: its
 * transposing pre-pass writes the range-scaled fp16 planes and takes a missing maximum with a reduction pass of its own. */
int agcn_conv_bwd_weight_ex(const float* dy, const float* x, float* dw, void* workspace, size_t workspace_bytes, int N,
                            int Cin, int Cout, int T, int V, int taps, int stride, const float* dy_absmax,
                            const float* x_absmax, void* stream);
int agcn_gcn_project_bwd_weight_ex(const float* dy, const float* x, const float* adj, float* dwcat, void* workspace,
                                   size_t workspace_bytes, int N, int C, int Cout, int T, int V, const float* dy_absmax,
                                   const float* x_absmax, void* stream);
int agcn_absmax(const float* x, long n, float* out, void* stream);   /* *out = max |x|: the pass the f16x3 kernels run when given no maximum */
int agcn_conv_fwd_ex(const float* x, const float* w, const float* bias, float* y, float* stats_part, void* workspace,
                     size_t workspace_bytes, int N, int Cin, int Cout, int T, int V, int taps, int stride,
                     const float* x_absmax, void* stream);
int agcn_conv_bwd_data_ex(const float* dy, const float* w, float* dx, int accumulate, const float* add1,
                          const float* mask1, const float* add2, const float* mask2, void* workspace,
                          size_t workspace_bytes, int N, int Cin, int Cout, int T, int V, int taps, int stride,
                          const float* dy_absmax, void* stream);

/* ---- temporal convolution with any kernel size, stride and padding ----------------------------------------------------
 * replaces the convolution of TCNUnit(kernel_size, stride, pad) (reference aagcn.py:184-207: padding = (kernel_size-1)//2
 * if pad else 0) and of unit_tcn(kernel_size, stride) (agcn.py:36-50) for the configurations agcn_conv_* rejects (the
 * aagcn_vNN backbones: kernel_size 3, stride 3, pad False, aagcn_v17.py:202-204; kernel_size 3 stride 1 in v37).
 * Domain: 1 <= taps <= 9, 1 <= stride <= 9, 0 <= pad <= (taps-1)/2, T + 2 pad >= taps; T_out = (T + 2 pad - taps)/stride + 1.
 * Outside it: AGCN_ERR_UNSUPPORTED (bad pointers / sizes: AGCN_ERR_ARG), checked on the host before any launch.
 * Shapes agcn_conv_* covers (taps 1 or 9, pad (taps-1)/2, stride 1 or 2) run there unchanged; stride-1 3/5/7-tap
 * convolutions run on the split-bf16 / f16x3 kernels in those AGCN_GEMM modes; everything else (and AGCN_GEMM=f32) on the
 * exact-f32 kernels.  Frames of x that no window reaches receive a zero gradient.  The *_absmax arguments are those of
 * the _ex forms (NULL: a pass of its own where the f16x3 kernels need it).  Workspaces: agcn_tconv_workspace (forward,
 * backward-data), agcn_tconv_bwd_weight_workspace; stats_part: N * agcn_tconv_stats_tiles slots. */
size_t agcn_tconv_workspace(int Cin, int Cout, int T, int V, int taps, int stride, int pad);
int agcn_tconv_stats_tiles(int Cin, int Cout, int T_out, int V, int taps, int stride, int pad);
int agcn_tconv_fwd(const float* x, const float* w, const float* bias, float* y, float* stats_part, void* workspace,
                   size_t workspace_bytes, int N, int Cin, int Cout, int T, int V, int taps, int stride, int pad,
                   const float* x_absmax, void* stream);
int agcn_tconv_bwd_data(const float* dy, const float* w, float* dx, int accumulate, const float* add1,
                        const float* mask1, const float* add2, const float* mask2, void* workspace,
                        size_t workspace_bytes, int N, int Cin, int Cout, int T, int V, int taps, int stride, int pad,
                        const float* dy_absmax, void* stream);
size_t agcn_tconv_bwd_weight_workspace(int N, int Cin, int Cout, int T, int V, int taps, int stride, int pad);
int agcn_tconv_bwd_weight(const float* dy, const float* x, float* dw, void* workspace, size_t workspace_bytes, int N,
                          int Cin, int Cout, int T, int V, int taps, int stride, int pad, const float* dy_absmax,
                          const float* x_absmax, void* stream);

/* ---- unit_gcn forward of the first layer (1..4 input channels) ----------------------------------------------------------
 * replaces agcn.py:103-105 AND the `down` convolution (agcn.py:74-77, 108) for in_channels = 3 in one pass over x:
 * ypre = bias + sum_i Wd_i (x . adj_i), dpre = bdown + Wdown x (wdown (Cout, C) row-major or NULL), and the per-tile
 * (sum, sumsq) partials of both ([N * agcn_gcn_first_tiles][2][Cout], NULL to skip) for agcn_bn_stats_finalize. */
int agcn_gcn_first_supported(int C, int Cout, int V);
int agcn_gcn_first_tiles(int T, int V);
int agcn_gcn_first_fwd(const float* x, const float* adj, const float* wcat, const float* bias, const float* wdown,
                       const float* bdown, float* ypre, float* ystats, float* dpre, float* dstats, int N, int C, int Cout,
                       int T, int V, void* stream);

/* ---- BN-folded inference (eval mode) ---------------------------------------------------------------------------------
 * replaces, for model.eval() under no_grad, the whole of unit_gcn.forward after the adjacency (agcn.py:103-109) and of
 * unit_tcn.forward + the TCN_GCN_unit tail (agcn.py:48-50, 127-129): the caller folds every BatchNorm into the weights
 * and bias of the contraction in front of it (w' = w * gamma/sqrt(var+eps), b' = (b - mean) * gamma/sqrt(var+eps) + beta),
 * the residual add and the ReLU ride in the store epilogue.
 *   agcn_gcn_unit_infer: y = act( bias + sum_i W_i (x . adj_i) [+ res] [+ W2 . x2] ); res (N,Cout,T,V) or NULL (the
 *     identity `down`); x2 (N,K2,T,V) with w2 (Cout,K2) row-major or both NULL (the folded conv `down`, K2 % 32 == 0)
 *   agcn_conv9_infer:    y = act( bias + conv9x1(x; w (Cout,Cin,9,1), stride) [+ res] ); res (N,Cout,T_out,V) or NULL
 * Both return AGCN_ERR_UNSUPPORTED where only the exact-f32 kernels apply (C < 32, AGCN_GEMM=f32): run the unfused
 * passes then.  Workspace of agcn_conv9_infer: agcn_conv_workspace. */
size_t agcn_gcn_unit_infer_workspace(int C, int Cout, int K2, int T, int V);
int agcn_gcn_unit_infer(const float* x, const float* adj, const float* wcat, const float* bias, const float* res,
                        const float* x2, const float* w2, int K2, int relu, float* y, void* workspace,
                        size_t workspace_bytes, int N, int C, int Cout, int T, int V, void* stream);
int agcn_conv9_infer(const float* x, const float* w, const float* bias, const float* res, int relu, float* y,
                     void* workspace, size_t workspace_bytes, int N, int Cin, int Cout, int T, int V, int stride,
                     void* stream);

/* agcn_tconv_infer: the same fold for every temporal kernel of agcn_tconv_fwd, with AAGCN's three attention gates applied
 * to the operand on load.  Replaces, for model.eval() under no_grad, `y = x * se + x` three times (aagcn.py:264-271, with
 * a = 1 + se of SpatialAttention / TemporalAttention / ChannelAttention :59-116), TCNUnit.forward (:194-207) and the
 * TCNGCNUnit tail relu(tcn(gcn(x)) + residual(x)) (:316-321):
 *     y = act( bias + tconv(x * gate ; w (Cout,Cin,taps,1), stride, pad) [+ res] ),  gate[n,c,t,v] = a_s[n,v] a_t[n,t] a_c[n,c]
 * a_s (N,V), a_t (N,T), a_c (N,Cin): each optional, NULL = ones; res (N,Cout,T_out,V) or NULL; x_absmax: optional device
 * scalar max |x| of the ungated x (NULL: taken by a pass inside where the f16x3 kernels need it).  The gated tensor is
 * never written: the factors multiply the operand tile between its global load and the LDS image the matrix cores read.
 * Domain and workspace (agcn_tconv_workspace) of agcn_tconv_fwd; AGCN_ERR_UNSUPPORTED outside it, nothing is launched. */
int agcn_tconv_infer(const float* x, const float* w, const float* bias, const float* a_s, const float* a_t,
                     const float* a_c, const float* res, int relu, float* y, void* workspace, size_t workspace_bytes,
                     int N, int Cin, int Cout, int T, int V, int taps, int stride, int pad, const float* x_absmax,
                     void* stream);

/* mask_bits = 1: mask1/mask2 are sign bit masks of agcn_bn_act_fwd (cast to const float*), 0: fp32 tensors (> 0 passes) */
int agcn_gcn_aggregate_project_bwd_data(const float* dy, const float* adj, const float* wcat, float* dx,
                                        int accumulate, const float* add1, const float* mask1, const float* add2,
                                        const float* mask2, int mask_bits, void* workspace, size_t workspace_bytes, int N, int C,
                                        int Cout, int T, int V, void* stream);
/* the same plus the 1x1 term of the adaptive branch in one pass: dx (+)= ... + w2^T dtp, dtp (N, K2, T, V), w2 (K2, C)
 * row-major = the stacked conv_a/conv_b weights (reference agcn.py:99-100 differentiated).  Chained (bf16x6) path only:
 * agcn_gcn_bwd_data_fused_supported() tells; workspace as agcn_gcn_workspace(C, Cout, T, V). */
int agcn_gcn_bwd_data_fused_supported(int C, int Cout, int V);
int agcn_gcn_aggregate_project_bwd_data_fused(const float* dy, const float* adj, const float* wcat, const float* dtp,
                                              const float* w2, int K2, float* dx, int accumulate, const float* add1,
                                              const float* mask1, const float* add2, const float* mask2, int mask_bits,
                                              void* workspace, size_t workspace_bytes, int N, int C, int Cout, int T,
                                              int V, void* stream);
size_t agcn_gcn_project_bwd_weight_workspace(int N, int C, int Cout, int T, int V);
int agcn_gcn_project_bwd_weight(const float* dy, const float* x, const float* adj, float* dwcat, void* workspace,
                                size_t workspace_bytes, int N, int C, int Cout, int T, int V, void* stream);
/* dadj_part: (N, 3, agcn_dadj_num_slots, V, V) partial adjacency gradients, summed by agcn_adjacency_bwd_softmax */
int agcn_gcn_dadj(const float* dy, const float* wcat, const float* x, float* dadj_part, void* workspace,
                  size_t workspace_bytes, int N, int C, int Cout, int T, int V, void* stream);

/* ---- adaptive adjacency ------------------------------------------------------------------------------------------------
 * replaces agcn.py:95,99-102:  A^_i = softmax_{dim -2}( theta_i^T phi_i / (Ci*T) ) + A_i + PA_i
 * tp: (N, 6*Ci, T, V), rows [theta_0|phi_0|theta_1|phi_1|theta_2|phi_2] (one agcn_conv_fwd with the six 1x1 weights
 * stacked).  A: (3,V,V) constant graph (NULL for the AAGCN form), PA: (3,V,V) parameter, alpha: 1 float or NULL
 * (AAGCN: A^ = PA + alpha*P, aagcn.py:172-173).  spart: scratch (N,3,agcn_scores_num_tiles,V,V).
 * Outputs P (softmax, kept for the backward) and adj, both (N,3,V,V). */
int agcn_adjacency_fwd(const float* tp, const float* A, const float* PA, const float* alpha, float* spart, float* P,
                       float* adj, int N, int Ci, int T, int V, void* stream);
/* The same WITHOUT the theta/phi tensor in HBM (SURVEY Appendix A "kernel A"): x (N,C,T,V) is read once per
 * workgroup tile, [theta;phi] = wab . x + bab (wab: (6*Ci, C) stacked conv_a/conv_b weights, rows as tp above) lives in
 * accumulators/LDS only and is reduced into spart on the spot; then the finalize above.  _bwd_scores recomputes the
 * tile and writes dtp / db exactly as agcn_adjacency_bwd_scores does from a stored tp.  tp_out (may be NULL): if
 * given, the forward also leaves theta/phi (N, 6*Ci, T, V) in HBM as a by-product (coalesced rows from the LDS tile)
 * for a backward that prefers re-reading to recomputing (measured faster on MI355X).  workspace: packed split
 * weights, agcn_adjacency_fused_workspace(C, Ci) bytes.  agcn_adjacency_fused_supported: Ci in {16,32,64}, bf16x6
 * arithmetic (AGCN_GEMM default); otherwise use agcn_conv_fwd + agcn_adjacency_fwd. */
int agcn_adjacency_fused_supported(int C, int Ci, int T, int V);
size_t agcn_adjacency_fused_workspace(int C, int Ci);
int agcn_adjacency_fused_fwd(const float* x, const float* wab, const float* bab, const float* A, const float* PA,
                             const float* alpha, float* tp_out, float* spart, float* P, float* adj, void* workspace,
                             size_t workspace_bytes, int N, int C, int Ci, int T, int V, void* stream);
/* same; x_absmax_out (optional, 4 bytes) receives max |x| as a by-product of the pass that reads all of x, for the f16x3
 * aggregate+project chain that reads x next (agcn_gcn_aggregate_project_fwd_ex); x_absmax_in (optional): max |x| where the
 * producer of x left it behind (the persistent kernel of the Ci <= 32 layers scales x by it; without it a reduction pass
 * takes the maximum first) */
int agcn_adjacency_fused_fwd_ex(const float* x, const float* wab, const float* bab, const float* A, const float* PA,
                                const float* alpha, float* tp_out, float* spart, float* P, float* adj, float* x_absmax_out,
                                const float* x_absmax_in, void* workspace, size_t workspace_bytes, int N, int C, int Ci, int T,
                                int V, void* stream);
int agcn_adjacency_fused_bwd_scores(const float* x, const float* wab, const float* bab, const float* dS, float* dtp,
                                    float* dbpart, void* scratch, float* db, void* workspace, size_t workspace_bytes,
                                    int N, int C, int Ci, int T, int V, void* stream);
/* dadj = sum of slots; dS = alpha*P*(dadj - sum_u P*dadj)/(Ci*T); dPA = sum_n dadj; dalpha_part (N*3) or NULL */
int agcn_adjacency_bwd_softmax(const float* dadj_part, const float* P, const float* alpha, float* dadj, float* dS,
                               float* dPA, float* dalpha_part, int N, int Ci, int T, int V, int nslots, void* stream);
/* dtp from dS; db (6*Ci) = bias gradients of the stacked conv_a/conv_b; dbpart: scratch (N*tiles, 6*Ci);
 * scratch: agcn_colsum_scratch_bytes(6*Ci) bytes */
int agcn_adjacency_bwd_scores(const float* tp, const float* dS, float* dtp, float* dbpart, void* scratch, float* db,
                              int N, int Ci, int T, int V, void* stream);

/* ---- BatchNorm2d (train/eval) + residual + ReLU ---------------------------------------------------------------------
 * replaces agcn.py:43,49 (unit_tcn.bn), :74 (down BN), :79,107-109 (unit_gcn.bn, += down(x), relu), :128-129
 * (TCN_GCN_unit: + residual, relu).  eps 1e-5, momentum 0.1, biased variance for normalisation, unbiased for
 * running_var -- the nn.BatchNorm2d defaults the reference uses. */
size_t agcn_colsum_scratch_bytes(int W);
int agcn_colsum(const float* X, int nslots, int W, void* scratch, float* out, void* stream);
int agcn_bn_stats_finalize(const float* stats_part, int nslots, int C, double count, const float* gamma,
                           const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                           void* scratch /* agcn_colsum_scratch_bytes(2*C) */, float* mean, float* invstd,
                           float* scale, float* shift, void* stream);
int agcn_bn_eval_coeff(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                       float eps, int C, float* scale, float* shift, void* stream);
/* out = act(scale1[c]*y1 + shift1[c] + res); res_mode 0: none, 1: r, 2: scale2[c]*r + shift2[c]; N*C*P % 4 == 0.
 * sign_bits (optional, may be NULL): ceil(N*C*P/32) words, bit e of word w = (out[32*w + e] > 0): the ReLU mask the
 * backward needs, 32x smaller than `out`. */
int agcn_bn_act_fwd(const float* y1, const float* scale1, const float* shift1, const float* r, const float* scale2,
                    const float* shift2, float* out, unsigned* sign_bits, int N, int C, int P, int res_mode, int relu,
                    void* stream);
/* train-mode backward of out = relu(bn1(y1) [+ bn2(y2)] [+ identity]); mask (NULL: no ReLU) is either the fp32 `out`
 * tensor (mask_bits = 0: positive elements pass) or the sign_bits of agcn_bn_act_fwd (mask_bits = 1);
 * part: scratch N*C*3 floats, coef: scratch 6*C floats */
/* the two stages of agcn_bn_bwd, exposed so that a synchronised BatchNorm (reference utils/processor.py:295) can
 * all-reduce the per-channel sums between them: part is (N*C*3); apply sums `nrows` rows of it per channel, uses
 * `count` elements per channel and scales dgamma/dbeta by param_grad_scale. */
int agcn_bn_bwd_reduce(const float* dout, const void* mask, int mask_bits, const float* y1, const float* y2, float* part,
                       int N, int C, int P, void* stream);
int agcn_bn_bwd_apply(const float* part, int nrows, double count, float param_grad_scale, const float* dout,
                      const void* mask, int mask_bits, const float* y1, const float* gamma1, const float* mean1,
                      const float* invstd1, const float* y2, const float* gamma2, const float* mean2, const float* invstd2, float* coef,
                      float* dy1, float* dgamma1, float* dbeta1, float* dy2, float* dgamma2, float* dbeta2, int N, int C,
                      int P, void* stream);
int agcn_bn_bwd(const float* dout, const void* mask, int mask_bits, const float* y1, const float* gamma1,
                const float* mean1, const float* invstd1, const float* y2, const float* gamma2, const float* mean2, const float* invstd2,
                float* part, float* coef, float* dy1, float* dgamma1, float* dbeta1, float* dy2, float* dgamma2,
                float* dbeta2, int N, int C, int P, void* stream);
/* eval-mode (frozen statistics) backward of the same stage, scale = gamma * rsqrt(running_var + eps): one streaming pass
 *   dz = dout*mask ; dy1 = scale1[c]*dz ; dy2 = scale2[c]*dz (branch 2 exists iff scale2 != NULL) ; absmax1_out
 *   (optional, 4 bytes) = max |dy1| ; want_sums = 1: part[(n*C + c)*3 + k] = per-row (sum dz, sum dz*y1, sum dz*y2).
 * want_sums = 0 reads neither y1 nor y2 and does not touch part (all three may be NULL): the input-gradient-only case.
 * Any N*C*P (rows of P % 4 != 0 included); mask as in agcn_bn_bwd_reduce.
 * agcn_bn_bwd_eval_finalize sums the `nrows` rows of part per channel in double, in row order:
 *   dbeta = S0 ; dgamma = invstd*(S1 - mean*S0) ; dbias (optional) = scale*S0, the gradient of the bias of the
 *   convolution in front of the BatchNorm -- not zero in eval mode, unlike train mode where the batch mean cancels it.
 * agcn_bn_eval_coeff_ex: agcn_bn_eval_coeff (same scale / shift bits) that also copies out the frozen mean and
 *   invstd = 1/sqrt(running_var + eps) the finalize takes. */
int agcn_bn_eval_coeff_ex(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                          float eps, int C, float* scale, float* shift, float* mean, float* invstd, void* stream);
int agcn_bn_bwd_eval(const float* dout, const void* mask, int mask_bits, const float* y1, const float* scale1,
                     const float* y2, const float* scale2, int want_sums, float* part /* N*C*3 floats */, float* dy1,
                     float* dy2, float* absmax1_out, int N, int C, int P, void* stream);
int agcn_bn_bwd_eval_finalize(const float* part, int nrows, int C, const float* scale1, const float* mean1,
                              const float* invstd1, const float* scale2, const float* mean2, const float* invstd2,
                              float* dgamma1, float* dbeta1, float* dbias1, float* dgamma2, float* dbeta2,
                              float* dbias2, void* stream);

/* ---- AAGCN attention gates (config 4) ---------------------------------------------------------------------------------
 * replaces the full-tensor passes of aagcn.py:59-116, 268-270 (three "mean -> tiny net -> sigmoid -> y*s + y" gates):
 * agcn_stc_row_reduce: one pass over y (and optionally an elementwise factor g) giving, per (n, c) row,
 *     out_t[t] = scale_t * sum_v wv[n][v] * y*g   and/or   out_v[v] = scale_v * sum_t wt[n or row][t] * y*g
 *   (forward: mean_t y, mean_v y*(1+se_s); backward: the two weighted sums of dout*y in one pass, and sum_t dmv*y);
 * agcn_stc_apply: out = y * a_s[n,v] * a_t[n,t] * a_c[n,c] with a_* = 1 + sigmoid gate, (N,V) / (N,T) / (N,C);
 * agcn_stc_bwd_apply: dy = dout * a_s a_t a_c + dmv[n,c,t] * a_s[n,v] + dms[n,c,v] (the gradients that reach y through
 *   the two means folded into the same pass).  The gate networks themselves: agcn_gate_conv_* / agcn_linear_* below. */
int agcn_stc_row_reduce(const float* y, const float* g, const float* wv, const float* wt, int wt_per_row, float* out_t,
                        float* out_v, float scale_t, float scale_v, int N, int C, int T, int V, void* stream);
int agcn_stc_apply(const float* y, const float* a_s, const float* a_t, const float* a_c, float* out, int N, int C, int T,
                   int V, void* stream);
/* same; absmax_out (optional, 4 bytes) receives max |out| for the f16x3 temporal convolution that reads the gated tensor */
int agcn_stc_apply_ex(const float* y, const float* a_s, const float* a_t, const float* a_c, float* out, float* absmax_out,
                      int N, int C, int T, int V, void* stream);
int agcn_stc_bwd_apply(const float* dout, const float* a_s, const float* a_t, const float* a_c, const float* dmv,
                       const float* dms, float* dy, int N, int C, int T, int V, void* stream);

/* ---- the small operators around the unit stack, deterministic (csrc/small_ops.hip) -----------------------------------
 * Every sum in a fixed order, no vendor library: the model path is bitwise reproducible from process to process
 * (MIOpen's Conv1d for the temporal gate was not: DESIGN.md section 3).
 *
 * data_bn  replaces agcn.py:143,163-165 (x.permute(0,4,3,1,2).view(N, M*V*C, T) -> BatchNorm1d -> view/permute ->
 *   (N*M, C, T, V)) and aagcn.py forward_preprocess.  x is the model input (N, C, T, V, M); channel ch = (m*V+v)*C + c.
 *   agcn_data_bn_stats: part [N][2][C*V*M] partial (sum, sumsq), finalised by agcn_bn_stats_finalize(part, N, C*V*M,
 *   count = N*T, ...); agcn_data_bn_apply: out[(n*M+m), c, t, v] = x[n,c,t,v,m]*scale[ch] + shift[ch];
 *   agcn_data_bn_bwd_reduce: part [N][2][C*V*M] partial (sum dy, sum dy*xhat) (agcn_colsum over N slots);
 *   agcn_data_bn_bwd_apply: dx from the GLOBAL sums [2][C*V*M] and the element count per channel behind them. */
int agcn_data_bn_stats(const float* x, float* part, int N, int C, int T, int V, int M, void* stream);
int agcn_data_bn_apply(const float* x, const float* scale, const float* shift, float* out, int N, int C, int T, int V,
                       int M, void* stream);
int agcn_data_bn_bwd_reduce(const float* dy, const float* x, const float* mean, const float* invstd, float* part, int N,
                            int C, int T, int V, int M, void* stream);
int agcn_data_bn_bwd_apply(const float* dy, const float* x, const float* gamma, const float* mean, const float* invstd,
                           const float* sums, double count, float* dx, int N, int C, int T, int V, int M, void* stream);
/* global average pool  replaces agcn.py:179-181 (x.view(N, M, C, -1).mean(3).mean(1)): x (N*M, C, P) -> pooled (N, C);
 * rowmean: scratch of N*M*C floats.  agcn_pool_bwd: dx[(n*M+m), c, p] = dpooled[n, c] / (M*P). */
int agcn_pool_fwd(const float* x, float* rowmean, float* pooled, int N, int M, int C, int P, void* stream);
int agcn_pool_bwd(const float* dpooled, float* dx, int N, int M, int C, int P, void* stream);
/* small Linear  replaces agcn.py:183 (self.fc) and aagcn.py:111-116 (fc1c -> ReLU -> fc2c -> sigmoid):
 * out[n, o] = act(b[o] + sum_k in[n, k] w[o, k]); act 0 identity, 1 ReLU, 2 "1 + sigmoid" (the gate's y*s + y factor).
 * agcn_linear_bwd: dpre (N, O) scratch = dout * act'(out); din (N, K, may be NULL), dw (O, K), db (O, may be NULL). */
int agcn_linear_fwd(const float* in, const float* w, const float* b, float* out, int N, int K, int O, int act,
                    void* stream);
int agcn_linear_bwd(const float* dout, const float* out, const float* in, const float* w, float* dpre, float* din,
                    float* dw, float* db, int N, int K, int O, int act, void* stream);
/* gate convolution  replaces aagcn.py:72-76 / 92-96 (Conv1d(C -> 1, Ks, padding (Ks-1)/2) + sigmoid on (N, C, L)):
 * a[n, l] = 1 + sigmoid(b + sum_c sum_k w[c, k] in[n, c, l + k - pad]); Ks odd.
 * agcn_gate_conv_bwd: da = gradient w.r.t. a; dpre (N, L) scratch; din (N, C, L), dw (C, Ks), db (1). */
int agcn_gate_conv_fwd(const float* in, const float* w, const float* b, float* a, int N, int C, int L, int Ks,
                       void* stream);
int agcn_gate_conv_bwd(const float* da, const float* a, const float* in, const float* w, float* dpre, float* din,
                       float* dw, float* db, int N, int C, int L, int Ks, void* stream);

/* ---- training-step tail on one flat parameter buffer ----------------------------------------------------------------
 * replaces processor.py:698 (clip_grad_norm_(params, 1.0)) + :703 (optimizer.step() of optim.SGD(momentum, nesterov,
 * weight_decay), :395-401).  grad_scale multiplies the gradient first (1/world_size after a SUM all-reduce).
 * norm_out: 2 device floats {global grad norm, clip coefficient}.  max_norm <= 0 disables clipping. */
size_t agcn_sgd_step_workspace(long n);
int agcn_sgd_step(float* param, const float* grad, float* momentum_buf, long n, float lr, float momentum,
                  float weight_decay, int nesterov, float max_norm, float grad_scale, int first_step, void* workspace,
                  size_t workspace_bytes, float* norm_out, void* stream);

/* ---- skeleton preprocessing on the device (online recognition, dataset generation) -------------------------------------
 * replaces infer/data_preprocess.py (DataPreprocessor.append_data, select_skeletons) and data_gen/preprocess.py
 * (pre_normalization).  A frame (joint) is null iff all its 3V (3) values are zero; the reference tests sum() == 0.
 *
 * skel_append: frame (Mmax, V, 3) -> slot `slot` of ring (Mmax, Tmax, V, 3).  `count` = frames present INCLUDING this
 *   one (1..Tmax; while count < Tmax the slot must be count - 1: the ring fills from slot 0 upward).  k > 1: once
 *   count >= k the slot holds the mean of the last k slots (sum oldest to newest in fp32, / k), the new frame included;
 *   earlier slots already hold averaged frames.  1 <= k <= Tmax.
 *
 * prenorm: in = N blocks (M, Tmax, V, 3); logical frame t of a block is slot (origin + t) mod Tmax (a plain tensor:
 *   origin 0, Tmax = T).  out (N, 3, T, V, K).  One workgroup per sample:
 *   select != 0: the K bodies of largest energy (sum over channels of the population std over valid frames x joints,
 *     fp64, fixed order), largest first, the higher index first among equals; else bodies 0..K-1.  sel (N, K) int32
 *     receives the indices, energy (N, M) the energies (only written, and only required, with select).
 *   pad != 0: a body whose frame 0 is null has its valid frames compacted to the front; frames after the last valid one
 *     repeat the frames before them cyclically.
 *   center: 0 none, 1 subtract the first selected body's joint 1 of the same (padded) frame, 2 that of its first
 *     non-null frame; null joints stay zero.
 *   (z0, z1): rotate the first body's frame-0 bone z1 - z0 onto z; (x0, x1): then x0 - x1 onto x; (zz0, zz1): then
 *   zz1 - zz0 onto z again.  A pair of -1 skips that rotation.  Matrices in fp64 (reference data_gen/rotation.py), their
 *   product applied once in fp32.
 *   AGCN_ERR_ARG: null pointer, V < 2, V > 32, T < 1, T > agcn_prenorm_max_frames() (2048: the per-body source-frame
 *   table lives in LDS), Tmax < T, origin outside [0, Tmax), M > 8, K < 1, K > M, an axis joint outside [0, V) or a
 *   half-given pair.  Every gathered index is clamped in the kernel as well.
 *
 * prenorm_windows: prenorm with per-sample addressing read on the device.  in = a pool of `nblocks` blocks
 *   (M, Tmax, V, 3); block, start, len = device int32 arrays of length N (block NULL: block 0 for every sample).  For
 *   t < len[n], logical frame t of sample n is slot (start[n] + t) mod Tmax of block block[n]; for t >= len[n] the frame
 *   is null: it reads as zeros and no memory is touched, whatever the slot holds (in a recording: a future frame).  The
 *   windows may overlap in any way: positions of one recording (nblocks 1, Tmax = its length), or the current windows of
 *   many rings (block = the ring, start = its oldest slot, len = its frame count).  The kernel clamps block into
 *   [0, nblocks), start into [0, Tmax) and len into [0, T], and every derived index as prenorm does: a wrong plan gives
 *   a wrong number, never an out-of-range read.  Outputs, options, limits and error codes are prenorm's (start and len
 *   may not be NULL); for the same logical window out, sel and energy are bit-identical to prenorm's.
 *
 * skel_smooth: a recording raw (L, Mmax, V, 3), time-major as frames arrive -> out (Mmax, L, V, 3), the layout the
 *   window kernel reads.  k = 1: a transposing copy.  k > 1: skel_append's recursion over the whole recording:
 *   out[t] = raw[t] while t + 1 < k, else (out[t-k+1] + ... + out[t-1] + raw[t]) / k, summed in that order in fp32:
 *   bit-identical to appending the frames one by one to a ring of any size >= k.  Serial in t, one thread per value.
 *   The k - 1 earlier outputs of a value are kept in LDS for k <= 33; beyond that the thread reads its own earlier
 *   stores back from `out` (same sums, more latency per frame).  1 <= k <= L, V <= 32.
 *
 * skel_append_many: skel_append for S rings (S, Mmax, Tmax, V, 3) and frames (S, Mmax, V, 3) in one launch.  slot, count
 *   = device int32 arrays of length S; slot[s] < 0: stream s has no frame this tick and its ring is untouched.  The
 *   kernel clamps slot into [0, Tmax) and count into [1, Tmax]; arithmetic and bits per stream are skel_append's.
 *   1 <= S <= 65535.
 *
 * None of these synchronises, allocates or copies to the host. */
int agcn_prenorm_max_frames(void);
int agcn_skel_append(const float* frame, float* ring, int Mmax, int Tmax, int V, int slot, int count, int k,
                     void* stream);
int agcn_prenorm(const float* in, float* out, int* sel, float* energy, int N, int M, int K, int T, int Tmax, int origin,
                 int V, int select, int pad, int center, int z0, int z1, int x0, int x1, int zz0, int zz1, void* stream);
int agcn_prenorm_windows(const float* in, float* out, int* sel, float* energy, const int* block, const int* start,
                         const int* len, int N, int nblocks, int M, int K, int T, int Tmax, int V, int select, int pad,
                         int center, int z0, int z1, int x0, int x1, int zz0, int zz1, void* stream);
int agcn_skel_smooth(const float* raw, float* out, int Mmax, int L, int V, int k, void* stream);
int agcn_skel_append_many(const float* frames, float* rings, const int* slot, const int* count, int S, int Mmax,
                          int Tmax, int V, int k, void* stream);

/* ---- transformer-encoder head of aagcn_v17 (csrc/encoder.hip; geometry in csrc/encoder_plan.h) ----
 * fp32 FMA in every AGCN_GEMM mode; no float atomics: every sum over rows, samples or heads has a fixed order, so all
 * outputs are bitwise reproducible.  Argument checks (AGCN_ERR_ARG: null pointer, size < 1, bad flag) and domain checks
 * (AGCN_ERR_UNSUPPORTED) come before any HIP call.  Domain: 1 <= L <= 640, 1 <= dh <= 256, D = H*dh <= 2048.
 *
 * tokens_fwd: x (N*M, C, T', V), cls (D) or NULL, pe (pe_rows >= L, D) or NULL -> tok (N, L, D), L = (cls ? 1 : 0) + M*T',
 *   D = V*C: tok[n, cls + m*T' + t, v*C + c] = x[n*M + m, c, t, v] + pe[l, v*C + c], tok[n, 0] = cls + pe[0]; the
 *   (C, T'*V) -> (T', V*C) transpose goes through LDS.
 * tokens_bwd: dtok -> dx (or NULL), dcls (D) = sum_n dtok[n, 0] (or NULL; needs has_cls), dpe (pe_rows, D) = sum_n dtok[n, l]
 *   for l < L and 0 for the rows behind (or NULL); n ascending.
 *
 * mha_fwd: qkv (N, L, 3D) as in_proj leaves it (q | k | v, head h at columns [h*dh, (h+1)*dh)); null_tok (N, L) uint8 or
 *   NULL: logit (i, j) is masked where both tokens are null; causal 0 none, 1 keeps j <= i, 2 keeps j >= i; keep
 *   (N, H, L, L) uint8 or NULL with keep_scale: the dropout of the probabilities.  Logits q.k / sqrt(dh); masked logits
 *   are removed before a max-subtracted softmax; a fully masked row has all-zero probabilities and a zero ctx row.
 *   Outputs: ctx (N, L, D); prob (N, H, L, L) or NULL, the softmax BEFORE dropout (what mha_bwd reads); avg (N, L, L) or
 *   NULL, the mean over heads of the probabilities AFTER dropout.
 * mha_bwd: dctx, qkv, prob, keep, keep_scale as in the forward -> dqkv (N, L, 3D), every element written:
 *   dV = P_d^T dctx, dP = (dctx V^T) * keep * keep_scale, dS = P o (dP - rowsum(dP o P)), dQ = dS K / sqrt(dh),
 *   dK = dS^T Q / sqrt(dh).  ws: scratch of N*H*L*L floats (dS), else AGCN_ERR_WORKSPACE.
 *
 * ln_fwd: out = LayerNorm(a + b) over rows of D (b NULL: of a), biased variance; mean, rstd (R) are kept for ln_bwd.
 * ln_bwd: dy -> dx = d(a + b), dgamma, dbeta (D); the normalised value is recomputed from a, b, mean, rstd (gamma may be
 *   0).  ws: (min(R, 1024) + 3) * 2 * D floats suffice for the partial sums (one row per wave, reduced in order), else
 *   AGCN_ERR_WORKSPACE.  D <= 2048. */
int agcn_tokens_fwd(const float* x, const float* cls, const float* pe, int pe_rows, float* tok, int N, int M, int C,
                    int Tp, int V, void* stream);
int agcn_tokens_bwd(const float* dtok, float* dx, float* dcls, float* dpe, int has_cls, int pe_rows, int N, int M, int C,
                    int Tp, int V, void* stream);
int agcn_mha_fwd(const float* qkv, const unsigned char* null_tok, int causal, const unsigned char* keep, float keep_scale,
                 float* ctx, float* prob, float* avg, int N, int L, int H, int dh, void* stream);
int agcn_mha_bwd(const float* dctx, const float* qkv, const float* prob, const unsigned char* keep, float keep_scale,
                 float* dqkv, void* ws, size_t ws_bytes, int N, int L, int H, int dh, void* stream);
int agcn_ln_fwd(const float* a, const float* b, const float* gamma, const float* beta, float eps, float* out, float* mean,
                float* rstd, long R, int D, void* stream);
int agcn_ln_bwd(const float* dy, const float* a, const float* b, const float* gamma, const float* mean, const float* rstd,
                float* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, long R, int D, void* stream);

/* ---- spatial transformer head of aagcn_v24 (csrc/encoder.hip; geometry in csrc/encoder_plan.h) ----
 * The same rules as the entries above: fp32 FMA, no float atomics, fixed summation orders, bitwise reproducible outputs,
 * AGCN_ERR_ARG / AGCN_ERR_UNSUPPORTED before any HIP call.  Sums over sequences take two stages: slot b of a slab holds
 * the sum over the sequences [32 b, 32 b + 32) in ascending order, the slots are then added in the fixed order of the
 * LayerNorm slab (16 interleaved chains, then the 16 chain sums in order).
 *
 * tokens_spatial_fwd: x (N*M, C, T', V), cls (C) or NULL, pe (pe_rows >= L, C) or NULL -> tok (N*T', L, C),
 *   L = (cls ? 1 : 0) + M*V: tok[n*T' + t, cls + m*V + v, c] = x[n*M + m, c, t, v] + pe[cls + m*V + v, c],
 *   tok[n*T' + t, 0] = cls + pe[0].  Domain: L <= 640, C <= 2048, C * (V | 1) <= 8192, N*T' <= 2 097 120.
 * tokens_spatial_bwd: dtok -> dx (or NULL), dcls (C) = sum over the N*T' sequences of dtok[s, 0] (or NULL; needs has_cls),
 *   dpe (pe_rows, C) = the same sum of dtok[s, l] for l < L and 0 for the rows behind (or NULL).  ws: the slab,
 *   tokens_spatial_bwd_workspace bytes (0 outside the domain), needed when dcls or dpe is asked for.
 *
 * mha_bias_fwd: mha_fwd with bias (Hb, L, L), Hb = 1 (one slice for all heads) or H (slice h for head h; anything else is
 *   AGCN_ERR_ARG): logits q.k / sqrt(dh) + bias, added before the masks and before the row maximum is taken.  mha_bwd
 *   serves both forwards: the bias changes prob, not the formulas.
 * mha_bias_grad: ds (N, H, L, L), the scratch mha_bwd has filled -> dbias (Hb, L, L) = sum_n (sum_h when Hb = 1) of
 *   ds[n, h], n ascending, h ascending inside n.  ws: mha_bias_grad_workspace bytes (0 outside the domain). */
int agcn_tokens_spatial_fwd(const float* x, const float* cls, const float* pe, int pe_rows, float* tok, int N, int M,
                            int C, int Tp, int V, void* stream);
size_t agcn_tokens_spatial_bwd_workspace(int N, int M, int C, int Tp, int V, int has_cls);
int agcn_tokens_spatial_bwd(const float* dtok, float* dx, float* dcls, float* dpe, int has_cls, int pe_rows, void* ws,
                            size_t ws_bytes, int N, int M, int C, int Tp, int V, void* stream);
int agcn_mha_bias_fwd(const float* qkv, const float* bias, int Hb, const unsigned char* null_tok, int causal,
                      const unsigned char* keep, float keep_scale, float* ctx, float* prob, float* avg, int N, int L,
                      int H, int dh, void* stream);
size_t agcn_mha_bias_grad_workspace(int N, int L, int H, int Hb);
int agcn_mha_bias_grad(const float* ds, float* dbias, void* ws, size_t ws_bytes, int N, int L, int H, int Hb,
                       void* stream);

/* ---- base SGN, eval-mode inference (csrc/sgn.hip; geometry and weight-image layouts in csrc/sgn_plan.h) ----
 * The model the reference's online recogniser deploys (model/architecture/sgn/archiv/sgn.py, infer/inference.py:129-150)
 * as three launches.  Exact-f32 MFMA in every AGCN_GEMM mode, fixed summation orders, no atomics: outputs are bitwise
 * reproducible and a clip's result does not depend on the batch it is in.  Argument checks (AGCN_ERR_ARG) and domain
 * checks (AGCN_ERR_UNSUPPORTED) come before any HIP call; none of the entries synchronises, allocates or reads the
 * environment.
 *
 * sgn_frames_weights / sgn_clip_weights: floats of the folded weight images (0 outside the domain).  The images are
 *   built by the caller (model/sgn.py::SGN._images): every BatchNorm folded, every matrix stored (K, N) row-major, in the order of
 *   SgnFramesW / SgnClipW.
 *
 * sgn_frames: the joint-level module (sgn.py:69-87), one workgroup per frame.  x (N, seg, V*3) -> feat (N, seg, 256),
 *   the maximum over the joints of gcn3's output (what local.maxpool, sgn.py:168, leaves when step == seg); g
 *   (N, seg, V, V) = softmax(g1(x)^T g2(x)) (sgn.py:206-211) is stored unless g is NULL.  dif (sgn.py:73-75) is zero at
 *   the first frame of every clip.  The V joint rows are padded to 32 for the matrix cores; padded rows enter neither
 *   the softmax, nor g.x, nor the maximum.  V in [2, 32], seg >= 1, in_channels 3, widths 64 / 128 / 256.
 *   AGCN_ERR_ARG: null x / w / feat, a size outside those limits, w_floats != sgn_frames_weights(V).
 *
 * sgn_clip: the frame-level module and the classifier (sgn.py:89-94, 167-177), one workgroup per clip.  feat
 *   (N, seg, 256) + tem1 -> 3-tap zero-padded temporal conv + bn1 + relu -> 1x1 conv 256 -> 512 + bn2 + relu -> maximum
 *   over the frames -> fc -> logits (N, num_class).  Dropout2d is the identity in eval.  num_class <= 4096.
 *
 * sgn_sample: NTUDataLoaders.to_fix_length, equal-interval branch (feeders/loader.py:203-232, 302-358), on normalised
 *   windows win (N, 3, T, V, K = 2) in prenorm's output layout, one workgroup per window.  Row (t, m) is kept iff body
 *   m's frame t is not all zero; kept rows in (t, m) order (zero-row deletion + turn_two_to_one); fewer than seg rows
 *   are followed by zero rows and L := seg (pad_to_segment_length); boundaries b_k = rint((double)k * ((double)L /
 *   (double)seg)); draw s takes row b_k + r[n, s, k] % (b_{k+1} - b_k) of interval k.  r (N, S, seg) uint32 -> out
 *   (N, S, seg, V*3), a bit-exact gather, and L (N) int32.  An empty window gives zeros and L = 0 (the reference raises).
 *   Every index is clamped: any r gives an in-range read.  T <= agcn_prenorm_max_frames().
 *   AGCN_ERR_ARG: null pointer, K != 2, V outside [2, 32], T, S or seg < 1, T too long. */
size_t agcn_sgn_frames_weights(int V);
size_t agcn_sgn_clip_weights(int seg, int num_class);
int agcn_sgn_frames(const float* x, const float* w, size_t w_floats, float* feat, float* g, int N, int seg, int V,
                    void* stream);
int agcn_sgn_clip(const float* feat, const float* w, size_t w_floats, float* logits, int N, int seg, int num_class,
                  void* stream);
int agcn_sgn_sample(const float* win, const unsigned* r, float* out, int* L, int N, int T, int V, int K, int S, int seg,
                    void* stream);

/* ---- base SGN, the training / evaluation collate (csrc/sgn.hip; plan and rotation in csrc/sgn_plan.h) ----
 * The reference's NTUDataLoaders.collate_fn_fix_train / _val / _test (feeders/loader.py:109-201) as one launch on a
 * dataset that lives on the device, one workgroup per clip, no atomics.
 *
 * sgn_collate: pool (P, 3, T, V, K = 2), a dataset in Feeder.__getitem__'s layout.  Workgroup n collates sample
 *   index[n] (int64), or sample n when index is null (then N <= P).  An index outside [0, P) gives an all-zero clip and
 *   L = 0, never a read outside the pool.  Sampling is sgn_sample's: r (N, S, seg) uint32 -> out (N, S, seg, V*3) and
 *   L (N) int32, the same rows, the same interval plan, the same bits.  subj (N, S, seg), may be null: the body
 *   (0.0 / 1.0) the picked row came from, 0.0 for a padding row (subject_seq after pad_to_segment_length).  angles
 *   (N, 3) radians, may be null: every joint p = (x, y, z) of every picked row of clip (n, s) becomes R_n . p with
 *   R = (Rz . Ry) . Rx in fp32 (feeders/tools.py::_rot, its sign convention, this association: sgn_rotation in
 *   sgn_plan.h); the S draws of a sample share R_n; padding rows stay exactly zero.
 *   AGCN_ERR_ARG: null pool / r / out / L, P < 1, index null and N > P, or outside sgn_sample's domain. */
int agcn_sgn_collate(const float* pool, const long long* index, const unsigned* r, const float* angles, float* out,
                     float* subj, int* L, long P, int N, int T, int V, int K, int S, int seg, void* stream);

/* ---- base SGN, input gradients in eval mode (csrc/sgn_bwd.hip; geometry in csrc/sgn_bwd_plan.h; the recomputed forward
 * is the forward's own device code, csrc/sgn_device.h) ----
 * What torch autograd does on the reference's eval forward (sgn.py:66-98) with respect to x (the parameter gradients
 * follow further down).  Same arithmetic rules as the forward: exact-f32 MFMA in every AGCN_GEMM mode, fixed summation orders, no
 * atomics, no launch reads another clip's intermediates, so a clip's gradient is the same bits alone and in any batch.
 * Nothing of the forward is stored: each kernel recomputes what it needs from x / feat.  ReLU's derivative at 0 is 0; a
 * maximum routes to its lowest index (MaxPool's choice; ties only happen at 0, where nothing flows).  Checks as above.
 *
 * sgn_frames_bwd_weights / sgn_clip_bwd_weights: floats of the TRANSPOSED weight images (0 outside the domain), built by
 *   the caller next to the forward images (model/sgn.py::SGN._images) in the order of SgnFramesWT / SgnClipWT: every
 *   matrix (N, K) row-major.  The kernels read the forward image as well (biases, 3 -> 64 layers, tem1, fc).
 * sgn_frames_bwd_workspace: bytes of the caller-owned workspace of sgn_frames_bwd (dj and dd, below).
 *
 * sgn_clip_bwd: feat (N, seg, 256), dlogits (N, num_class) -> dfeat (N, seg, 256), one workgroup per clip: fc
 *   (sgn.py:94), the maximum over the frames (sgn.py:92), local.cnn2 + bn2 + relu, local.cnn1 + bn1 + relu
 *   (sgn.py:169-175), + tem1 (sgn.py:89).  The conv's zero padding receives nothing; for seg > 32 a tile's gradient
 *   reaches one frame of either neighbouring tile, added in the order of the tiles.
 *
 * sgn_frames_bwd: x (N, seg, V*3), dfeat -> dx (N, seg, V*3), one workgroup per frame and a combining launch: the
 *   maximum over the joints (sgn.py:168), gcn3..1 (sgn.py:188-194) with dG, the softmax and g1 / g2 (sgn.py:206-211),
 *   the two embeddings and norm_data (sgn.py:76-81, 107-143).  spa1 and tem1 are input independent.  dif (sgn.py:73-75)
 *   couples neighbouring frames of a clip: every frame writes dj (joint branch) and dd (dif branch) to the workspace and
 *   dx[t] = dj[t] + dd[t] [t > 0] - dd[t + 1] [t + 1 < seg].  Padded joint rows and columns take part in nothing.
 *   AGCN_ERR_WORKSPACE: ws_bytes < sgn_frames_bwd_workspace(N, seg, V).
 *
 * sgn_sample_bwd: the adjoint of sgn_sample's gather (feeders/loader.py:203-232, 302-358): win, r as there, dout
 *   (N, S, seg, V*3) -> dwin (N, 3, T, V, 2), zeroed and then added to row by row in the order s major, k minor by the
 *   thread that owns the feature column.  Padding rows and empty windows contribute nothing. */
size_t agcn_sgn_frames_bwd_weights(int V);
size_t agcn_sgn_clip_bwd_weights(int seg, int num_class);
size_t agcn_sgn_frames_bwd_workspace(int N, int seg, int V);
int agcn_sgn_clip_bwd(const float* feat, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                      const float* dlogits, float* dfeat, int N, int seg, int num_class, void* stream);
int agcn_sgn_frames_bwd(const float* x, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                        const float* dfeat, float* dx, void* ws, size_t ws_bytes, int N, int seg, int V, void* stream);
int agcn_sgn_sample_bwd(const float* win, const unsigned* r, const float* dout, float* dwin, int N, int T, int V, int K,
                        int S, int seg, void* stream);

/* ---- base SGN, parameter gradients in eval mode (the two taping backward entries: csrc/sgn_bwd.hip; the size queries
 * and the reductions: csrc/sgn_wgrad.hip; geometry in csrc/sgn_wgrad_plan.h) ----
 * Frozen-BatchNorm fine-tuning: the gradient of a loss on the logits with respect to the two folded weight images, each
 * in its image's own layout (SgnFramesW / SgnClipW, the offsets of the forward image).  The caller takes them through
 * the fold to the parameters (model/sgn.py).  Arithmetic rules as above: exact-f32 MFMA, fixed summation orders, no
 * atomics.  Train-mode BatchNorm is not covered.
 *
 * sgn_frames_tape_floats / sgn_clip_tape_floats: floats of the caller-owned tapes (0 outside the domain).
 * sgn_wgrad_workspace: bytes of the workspace both wgrad entries take (the largest partial: elements of a section times
 *   the splits of its rows).  rows_per_split = 0 is the plan's default; tests pass small and odd values.
 * sgn_clip_bwd_tape / sgn_frames_bwd_tape: sgn_clip_bwd / sgn_frames_bwd with the same results bit for bit, which also
 *   copy every operand pair of a weight gradient to the tape (SgnClipTape / SgnFramesTape: the V real joint rows of a
 *   frame only, H with the convolution's two zero rows per clip, columns 64..127 of d x0, d xn before the folded scale).
 *   AGCN_ERR_WORKSPACE: tape_floats below the size query (or ws_bytes, as for sgn_frames_bwd).
 * sgn_frames_wgrad: x, the frames tape -> d_w (sgn_frames_weights(V) floats, every float written).  w is the forward
 *   image (not read at present: the tape holds every operand).  sgn_clip_wgrad: the clip tape, dfeat (N, seg, 256) as
 *   sgn_clip_bwd_tape returned it, dlogits -> d_w (sgn_clip_weights(seg, num_class) floats).  Each section is a launch
 *   over row splits that writes partials to ws and a launch that adds them in ascending split order.
 *   AGCN_ERR_WORKSPACE: ws_bytes < sgn_wgrad_workspace(...).  AGCN_ERR_ARG: null pointers, V outside [2, 32],
 *   num_class < 1, rows_per_split < 0. */
size_t agcn_sgn_frames_tape_floats(int N, int seg, int V);
size_t agcn_sgn_clip_tape_floats(int N, int seg, int num_class);
size_t agcn_sgn_wgrad_workspace(int N, int seg, int V, int num_class, int rows_per_split);
int agcn_sgn_clip_bwd_tape(const float* feat, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                           const float* dlogits, float* dfeat, int N, int seg, int num_class, float* tape,
                           size_t tape_floats, void* stream);
int agcn_sgn_frames_bwd_tape(const float* x, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                             const float* dfeat, float* dx, void* ws, size_t ws_bytes, int N, int seg, int V, float* tape,
                             size_t tape_floats, void* stream);
int agcn_sgn_frames_wgrad(const float* x, const float* w, const float* tape, float* d_w, void* ws, size_t ws_bytes, int N,
                          int seg, int V, int rows_per_split, void* stream);
int agcn_sgn_clip_wgrad(const float* tape, const float* dfeat, const float* dlogits, float* d_w, void* ws, size_t ws_bytes,
                        int N, int seg, int num_class, int rows_per_split, void* stream);

/* ---- base SGN, batch statistics of its seven BatchNorms (csrc/sgn_stats.hip; geometry in csrc/sgn_stats_plan.h) ----
 * The forward half of train-mode BatchNorm: what nn.BatchNorm1d / 2d measure in training mode in norm_data
 * (sgn.py:110-117), gcn_spa (sgn.py:183-194) and local (sgn.py:161-175) during one forward of the whole batch.
 * BatchNorm k sees activations normalised by the batch statistics of every BatchNorm in front of it, so the caller runs
 * the passes in dependency order, each on a folded weight image (sgn_frames_weights / sgn_clip_weights floats) in which
 * the earlier BatchNorms carry their batch statistics and the BatchNorm under measurement is folded as the identity
 * (scale 1, shift 0); the later sections of the image are not read.  A pass writes per group (a clip, a frame, a row
 * tile of a clip) and channel the sum and M2 = the sum of squares about the group's own mean to `part`
 * ((groups, 2, C) floats); sgn_stats_finalize merges the groups.  Arithmetic rules as above: exact-f32 MFMA, fixed
 * orders, no atomics; a group's partials do not depend on the batch around it.
 *
 * kind: 0 = input (layer 0), 1 = frames (layer 1..3 = gcn1..3.bn), 2 = clip (layer 1..2 = cnn.bn1, cnn.bn2; V ignored).
 * sgn_stats_part_floats: floats of `part` for a launch of N clips (0 outside the domain).  sgn_stats_channels: C.
 * sgn_input_stats: x (N, seg, V*3) -> C = 2 * 3V channels: x[:, e], then dif[:, e] (sgn.py:73-75, zero at t = 0, which
 *   counts as a sample), e = v*3 + c; one group per clip, seg samples each.
 * sgn_frames_stats: sgn_frames cut off at gcn<layer>'s product (sgn.py:192, the input of the bn of sgn.py:193): C = 128, 256, 256; one
 *   group per frame, the V real joint rows each.  Checks as sgn_frames, AGCN_ERR_ARG for layer outside 1..3.
 * sgn_clip_stats: sgn_clip cut off at cnn1's (layer 1, sgn.py:169) or cnn2's (layer 2, sgn.py:173) output: C = 256, 512;
 *   one group per (clip, 32-frame tile), the tile's valid frames each.  Checks as sgn_clip, AGCN_ERR_ARG for layer
 *   outside 1..2.
 * sgn_stats_finalize: (count, sum, M2) of the groups of `part` merged by the pairwise update (Chan et al.) with the state
 *   in fp64 -> mean, biased variance (C floats each; both may be NULL when carry_out is given).  Two launches: one thread
 *   per (clip, channel) merges the clip's groups in ascending group index into ws ((N, 3, C) doubles), then one thread
 *   per channel merges the clips in ascending clip index: the order is a function of the group index alone.  carry_in /
 *   carry_out: optional (3, C) doubles (count, mean, M2) under / after the clips, so that a batch processed in chunks of
 *   whole clips merges in the order of one launch and gives the same bits.  sgn_stats_finalize_workspace: bytes of ws.
 *   AGCN_ERR_WORKSPACE: part_floats or ws_bytes below their size queries. */
size_t agcn_sgn_stats_part_floats(int kind, int layer, int N, int seg, int V);
size_t agcn_sgn_stats_channels(int kind, int layer, int V);
int agcn_sgn_input_stats(const float* x, float* part, size_t part_floats, int N, int seg, int V, void* stream);
int agcn_sgn_frames_stats(const float* x, const float* w, size_t w_floats, float* part, size_t part_floats, int layer,
                          int N, int seg, int V, void* stream);
int agcn_sgn_clip_stats(const float* feat, const float* w, size_t w_floats, float* part, size_t part_floats, int layer,
                        int N, int seg, int num_class, void* stream);
size_t agcn_sgn_stats_finalize_workspace(int kind, int layer, int N, int seg, int V);
int agcn_sgn_stats_finalize(const float* part, size_t part_floats, int kind, int layer, int N, int seg, int V,
                            const double* carry_in, double* carry_out, float* mean, float* var, void* ws, size_t ws_bytes,
                            void* stream);

/* ---- SGN v15, the attention SGN: eval-mode inference (csrc/sgn_v15.hip; the block: csrc/sgn_v15_device.h; geometry and
 * weight-image layouts: csrc/sgn_v15_plan.h) ----
 * reference model/architecture/sgn/sgn_v15.py in the structure of config/nturgbd-cross-view/train_sgn_v15.yaml: the base
 * SGN's input side, one pre-norm multi-head-attention block (model/layers/attention/crossattention.py::Transformer, one
 * layer, BatchNorm, relu) 128 -> 256 over the joints of a frame, and the same block 256 -> 512 over the frames of a clip.
 * heads, d_head, ff describe the block of the entry they are passed to.  Arithmetic rules as for the base SGN: exact-f32
 * MFMA in every AGCN_GEMM mode, fixed summation orders, no atomics; a clip's result does not depend on its batch.
 * Domain: N * seg <= 2097151 frames (sgn15_frames, as sgn_frames), N <= 524287 clips (sgn15_clip), 2 <= V <= 32,
 *   1 <= seg <= 32 (sgn15_clip; one row tile), heads * d_head and ff multiples of 128 up to 1024,
 *   d_head 16, 32, 64 or a multiple of 128.
 * sgn15_frames_weights / sgn15_clip_weights: floats of the folded weight images (0 outside the domain), built by the
 *   caller (model/sgn_v15.py::SGN._images) in the order of sgn_v15_plan.h.
 * sgn15_frames: x (N, seg, V*3) -> feat (N, seg, 256), the maximum over the real joints of the block's output (no ReLU
 *   in front: it may be negative); tem_emb is added by sgn15_clip, which gives the reference's bits (max_v(y + tem) =
 *   max_v(y) + tem).  attn (N*seg, heads, V, V) is stored unless NULL.
 * sgn15_clip: feat (N, seg, 256) -> logits (N, num_class): + tem_emb, the block, the maximum over the real frames, fc.
 *   attn (N, heads, seg, seg) is stored unless NULL.
 * AGCN_ERR_ARG: a null x / feat / w / logits, sizes outside the domain, w_floats different from the size query. */
size_t agcn_sgn15_frames_weights(int V, int heads, int d_head, int ff);
size_t agcn_sgn15_clip_weights(int seg, int num_class, int heads, int d_head, int ff);
int agcn_sgn15_frames(const float* x, const float* w, size_t w_floats, float* feat, float* attn, int N, int seg, int V,
                      int heads, int d_head, int ff, void* stream);
int agcn_sgn15_clip(const float* feat, const float* w, size_t w_floats, float* logits, float* attn, int N, int seg,
                    int num_class, int heads, int d_head, int ff, void* stream);

/* ---- SGN v15: input gradients in eval mode (csrc/sgn_v15_bwd.hip; the block backward: csrc/sgn_v15_device.h; geometry,
 * the transposed images and the LDS lifetimes: csrc/sgn_v15_bwd_plan.h) ----
 * The backward of sgn15_clip and sgn15_frames, in that order: dx = d sum(logits * dlogits) / dx.  Nothing of the forward is
 * stored: each kernel recomputes what it needs from x / feat with the forward's device code.  ReLU's derivative at 0 is 0;
 * a maximum (no ReLU in front of it: it may be negative) routes to its lowest index.  Arithmetic rules and domain as for
 * the forward; a clip's gradient does not depend on its batch.
 * sgn15_frames_bwd_weights / sgn15_clip_bwd_weights: floats of the TRANSPOSED weight images (0 outside the domain), built
 *   by the caller next to the forward images (model/sgn_v15.py::SGN._images) in the order of Sgn15FramesWT / Sgn15ClipWT:
 *   every matrix (N, K) row-major -- the second embedding layers (frames) and qkv_w, o_w, f1_w, f2_w of the block.  The
 *   kernels read the forward image as well (biases, 3 -> 64 layers, aff, tem, fc).
 * sgn15_frames_bwd_workspace: bytes of the caller-owned workspace of sgn15_frames_bwd (dj and dd, below).
 * sgn15_clip_bwd: feat (N, seg, 256) as sgn15_frames returns it, dlogits (N, num_class) -> dfeat (N, seg, 256), one
 *   workgroup per clip: fc, the maximum over the real frames, the block; tem_emb is a constant.
 * sgn15_frames_bwd: x (N, seg, V*3), dfeat -> dx (N, seg, V*3), one workgroup per frame and a combining launch: the
 *   maximum over the real joints, the block (its spa columns go nowhere), the two embeddings and their DataNorm.  The
 *   velocity couples neighbouring frames of a clip: every frame writes dj (position branch) and dd (velocity branch) to
 *   the workspace and dx[t] = dj[t] + dd[t] [t > 0] - dd[t + 1] [t + 1 < seg].
 * AGCN_ERR_ARG: a null pointer, sizes outside the domain, w_floats / wt_floats / ws_bytes different from the size
 *   queries. */
size_t agcn_sgn15_frames_bwd_weights(int V, int heads, int d_head, int ff);
size_t agcn_sgn15_clip_bwd_weights(int seg, int num_class, int heads, int d_head, int ff);
size_t agcn_sgn15_frames_bwd_workspace(int N, int seg, int V);
int agcn_sgn15_clip_bwd(const float* feat, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                        const float* dlogits, float* dfeat, int N, int seg, int num_class, int heads, int d_head, int ff,
                        void* stream);
int agcn_sgn15_frames_bwd(const float* x, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                          const float* dfeat, float* dx, void* ws, size_t ws_bytes, int N, int seg, int V, int heads,
                          int d_head, int ff, void* stream);

/* ---- SGN v15: parameter gradients in eval mode (the two taping backward entries: csrc/sgn_v15_bwd.hip; the size queries
 * and the reductions: csrc/sgn_v15_wgrad.hip on the kernels of csrc/sgn_wgrad_device.h; tapes and workspace:
 * csrc/sgn_v15_wgrad_plan.h) ----
 * Frozen-BatchNorm fine-tuning of the attention SGN: the gradient of a loss on the logits with respect to the two folded
 * weight images, each in its image's own layout (the offsets of sgn15_frames_weights / sgn15_clip_weights).  The caller
 * takes them through the fold to the parameters (model/sgn_v15.py).  Arithmetic rules and domain as above: exact-f32 MFMA,
 * fixed summation orders, no atomics.  heads, d_head, ff describe the block of the entry they are passed to.
 *
 * sgn15_frames_tape_floats / sgn15_clip_tape_floats: floats of the caller-owned tapes (0 outside the domain).
 * sgn15_wgrad_workspace: bytes of the workspace of ONE wgrad entry (the largest partial: elements of a section times the
 *   splits of its rows).  V > 0: sgn15_frames_wgrad with the spatial block's heads, d_head, ff (num_class is not read);
 *   V = 0: sgn15_clip_wgrad with the temporal block's.  rows_per_split = 0 is the plan's default; tests pass small and odd
 *   values.  0 outside the domain or for rows_per_split < 0.
 * sgn15_clip_bwd_tape / sgn15_frames_bwd_tape: sgn15_clip_bwd / sgn15_frames_bwd with the same results bit for bit, which
 *   also copy every operand pair of a weight gradient to the tape (Sgn15ClipTape / Sgn15FramesTape: one row per real frame
 *   of a clip / real joint of a frame with x, [dq | dk | dv], o, dx1, [relu(hidden) | x1], d hidden and dy of the block; the
 *   clip tape also the block's dX and the pooled maxima (N, 512), the frames tape the embeddings' operands, columns
 *   64..127 of the block's dX and d xn before the folded scale).  Checks as the untaped entries; AGCN_ERR_ARG for a null
 *   tape, AGCN_ERR_WORKSPACE for tape_floats below the size query.
 * sgn15_frames_wgrad: x, the frames tape -> d_w (sgn15_frames_weights floats, every float written).
 * sgn15_clip_wgrad: the clip tape, dlogits (N, num_class) -> d_w (sgn15_clip_weights floats, every float written).  Each
 *   section is a launch over row splits that writes partials to ws and a launch that adds them in ascending split order.
 *   AGCN_ERR_ARG: a null pointer, sizes outside the domain, rows_per_split < 0, d_w_floats different from the size query.
 *   AGCN_ERR_WORKSPACE: tape_floats or ws_bytes below their size queries.  Nothing is launched on an error. */
size_t agcn_sgn15_frames_tape_floats(int N, int seg, int V, int heads, int d_head, int ff);
size_t agcn_sgn15_clip_tape_floats(int N, int seg, int num_class, int heads, int d_head, int ff);
size_t agcn_sgn15_wgrad_workspace(int N, int seg, int V, int num_class, int heads, int d_head, int ff, int rows_per_split);
int agcn_sgn15_clip_bwd_tape(const float* feat, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                             const float* dlogits, float* dfeat, int N, int seg, int num_class, int heads, int d_head,
                             int ff, float* tape, size_t tape_floats, void* stream);
int agcn_sgn15_frames_bwd_tape(const float* x, const float* w, size_t w_floats, const float* wt, size_t wt_floats,
                               const float* dfeat, float* dx, void* ws, size_t ws_bytes, int N, int seg, int V, int heads,
                               int d_head, int ff, float* tape, size_t tape_floats, void* stream);
int agcn_sgn15_frames_wgrad(const float* x, const float* tape, size_t tape_floats, float* d_w, size_t d_w_floats, void* ws,
                            size_t ws_bytes, int N, int seg, int V, int heads, int d_head, int ff, int rows_per_split,
                            void* stream);
int agcn_sgn15_clip_wgrad(const float* tape, size_t tape_floats, const float* dlogits, float* d_w, size_t d_w_floats,
                          void* ws, size_t ws_bytes, int N, int seg, int num_class, int heads, int d_head, int ff,
                          int rows_per_split, void* stream);

/* ---- SGN v15: batch statistics of its block BatchNorms (csrc/sgn_v15_stats.hip; geometry in
 * csrc/sgn_v15_stats_plan.h; the merge: csrc/sgn_stats_device.h, shared with the base SGN) ----
 * The forward half of train-mode BatchNorm for the four BatchNorms of the two attention blocks: PreNorm's BatchNorm1d of
 * the attention (n_a, on the block's input x) and of the feed-forward (n_f, on x1 = attention + bo + x).  The two
 * DataNorms in front are measured by sgn_input_stats / sgn_stats_finalize(kind 0) above, unchanged.  The caller runs the
 * passes in dependency order, each on folded weight images (sgn15_frames_weights / sgn15_clip_weights floats) in which
 * the EARLIER BatchNorms carry their batch statistics.  A pass never reads a section that depends on the BatchNorm it
 * measures: layer 1 reads no block section at all, layer 2 reads qkv_w, qkv_b, o_w, o_b and never f1_*, f2_* or fc_*; no
 * identity fold is needed.  A pass writes per group and channel the sum and M2 = the sum of squares about the group's own
 * mean to `part` ((groups, 2, C) floats), reduced in fp32 over the real token rows of the LDS tile in ascending order;
 * sgn15_stats_finalize merges the groups.  Exact-f32 MFMA, fixed orders, no atomics; a group's partials do not depend on
 * the batch around it.
 *
 * kind: 1 = frames (the spatial block, C = 128; one group per frame, V samples each), 2 = clip (the temporal block,
 *   C = 256; one group per clip, seg samples each; V ignored).  layer: 1 = n_a, 2 = n_f.
 * sgn15_stats_part_floats: floats of `part` for a launch of N clips (0 outside the domain).  sgn15_stats_channels: C.
 * sgn15_frames_stats: sgn15_frames cut off at the complete token tile [pos + vel | spa] (layer 1) or behind the attention
 *   half of the block (layer 2).  Takes the whole frames image (w_floats as for sgn15_frames).
 * sgn15_clip_stats: sgn15_clip cut off behind its load of feat + tem (layer 1) or behind the attention half (layer 2).
 * sgn15_stats_finalize: as sgn_stats_finalize -- the groups of a clip in ascending index, then the clips in ascending
 *   index on top of carry_in, state (count, mean, M2) in fp64 -> mean, biased variance; carry_in / carry_out (3, C)
 *   doubles, so a batch processed in chunks of whole clips gives the bits of one launch.
 *   sgn15_stats_finalize_workspace: bytes of ws.
 * AGCN_ERR_ARG: a null pointer, non-positive sizes, V outside 2..32, kind or layer outside 1..2, w_floats different from
 *   the size query.  AGCN_ERR_UNSUPPORTED: sizes outside the domain of the forward launch the pass is cut from.
 *   AGCN_ERR_WORKSPACE: part_floats or ws_bytes below their size queries.  All before any launch. */
size_t agcn_sgn15_stats_part_floats(int kind, int layer, int N, int seg, int V);
size_t agcn_sgn15_stats_channels(int kind, int layer);
int agcn_sgn15_frames_stats(const float* x, const float* w, size_t w_floats, float* part, size_t part_floats, int layer,
                            int N, int seg, int V, int heads, int d_head, int ff, void* stream);
int agcn_sgn15_clip_stats(const float* feat, const float* w, size_t w_floats, float* part, size_t part_floats, int layer,
                          int N, int seg, int num_class, int heads, int d_head, int ff, void* stream);
size_t agcn_sgn15_stats_finalize_workspace(int kind, int layer, int N, int seg, int V);
int agcn_sgn15_stats_finalize(const float* part, size_t part_floats, int kind, int layer, int N, int seg, int V,
                              const double* carry_in, double* carry_out, float* mean, float* var, void* ws, size_t ws_bytes,
                              void* stream);

/* ---- bone and motion input streams from joint data (csrc/streams.hip; index arithmetic in csrc/streams_plan.h) ----
 * replaces the reference's offline passes over the dataset files: data_gen/gen_bone_data.py:40-55 (bone),
 * data_gen/gen_motion_data.py:18-31 (joint_motion, bone_motion), and their autograd transpose.  Tensors are contiguous
 * (N, C, T, V, M) fp32 on the device.
 *   bone[.., v, m] = x[.., v, m] - x[.., parent[v], m]                 (a joint that is its own parent gives exactly 0)
 *   joint_motion[t] = x[t+1] - x[t] for t < T-1, 0 at t = T-1          (padded zero frames are frames like any other)
 *   bone_motion[t]  = bone[t+1] - bone[t] for t < T-1, 0 at t = T-1
 * streams_fwd reads x once and writes every output whose pointer is not NULL in one launch; each value is one or two
 * correctly rounded fp32 subtractions in a fixed order: the result is bit-exact.
 * streams_bwd: dx = w_joint d_joint + w_bone bone^T(d_bone) + w_joint_motion motion^T(d_joint_motion)
 *                 + w_bone_motion bone^T(motion^T(d_bone_motion)),  a NULL cotangent contributes nothing;
 *   motion^T(d)[t] = (t > 0 ? d[t-1] : 0) - (t < T-1 ? d[t] : 0),  bone^T(d)[v] = d[v] - sum_{c : parent[c] == v} d[c].
 *   One launch, gather form, no atomics: the streams are added in the order written, the children c ascending.
 * host_parent is a HOST array of V ints, the only pointer of this header that is not a device pointer.  It is validated
 * on the host at every call and copied into the kernel's arguments by value: no index is ever read from device memory,
 * and an index outside [0, V) cannot reach a kernel.
 * AGCN_ERR_ARG: x (dx) NULL, no output (no cotangent) given, host_parent NULL, a non-positive size, a table entry outside
 *   [0, V).  AGCN_ERR_UNSUPPORTED: V > 32, or N*C*T*V*M > 2^31 - 1 (the kernels index with 32 bits).  All before any
 *   launch.  M of 2 or 4 with every pointer aligned to 4 M bytes moves one joint per lane as a vector; anything else runs
 *   element by element, with the same bits. */
int agcn_streams_fwd(const float* x, float* bone, float* joint_motion, float* bone_motion, const int* host_parent, int N,
                     int C, int T, int V, int M, void* stream);
int agcn_streams_bwd(const float* d_joint, const float* d_bone, const float* d_joint_motion, const float* d_bone_motion,
                     float* dx, const int* host_parent, float w_joint, float w_bone, float w_joint_motion,
                     float w_bone_motion, int N, int C, int T, int V, int M, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AGCN_HIP_H */
