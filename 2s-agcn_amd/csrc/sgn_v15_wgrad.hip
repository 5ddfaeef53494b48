// Parameter gradients of SGN v15 in eval mode (frozen-BatchNorm fine-tuning): the gradient of a loss on the logits with
// respect to the two folded weight images of sgn_v15.hip, each in its image's own layout (sgn_v15_plan.h: SgnFramesW up
// to spa1 + Sgn15BlockW, Sgn15ClipW).  torch autograd carries them through the fold to the parameters
// (model/sgn_v15.py::SGN._folded).  The operands come from the two tapes that the taping instantiations of sgn_v15_bwd.hip
// write (agcn_sgn15_clip_bwd_tape, agcn_sgn15_frames_bwd_tape; real token rows only; layout and where it can go wrong:
// sgn_v15_wgrad_plan.h).  The two entries here walk the sections of an image; per section they launch the base SGN's
// reduction kernels (sgn_wgrad_device.h): X^T . Z over row splits into partials on exact-f32 MFMA, then the add in
// ascending split order, and the column sums for the biases.  Fixed orders, no atomics: the same inputs give the same
// bits.  Every float of d_w is written: every section of both images receives a gradient.
#include "agcn_common.h"
#include "sgn_v15_wgrad_plan.h"
#include "sgn_wgrad_device.h"

// the eight sections of one block from the R rows of a tape with row stride C
static int sgn15_block_wgrad(const float* tape, long C, const Sgn15BlockTape& t, const Sgn15BlockW& o, int din, int dout,
                             int heads, int d_head, int ff, long R, float* d_w, float* part, int rps, hipStream_t st) {
  const int inner = heads * d_head;
  const SgnWgradRows plain = sgn_wgrad_plain_rows(R);
  WGRAD_TRY(wgrad_gemm(tape + t.x, C, tape + t.dqkv, C, din, 3 * inner, R, plain, d_w + o.qkv_w, part, rps, st));
  WGRAD_TRY(wgrad_colsum(tape + t.dqkv, C, 3 * inner, 0, 3 * inner, R, d_w + o.qkv_b, part, rps, st));
  WGRAD_TRY(wgrad_gemm(tape + t.o, C, tape + t.dx1, C, inner, din, R, plain, d_w + o.o_w, part, rps, st));
  WGRAD_TRY(wgrad_colsum(tape + t.dx1, C, din, 0, din, R, d_w + o.o_b, part, rps, st));
  WGRAD_TRY(wgrad_gemm(tape + t.x1, C, tape + t.dhid, C, din, ff, R, plain, d_w + o.f1_w, part, rps, st));
  WGRAD_TRY(wgrad_colsum(tape + t.dhid, C, ff, 0, ff, R, d_w + o.f1_b, part, rps, st));
  WGRAD_TRY(wgrad_gemm(tape + t.hid, C, tape + t.dy, C, ff + din, dout, R, plain, d_w + o.f2_w, part, rps, st));
  WGRAD_TRY(wgrad_colsum(tape + t.dy, C, dout, 0, dout, R, d_w + o.f2_b, part, rps, st));
  return AGCN_OK;
}

extern "C" size_t agcn_sgn15_frames_tape_floats(int N, int seg, int V, int heads, int d_head, int ff) {
  return sgn15_frames_domain(N, seg, V, heads, d_head, ff) ? sgn15_frames_tape_floats(N, seg, V, heads, d_head, ff) : 0;
}
extern "C" size_t agcn_sgn15_clip_tape_floats(int N, int seg, int num_class, int heads, int d_head, int ff) {
  return sgn15_clip_domain(N, seg, num_class, heads, d_head, ff) ? sgn15_clip_tape(N, seg, heads, d_head, ff).total : 0;
}
extern "C" size_t agcn_sgn15_wgrad_workspace(int N, int seg, int V, int num_class, int heads, int d_head, int ff,
                                             int rows_per_split) {
  if (rows_per_split < 0) return 0;
  if (V > 0)
    return sgn15_frames_domain(N, seg, V, heads, d_head, ff)
               ? sgn15_frames_wgrad_ws_floats(N, seg, V, heads, d_head, ff, rows_per_split) * sizeof(float) : 0;
  return sgn15_clip_domain(N, seg, num_class, heads, d_head, ff)
             ? sgn15_clip_wgrad_ws_floats(N, seg, num_class, heads, d_head, ff, rows_per_split) * sizeof(float) : 0;
}

extern "C" int agcn_sgn15_frames_wgrad(const float* x, const float* tape, size_t tape_floats, float* d_w, size_t d_w_floats,
                                       void* ws, size_t ws_bytes, int N, int seg, int V, int heads, int d_head, int ff,
                                       int rows_per_split, void* stream) {
  if (!x || !tape || !d_w || !ws || rows_per_split < 0) return AGCN_ERR_ARG;
  if (!sgn15_frames_domain(N, seg, V, heads, d_head, ff)) return AGCN_ERR_ARG;
  if (d_w_floats != (size_t)sgn15_frames_floats(V, heads, d_head, ff)) return AGCN_ERR_ARG;
  const long frames = (long)N * seg, R = frames * V;
  if (!sgn_wgrad_splits_ok(R, rows_per_split)) return AGCN_ERR_UNSUPPORTED;
  if (tape_floats < sgn15_frames_tape_floats(N, seg, V, heads, d_head, ff)) return AGCN_ERR_WORKSPACE;
  if (ws_bytes < sgn15_frames_wgrad_ws_floats(N, seg, V, heads, d_head, ff, rows_per_split) * sizeof(float))
    return AGCN_ERR_WORKSPACE;
  const SgnFramesW o = sgn_frames_w(V);          // the input sections (aff .. spa1)
  const Sgn15BlockW b = sgn15_block_w(sgn15_frames_block_base(V), SGN15_SPA_IN, SGN15_SPA_OUT, heads, d_head, ff);
  const Sgn15FramesTape tp = sgn15_frames_tape(heads, d_head, ff);
  const long C = tp.cols;
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)ws;
  AGCN_NOTE_KERNEL("sgn_wgrad_gemm_kernel<f32 mfma> v15 frames image V=%d heads=%dx%d ff=%d rows=%ld splits=%ld", V, heads,
                   d_head, ff, R, sgn_wgrad_splits(R, rows_per_split));
  WGRAD_TRY(sgn15_block_wgrad(tape, C, tp.blk, b, SGN15_SPA_IN, SGN15_SPA_OUT, heads, d_head, ff, R, d_w, part,
                              rows_per_split, st));
  return wgrad_input_side(x, tape, tp.e1, tp.de2, tp.dspa, SgnWgradInputCols{tp.de1, tp.xn, tp.dxn, C}, o, d_w, part, frames,
                          seg, V, rows_per_split, st);
}

extern "C" int agcn_sgn15_clip_wgrad(const float* tape, size_t tape_floats, const float* dlogits, float* d_w,
                                     size_t d_w_floats, void* ws, size_t ws_bytes, int N, int seg, int num_class, int heads,
                                     int d_head, int ff, int rows_per_split, void* stream) {
  if (!tape || !dlogits || !d_w || !ws || rows_per_split < 0) return AGCN_ERR_ARG;
  if (!sgn15_clip_domain(N, seg, num_class, heads, d_head, ff)) return AGCN_ERR_ARG;
  const Sgn15ClipW o = sgn15_clip_w(seg, num_class, heads, d_head, ff);
  if (d_w_floats != (size_t)o.total) return AGCN_ERR_ARG;
  const long R = (long)N * seg;
  if (!sgn_wgrad_splits_ok(R, rows_per_split)) return AGCN_ERR_UNSUPPORTED;
  const Sgn15ClipTape tp = sgn15_clip_tape(N, seg, heads, d_head, ff);
  if (tape_floats < tp.total) return AGCN_ERR_WORKSPACE;
  if (ws_bytes < sgn15_clip_wgrad_ws_floats(N, seg, num_class, heads, d_head, ff, rows_per_split) * sizeof(float))
    return AGCN_ERR_WORKSPACE;
  const long C = tp.cols;
  const int rps = rows_per_split;
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)ws;
  AGCN_NOTE_KERNEL("sgn_wgrad_gemm_kernel<f32 mfma> v15 clip image seg=%d heads=%dx%d ff=%d clips=%d splits=%ld", seg, heads,
                   d_head, ff, N, sgn_wgrad_splits(R, rps));
  // tem (seg, 256): the block's dX summed over the clips, the tape as a (clips, seg * 256) view
  WGRAD_TRY(wgrad_colsum(tape + tp.dx, (long)seg * C, SGN15_SPA_OUT, C, seg * SGN15_SPA_OUT, N, d_w + o.tem, part, rps, st));
  WGRAD_TRY(sgn15_block_wgrad(tape, C, tp.blk, o.blk, SGN15_SPA_OUT, SGN15_TEM_OUT, heads, d_head, ff, R, d_w, part, rps, st));
  WGRAD_TRY(wgrad_gemm(tape + tp.ymax, SGN15_TEM_OUT, dlogits, num_class, SGN15_TEM_OUT, num_class, N,
                       sgn_wgrad_plain_rows(N), d_w + o.fc_w, part, rps, st));
  WGRAD_TRY(wgrad_colsum(dlogits, num_class, num_class, 0, num_class, N, d_w + o.fc_b, part, rps, st));
  return AGCN_OK;
}
