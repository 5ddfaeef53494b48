// Parameter gradients of the base SGN in eval mode (frozen-BatchNorm fine-tuning): the gradient of a loss on the logits
// with respect to the two folded weight images of sgn.hip, each in its image's own layout (sgn_plan.h: SgnFramesW,
// SgnClipW).  torch autograd carries them through the fold to the parameters (model/sgn.py::SGN._folded).
// The operands come from the two tapes that the taping backward kernels of sgn_bwd.hip write (agcn_sgn_clip_bwd_tape,
// agcn_sgn_frames_bwd_tape; V real joint rows per frame; layout in sgn_wgrad_plan.h).  The reduction kernels
// (sgn_wgrad_device.h, shared with SGN v15): X^T . Z over row splits on exact-f32 MFMA, column sums (biases, and tem1 / spa1
// as (clips, seg * 256) / (frames, V * 64) views), the 3 x 64 first embedding layers, the folded norm_data, and the add of
// the partials in ascending split order.
// Every sum runs in a fixed order (rows ascending inside a split, splits ascending), no atomics: the same inputs give the
// same bits.  Geometry, splits, workspace and every guarded index: sgn_wgrad_plan.h.
#include "agcn_common.h"
#include "sgn_wgrad_plan.h"
#include "sgn_wgrad_device.h"

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
  // the two embeddings, spa1 and aff: the input side, shared with SGN v15
  WGRAD_TRY(wgrad_input_side(x, tape, tp.e1, tp.de2, tp.dspa, SgnWgradInputCols{tp.de1, tp.xn, tp.dxn, C}, o, d_w, part, frames,
                             seg, V, rps, st));
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
