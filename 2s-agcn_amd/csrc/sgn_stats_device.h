// The merge of the batch-statistics partials, shared by sgn_stats.hip (base SGN) and sgn_v15_stats.hip (SGN v15):
// every pass emits per group and channel (sum, M2 about the group's own mean) in the layout of sgn_stats_plan.h, and the
// two kernels here merge them with the state (count, mean, M2) in fp64 -- the groups of a clip in ascending index, then
// the clips in ascending index on top of the carry state.  What differs between the models is how many groups a clip has
// and how many samples a group stands for: the Rule, a small struct passed by value
//   int per;                       groups per clip
//   int count(long g) const;       samples of group g (a group with count 0 is skipped)
// Static / template, one copy per source that includes it (like sgn_wgrad_device.h).
#pragma once
#include "agcn_common.h"
#include "sgn_stats_plan.h"

// (n, mean, M2) <- (n, mean, M2) merged with (nb, meanb, m2b), nb >= 1: the pairwise update of Chan, Golub and LeVeque.
// From the zero state it returns the second operand itself (nb / tot = 1 and n * nb / tot = 0 exactly).
__device__ __forceinline__ void chan_merge(double& n, double& mean, double& m2, double nb, double meanb, double m2b) {
  const double tot = n + nb;
  const double delta = meanb - mean;
  mean = mean + delta * (nb / tot);
  m2 = m2 + m2b + delta * delta * (n * nb / tot);
  n = tot;
}

// First level, one thread per (clip, channel): the groups of the clip merged one after the other in ascending index,
// state in fp64, to the clip's (count, mean, M2) in the workspace.  A group with count 0 is skipped.
template <class Rule>
__global__ __launch_bounds__(SGN_STATS_THREADS) void sgn_stats_clip_merge_kernel(const float* __restrict__ part,
                                                                                 double* __restrict__ ws, int C, Rule rule) {
  const int c = blockIdx.y * SGN_STATS_THREADS + threadIdx.x;
  const long clip = blockIdx.x;
  if (c >= C) return;
  const int per = rule.per;
  double n = 0., mean = 0., m2 = 0.;
  for (int i = 0; i < per; ++i) {
    const long g = clip * per + i;
    const int cnt = rule.count(g);
    if (cnt < 1) continue;
    const double nb = (double)cnt;
    chan_merge(n, mean, m2, nb, (double)part[sgn_stats_part_index(g, 0, c, C)] / nb,
               (double)part[sgn_stats_part_index(g, 1, c, C)]);
  }
  ws[sgn_stats_clip_state_index(clip, 0, c, C)] = n;
  ws[sgn_stats_clip_state_index(clip, 1, c, C)] = mean;
  ws[sgn_stats_clip_state_index(clip, 2, c, C)] = m2;
}

// Second level, one thread per channel: the clips' states merged one after the other in ascending clip index on top of
// the carry-in state ("no carry-in" and "a carry-in of zeros" are the same bits).
static __global__ __launch_bounds__(SGN_STATS_THREADS) void sgn_stats_finalize_kernel(const double* __restrict__ ws,
                                                                                      const double* __restrict__ carry_in,
                                                                                      double* __restrict__ carry_out,
                                                                                      float* __restrict__ mean_out,
                                                                                      float* __restrict__ var_out, long N,
                                                                                      int C) {
  const int c = blockIdx.x * SGN_STATS_THREADS + threadIdx.x;
  if (c >= C) return;
  double n = 0., mean = 0., m2 = 0.;
  if (carry_in) {
    n = carry_in[c];
    mean = carry_in[C + c];
    m2 = carry_in[2 * C + c];
  }
#pragma unroll 4
  for (long clip = 0; clip < N; ++clip) {
    const double nb = ws[sgn_stats_clip_state_index(clip, 0, c, C)];
    const double mb = ws[sgn_stats_clip_state_index(clip, 1, c, C)];
    const double qb = ws[sgn_stats_clip_state_index(clip, 2, c, C)];
    if (nb >= 1.) chan_merge(n, mean, m2, nb, mb, qb);
  }
  if (carry_out) {
    carry_out[c] = n;
    carry_out[C + c] = mean;
    carry_out[2 * C + c] = m2;
  }
  if (mean_out) mean_out[c] = (float)mean;
  if (var_out) var_out[c] = n > 0. ? (float)(m2 / n) : 0.f;
}

// the two launches of a finalize on N clips of C channels; the callers have checked every size
template <class Rule>
static int sgn_stats_merge(const float* part, double* ws, Rule rule, int C, long N, const double* carry_in,
                           double* carry_out, float* mean, float* var, hipStream_t stream) {
  const unsigned blocks = (unsigned)((C + SGN_STATS_THREADS - 1) / SGN_STATS_THREADS);
  hipLaunchKernelGGL(sgn_stats_clip_merge_kernel<Rule>, dim3((unsigned)N, blocks), dim3(SGN_STATS_THREADS), 0, stream, part,
                     ws, C, rule);
  hipLaunchKernelGGL(sgn_stats_finalize_kernel, dim3(blocks), dim3(SGN_STATS_THREADS), 0, stream, (const double*)ws,
                     carry_in, carry_out, mean, var, N, C);
  return agcn_check_launch();
}
