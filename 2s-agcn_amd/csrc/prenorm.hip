// Skeleton preprocessing next to the data, for online recognition and for dataset generation:
//
//   * agcn_skel_append: one frame (Mmax, V, 3) into a device ring (Mmax, Tmax, V, 3), with the reference's recursive
//     moving average (infer/data_preprocess.py DataPreprocessor.append_data) on the slot just written.  The reference
//     shifts its whole window by one frame per append; here the host keeps (slot, count) and nothing moves.
//   * agcn_prenorm: body selection (data_preprocess.py select_skeletons / ntu_gendata.py get_nonzero_std) and
//     data_gen/preprocess.py pre_normalization (pad null frames, centre on the first body's joint 1, rotate one bone
//     onto z and one onto x) of N samples, one workgroup per sample, written in the model's (N, 3, T, V, K) layout.
//
//   * agcn_prenorm_windows: the same kernel, second instantiation, with per-sample addressing read on the device: sample
//     n is the window (block[n], start[n], len[n]) of a pool of (M, Tmax, V, 3) blocks.  The windows may be any
//     positions of one long recording or the current windows of many rings.
//   * agcn_skel_smooth: a whole recording (L, Mmax, V, 3) -> (Mmax, L, V, 3) with the moving average of agcn_skel_append
//     run over all its frames, and agcn_skel_append_many: one frame into each of S rings in one launch.
//
// Logical frame t of a sample lives in slot (origin + t) mod Tmax of its (M, Tmax, V, 3) block: a ring passes its oldest
// slot, a plain (N, M, T, V, 3) tensor passes origin 0 and Tmax = T.  A window has len <= T frames; frames t >= len are
// null: they read as zeros and no memory is touched (in a recording the slots behind a window hold future frames).
// Every read of a frame goes through one helper (Frames::load3) that knows this.
//
// Null tests: a frame (joint) is null iff ALL its 3V (3) values are zero; the reference tests sum() == 0, which differs
// only where a non-null frame or joint sums to exactly zero by cancellation.
//
// No float atomics: the frame flags are integer ORs into LDS, every sum runs in a fixed order (per-lane strided partials
// in fp64, a butterfly inside the wave, the waves in index order).  Every gathered index (selected body, source frame,
// axis joint, ring slot) is clamped before use, so a wrong plan gives a wrong number and never an out-of-range read.
#include "agcn_common.h"

#define PRENORM_MAX_T 2048        // frames per sample the LDS plan holds (src table: MAX_K * MAX_T * 2 bytes = 32 KB)
#define PRENORM_MAX_M 8           // bodies per sample / selected bodies
#define PRENORM_THREADS 1024
#define PRENORM_WAVES (PRENORM_THREADS / 64)
#define PRENORM_FLAG_WORDS (PRENORM_MAX_T / 32)
#define SMOOTH_THREADS 64
#define SMOOTH_CHIP 32            // earlier outputs agcn_skel_smooth keeps in LDS per value (k - 1 <= 32)
#define SMOOTH_AHEAD 8            // raw frames loaded ahead of the serial recursion

namespace {

// one value e of one ring: the arithmetic of agcn_skel_append, shared by the one-ring and the many-ring kernel
__device__ __forceinline__ void append_value(const float* __restrict__ frame, float* __restrict__ ring, int e, int Mmax,
                                             int Tmax, int V, int slot, int count, int k) {
  const int row = V * 3;
  if (e >= Mmax * row) return;
  const int m = e / row, j = e - m * row;
  float* body = ring + (long)m * Tmax * row;
  float val = frame[e];
  if (k > 1 && count >= k) {
    // mean of the last k slots, oldest first, the new frame last (numpy: fp32 sum along the axis, then / k)
    float s = 0.f;
    for (int i = k - 1; i >= 1; --i) {
      int sl = slot - i;
      if (sl < 0) sl += Tmax;
      sl = min(max(sl, 0), Tmax - 1);
      s += body[(long)sl * row + j];
    }
    s += val;
    val = s / (float)k;
  }
  body[(long)slot * row + j] = val;
}

__global__ void __launch_bounds__(256) skel_append_kernel(const float* __restrict__ frame, float* __restrict__ ring,
                                                          int Mmax, int Tmax, int V, int slot, int count, int k) {
  append_value(frame, ring, blockIdx.x * 256 + threadIdx.x, Mmax, Tmax, V, slot, count, k);
}

// stream blockIdx.y: its frame into its ring at slot[s] (< 0: no frame this tick), with count[s] frames present
__global__ void __launch_bounds__(256) skel_append_many_kernel(const float* __restrict__ frames, float* __restrict__ rings,
                                                               const int* __restrict__ slot, const int* __restrict__ count,
                                                               int Mmax, int Tmax, int V, int k) {
  const int s = blockIdx.y;
  const int sl = slot[s];
  if (sl < 0) return;
  const long per = (long)Mmax * V * 3;
  append_value(frames + s * per, rings + s * per * Tmax, blockIdx.x * 256 + threadIdx.x, Mmax, Tmax, V,
               min(sl, Tmax - 1), min(max(count[s], 1), Tmax), k);
}

// k = 1: raw (L, E) -> out (Mmax, L, row), E = Mmax * row
__global__ void __launch_bounds__(256) skel_transpose_kernel(const float* __restrict__ raw, float* __restrict__ out,
                                                             int Mmax, int L, int row) {
  const long total = (long)L * Mmax * row;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int E = Mmax * row;
  const int t = (int)(i / E), e = (int)(i - (long)t * E);
  const int m = e / row, j = e - m * row;
  out[((long)m * L + t) * row + j] = raw[i];
}

// k > 1: one thread per value, serial in t.  The k - 1 earlier outputs of the value are a circular history: in LDS
// (CHIP) or, for k - 1 > SMOOTH_CHIP, the thread's own earlier stores to `out`, read back.  Summed oldest first, the raw
// frame last, from 0.f, then / k: the expression of append_value.
template <bool CHIP>
__global__ void __launch_bounds__(SMOOTH_THREADS) skel_smooth_kernel(const float* __restrict__ raw, float* out, int Mmax,
                                                                     int L, int row, int k) {
  __shared__ float hist[CHIP ? SMOOTH_CHIP : 1][SMOOTH_THREADS];
  const int E = Mmax * row, lane = threadIdx.x;
  const int e = blockIdx.x * SMOOTH_THREADS + lane;
  if (e >= E) return;                            // no barrier below: a thread reads only what it wrote itself
  const int m = e / row, j = e - m * row;
  float* mine = out + (long)m * L * row + j;     // mine[t * row]
  const int H = k - 1;
  int pos = 0;                                   // t mod H: the oldest entry of the history, overwritten by frame t
  for (int t0 = 0; t0 < L; t0 += SMOOTH_AHEAD) {
    float r[SMOOTH_AHEAD];
#pragma unroll
    for (int i = 0; i < SMOOTH_AHEAD; ++i) r[i] = t0 + i < L ? raw[(long)(t0 + i) * E + e] : 0.f;
#pragma unroll
    for (int i = 0; i < SMOOTH_AHEAD; ++i) {
      const int t = t0 + i;
      if (t >= L) break;
      float val = r[i];
      if (t >= H) {
        float s = 0.f;
        if (CHIP) {
          int p = pos;
          for (int q = 0; q < H; ++q) {
            s += hist[p][lane];
            if (++p == H) p = 0;
          }
        } else {
          for (int q = t - H; q < t; ++q) s += mine[(long)q * row];
        }
        s += val;
        val = s / (float)k;
      }
      mine[(long)t * row] = val;
      if (CHIP) {
        hist[pos][lane] = val;
        if (++pos == H) pos = 0;
      }
    }
  }
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k);
  return v;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

struct PrenormArgs {
  const float* in;
  float* out;
  int* sel;
  float* energy;
  int M, K, T, Tmax, origin, V, select, pad, center;
  int z0, z1, x0, x1, zz0, zz1;
  const int* block;                 // windows only: (N) block of the pool, or NULL = block 0; (N) first slot; (N) frames
  const int* start;
  const int* len;
  int nblocks;
};

// The frames of one sample.  WINDOWS = false: block n of the input, origin and T from the host (agcn_prenorm).
// WINDOWS = true: block, first slot and length from the device arrays, clamped into the pool; frames t >= len are null.
template <bool WINDOWS>
struct Frames {
  const float* in;                  // the sample's (M, Tmax, V, 3) block
  long body_stride;
  int Tmax, row, origin, len;

  __device__ Frames(const PrenormArgs& a, int n) : body_stride((long)a.Tmax * a.V * 3), Tmax(a.Tmax), row(a.V * 3) {
    int blk = n;
    origin = a.origin;
    len = a.T;
    if (WINDOWS) {
      blk = a.block ? clampi(a.block[n], 0, a.nblocks - 1) : 0;
      origin = clampi(a.start[n], 0, a.Tmax - 1);
      len = clampi(a.len[n], 0, a.T);
    }
    in = a.in + (long)blk * a.M * body_stride;
  }
  __device__ __forceinline__ int slot_of(int t) const {      // ring slot of logical frame t, clamped into the block
    int s = origin + t;
    if (s >= Tmax) s -= Tmax;
    return clampi(s, 0, Tmax - 1);
  }
  // joint j of logical frame t of body m: THE read of a frame (flags, energy, centre / rotation, gather)
  __device__ __forceinline__ void load3(int m, int t, int j, float& x0, float& x1, float& x2) const {
    if (WINDOWS && t >= len) {
      x0 = x1 = x2 = 0.f;
      return;
    }
    const float* q = in + m * body_stride + (long)slot_of(t) * row + j * 3;
    x0 = q[0]; x1 = q[1]; x2 = q[2];
  }
};

// reference data_gen/rotation.py angle_between + rotation_matrix for the rotation that takes v onto the unit axis e
// (e = z: ez = 1, e = x: ez = 0), in fp64: R (row major)
__device__ void rotation_onto(const double v[3], int ez, double R[9]) {
  for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  // axis = cross(v, e)
  double ax[3];
  if (ez) { ax[0] = v[1]; ax[1] = -v[0]; ax[2] = 0.0; }
  else { ax[0] = 0.0; ax[1] = v[2]; ax[2] = -v[1]; }
  double theta = 0.0;
  if (fabs(v[0]) + fabs(v[1]) + fabs(v[2]) >= 1e-6) {
    const double nv = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    double d = (ez ? v[2] : v[0]) / nv;
    d = fmin(1.0, fmax(-1.0, d));
    theta = acos(d);
  }
  if (fabs(ax[0]) + fabs(ax[1]) + fabs(ax[2]) < 1e-6 || fabs(theta) < 1e-6) return;
  const double na = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
  const double a = cos(theta / 2.0), sn = sin(theta / 2.0);
  const double b = -(ax[0] / na) * sn, c = -(ax[1] / na) * sn, d = -(ax[2] / na) * sn;
  const double aa = a * a, bb = b * b, cc = c * c, dd = d * d;
  const double bc = b * c, ad = a * d, ac = a * c, ab = a * b, bd = b * d, cd = c * d;
  R[0] = aa + bb - cc - dd; R[1] = 2 * (bc + ad);     R[2] = 2 * (bd - ac);
  R[3] = 2 * (bc - ad);     R[4] = aa + cc - bb - dd; R[5] = 2 * (cd + ab);
  R[6] = 2 * (bd + ac);     R[7] = 2 * (cd - ab);     R[8] = aa + dd - bb - cc;
}

__device__ void matmul3(const double A[9], const double B[9], double C[9]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}

template <bool WINDOWS>
__global__ void __launch_bounds__(PRENORM_THREADS) prenorm_kernel(PrenormArgs a) {
  __shared__ unsigned flags[PRENORM_MAX_M][PRENORM_FLAG_WORDS];     // bit t of body m: frame t has a non-zero value
  __shared__ unsigned short src[PRENORM_MAX_M][PRENORM_MAX_T];      // source frame of output frame t, per selected body
  __shared__ double red[PRENORM_WAVES][PRENORM_MAX_M][3];
  __shared__ double mean[PRENORM_MAX_M][3];
  __shared__ float energy_s[PRENORM_MAX_M];
  __shared__ int sel_s[PRENORM_MAX_M];
  __shared__ int first_s;                                           // first non-null frame of the first body, or -1
  __shared__ float rot_s[9];

  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = a.M, K = a.K, T = a.T, V = a.V;
  const Frames<WINDOWS> fr(a, n);
  const int TV = T * V;
  auto valid = [&](int m, int t) { return (flags[m][t >> 5] >> (t & 31)) & 1u; };

  for (int i = tid; i < PRENORM_MAX_M * PRENORM_FLAG_WORDS; i += PRENORM_THREADS) (&flags[0][0])[i] = 0u;
  __syncthreads();

  // ---- frame flags of every body ------------------------------------------------------------------------------------
  for (int m = 0; m < M; ++m) {
    for (int p = tid; p < TV; p += PRENORM_THREADS) {
      const int t = p / V, v = p - t * V;
      float q0, q1, q2;
      fr.load3(m, t, v, q0, q1, q2);
      if (q0 != 0.f || q1 != 0.f || q2 != 0.f) atomicOr(&flags[m][t >> 5], 1u << (t & 31));
    }
  }
  __syncthreads();

  // ---- body selection: energy = sum over channels of the population std over (valid frames x joints) -----------------
  if (a.select) {
    for (int pass = 0; pass < 2; ++pass) {
      for (int m = 0; m < M; ++m) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        const double m0 = pass ? mean[m][0] : 0.0, m1 = pass ? mean[m][1] : 0.0, m2 = pass ? mean[m][2] : 0.0;
        for (int p = tid; p < TV; p += PRENORM_THREADS) {
          const int t = p / V, v = p - t * V;
          if (!valid(m, t)) continue;
          float q0, q1, q2;
          fr.load3(m, t, v, q0, q1, q2);
          const double d0 = (double)q0 - m0, d1 = (double)q1 - m1, d2 = (double)q2 - m2;
          if (pass) { s0 += d0 * d0; s1 += d1 * d1; s2 += d2 * d2; }
          else { s0 += d0; s1 += d1; s2 += d2; }
        }
        s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
        if (lane == 0) { red[wave][m][0] = s0; red[wave][m][1] = s1; red[wave][m][2] = s2; }
      }
      __syncthreads();
      if (tid < M) {
        int nvalid = 0;
        for (int w = 0; w < (T + 31) / 32; ++w) nvalid += __popc(flags[tid][w]);
        const double cnt = (double)nvalid * V;
        double e = 0.0;
        for (int c = 0; c < 3; ++c) {
          double s = 0.0;
          for (int w = 0; w < PRENORM_WAVES; ++w) s += red[w][tid][c];
          if (pass) e += nvalid ? sqrt(s / cnt) : 0.0;
          else mean[tid][c] = nvalid ? s / cnt : 0.0;
        }
        if (pass) energy_s[tid] = (float)e;
      }
      __syncthreads();
    }
    if (tid == 0) {
      // the K largest, largest first; among equal energies the higher index first (argsort()[::-1])
      unsigned taken = 0u;
      for (int k = 0; k < K; ++k) {
        int best = -1;
        for (int m = 0; m < M; ++m)
          if (!((taken >> m) & 1u) && (best < 0 || energy_s[m] >= energy_s[best])) best = m;
        best = clampi(best, 0, M - 1);
        taken |= 1u << best;
        sel_s[k] = best;
      }
    }
    if (tid < M && a.energy) a.energy[(long)n * M + tid] = energy_s[tid];
  } else if (tid < K) {
    sel_s[tid] = clampi(tid, 0, M - 1);
  }
  __syncthreads();
  if (tid < K) a.sel[(long)n * K + tid] = sel_s[tid];

  // ---- padding plan: one wave per selected body ----------------------------------------------------------------------
  const int nchunk = (T + 63) / 64;
  const int k = wave;                            // K <= PRENORM_MAX_M < PRENORM_WAVES
  int L = T;
  bool loops = false;
  if (k < K) {
    const int m = clampi(sel_s[k], 0, M - 1);
    int nvalid = 0, last = -1;
    for (int ch = 0; ch < nchunk; ++ch) {
      const int t = ch * 64 + lane;
      const unsigned long long b = __ballot(t < T && valid(m, t));
      nvalid += __popcll(b);
      if (b) last = ch * 64 + 63 - __clzll(b);
    }
    const bool compact = a.pad && nvalid > 0 && !valid(m, 0);
    int base = 0;
    for (int ch = 0; ch < nchunk; ++ch) {
      const int t = ch * 64 + lane;
      const bool ok = t < T && valid(m, t);
      const unsigned long long b = __ballot(ok);
      if (compact) {
        if (ok) src[k][clampi(base + __popcll(b & ((1ull << lane) - 1ull)), 0, T - 1)] = (unsigned short)t;
        base += __popcll(b);
      } else if (t < T) {
        src[k][t] = (unsigned short)t;
      }
    }
    if (k == 0 && lane == 0) {
      // first frame of the first body with any non-zero value, after its padding (center_firstframe)
      int f = -1;
      if (nvalid > 0) {
        if (compact) f = 0;
        else for (int t = 0; t < T && f < 0; ++t) if (valid(m, t)) f = t;
      }
      first_s = f;
    }
    L = compact ? nvalid : last + 1;
    loops = a.pad && nvalid > 0 && L < T;
  }
  __syncthreads();
  // frames past the valid run loop over it: they read entries below L only, which the pass above has finished
  if (loops)
    for (int t = L + lane; t < T; t += 64) src[k][t] = src[k][clampi((t - L) % L, 0, T - 1)];
  __syncthreads();

  // ---- centre of frame 0 and the rotations, one lane, fp64 -----------------------------------------------------------
  const int b0 = clampi(sel_s[0], 0, M - 1);
  // joint 1 of the first body's first non-null frame (center == 2)
  auto first_centre = [&](float o[3]) {
    fr.load3(b0, clampi((int)src[0][clampi(first_s, 0, T - 1)], 0, T - 1), 1, o[0], o[1], o[2]);
  };
  if (tid == 0) {
    const int f0 = clampi((int)src[0][0], 0, T - 1);
    float c0[3] = {0.f, 0.f, 0.f};
    if (a.center == 1) fr.load3(b0, f0, 1, c0[0], c0[1], c0[2]);
    else if (a.center == 2 && first_s >= 0) first_centre(c0);
    // centred, masked joints of the first body's frame 0, as the reference holds them (fp32) when it builds a matrix
    auto joint = [&](int j, float o[3]) {
      float q[3];
      fr.load3(b0, f0, clampi(j, 0, V - 1), q[0], q[1], q[2]);
      const bool nz = q[0] != 0.f || q[1] != 0.f || q[2] != 0.f;
      for (int c = 0; c < 3; ++c) o[c] = nz ? q[c] - c0[c] : 0.f;
    };
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const int ax[3][3] = {{a.z0, a.z1, 1}, {a.x1, a.x0, 0}, {a.zz0, a.zz1, 1}};     // {from, to, onto z?}
    for (int s = 0; s < 3; ++s) {
      if (ax[s][0] < 0 || ax[s][1] < 0) continue;
      float p0[3], p1[3], r0[3], r1[3];
      joint(ax[s][0], p0);
      joint(ax[s][1], p1);
      for (int i = 0; i < 3; ++i) {              // the rotations so far, applied in fp64 and stored as fp32
        r0[i] = (float)(R[i * 3] * p0[0] + R[i * 3 + 1] * p0[1] + R[i * 3 + 2] * p0[2]);
        r1[i] = (float)(R[i * 3] * p1[0] + R[i * 3 + 1] * p1[1] + R[i * 3 + 2] * p1[2]);
      }
      const double v[3] = {(double)(r1[0] - r0[0]), (double)(r1[1] - r0[1]), (double)(r1[2] - r0[2])};
      double Rs[9], Rn[9];
      rotation_onto(v, ax[s][2], Rs);
      matmul3(Rs, R, Rn);
      for (int i = 0; i < 9; ++i) R[i] = Rn[i];
    }
    for (int i = 0; i < 9; ++i) rot_s[i] = (float)R[i];
  }
  __syncthreads();

  // ---- gather, centre, mask, rotate, write (N, 3, T, V, K): lane <-> (t, v), all K bodies of the joint ---------------
  float R[9];
  for (int i = 0; i < 9; ++i) R[i] = rot_s[i];
  float cf[3] = {0.f, 0.f, 0.f};
  if (a.center == 2 && first_s >= 0) first_centre(cf);
  float* out = a.out + (long)n * 3 * TV * K;
  for (int p = tid; p < TV; p += PRENORM_THREADS) {
    const int t = p / V, v = p - t * V;
    float ctr[3] = {cf[0], cf[1], cf[2]};
    if (a.center == 1) fr.load3(b0, clampi((int)src[0][t], 0, T - 1), 1, ctr[0], ctr[1], ctr[2]);
    for (int k = 0; k < K; ++k) {
      const int m = clampi(sel_s[k], 0, M - 1);
      float x0, x1, x2;
      fr.load3(m, clampi((int)src[k][t], 0, T - 1), v, x0, x1, x2);
      const bool nz = x0 != 0.f || x1 != 0.f || x2 != 0.f;
      const float d0 = nz ? x0 - ctr[0] : 0.f, d1 = nz ? x1 - ctr[1] : 0.f, d2 = nz ? x2 - ctr[2] : 0.f;
      for (int c = 0; c < 3; ++c)
        out[((long)c * T + t) * V * K + v * K + k] = R[c * 3] * d0 + R[c * 3 + 1] * d1 + R[c * 3 + 2] * d2;
    }
  }
}

bool axis_ok(int j0, int j1, int V) { return (j0 == -1 && j1 == -1) || (j0 >= 0 && j0 < V && j1 >= 0 && j1 < V); }

}  // namespace

extern "C" int agcn_prenorm_max_frames() { return PRENORM_MAX_T; }

extern "C" int agcn_skel_append(const float* frame, float* ring, int Mmax, int Tmax, int V, int slot, int count, int k,
                                void* stream) {
  if (!frame || !ring) return AGCN_ERR_ARG;
  if (Mmax < 1 || Tmax < 1 || V < 1 || V > 32 || k < 1 || k > Tmax) return AGCN_ERR_ARG;
  if (slot < 0 || slot >= Tmax || count < 1 || count > Tmax) return AGCN_ERR_ARG;
  if (count < Tmax && slot != count - 1) return AGCN_ERR_ARG;      // while filling, frames go in from slot 0 upward
  const int total = Mmax * V * 3;
  skel_append_kernel<<<(total + 255) / 256, 256, 0, (hipStream_t)stream>>>(frame, ring, Mmax, Tmax, V, slot, count, k);
  return agcn_check_launch();
}

extern "C" int agcn_prenorm(const float* in, float* out, int* sel, float* energy, int N, int M, int K, int T, int Tmax,
                            int origin, int V, int select, int pad, int center, int z0, int z1, int x0, int x1, int zz0,
                            int zz1, void* stream) {
  if (!in || !out || !sel || (select && !energy)) return AGCN_ERR_ARG;
  if (N < 1 || M < 1 || M > PRENORM_MAX_M || K < 1 || K > M) return AGCN_ERR_ARG;
  if (V < 2 || V > 32 || T < 1 || T > PRENORM_MAX_T || Tmax < T || origin < 0 || origin >= Tmax) return AGCN_ERR_ARG;
  if (center < 0 || center > 2) return AGCN_ERR_ARG;
  if (!axis_ok(z0, z1, V) || !axis_ok(x0, x1, V) || !axis_ok(zz0, zz1, V)) return AGCN_ERR_ARG;
  PrenormArgs a;
  a.in = in; a.out = out; a.sel = sel; a.energy = energy;
  a.M = M; a.K = K; a.T = T; a.Tmax = Tmax; a.origin = origin; a.V = V;
  a.select = select ? 1 : 0; a.pad = pad ? 1 : 0; a.center = center;
  a.z0 = z0; a.z1 = z1; a.x0 = x0; a.x1 = x1; a.zz0 = zz0; a.zz1 = zz1;
  a.block = a.start = a.len = nullptr;
  a.nblocks = N;
  prenorm_kernel<false><<<N, PRENORM_THREADS, 0, (hipStream_t)stream>>>(a);
  return agcn_check_launch();
}

extern "C" int agcn_prenorm_windows(const float* in, float* out, int* sel, float* energy, const int* block,
                                    const int* start, const int* len, int N, int nblocks, int M, int K, int T, int Tmax,
                                    int V, int select, int pad, int center, int z0, int z1, int x0, int x1, int zz0,
                                    int zz1, void* stream) {
  if (!in || !out || !sel || (select && !energy) || !start || !len) return AGCN_ERR_ARG;
  if (N < 1 || nblocks < 1 || M < 1 || M > PRENORM_MAX_M || K < 1 || K > M) return AGCN_ERR_ARG;
  if (V < 2 || V > 32 || T < 1 || T > PRENORM_MAX_T || Tmax < T) return AGCN_ERR_ARG;
  if (center < 0 || center > 2) return AGCN_ERR_ARG;
  if (!axis_ok(z0, z1, V) || !axis_ok(x0, x1, V) || !axis_ok(zz0, zz1, V)) return AGCN_ERR_ARG;
  PrenormArgs a;
  a.in = in; a.out = out; a.sel = sel; a.energy = energy;
  a.M = M; a.K = K; a.T = T; a.Tmax = Tmax; a.origin = 0; a.V = V;
  a.select = select ? 1 : 0; a.pad = pad ? 1 : 0; a.center = center;
  a.z0 = z0; a.z1 = z1; a.x0 = x0; a.x1 = x1; a.zz0 = zz0; a.zz1 = zz1;
  a.block = block; a.start = start; a.len = len; a.nblocks = nblocks;
  prenorm_kernel<true><<<N, PRENORM_THREADS, 0, (hipStream_t)stream>>>(a);
  return agcn_check_launch();
}

extern "C" int agcn_skel_smooth(const float* raw, float* out, int Mmax, int L, int V, int k, void* stream) {
  if (!raw || !out) return AGCN_ERR_ARG;
  if (Mmax < 1 || L < 1 || V < 1 || V > 32 || k < 1 || k > L) return AGCN_ERR_ARG;
  const int row = V * 3, E = Mmax * row;
  if (k == 1) {
    const long total = (long)L * E;
    if ((total + 255) / 256 > 0x7fffffffL) return AGCN_ERR_ARG;
    skel_transpose_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(raw, out, Mmax, L, row);
  } else if (k - 1 <= SMOOTH_CHIP) {
    skel_smooth_kernel<true><<<(E + SMOOTH_THREADS - 1) / SMOOTH_THREADS, SMOOTH_THREADS, 0, (hipStream_t)stream>>>(
        raw, out, Mmax, L, row, k);
  } else {
    skel_smooth_kernel<false><<<(E + SMOOTH_THREADS - 1) / SMOOTH_THREADS, SMOOTH_THREADS, 0, (hipStream_t)stream>>>(
        raw, out, Mmax, L, row, k);
  }
  return agcn_check_launch();
}

extern "C" int agcn_skel_append_many(const float* frames, float* rings, const int* slot, const int* count, int S,
                                     int Mmax, int Tmax, int V, int k, void* stream) {
  if (!frames || !rings || !slot || !count) return AGCN_ERR_ARG;
  if (S < 1 || S > 65535 || Mmax < 1 || Tmax < 1 || V < 1 || V > 32 || k < 1 || k > Tmax) return AGCN_ERR_ARG;
  const int total = Mmax * V * 3;
  skel_append_many_kernel<<<dim3((total + 255) / 256, S), 256, 0, (hipStream_t)stream>>>(frames, rings, slot, count, Mmax,
                                                                                       Tmax, V, k);
  return agcn_check_launch();
}
