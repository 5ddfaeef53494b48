// Geometry and index arithmetic of the SGN inference kernels (sgn.hip): the layout of the folded weight images, the LDS
// carve of the joint-level kernel, the row tiles of the frame-level kernel and the interval plan of the sampler.
// Plain C++17 without HIP: sgn.hip includes it for the launchers AND the kernels (SGN_HD), and tests/sgn_plan_check.cpp
// compiles it with the host compiler.
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define SGN_HD __host__ __device__ __forceinline__
#else
#define SGN_HD static inline
#endif

#define SGN_THREADS 256
#define SGN_WAVES 4
#define SGN_VP 32              // joint rows of a frame padded to the height of v_mfma_f32_32x32x2_f32
#define SGN_MAX_V 32
#define SGN_C1 64              // widths fixed by the class (reference sgn.py:23-25)
#define SGN_C2 128
#define SGN_C3 256
#define SGN_C4 512             // local.cnn2 output = fc input
#define SGN_MAX_CLASS 4096
#define SGN_LDS_LIMIT (160 * 1024)

SGN_HD bool sgn_frames_domain(long N, int seg, int V) {
  return N >= 1 && seg >= 1 && V >= 2 && V <= SGN_MAX_V && N * (long)seg <= 0x7fffffffL / (SGN_MAX_V * SGN_MAX_V);
}
SGN_HD bool sgn_clip_domain(long N, int seg, int num_class) {
  return N >= 1 && N <= 0x7fffffffL / SGN_MAX_CLASS && seg >= 1 && seg <= (1 << 20) && num_class >= 1 &&
         num_class <= SGN_MAX_CLASS;
}

// ---- folded weight image of agcn_sgn_frames (floats).  Every matrix is stored (K, N) row-major: row k = the input
// channel, so the 32 lanes of an MFMA B operand read 32 consecutive floats. ----
struct SgnFramesW {
  int aff;                     // (4, V, 3): joint scale, joint shift, dif scale, dif shift of the two norm_data, [v*3 + c]
  int je1_w, je1_b, je2_w, je2_b;      // joint_embed: (3, 64), (64), (64, 64), (64)
  int de1_w, de1_b, de2_w, de2_b;      // dif_embed
  int spa1;                    // (V, 64): spa_embed of the one-hot joints, input independent
  int g_w, g_b;                // compute_g1: [g1 | g2] side by side, (128, 512), (512)
  int c1_w, c1_b;              // gcn1 with its BatchNorm folded: ([W ; W1] (256, 128)), (128)
  int c2_w, c2_b;              // gcn2: (256, 256), (256)
  int c3_w, c3_b;              // gcn3: (512, 256), (256)
  int total;
};
SGN_HD SgnFramesW sgn_frames_w(int V) {
  SgnFramesW w;
  int o = 0;
  w.aff = o;   o += 4 * V * 3;
  w.je1_w = o; o += 3 * SGN_C1;
  w.je1_b = o; o += SGN_C1;
  w.je2_w = o; o += SGN_C1 * SGN_C1;
  w.je2_b = o; o += SGN_C1;
  w.de1_w = o; o += 3 * SGN_C1;
  w.de1_b = o; o += SGN_C1;
  w.de2_w = o; o += SGN_C1 * SGN_C1;
  w.de2_b = o; o += SGN_C1;
  w.spa1 = o;  o += V * SGN_C1;
  w.g_w = o;   o += SGN_C2 * 2 * SGN_C3;
  w.g_b = o;   o += 2 * SGN_C3;
  w.c1_w = o;  o += 2 * SGN_C2 * SGN_C2;
  w.c1_b = o;  o += SGN_C2;
  w.c2_w = o;  o += 2 * SGN_C2 * SGN_C3;
  w.c2_b = o;  o += SGN_C3;
  w.c3_w = o;  o += 2 * SGN_C3 * SGN_C3;
  w.c3_b = o;  o += SGN_C3;
  w.total = o;
  return w;
}

// ---- LDS of agcn_sgn_frames (floats): two activation buffers of SGN_VP rows x SGN_BUF_STRIDE, the four K-split
// partials of g3, the adjacency, and the normalised input.  Row strides are odd: the 32 lanes of an MFMA A operand
// (one row each, same column) fall into 32 different banks of ds_read_b32. ----
#define SGN_BUF_STRIDE (2 * SGN_C3 + 1)        // 513: [g.x | x] of gcn3
#define SGN_G_STRIDE (SGN_VP + 1)              // 33
#define SGN_LDS_BUF_A 0
#define SGN_LDS_BUF_B (SGN_LDS_BUF_A + SGN_VP * SGN_BUF_STRIDE)
#define SGN_LDS_PART (SGN_LDS_BUF_B + SGN_VP * SGN_BUF_STRIDE)          // (SGN_WAVES, SGN_VP, SGN_G_STRIDE)
#define SGN_LDS_G (SGN_LDS_PART + SGN_WAVES * SGN_VP * SGN_G_STRIDE)    // (SGN_VP, SGN_G_STRIDE)
#define SGN_LDS_XIN (SGN_LDS_G + SGN_VP * SGN_G_STRIDE)                 // (2, SGN_VP, 4): joint, dif after norm_data
#define SGN_FRAMES_LDS_FLOATS (SGN_LDS_XIN + 2 * SGN_VP * 4)
static_assert(SGN_FRAMES_LDS_FLOATS * 4 <= SGN_LDS_LIMIT, "agcn_sgn_frames: LDS");

// ---- dif[t] = x[t] - x[t - 1] inside a clip, zero at t = 0.  The neighbours of frame f = n * seg + t as guarded frame
// indices: -1 = no such term, so that no index ever leaves the clip. ----
SGN_HD long sgn_dif_prev(long f, int seg) { return f % seg > 0 ? f - 1 : -1; }          // the frame dif[t] subtracts
SGN_HD long sgn_dif_own(long f, int seg) { return f % seg > 0 ? f : -1; }               // dd[t] reaches x[t] iff t > 0
SGN_HD long sgn_dif_next(long f, int seg) { return f % seg + 1 < seg ? f + 1 : -1; }    // dd[t + 1] reaches x[t]

// ---- folded weight image of agcn_sgn_clip ----
struct SgnClipW {
  int tem1;                    // (seg, 256): tem_embed of the one-hot frames
  int t1_w, t1_b;              // local.cnn1 + bn1: (3 * 256, 256) with row dt * 256 + c, (256)
  int t2_w, t2_b;              // local.cnn2 + bn2: (256, 512), (512)
  int fc_w, fc_b;              // fc: (512, num_class), (num_class)
  long total;
};
SGN_HD SgnClipW sgn_clip_w(int seg, int num_class) {
  SgnClipW w;
  long o = 0;
  w.tem1 = (int)o; o += (long)seg * SGN_C3;
  w.t1_w = (int)o; o += 3 * SGN_C3 * SGN_C3;
  w.t1_b = (int)o; o += SGN_C3;
  w.t2_w = (int)o; o += SGN_C3 * SGN_C4;
  w.t2_b = (int)o; o += SGN_C4;
  w.fc_w = (int)o; o += (long)SGN_C4 * num_class;
  w.fc_b = (int)o; o += num_class;
  w.total = o;
  return w;
}

// LDS of agcn_sgn_clip: a tile of 32 frames with one halo frame on either side, its conv output, the running maximum
#define SGN_CLIP_STRIDE (SGN_C3 + 1)           // 257
#define SGN_CLIP_LDS_H 0                                               // (SGN_VP + 2, SGN_CLIP_STRIDE)
#define SGN_CLIP_LDS_Y (SGN_CLIP_LDS_H + (SGN_VP + 2) * SGN_CLIP_STRIDE)   // (SGN_VP, SGN_CLIP_STRIDE)
#define SGN_CLIP_LDS_MAX (SGN_CLIP_LDS_Y + SGN_VP * SGN_CLIP_STRIDE)   // (512)
#define SGN_CLIP_LDS_FLOATS (SGN_CLIP_LDS_MAX + SGN_C4)
static_assert(SGN_CLIP_LDS_FLOATS * 4 <= SGN_LDS_LIMIT, "agcn_sgn_clip: LDS");
SGN_HD int sgn_clip_tiles(int seg) { return (seg + SGN_VP - 1) / SGN_VP; }
// tile k owns the frames [32 k, 32 k + rows)
SGN_HD int sgn_tile_rows(int tile, int seg) {
  const int left = seg - tile * SGN_VP;
  return left < 0 ? 0 : left < SGN_VP ? left : SGN_VP;
}
// row 0..33 of a tile's H buffer holds frame 32 k - 1 + row, or the conv's zero padding (-1) outside the clip
SGN_HD int sgn_tile_frame(int tile, int row, int seg) {
  const int t = tile * SGN_VP - 1 + row;
  return t >= 0 && t < seg ? t : -1;
}

// ---- the sampler (reference feeders/loader.py:203-232, 302-358, equal-interval branch) ----
#define SGN_SAMPLE_MAX_T 2048                  // = agcn_prenorm_max_frames()
#define SGN_SAMPLE_MAX_ROWS (2 * SGN_SAMPLE_MAX_T)
#define SGN_SAMPLE_CHUNK (SGN_SAMPLE_MAX_ROWS / SGN_THREADS)      // rows (t, m) one thread flags and compacts: 16
SGN_HD bool sgn_sample_domain(long N, int T, int V, int K, long S, int seg) {
  return N >= 1 && N <= 0x7fffffffL && T >= 1 && T <= SGN_SAMPLE_MAX_T && V >= 2 && V <= SGN_MAX_V && K == 2 && S >= 1 &&
         seg >= 1 && S * seg <= (1 << 20);
}
// rows of the sequence that is sampled: the kept rows, followed by zero rows up to seg (pad_to_segment_length)
SGN_HD int sgn_sample_rows(int kept, int seg) { return kept < seg ? seg : kept; }
// interval boundary k of L rows in seg intervals: np.multiply(range(seg + 1), L / seg).round(), this expression order
SGN_HD int sgn_interval(int k, int L, int seg) { return (int)rint((double)k * ((double)L / (double)seg)); }
// the row a draw r picks in interval k, clamped into [0, L): a wrong plan gives a wrong number, never a wild read
SGN_HD int sgn_pick(int k, int L, int seg, unsigned r) {
  const int lo = sgn_interval(k, L, seg);
  int width = sgn_interval(k + 1, L, seg) - lo;
  if (width < 1) width = 1;
  int idx = lo + (int)(r % (unsigned)width);
  if (idx < 0) idx = 0;
  if (idx > L - 1) idx = L - 1;
  return idx;
}
// window (N, 3, T, V, 2) and output (N, S, seg, V * 3)
SGN_HD long sgn_win_index(long n, int c, int t, int v, int m, int T, int V) {
  return ((((n * 3 + c) * T + t) * V + v) << 1) + m;
}
SGN_HD long sgn_sample_out_index(long n, int s, int k, int f, int S, int seg, int V) {
  return ((n * S + s) * seg + k) * (long)(V * 3) + f;
}

// ---- the collate (reference feeders/loader.py:109-201: collate_fn_fix_{train,val,test}; feeders/tools.py:278-314) ----
// the sampler's domain on a pool of P samples; N clips are collated per launch
SGN_HD bool sgn_collate_domain(long P, long N, int T, int V, int K, long S, int seg) {
  return P >= 1 && P <= 0x7fffffffL && sgn_sample_domain(N, T, V, K, S, seg);
}
// the pool sample workgroup n collates, or -1: an index outside [0, P) selects nothing (an all-zero clip, L = 0)
SGN_HD long sgn_collate_source(const long long* index, long n, long P) {
  const long long i = index ? index[n] : (long long)n;
  return i >= 0 && i < (long long)P ? (long)i : -1;
}
// c = a . b, 3 x 3 row-major, each element summed in column order
SGN_HD void sgn_mat3_mul(const float* a, const float* b, float* c) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) c[i * 3 + j] = a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j];
}
// R = (Rz . Ry) . Rx of the angles a = (ax, ay, az) in radians, row-major, in fp32: the reference's _rot with its sign
// convention (the transposes of the usual right-handed matrices) and its association
SGN_HD void sgn_rotation(const float* a, float* R) {
  const float cx = cosf(a[0]), sx = sinf(a[0]), cy = cosf(a[1]), sy = sinf(a[1]), cz = cosf(a[2]), sz = sinf(a[2]);
  const float rx[9] = {1.f, 0.f, 0.f, 0.f, cx, sx, 0.f, -sx, cx};
  const float ry[9] = {cy, 0.f, -sy, 0.f, 1.f, 0.f, sy, 0.f, cy};
  const float rz[9] = {cz, sz, 0.f, -sz, cz, 0.f, 0.f, 0.f, 1.f};
  float zy[9];
  sgn_mat3_mul(rz, ry, zy);
  sgn_mat3_mul(zy, rx, R);
}
// component i of R . p
SGN_HD float sgn_rotate(const float* R, int i, float x, float y, float z) {
  return R[i * 3] * x + R[i * 3 + 1] * y + R[i * 3 + 2] * z;
}
// subject flags (N, S, seg)
SGN_HD long sgn_subject_index(long n, int s, int k, int S, int seg) { return (n * S + s) * seg + k; }
