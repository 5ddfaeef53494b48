// Implicit-GEMM channel contraction on NCHW skeleton tensors, exact fp32 on the CDNA4 matrix cores
// (v_mfma_f32_32x32x2_f32).  One kernel template covers
//   * unit_tcn's (9x1)/(1x1) temporal convolution forward           (reference agcn.py:40-41,49)
//   * its backward-data (transposed, tap-flipped; stride 2 split by output-frame parity into a 5-tap and a
//     4-tap stride-1 problem so no matrix-core work is spent on structural zeros)
//   * every 1x1 conv of unit_gcn (conv_a/conv_b/down)               (reference agcn.py:66-75,99-100)
//   * unit_gcn's fused aggregate+project  y = sum_i Wd_i (x . A^_i)  (reference agcn.py:103-105)
//     and its backward-data  dx = sum_i Wd_i^T (dy . A^_i^T)
//   * the adjacency gradient  dA^_i[u,v] = sum_{c,t} x[c,t,u] (Wd_i^T dy)[c,t,v]
//
// GEMM view per sample n and per tile of `tt` whole frames (tt*V <= BN positions):
//   out[n][m][q] = sum_{kc,tap} A(m,kc,tap) * B(n,kc,tap,q),   q = t_local*V + v
// * A: a tiny pack kernel first lays the weights out as the exact LDS image of every (row block, K chunk)
//   (zero padded, tap-flipped / transposed as the mode needs), so the hot kernel stages A with contiguous float4.
// * B: per K-chunk of CK channels the SOURCE WINDOW (tt+taps-1 frames) is staged in LDS once and every tap reads the
//   same window at +tap*V floats: the 9x reuse of the temporal convolution is served from LDS, not HBM.
//   For the aggregated variants the chunk is first multiplied by the sample's padded VxV adjacency on the matrix
//   cores and kept in LDS.
// * Software pipeline (register prefetch): the global loads of chunk k+1 are issued before the matrix-core loop of
//   chunk k and committed to LDS after it, so HBM/L2 latency hides under the MFMAs; operand fragments are read one
//   step ahead of the MFMAs that use them.
#include "agcn_common.h"
#include "epilogue.h"
#include "gate.h"
#include "split_f16.h"

namespace {

struct ConvGemmArgs {
  const float* in;
  const float* wp;     // packed weight images [mblocks][nchunks][KK][BM]
  const float* bias;
  float* out;
  const float* adj;    // AGG: (N,3,V,V)
  float* stats;        // [N*ntiles][2][M] partial (sum, sum of squares) or null
  const float* add1;
  const float* mask1;
  const float* add2;
  const float* mask2;
  const float* xin;    // DADJ: x (N,C,P)
  float* dadj;         // DADJ: partial buffer
  int N, M, Kinner, in_rows;
  int V, T_src, T_out, tt, ntiles;   // T_out = number of output frame slots tau this launch covers
  int src_stride, f_off;             // first source frame of a tile: t0*src_stride + f_off
  int out_fs, out_fo, T_full;        // output frame = tau*out_fs + out_fo ; T_full = frames of the out tensor
  int FW, WLP;
  int accumulate;
  int mask_bits;                     // mask1/mask2 are sign bit masks instead of fp32 tensors
  int C;                             // DADJ: channels of x
  int nchunks, nmb;
  int off_bx, off_bg, off_adj;       // LDS offsets (floats)
};

// EPI == 2 (agcn_tconv_infer) only -- a kernel argument type of its own, so that every other instantiation keeps the
// argument block it was tuned with: attention factors applied to `in` while it is staged (gate.h), the folded-BatchNorm
// store epilogue of epilogue.h (bias, residual `add1`, ReLU)
struct InferGemmArgs : ConvGemmArgs {
  GateArgs gate;
  int gated, relu;
  int off_bias, off_gate;            // LDS offsets (floats) of the bias row and the gate image, behind the epilogue tile
};
template <int EPI> struct GemmArgsOf { typedef ConvGemmArgs type; };
template <> struct GemmArgsOf<2> { typedef InferGemmArgs type; };

struct PackArgs {
  const float* w;
  float* wp;
  int M, Kinner, nchunks;
  long sa_m, sa_i, sa_c;
  int tap_mul, tap_add, tap_flip_from;   // weight tap = tap_flip_from >= 0 ? tap_flip_from - (j*tap_mul+tap_add) : j
};

// wp[((mb*nchunks + ch)*KK + kk)*BM + ml],  kk = (i*CK + kcl)*TAPS + j
template <int TAPS, int NSUB, int CK, int BM>
__global__ void __launch_bounds__(256) pack_weights_kernel(const PackArgs p) {
  constexpr int KK = NSUB * CK * TAPS;
  const int ch = blockIdx.x % p.nchunks, mb = blockIdx.x / p.nchunks;
  float* dst = p.wp + (long)blockIdx.x * KK * BM;
  for (int e = threadIdx.x; e < KK * BM; e += 256) {
    const int kk = e / BM, ml = e - kk * BM;
    const int i = kk / (CK * TAPS), r = kk - i * (CK * TAPS);
    const int kcl = r / TAPS, j = r - kcl * TAPS;
    const int m = mb * BM + ml, kc = ch * CK + kcl;
    const int gt = p.tap_flip_from >= 0 ? (p.tap_flip_from - (j * p.tap_mul + p.tap_add)) : j;
    float v = 0.f;
    if (m < p.M && kc < p.Kinner) v = p.w[(long)m * p.sa_m + (long)i * p.sa_i + (long)kc * p.sa_c + gt];
    dst[e] = v;
  }
}

// One 32x32 tile of the aggregation G = X . A^: all NS operand pairs are fetched from LDS first, then the NS
// dependent matrix-core steps run back to back (one LDS latency per tile instead of one per step).
// Rows u >= V of the padded adjacency image are zero, so the clamped x operand needs no masking.
template <int S0, int NS, int VMIN>   // VMIN = smallest V this chain is used with: only u >= VMIN needs the clamp
__device__ __forceinline__ f32x16 agg_chain(const float* bxrow, const float* adjcol, int V, int h, f32x16 d) {
  float av[NS], bv[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int u = 2 * (S0 + s) + h;
    av[s] = (2 * (S0 + s) + 1 < VMIN) ? bxrow[u] : bxrow[min(u, V - 1)];
    bv[s] = adjcol[u * 32];
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) d = mfma32(av[s], bv[s], d);
  __builtin_amdgcn_sched_barrier(0);   // keep the next chain's operand fetches from being hoisted above this one
  return d;
}

// WB = max number of 64-float column blocks of a staged window row (compile-time bound of the prefetch registers)
// EPI: 0 = plain store with BatchNorm partials, 1 = adjacency gradient, 2 = folded inference (gates on load, epilogue.h)
template <int TAPS, int AGG, int WM, int WN, int TM, int TN, int CK, int WB, int EPI>
__global__ void __launch_bounds__(WM* WN * 64, (TAPS == 1 && EPI == 0 && (AGG == 0 || WM * WN == 8) && (WB < 8 || WM * WN == 8)) ? 4 : 2) conv_gemm_kernel(const typename GemmArgsOf<EPI>::type a) {
  constexpr int NW = WM * WN, NT = NW * 64;
  constexpr int BM = WM * TM * 32;
  constexpr int NSUB = AGG ? 3 : 1;
  constexpr int KK = NSUB * CK * TAPS;       // rows of the staged A chunk
  constexpr int N4 = KK * BM / 4;            // float4s of one A image
  constexpr int EA = (N4 + NT - 1) / NT;     // A float4 per thread
  constexpr int RPW = (CK + NW - 1) / NW;    // B rows per wave
  static_assert(CK % 2 == 0, "CK must be even");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Aw = smem;
  float* Bx = smem + a.off_bx;
  float* Bg = smem + a.off_bg;
  float* adjp = smem + a.off_adj;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 31, h = lane >> 5;
  const int wm = wave / WN, wn = wave - wm * WN;
  // 1-D grid: the row blocks of one (sample, frame tile) are adjacent (they stage the same source window, so
  // it is served from the XCD's L2), and xcd_remap keeps neighbouring tiles on one XCD
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int mbk = bid % a.nmb;
  const int nt_id = bid / a.nmb;
  const int n = nt_id / a.ntiles, tile = nt_id - n * a.ntiles;
  const int m0 = mbk * BM;
  const int V = a.V, tt = a.tt, t0 = tile * tt;
  const int ttv = tt * V;
  const int tvalid = min(tt, a.T_out - t0);
  const int nvalid = tvalid * V;
  const int Psrc = a.T_src * V;
  const int f0 = t0 * a.src_stride + a.f_off;
  const int WL = a.FW * V;
  const int WLP = a.WLP;

  // per-lane B offsets / output offsets for the TN position tiles of this wave
  int boff[TN], ooff[TN];
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) {
    int q = (wn * TN + tn) * 32 + lr;
    if (q >= ttv) q = 0;              // padding lanes read position 0; their results are discarded
    const int tl = q / V, v = q - tl * V;
    boff[tn] = AGG ? q : (tl * a.src_stride * V + v);
    ooff[tn] = ((t0 + tl) * a.out_fs + a.out_fo) * V + v;
  }

  if (AGG) {
    // zero-padded adjacency fragments: adjp[i][u][col], u < VP (even), col < 32
    const int VP = 2 * ((V + 1) / 2);
    const float* adjn = a.adj + (long)n * 3 * V * V;
    for (int e = tid; e < 3 * VP * 32; e += NT) {
      const int i = e / (VP * 32), r = e - i * (VP * 32);
      const int u = r >> 5, col = r & 31;
      const bool ok = u < V && col < V;
      const int gi = ok ? ((AGG == 1) ? ((i * V + u) * V + col) : ((i * V + col) * V + u)) : 0;
      const float t = adjn[gi];
      adjp[e] = ok ? t : 0.f;
    }
  }

  f32x16 acc[TM][TN];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[tm][tn][j] = 0.f;

  // ---- prefetch registers ----
  f32x4 ra[EA];
  float rb[RPW][WB];
  // EPI == 2: bias row and gate vectors in LDS; a lane stages the same window positions in every K chunk, so their
  // (joint, frame) factor is taken once
  const int KPG = a.nchunks * CK;
  const float* gl = smem;
  bool gated = false;
  float gpos[WB];
  if constexpr (EPI == 2) {
    gl = smem + a.off_gate;
    gated = a.gated != 0;
    for (int e = tid; e < BM; e += NT) smem[a.off_bias + e] = (a.bias && m0 + e < a.M) ? a.bias[m0 + e] : 0.f;
    if (gated) {
      gate_stage<NT>(smem + a.off_gate, a.gate, n, V, a.T_src, a.Kinner, f0, a.FW, KPG);
      __syncthreads();
#pragma unroll
      for (int u = 0; u < WB; ++u) gpos[u] = gate_pos(gl, KPG, lane + 64 * u, V, WL);
    }
  }
  const f32x4* wp4 = reinterpret_cast<const f32x4*>(a.wp) + (long)mbk * a.nchunks * N4;
  const int g0 = f0 * V;

  // NOTE: the loaded values are kept RAW in registers; range predicates are re-evaluated at commit time, so
  // nothing consumes a load result before the matrix-core loop it is meant to hide under.
  auto issue_loads = [&](int ch) __attribute__((always_inline)) {
    const f32x4* src = wp4 + (long)ch * N4;
#pragma unroll
    for (int u = 0; u < EA; ++u) ra[u] = src[min(tid + u * NT, N4 - 1)];
    const int kc0 = ch * CK;
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
      const int kcl = wave + j * NW;
      const bool rok = kcl < CK && (kc0 + kcl) < a.Kinner;
      const float* rowp = a.in + ((long)n * a.in_rows + (rok ? (kc0 + kcl) : 0)) * Psrc;
#pragma unroll
      for (int u = 0; u < WB; ++u) {
        const int r = lane + 64 * u;
        const int gp = g0 + r;
        const bool ok = rok && r < WL && gp >= 0 && gp < Psrc;
        rb[j][u] = rowp[ok ? gp : 0];
      }
    }
  };
  auto commit_lds = [&](int ch) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < EA; ++u)
      if (tid + u * NT < N4) reinterpret_cast<f32x4*>(Aw)[tid + u * NT] = ra[u];
    const int kc0 = ch * CK;
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
      const int kcl = wave + j * NW;
      const bool rok = kcl < CK && (kc0 + kcl) < a.Kinner;
#pragma unroll
      for (int u = 0; u < WB; ++u) {
        const int r = lane + 64 * u;
        const int gp = g0 + r;
        const bool ok = rok && gp >= 0 && gp < Psrc;
        if constexpr (EPI == 2) {
          float xv = ok ? rb[j][u] : 0.f;
          if (gated) xv = xv * gpos[u] * gl[min(kc0 + kcl, KPG - 1)];   // (the channel factor is a wave-uniform LDS read)
          if (kcl < CK && r < WL) Bx[kcl * WLP + r] = xv;
        } else {
          if (kcl < CK && r < WL) Bx[kcl * WLP + r] = ok ? rb[j][u] : 0.f;
        }
      }
    }
  };

  // DADJ: the x tile of the epilogue is fetched now (raw, into registers) so its latency hides under the K loop
  constexpr int XR = (EPI == 1) ? (BM / NW) : 1;
  float rx[XR][2];
  if (EPI == 1) {
#pragma unroll
    for (int j = 0; j < XR; ++j) {
      const int m = m0 + wave + j * NW;
      const bool okr = m < a.M;
      const float* src = a.xin + ((long)n * a.C + (okr ? (m % a.C) : 0)) * ((long)a.T_full * V) + (long)t0 * V;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int q = lane + 64 * u;
        rx[j][u] = src[(okr && q < nvalid) ? q : 0];
      }
    }
  }

  const int nchunks = a.nchunks;
  if (nchunks > 0) issue_loads(0);
  for (int ch = 0; ch < nchunks; ++ch) {
    __syncthreads();                       // every wave is done reading the previous chunk from LDS
    commit_lds(ch);
    if (ch + 1 < nchunks) issue_loads(ch + 1);   // in flight during this chunk's matrix-core loop
    __syncthreads();
    if (AGG) {
      // Bg[i][c_local][q] = sum_u Bx[c_local][t*V+u] * adj_i[u][v]   (rows r=(c_local,t), 32 per MFMA tile)
      const int nrows = CK * tt;
      const int nrt = (nrows + 31) >> 5;
      const int VS = (V + 1) >> 1;
      const int VP = 2 * VS;
      for (int tl = wave; tl < 3 * nrt; tl += NW) {
        const int i = tl / nrt, rt = tl - i * nrt;
        const int row = min(rt * 32 + lr, nrows - 1);
        const float* bxrow = Bx + row * V;
        const float* adjcol = adjp + i * VP * 32 + lr;
        f32x16 d;
#pragma unroll
        for (int j = 0; j < 16; ++j) d[j] = 0.f;
        if (NW != 8 && VS == 13) {          // V = 25 (NTU)
          d = agg_chain<0, 13, 25>(bxrow, adjcol, V, h, d);
        } else if (NW != 8 && VS == 9) {    // V = 18 (Kinetics)
          d = agg_chain<0, 9, 17>(bxrow, adjcol, V, h, d);
        } else {
          // 8-wave variant (128-register budget) and other V: plain loop (a longer unrolled chain spills there)
          for (int s = 0; s < VS; ++s) {
            const int u = 2 * s + h;
            d = mfma32(bxrow[min(u, V - 1)], adjcol[u * 32], d);
          }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int r2 = rt * 32 + mfma_row(j, h);
          if (r2 < nrows && lr < V) Bg[i * CK * ttv + r2 * V + lr] = d[j];
        }
      }
      __syncthreads();
    }
    // ---- matrix-core contraction over this chunk; operands are fetched one step ahead ----
    constexpr int KP = (NSUB * CK) / 2;
    const float* Bsrc = AGG ? Bg : Bx;
    const int BP = AGG ? ttv : WLP;
    const float* Arow = Aw + (wm * TM) * 32 + lr;
    float av[TM], bv[TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) av[tm] = Arow[(h * TAPS) * BM + tm * 32];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) bv[tn] = Bsrc[h * BP + boff[tn]];
#pragma unroll 1
    for (int kp = 0; kp < KP; ++kp) {
      const int krow = 2 * kp + h;
#pragma unroll
      for (int tap = 0; tap < TAPS; ++tap) {
        // next step (clamped at the end: a harmless re-read)
        const int ntap = (tap == TAPS - 1) ? 0 : tap + 1;
        const int nkrow = (tap == TAPS - 1) ? min(krow + 2, 2 * (KP - 1) + h) : krow;
        float an[TM], bn[TN];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) an[tm] = Arow[(nkrow * TAPS + ntap) * BM + tm * 32];
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) bn[tn] = Bsrc[nkrow * BP + boff[tn] + (AGG ? 0 : ntap * V)];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = mfma32(av[tm], bv[tn], acc[tm][tn]);
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) av[tm] = an[tm];
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) bv[tn] = bn[tn];
      }
    }
  }

  if constexpr (EPI == 2) {
    // ---- folded inference: tile -> LDS -> epilogue.h (bias, residual, ReLU; coalesced row stores) ----
    constexpr int TP = WN * TN * 32 + 1;
    float* otile = smem;                // [BM][TP]; the bias row and the gate image lie behind it
    float* red = otile + BM * TP;
    __syncthreads();                   // every wave is done with the A/B images
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int j = 0; j < 16; ++j)
          otile[((wm * TM + tm) * 32 + mfma_row(j, h)) * TP + (wn * TN + tn) * 32 + lr] = acc[tm][tn][j];
    __syncthreads();
    constexpr int XB = WN * TN * 32 / 64;
    int poff[XB];
#pragma unroll
    for (int u = 0; u < XB; ++u) {
      const int q2 = lane + 64 * u;
      const int tl2 = q2 / V;
      poff[u] = tl2 * a.out_fs * V + (q2 - tl2 * V);
    }
    EpiPtrs ep;
    ep.out = a.out; ep.add1 = a.add1; ep.mask1 = nullptr; ep.add2 = nullptr; ep.mask2 = nullptr; ep.stats = nullptr;
    ep.accumulate = 0; ep.relu = a.relu;
    const long Pfull = (long)a.T_full * V;
    const long rows0 = (long)n * a.M * Pfull + ((long)t0 * a.out_fs + a.out_fo) * V;
    epilogue_rows<BM, NW, XB>(ep, otile, TP, smem + a.off_bias, red, a.M, m0, rows0, Pfull, nvalid, poff,
                              (long)n * a.ntiles + tile);
  } else if (EPI == 0) {
    // ---- store (+bias, +accumulate, +masked addends) and per-channel (sum, sumsq) partials ----
    float* red = smem;   // aliases Aw: [WN][2][BM]
    const long Pfull = (long)a.T_full * V;
    if (a.stats) __syncthreads();
    const bool has_extra = a.accumulate || a.add1 || a.add2;   // kernel-uniform
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) {
        // 4 rows x TN columns per batch: all residual/accumulate loads of the batch are issued together, with
        // clamped (always valid) addresses, instead of one exec-masked load -> wait per element
        float ex[4][TN];
        long idxs[4][TN];
        bool oks[4][TN];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int m = m0 + (wm * TM + tm) * 32 + mfma_row(jb * 4 + jj, h);
#pragma unroll
          for (int tn = 0; tn < TN; ++tn) {
            const int q = (wn * TN + tn) * 32 + lr;
            oks[jj][tn] = (m < a.M) && (q < nvalid);
            idxs[jj][tn] = oks[jj][tn] ? (((long)n * a.M + m) * Pfull + ooff[tn]) : 0;
            ex[jj][tn] = 0.f;
          }
        }
        if (has_extra) {
#pragma unroll
          for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
              const long idx = idxs[jj][tn];
              float e = 0.f;
              if (a.accumulate) e += a.out[idx];
              if (a.add1) {
                float t = a.add1[idx];
                if (a.mask1) t = mask_pass(mask_load(a.mask1, idx, a.mask_bits), idx, a.mask_bits) ? t : 0.f;
                e += t;
              }
              if (a.add2) {
                float t = a.add2[idx];
                if (a.mask2) t = mask_pass(mask_load(a.mask2, idx, a.mask_bits), idx, a.mask_bits) ? t : 0.f;
                e += t;
              }
              ex[jj][tn] = e;
            }
        }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int j = jb * 4 + jj;
          const int ml = (wm * TM + tm) * 32 + mfma_row(j, h);
          const int m = m0 + ml;
          const float bval = (a.bias && m < a.M) ? a.bias[m] : 0.f;
          float bsum = 0.f, bsq = 0.f;
#pragma unroll
          for (int tn = 0; tn < TN; ++tn) {
            const float val = acc[tm][tn][j] + bval + ex[jj][tn];
            if (oks[jj][tn]) {
              a.out[idxs[jj][tn]] = val;
              bsum += val;
              bsq += val * val;
            }
          }
          if (a.stats) {
            bsum = half_sum(bsum);
            bsq = half_sum(bsq);
            if (lr == 0) {
              red[(wn * 2 + 0) * BM + ml] = bsum;
              red[(wn * 2 + 1) * BM + ml] = bsq;
            }
          }
        }
      }
    }
    if (a.stats) {
      __syncthreads();
      const long slot = (long)n * a.ntiles + tile;
      for (int e = tid; e < 2 * BM; e += NT) {
        const int k = e / BM, ml = e - k * BM;
        float s = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < WN; ++w2) s += red[(w2 * 2 + k) * BM + ml];
        if (m0 + ml < a.M) a.stats[(slot * 2 + k) * a.M + m0 + ml] = s;
      }
    }
  } else {
    // ---- DADJ: dadj_i[u][v] = sum_{c,t} x[c][t,u] * acc[(i,c)][t,v]; rows of this block are m=(i,c) ----
    const int C = a.C;
    const int Pout = a.T_full * V;
    float* Dg = smem;                 // [BM][ttv]
    float* Xs = smem + BM * ttv;      // [BM][ttv]
    float* red2 = Xs + BM * ttv;      // [NW][V*V]
    __syncthreads();
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int ml = (wm * TM + tm) * 32 + mfma_row(j, h);
          const int q = (wn * TN + tn) * 32 + lr;
          if (q < ttv) Dg[ml * ttv + q] = (q < nvalid && m0 + ml < a.M) ? acc[tm][tn][j] : 0.f;
        }
#pragma unroll
    for (int j = 0; j < XR; ++j) {
      const int ml = wave + j * NW;
      const bool okr = (m0 + ml) < a.M;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int q = lane + 64 * u;
        if (q < ttv) Xs[ml * ttv + q] = (okr && q < nvalid) ? rx[j][u] : 0.f;
      }
    }
    __syncthreads();
    const int nmb = (C >= BM) ? (C / BM) : 1;
    const int VV = V * V;
    for (int i = 0; i < 3; ++i) {
      if (i * C >= a.M) continue;   // block-uniform: a launch over one subset's rows (gcn_dadj_route) has no others
      const int c_lo = max(0, m0 - i * C), c_hi = min(C, m0 + BM - i * C);
      if (c_lo >= c_hi) continue;   // block-uniform
      const int npairs = (c_hi - c_lo + 1) >> 1;
      f32x16 d;
#pragma unroll
      for (int j = 0; j < 16; ++j) d[j] = 0.f;
      const int lc = min(lr, V - 1);
      for (int it = wave; it < npairs * tt; it += NW) {
        const int ap = it / tt, tl = it - ap * tt;
        const int c = c_lo + 2 * ap + h;
        const bool ok = (c < c_hi) && (lr < V);
        const int ml = i * C + min(c, c_hi - 1) - m0;
        float xv = Xs[ml * ttv + tl * V + lc];
        float gv = Dg[ml * ttv + tl * V + lc];
        xv = ok ? xv : 0.f;
        gv = ok ? gv : 0.f;
        d = mfma32(xv, gv, d);
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int u = mfma_row(j, h);
        if (u < V && lr < V) red2[wave * VV + u * V + lr] = d[j];
      }
      __syncthreads();
      const int slot = tile * nmb + ((C >= BM) ? (mbk - i * nmb) : 0);
      float* dst = a.dadj + (((long)n * 3 + i) * ((long)a.ntiles * nmb) + slot) * VV;
      for (int e = tid; e < VV; e += NT) {
        float s = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < NW; ++w2) s += red2[w2 * VV + e];
        dst[e] = s;
      }
      __syncthreads();
    }
  }
}

struct Geometry {
  int tt, ntiles, FW, WLP, ttv, nchunks, nmb;
  size_t smem_bytes, pack_floats;
  int off_bx, off_bg, off_adj;
  int off_bias, off_gate;            // EPI == 2
};

// host-side tile geometry shared by the launcher and the workspace queries
template <int TAPS, int AGG, int WM, int WN, int TM, int TN, int CK, int EPI>
Geometry make_geometry(int V, int T_out, int src_stride, int M, int Kinner, int tt_cap = 0) {
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32, NSUB = AGG ? 3 : 1, NW = WM * WN;
  Geometry g;
  g.tt = BN / V;
  if (g.tt > T_out) g.tt = T_out;
  if (tt_cap > 0 && g.tt > tt_cap) g.tt = tt_cap;     // long strided windows (agcn_tconv_*): fewer frames per tile
  if (g.tt < 1) g.tt = 1;
  g.ttv = g.tt * V;
  g.ntiles = (T_out + g.tt - 1) / g.tt;
  g.FW = AGG ? g.tt : ((g.tt - 1) * src_stride + TAPS);
  g.WLP = AGG ? g.ttv : g.FW * V + 8;
  g.nchunks = (Kinner + CK - 1) / CK;
  g.nmb = (M + BM - 1) / BM;
  const int aw = NSUB * CK * TAPS * BM;
  g.off_bx = (aw + 3) & ~3;
  const int bx = CK * g.WLP + 64;
  g.off_bg = g.off_bx + ((bx + 3) & ~3);
  const int bgsz = AGG ? (3 * CK * g.ttv + 64) : 0;
  g.off_adj = g.off_bg + ((bgsz + 3) & ~3);
  const int VP = 2 * ((V + 1) / 2);
  const int adjsz = AGG ? 3 * VP * 32 : 0;
  size_t main_f = (size_t)g.off_adj + adjsz;
  size_t epi_f = (EPI == 0) ? (size_t)WN * 2 * BM : (size_t)2 * BM * g.ttv + (size_t)NW * V * V;
  if (EPI == 2) epi_f = (size_t)BM * (WN * TN * 32 + 1) + (size_t)NW * 64 * 2;   // epilogue.h: tile + scratch
  g.smem_bytes = 4 * (main_f > epi_f ? main_f : epi_f);
  g.off_bias = g.off_gate = 0;
  if (EPI == 2) {                     // bias row and gate image (gate.h) behind everything the epilogue overwrites
    g.off_bias = (int)((g.smem_bytes / 4 + 3) & ~(size_t)3);
    g.off_gate = g.off_bias + BM;
    g.smem_bytes = 4 * ((size_t)g.off_gate + gate_lds_floats(g.FW, g.nchunks * CK));
  }
  g.pack_floats = (size_t)g.nmb * g.nchunks * aw;
  return g;
}

struct Problem {          // what differs between the entry points
  ConvGemmArgs a;
  GateArgs gate;          // EPI == 2: see InferGemmArgs
  int gated, relu;
  const float* w;
  long sa_m, sa_i, sa_c;
  int tap_mul, tap_add, tap_flip_from;
  void* ws;
  size_t ws_bytes;
  int tt_cap;             // 0: frames per tile as the tile width gives them
  AgcnDryRun* dry;        // non-null: a size query (agcn_common.h), nothing is launched
};

template <int TAPS, int AGG, int WM, int WN, int TM, int TN, int CK, int WB, int EPI>
int launch_cfg(Problem& p, hipStream_t stream) {
  constexpr int BM = WM * TM * 32, NSUB = AGG ? 3 : 1;
  typename GemmArgsOf<EPI>::type a;
  static_cast<ConvGemmArgs&>(a) = p.a;
  const Geometry g = make_geometry<TAPS, AGG, WM, WN, TM, TN, CK, EPI>(a.V, a.T_out, a.src_stride, a.M, a.Kinner, p.tt_cap);
  if (g.smem_bytes > 160 * 1024) return AGCN_ERR_UNSUPPORTED;
  if (g.FW * a.V > WB * 64) return AGCN_ERR_UNSUPPORTED;
  if (p.dry) {            // BatchNorm partials: one slot per (sample, tile); adjacency partials: per (sample, subset, tile, row block)
    const long slots = a.stats ? (long)a.N * g.ntiles : a.dadj ? 3L * a.N * g.ntiles * (a.C >= BM ? a.C / BM : 1) : 0;
    return agcn_dry_note(p.dry, slots, g.pack_floats * 4);
  }
  if (g.pack_floats * 4 > p.ws_bytes) return AGCN_ERR_WORKSPACE;
  a.tt = g.tt; a.ntiles = g.ntiles; a.FW = g.FW; a.WLP = g.WLP; a.nchunks = g.nchunks; a.nmb = g.nmb;
  a.off_bx = g.off_bx; a.off_bg = g.off_bg; a.off_adj = g.off_adj;
  if constexpr (EPI == 2) {
    a.gate = p.gate; a.gated = p.gated; a.relu = p.relu;
    a.off_bias = g.off_bias; a.off_gate = g.off_gate;
  }
  a.wp = (const float*)p.ws;
  if (g.nchunks > 0) {
    PackArgs pk;
    pk.w = p.w; pk.wp = (float*)p.ws; pk.M = a.M; pk.Kinner = a.Kinner; pk.nchunks = g.nchunks;
    pk.sa_m = p.sa_m; pk.sa_i = p.sa_i; pk.sa_c = p.sa_c;
    pk.tap_mul = p.tap_mul; pk.tap_add = p.tap_add; pk.tap_flip_from = p.tap_flip_from;
    hipLaunchKernelGGL((pack_weights_kernel<TAPS, NSUB, CK, BM>), dim3(g.nmb * g.nchunks), dim3(256), 0, stream, pk);
    int rc = agcn_check_launch();
    if (rc) return rc;
  }
  if (EPI == 2 && p.gated)
    AGCN_NOTE_KERNEL("conv_gemm_kernel<%d, %d, %d, %d, %d, %d, %d, %d, %d> [gates on load]", TAPS, AGG, WM, WN, TM, TN, CK, WB, EPI);
  else
    AGCN_NOTE_KERNEL("conv_gemm_kernel<%d, %d, %d, %d, %d, %d, %d, %d, %d>", TAPS, AGG, WM, WN, TM, TN, CK, WB, EPI);
  return agcn_launch_big<conv_gemm_kernel<TAPS, AGG, WM, WN, TM, TN, CK, WB, EPI>>(
      dim3((unsigned)(a.N * g.ntiles * g.nmb)), dim3(WM * WN * 64), g.smem_bytes, stream, a);
}

// BM = 64 (4 waves) unless M is a multiple of 128 (8 waves, BM = 128)
#define DISPATCH_BM(TAPS, AGG, CK64, CK128, WB, p, s)                                        \
  (((p).a.M % 128 == 0) ? launch_cfg<TAPS, AGG, 2, 4, 2, 2, CK128, WB, 0>((p), (s))          \
                        : launch_cfg<TAPS, AGG, 1, 4, 2, 2, CK64, WB, 0>((p), (s)))

constexpr int CK9 = 8, CK1 = 16, CKA = 8, CKD = 64;

// ---- temporal convolution with any taps (1..9), stride (1..9) and padding (0..(taps-1)/2): agcn_tconv_* ----
constexpr int WBT = 12;                 // window bound of the exact-f32 kernel (768 floats per staged row)

// frames per tile of the exact-f32 kernel: a staged window row of (tt-1)*stride + taps frames must fit WBT*64 floats
inline int tconv_f32_tt(int V, int T_out, int taps, int stride) {
  int tt = 256 / V;
  if (tt > T_out) tt = T_out;
  while (tt > 1 && ((tt - 1) * stride + taps) * V > WBT * 64) --tt;
  return tt < 1 ? 1 : tt;
}

// One pass of a plan (tconv_plan.h) on the exact-f32 kernel.  The passes of the legacy shapes (1 or 9 taps, "same"
// padding, stride 1 or 2; backward: 9, or 5 and 4 at stride 2, or 1, the empty pass included) keep the window bounds they
// were tuned with and the full tile; every other pass takes WBT and as many frames per tile as its window allows.
template <int TAPS>
int tconv_f32_launch(Problem& p, bool legacy, bool bwd, hipStream_t s) {
  constexpr int CK = TAPS == 1 ? CK1 : CK9;
  if (legacy) {
    if constexpr (TAPS == 9) return bwd ? DISPATCH_BM(9, 0, CK9, CK9, 8, p, s) : DISPATCH_BM(9, 0, CK9, CK9, 11, p, s);
    if constexpr (TAPS == 5 || TAPS == 4) return DISPATCH_BM(TAPS, 0, CK9, CK9, 8, p, s);
    if constexpr (TAPS == 1) return p.a.src_stride == 2 ? DISPATCH_BM(1, 0, CK1, CK1, 8, p, s) : DISPATCH_BM(1, 0, CK1, CK1, 4, p, s);
  }
  p.tt_cap = tconv_f32_tt(p.a.V, p.a.T_out, TAPS, p.a.src_stride);
  return DISPATCH_BM(TAPS, 0, CK, CK, WBT, p, s);
}

// folded inference on the exact-f32 kernel: 64-row blocks (the epilogue tile of epilogue.h is 64 x 257 floats of LDS)
template <int TAPS>
int tconv_f32_infer_launch(Problem& p, hipStream_t s) {
  constexpr int CK = TAPS == 1 ? CK1 : CK9;
  p.tt_cap = tconv_f32_tt(p.a.V, p.a.T_out, TAPS, p.a.src_stride);
  return launch_cfg<TAPS, 0, 1, 4, 2, 2, CK, WBT, 2>(p, s);
}

// ---- the routing of each entry point, after its argument checks.  The size queries walk the same functions with null
// tensors and a dry-run record (agcn_common.h): there is one copy of every routing decision.  In a dry run an operand
// whose presence steers the routing may be a placeholder (agcn_dry_present): no route function dereferences a tensor. ----

// what every call of the register-chained graph kernels (gcn_chain.hip) sets; the routes add their operands
GcnChainCall gcn_chain_call(int mode, const float* adj, const float* wcat, void* ws, size_t ws_bytes, int N, int C,
                            int Cout, int T, int V, AgcnDryRun* dry) {
  GcnChainCall c;
  c.mode = mode; c.adj = adj; c.wcat = wcat; c.ws = ws; c.ws_bytes = ws_bytes;
  c.N = N; c.C = C; c.Cout = Cout; c.T = T; c.V = V; c.dry = dry;
  return c;
}

// y[n][o][t,v] = bias[o] + sum_i sum_c wcat[o][i*C+c] * sum_u x[n][c][t,u] adj[n][i][u][v]
int gcn_fwd_route(const float* x, const float* adj, const float* wcat, const float* bias, float* y, float* stats_part,
                  void* workspace, size_t workspace_bytes, int N, int C, int Cout, int T, int V, const float* x_absmax,
                  hipStream_t s, AgcnDryRun* dry) {
  // (the 3-channel first layer's forward stays on the f32 kernel: measured 193 us against 260 us chained)
  if (agcn_chained() && C >= 32 && agcn_gcn_chain_supported(Cout, C, V)) {
    GcnChainCall c = gcn_chain_call(0, adj, wcat, workspace, workspace_bytes, N, C, Cout, T, V, dry);
    c.in = x; c.in_absmax = x_absmax; c.bias = bias; c.out = y; c.stats_part = stats_part;
    return agcn_gcn_chain(c, s);
  }
  Problem p = {};
  p.dry = dry;
  ConvGemmArgs& a = p.a;
  a.in = x; a.bias = bias; a.out = y; a.adj = adj; a.stats = stats_part;
  a.N = N; a.M = Cout; a.Kinner = C; a.in_rows = C; a.V = V; a.T_src = T; a.T_out = T; a.T_full = T;
  a.src_stride = 1; a.f_off = 0; a.out_fs = 1; a.out_fo = 0;
  p.w = wcat; p.sa_m = 3L * C; p.sa_i = C; p.sa_c = 1; p.tap_flip_from = -1;
  p.ws = workspace; p.ws_bytes = workspace_bytes;
  return DISPATCH_BM(1, 1, CKA, CKA, 4, p, s);
}

// dx[n][c][t,u] (+)= sum_i sum_o wcat[o][i*C+c] * sum_v dy[n][o][t,v] adj[n][i][u][v]   (+ masked addends); dtp
// non-null: plus the fused 1x1 term W2^T dtp (chained path only)
int gcn_bwd_data_route(const float* dy, const float* adj, const float* wcat, const float* dtp, const float* w2, int K2,
                       float* dx, int accumulate, const float* add1, const float* mask1, const float* add2,
                       const float* mask2, int mask_bits, void* workspace, size_t workspace_bytes, int N, int C, int Cout,
                       int T, int V, const float* dy_absmax, const float* dtp_absmax, hipStream_t s, AgcnDryRun* dry) {
  const bool chain = agcn_chained() && agcn_gcn_chain_supported(C, Cout, V);
  if (dtp && !chain) return AGCN_ERR_UNSUPPORTED;
  if (chain) {
    GcnChainCall c = gcn_chain_call(1, adj, wcat, workspace, workspace_bytes, N, C, Cout, T, V, dry);
    c.in = dy; c.in_absmax = dy_absmax; c.out = dx; c.accumulate = accumulate;
    c.add1 = add1; c.mask1 = mask1; c.add2 = add2; c.mask2 = mask2; c.mask_bits = mask_bits;
    if (dtp) { c.in2 = dtp; c.w2 = w2; c.K2 = K2; c.in2_absmax = dtp_absmax; }
    return agcn_gcn_chain(c, s);
  }
  Problem p = {};
  p.dry = dry;
  ConvGemmArgs& a = p.a;
  a.in = dy; a.out = dx; a.adj = adj; a.accumulate = accumulate;
  a.add1 = add1; a.mask1 = mask1; a.add2 = add2; a.mask2 = mask2; a.mask_bits = mask_bits;
  a.N = N; a.M = C; a.Kinner = Cout; a.in_rows = Cout; a.V = V; a.T_src = T; a.T_out = T; a.T_full = T;
  a.src_stride = 1; a.f_off = 0; a.out_fs = 1; a.out_fo = 0;
  p.w = wcat; p.sa_m = 1; p.sa_i = C; p.sa_c = 3L * C; p.tap_flip_from = -1;
  p.ws = workspace; p.ws_bytes = workspace_bytes;
  return DISPATCH_BM(1, 2, CKA, CKA, 4, p, s);
}

// dadj_part[n][i][slot][u][v] = sum over the slot's (c,t) of x[n][c][t,u] * (sum_o wcat[o][i*C+c] dy[n][o][t,v])
int gcn_dadj_route(const float* dy, const float* wcat, const float* x, float* dadj_part, void* workspace,
                   size_t workspace_bytes, int N, int C, int Cout, int T, int V, const float* dy_absmax,
                   const float* x_absmax, hipStream_t s, AgcnDryRun* dry) {
  if (agcn_chained() && agcn_gcn_dadj_chain_supported(C, V))
    return agcn_gcn_dadj_chain(dy, wcat, x, dadj_part, workspace, workspace_bytes, N, C, Cout, T, V, s, dy_absmax,
                               x_absmax, dry);
  if (C >= 64 && C % 64 != 0) return AGCN_ERR_UNSUPPORTED;
  Problem p = {};
  p.dry = dry;
  ConvGemmArgs& a = p.a;
  a.in = dy; a.xin = x; a.dadj = dadj_part;
  a.N = N; a.M = 3 * C; a.Kinner = Cout; a.in_rows = Cout; a.V = V; a.T_src = T; a.T_out = T; a.T_full = T;
  a.src_stride = 1; a.f_off = 0; a.out_fs = 1; a.out_fo = 0; a.C = C;
  p.w = wcat; p.sa_m = 1; p.sa_i = 0; p.sa_c = 3L * C; p.tap_flip_from = -1;
  p.ws = workspace; p.ws_bytes = workspace_bytes;
  constexpr int BM = 64;            // rows of a block of this configuration
  if (C < BM && 3 * C > BM) {
    // the rows of one subset would straddle two row blocks, which share one slot per (sample, subset, tile): one launch
    // per subset instead (C rows, a single row block), each into its own third of every sample's slots.  The size
    // query dry-runs one of the three (they are alike): the same slots as the 3C-row form, the C-row launch's workspace.
    a.M = C;
    if (dry) return launch_cfg<1, 0, 1, 4, 2, 1, CKD, 2, 1>(p, s);
    const long per_subset = (long)make_geometry<1, 0, 1, 4, 2, 1, CKD, 1>(V, T, 1, C, Cout).ntiles * V * V;
    for (int i = 0; i < 3; ++i) {
      p.w = wcat + (long)i * C;
      a.dadj = dadj_part + i * per_subset;
      int rc = launch_cfg<1, 0, 1, 4, 2, 1, CKD, 2, 1>(p, s);
      if (rc != AGCN_OK) return rc;
    }
    char name[128];
    snprintf(name, sizeof(name), "%s", agcn_last_kernel_buf);
    AGCN_NOTE_KERNEL("%s [one launch per subset]", name);
    return AGCN_OK;
  }
  return launch_cfg<1, 0, 1, 4, 2, 1, CKD, 2, 1>(p, s);
}

// y = act( bias + sum_i W_i (x . adj_i) [+ res] [+ W2 . x2] ): only on the chained split-bf16 path (C >= 32)
int gcn_unit_infer_route(const float* x, const float* adj, const float* wcat, const float* bias, const float* res,
                         const float* x2, const float* w2, int K2, int relu, float* y, void* workspace,
                         size_t workspace_bytes, int N, int C, int Cout, int T, int V, hipStream_t s, AgcnDryRun* dry) {
  if (!(agcn_chained() && C >= 32 && agcn_gcn_chain_supported(Cout, C, V))) return AGCN_ERR_UNSUPPORTED;
  if (x2 && K2 % 32 != 0) return AGCN_ERR_UNSUPPORTED;
  GcnChainCall c = gcn_chain_call(0, adj, wcat, workspace, workspace_bytes, N, C, Cout, T, V, dry);
  c.in = x; c.bias = bias; c.out = y; c.add1 = res; c.relu = relu;
  c.in2 = x2; c.w2 = w2; c.K2 = x2 ? K2 : 0; c.w2_rows_are_outputs = 1;
  return agcn_gcn_chain(c, s);
}

// The temporal convolution's three data routes.  Each builds the plan of tconv_plan.h and hands its passes to one rung:
// the split-bf16 / f16x3 kernels of conv_gemm_bf16.hip for the shapes they are tuned for (unless AGCN_GEMM=f32), else the
// exact-f32 kernel with the window bound of tconv_f32_launch.

// y[n][o][t,v] = bias[o] + sum_{c,k} w[o][c][k] x[n][c][t*stride + k - pad, v],  T_out = (T + 2 pad - taps)/stride + 1
int tconv_fwd_route(const float* x, const float* w, const float* bias, float* y, float* stats_part, void* workspace,
                    size_t workspace_bytes, int N, int Cin, int Cout, int T, int V, int taps, int stride, int pad,
                    const float* x_absmax, hipStream_t s, AgcnDryRun* dry) {
  if (!agcn_tconv_domain(T, taps, stride, pad)) return AGCN_ERR_UNSUPPORTED;
  // (the 1x1 forward is store-bound and stays on the exact kernel)
  if (agcn_gemm_precision() != 0 && agcn_bf16_tconv_supported(AGCN_TCONV_FWD, taps, stride, pad))
    return agcn_bf16_tconv_fwd(x, w, bias, y, stats_part, workspace, workspace_bytes, N, Cin, Cout, T, V, taps, stride, pad,
                               agcn_gemm_precision(), s, nullptr, 0, x_absmax, nullptr, dry);
  Problem p = {};
  p.dry = dry;
  p.w = w; p.ws = workspace; p.ws_bytes = workspace_bytes;
  ConvGemmArgs& a = p.a;
  a.in = x; a.bias = bias; a.out = y; a.stats = stats_part;
  a.N = N; a.V = V;
  const TconvPlan plan = tconv_plan_fwd(T, taps, stride, pad);
  tconv_fill(p, plan, plan.pass[0], Cin, Cout);
  const bool legacy = agcn_tconv_legacy(taps, stride, pad);
  return dispatch_taps(taps, [&](auto K) { return tconv_f32_launch<decltype(K)::value>(p, legacy, false, s); });
}

// y = act( bias + tconv(x * gate) [+ res] ): the same ladder with one epilogue (epilogue.h); a window too long for the
// split kernels' LDS is refused there before anything is launched and runs on the exact kernel
int tconv_infer_route(const float* x, const float* w, const float* bias, const float* a_s, const float* a_t,
                      const float* a_c, const float* res, int relu, float* y, void* workspace, size_t workspace_bytes,
                      int N, int Cin, int Cout, int T, int V, int taps, int stride, int pad, const float* x_absmax,
                      hipStream_t s, AgcnDryRun* dry) {
  if (!agcn_tconv_domain(T, taps, stride, pad)) return AGCN_ERR_UNSUPPORTED;
  GateArgs gate = {a_s, a_t, a_c};
  if (agcn_gemm_precision() != 0 && agcn_bf16_tconv_supported(AGCN_TCONV_FWD, taps, stride, pad)) {
    const int rc = agcn_bf16_tconv_fwd(x, w, bias, y, nullptr, workspace, workspace_bytes, N, Cin, Cout, T, V, taps, stride,
                                       pad, agcn_gemm_precision(), s, res, relu, x_absmax, &gate, dry);
    if (rc != AGCN_ERR_UNSUPPORTED) return rc;
  }
  Problem p = {};
  p.dry = dry;
  p.w = w; p.ws = workspace; p.ws_bytes = workspace_bytes;
  ConvGemmArgs& a = p.a;
  a.in = x; a.bias = bias; a.out = y; a.add1 = res;
  p.gate = gate; p.gated = (a_s || a_t || a_c) ? 1 : 0; p.relu = relu;
  a.N = N; a.V = V;
  const TconvPlan plan = tconv_plan_fwd(T, taps, stride, pad);
  tconv_fill(p, plan, plan.pass[0], Cin, Cout);
  return dispatch_taps(taps, [&](auto K) { return tconv_f32_infer_launch<decltype(K)::value>(p, s); });
}

// dx[n][c][t,v] (+)= sum_{o,k: (t + pad - k) = stride*tau} w[o][c][k] dy[n][o][tau, v]  (+ masked addends): one stride-1
// pass per output-frame residue (tconv_plan_bwd_data); frames no window reaches get 0 (+ addends)
int tconv_bwd_data_route(const float* dy, const float* w, float* dx, int accumulate, const float* add1,
                         const float* mask1, const float* add2, const float* mask2, void* workspace,
                         size_t workspace_bytes, int N, int Cin, int Cout, int T, int V, int taps, int stride, int pad,
                         const float* dy_absmax, hipStream_t s, AgcnDryRun* dry) {
  if (!agcn_tconv_domain(T, taps, stride, pad)) return AGCN_ERR_UNSUPPORTED;
  // the 1x1 is measured 10-17% faster on the split-bf16 kernel at these widths, in the chained modes
  if (agcn_gemm_precision() != 0 && agcn_bf16_tconv_supported(AGCN_TCONV_BWD_DATA, taps, stride, pad) &&
      (taps > 1 || (agcn_chained() && Cin >= 64 && Cout >= 32)))
    return agcn_bf16_tconv_bwd_data(dy, w, dx, accumulate, add1, mask1, add2, mask2, workspace, workspace_bytes, N, Cin,
                                    Cout, T, V, taps, stride, pad, agcn_gemm_precision(), s, dy_absmax, dry);
  Problem p = {};
  p.dry = dry;
  p.w = w; p.ws = workspace; p.ws_bytes = workspace_bytes;
  ConvGemmArgs& a = p.a;
  a.in = dy; a.out = dx; a.accumulate = accumulate;
  a.add1 = add1; a.mask1 = mask1; a.add2 = add2; a.mask2 = mask2;
  a.N = N; a.V = V;
  const TconvPlan plan = tconv_plan_bwd_data(T, taps, stride, pad);
  const bool legacy = agcn_tconv_legacy(taps, stride, pad);
  for (int i = 0; i < plan.npasses; ++i) {
    tconv_fill(p, plan, plan.pass[i], Cin, Cout);
    const int rc = dispatch_taps(plan.pass[i].taps,
                                 [&](auto K) { return tconv_f32_launch<decltype(K)::value>(p, legacy, true, s); });
    if (rc) return rc;
  }
  return AGCN_OK;
}

}  // namespace

extern "C" {

// frames per tile / tiles per sample used by the stats-partial layout of the conv kernels
int agcn_conv_tile_frames(int V, int T_out) {
  int tt = 256 / V;
  return tt > T_out ? T_out : tt;
}
// diagnostic: kernel instantiation the calling thread's last contraction launch used ("" if none)
const char* agcn_last_kernel(void) { return agcn_last_kernel_buf; }
// "bf16x6" | "f32" | "bf16x3": the arithmetic of the channel contractions, fixed per process by AGCN_GEMM
const char* agcn_gemm_mode(void) {
  const int m = agcn_gemm_precision();
  return m == 3 ? "bf16x6" : (m == 0 ? "f32" : (m == 1 ? "bf16" : "bf16x3"));
}
// *out = max |x| over n floats: the streaming pass the f16x3 kernels run themselves when no producer supplied the maximum
int agcn_absmax(const float* x, long n, float* out, void* stream) {
  if (!x || !out || n <= 0) return AGCN_ERR_ARG;
  return agcn_launch_absmax(x, n, reinterpret_cast<unsigned*>(out), (hipStream_t)stream);
}
// arithmetic of unit_gcn's aggregate+project chain (forward and backward-data): "f16x3" in the default fp32-equivalent
// mode (AGCN_CHAIN_F16X3=0: "bf16x6"), else AGCN_GEMM's mode
const char* agcn_chain_mode(void) { return agcn_chain_f16x3() ? "f16x3" : agcn_gemm_mode(); }
int agcn_conv_num_tiles(int V, int T_out) {
  int tt = agcn_conv_tile_frames(V, T_out);
  return (T_out + tt - 1) / tt;
}

// ---- size queries: dry runs of the launches they size (agcn_common.h).  Per-sample counts run with N = 1; a shape the
// launch refuses has no slots; a workspace query serving several operations returns the largest of their dry runs,
// plus 256 bytes of slack (the f16x3 temporal convolutions park the operand maximum in the workspace tail). ----

// slots per sample of the (sum, sumsq) partials agcn_tconv_fwd writes for these sizes
int agcn_tconv_stats_tiles(int Cin, int Cout, int T_out, int V, int taps, int stride, int pad) {
  if (!agcn_sizes_ok(1, Cin, Cout, T_out, V)) return 0;
  AgcnDryRun d = {};
  const int T = (T_out - 1) * stride + taps - 2 * pad;       // a source length with T_out output frames
  if (T <= 0 || tconv_fwd_route(nullptr, nullptr, nullptr, nullptr, agcn_dry_present(), nullptr, 0, 1, Cin, Cout, T, V, taps,
                                stride, pad, nullptr, nullptr, &d))
    return 0;
  return (int)d.slab_slots;
}
// same for agcn_conv_fwd (taps 1 or 9, padding (taps-1)/2, stride 1 or 2)
int agcn_conv_stats_tiles(int Cin, int Cout, int T_out, int V, int taps, int stride) {
  if (!agcn_tconv_legacy(taps, stride, (taps - 1) / 2)) return 0;
  return agcn_tconv_stats_tiles(Cin, Cout, T_out, V, taps, stride, (taps - 1) / 2);
}
// slots per (sample, subset) of the adjacency-gradient partials agcn_gcn_dadj writes (its tiling does not depend on Cout)
int agcn_dadj_num_slots(int C, int V, int T) {
  if (!agcn_sizes_ok(1, C, C, T, V)) return 0;
  AgcnDryRun d = {};
  if (gcn_dadj_route(nullptr, nullptr, nullptr, agcn_dry_present(), nullptr, 0, 1, C, C, T, V, nullptr, nullptr, nullptr, &d))
    return 0;
  return (int)(d.slab_slots / 3);
}

// bytes of workspace (packed weight images) agcn_tconv_fwd, agcn_tconv_bwd_data and agcn_tconv_infer need
size_t agcn_tconv_workspace(int Cin, int Cout, int T, int V, int taps, int stride, int pad) {
  AgcnDryRun d = {};
  if (agcn_sizes_ok(1, Cin, Cout, T, V)) {
    tconv_fwd_route(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, Cin, Cout, T, V, taps, stride, pad, nullptr,
                    nullptr, &d);
    tconv_bwd_data_route(nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, Cin, Cout, T, V,
                         taps, stride, pad, nullptr, nullptr, &d);
    // ungated and gated: the gate image takes LDS, which can move a shape down the ladder (placeholders, as for a slab)
    for (const float* g : {(const float*)nullptr, (const float*)agcn_dry_present()})
      tconv_infer_route(nullptr, nullptr, nullptr, g, g, g, nullptr, 0, nullptr, nullptr, 0, 1, Cin, Cout, T, V, taps,
                        stride, pad, nullptr, nullptr, &d);
  }
  return d.ws_bytes + 256;
}
// same for agcn_conv_fwd / agcn_conv_bwd_data / agcn_conv9_infer (the shapes they cover)
size_t agcn_conv_workspace(int Cin, int Cout, int T, int V, int taps, int stride) {
  if (!agcn_tconv_legacy(taps, stride, (taps - 1) / 2)) return 256;
  return agcn_tconv_workspace(Cin, Cout, T, V, taps, stride, (taps - 1) / 2);
}
// aggregate+project forward, backward-data (with room for the fused theta/phi term of 6*(Cout/4) channels) and dadj
size_t agcn_gcn_workspace(int C, int Cout, int T, int V) {
  AgcnDryRun d = {};
  if (agcn_sizes_ok(1, C, Cout, T, V)) {
    gcn_fwd_route(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, C, Cout, T, V, nullptr, nullptr, &d);
    gcn_bwd_data_route(nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0,
                       nullptr, 0, 1, C, Cout, T, V, nullptr, nullptr, nullptr, &d);
    const int K2 = 6 * (Cout / 4);
    if (K2 > 0)      // (a null operand means "no fused term": the dry run names them by a placeholder)
      gcn_bwd_data_route(nullptr, nullptr, nullptr, agcn_dry_present(), agcn_dry_present(), K2, nullptr, 0, nullptr, nullptr,
                         nullptr, nullptr, 0, nullptr, 0, 1, C, Cout, T, V, nullptr, nullptr, nullptr, &d);
    gcn_dadj_route(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, C, Cout, T, V, nullptr, nullptr, nullptr, &d);
  }
  return d.ws_bytes + 256;
}

// slots per sample of the (sum, sumsq) partials of the TILE-PER-WORKGROUP aggregate+project kernels.  No caller: the
// persistent kernel's count depends on N, which this signature cannot describe, so it is not a dry run and keeps the
// values it always returned.  What a caller allocates is agcn_gcn_stats_slots.
int agcn_gcn_stats_tiles(int C, int Cout, int T, int V) {
  if (agcn_chained() && C >= 32 && agcn_gcn_chain_supported(Cout, C, V)) return agcn_gcn_chain_tiles(T);
  return agcn_conv_num_tiles(V, T);
}

// total slots (all samples) agcn_gcn_aggregate_project_fwd writes: what the caller allocates (the persistent chain kernel
// writes one slot per (sample, frame split), whose count depends on N)
int agcn_gcn_stats_slots(int N, int C, int Cout, int T, int V) {
  if (!agcn_sizes_ok(N, C, Cout, T, V)) return 0;
  AgcnDryRun d = {};
  if (gcn_fwd_route(nullptr, nullptr, nullptr, nullptr, nullptr, agcn_dry_present(), nullptr, 0, N, C, Cout, T, V, nullptr,
                    nullptr, &d))
    return 0;
  return (int)d.slab_slots;
}

int agcn_conv_fwd(const float* x, const float* w, const float* bias, float* y, float* stats_part, void* workspace,
                  size_t workspace_bytes, int N, int Cin, int Cout, int T, int V, int taps, int stride,
                  void* stream) {
  return agcn_conv_fwd_ex(x, w, bias, y, stats_part, workspace, workspace_bytes, N, Cin, Cout, T, V, taps, stride, nullptr,
                          stream);
}

// same; x_absmax (optional): device scalar max |x| left by agcn_bn_act_fwd_ex when it produced x -- saves the split-fp16
// temporal convolution its own pass over x for the range scale
int agcn_conv_fwd_ex(const float* x, const float* w, const float* bias, float* y, float* stats_part, void* workspace,
                     size_t workspace_bytes, int N, int Cin, int Cout, int T, int V, int taps, int stride,
                     const float* x_absmax, void* stream) {
  if (!x || !w || !y || !workspace || !agcn_sizes_ok(N, Cin, Cout, T, V)) return AGCN_ERR_ARG;
  if (!agcn_tconv_legacy(taps, stride, (taps - 1) / 2)) return AGCN_ERR_UNSUPPORTED;
  return tconv_fwd_route(x, w, bias, y, stats_part, workspace, workspace_bytes, N, Cin, Cout, T, V, taps, stride,
                         (taps - 1) / 2, x_absmax, (hipStream_t)stream, nullptr);
}

int agcn_conv_bwd_data(const float* dy, const float* w, float* dx, int accumulate, const float* add1,
                       const float* mask1, const float* add2, const float* mask2, void* workspace,
                       size_t workspace_bytes, int N, int Cin, int Cout, int T, int V, int taps, int stride,
                       void* stream) {
  return agcn_conv_bwd_data_ex(dy, w, dx, accumulate, add1, mask1, add2, mask2, workspace, workspace_bytes, N, Cin, Cout, T,
                               V, taps, stride, nullptr, stream);
}

// same; dy_absmax (optional): device scalar max |dy| left by agcn_bn_bwd_apply_ex
int agcn_conv_bwd_data_ex(const float* dy, const float* w, float* dx, int accumulate, const float* add1,
                          const float* mask1, const float* add2, const float* mask2, void* workspace,
                          size_t workspace_bytes, int N, int Cin, int Cout, int T, int V, int taps, int stride,
                          const float* dy_absmax, void* stream) {
  if (!dy || !w || !dx || !workspace || !agcn_sizes_ok(N, Cin, Cout, T, V)) return AGCN_ERR_ARG;
  if (!agcn_tconv_legacy(taps, stride, (taps - 1) / 2)) return AGCN_ERR_UNSUPPORTED;
  return tconv_bwd_data_route(dy, w, dx, accumulate, add1, mask1, add2, mask2, workspace, workspace_bytes, N, Cin, Cout, T,
                              V, taps, stride, (taps - 1) / 2, dy_absmax, (hipStream_t)stream, nullptr);
}

int agcn_gcn_aggregate_project_fwd(const float* x, const float* adj, const float* wcat, const float* bias, float* y,
                                   float* stats_part, void* workspace, size_t workspace_bytes, int N, int C, int Cout,
                                   int T, int V, void* stream) {
  return agcn_gcn_aggregate_project_fwd_ex(x, adj, wcat, bias, y, stats_part, workspace, workspace_bytes, N, C, Cout, T, V,
                                           nullptr, stream);
}
// x_absmax: device scalar max |x| left behind by the kernel that produced x (agcn_bn_act_fwd_ex), for the range scale
// of the f16x3 chain; null: the chain takes it with a streaming pass of its own
int agcn_gcn_aggregate_project_fwd_ex(const float* x, const float* adj, const float* wcat, const float* bias, float* y,
                                      float* stats_part, void* workspace, size_t workspace_bytes, int N, int C, int Cout,
                                      int T, int V, const float* x_absmax, void* stream) {
  if (!x || !adj || !wcat || !y || !workspace || !agcn_sizes_ok(N, C, Cout, T, V)) return AGCN_ERR_ARG;
  return gcn_fwd_route(x, adj, wcat, bias, y, stats_part, workspace, workspace_bytes, N, C, Cout, T, V, x_absmax,
                       (hipStream_t)stream, nullptr);
}

// ---- BN-folded inference (eval mode): the BatchNorm that follows a contraction is folded into its weights and bias
// by the caller; the residual add and the ReLU ride in the store epilogue, so a unit is adjacency + two kernels ----
// y = act( bias + sum_i W_i (x . adj_i) [+ res] [+ W2 . x2] ),  W2 (Cout, K2) row-major (a folded 1x1 `down` conv on x2)
// Only on the chained split-bf16 path (C >= 32): AGCN_ERR_UNSUPPORTED otherwise (the caller runs the unfused passes).
int agcn_gcn_unit_infer(const float* x, const float* adj, const float* wcat, const float* bias, const float* res,
                        const float* x2, const float* w2, int K2, int relu, float* y, void* workspace,
                        size_t workspace_bytes, int N, int C, int Cout, int T, int V, void* stream) {
  if (!x || !adj || !wcat || !y || !workspace || !agcn_sizes_ok(N, C, Cout, T, V)) return AGCN_ERR_ARG;
  if ((x2 == nullptr) != (w2 == nullptr) || (x2 && K2 <= 0)) return AGCN_ERR_ARG;
  return gcn_unit_infer_route(x, adj, wcat, bias, res, x2, w2, K2, relu, y, workspace, workspace_bytes, N, C, Cout, T, V,
                              (hipStream_t)stream, nullptr);
}

size_t agcn_gcn_unit_infer_workspace(int C, int Cout, int K2, int T, int V) {
  AgcnDryRun d = {};
  const float* x2 = K2 > 0 ? agcn_dry_present() : nullptr;
  if (agcn_sizes_ok(1, C, Cout, T, V))
    gcn_unit_infer_route(nullptr, nullptr, nullptr, nullptr, nullptr, x2, x2, K2, 0, nullptr, nullptr, 0, 1, C, Cout, T, V,
                         nullptr, &d);
  return d.ws_bytes + 256;
}

// y = act( bias + conv9x1(x; w, stride) [+ res] ),  res (N, Cout, T_out, V).  Split-bf16 modes only.
int agcn_conv9_infer(const float* x, const float* w, const float* bias, const float* res, int relu, float* y,
                     void* workspace, size_t workspace_bytes, int N, int Cin, int Cout, int T, int V, int stride,
                     void* stream) {
  if (!x || !w || !y || !workspace || !agcn_sizes_ok(N, Cin, Cout, T, V)) return AGCN_ERR_ARG;
  if (stride != 1 && stride != 2) return AGCN_ERR_UNSUPPORTED;
  if (agcn_gemm_precision() == 0) return AGCN_ERR_UNSUPPORTED;
  return agcn_bf16_tconv_fwd(x, w, bias, y, nullptr, workspace, workspace_bytes, N, Cin, Cout, T, V, 9, stride, 4,
                             agcn_gemm_precision(), (hipStream_t)stream, res, relu, nullptr, nullptr, nullptr);
}

int agcn_gcn_aggregate_project_bwd_data(const float* dy, const float* adj, const float* wcat, float* dx,
                                        int accumulate, const float* add1, const float* mask1, const float* add2,
                                        const float* mask2, int mask_bits, void* workspace, size_t workspace_bytes,
                                        int N, int C, int Cout, int T, int V, void* stream) {
  return agcn_gcn_aggregate_project_bwd_data_ex(dy, adj, wcat, nullptr, nullptr, 0, dx, accumulate, add1, mask1, add2,
                                                mask2, mask_bits, workspace, workspace_bytes, N, C, Cout, T, V, nullptr,
                                                nullptr, stream);
}
// Both backward-data forms behind one entry point (dtp null: the plain one; else the fused 1x1 term as in
// agcn_gcn_aggregate_project_bwd_data_fused), with the device scalars max |dy| / max |dtp| their producers left behind
// (agcn_bn_bwd_apply_ex; null: the f16x3 chain takes them with a streaming pass of its own).
int agcn_gcn_aggregate_project_bwd_data_ex(const float* dy, const float* adj, const float* wcat, const float* dtp,
                                           const float* w2, int K2, float* dx, int accumulate, const float* add1,
                                           const float* mask1, const float* add2, const float* mask2, int mask_bits,
                                           void* workspace, size_t workspace_bytes, int N, int C, int Cout, int T, int V,
                                           const float* dy_absmax, const float* dtp_absmax, void* stream) {
  if (!dy || !adj || !wcat || !dx || !workspace || !agcn_sizes_ok(N, C, Cout, T, V)) return AGCN_ERR_ARG;
  if (dtp && (!w2 || K2 <= 0)) return AGCN_ERR_ARG;
  return gcn_bwd_data_route(dy, adj, wcat, dtp, w2, K2, dx, accumulate, add1, mask1, add2, mask2, mask_bits, workspace,
                            workspace_bytes, N, C, Cout, T, V, dy_absmax, dtp_absmax, (hipStream_t)stream, nullptr);
}

// Same, plus the 1x1 term of the adaptive branch in one pass:  dx (+)= ... + W2^T dtp  with dtp (N, K2, T, V) and
// w2 (K2, C) row-major (the stacked conv_a/conv_b weights).  Only on the chained (bf16x6) path: check
// agcn_gcn_bwd_data_fused_supported first.
int agcn_gcn_bwd_data_fused_supported(int C, int Cout, int V) {
  return agcn_chained() && agcn_gcn_chain_supported(C, Cout, V) ? 1 : 0;
}
int agcn_gcn_aggregate_project_bwd_data_fused(const float* dy, const float* adj, const float* wcat, const float* dtp,
                                              const float* w2, int K2, float* dx, int accumulate, const float* add1,
                                              const float* mask1, const float* add2, const float* mask2, int mask_bits,
                                              void* workspace, size_t workspace_bytes, int N, int C, int Cout, int T,
                                              int V, void* stream) {
  if (!dtp) return AGCN_ERR_ARG;
  return agcn_gcn_aggregate_project_bwd_data_ex(dy, adj, wcat, dtp, w2, K2, dx, accumulate, add1, mask1, add2, mask2,
                                                mask_bits, workspace, workspace_bytes, N, C, Cout, T, V, nullptr, nullptr,
                                                stream);
}

int agcn_gcn_dadj(const float* dy, const float* wcat, const float* x, float* dadj_part, void* workspace,
                  size_t workspace_bytes, int N, int C, int Cout, int T, int V, void* stream) {
  return agcn_gcn_dadj_ex(dy, wcat, x, dadj_part, workspace, workspace_bytes, N, C, Cout, T, V, nullptr, nullptr, stream);
}
// dy_absmax: device scalar max |dy| (agcn_bn_bwd_apply_ex) for the f16x3 projection; null: a streaming pass inside.
// x_absmax: device scalar max |x| (kept by the forward) for the f16x3 reduction against x; null: a streaming pass inside
int agcn_gcn_dadj_ex(const float* dy, const float* wcat, const float* x, float* dadj_part, void* workspace,
                     size_t workspace_bytes, int N, int C, int Cout, int T, int V, const float* dy_absmax,
                     const float* x_absmax, void* stream) {
  if (!dy || !wcat || !x || !dadj_part || !workspace || !agcn_sizes_ok(N, C, Cout, T, V)) return AGCN_ERR_ARG;
  return gcn_dadj_route(dy, wcat, x, dadj_part, workspace, workspace_bytes, N, C, Cout, T, V, dy_absmax, x_absmax,
                        (hipStream_t)stream, nullptr);
}


// ---- temporal convolution with explicit padding (reference aagcn.py:184-207 TCNUnit(kernel_size, stride, pad),
// agcn.py:36-50 unit_tcn(kernel_size, stride)): taps 1..9, stride 1..9, pad 0..(taps-1)/2 ----
int agcn_tconv_fwd(const float* x, const float* w, const float* bias, float* y, float* stats_part, void* workspace,
                   size_t workspace_bytes, int N, int Cin, int Cout, int T, int V, int taps, int stride, int pad,
                   const float* x_absmax, void* stream) {
  if (!x || !w || !y || !workspace || !agcn_sizes_ok(N, Cin, Cout, T, V)) return AGCN_ERR_ARG;
  return tconv_fwd_route(x, w, bias, y, stats_part, workspace, workspace_bytes, N, Cin, Cout, T, V, taps, stride, pad,
                         x_absmax, (hipStream_t)stream, nullptr);
}

// BN-folded inference form (eval mode; reference aagcn.py:264-271 gates, :194-201 TCNUnit, :316-321 unit tail):
//   y = act( bias + tconv(x * gate ; w, stride, pad) [+ res] ),   gate[n,c,t,v] = a_s[n,v] * a_t[n,t] * a_c[n,c]
// The caller has folded the BatchNorm into w and bias.  a_s (N,V), a_t (N,T), a_c (N,Cin): each optional, null = ones;
// they multiply x where its tile is staged for the matrix cores (gate.h), so the gated tensor is never stored.  res
// (N, Cout, T_out, V) or null; x_absmax: optional device scalar max |x| (of the UNGATED x) for the f16x3 range scale.
// Same domain and workspace as agcn_tconv_fwd.  As everywhere, it is the launcher that compares its need with
// workspace_bytes (AGCN_ERR_WORKSPACE): there is no separate comparison with the query's answer up front.
int agcn_tconv_infer(const float* x, const float* w, const float* bias, const float* a_s, const float* a_t,
                     const float* a_c, const float* res, int relu, float* y, void* workspace, size_t workspace_bytes,
                     int N, int Cin, int Cout, int T, int V, int taps, int stride, int pad, const float* x_absmax,
                     void* stream) {
  if (!x || !w || !y || !workspace || !agcn_sizes_ok(N, Cin, Cout, T, V)) return AGCN_ERR_ARG;
  return tconv_infer_route(x, w, bias, a_s, a_t, a_c, res, relu, y, workspace, workspace_bytes, N, Cin, Cout, T, V, taps,
                           stride, pad, x_absmax, (hipStream_t)stream, nullptr);
}

int agcn_tconv_bwd_data(const float* dy, const float* w, float* dx, int accumulate, const float* add1,
                        const float* mask1, const float* add2, const float* mask2, void* workspace,
                        size_t workspace_bytes, int N, int Cin, int Cout, int T, int V, int taps, int stride, int pad,
                        const float* dy_absmax, void* stream) {
  if (!dy || !w || !dx || !workspace || !agcn_sizes_ok(N, Cin, Cout, T, V)) return AGCN_ERR_ARG;
  return tconv_bwd_data_route(dy, w, dx, accumulate, add1, mask1, add2, mask2, workspace, workspace_bytes, N, Cin, Cout, T,
                              V, taps, stride, pad, dy_absmax, (hipStream_t)stream, nullptr);
}

}  // extern "C"
