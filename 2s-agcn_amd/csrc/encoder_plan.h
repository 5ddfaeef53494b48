// Tile geometry and index arithmetic of the transformer-encoder kernels (encoder.hip): rows per workgroup, key-block
// size, LDS layout and bytes, grids, and every offset the kernels form into LDS and into the tensors they are given.
// Plain C++17 without HIP: encoder.hip includes it for the launchers AND the kernels (ENC_HD), and
// tests/encoder_plan_check.cpp compiles it with the host compiler and sweeps the whole domain.
#pragma once

#if defined(__HIPCC__)
#define ENC_HD __host__ __device__ __forceinline__
#else
#define ENC_HD static inline
#endif

// domain of the attention core
#define ENC_MAX_L 640          // tokens (the positional table has 601 rows)
#define ENC_MAX_DH 256         // head width
#define ENC_MAX_D 2048         // model width H*dh, and rows of LayerNorm
#define ENC_LDS_LIMIT (160 * 1024)

#define ENC_THREADS 256
#define ENC_ROWS 16            // query rows (forward, backward A) or key rows (backward B) of one workgroup
#define ENC_KB 32              // rows of the K / V / Q / dctx block staged in LDS at a time
#define ENC_NI 16              // most output elements per thread of the (ENC_ROWS x dh) tile: ENC_ROWS*ENC_MAX_DH/ENC_THREADS

ENC_HD bool enc_mha_domain(int N, int L, int H, int dh) {
  return N >= 1 && L >= 1 && L <= ENC_MAX_L && H >= 1 && dh >= 1 && dh <= ENC_MAX_DH && (long)H * dh <= ENC_MAX_D;
}

// LDS of one workgroup, in floats: A (ENC_ROWS x ap) the row tile, B (ENC_KB x bp) the staged block, S (ENC_ROWS x sp)
// the score / probability rows over all L keys (sp - 4 = nkb*ENC_KB columns are written, those past L with zeros).
// dh is zero-padded to a multiple of 4 (the width of a 16-byte LDS read, and the K step of v_mfma_f32_16x16x4_f32,
// should the products move there).  Every row starts 16-byte aligned; bp/4 is odd, so the 16-byte reads of 16
// consecutive B rows at one column fall into 16 different bank quads.
//
// The (ENC_ROWS x dh) output tile of tile_apply: thread t owns column d = t % dw of the rpt rows rg*rpt .. rg*rpt+rpt-1,
// rg = t / dw; dw = the power of two >= dh, rg < ngroups = min(ENC_ROWS, ENC_THREADS/dw), rpt = ENC_ROWS/ngroups.
struct EncMhaPlan {
  int L, dh;
  int nrb;                     // row blocks: ceil(L / ENC_ROWS)
  int nkb;                     // key blocks: ceil(L / ENC_KB)
  int dhp, ap, bp, sp;
  int a_off, b_off, s_off;     // float offsets of the three regions
  int lds_floats;
  int dw, ngroups, rpt;        // rpt <= ENC_NI
};

ENC_HD EncMhaPlan enc_mha_plan(int L, int dh) {
  EncMhaPlan p;
  p.L = L; p.dh = dh;
  p.nrb = (L + ENC_ROWS - 1) / ENC_ROWS;
  p.nkb = (L + ENC_KB - 1) / ENC_KB;
  p.dhp = (dh + 3) & ~3;
  p.ap = p.dhp;
  p.bp = p.dhp + (((p.dhp >> 2) & 1) ? 8 : 4);
  p.sp = p.nkb * ENC_KB + 4;
  p.a_off = 0;
  p.b_off = p.a_off + ENC_ROWS * p.ap;
  p.s_off = p.b_off + ENC_KB * p.bp;
  p.lds_floats = p.s_off + ENC_ROWS * p.sp;
  p.dw = 1;
  while (p.dw < dh) p.dw <<= 1;
  p.ngroups = ENC_THREADS / p.dw < ENC_ROWS ? ENC_THREADS / p.dw : ENC_ROWS;
  p.rpt = ENC_ROWS / p.ngroups;
  return p;
}
ENC_HD long enc_mha_lds_bytes(const EncMhaPlan& p) { return (long)p.lds_floats * 4; }

// LDS offsets (floats, from the start of the dynamic LDS)
ENC_HD int enc_lds_a(const EncMhaPlan& p, int r, int d) { return p.a_off + r * p.ap + d; }      // r < ENC_ROWS, d < dhp
ENC_HD int enc_lds_b(const EncMhaPlan& p, int j, int d) { return p.b_off + j * p.bp + d; }      // j < ENC_KB, d < dhp
ENC_HD int enc_lds_s(const EncMhaPlan& p, int r, int j) { return p.s_off + r * p.sp + j; }      // r < ENC_ROWS, j < sp

// tensor offsets (floats / bytes of the uint8 tensors)
//   qkv (N, L, 3D): part 0 q, 1 k, 2 v; head h at columns [h*dh, (h+1)*dh)
ENC_HD long enc_qkv_index(int n, int l, int part, int h, int d, int L, int H, int dh) {
  return ((long)n * L + l) * (3L * H * dh) + (long)part * H * dh + (long)h * dh + d;
}
ENC_HD long enc_ctx_index(int n, int l, int h, int d, int L, int H, int dh) {
  return ((long)n * L + l) * ((long)H * dh) + (long)h * dh + d;
}
ENC_HD long enc_prob_index(int n, int h, int i, int j, int L, int H) { return (((long)n * H + h) * L + i) * L + j; }
ENC_HD long enc_avg_index(int n, int i, int j, int L) { return ((long)n * L + i) * L + j; }
ENC_HD long enc_null_index(int n, int l, int L) { return (long)n * L + l; }

// mask of the logits: both tokens null (frame mask), or the causal side the caller asked for
ENC_HD bool enc_allowed(int i, int j, int causal, bool null_i, bool null_j) {
  if (null_i && null_j) return false;
  if (causal == 1) return j <= i;
  if (causal == 2) return j >= i;
  return true;
}

// bytes of the dS scratch agcn_mha_bwd needs (one float per probability)
ENC_HD long enc_mha_bwd_ws_bytes(int N, int L, int H) { return (long)N * H * L * L * 4; }

// ---- LayerNorm over rows of D ----
// forward: one workgroup normalises one row at a time, thread t owns columns t + k*ENC_THREADS;
// backward: one wave per row (no workgroup barrier), lane l owns columns l + 64*k; wave w of the grid owns the rows
// [w*rows_per_wave, min(R, (w+1)*rows_per_wave)) and slot w of the (dgamma, dbeta) partial slab.
#define ENC_LN_PER_THREAD (ENC_MAX_D / ENC_THREADS)     // 8
#define ENC_LN_PER_LANE (ENC_MAX_D / 64)                // 32
#define ENC_LN_WAVES (ENC_THREADS / 64)                 // waves of a workgroup
#define ENC_LN_MAX_WAVES 1024                           // backward: most waves that own rows
ENC_HD bool enc_ln_domain(long R, int D) { return R >= 1 && R <= 0x7fffffffL / ENC_MAX_D && D >= 1 && D <= ENC_MAX_D; }
struct EncLnPlan {
  int nblocks;                 // backward workgroups
  int nslots;                  // nblocks * ENC_LN_WAVES rows of the slab (waves past the last row write zeros)
  int rows_per_wave;
};
ENC_HD EncLnPlan enc_ln_plan(long R) {
  EncLnPlan p;
  p.rows_per_wave = (int)((R + ENC_LN_MAX_WAVES - 1) / ENC_LN_MAX_WAVES);
  const int nwaves = (int)((R + p.rows_per_wave - 1) / p.rows_per_wave);
  p.nblocks = (nwaves + ENC_LN_WAVES - 1) / ENC_LN_WAVES;
  p.nslots = p.nblocks * ENC_LN_WAVES;
  return p;
}
// slab [nslots][2][D] (dgamma partials, dbeta partials)
ENC_HD long enc_ln_bwd_ws_bytes(long R, int D) { return (long)enc_ln_plan(R).nslots * 2 * D * 4; }

// ---- tokens: x (N*M, C, T', V) <-> tok (N, L, D), L = cls + M*T', D = V*C; token cls + m*T' + t, feature v*C + c ----
// One workgroup transposes TT frames of one (n, m): it reads C runs of TT*V contiguous floats and writes TT runs of
// V*C contiguous floats, through an LDS tile (C x (TT*V + pad)).
#define ENC_TOK_TILE 4096      // floats of the tile before padding
#define ENC_TOK_LDS (ENC_TOK_TILE + 2 * ENC_MAX_D)
ENC_HD bool enc_tok_domain(int N, int M, int C, int Tp, int V, int has_cls) {
  if (N < 1 || M < 1 || C < 1 || Tp < 1 || V < 1) return false;
  if ((long)V * C > ENC_MAX_D) return false;
  const long L = (long)M * Tp + (has_cls ? 1 : 0);
  return L <= ENC_MAX_L && (long)N * M * Tp <= (1L << 30);      // (the grid: frame blocks x N*M)
}
struct EncTokPlan {
  int tt;                      // frames per workgroup
  int ntb;                     // frame blocks: ceil(T' / tt)
  int w;                       // LDS row stride: tt*V rounded up to odd
  int lds_floats;              // C * w
};
ENC_HD EncTokPlan enc_tok_plan(int C, int Tp, int V) {
  EncTokPlan p;
  const int D = V * C;
  p.tt = ENC_TOK_TILE / D;
  if (p.tt < 1) p.tt = 1;
  if (p.tt > Tp) p.tt = Tp;
  p.ntb = (Tp + p.tt - 1) / p.tt;
  p.w = (p.tt * V) | 1;
  p.lds_floats = C * p.w;
  return p;
}
ENC_HD long enc_x_index(int nm, int c, int t, int v, int C, int Tp, int V) { return (((long)nm * C + c) * Tp + t) * V + v; }
ENC_HD long enc_tok_index(int n, int l, int f, int L, int D) { return ((long)n * L + l) * D + f; }

// ---- additive attention bias (aagcn_v24): bias (Hb, L, L), Hb = 1 (shared by the heads) or H (one slice per head) ----
ENC_HD bool enc_bias_heads_ok(int Hb, int H) { return Hb == 1 || Hb == H; }
ENC_HD long enc_bias_index(int h, int i, int j, int L, int Hb) { return (((long)(Hb == 1 ? 0 : h)) * L + i) * L + j; }

// ---- sums over sequences (the bias gradient, dcls / dpe of the spatial tokens), two stages ----
// Stage 1: slot b holds the sum over the sequences [b*ENC_SEQ_CHUNK, min(S, (b+1)*ENC_SEQ_CHUNK)), ascending, of every
// column; stage 2 (enc_slab_sum_kernel) adds the slots in its fixed order.  ENC_SEQ_CHUNK = 32 sequences per slot.
#define ENC_SEQ_CHUNK 32
#define ENC_SEQ_MAX_W (1L << 28)        // most columns of a slab (an int column index, W + 16 without overflow)
#define ENC_SEQ_MAX_SLOTS 65535         // the slots are the y dimension of stage 1's grid: at most 2 097 120 sequences
ENC_HD long enc_seq_slots(long S) { return (S + ENC_SEQ_CHUNK - 1) / ENC_SEQ_CHUNK; }
ENC_HD long enc_seq_slab_index(long slot, long col, long W) { return slot * W + col; }

// dbias[hb, i, j] = sum_n (sum_h when Hb = 1) dS[n, h, i, j]: n ascending, h ascending inside n; slab [slots][Hb*L*L]
ENC_HD bool enc_bias_grad_domain(int N, int L, int H, int Hb) {
  return N >= 1 && L >= 1 && L <= ENC_MAX_L && H >= 1 && H <= ENC_MAX_D && enc_bias_heads_ok(Hb, H) &&
         (long)Hb * L * L <= ENC_SEQ_MAX_W && enc_seq_slots(N) <= ENC_SEQ_MAX_SLOTS;
}
ENC_HD long enc_bias_grad_ws_bytes(int N, int L, int H, int Hb) { return enc_seq_slots(N) * ((long)Hb * L * L) * 4; }

// ---- spatial tokens (aagcn_v24): x (N*M, C, T', V) <-> tok (N*T', L, C), L = cls + M*V: sequence n*T' + t, token
// cls + m*V + v, feature c.  For a fixed (n, m, t) the V*C floats of tok are contiguous, as in the temporal tokens: the
// same tile (enc_tok_plan), another outer index.  The positional row of token l is pe[l, :]. ----
ENC_HD bool enc_stok_domain(int N, int M, int C, int Tp, int V, int has_cls) {
  if (N < 1 || M < 1 || C < 1 || Tp < 1 || V < 1) return false;
  if (C > ENC_MAX_D || (long)C * (V | 1) > ENC_TOK_LDS) return false;       // one frame of the tile fits the LDS
  const long L = (long)M * V + (has_cls ? 1 : 0);
  if (L > ENC_MAX_L || L * C > ENC_SEQ_MAX_W) return false;
  return (long)N * M * Tp <= (1L << 30) && (long)N * Tp * L * C <= (1L << 40) &&
         enc_seq_slots((long)N * Tp) <= ENC_SEQ_MAX_SLOTS;
}
ENC_HD long enc_stok_index(int n, int t, int l, int c, int Tp, int L, int C) {
  return ((((long)n * Tp + t) * L) + l) * C + c;
}
// slab [slots][L*C] of the sums over the N*T' sequences
ENC_HD long enc_stok_bwd_ws_bytes(int N, int M, int C, int Tp, int V, int has_cls) {
  return enc_seq_slots((long)N * Tp) * (((long)M * V + (has_cls ? 1 : 0)) * C) * 4;
}
