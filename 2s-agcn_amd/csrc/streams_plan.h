// Index arithmetic of the bone / motion stream kernels (streams.hip), shared with the host-side checker
// tests/streams_plan_check.cpp.  Plain C++: no HIP type, nothing that needs a device.
//
// A tensor is contiguous (N, C, T, V, M).  The kernels walk it in ITEMS of W floats: W = M where one joint's M persons are
// moved as one vector (M 2 or 4, every pointer aligned to 4 M bytes), W = 1 otherwise.  Mw = M / W is the number of items
// per joint (1 on the vector path, M on the scalar path), so item i is
//     mw = i % Mw,  v = (i / Mw) % V,  t = (i / (Mw V)) % T,  and (n, c) = i / (Mw V T).
// The neighbours of an item lie at item offsets (parent[v] - v) Mw (the parent joint of the same frame) and V Mw (the
// same joint of the next frame).
//
// The parent table never lives in device memory: the C entries take it as a HOST array, validate it on the host at every
// call (agcn_stream_table_ok) and copy it into AgcnStreamTable, which the kernels receive BY VALUE in their arguments.
// No index is ever read from a tensor.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AGCN_STREAM_HD __host__ __device__ __forceinline__
#define AGCN_STREAM_UNROLL _Pragma("unroll")
#else
#define AGCN_STREAM_HD inline
#define AGCN_STREAM_UNROLL
#endif

#define AGCN_STREAM_MAX_V 32

struct AgcnStreamTable {
  int parent[AGCN_STREAM_MAX_V];   // entries at and behind V are 0
};

// 1 <= V <= AGCN_STREAM_MAX_V and 0 <= parent[v] < V for every joint: what makes every offset below stay in its frame
inline bool agcn_stream_table_ok(const int* parent, int V) {
  if (!parent || V < 1 || V > AGCN_STREAM_MAX_V) return false;
  for (int v = 0; v < V; ++v)
    if (parent[v] < 0 || parent[v] >= V) return false;
  return true;
}

// the vector width in floats for a tensor with M persons whose pointers are all aligned to `align_bytes`
inline int agcn_stream_width(int M, unsigned long long align_bytes) {
  return ((M == 2 || M == 4) && align_bytes % (4ull * M) == 0) ? M : 1;
}

// items of W floats in the tensor, or -1 where the element count does not fit the kernels' 32-bit index
inline long long agcn_stream_items(int N, int C, int T, int V, int M, int W) {
  const long long total = (long long)N * C * T * V * M;
  return total > 0x7fffffffLL ? -1 : total / W;
}

// workgroups of 256 threads: one item per thread up to 2048 workgroups, a grid-stride loop beyond
inline unsigned agcn_stream_grid(long long items) {
  const long long wg = (items + 255) / 256;
  return (unsigned)(wg < 1 ? 1 : (wg > 2048 ? 2048 : wg));
}

struct AgcnStreamPos {
  int v, t;
};

AGCN_STREAM_HD AgcnStreamPos agcn_stream_pos(unsigned i, int T, int V, int Mw) {
  const unsigned j = i / (unsigned)Mw;
  AgcnStreamPos p;
  p.v = (int)(j % (unsigned)V);
  p.t = (int)((j / (unsigned)V) % (unsigned)T);
  return p;
}

// parent[v] out of the by-value table without a dynamically indexed load: v is per lane, the table is uniform.  The
// result is clamped into [0, V) as well: with a table that passed agcn_stream_table_ok the clamp changes nothing.
AGCN_STREAM_HD int agcn_stream_parent(const AgcnStreamTable& tab, int v, int V) {
  int p = 0;
  AGCN_STREAM_UNROLL
  for (int c = 0; c < AGCN_STREAM_MAX_V; ++c)
    if (c == v) p = tab.parent[c];
  return p < 0 ? 0 : (p >= V ? V - 1 : p);
}

// the children of joint v as a bit mask: bit c is set iff c < V and parent[c] == v (a self-parent is its own child).  Only
// compares on the uniform table: the loads then take one step per CHILD of the lane's joint, not one per joint.
AGCN_STREAM_HD unsigned agcn_stream_children(const AgcnStreamTable& tab, int v, int V) {
  unsigned kids = 0;
  AGCN_STREAM_UNROLL
  for (int c = 0; c < AGCN_STREAM_MAX_V; ++c)
    if (c < V && tab.parent[c] == v) kids |= 1u << c;
  return kids;
}

// item offset from joint v to joint u of the same frame, and from a frame to the next
AGCN_STREAM_HD long agcn_stream_joint_offset(int v, int u, int Mw) { return (long)(u - v) * Mw; }
AGCN_STREAM_HD long agcn_stream_frame_offset(int V, int Mw) { return (long)V * Mw; }

// ---- the work of one item, as the kernels run it and as the host checker runs it ------------------------------------------
// `vec` is the value of an item (float, or a vector of W floats whose lanes never mix); In / Out are whatever is indexed
// with an item index: raw pointers in the kernels, bounds-checking views in tests/streams_plan_check.cpp.  A null
// (false) In / Out is a stream that is not wanted.

// forward: bone = a0 - b0, joint_motion = a1 - a0, bone_motion = (a1 - b1) - (a0 - b0); a = the joint, b = its parent,
// 0 = this frame, 1 = the next; the motions of the last frame are 0
template <class vec, class In, class Out>
AGCN_STREAM_HD void agcn_stream_fwd_item(In x, Out bone, Out jm, Out bm, const AgcnStreamTable& tab, unsigned i, int T,
                                         int V, int Mw) {
  const AgcnStreamPos pos = agcn_stream_pos(i, T, V, Mw);
  const bool next = pos.t + 1 < T;
  const bool want_b = bone || bm, want_m = jm || bm;
  const long foff = agcn_stream_frame_offset(V, Mw);
  const vec zero = vec();
  const vec a0 = x[(long)i];
  vec b0 = zero, a1 = zero, b1 = zero;
  long poff = 0;
  if (want_b) {
    poff = agcn_stream_joint_offset(pos.v, agcn_stream_parent(tab, pos.v, V), Mw);
    b0 = x[(long)i + poff];
  }
  if (want_m && next) {
    a1 = x[(long)i + foff];
    if (bm) b1 = x[(long)i + foff + poff];
  }
  if (bone) bone[(long)i] = a0 - b0;
  if (jm) jm[(long)i] = next ? a1 - a0 : zero;
  if (bm) bm[(long)i] = next ? (a1 - b1) - (a0 - b0) : zero;
}

// motion^T of d at item j of frame t: (t > 0 ? d[t-1] : 0) - (t < T-1 ? d[t] : 0)
template <class vec, class In>
AGCN_STREAM_HD vec agcn_stream_motion_t(In d, long j, long foff, bool prev, bool next) {
  const vec zero = vec();
  const vec lo = prev ? d[j - foff] : zero;
  const vec hi = next ? d[j] : zero;
  return lo - hi;
}

// backward, gather form: dx = wj dj + wb bone^T(db) + wjm motion^T(djm) + wbm bone^T(motion^T(dbm)), added in that order;
// bone^T(d)[v] = d[v] - sum of d[c] over the children c of v, ascending (every c < V: inside the frame)
template <class vec, class In, class Out>
AGCN_STREAM_HD void agcn_stream_bwd_item(In dj, In db, In djm, In dbm, Out dx, const AgcnStreamTable& tab, float wj,
                                         float wb, float wjm, float wbm, unsigned i, int T, int V, int Mw) {
  const AgcnStreamPos pos = agcn_stream_pos(i, T, V, Mw);
  const bool prev = pos.t > 0, next = pos.t + 1 < T;
  const long foff = agcn_stream_frame_offset(V, Mw);
  const unsigned kids = (db || dbm) ? agcn_stream_children(tab, pos.v, V) : 0u;
  vec acc = vec();
  if (dj) acc += wj * dj[(long)i];
  if (db) {
    vec s = db[(long)i];
    for (unsigned k = kids; k; k &= k - 1)      // lowest set bit first: the children ascending
      s -= db[(long)i + agcn_stream_joint_offset(pos.v, __builtin_ctz(k), Mw)];
    acc += wb * s;
  }
  if (djm) acc += wjm * agcn_stream_motion_t<vec>(djm, (long)i, foff, prev, next);
  if (dbm) {
    vec s = agcn_stream_motion_t<vec>(dbm, (long)i, foff, prev, next);
    for (unsigned k = kids; k; k &= k - 1)
      s -= agcn_stream_motion_t<vec>(dbm, (long)i + agcn_stream_joint_offset(pos.v, __builtin_ctz(k), Mw), foff, prev,
                                     next);
    acc += wbm * s;
  }
  dx[(long)i] = acc;
}
