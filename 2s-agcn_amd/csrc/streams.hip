// Bone and motion input streams of 2s-AGCN / MS-AAGCN computed from joint data on the device, and their transpose.
//
//   bone[n,c,t,v,m]   = x[n,c,t,v,m] - x[n,c,t,parent[v],m]
//   joint_motion[t]   = x[t+1] - x[t]        for t < T-1, 0 at t = T-1
//   bone_motion[t]    = bone[t+1] - bone[t]  for t < T-1, 0 at t = T-1      ((a1 - b1) - (a0 - b0), in that order)
//
// Every output element is one or two correctly rounded fp32 subtractions of loaded values in a fixed order, so the forward
// has one bit-exact answer.  The backward is the transpose in gather form: each dx element sums its own addends in a fixed
// order (the streams in the order joint, bone, joint_motion, bone_motion; the children of a joint ascending), no atomics.
//
// Memory-paced: x (or the cotangents) is read once from HBM, the neighbour reads (parent joint: same 100..200-byte frame
// row; next frame: one row on) hit L2.  One item per thread, 8 or 16 bytes per lane where M is 2 or 4; the work of an item
// is written once, in streams_plan.h, where the host checker runs the same code behind bounds-checking views.
//
// The parent table reaches the kernels by value inside their arguments (AgcnStreamTable), after the host entry has
// validated it: there is no index memory on the device and no index comes from a tensor.
#include "agcn_common.h"
#include "streams_plan.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {

template <int W> struct StreamVec;
template <> struct StreamVec<1> { typedef float type; };
template <> struct StreamVec<2> { typedef f32x2 type; };
template <> struct StreamVec<4> { typedef f32x4 type; };

template <int W>
__global__ __launch_bounds__(256) void streams_fwd_kernel(const typename StreamVec<W>::type* __restrict__ x,
                                                          typename StreamVec<W>::type* __restrict__ bone,
                                                          typename StreamVec<W>::type* __restrict__ jm,
                                                          typename StreamVec<W>::type* __restrict__ bm,
                                                          AgcnStreamTable tab, unsigned items, int T, int V, int Mw) {
  typedef typename StreamVec<W>::type vec;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < items; i += gridDim.x * 256u)
    agcn_stream_fwd_item<vec>(x, bone, jm, bm, tab, i, T, V, Mw);
}

template <int W>
__global__ __launch_bounds__(256) void streams_bwd_kernel(const typename StreamVec<W>::type* __restrict__ dj,
                                                          const typename StreamVec<W>::type* __restrict__ db,
                                                          const typename StreamVec<W>::type* __restrict__ djm,
                                                          const typename StreamVec<W>::type* __restrict__ dbm,
                                                          typename StreamVec<W>::type* __restrict__ dx, AgcnStreamTable tab,
                                                          float wj, float wb, float wjm, float wbm, unsigned items, int T,
                                                          int V, int Mw) {
  typedef typename StreamVec<W>::type vec;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < items; i += gridDim.x * 256u)
    agcn_stream_bwd_item<vec>(dj, db, djm, dbm, dx, tab, wj, wb, wjm, wbm, i, T, V, Mw);
}

// what both entries check before anything is launched; fills the by-value table and the item geometry
struct StreamLaunch {
  AgcnStreamTable tab;
  int W, Mw;
  unsigned items, grid;
};

int stream_plan(const int* host_parent, int N, int C, int T, int V, int M, unsigned long long address_bits,
                StreamLaunch* L) {
  if (!host_parent || N <= 0 || C <= 0 || T <= 0 || V <= 0 || M <= 0) return AGCN_ERR_ARG;
  if (V > AGCN_STREAM_MAX_V) return AGCN_ERR_UNSUPPORTED;
  if (!agcn_stream_table_ok(host_parent, V)) return AGCN_ERR_ARG;
  L->W = agcn_stream_width(M, address_bits);
  const long long items = agcn_stream_items(N, C, T, V, M, L->W);
  if (items < 0) return AGCN_ERR_UNSUPPORTED;
  for (int v = 0; v < AGCN_STREAM_MAX_V; ++v) L->tab.parent[v] = v < V ? host_parent[v] : 0;
  L->Mw = M / L->W;
  L->items = (unsigned)items;
  L->grid = agcn_stream_grid(items);
  return AGCN_OK;
}

inline unsigned long long bits_of(const void* p) { return (unsigned long long)(uintptr_t)p; }

template <int W>
int launch_fwd(const float* x, float* bone, float* jm, float* bm, const StreamLaunch& L, int T, int V, hipStream_t s) {
  typedef typename StreamVec<W>::type vec;
  hipLaunchKernelGGL(streams_fwd_kernel<W>, dim3(L.grid), dim3(256), 0, s, (const vec*)x, (vec*)bone, (vec*)jm, (vec*)bm,
                     L.tab, L.items, T, V, L.Mw);
  return agcn_check_launch();
}

template <int W>
int launch_bwd(const float* dj, const float* db, const float* djm, const float* dbm, float* dx, const StreamLaunch& L,
               float wj, float wb, float wjm, float wbm, int T, int V, hipStream_t s) {
  typedef typename StreamVec<W>::type vec;
  hipLaunchKernelGGL(streams_bwd_kernel<W>, dim3(L.grid), dim3(256), 0, s, (const vec*)dj, (const vec*)db,
                     (const vec*)djm, (const vec*)dbm, (vec*)dx, L.tab, wj, wb, wjm, wbm, L.items, T, V, L.Mw);
  return agcn_check_launch();
}

}  // namespace

extern "C" {

int agcn_streams_fwd(const float* x, float* bone, float* joint_motion, float* bone_motion, const int* host_parent, int N,
                     int C, int T, int V, int M, void* stream) {
  if (!x || (!bone && !joint_motion && !bone_motion)) return AGCN_ERR_ARG;
  StreamLaunch L;
  const int rc = stream_plan(host_parent, N, C, T, V, M,
                             bits_of(x) | bits_of(bone) | bits_of(joint_motion) | bits_of(bone_motion), &L);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (L.W == 4) return launch_fwd<4>(x, bone, joint_motion, bone_motion, L, T, V, s);
  if (L.W == 2) return launch_fwd<2>(x, bone, joint_motion, bone_motion, L, T, V, s);
  return launch_fwd<1>(x, bone, joint_motion, bone_motion, L, T, V, s);
}

int agcn_streams_bwd(const float* d_joint, const float* d_bone, const float* d_joint_motion, const float* d_bone_motion,
                     float* dx, const int* host_parent, float w_joint, float w_bone, float w_joint_motion,
                     float w_bone_motion, int N, int C, int T, int V, int M, void* stream) {
  if (!dx || (!d_joint && !d_bone && !d_joint_motion && !d_bone_motion)) return AGCN_ERR_ARG;
  StreamLaunch L;
  const int rc = stream_plan(host_parent, N, C, T, V, M,
                             bits_of(dx) | bits_of(d_joint) | bits_of(d_bone) | bits_of(d_joint_motion) |
                                 bits_of(d_bone_motion), &L);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (L.W == 4)
    return launch_bwd<4>(d_joint, d_bone, d_joint_motion, d_bone_motion, dx, L, w_joint, w_bone, w_joint_motion,
                         w_bone_motion, T, V, s);
  if (L.W == 2)
    return launch_bwd<2>(d_joint, d_bone, d_joint_motion, d_bone_motion, dx, L, w_joint, w_bone, w_joint_motion,
                         w_bone_motion, T, V, s);
  return launch_bwd<1>(d_joint, d_bone, d_joint_motion, d_bone_motion, dx, L, w_joint, w_bone, w_joint_motion,
                       w_bone_motion, T, V, s);
}

}  // extern "C"
