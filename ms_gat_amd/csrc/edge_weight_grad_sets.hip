// Gradient of the stored values of a per-sample sparse adjacency: one shared structure, V value sets (val [V,nnz]).
//
//   dval[v,e] = sum_{g : g % V == v} P_g[n_e,m_e] (H_g[n_e,m_e] + dEx[g,e]),  H_g[n,m] = sum_{c,t} dv[g,c,n,t] feat[g,c,m,t]
//
// k_edge_weight_grad (edge_weight_grad.hip) with the sum over the groups cut at the value sets: group g = r*Bg + b reads
// set g % V, so a set's groups are the G / V relations of ONE sample (V = Bg), or one group (V = G).  P is re-created at
// the edge as there, with the forward's k-ordered score sum; dEx [G,nnz] is the gradient that arrives at the returned
// attention weights (or NULL), folded in here so that P is formed once.
//
// A block owns 64 consecutive edges of one set (four lanes per edge, pieces of 16 B dealt round-robin as in
// k_edge_weight_grad) and adds the set's groups in ascending order: every (v,e) has one owner, so there is no split, no
// workspace, no reduction launch and no atomics.  NG = G / V groups per set is a template parameter up to 4 (1 for a
// set per group, the relation count for a set per sample): the scores of exactly those groups are formed first (their
// q / kW / lse loads leave together), then the group loop runs over the feature rows.  More than 4 groups per set
// (NG = 0) go four at a time, a slot past the last group skipped (block-uniform).
//
// Block -> (set, tile): set v runs on XCD v % 8 (consecutive block ids go round the 8 XCDs, as for k_agg_sell), all its
// tiles side by side there, so the [Cu,N,T] slabs of a set's groups are fetched into ONE L2 instead of all eight.
// Placement is for speed only: a block computes the same (v, tile) whatever CU runs it.  At R = 3, B = 32, N = 883,
// Cu = 24: 60 us with this map, 91 us with blocks in plain (set, tile) order, 94 us for k_edge_weight_grad plus its
// reduction on the same buffers.  With fewer than 8 sets some XCDs get no set; measured at V = 2, 4, 6 and 12 the two
// maps are within 3 % of each other there (a few dozen blocks: the launch is latency-bound), so there is one map
// (DESIGN.md "Per-sample edge weights"; lab builds: MSGAT_LAB_EWS_LINEAR=1 is the plain order).
#include "common.hpp"

#ifdef MSGAT_LAB
#include <cstdlib>
#endif

namespace msgat {

constexpr int kEwsLanes = 4;                     // lanes per edge
constexpr int kEwsEdges = kBlock / kEwsLanes;    // edges per block
constexpr int kEwsXcds = 8;
constexpr int kEwsAhead = 4;                     // groups of a set whose scores are formed together

template <int T>
__device__ __forceinline__ float ews_prob(const float* __restrict__ q, const float* __restrict__ kW,
                                          const float* __restrict__ lse, int g, int n, int m, int N) {
  constexpr int T4 = T / 4;
  const size_t NT = (size_t)N * T;
  const float4* kr = reinterpret_cast<const float4*>(kW + g * NT + (size_t)n * T);
  const float4* qr = reinterpret_cast<const float4*>(q + g * NT + (size_t)m * T);
  float s = 0.f;
#pragma unroll
  for (int t4 = 0; t4 < T4; ++t4) {
    const float4 a = kr[t4], b = qr[t4];
    s = fmaf(a.x * kLog2e, b.x, s);
    s = fmaf(a.y * kLog2e, b.y, s);
    s = fmaf(a.z * kLog2e, b.z, s);
    s = fmaf(a.w * kLog2e, b.w, s);
  }
  return fast_exp2(s - lse[(size_t)g * N + n]);
}

template <int T, int NG>
__global__ __launch_bounds__(kBlock) void k_edge_weight_grad_sets(
    const float* __restrict__ dv, size_t dv_gstride, const float* __restrict__ feat, const float* __restrict__ q,
    const float* __restrict__ kW, const float* __restrict__ lse, const float* __restrict__ dEx,
    const int* __restrict__ erow, const int* __restrict__ col, float* __restrict__ dval, int N, int nnz, int Cu, int G,
    int V, int tiles, int xcd) {
  constexpr int T4 = T / 4;
  constexpr int kSlots = NG > 0 ? NG : kEwsAhead;
  int v, tile;
  if (xcd) {
    const int local = blockIdx.x / kEwsXcds;
    v = (local / tiles) * kEwsXcds + blockIdx.x % kEwsXcds;
    tile = local % tiles;
    if (v >= V) return;                          // the last round of sets is not full (block-uniform)
  } else {
    v = blockIdx.x / tiles;
    tile = blockIdx.x % tiles;
  }
  const int sub = threadIdx.x & (kEwsLanes - 1);
  const int e = tile * kEwsEdges + threadIdx.x / kEwsLanes;
  const int ee = min(e, nnz - 1);                // lanes past the last edge compute on it and store nothing
  const int n = erow[ee], m = col[ee];
  const size_t NT = (size_t)N * T;
  const int pieces = Cu * T4;

  float acc = 0.f;
  for (int g0 = v; g0 < G; g0 += kSlots * V) {   // NG > 0: G = NG * V, one trip
    float p[kSlots], x[kSlots];
#pragma unroll
    for (int i = 0; i < kSlots; ++i) {
      const int g = g0 + i * V;
      p[i] = x[i] = 0.f;
      if (NG > 0 || g < G) {
        p[i] = ews_prob<T>(q, kW, lse, g, n, m, N);
        if (dEx) x[i] = dEx[(size_t)g * nnz + ee];
      }
    }
#pragma unroll
    for (int i = 0; i < kSlots; ++i) {
      const int g = g0 + i * V;
      if (NG > 0 || g < G) {
        const float* dvr = dv + g * dv_gstride + (size_t)n * T;
        const float* fr = feat + (size_t)g * Cu * NT + (size_t)m * T;
        float h = 0.f;
#pragma unroll 4
        for (int pc = sub; pc < pieces; pc += kEwsLanes) {
          const int c = pc / T4, t = 4 * (pc - c * T4);
          const float4 a = *reinterpret_cast<const float4*>(dvr + c * NT + t);
          const float4 b = *reinterpret_cast<const float4*>(fr + c * NT + t);
          h = f4dot(a, b, h);
        }
        h += __shfl_xor(h, 1);
        h += __shfl_xor(h, 2);
        acc = fmaf(p[i], h + x[i], acc);
      }
    }
  }
  if (e < nnz && sub == 0) dval[(size_t)v * nnz + e] = acc;
}

#ifdef MSGAT_LAB
static int ews_lab_linear() {   // lab builds only: 1 = blocks in plain (set, tile) order, for A/B runs of the map
  static const int linear = [] { const char* s = getenv("MSGAT_LAB_EWS_LINEAR"); return s ? atoi(s) : 0; }();
  return linear;
}
#endif

int launch_edge_weight_grad_sets(const float* dv, int dv_group_channels, const float* feat, const float* q,
                                 const float* kW, const float* lse, const float* dEx, const int* erow, const int* col,
                                 float* dval, int G, int V, int Cu, int N, int nnz, int T, hipStream_t s) {
  if (nnz == 0) return MSGAT_OK;
  const size_t dv_gstride = (size_t)(dv_group_channels > 0 ? dv_group_channels : Cu) * N * T;
  const int tiles = cdiv(nnz, kEwsEdges);
  int xcd = 1;
#ifdef MSGAT_LAB
  xcd = !ews_lab_linear();
#endif
  const long long blocks = xcd ? (long long)cdiv(V, kEwsXcds) * kEwsXcds * tiles : (long long)V * tiles;
  if (blocks >= (1ll << 31)) return MSGAT_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)blocks);
  const int per_set = G / V;                     // V divides G (checked by the caller)
#define MSGAT_EWS_RUN(TT, NG)                                                                                        \
  hipLaunchKernelGGL((k_edge_weight_grad_sets<TT, NG>), grid, dim3(kBlock), 0, s, dv, dv_gstride, feat, q, kW, lse, \
                     dEx, erow, col, dval, N, nnz, Cu, G, V, tiles, xcd)
#define MSGAT_EWS(TT)                        \
  switch (per_set) {                         \
    case 1: MSGAT_EWS_RUN(TT, 1); break;     \
    case 2: MSGAT_EWS_RUN(TT, 2); break;     \
    case 3: MSGAT_EWS_RUN(TT, 3); break;     \
    case 4: MSGAT_EWS_RUN(TT, 4); break;     \
    default: MSGAT_EWS_RUN(TT, 0); break;    \
  }
  switch (T) {
    case 4: MSGAT_EWS(4); break;
    case 8: MSGAT_EWS(8); break;
    case 12: MSGAT_EWS(12); break;
    case 16: MSGAT_EWS(16); break;
    default: return MSGAT_ERR_UNSUPPORTED;
  }
#undef MSGAT_EWS
#undef MSGAT_EWS_RUN
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

}  // namespace msgat
