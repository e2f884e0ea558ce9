// Gradient of a sparse adjacency's stored values (a learned weight per existing edge): one shared structure, V value
// sets (val [V,nnz]; V = 1 is one [N,N] matrix).
//
//   dval[v,e] = sum_{g : g % V == v} P_g[n_e,m_e] (H_g[n_e,m_e] + dEx[g,e]),  H_g[n,m] = sum_{c,t} dv[g,c,n,t] feat[g,c,m,t]
//
// the dense gradient of adjacency_grad.hip restricted to the structure's edges, in CSR order.  Nothing [N,N] is read
// or written: P is re-created at the edge (edge_prob, softmax_recreate.hpp) from what the forward saved; H is the
// backward SDDMM's gather, Cu rows of T floats of dv at the edge's row and of feat at its column; dEx [G,nnz] is the
// gradient that arrives at the returned attention weights (or NULL).
//
// Four lanes own an edge (lane quad).  An edge's operands are Cu rows of T floats, Cu * T/4 16-B pieces in (channel, t)
// order; lane s takes pieces s, s + 4, ..., so the quad reads consecutive pieces: a row of T = 16 is one contiguous
// 64-B read, a row of T = 12 and the first piece of the next (lane s owning channels s, s + 4, ... was 5 % slower).
// A wave covers 16 edges, consecutive in CSR order, so the dv rows it reads are a few neighbouring rows per channel and
// the feat rows are gathered through the cache (a group's [Cu,N,T] slab is ~1 MB at PEMSD7 size).  The quad adds its
// four partial sums with two xor shuffles, a fixed order (edge_feature_dot).  Deterministic, no atomics.  The two
// kernels differ in who sums the groups:
//
// k_edge_weight_grad (V = 1).  One [N,N] graph has few edges (2 615 at N = 883: 41 blocks of 64 edges), so the groups
// are split over blocks as in msgat_adjacency_grad: split j sums its groups in ascending order into the workspace and
// the library's reduction (k_reduce_few, k_reduce_partials past 16 splits) adds the splits in order.  The split count is
// set by memory parallelism: 16 splits (about 10 waves per CU at the headline size) left the waves waiting on memory
// 44 % of their cycles; 48 were 9 % faster.  The share of dEx is added by k_edge_softmax_grad afterwards.
//
// k_edge_weight_grad_sets (V > 1).  Group g = r*Bg + b reads set g % V, so a set's groups are the G / V relations of ONE
// sample (V = Bg), or one group (V = G).  A block owns 64 consecutive edges of one set and adds the set's groups in
// ascending order, dEx folded in so that P is formed once: every (v,e) has one owner, so there is no split, no
// workspace and no reduction launch.  NG = G / V groups per set is a template parameter up to 4 (1 for a set per
// group, the relation count for a set per sample): the scores of exactly those groups are formed first (their q / kW /
// lse loads leave together), then the group loop runs over the feature rows.  More than 4 groups per set (NG = 0) go
// four at a time, a slot past the last group skipped (block-uniform).
//
// Block -> (set, tile): set v runs on XCD v % 8 (consecutive block ids go round the 8 XCDs, as for k_agg_sell), all its
// tiles side by side there, so the [Cu,N,T] slabs of a set's groups are fetched into ONE L2 instead of all eight.
// Placement is for speed only: a block computes the same (v, tile) whatever CU runs it.  At R = 3, B = 32, N = 883,
// Cu = 24: 60 us with this map, 91 us with blocks in plain (set, tile) order, 94 us for k_edge_weight_grad plus its
// reduction on the same buffers.  With fewer than 8 sets some XCDs get no set; measured at V = 2, 4, 6 and 12 the two
// maps are within 3 % of each other there (a few dozen blocks: the launch is latency-bound), so there is one map
// (DESIGN.md "Per-sample edge weights"; lab builds: MSGAT_LAB_EWS_LINEAR=1 is the plain order).
#include "softmax_recreate.hpp"

#ifdef MSGAT_LAB
#include <cstdlib>
#endif

namespace msgat {

constexpr int kEwEdges = kBlock / kEwLanes;    // edges per block
constexpr int kEwTargetBlocks = 4096;          // 16 blocks per CU on a 256-CU part before the groups are split
constexpr int kEwMaxSplit = 48;                // past 16, k_reduce_partials adds the splits (still in order)
constexpr int kEwsXcds = 8;
constexpr int kEwsAhead = 4;                   // groups of a set whose scores are formed together

template <int T>
__global__ __launch_bounds__(kBlock) void k_edge_weight_grad(
    const float* __restrict__ dv, size_t dv_gstride, const float* __restrict__ feat, const float* __restrict__ q,
    const float* __restrict__ kW, const float* __restrict__ lse, const int* __restrict__ erow,
    const int* __restrict__ col, float* __restrict__ out, int N, int nnz, int Cu, int G, int per) {
  const int sub = threadIdx.x & (kEwLanes - 1);
  const int e = blockIdx.x * kEwEdges + threadIdx.x / kEwLanes;
  const int ee = min(e, nnz - 1);              // lanes past the last edge compute on it and store nothing
  const int n = erow[ee], m = col[ee];
  const int g0 = blockIdx.y * per, g1 = min(G, g0 + per);
  const size_t NT = (size_t)N * T;

  float acc = 0.f;
  for (int g = g0; g < g1; ++g) {
    const float p = edge_prob<T>(q, kW, lse, g, n, m, N, NT);
    const float h = edge_feature_dot<T>(dv + g * dv_gstride + (size_t)n * T, feat + (size_t)g * Cu * NT + (size_t)m * T,
                                        NT, Cu * (T / 4), sub);
    acc = fmaf(p, h, acc);
  }
  if (e < nnz && sub == 0) out[(size_t)blockIdx.y * nnz + e] = acc;
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
  const int sub = threadIdx.x & (kEwLanes - 1);
  const int e = tile * kEwEdges + threadIdx.x / kEwLanes;
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
        p[i] = edge_prob<T>(q, kW, lse, g, n, m, N);
        if (dEx) x[i] = dEx[(size_t)g * nnz + ee];
      }
    }
#pragma unroll
    for (int i = 0; i < kSlots; ++i) {
      const int g = g0 + i * V;
      if (NG > 0 || g < G) {
        // edge_feature_dot's loop, written out: through the helper the compiler serialised the loads of the slots'
        // rows (T = 16, NG = 3: 89 us against 76 us at R = 3, B = 32, N = 883)
        const float* dvr = dv + g * dv_gstride + (size_t)n * T;
        const float* fr = feat + (size_t)g * Cu * NT + (size_t)m * T;
        float h = 0.f;
#pragma unroll 4
        for (int pc = sub; pc < pieces; pc += kEwLanes) {
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

// V = 1: the groups split over `nsplit` blocks per edge tile
static void edge_weight_grad_split(int nnz, int G, int* nsplit, int* per) {
  group_split(cdiv(max(nnz, 1), kEwEdges), G, kEwTargetBlocks, kEwMaxSplit, nsplit, per);
}

size_t edge_weight_grad_workspace_bytes(int nnz, int G, int V) {
  if (V != 1) return 0;
  int nsplit, per;
  edge_weight_grad_split(nnz, G, &nsplit, &per);
  return nsplit > 1 ? sizeof(float) * (size_t)nsplit * nnz : 0;
}

int launch_edge_weight_grad(const float* dv, int dv_group_channels, const float* feat, const float* q, const float* kW,
                            const float* lse, const float* dEx, const int* erow, const int* col, float* dval, float* ws,
                            int G, int V, int Cu, int N, int nnz, int T, hipStream_t s) {
  if (nnz == 0) return MSGAT_OK;
  const size_t dv_gstride = (size_t)(dv_group_channels > 0 ? dv_group_channels : Cu) * N * T;
  const int tiles = cdiv(nnz, kEwEdges);
  if (V == 1) {   // one [N,N] matrix: the split kernel, the reduction of its partial sums, then the share of dEx
    int nsplit, per;
    edge_weight_grad_split(nnz, G, &nsplit, &per);
    float* out = nsplit > 1 ? ws : dval;
    int st = dispatch_T(T, [&](auto t) -> int {
      hipLaunchKernelGGL(k_edge_weight_grad<decltype(t)::value>, dim3(tiles, nsplit), dim3(kBlock), 0, s, dv, dv_gstride,
                         feat, q, kW, lse, erow, col, out, N, nnz, Cu, G, per);
      MSGAT_CHECK_LAUNCH();
      return MSGAT_OK;
    });
    if (st == MSGAT_OK && nsplit > 1) st = launch_reduce_groups(ws, 1, nsplit, nnz, dval, s);
    if (st != MSGAT_OK || !dEx) return st;
    return launch_edge_softmax_grad(q, kW, lse, dEx, erow, col, dval, false, G, 1, N, nnz, T, s);
  }
  int xcd = 1;
#ifdef MSGAT_LAB
  xcd = !ews_lab_linear();
#endif
  const long long blocks = xcd ? (long long)cdiv(V, kEwsXcds) * kEwsXcds * tiles : (long long)V * tiles;
  if (blocks >= (1ll << 31)) return MSGAT_ERR_UNSUPPORTED;
  const int per_set = G / V;                     // V divides G (checked by the caller)
  return dispatch_T(T, [&](auto t) -> int {
    auto run = [&](auto ng) {
      hipLaunchKernelGGL((k_edge_weight_grad_sets<decltype(t)::value, decltype(ng)::value>), dim3((unsigned)blocks),
                         dim3(kBlock), 0, s, dv, dv_gstride, feat, q, kW, lse, dEx, erow, col, dval, N, nnz, Cu, G, V,
                         tiles, xcd);
    };
    switch (per_set) {
      case 1: run(std::integral_constant<int, 1>{}); break;
      case 2: run(std::integral_constant<int, 2>{}); break;
      case 3: run(std::integral_constant<int, 3>{}); break;
      case 4: run(std::integral_constant<int, 4>{}); break;
      default: run(std::integral_constant<int, 0>{}); break;
    }
    MSGAT_CHECK_LAUNCH();
    return MSGAT_OK;
  });
}

}  // namespace msgat
