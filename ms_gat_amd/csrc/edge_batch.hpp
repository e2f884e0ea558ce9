// What the per-sample edge-weight kernels (edge_time.hip, edge_signal.hip, edge_dropout.hip, edge_validity.hip) share.
//
// The contract of a weight shared by the batch ("The ascending-sample-order contract"): its gradient is
// +0 + term(0,e) + term(1,e) + ... in ascending sample order, every term rounded before it is added, every entry written,
// nothing atomic.  The two forms below are its only implementations on the device:
//   for_samples_ahead   a lane owns its edge and walks the samples itself (the terms are loads: edge_time, edge_signal)
//   edge_batch_sum      a block forms the terms of a tile of samples in parallel, one wave adds them (the terms cost
//                       arithmetic: edge_dropout's generator; edge_validity's gate keeps the skeleton written out)
#pragma once
#include "common.hpp"

namespace msgat {

// the grid of an elementwise launch: `units` of work (edges, or quads of edges) in x, `block` per block; a block row per
// sample in y, at most 65535 of them -- the kernels stride their sample loop by gridDim.y
inline dim3 edge_sample_grid(long long units, int block, int V) {
  return dim3((unsigned)((units + block - 1) / block), (unsigned)(V < 65535 ? V : 65535));
}

// f(src[i * stride], i) for i = 0 .. n - 1 in ascending order, kAhead loads requested before the first of them is used
// (what follows a load is a dependent chain: the loads of a group are in flight together), then a scalar tail
template <int kAhead, class F>
__device__ __forceinline__ void for_samples_ahead(const float* __restrict__ src, long long stride, int n, F f) {
  int i = 0;
  for (; i + kAhead <= n; i += kAhead) {
    float g[kAhead];
#pragma unroll
    for (int k = 0; k < kAhead; ++k) g[k] = src[(long long)(i + k) * stride];
#pragma unroll
    for (int k = 0; k < kAhead; ++k) f(g[k], i + k);
  }
  for (; i < n; ++i) f(src[(long long)i * stride], i);
}

constexpr int kEbSumBlock = 256;    // lanes of a summing block
constexpr int kEbSumEdges = 64;     // edges per block of a summing backward: one wave adds them
constexpr int kEbSumSamples = 64;   // samples per LDS tile of terms (16 KiB)

// dw[e] = +0 + term(0,e) + term(1,e) + ... for the block's kEbSumEdges edges; kEbSumBlock lanes, a block per kEbSumEdges
// edges.  A lane owns one unit of kUnit consecutive edges and every (kEbSumBlock * kUnit / kEbSumEdges)-th sample of a tile:
// fill(e0, n, v, dst) writes the n <= kUnit rounded terms of the unit that starts at edge e0 for sample v to dst[0..n).
// Then a lane per edge adds its column of the tile; two barriers per tile.  Every live entry is written (V = 0: +0).
template <int kUnit, class Fill>
__device__ __forceinline__ void edge_batch_sum(float* __restrict__ dw, int V, long long nnz, Fill fill) {
  static_assert(kEbSumEdges % kUnit == 0 && kEbSumBlock % (kEbSumEdges / kUnit) == 0, "a unit divides the block's edges");
  constexpr int kUnits = kEbSumEdges / kUnit;                      // units per block
  __shared__ float term[kEbSumSamples][kEbSumEdges];
  const int tid = threadIdx.x;
  const long long eb = (long long)blockIdx.x * kEbSumEdges;       // the block's first edge: a multiple of kUnit
  const int ul = tid & (kUnits - 1);                               // this lane's unit inside the block
  const long long e0 = eb + kUnit * ul;
  const int n = e0 >= nnz ? 0 : (nnz - e0 < kUnit ? (int)(nnz - e0) : kUnit);
  float acc = 0.f;
  for (int v0 = 0; v0 < V; v0 += kEbSumSamples) {
    const int nv = V - v0 < kEbSumSamples ? V - v0 : kEbSumSamples;
    __syncthreads();                                               // the previous tile's terms have been added
    if (n > 0)
      for (int i = tid / kUnits; i < nv; i += kEbSumBlock / kUnits) fill(e0, n, v0 + i, &term[i][kUnit * ul]);
    __syncthreads();
    if (tid < kEbSumEdges && eb + tid < nnz)
      for (int i = 0; i < nv; ++i) acc += term[i][tid];            // rounded terms, added from +0 in sample order
  }
  if (tid < kEbSumEdges && eb + tid < nnz) dw[eb + tid] = acc;
}

}  // namespace msgat
