// Device helpers of the kernels that walk CSR / CSC rows (aggregate.hip): the row-walk contract of DESIGN.md section 4,
// written once.  A row's edges [e0, e1) are read as ONE window of 8 edge slots -- two 16-byte loads of indices, two of
// coefficients -- and, for the rare row longer than that, 4 more slots per trip.  Edge ranges start at arbitrary dword
// offsets; gfx950 global loads of 128 bits need only dword alignment, which the packed types tell the compiler.  A
// window or trip may cover slots outside the row (the neighbouring rows', always inside the array: it is clamped to end
// at nnz) -- those slots are masked: they read a valid row and take coefficient 0.  Trips follow each other in ascending
// edge order; the order inside the window is the caller's (gather_row alternates its halves, the others ascend).
#pragma once
#include "common.hpp"

namespace msgat {

struct __attribute__((packed, aligned(4))) int4u { int v[4]; };
struct __attribute__((packed, aligned(4))) float4u { float v[4]; };

// The first eight edge slots of a row: b0 .. b0 + 7.  Needs nnz >= 8 (a launch condition of every user).  The loads
// depend on the row's ptr entry only, so a caller may ask for them well ahead of the gather that reads them; indices and
// coefficients load apart for the caller that keeps the one and reloads the other (k_agg_ring).
struct EdgeWindow {
  int b0;
  int4u m0, m1;
  float4u w0, w1;
  __device__ __forceinline__ void load_indices(const int* __restrict__ idx) {
    m0 = *reinterpret_cast<const int4u*>(idx + b0);
    m1 = *reinterpret_cast<const int4u*>(idx + b0 + 4);
  }
  __device__ __forceinline__ void load_coefs(const float* __restrict__ Eg) {
    w0 = *reinterpret_cast<const float4u*>(Eg + b0);
    w1 = *reinterpret_cast<const float4u*>(Eg + b0 + 4);
  }
  // slot k of 0..7 (a compile-time k in every user: the selects fold away)
  __device__ __forceinline__ bool valid(int k, int e0, int e1) const { return b0 + k >= e0 && b0 + k < e1; }
  __device__ __forceinline__ int index(int k) const { return k < 4 ? m0.v[k & 3] : m1.v[k & 3]; }
  __device__ __forceinline__ float coef(int k) const { return k < 4 ? w0.v[k & 3] : w1.v[k & 3]; }
};
__device__ __forceinline__ EdgeWindow edge_window_at(int e0, int nnz) {
  EdgeWindow w;
  w.b0 = min(e0, nnz - 8);
  return w;
}
__device__ __forceinline__ EdgeWindow load_edge_window(const int* __restrict__ idx, const float* __restrict__ Eg,
                                                       int e0, int nnz) {
  EdgeWindow w = edge_window_at(e0, nnz);
  w.load_indices(idx);
  w.load_coefs(Eg);
  return w;
}

// The edges of a row behind its window, four slots per trip: a caller walks `for (int e = b0 + 8; e < e1; e += 4)` in
// ascending order and loads the trip at e -- slots b .. b + 3, clamped to end at nnz, masked like the window's.
struct EdgeTrip {
  int b;
  int4u m;
  float4u w;
  __device__ __forceinline__ bool valid(int k, int e, int e1) const { return b + k >= e && b + k < e1; }
};
__device__ __forceinline__ EdgeTrip load_edge_trip(const int* __restrict__ idx, const float* __restrict__ Eg, int e, int nnz) {
  EdgeTrip t;
  t.b = min(e, nnz - 4);
  t.m = *reinterpret_cast<const int4u*>(idx + t.b);
  t.w = *reinterpret_cast<const float4u*>(Eg + t.b);
  return t;
}

// float4 slot s of an [N][T4] slab = (node n, timesteps 4j .. 4j + 3)
struct SlotNode {
  int n, j;
};
template <int T4>
__device__ __forceinline__ SlotNode slot_node(int s) {
  const int n = s / T4;
  return {n, s - n * T4};
}

// Channel chunk k of group g: channels c0 .. c0 + ch - 1 of Cu, CH per chunk (the last one may be short), whose slabs
// of NT4 float4 start at `base` of a [G, Cu, N, T] tensor
struct ChannelChunk {
  int c0, ch;
  size_t base;
};
__device__ __forceinline__ ChannelChunk channel_chunk(int k, int CH, int Cu, int g, int NT4) {
  ChannelChunk c;
  c.c0 = k * CH;
  c.ch = min(CH, Cu - c.c0);
  c.base = ((size_t)g * Cu + c.c0) * NT4;
  return c;
}

// The aggregate forms' epilogue: v = acc + av * extra when the launch has an addvec (av = addvec_at(...)), else v = acc
__device__ __forceinline__ float addvec_at(const float* __restrict__ addvec, int i) {
  return (addvec != nullptr) ? addvec[i] : 0.f;
}
__device__ __forceinline__ void store_plus_extra(float4* v, float4 acc, const float* addvec, float av,
                                                 const float4* extra) {
  if (addvec != nullptr) f4fma(av, *extra, acc);
  *v = acc;
}

}  // namespace msgat
