// Per-sample edge weights of a batched adjacency (the `* adjacency` of attention.py:36 with adjacency [V,N,N]).
//
//   vals[v, e] = adj[v, erow_e, col_e]                      for every edge e of ONE shared CSR structure
//   outside   += #{(v, n, m) : adj[v,n,m] != 0, (n, m) not an edge of the structure}
//
// The structure is the union of the samples' patterns, so a sample that lacks a union edge gets an explicit 0 there
// (E = 0: that edge contributes nothing, forward or backward).  The kernel streams every row of the dense tensor once,
// with 16-B loads, counting its non-zeros (`!(v == 0)`, the predicate of graph_host.cpp's is_edge: NaN is an edge); it
// then gathers the row's pattern positions (L2 hits: the row was just read), counts the non-zeros among them and adds the
// difference to the counter.  Every refresh is checked; whether the count is ever read back is the caller's choice.
//
// HBM-bound: 4 V N^2 bytes read + 4 V nnz written.  One wave per (sample, row); a row's body goes as float4 loads four
// per lane in flight per trip, its unaligned head and tail (rows of N % 4 != 0 start anywhere) as single floats.
#include "common.hpp"

namespace msgat {

constexpr int kEvWaves = 4;
constexpr int kEvBlock = 64 * kEvWaves;
constexpr int kEvUnroll = 4;   // float4 loads in flight per lane

__device__ __forceinline__ int nz(float v) { return !(v == 0.f); }

__global__ __launch_bounds__(kEvBlock) void k_edge_values(const float* __restrict__ adj, const int* __restrict__ rowptr,
                                                          const int* __restrict__ col, float* __restrict__ vals,
                                                          int* __restrict__ outside, int V, int N, int nnz) {
  const int64_t row = (int64_t)blockIdx.x * kEvWaves + (threadIdx.x >> 6);   // v * N + n
  const int lane = threadIdx.x & 63;
  if (row >= (int64_t)V * N) return;
  const int v = (int)(row / N), n = (int)(row - (int64_t)v * N);
  const float* a = adj + row * N;

  // head: up to 3 floats until a 16-B boundary; body: float4s; tail: the rest
  const int head = min((int)((4 - (((uintptr_t)a >> 2) & 3)) & 3), N);
  const int nbody = (N - head) >> 2;
  const float4* body = reinterpret_cast<const float4*>(a + head);
  int cnt = 0;
  if (lane < head) cnt += nz(a[lane]);
  const int tail0 = head + 4 * nbody;
  if (lane < N - tail0) cnt += nz(a[tail0 + lane]);
  int i = lane;
  for (; i + 64 * (kEvUnroll - 1) < nbody; i += 64 * kEvUnroll) {
    float4 x[kEvUnroll];
#pragma unroll
    for (int k = 0; k < kEvUnroll; ++k) x[k] = body[i + 64 * k];
#pragma unroll
    for (int k = 0; k < kEvUnroll; ++k) cnt += nz(x[k].x) + nz(x[k].y) + nz(x[k].z) + nz(x[k].w);
  }
  for (; i < nbody; i += 64) {
    const float4 x = body[i];
    cnt += nz(x.x) + nz(x.y) + nz(x.z) + nz(x.w);
  }

  // the pattern's positions of this row: gather, store, and take their non-zeros off the row's count
  const int e0 = rowptr[n], e1 = rowptr[n + 1];
  float* vo = vals + (int64_t)v * nnz;
  for (int e = e0 + lane; e < e1; e += 64) {
    const float x = a[col[e]];
    vo[e] = x;
    cnt -= nz(x);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0 && cnt != 0) atomicAdd(outside, cnt);
}

int launch_edge_values(const float* adj, const int* rowptr, const int* col, float* vals, int* outside, int V, int N,
                       int nnz, hipStream_t s) {
  const int64_t rows = (int64_t)V * N;
  hipLaunchKernelGGL(k_edge_values, dim3((unsigned)cdiv64(rows, kEvWaves)), dim3(kEvBlock), 0, s, adj, rowptr, col, vals,
                     outside, V, N, nnz);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

}  // namespace msgat
