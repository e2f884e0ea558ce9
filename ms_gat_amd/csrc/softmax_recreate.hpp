// The one place where the softmax is re-created from what the forward saved:  P_g[n,m] = 2^(S_g[n,m] - lse_g[n]),
// S_g[n,m] = sum_k (kW_g[n,k] log2 e) q_g[m,k]  in log2 units, lse from the forward.
//
// INVARIANT: every kernel that needs P after the forward forms S with the forward's own operations in the forward's own
// order, so that P comes out bit for bit as the forward formed it -- at an edge, P A is then exactly the E the forward
// kept, and a gradient through P is the gradient of the value that was used.  The order is fixed by dense.hip:
//   - kW is scaled by log2 e FIRST (one rounding), then multiplied with q;
//   - the sum runs over k = 0 .. T-1 in ascending order from 0, one fused multiply-add per k.
// Two forms give those bits.  The VALU form (edge_prob) is the chain of dense.hip's edge pass: T fmaf() in k order.  The
// matrix-core form (score_tile) is dense.hip's score chain: T/4 v_mfma_f32_16x16x4_f32 from C = 0, instruction kk
// taking k = 4 kk .. 4 kk + 3 (lane quad `quad` supplies k = 4 kk + quad), which adds the same products in the same
// order.  Which operand is the MFMA's A and which its B only transposes the tile.  Both end in v_exp_f32 (fast_exp2) of
// S - lse, one subtraction.  Nothing outside this header applies kLog2e or chains a score in the kernels that re-create
// P; a change here changes all of them together, and tests/test_gpu_score_edges.py (bits against the forward's E at
// the edges, large scores) and tests/test_gpu_group_counts.py (every kernel at training group counts) pin the result.
// dense.hip, which defines the order, includes this header too and builds its own chains (score_trip, column_trip: the
// A operand comes out of LDS there) on the same f32x4 / mfma_16x16x4 (common.hpp).
#pragma once
#include "common.hpp"

namespace msgat {

// ---- at one (n, m): the edge kernels ----------------------------------------------------------------------------------
// P_g[n,m] from [G,N,T] q / kW and [G,N] lse; NT = (size_t)N * T, hoisted by the caller
template <int T>
__device__ __forceinline__ float edge_prob(const float* __restrict__ q, const float* __restrict__ kW,
                                           const float* __restrict__ lse, int g, int n, int m, int N, size_t NT) {
  const float4* kr = reinterpret_cast<const float4*>(kW + g * NT + (size_t)n * T);
  const float4* qr = reinterpret_cast<const float4*>(q + g * NT + (size_t)m * T);
  float s = 0.f;
#pragma unroll
  for (int t4 = 0; t4 < T / 4; ++t4) {
    const float4 a = kr[t4], b = qr[t4];
    s = fmaf(a.x * kLog2e, b.x, s);
    s = fmaf(a.y * kLog2e, b.y, s);
    s = fmaf(a.z * kLog2e, b.z, s);
    s = fmaf(a.w * kLog2e, b.w, s);
  }
  return fast_exp2(s - lse[(size_t)g * N + n]);
}
// the same with N * T formed here: the compiler then folds the group offsets g * N * T with lse's g * N
template <int T>
__device__ __forceinline__ float edge_prob(const float* __restrict__ q, const float* __restrict__ kW,
                                           const float* __restrict__ lse, int g, int n, int m, int N) {
  return edge_prob<T>(q, kW, lse, g, n, m, N, (size_t)N * T);
}

// H_g[n,m] = sum_{c,t} dv[g,c,n,t] feat[g,c,m,t] by the four lanes (`sub` = 0..3) that own the edge: dvr / fr are the
// rows of channel 0 (channel stride NT), an edge's operands are `pieces` = Cu * T/4 16-B pieces in (channel, t) order and
// lane `sub` takes pieces sub, sub + 4, ...; the quad adds its partial sums with two xor shuffles, a fixed order.
constexpr int kEwLanes = 4;   // lanes per edge
template <int T>
__device__ __forceinline__ float edge_feature_dot(const float* dvr, const float* fr, size_t NT,
                                                  int pieces, int sub) {
  constexpr int T4 = T / 4;
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
  return h;
}

// ---- a 16 x 16 tile: the matrix-core kernels ----------------------------------------------------------------------------
// This lane's fragments of row `row` of a group's [N,T] kW (scaled) / q: element kk is k = 4 kk + quad.
template <int T>
__device__ __forceinline__ void score_frag_kw(const float* __restrict__ kWg, int row, int quad, float (&f)[T / 4]) {
#pragma unroll
  for (int kk = 0; kk < T / 4; ++kk) f[kk] = kWg[(size_t)row * T + 4 * kk + quad] * kLog2e;
}
template <int T>
__device__ __forceinline__ void score_frag_q(const float* __restrict__ qg, int row, int quad, float (&f)[T / 4]) {
#pragma unroll
  for (int kk = 0; kk < T / 4; ++kk) f[kk] = qg[(size_t)row * T + 4 * kk + quad];
}
// both at once, the loads of a k interleaved (the order k_adjacency_grad and k_attention_map were tuned with)
template <int T>
__device__ __forceinline__ void score_frags(const float* __restrict__ kWg, int krow, const float* __restrict__ qg, int qrow,
                                            int quad, float (&fk)[T / 4], float (&fq)[T / 4]) {
#pragma unroll
  for (int kk = 0; kk < T / 4; ++kk) {
    fk[kk] = kWg[(size_t)krow * T + 4 * kk + quad] * kLog2e;
    fq[kk] = qg[(size_t)qrow * T + 4 * kk + quad];
  }
}
// S of the tile, rows = a's rows: lane (j, quad) holds rows 4 quad .. 4 quad + 3 of column j
template <int T>
__device__ __forceinline__ f32x4 score_tile(const float (&a)[T / 4], const float (&b)[T / 4]) {
  f32x4 S = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < T / 4; ++kk) S = mfma_16x16x4(a[kk], b[kk], S);
  return S;
}

}  // namespace msgat
