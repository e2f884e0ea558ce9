// Reading the attention: the dense softmax map, and the adjacency's share of a gradient that arrives at the weights.
//
//   msgat_attention_map:      out[g,n,m] = P_g[n,m] = 2^(S_g[n,m] log2 e - lse_g[n])   (the reference's `att`,
//                             attention.py:34), for every (n, m) of every group: [G,N,N], nothing else.
//   msgat_edge_softmax_grad:  dst[v,e] += sum_{g % V == v} P_g[e] dEx[g,e]   at the CSR edges e
//                             (E = P (.) A at the edges, so dA picks up P dE there; attention.py:36).
//
// Both re-create P from what the forward saved (q, kW, lse in log2 units), as k_adjacency_grad / k_edge_weight_grad do.
//
// k_attention_map is bound by its writes (4 N^2 bytes per group against 8 N T bytes of operands).  A block owns a
// 64 x 64 tile of one group, its 4 waves 32 x 32 quadrants (2 x 2 tiles of 16 x 16), and each tile is ONE chain of T/4
// v_mfma_f32_16x16x4_f32 in k order -- k_adjacency_grad's score chain with the operands swapped: A = q rows (the
// columns m), B = kW rows * log2 e (the rows n).  The accumulator then holds S^T, so lane (j, quad) owns row n = j and
// the four consecutive columns 4 quad .. 4 quad + 3: one 16-B store per lane and tile when N % 4 == 0 (the row starts
// are then 16-B aligned), four 4-B stores of consecutive addresses otherwise.
#include "common.hpp"

namespace msgat {

constexpr int kAmWaves = 4;
constexpr int kAmBlock = 64 * kAmWaves;
constexpr int kAmTile = 64;

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int T, bool VEC>
__global__ __launch_bounds__(kAmBlock) void k_attention_map(const float* __restrict__ q, const float* __restrict__ kW,
                                                            const float* __restrict__ lse, float* __restrict__ out,
                                                            int N) {
  constexpr int T4 = T / 4;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int j = lane & 15, quad = lane >> 4;
  const int n0 = blockIdx.y * kAmTile, m0 = blockIdx.x * kAmTile;
  const size_t g = blockIdx.z;
  const size_t NT = (size_t)N * T;
  const float* kWg = kW + g * NT;
  const float* qg = q + g * NT;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;

  // rows / columns past N are clamped: they feed outputs that are never written
  float kb[2][T4], qa[2][T4], ls[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int nr = min(n0 + wr + 16 * h + j, N - 1);
    const int mr = min(m0 + wc + 16 * h + j, N - 1);
#pragma unroll
    for (int kk = 0; kk < T4; ++kk) {
      kb[h][kk] = kWg[(size_t)nr * T + 4 * kk + quad] * kLog2e;
      qa[h][kk] = qg[(size_t)mr * T + 4 * kk + quad];
    }
    ls[h] = lse[g * N + nr];
  }

  float* og = out + g * N * N;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int n = n0 + wr + 16 * a + j;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      f32x4 S = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < T4; ++kk) S = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[b][kk], kb[a][kk], S, 0, 0, 0);
      const int m = m0 + wc + 16 * b + 4 * quad;
      if (n >= N || m >= N) continue;
      float* dst = og + (size_t)n * N + m;
      const float p0 = fast_exp2(S[0] - ls[a]), p1 = fast_exp2(S[1] - ls[a]);
      const float p2 = fast_exp2(S[2] - ls[a]), p3 = fast_exp2(S[3] - ls[a]);
      if (VEC) {   // N % 4 == 0: m + 3 < N and dst is 16-B aligned
        *reinterpret_cast<float4*>(dst) = make_float4(p0, p1, p2, p3);
      } else {
        dst[0] = p0;
        if (m + 1 < N) dst[1] = p1;
        if (m + 2 < N) dst[2] = p2;
        if (m + 3 < N) dst[3] = p3;
      }
    }
  }
}

int launch_attention_map(const float* q, const float* kW, const float* lse, float* out, int G, int N, int T,
                         hipStream_t s) {
  const dim3 grid(cdiv(N, kAmTile), cdiv(N, kAmTile), G);
  const bool vec = (N & 3) == 0;
#define MSGAT_AM(TT)                                                                                               \
  if (vec)                                                                                                         \
    hipLaunchKernelGGL((k_attention_map<TT, true>), grid, dim3(kAmBlock), 0, s, q, kW, lse, out, N);               \
  else                                                                                                             \
    hipLaunchKernelGGL((k_attention_map<TT, false>), grid, dim3(kAmBlock), 0, s, q, kW, lse, out, N)
  switch (T) {
    case 4: MSGAT_AM(4); break;
    case 8: MSGAT_AM(8); break;
    case 12: MSGAT_AM(12); break;
    case 16: MSGAT_AM(16); break;
    default: return MSGAT_ERR_UNSUPPORTED;
  }
#undef MSGAT_AM
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

// One lane per (edge, value set): it walks the set's groups in ascending order, re-creates P_g at the edge with the
// forward's k-ordered score sum (k_edge_weight_grad's), and adds P_g dEx[g,e] to its own output element -- no other lane
// writes it, so there are no atomics and the sum has a fixed order.  DENSE: the element is dst[v, erow[e], col[e]] of a
// [V,N,N] gradient, else dst[v, e].
template <int T, bool DENSE>
__global__ __launch_bounds__(kBlock) void k_edge_softmax_grad(const float* __restrict__ q, const float* __restrict__ kW,
                                                              const float* __restrict__ lse, const float* __restrict__ dEx,
                                                              const int* __restrict__ erow, const int* __restrict__ col,
                                                              float* __restrict__ dst, int G, int V, int N, int nnz) {
  constexpr int T4 = T / 4;
  const int e = blockIdx.x * kBlock + threadIdx.x;
  const int v = blockIdx.y;
  if (e >= nnz) return;
  const int n = erow[e], m = col[e];
  const size_t NT = (size_t)N * T;
  float acc = 0.f;
  for (int g = v; g < G; g += V) {
    const float4* kr = reinterpret_cast<const float4*>(kW + g * NT + (size_t)n * T);
    const float4* qr = reinterpret_cast<const float4*>(q + g * NT + (size_t)m * T);
    float sc = 0.f;
#pragma unroll
    for (int t4 = 0; t4 < T4; ++t4) {
      const float4 a = kr[t4], b = qr[t4];
      sc = fmaf(a.x * kLog2e, b.x, sc);
      sc = fmaf(a.y * kLog2e, b.y, sc);
      sc = fmaf(a.z * kLog2e, b.z, sc);
      sc = fmaf(a.w * kLog2e, b.w, sc);
    }
    acc = fmaf(fast_exp2(sc - lse[(size_t)g * N + n]), dEx[(size_t)g * nnz + e], acc);
  }
  float* o = DENSE ? dst + (size_t)v * N * N + (size_t)n * N + m : dst + (size_t)v * nnz + e;
  *o += acc;
}

int launch_edge_softmax_grad(const float* q, const float* kW, const float* lse, const float* dEx, const int* erow,
                             const int* col, float* dst, bool dense, int G, int V, int N, int nnz, int T, hipStream_t s) {
  if (nnz == 0) return MSGAT_OK;
  const dim3 grid(cdiv(nnz, kBlock), V);
#define MSGAT_ES(TT)                                                                                                 \
  if (dense)                                                                                                         \
    hipLaunchKernelGGL((k_edge_softmax_grad<TT, true>), grid, dim3(kBlock), 0, s, q, kW, lse, dEx, erow, col, dst, G, \
                       V, N, nnz);                                                                                   \
  else                                                                                                               \
    hipLaunchKernelGGL((k_edge_softmax_grad<TT, false>), grid, dim3(kBlock), 0, s, q, kW, lse, dEx, erow, col, dst,  \
                       G, V, N, nnz)
  switch (T) {
    case 4: MSGAT_ES(4); break;
    case 8: MSGAT_ES(8); break;
    case 12: MSGAT_ES(12); break;
    case 16: MSGAT_ES(16); break;
    default: return MSGAT_ERR_UNSUPPORTED;
  }
#undef MSGAT_ES
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

}  // namespace msgat
