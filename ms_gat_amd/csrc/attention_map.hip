// Reading the attention: the dense softmax map, and the adjacency's share of a gradient that arrives at the weights.
//
//   msgat_attention_map:      out[g,n,m] = P_g[n,m] = 2^(S_g[n,m] log2 e - lse_g[n])   (the reference's `att`,
//                             attention.py:34), for every (n, m) of every group: [G,N,N], nothing else.
//   msgat_edge_softmax_grad:  dst[v,e] += sum_{g % V == v} P_g[e] dEx[g,e]   at the CSR edges e
//                             (E = P (.) A at the edges, so dA picks up P dE there; attention.py:36).
//
// Both re-create P from what the forward saved (q, kW, lse in log2 units), as k_adjacency_grad / k_edge_weight_grad do:
// through softmax_recreate.hpp, the one definition of that arithmetic.
//
// k_attention_map is bound by its writes (4 N^2 bytes per group against 8 N T bytes of operands).  A block owns a
// 64 x 64 tile of one group, its 4 waves 32 x 32 quadrants (2 x 2 tiles of 16 x 16), and each tile is ONE chain of T/4
// v_mfma_f32_16x16x4_f32 in k order -- k_adjacency_grad's score chain with the operands swapped: A = q rows (the
// columns m), B = kW rows * log2 e (the rows n).  The accumulator then holds S^T, so lane (j, quad) owns row n = j and
// the four consecutive columns 4 quad .. 4 quad + 3: one 16-B store per lane and tile when N % 4 == 0 (the row starts
// are then 16-B aligned), four 4-B stores of consecutive addresses otherwise.
#include "softmax_recreate.hpp"

namespace msgat {

constexpr int kAmWaves = 4;
constexpr int kAmBlock = 64 * kAmWaves;
constexpr int kAmTile = 64;

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
    score_frags<T>(kWg, nr, qg, mr, quad, kb[h], qa[h]);
    ls[h] = lse[g * N + nr];
  }

  float* og = out + g * N * N;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int n = n0 + wr + 16 * a + j;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const f32x4 S = score_tile<T>(qa[b], kb[a]);
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
  return dispatch_T(T, [&](auto t) -> int {
    constexpr int TT = decltype(t)::value;
    if (vec)
      hipLaunchKernelGGL((k_attention_map<TT, true>), grid, dim3(kAmBlock), 0, s, q, kW, lse, out, N);
    else
      hipLaunchKernelGGL((k_attention_map<TT, false>), grid, dim3(kAmBlock), 0, s, q, kW, lse, out, N);
    MSGAT_CHECK_LAUNCH();
    return MSGAT_OK;
  });
}

// One lane per (edge, value set): it walks the set's groups in ascending order, re-creates P_g at the edge with the
// forward's k-ordered score sum (edge_prob), and adds P_g dEx[g,e] to its own output element -- no other lane
// writes it, so there are no atomics and the sum has a fixed order.  DENSE: the element is dst[v, erow[e], col[e]] of a
// [V,N,N] gradient, else dst[v, e].
template <int T, bool DENSE>
__global__ __launch_bounds__(kBlock) void k_edge_softmax_grad(const float* __restrict__ q, const float* __restrict__ kW,
                                                              const float* __restrict__ lse, const float* __restrict__ dEx,
                                                              const int* __restrict__ erow, const int* __restrict__ col,
                                                              float* __restrict__ dst, int G, int V, int N, int nnz) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  const int v = blockIdx.y;
  if (e >= nnz) return;
  const int n = erow[e], m = col[e];
  const size_t NT = (size_t)N * T;
  float acc = 0.f;
  for (int g = v; g < G; g += V) {
    acc = fmaf(edge_prob<T>(q, kW, lse, g, n, m, N, NT), dEx[(size_t)g * nnz + e], acc);
  }
  float* o = DENSE ? dst + (size_t)v * N * N + (size_t)n * N + m : dst + (size_t)v * nnz + e;
  *o += acc;
}

int launch_edge_softmax_grad(const float* q, const float* kW, const float* lse, const float* dEx, const int* erow,
                             const int* col, float* dst, bool dense, int G, int V, int N, int nnz, int T, hipStream_t s) {
  if (nnz == 0) return MSGAT_OK;
  const dim3 grid(cdiv(nnz, kBlock), V);
  return dispatch_T(T, [&](auto t) -> int {
    constexpr int TT = decltype(t)::value;
    if (dense)
      hipLaunchKernelGGL((k_edge_softmax_grad<TT, true>), grid, dim3(kBlock), 0, s, q, kW, lse, dEx, erow, col, dst, G, V,
                         N, nnz);
    else
      hipLaunchKernelGGL((k_edge_softmax_grad<TT, false>), grid, dim3(kBlock), 0, s, q, kW, lse, dEx, erow, col, dst, G, V,
                         N, nnz);
    MSGAT_CHECK_LAUNCH();
    return MSGAT_OK;
  });
}


// ---- the gradient that arrives at the dense map (weights = "softmax_grad") --------------------------------------------
// Given dP [G,N,N] at P = softmax_m(S), S = kW q^T:   r[n] = sum_m P[n,m] dP[n,m],   dS = P (.) (dP - r),
//   dkW = dS q,   dq_map = dS^T kW + dkW Wg^T,   dWg_map[rel] = sum_{g in rel} q^T dkW.
// dP is read twice and P is never stored: both passes re-create it per 16 x 16 tile with k_attention_map's k-ordered
// v_mfma_f32_16x16x4_f32 chain, and form their product with q / kW on the matrix core as well (4 more instructions of
// the same kind per tile, the tile's own P dP or dS values as one operand).  A wave owns 16 rows (row pass) or 16 columns
// (column pass) and walks the other axis alone: no LDS, no barrier, every sum in a fixed order, no atomics.
//   k_map_grad_rows:  r and dkW = sum_m (P dP)[n,m] q[m] - r[n] sum_m P[n,m] q[m]   (one read of dP, along its rows)
//   k_map_grad_cols:  dq_add[m] += sum_n dS[n,m] kW[n] + dkW[m] Wg^T                (the second read, 64-B row pieces)
//   k_map_grad_dwg / k_map_grad_dwg_sum:  dWg_add[rel] += sum_{g in rel} sum_n q[n]^T dkW[n]   (per 64-row partials first)
constexpr int kMgWaves = 2;
constexpr int kMgBlock = 64 * kMgWaves;
constexpr int kMgSpan = 16 * kMgWaves;   // rows (columns) of a block
constexpr int kMgChunk = 64;             // rows per dWg partial

template <int T, bool VEC>
__global__ __launch_bounds__(kMgBlock) void k_map_grad_rows(const float* __restrict__ q, const float* __restrict__ kW,
                                                            const float* __restrict__ lse, const float* __restrict__ dP,
                                                            float* __restrict__ dkW, float* __restrict__ r, int N) {
  constexpr int T4 = T / 4;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j = lane & 15, quad = lane >> 4;
  const int n0 = blockIdx.x * kMgSpan + 16 * wave;
  if (n0 >= N) return;   // the whole wave: there is no barrier below
  const size_t g = blockIdx.y;
  const size_t NT = (size_t)N * T;
  const float* kWg = kW + g * NT;
  const float* qg = q + g * NT;
  const int n = n0 + j, nr = min(n, N - 1);   // rows past N are clamped: their results are never written

  float kb[T4];
  score_frag_kw<T>(kWg, nr, quad, kb);
  const float ls = lse[g * N + nr];
  const float* dPr = dP + g * N * N + (size_t)nr * N;

  f32x4 accX = {0.f, 0.f, 0.f, 0.f}, accP = {0.f, 0.f, 0.f, 0.f};   // [t = 4 quad + v][n = j]
  float rsum = 0.f;
  for (int m0 = 0; m0 < N; m0 += 64) {
    float qa[4][T4], qv[4][4], d[4][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int mt = m0 + 16 * b, m = mt + 4 * quad;
      const int mr = min(mt + j, N - 1);
      score_frag_q<T>(qg, mr, quad, qa[b]);
#pragma unroll
      for (int v = 0; v < 4; ++v) qv[b][v] = j < T ? qg[(size_t)min(m + v, N - 1) * T + j] : 0.f;
      if (VEC) {   // N % 4 == 0 and dP 16-B aligned: m + 3 < N whenever m < N
        const float4 t = m < N ? *reinterpret_cast<const float4*>(dPr + m) : f4zero();
        d[b][0] = t.x; d[b][1] = t.y; d[b][2] = t.z; d[b][3] = t.w;
      } else {
#pragma unroll
        for (int v = 0; v < 4; ++v) d[b][v] = m + v < N ? dPr[m + v] : 0.f;
      }
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int m = m0 + 16 * b + 4 * quad;
      const f32x4 S = score_tile<T>(qa[b], kb);
      float p[4], x[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        p[v] = m + v < N ? fast_exp2(S[v] - ls) : 0.f;
        x[v] = p[v] * d[b][v];
      }
      rsum += (x[0] + x[1]) + (x[2] + x[3]);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        accX = mfma_16x16x4(qv[b][v], x[v], accX);
        accP = mfma_16x16x4(qv[b][v], p[v], accP);
      }
    }
  }
  // the four quads of a row: the same two additions in every lane (a + b == b + a bit for bit)
  rsum += __shfl_xor(rsum, 16);
  rsum += __shfl_xor(rsum, 32);
  if (n >= N) return;
  if (quad == 0) r[g * N + n] = rsum;
  if (quad < T4)
    *reinterpret_cast<float4*>(dkW + g * NT + (size_t)n * T + 4 * quad) =
        make_float4(accX[0] - rsum * accP[0], accX[1] - rsum * accP[1], accX[2] - rsum * accP[2], accX[3] - rsum * accP[3]);
}

template <int T>
__global__ __launch_bounds__(kMgBlock) void k_map_grad_cols(const float* __restrict__ q, const float* __restrict__ kW,
                                                            const float* __restrict__ lse, const float* __restrict__ Wg,
                                                            const float* __restrict__ dP, const float* __restrict__ dkW,
                                                            const float* __restrict__ r, float* __restrict__ dq_add, int N,
                                                            int Bg) {
  constexpr int T4 = T / 4;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j = lane & 15, quad = lane >> 4;
  const int c0 = blockIdx.x * kMgSpan + 16 * wave;
  if (c0 >= N) return;   // the whole wave: there is no barrier below
  const size_t g = blockIdx.y;
  const size_t NT = (size_t)N * T;
  const float* kWg = kW + g * NT;
  const float* qg = q + g * NT;
  const int m = c0 + j, mr = min(m, N - 1);   // columns past N are clamped: their results are never written

  float qb[T4];
  score_frag_q<T>(qg, mr, quad, qb);
  const float* dPc = dP + g * N * N + mr;

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};   // [t = 4 quad + v][m = j]
  for (int nb = 0; nb < N; nb += 64) {
    float ka[4][T4], kv[4][4], d[4][4], lsj[4], rj[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int nt = nb + 16 * b;
      const int na = min(nt + j, N - 1);
      score_frag_kw<T>(kWg, na, quad, ka[b]);
      lsj[b] = lse[g * N + na];
      rj[b] = r[g * N + na];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int nv = min(nt + 4 * quad + v, N - 1);
        kv[b][v] = j < T ? kWg[(size_t)nv * T + j] : 0.f;
        d[b][v] = dPc[(size_t)nv * N];
      }
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int nt = nb + 16 * b;
      const f32x4 S = score_tile<T>(ka[b], qb);   // [n = 4 quad + v][m = j]
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float lv = __shfl(lsj[b], 4 * quad + v), rv = __shfl(rj[b], 4 * quad + v);   // lane i < 16 holds row nt + i
        const float ds = nt + 4 * quad + v < N ? fast_exp2(S[v] - lv) * (d[b][v] - rv) : 0.f;
        acc = mfma_16x16x4(kv[b][v], ds, acc);
      }
    }
  }
  if (m >= N || quad >= T4) return;
  // + dkW[m] Wg^T:  dq[m,t] += sum_s dkW[m,s] Wg[t,s]
  const float4* dk = reinterpret_cast<const float4*>(dkW + g * NT + (size_t)m * T);
  const float* Wr = Wg + (g / Bg) * (size_t)(T * T);
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const float4* w = reinterpret_cast<const float4*>(Wr + (4 * quad + v) * T);
    float a = acc[v];
#pragma unroll
    for (int s4 = 0; s4 < T4; ++s4) a = f4dot(dk[s4], w[s4], a);
    acc[v] = a;
  }
  float4* dst = reinterpret_cast<float4*>(dq_add + g * NT + (size_t)m * T + 4 * quad);
  float4 o = *dst;
  o.x += acc[0]; o.y += acc[1]; o.z += acc[2]; o.w += acc[3];
  *dst = o;
}

// part[g, c, t, s] = sum_{n in chunk c} q[g,n,t] dkW[g,n,s]: one thread per (t, s), its rows in ascending order
__global__ __launch_bounds__(kBlock) void k_map_grad_dwg(const float* __restrict__ q, const float* __restrict__ dkW,
                                                         float* __restrict__ part, int N, int T) {
  const int tid = threadIdx.x;
  if (tid >= T * T) return;
  const int t = tid / T, s = tid % T;
  const size_t g = blockIdx.y;
  const int n1 = min(N, ((int)blockIdx.x + 1) * kMgChunk);
  const float* qg = q + g * N * T;
  const float* dg = dkW + g * N * T;
  float acc = 0.f;
  for (int n = blockIdx.x * kMgChunk; n < n1; ++n) acc = fmaf(qg[(size_t)n * T + t], dg[(size_t)n * T + s], acc);
  part[(g * gridDim.x + blockIdx.x) * (size_t)(T * T) + tid] = acc;
}

// dWg_add[rel, t, s] += sum_{g in rel} sum_c part[g, c, t, s], in ascending (g, c)
__global__ __launch_bounds__(kBlock) void k_map_grad_dwg_sum(const float* __restrict__ part, float* __restrict__ dWg_add,
                                                             int J, int TT) {
  const int tid = threadIdx.x;
  if (tid >= TT) return;
  const float* p = part + (size_t)blockIdx.x * J * TT + tid;
  float acc = 0.f;
  for (int i = 0; i < J; ++i) acc += p[(size_t)i * TT];
  dWg_add[(size_t)blockIdx.x * TT + tid] += acc;
}

__global__ __launch_bounds__(kBlock) void k_add_into(float* __restrict__ dst, const float* __restrict__ src, size_t n) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) dst[i] += src[i];
}

int launch_add_into(float* dst, const float* src, size_t n, hipStream_t s) {
  if (n == 0) return MSGAT_OK;
  hipLaunchKernelGGL(k_add_into, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, dst, src, n);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

static inline size_t mg_align(size_t floats) { return (floats + 63) & ~(size_t)63; }

size_t map_grad_workspace_bytes(int G, int N, int T) {
  return 4 * (mg_align((size_t)G * N * T) + mg_align((size_t)G * N) + mg_align((size_t)G * cdiv(N, kMgChunk) * T * T));
}

int launch_map_grad(const float* q, const float* kW, const float* lse, const float* Wg, const float* dP, float* dq_add,
                    float* dWg_add, float* ws, int G, int Bg, int N, int T, hipStream_t s) {
  float* dkW = ws;
  float* r = dkW + mg_align((size_t)G * N * T);
  float* part = r + mg_align((size_t)G * N);
  const dim3 grid(cdiv(N, kMgSpan), G);
  const bool vec = (N & 3) == 0 && ((uintptr_t)dP & 15) == 0;
  const int st = dispatch_T(T, [&](auto t) -> int {
    constexpr int TT = decltype(t)::value;
    if (vec)
      hipLaunchKernelGGL((k_map_grad_rows<TT, true>), grid, dim3(kMgBlock), 0, s, q, kW, lse, dP, dkW, r, N);
    else
      hipLaunchKernelGGL((k_map_grad_rows<TT, false>), grid, dim3(kMgBlock), 0, s, q, kW, lse, dP, dkW, r, N);
    MSGAT_CHECK_LAUNCH();
    hipLaunchKernelGGL((k_map_grad_cols<TT>), grid, dim3(kMgBlock), 0, s, q, kW, lse, Wg, dP, dkW, r, dq_add, N, Bg);
    MSGAT_CHECK_LAUNCH();
    return MSGAT_OK;
  });
  if (st != MSGAT_OK) return st;
  const int nchunk = cdiv(N, kMgChunk);
  hipLaunchKernelGGL(k_map_grad_dwg, dim3(nchunk, G), dim3(kBlock), 0, s, q, dkW, part, N, T);
  MSGAT_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_map_grad_dwg_sum, dim3(G / Bg), dim3(kBlock), 0, s, part, dWg_add, Bg * nchunk, T * T);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

}  // namespace msgat
