// Gradient of the adjacency (the `att * adjacency` of attention.py:36 when the adjacency requires grad).
//
//   z[g,c,n,:] = sum_m P_g[n,m] A[n,m] feat[g,c,m,:]      P_g = softmax(S_g) over ALL N columns, S_g = kW_g q_g^T
//   dA[v,n,m]  = sum_{g : g % n_sets == v}  P_g[n,m] H_g[n,m],    H_g[n,m] = sum_{c,t} dv[g,c,n,t] feat[g,c,m,t]
//
// P does not depend on A, so the gradient is dense: it is written for every (n, m), edge or not.  P is re-created
// from what the forward saved (q, kW, lse in log2 units; softmax_recreate.hpp), the way k_bwd_dense_col7 does: nothing
// [N,N] is stored.
//
// A block owns a 64 x 64 output tile and a contiguous range of the groups of one value set; its 4 waves own 32 x 32
// quadrants (2 x 2 tiles of 16 x 16).  Per group, both products run on v_mfma_f32_16x16x4_f32:
//   S  T/4 MFMAs per tile (score_tile, A = kW rows, B = q rows: the forward's k-ordered chain, the same score bits)
//   H  Cu*T/4 MFMAs per tile, chained.  The contraction runs over (c, t) in any order, so a staged step of 4 channels
//      gives lane quad k channel k: MFMA s of the step takes t = s.  A lane then reads its A and B fragments of four
//      MFMAs with ONE ds_read_b128 each, and the block stages dv rows / feat rows as plain 16-B loads of [T] rows.
// then dA += exp2(S - lse) * H on the accumulators.  Staging is double buffered through registers: the next step's
// rows are in flight while the current one multiplies.
//
// Deterministic, no atomics: a block sums its groups in ascending order; when the tile grid alone is too small for the
// chip (one [N,N] adjacency: 196 tiles at N = 883) the groups are split over up to kAgMaxSplit blocks per tile, each
// writes its partial sum to the workspace, and k_reduce_partials / k_reduce_few add the partials in split order.
#include "softmax_recreate.hpp"

namespace msgat {

constexpr int kAgWaves = 4;
constexpr int kAgBlock = 64 * kAgWaves;
constexpr int kAgTile = 64;          // output rows = columns per block
constexpr int kAgCh = 4;             // channels per staged step: one per lane quad
constexpr int kAgTargetBlocks = 1024;   // 4 blocks per CU on a 256-CU part before the groups are split
constexpr int kAgMaxSplit = 16;      // the partial sums stay in k_reduce_few's one-lane-per-column form

__device__ __forceinline__ float f4get(const float4& v, int e) {
  return e == 0 ? v.x : (e == 1 ? v.y : (e == 2 ? v.z : v.w));
}

template <int T>
__global__ __launch_bounds__(kAgBlock) void k_adjacency_grad(
    const float* __restrict__ dv, size_t dv_gstride, const float* __restrict__ feat, const float* __restrict__ q,
    const float* __restrict__ kW, const float* __restrict__ lse, float* __restrict__ out, int N, int Cu, int V,
    int Gs, int per, int nsplit) {
  constexpr int T4 = T / 4;
  constexpr int RS = kAgCh * T + 4;   // floats per staged row: 4 channels of T, + 4 against bank conflicts
  __shared__ float4 sa4[kAgTile * RS / 4];
  __shared__ float4 sb4[kAgTile * RS / 4];
  const float* sa = reinterpret_cast<const float*>(sa4);
  const float* sb = reinterpret_cast<const float*>(sb4);

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int j = lane & 15, quad = lane >> 4;
  const int n0 = blockIdx.y * kAgTile, m0 = blockIdx.x * kAgTile;
  const int v = blockIdx.z / nsplit, sp = blockIdx.z - v * nsplit;
  const int k0 = sp * per, k1 = min(Gs, k0 + per);
  const size_t NT = (size_t)N * T;
  const int nch = cdiv(Cu, kAgCh);
  const int nstep = max(k1 - k0, 0) * nch;

  // staging role: tile row sr of channel sq of the step (rows past N are clamped: they only feed outputs never written)
  const int sr = tid & 63, sq = tid >> 6;
  const size_t arow = (size_t)min(n0 + sr, N - 1) * T, brow = (size_t)min(m0 + sr, N - 1) * T;
  float4 pa[T4], pb[T4];
  auto fetch = [&](int step) {
    const int k = k0 + step / nch, c = (step % nch) * kAgCh + sq;
    const int g = v + V * k;
    const bool live = c < Cu;
    const int cc = live ? c : 0;
    const float4* ap = reinterpret_cast<const float4*>(dv + g * dv_gstride + cc * NT + arow);
    const float4* bp = reinterpret_cast<const float4*>(feat + ((size_t)g * Cu + cc) * NT + brow);
#pragma unroll
    for (int t4 = 0; t4 < T4; ++t4) {
      pa[t4] = live ? ap[t4] : f4zero();
      pb[t4] = live ? bp[t4] : f4zero();
    }
  };

  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
  int rrow[2], rcol[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    rrow[h] = min(n0 + wr + 16 * h + j, N - 1);   // this lane's A row of the score product
    rcol[h] = min(m0 + wc + 16 * h + j, N - 1);   // and its B column
  }
  f32x4 acc[2][2], H[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  float ka[2][T4], qb[2][T4], ls[2][4];

  if (nstep > 0) fetch(0);
  for (int st = 0; st < nstep; ++st) {
    const int ch = st % nch;
    __syncthreads();   // the previous step's fragments have been read
    {
      float4* da = sa4 + (sr * RS + sq * T) / 4;
      float4* db = sb4 + (sr * RS + sq * T) / 4;
#pragma unroll
      for (int t4 = 0; t4 < T4; ++t4) { da[t4] = pa[t4]; db[t4] = pb[t4]; }
    }
    __syncthreads();
    if (ch == 0) {
      // the group's score operands, requested now and used after its last step
      const int g = v + V * (k0 + st / nch);
      const float* kWg = kW + (size_t)g * NT;
      const float* qg = q + (size_t)g * NT;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        score_frags<T>(kWg, rrow[h], qg, rcol[h], quad, ka[h], qb[h]);
#pragma unroll
        for (int r = 0; r < 4; ++r) ls[h][r] = lse[(size_t)g * N + min(n0 + wr + 16 * h + 4 * quad + r, N - 1)];
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) H[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (st + 1 < nstep) fetch(st + 1);

#pragma unroll
    for (int s4 = 0; s4 < T4; ++s4) {
      float4 fa[2], fb[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        fa[h] = *reinterpret_cast<const float4*>(sa + (wr + 16 * h + j) * RS + quad * T + 4 * s4);
        fb[h] = *reinterpret_cast<const float4*>(sb + (wc + 16 * h + j) * RS + quad * T + 4 * s4);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) H[a][b] = mfma_16x16x4(f4get(fa[a], e), f4get(fb[b], e), H[a][b]);
    }

    if (ch == nch - 1) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const f32x4 S = score_tile<T>(ka[a], qb[b]);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[a][b][r] += fast_exp2(S[r] - ls[a][r]) * H[a][b][r];
        }
    }
  }

  float* o = out + (size_t)blockIdx.z * N * N;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int m = m0 + wc + 16 * b + j;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wr + 16 * a + 4 * quad + r;
        if (n < N && m < N) o[(size_t)n * N + m] = acc[a][b][r];
      }
    }
}

// groups of a value set split over `nsplit` blocks per tile
static void adjacency_grad_split(int N, int G, int V, int* nsplit, int* per) {
  group_split(cdiv(N, kAgTile) * cdiv(N, kAgTile) * V, G / V, kAgTargetBlocks, kAgMaxSplit, nsplit, per);
}

size_t adjacency_grad_workspace_bytes(int N, int G, int V) {
  int nsplit, per;
  adjacency_grad_split(N, G, V, &nsplit, &per);
  return nsplit > 1 ? sizeof(float) * (size_t)V * nsplit * N * N : 0;
}

int launch_adjacency_grad(const float* dv, int dv_group_channels, const float* feat, const float* q, const float* kW,
                          const float* lse, float* dadj, float* ws, int G, int V, int Cu, int N, int T, hipStream_t s) {
  int nsplit, per;
  adjacency_grad_split(N, G, V, &nsplit, &per);
  const size_t dv_gstride = (size_t)(dv_group_channels > 0 ? dv_group_channels : Cu) * N * T;
  float* out = nsplit > 1 ? ws : dadj;
  const dim3 grid(cdiv(N, kAgTile), cdiv(N, kAgTile), V * nsplit);
  const int st = dispatch_T(T, [&](auto t) -> int {
    hipLaunchKernelGGL(k_adjacency_grad<decltype(t)::value>, grid, dim3(kAgBlock), 0, s, dv, dv_gstride, feat, q, kW, lse,
                       out, N, Cu, V, G / V, per, nsplit);
    MSGAT_CHECK_LAUNCH();
    return MSGAT_OK;
  });
  if (st != MSGAT_OK || nsplit == 1) return st;
  return launch_reduce_groups(ws, V, nsplit, N * N, dadj, s);
}

}  // namespace msgat
