// Gradient of a sparse adjacency's stored values (a learned weight per existing edge).
//
//   dval[e] = sum_g P_g[n_e,m_e] H_g[n_e,m_e],   H_g[n,m] = sum_{c,t} dv[g,c,n,t] feat[g,c,m,t]
//
// the dense gradient of adjacency_grad.hip restricted to the structure's edges, in CSR order.  Nothing [N,N] is read
// or written: P is re-created at the edge as 2^(kW_n . q_m log2 e - lse_n), the forward's k-ordered score sum in log2
// units, from what the forward saved; H is the backward SDDMM's gather, Cu rows of T floats of dv at the edge's row and
// of feat at its column.
//
// Four lanes own an edge (lane quad).  An edge's operands are Cu rows of T floats, Cu * T/4 16-B pieces in (channel, t)
// order; lane s takes pieces s, s + 4, ..., so the quad reads consecutive pieces: a row of T = 16 is one contiguous
// 64-B read, a row of T = 12 and the first piece of the next (lane s owning channels s, s + 4, ... was 5 % slower).
// A wave covers 16 edges, consecutive in CSR order, so the dv rows it reads are a few neighbouring rows per channel and
// the feat rows are gathered through the cache (a group's [Cu,N,T] slab is ~1 MB at PEMSD7 size).  The quad adds its
// four partial sums with two xor shuffles, a fixed order.  One [N,N] graph has few edges (2 615 at N = 883: 41 blocks of 64 edges),
// so the groups are split over blocks as in msgat_adjacency_grad: split j sums its groups in ascending order into the
// workspace and the library's reduction (k_reduce_few, k_reduce_partials past 16 splits) adds the splits in order.
// Deterministic, no atomics.  The split count is set by memory parallelism: 16 splits (about 10 waves per CU at the
// headline size) left the waves waiting on memory 44 % of their cycles; 48 were 9 % faster.
#include "common.hpp"

namespace msgat {

constexpr int kEwLanes = 4;                    // lanes per edge
constexpr int kEwEdges = kBlock / kEwLanes;    // edges per block
constexpr int kEwTargetBlocks = 4096;          // 16 blocks per CU on a 256-CU part before the groups are split
constexpr int kEwMaxSplit = 48;                // past 16, k_reduce_partials adds the splits (still in order)

template <int T>
__global__ __launch_bounds__(kBlock) void k_edge_weight_grad(
    const float* __restrict__ dv, size_t dv_gstride, const float* __restrict__ feat, const float* __restrict__ q,
    const float* __restrict__ kW, const float* __restrict__ lse, const int* __restrict__ erow,
    const int* __restrict__ col, float* __restrict__ out, int N, int nnz, int Cu, int G, int per) {
  constexpr int T4 = T / 4;
  const int sub = threadIdx.x & (kEwLanes - 1);
  const int e = blockIdx.x * kEwEdges + threadIdx.x / kEwLanes;
  const int ee = min(e, nnz - 1);              // lanes past the last edge compute on it and store nothing
  const int n = erow[ee], m = col[ee];
  const int g0 = blockIdx.y * per, g1 = min(G, g0 + per);
  const size_t NT = (size_t)N * T;

  float acc = 0.f;
  for (int g = g0; g < g1; ++g) {
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
    const float p = fast_exp2(s - lse[(size_t)g * N + n]);

    const float* dvr = dv + g * dv_gstride + (size_t)n * T;
    const float* fr = feat + (size_t)g * Cu * NT + (size_t)m * T;
    float h = 0.f;
    const int pieces = Cu * T4;
#pragma unroll 4
    for (int pc = sub; pc < pieces; pc += kEwLanes) {
      const int c = pc / T4, t = 4 * (pc - c * T4);
      const float4 a = *reinterpret_cast<const float4*>(dvr + c * NT + t);
      const float4 b = *reinterpret_cast<const float4*>(fr + c * NT + t);
      h = f4dot(a, b, h);
    }
    h += __shfl_xor(h, 1);
    h += __shfl_xor(h, 2);
    acc = fmaf(p, h, acc);
  }
  if (e < nnz && sub == 0) out[(size_t)blockIdx.y * nnz + e] = acc;
}

// groups split over `nsplit` blocks per edge tile, `per` consecutive groups each (no split is empty)
static void edge_weight_grad_split(int nnz, int G, int* nsplit, int* per) {
  const int tiles = cdiv(max(nnz, 1), kEwEdges);
  const int want = max(1, cdiv(kEwTargetBlocks, tiles));
  const int ns = min(min(G, kEwMaxSplit), want);
  *per = cdiv(G, ns);
  *nsplit = cdiv(G, *per);
}

size_t edge_weight_grad_workspace_bytes(int nnz, int G) {
  int nsplit, per;
  edge_weight_grad_split(nnz, G, &nsplit, &per);
  return nsplit > 1 ? sizeof(float) * (size_t)nsplit * nnz : 0;
}

int launch_edge_weight_grad(const float* dv, int dv_group_channels, const float* feat, const float* q, const float* kW,
                            const float* lse, const int* erow, const int* col, float* dval, float* ws, int G, int Cu,
                            int N, int nnz, int T, hipStream_t s) {
  if (nnz == 0) return MSGAT_OK;
  int nsplit, per;
  edge_weight_grad_split(nnz, G, &nsplit, &per);
  const size_t dv_gstride = (size_t)(dv_group_channels > 0 ? dv_group_channels : Cu) * N * T;
  float* out = nsplit > 1 ? ws : dval;
  const dim3 grid(cdiv(nnz, kEwEdges), nsplit);
#define MSGAT_EW(TT)                                                                                                 \
  hipLaunchKernelGGL(k_edge_weight_grad<TT>, grid, dim3(kBlock), 0, s, dv, dv_gstride, feat, q, kW, lse, erow, col, \
                     out, N, nnz, Cu, G, per)
  switch (T) {
    case 4: MSGAT_EW(4); break;
    case 8: MSGAT_EW(8); break;
    case 12: MSGAT_EW(12); break;
    case 16: MSGAT_EW(16); break;
    default: return MSGAT_ERR_UNSUPPORTED;
  }
#undef MSGAT_EW
  MSGAT_CHECK_LAUNCH();
  if (nsplit == 1) return MSGAT_OK;
  ReduceJobs jobs{};
  jobs.n = 1;
  jobs.job[0].part = ws;
  jobs.job[0].R = 1;
  jobs.job[0].J = nsplit;
  jobs.job[0].Wd = nnz;
  jobs.job[0].dst0 = dval;
  jobs.job[0].n0 = nnz;
  jobs.job[0].dst1 = nullptr;
  jobs.job[0].n1 = 0;
  return launch_reduce_jobs(jobs, s);
}

}  // namespace msgat
