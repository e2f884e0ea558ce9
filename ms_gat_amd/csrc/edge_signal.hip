// Signal-dependent edge weights on one shared sparse pattern: w[b,e] = base[e] + sum_k a[b,row(e),k] * b[b,col(e),k], with
// ab [B,N,2d] the per-sample node projection (a = ab[..., :d] the row side, b = ab[..., d:] the column side).
//
//   torch ops              forward two [B,nnz,d] gathers, a product, a reduction and an add; backward a batch sum, two products
//                          and two index_add_ scatters whose summation order torch does not promise.
//   here                   one launch each way, no atomics, nothing zeroed beforehand (held to it by
//                          tests/test_gpu_poisoned_buffers.py::test_edge_weight_op: every output pre-filled three ways,
//                          equal bits), nothing read back.
//     k_edge_signal_fwd    a lane per edge, a block row per sample stripe: the lane reads its two node indices and base[e]
//                          once and walks the stripe's samples; per sample the two d-float rows arrive as 16-byte pieces.
//                          Each product is rounded, the products are added in ascending k and base[e] is added last, so
//                          the result has the bits of the torch expression base + (((p_0 + p_1) + p_2) + ...), p = a * b.
//     k_edge_signal_bwd    the first `node_blocks` block columns: a lane per (node, 16-byte piece of the node's 2d-float
//                          gradient row), a block row per sample stripe.  A piece of the row side walks the node's CSR row
//                          (rowptr, col) in ascending edge order, da += dout[b,e] * b[b,col(e)]; a piece of the column side
//                          walks the node's CSC column (colptr, crow, cperm) in ascending position, db += dout[b,cperm(p)] *
//                          a[b,crow(p)].  The lanes of one node are neighbours and store 2d contiguous floats; a node
//                          without edges stores +0.  A walk is serial in the node's degree: any degree is correct, a hub of
//                          hundreds is one slow lane group (left out: splitting long lists).
//                          The remaining block columns: a lane per edge, dbase[e] = +0 + dout[0,e] + dout[1,e] + ... in
//                          ascending b, additions only (the ascending-sample-order contract).
// At the road graph's size (N = 883, nnz ~ 2.6 K, B = 32, d = 8) ab is 1.8 MB and stays in L2; every list is a handful of
// dependent 16-byte reads -- latency, not bandwidth -- so the blocks are single waves spread over as many compute units as
// the shape gives.
#include "edge_batch.hpp"

namespace msgat {

constexpr int kEsLanes = 64;       // one wave per block, both ways
constexpr int kEsStripes = 8;      // block rows of the forward: sample b belongs to stripe b % rows
constexpr int kEsAhead = 8;        // samples of dout a dbase lane loads before it adds them
constexpr int kEsMaxRank = 32;

__global__ __launch_bounds__(kEsLanes) void k_edge_signal_fwd(const int* __restrict__ erow, const int* __restrict__ col,
                                                              const float* __restrict__ base, const float* __restrict__ ab,
                                                              float* __restrict__ out, int B, int N, int nnz, int d) {
#pragma clang fp contract(off)                       // a * b + s stays a rounded product and an add (hipcc fuses by default)
  const int e = (int)blockIdx.x * kEsLanes + threadIdx.x;
  if (e >= nnz) return;
  const int q = d >> 2;                              // 16-byte pieces per side
  const long long node = 2LL * d;                    // floats per node row of ab
  const long long ia = (long long)erow[e] * node, ib = (long long)col[e] * node + d;
  const float bv = base[e];
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const float* sample = ab + (long long)b * N * node;
    const float4* pa = reinterpret_cast<const float4*>(sample + ia);
    const float4* pb = reinterpret_cast<const float4*>(sample + ib);
    float s = -0.f;                                  // -0 + p = p for every p: the sum starts AT the first product
    for (int k = 0; k < q; ++k) {                    // rounded products added in ascending k, nothing contracted
      const float4 x = pa[k], y = pb[k];
      s = s + x.x * y.x;
      s = s + x.y * y.y;
      s = s + x.z * y.z;
      s = s + x.w * y.w;
    }
    out[(long long)b * nnz + e] = bv + s;
  }
}

// grid (node_blocks + edge_blocks, sample stripes).  dab == nullptr: node_blocks = 0; dbase == nullptr: edge_blocks = 0.
// The dbase columns exist in block row 0 only.
__global__ __launch_bounds__(kEsLanes) void k_edge_signal_bwd(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                              const int* __restrict__ colptr, const int* __restrict__ crow,
                                                              const int* __restrict__ cperm, const float* __restrict__ dout,
                                                              const float* __restrict__ ab, float* __restrict__ dbase,
                                                              float* __restrict__ dab, int B, int N, int nnz, int d,
                                                              int node_blocks) {
  if ((int)blockIdx.x >= node_blocks) {              // dbase: wave-uniform branch
    const int e = ((int)blockIdx.x - node_blocks) * kEsLanes + threadIdx.x;
    if (blockIdx.y != 0 || e >= nnz) return;
    float sum = 0.f;
    for_samples_ahead<kEsAhead>(dout + e, nnz, B, [&](float g, int) { sum += g; });
    dbase[e] = sum;
    return;
  }
  const int q = d >> 2;                              // pieces per side; a node row has 2 q pieces
  const long long t = (long long)blockIdx.x * kEsLanes + threadIdx.x;
  const int n = (int)(t / (2 * q)), piece = (int)(t % (2 * q));
  if (n >= N) return;
  const bool cols = piece >= q;                      // this piece belongs to db: walk the CSC column of n
  const long long node = 2LL * d;
  const int* ptr = cols ? colptr : rowptr;
  const int* other = cols ? crow : col;              // the node at the far end of each list entry
  const int p0 = ptr[n], p1 = ptr[n + 1];
  // the far end's piece: a row-side piece k reads b[., k] (offset d + 4k), a column-side piece q + k reads a[., k] (4k)
  const int far = cols ? (piece - q) * 4 : d + piece * 4;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const float* sample = ab + (long long)b * N * node;
    const float* g = dout + (long long)b * nnz;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p = p0; p < p1; ++p) {
      const float w = g[cols ? cperm[p] : p];
      const float4 x = *reinterpret_cast<const float4*>(sample + (long long)other[p] * node + far);
      acc.x = fmaf(w, x.x, acc.x);
      acc.y = fmaf(w, x.y, acc.y);
      acc.z = fmaf(w, x.z, acc.z);
      acc.w = fmaf(w, x.w, acc.w);
    }
    *reinterpret_cast<float4*>(dab + ((long long)b * N + n) * node + piece * 4) = acc;
  }
}

}  // namespace msgat

static int check_edge_signal(const msgat_graph_t* graph, int32_t B, int32_t d) {
  if (!graph) return MSGAT_ERR_NULL;
  if (B < 0 || d <= 0 || graph->n_nodes < 0 || graph->nnz < 0) return MSGAT_ERR_SHAPE;
  if (d % 4 != 0 || d > msgat::kEsMaxRank) return MSGAT_ERR_UNSUPPORTED;
  return MSGAT_OK;
}

extern "C" int msgat_edge_signal_weights(const msgat_graph_t* graph, const float* base, const float* ab, int32_t B, int32_t d,
                                         float* out, void* stream) {
  using namespace msgat;
  if (int st = check_edge_signal(graph, B, d)) return st;
  if (B == 0 || graph->nnz == 0) return MSGAT_OK;
  if (!base || !ab || !out || !graph->erow || !graph->col) return MSGAT_ERR_NULL;
  const dim3 grid((unsigned)((graph->nnz + kEsLanes - 1) / kEsLanes), (unsigned)(B < kEsStripes ? B : kEsStripes));
  hipLaunchKernelGGL(k_edge_signal_fwd, grid, dim3(kEsLanes), 0, (hipStream_t)stream, graph->erow, graph->col, base, ab, out,
                     B, graph->n_nodes, graph->nnz, d);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

extern "C" int msgat_edge_signal_weights_backward(const msgat_graph_t* graph, const float* dout, const float* ab, int32_t B,
                                                  int32_t d, float* dbase, float* dab, void* stream) {
  using namespace msgat;
  if (int st = check_edge_signal(graph, B, d)) return st;
  if (B == 0) return MSGAT_OK;
  const int N = graph->n_nodes, nnz = graph->nnz;
  if (nnz == 0) dbase = nullptr;                     // no edge: no dbase entry; dab is all zeros
  if (N == 0) dab = nullptr;
  if (!dbase && !dab) return MSGAT_OK;
  if (nnz > 0 && !dout) return MSGAT_ERR_NULL;
  if (dab && (!graph->rowptr || !graph->colptr || (nnz > 0 && (!ab || !graph->col || !graph->crow || !graph->cperm))))
    return MSGAT_ERR_NULL;
  const long long node_lanes = dab ? (long long)N * (d / 2) : 0;   // 2 d / 4 pieces per node
  const long long node_blocks = (node_lanes + kEsLanes - 1) / kEsLanes;
  const long long edge_blocks = dbase ? (nnz + kEsLanes - 1) / kEsLanes : 0;
  if (node_blocks + edge_blocks > 0x7fffffffLL) return MSGAT_ERR_UNSUPPORTED;
  // sample stripes: with a node gradient as many block rows as samples (one pass of every list per sample), else one
  const dim3 grid((unsigned)(node_blocks + edge_blocks), (unsigned)(dab ? (B < 65535 ? B : 65535) : 1));
  hipLaunchKernelGGL(k_edge_signal_bwd, grid, dim3(kEsLanes), 0, (hipStream_t)stream, graph->rowptr, graph->col, graph->colptr,
                     graph->crow, graph->cperm, dout, ab, dbase, dab, B, N, nnz, d, (int)node_blocks);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}
