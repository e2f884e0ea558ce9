// Validity-gated edges on one shared sparse pattern: out[v,e] = w[v,e] * g[v,col(e)], where g[v,n] = table[count[v,n]] and
// count[v,n] is the number of valid readings (val[v,n,t] > 0.5, a NaN is not counted) in node n's input window of sample v.
// A sensor that measured nothing stops sending messages: its outgoing edges carry +0 for that sample.
//
//   torch ops            forward a compare, a sum over T, a table gather, a [V,nnz] gather by column, a compare, a select and
//                        a multiply (plus a select for the exempt edges); backward the same gate again or kept in between, a
//                        multiply and a batch sum.
//   here                 one launch each way, no atomics, nothing stored in between, nothing zeroed beforehand (checked by
//                        tests/test_gpu_poisoned_buffers.py::test_edge_weight_op: outputs pre-filled three ways, equal
//                        bits), nothing read back.
//     k_edge_validity    a lane per edge, a block row per sample: the lane reads col(e) and exempt[e] once and walks its
//                        block row's samples; per sample the T validity floats of the source node arrive as T/4 16-byte
//                        pieces (kVec) or as T single loads (a base or sample stride that is not 16-byte aligned), the
//                        count picks its table entry through a chain of T selects -- the table travels by value and stays
//                        in scalar registers -- and dst = exempt ? src : (g == 0 ? +0 : src * g), one fp32 multiply.
//                        src is w (forward; src_sets = 0: [nnz] shared by the samples) or dout (backward of w [V,nnz]): the
//                        two are the same expression.
//     k_edge_validity_bwd_sum   w [nnz] shared by the samples: dw[e] = sum_v of those rounded terms under the
//                        ascending-sample-order contract.  The skeleton and tile constants of edge_batch_sum
//                        (edge_batch.hpp), a lane per (edge, sample), loads of dout coalesced along e -- written out: as
//                        edge_batch_sum<1> the pair's cold replay was slower than the parent's spread (lab_variants.txt).
// At the road graph's size (N = 883, nnz ~ 2.6 K, V = 32, T = 12) the validity windows are 1.4 MB and each node's row is read
// by its few out-edges: latency, not bandwidth.
#include "edge_batch.hpp"

namespace msgat {

constexpr int kGateBlock = 256;     // edges per block of the elementwise kernel

struct EvTable {
  float g[kMaxT + 1];
};

// table[count of val[0..T) > 0.5f]: row points at the T validity floats of one node of one sample
template <int T, bool kVec>
__device__ __forceinline__ float edge_validity_gate(const float* __restrict__ row, const EvTable& tb) {
  int count = 0;
  if (kVec) {
    const float4* p = reinterpret_cast<const float4*>(row);
    float4 x[T / 4];
#pragma unroll
    for (int k = 0; k < T / 4; ++k) x[k] = p[k];
#pragma unroll
    for (int k = 0; k < T / 4; ++k)
      count += (int)(x[k].x > 0.5f) + (int)(x[k].y > 0.5f) + (int)(x[k].z > 0.5f) + (int)(x[k].w > 0.5f);
  } else {
    float x[T];
#pragma unroll
    for (int t = 0; t < T; ++t) x[t] = row[t];
#pragma unroll
    for (int t = 0; t < T; ++t) count += (int)(x[t] > 0.5f);
  }
  float g = tb.g[0];
#pragma unroll
  for (int c = 1; c <= T; ++c) g = count == c ? tb.g[c] : g;
  return g;
}

__device__ __forceinline__ float edge_validity_term(float x, float g, bool exempt) {
  return exempt ? x : (g == 0.f ? 0.f : x * g);
}

template <int T, bool kVec>
__global__ __launch_bounds__(kGateBlock) void k_edge_validity(const int* __restrict__ col, const float* __restrict__ src,
                                                              int src_sets, const unsigned char* __restrict__ exempt,
                                                              const float* __restrict__ val, long long val_stride,
                                                              EvTable tb, float* __restrict__ dst, int V, int nnz) {
  const int e = (int)blockIdx.x * kGateBlock + threadIdx.x;
  if (e >= nnz) return;
  const long long node = (long long)col[e] * T;
  const bool ex = exempt != nullptr && exempt[e] != 0;
  const float shared = src_sets ? 0.f : src[e];
  for (int v = blockIdx.y; v < V; v += gridDim.y) {
    const long long at = (long long)v * nnz + e;
    const float x = src_sets ? src[at] : shared;
    const float g = edge_validity_gate<T, kVec>(val + (long long)v * val_stride + node, tb);
    dst[at] = edge_validity_term(x, g, ex);
  }
}

template <int T, bool kVec>
__global__ __launch_bounds__(kEbSumBlock) void k_edge_validity_bwd_sum(const int* __restrict__ col,
                                                                       const float* __restrict__ dout,
                                                                       const unsigned char* __restrict__ exempt,
                                                                       const float* __restrict__ val, long long val_stride,
                                                                       EvTable tb, float* __restrict__ dw, int V, int nnz) {
  __shared__ float term[kEbSumSamples][kEbSumEdges];
  const int tid = threadIdx.x;
  const int el = tid & (kEbSumEdges - 1);                          // this lane's edge inside the block
  const int sl = tid / kEbSumEdges;                                // and its first sample inside a tile
  const long long e = (long long)blockIdx.x * kEbSumEdges + el;
  const bool live = e < nnz;
  const long long node = live ? (long long)col[e] * T : 0;
  const bool ex = live && exempt != nullptr && exempt[e] != 0;
  float acc = 0.f;
  for (int v0 = 0; v0 < V; v0 += kEbSumSamples) {
    const int nv = V - v0 < kEbSumSamples ? V - v0 : kEbSumSamples;
    __syncthreads();                                               // the previous tile's terms have been added
    if (live) {
      for (int i = sl; i < nv; i += kEbSumBlock / kEbSumEdges) {
        const long long v = v0 + i;
        const float g = edge_validity_gate<T, kVec>(val + v * val_stride + node, tb);
        term[i][el] = edge_validity_term(dout[v * nnz + e], g, ex);
      }
    }
    __syncthreads();
    if (tid < kEbSumEdges && live)
      for (int i = 0; i < nv; ++i) acc += term[i][tid];            // rounded terms, added from +0 in sample order
  }
  if (tid < kEbSumEdges && live) dw[e] = acc;
}

}  // namespace msgat

static int check_edge_validity(const msgat_graph_t* graph, int32_t V, int32_t T, int64_t val_stride) {
  if (!graph) return MSGAT_ERR_NULL;
  if (V < 0 || T < 0 || val_stride < 0 || graph->n_nodes < 0 || graph->nnz < 0) return MSGAT_ERR_SHAPE;
  if (!msgat::t_supported(T)) return MSGAT_ERR_UNSUPPORTED;
  return MSGAT_OK;
}

// the elementwise kernel (forward, and the backward of w [V,nnz]) or, sum = true, the batch-summing backward; 16-byte
// pieces need an aligned base and sample stride (a node's row is T floats, T a multiple of 4)
static int run_edge_validity(bool sum, const msgat_graph_t* graph, const float* src, int src_sets, const uint8_t* exempt,
                             const float* val, int64_t val_stride, const float* table, float* dst, int32_t V, int32_t T,
                             void* stream) {
  using namespace msgat;
  EvTable tb = {};
  for (int c = 0; c <= T; ++c) tb.g[c] = table[c];
  const bool aligned = (reinterpret_cast<uintptr_t>(val) & 15) == 0 && (val_stride & 3) == 0;
  const int nnz = graph->nnz;
  const int* col = graph->col;
  const long long stride = val_stride;
  hipStream_t s = (hipStream_t)stream;
  auto launch = [&](auto t, auto vec) -> int {
    constexpr int kT = decltype(t)::value;
    constexpr bool kVec = decltype(vec)::value;
    if (sum)
      hipLaunchKernelGGL((k_edge_validity_bwd_sum<kT, kVec>), dim3((unsigned)cdiv(nnz, kEbSumEdges)), dim3(kEbSumBlock), 0, s,
                         col, src, exempt, val, stride, tb, dst, V, nnz);
    else
      hipLaunchKernelGGL((k_edge_validity<kT, kVec>), edge_sample_grid(nnz, kGateBlock, V), dim3(kGateBlock), 0, s, col, src,
                         src_sets, exempt, val, stride, tb, dst, V, nnz);
    MSGAT_CHECK_LAUNCH();
    return MSGAT_OK;
  };
  return dispatch_T(T, [&](auto t) { return aligned ? launch(t, std::true_type{}) : launch(t, std::false_type{}); });
}

extern "C" int msgat_edge_validity(const msgat_graph_t* graph, const float* w, const uint8_t* exempt, const float* val,
                                   int64_t val_stride, const float* table, float* out, int32_t V, int32_t T, int32_t w_sets,
                                   void* stream) {
  if (int st = check_edge_validity(graph, V, T, val_stride)) return st;
  if (V == 0 || graph->nnz == 0) return MSGAT_OK;
  if (!w || !val || !table || !out || !graph->col) return MSGAT_ERR_NULL;
  return run_edge_validity(false, graph, w, w_sets ? 1 : 0, exempt, val, val_stride, table, out, V, T, stream);
}

extern "C" int msgat_edge_validity_backward(const msgat_graph_t* graph, const float* dout, const uint8_t* exempt,
                                            const float* val, int64_t val_stride, const float* table, float* dw, int32_t V,
                                            int32_t T, int32_t w_sets, void* stream) {
  if (int st = check_edge_validity(graph, V, T, val_stride)) return st;
  if (V == 0 || graph->nnz == 0 || !dw) return MSGAT_OK;
  if (!dout || !val || !table || !graph->col) return MSGAT_ERR_NULL;
  return run_edge_validity(!w_sets, graph, dout, 1, exempt, val, val_stride, table, dw, V, T, stream);
}
