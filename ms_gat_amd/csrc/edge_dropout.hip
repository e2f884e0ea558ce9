// Edge dropout on one shared sparse pattern: out[v,e] = w[v,e] * m[v,e], m = 0 (dropped), scale = 1/(1-p) (kept) or 1
// (exempt), the mask drawn from a counter-based generator so that nothing about it has to be stored or read back.
//
//   torch ops            forward a uniform draw, a compare, a select and a multiply; backward a multiply and a batch sum; the
//                        draw comes from torch's own generator, whose offset a sharded batch does not share with the whole one.
//   here                 Philox4x32-10 (Random123 constants): edge e of global sample s at step t under seed k reads word e & 3
//                        of philox(counter = (e >> 2, s, t lo, t hi), key = (k lo, k hi)) and is dropped iff word < thr.
//     k_edge_dropout     a lane per QUAD of four consecutive edges (one Philox call serves them), a block row per sample;
//                        kBackward = false writes out = kept ? w * scale : +0 (exempt: w), kBackward = true writes
//                        dw = dout * m, one fp32 multiply.  seed and step come from device memory: `state` {seed, step} for
//                        the forward, which leaves the step it drew from in `used`; seed and `used` for the backward, so two
//                        forwards followed by their two backwards each see their own masks.
//     k_edge_dropout_advance   one thread: state.step += 1.  It follows the forward in stream order, so every block of the
//                        forward has read the step before it moves; no ticket, no counter to reset, nothing read back.
//     k_edge_dropout_bwd_sum   w [nnz] shared by the samples: dw[e] = sum_v dout[v,e] * m[v,e] under the
//                        ascending-sample-order contract, as edge_batch_sum (edge_batch.hpp) with a unit of one
//                        quad: a lane per (quad, sample) forms four rounded products from one Philox call and four loads.
//                        The generator's ~80 integer operations per call are spread over the block that way, not chained
//                        4 V deep in front of one lane's sum.
#include "edge_batch.hpp"

namespace msgat {

constexpr int kEdBlock = 256;       // quads per block of the elementwise kernel: 1024 edges

struct Philox4 {
  uint32_t w[4];
};

// Philox4x32-10, Random123: ten rounds, the key bumped between rounds
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// the multipliers of quad `quad` of global sample `s`: +0 dropped, `scale` kept, 1 exempt (ex: the quad's four flags)
__device__ __forceinline__ void edge_dropout_quad(uint32_t quad, uint32_t s, unsigned long long seed, unsigned long long step,
                                                  uint32_t thr, float scale, const bool ex[4], float m[4]) {
  const Philox4 r = philox4x32_10(quad, s, (uint32_t)step, (uint32_t)(step >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
  for (int k = 0; k < 4; ++k) m[k] = ex[k] ? 1.f : (r.w[k] < thr ? 0.f : scale);
}

// src: w (kBackward = false; src_sets = 0: [nnz] shared by the samples) or dout [V,nnz]; step_src: state + 1 or `used`
template <bool kBackward>
__global__ __launch_bounds__(kEdBlock) void k_edge_dropout(const float* __restrict__ src, int src_sets,
                                                           const unsigned char* __restrict__ exempt,
                                                           const long long* __restrict__ state,
                                                           const long long* __restrict__ step_src, long long* __restrict__ used,
                                                           float* __restrict__ dst, int V, long long nnz,
                                                           uint32_t sample_offset, uint32_t thr, float scale) {
  const unsigned long long seed = (unsigned long long)state[0], step = (unsigned long long)step_src[0];
  if (!kBackward && used != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) used[0] = (long long)step;
  const long long quad = (long long)blockIdx.x * kEdBlock + threadIdx.x;
  const long long e0 = quad * 4;
  if (e0 >= nnz) return;
  const int n = nnz - e0 < 4 ? (int)(nnz - e0) : 4;
  bool ex[4];
  float shared[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    ex[k] = exempt != nullptr && k < n && exempt[e0 + k] != 0;
    shared[k] = (!src_sets && k < n) ? src[e0 + k] : 0.f;
  }
  for (int v = blockIdx.y; v < V; v += gridDim.y) {
    float m[4];
    edge_dropout_quad((uint32_t)quad, sample_offset + (uint32_t)v, seed, step, thr, scale, ex, m);
    const long long row = (long long)v * nnz + e0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= n) break;
      const float x = src_sets ? src[row + k] : shared[k];
      if (kBackward) dst[row + k] = x * m[k];
      else dst[row + k] = ex[k] ? x : (m[k] != 0.f ? x * scale : 0.f);
    }
  }
}

__global__ void k_edge_dropout_advance(long long* __restrict__ state) { state[1] = state[1] + 1; }

__global__ __launch_bounds__(kEbSumBlock) void k_edge_dropout_bwd_sum(const float* __restrict__ dout,
                                                                      const unsigned char* __restrict__ exempt,
                                                                      const long long* __restrict__ state,
                                                                      const long long* __restrict__ used,
                                                                      float* __restrict__ dw, int V, long long nnz,
                                                                      uint32_t sample_offset, uint32_t thr, float scale) {
  const unsigned long long seed = (unsigned long long)state[0], step = (unsigned long long)used[0];
  // this lane's quad, as edge_batch_sum<4> assigns it: its four flags are read once
  const long long q0 = (long long)blockIdx.x * kEbSumEdges + 4 * (threadIdx.x & (kEbSumEdges / 4 - 1));
  bool ex[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) ex[k] = exempt != nullptr && q0 + k < nnz && exempt[q0 + k] != 0;
  edge_batch_sum<4>(dw, V, nnz, [&](long long e0, int n, int v, float* dst) {
    float m[4];
    edge_dropout_quad((uint32_t)(e0 >> 2), sample_offset + (uint32_t)v, seed, step, thr, scale, ex, m);
    const long long row = (long long)v * nnz + e0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n) dst[k] = dout[row + k] * m[k];
  });
}

}  // namespace msgat

static int check_edge_dropout(int32_t V, int64_t nnz, int64_t sample_offset) {
  if (V < 0 || nnz < 0 || sample_offset < 0) return MSGAT_ERR_SHAPE;
  // the counter's words: e >> 2 and the global sample index are 32 bits each
  if (nnz >= (1LL << 34) || sample_offset + (int64_t)V > (1LL << 32)) return MSGAT_ERR_UNSUPPORTED;
  return MSGAT_OK;
}

extern "C" int msgat_edge_dropout(const float* w, const uint8_t* exempt, int64_t* state, int64_t* used, float* out, int32_t V,
                                  int64_t nnz, int32_t w_sets, int64_t sample_offset, uint32_t thr, float scale,
                                  int32_t advance, void* stream) {
  using namespace msgat;
  if (int st = check_edge_dropout(V, nnz, sample_offset)) return st;
  if (V == 0 || nnz == 0) return MSGAT_OK;              // nothing is drawn: `used` is not written and the step stays
  if (!w || !state || !used || !out) return MSGAT_ERR_NULL;
  hipLaunchKernelGGL(k_edge_dropout<false>, edge_sample_grid((nnz + 3) / 4, kEdBlock, V), dim3(kEdBlock), 0,
                     (hipStream_t)stream, w, w_sets ? 1 : 0, exempt, (const long long*)state, (const long long*)state + 1,
                     (long long*)used, out, V, (long long)nnz, (uint32_t)sample_offset, thr, scale);
  MSGAT_CHECK_LAUNCH();
  if (advance) {
    hipLaunchKernelGGL(k_edge_dropout_advance, dim3(1), dim3(1), 0, (hipStream_t)stream, (long long*)state);
    MSGAT_CHECK_LAUNCH();
  }
  return MSGAT_OK;
}

extern "C" int msgat_edge_dropout_backward(const float* dout, const uint8_t* exempt, const int64_t* state, const int64_t* used,
                                           float* dw, int32_t V, int64_t nnz, int32_t w_sets, int64_t sample_offset,
                                           uint32_t thr, float scale, void* stream) {
  using namespace msgat;
  if (int st = check_edge_dropout(V, nnz, sample_offset)) return st;
  if (V == 0 || nnz == 0 || !dw) return MSGAT_OK;
  if (!dout || !state || !used) return MSGAT_ERR_NULL;
  if (w_sets) {
    hipLaunchKernelGGL(k_edge_dropout<true>, edge_sample_grid((nnz + 3) / 4, kEdBlock, V), dim3(kEdBlock), 0,
                       (hipStream_t)stream, dout, 1, exempt, (const long long*)state, (const long long*)used,
                       (long long*)nullptr, dw, V, (long long)nnz, (uint32_t)sample_offset, thr, scale);
  } else {
    const dim3 grid((unsigned)((nnz + kEbSumEdges - 1) / kEbSumEdges));
    hipLaunchKernelGGL(k_edge_dropout_bwd_sum, grid, dim3(kEbSumBlock), 0, (hipStream_t)stream, dout, exempt,
                       (const long long*)state, (const long long*)used, dw, V, (long long)nnz, (uint32_t)sample_offset, thr,
                       scale);
  }
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}
