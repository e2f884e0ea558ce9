// Hour- and day-dependent edge weights on one shared sparse pattern: w[b,e] = (base[e] + h_w[H[b]][e]) + d_w[D[b]][e].
//
//   torch ops            forward two embedding gathers and two adds; backward a batch sum, and per table a zero fill and an
//                        embedding scatter whose summation order torch does not promise.
//   here                 one launch each way; the gradients keep the ascending-sample-order contract.
//     k_edge_time_fwd    a lane per edge, a block row per sample: three coalesced reads, one coalesced store.  Plain fp32 adds
//                        in the order above (nothing to contract), so the result has the bits of the torch expression.
//     k_edge_time_bwd    a lane per edge, ONE pass over dout: the lane walks the samples in ascending order and adds
//                        dout[b,e] to its base sum (a register) and to the running sums of the two table rows sample b
//                        selected, which sit in an LDS column acc[row][lane] (a dynamic row index is an address in LDS; in
//                        registers it would be scratch).  Every sum starts at +0 and adds in sample order, every row of both
//                        tables is written (a row nobody selected is zero), nothing is atomic and nothing is read back;
//                        nothing is zeroed beforehand either: tests/test_gpu_poisoned_buffers.py::test_edge_weight_op
//                        pre-fills every output three ways and asks for equal bits.
//                        The samples' clamped rows are staged in LDS a tile of kEtSamples at a time, so any B takes the same
//                        path; a block keeps kEtRows table rows (hours first, then days: 31 for 24 + 7), more rows are
//                        further block rows that each re-read dout.
// A block of the backward is one wave: at the road graph's size (nnz ~ 2.6 K, B = 32) the launch is 41 waves of 32 dependent
// LDS updates each -- latency, not bandwidth -- and a wider block would only leave fewer compute units busy.
#include "edge_batch.hpp"

namespace msgat {

constexpr int kEtFwdBlock = 256;
constexpr int kEtLanes = 64;       // edges per block of the backward: one wave
constexpr int kEtRows = 32;        // table rows whose sums a block of the backward keeps in LDS (8 KiB)
constexpr int kEtSamples = 256;    // samples whose table rows are staged per tile
constexpr int kEtAhead = 8;        // samples of dout a lane loads before it adds them

__global__ __launch_bounds__(kEtFwdBlock) void k_edge_time_fwd(const float* __restrict__ base, const float* __restrict__ h_w,
                                                               const float* __restrict__ d_w, const long long* __restrict__ H,
                                                               const long long* __restrict__ D, float* __restrict__ out, int B,
                                                               long long nnz, int nh, int nd) {
  const long long e = (long long)blockIdx.x * kEtFwdBlock + threadIdx.x;
  if (e >= nnz) return;
  const float bv = base[e];
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    float v = bv + h_w[(long long)gate_row(H, b, nh) * nnz + e];
    if (d_w) v = v + d_w[(long long)gate_row(D, b, nd) * nnz + e];
    out[(long long)b * nnz + e] = v;
  }
}

// grid (edge tiles, row chunks): block row y owns the combined table rows [y * kEtRows, (y + 1) * kEtRows) of
// (h_w's nh rows, then d_w's nd rows); nh = 0 / nd = 0: that table gets no gradient.  Block row 0 also owns dbase.
__global__ __launch_bounds__(kEtLanes) void k_edge_time_bwd(const float* __restrict__ dout, const long long* __restrict__ H,
                                                            const long long* __restrict__ D, float* __restrict__ dbase,
                                                            float* __restrict__ dh_w, float* __restrict__ dd_w, int B,
                                                            long long nnz, int nh, int nd) {
  __shared__ float acc[kEtRows][kEtLanes];           // column `lane` belongs to this lane alone
  __shared__ int rows_h[kEtSamples], rows_d[kEtSamples];
  const int lane = threadIdx.x;
  const long long e = (long long)blockIdx.x * kEtLanes + lane;
  const int r0 = (int)blockIdx.y * kEtRows;
  const bool live = e < nnz;
#pragma unroll
  for (int r = 0; r < kEtRows; ++r) acc[r][lane] = 0.f;
  float base = 0.f;
  for (int b0 = 0; b0 < B; b0 += kEtSamples) {
    const int nb = B - b0 < kEtSamples ? B - b0 : kEtSamples;
    __syncthreads();                                 // the previous tile's rows have been consumed
    for (int i = lane; i < nb; i += kEtLanes) {      // a sample's row inside this block's chunk, or -1
      const int rh = nh > 0 ? gate_row(H, b0 + i, nh) - r0 : -1;
      const int rd = nd > 0 ? nh + gate_row(D, b0 + i, nd) - r0 : -1;
      rows_h[i] = (unsigned)rh < (unsigned)kEtRows ? rh : -1;
      rows_d[i] = (unsigned)rd < (unsigned)kEtRows ? rd : -1;
    }
    __syncthreads();
    if (live) {
      const float* src = dout + (long long)b0 * nnz + e;
      auto add = [&](float g, int i) {
        base += g;
        const int rh = __builtin_amdgcn_readfirstlane(rows_h[i]);   // the same for every lane: a scalar row offset
        const int rd = __builtin_amdgcn_readfirstlane(rows_d[i]);
        if (rh >= 0) acc[rh][lane] += g;
        if (rd >= 0) acc[rd][lane] += g;
      };
      for_samples_ahead<kEtAhead>(src, nnz, nb, add);   // kEtAhead loads in flight ahead of the dependent LDS updates
    }
  }
  if (!live) return;
  if (blockIdx.y == 0 && dbase) dbase[e] = base;
  const int total = nh + nd;
  for (int r = 0; r < kEtRows && r0 + r < total; ++r) {
    const int row = r0 + r;
    float* dst = row < nh ? dh_w + (long long)row * nnz : dd_w + (long long)(row - nh) * nnz;
    dst[e] = acc[r][lane];
  }
}

}  // namespace msgat

static int check_edge_time(int32_t B, int64_t nnz, int32_t nh, int32_t nd) {
  if (B < 0 || nnz < 0 || nh < 0 || nd < 0) return MSGAT_ERR_SHAPE;
  // the launches' grids: 64-edge tiles in x (a 31-bit count), sample rows / 32-row chunks in y (at most 65535)
  if (nnz > 0x7fffffffLL * msgat::kEtLanes || ((long long)nh + nd + msgat::kEtRows - 1) / msgat::kEtRows > 65535)
    return MSGAT_ERR_UNSUPPORTED;
  return MSGAT_OK;
}

extern "C" int msgat_edge_time_weights(const float* base, const float* h_w, const float* d_w, const int64_t* H,
                                       const int64_t* D, float* out, int32_t B, int64_t nnz, int32_t nh, int32_t nd,
                                       void* stream) {
  using namespace msgat;
  if (int st = check_edge_time(B, nnz, nh, nd)) return st;
  if (nnz == 0 || B == 0) return MSGAT_OK;
  if (!base || !h_w || !H || !out) return MSGAT_ERR_NULL;
  if ((d_w != nullptr) != (D != nullptr) || nh <= 0 || (d_w && nd <= 0)) return MSGAT_ERR_SHAPE;
  hipLaunchKernelGGL(k_edge_time_fwd, edge_sample_grid(nnz, kEtFwdBlock, B), dim3(kEtFwdBlock), 0, (hipStream_t)stream, base,
                     h_w, d_w, (const long long*)H, (const long long*)D, out, B, (long long)nnz, nh, d_w ? nd : 0);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

extern "C" int msgat_edge_time_weights_backward(const float* dout, const int64_t* H, const int64_t* D, float* dbase,
                                                float* dh_w, float* dd_w, int32_t B, int64_t nnz, int32_t nh, int32_t nd,
                                                void* stream) {
  using namespace msgat;
  if (int st = check_edge_time(B, nnz, nh, nd)) return st;
  if (nnz == 0) return MSGAT_OK;
  if (B > 0 && (!dout || (dh_w && !H) || (dd_w && !D))) return MSGAT_ERR_NULL;
  if (!dh_w) nh = 0;                                 // a table without an output: its rows are not summed
  if (!dd_w) nd = 0;
  if (!dbase && nh + nd == 0) return MSGAT_OK;
  const int chunks = (nh + nd + kEtRows - 1) / kEtRows;
  const dim3 grid((unsigned)((nnz + kEtLanes - 1) / kEtLanes), (unsigned)(chunks > 0 ? chunks : 1));
  hipLaunchKernelGGL(k_edge_time_bwd, grid, dim3(kEtLanes), 0, (hipStream_t)stream, dout, (const long long*)H,
                     (const long long*)D, dbase, dh_w, dd_w, B, (long long)nnz, nh, nd);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}
