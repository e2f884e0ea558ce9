// Online forecasting: the history of a growing series as a ring in device memory, and the input windows of the one
// forecast origin "now" built from it -- a reading goes in and X, H, D come out with no host arithmetic and no readback.
//
//   reference            data_loader.py:92-120 (TimeSeriesSlice and the z-score): windows are slices of a series that
//                        exists in full on the host, normalised once before training; the statistics are not kept, and
//                        there is no path for a reading that arrives afterwards.
//   here                 ring [L, C*N] fp32, TIME-MAJOR as the resident series of windows.hip: the row of absolute step s
//                        is s mod L.  clock [2] int64 in device memory: clock[0] the absolute index of the next reading
//                        (= the forecast origin t), clock[1] the count of readings held, saturating at L.
//     k_ring_push        a lane per (step k, row m) of raw [K, C*N]: ring[(clock[0] + k) mod L][m] = (raw - mean[m]) /
//                        std[m], one IEEE subtract and one correctly rounded divide (the bits of the torch expression the
//                        training series was normalised with); kNull: a reading that is NaN or equal to null_value is
//                        stored as the canonical NaN 0x7fc00000, which the window kernel takes for "missing".  Reads and
//                        stores are coalesced over m.
//     k_ring_advance     one thread: clock[0] += K, clock[1] = min(clock[1] + K, L).  It follows the push in stream order
//                        (the idiom of k_edge_dropout_advance), so no block of the push can see the new value.
//     k_ring_windows     k_window_gather / k_window_gather_imputed of windows.hip for ONE sample whose origin is clock[0],
//                        read on the device: a block owns 256 consecutive (channel, node) rows of one component, lane m
//                        reads its tau values (each read coalesced over the lanes) and stores them as tau / 4 16-byte
//                        stores; a validity lane reads the C words itself.  Step t - offsets[r] + k lives in row
//                        (t - offsets[r] + k) floor-mod L: the mod is taken once in 64 bits for k = 0 and carried per
//                        step (a window may straddle the end of the ring), the slot of a missing reading likewise from
//                        (absolute step) floor-mod period.  Block 0 also writes H and D.
// A floor-mod lies in [0, L) for ANY clock and offsets content (a cold ring, a negative t - offsets[r], a wild word): no
// launch can read outside ring or climatology or write outside ring, X, H, D.  Every offset is 64-bit.
#include "common.hpp"

namespace msgat {

constexpr int kRingBlock = 256;

__device__ __forceinline__ long long floor_mod_ll(long long a, long long n) {   // n > 0
  const long long r = a % n;
  return r < 0 ? r + n : r;
}

__device__ __forceinline__ long long floor_div_ll(long long a, long long n) {   // n > 0
  const long long d = a / n;
  return (a % n) < 0 ? d - 1 : d;
}

// two's-complement sum and difference: a wild clock word wraps instead of overflowing a signed type
__device__ __forceinline__ long long wrap_add_ll(long long a, long long b) {
  return (long long)((unsigned long long)a + (unsigned long long)b);
}

__device__ __forceinline__ long long wrap_sub_ll(long long a, long long b) {
  return (long long)((unsigned long long)a - (unsigned long long)b);
}

__device__ __forceinline__ bool ring_nan_word(unsigned w) { return (w & 0x7fffffffu) > 0x7f800000u; }

template <bool kNull>
__global__ __launch_bounds__(kRingBlock) void k_ring_push(const float* __restrict__ raw, const float* __restrict__ mean,
                                                          const float* __restrict__ std_,
                                                          unsigned* __restrict__ ring,
                                                          const long long* __restrict__ clock, int M, long long L,
                                                          int m_tiles, float null_value) {
#pragma clang fp contract(off)
  const int k = (int)(blockIdx.x / (unsigned)m_tiles);
  const int m = (int)(blockIdx.x - (unsigned)k * (unsigned)m_tiles) * kRingBlock + (int)threadIdx.x;
  if (m >= M) return;
  const long long row = floor_mod_ll(wrap_add_ll(clock[0], k), L);
  const float x = raw[(long long)k * M + m];
  const float d = x - mean[m];
  const float z = d / std_[m];
  unsigned w = __float_as_uint(z);
  if (kNull && (x != x || x == null_value)) w = 0x7fc00000u;
  ring[row * M + m] = w;
}

__global__ void k_ring_advance(long long* __restrict__ clock, long long K, long long L) {
  const long long held = clock[1] + K;
  clock[0] = wrap_add_ll(clock[0], K);
  clock[1] = held < L ? held : L;
}

// kTable: missing readings (NaN words) become the slot table's entry of their step; Mx = M + N then appends the
// validity rows.  Without it words move as they are and Mx == M.
template <int TAU, bool kTable>
__global__ __launch_bounds__(kRingBlock) void k_ring_windows(
    const unsigned* __restrict__ ring, const unsigned* __restrict__ climatology, const long long* __restrict__ clock,
    const long long* __restrict__ offsets, unsigned* __restrict__ X, long long* __restrict__ H,
    long long* __restrict__ D, int M, int Mx, int N, long long L, int period, int x_tiles) {
  const long long t = clock[0];
  const int r = (int)(blockIdx.x / (unsigned)x_tiles);          // component
  const int tile = (int)(blockIdx.x - (unsigned)r * (unsigned)x_tiles);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const long long hour = floor_div_ll(t, TAU);
    H[0] = floor_mod_ll(hour, 24);
    D[0] = floor_mod_ll(floor_div_ll(hour, 24), 7);
  }
  const int m = tile * kRingBlock + (int)threadIdx.x;
  if (m >= Mx) return;
  const long long s0 = wrap_sub_ll(t, offsets[r]);              // absolute step of the window's first reading
  const long long row0 = floor_mod_ll(s0, L);
  long long rows[TAU];                                          // row of step s0 + k: L >= TAU, so one wrap at most
#pragma unroll
  for (int k = 0; k < TAU; ++k) rows[k] = row0 + k < L ? row0 + k : row0 + k - L;
  unsigned v[TAU];
  if (m < M) {
#pragma unroll
    for (int k = 0; k < TAU; ++k) v[k] = ring[rows[k] * M + m];
    if (kTable) {
      const unsigned slot0 = (unsigned)floor_mod_ll(s0, period);
#pragma unroll
      for (int k = 0; k < TAU; ++k)
        if (ring_nan_word(v[k])) v[k] = climatology[(long long)((slot0 + k) % (unsigned)period) * M + m];
    }
  } else {                                                      // kTable only: the validity row of node m - M
#pragma unroll
    for (int k = 0; k < TAU; ++k) v[k] = 0x3f800000u;
    for (int c = m - M; c < M; c += N) {
#pragma unroll
      for (int k = 0; k < TAU; ++k)
        if (ring_nan_word(ring[rows[k] * M + c])) v[k] = 0u;
    }
  }
  uint4* dst = reinterpret_cast<uint4*>(X + ((long long)r * Mx + m) * TAU);     // 16-byte aligned: TAU % 4 == 0
#pragma unroll
  for (int k = 0; k < TAU; k += 4) dst[k / 4] = make_uint4(v[k], v[k + 1], v[k + 2], v[k + 3]);
}

}  // namespace msgat

extern "C" int msgat_ring_push(const float* raw, const float* mean, const float* std_, float* ring, int64_t* clock,
                               int32_t K, int32_t C, int32_t N, int64_t L, int32_t has_null, float null_value,
                               void* stream) {
  using namespace msgat;
  if (!raw || !mean || !std_ || !ring || !clock) return MSGAT_ERR_NULL;
  if (K <= 0 || C <= 0 || N <= 0 || L <= 0 || (int64_t)K > L) return MSGAT_ERR_SHAPE;
  if ((long long)C * N > 0x7fffff00LL) return MSGAT_ERR_UNSUPPORTED;       // C * N plus a tile is held in an int
  const int M = C * N;
  const int m_tiles = (M + kRingBlock - 1) / kRingBlock;
  const long long blocks = (long long)K * m_tiles;
  if (blocks > 0x7fffffffLL) return MSGAT_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)blocks), block(kRingBlock);
  if (has_null)
    hipLaunchKernelGGL(k_ring_push<true>, grid, block, 0, (hipStream_t)stream, raw, mean, std_,
                       reinterpret_cast<unsigned*>(ring), (const long long*)clock, M, (long long)L, m_tiles, null_value);
  else
    hipLaunchKernelGGL(k_ring_push<false>, grid, block, 0, (hipStream_t)stream, raw, mean, std_,
                       reinterpret_cast<unsigned*>(ring), (const long long*)clock, M, (long long)L, m_tiles, null_value);
  MSGAT_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_ring_advance, dim3(1), dim3(1), 0, (hipStream_t)stream, (long long*)clock, (long long)K,
                     (long long)L);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

extern "C" int msgat_ring_windows(const float* ring, const float* climatology_or_null, const int64_t* clock,
                                  const int64_t* offsets, float* X, int64_t* H, int64_t* D, int32_t R, int32_t C,
                                  int32_t N, int64_t L, int32_t tau, int32_t period, int32_t mask_channel,
                                  void* stream) {
  using namespace msgat;
  if (!ring || !clock || !offsets || !X || !H || !D) return MSGAT_ERR_NULL;
  if (R <= 0 || C <= 0 || N <= 0 || L <= 0 || tau <= 0 || L % tau != 0) return MSGAT_ERR_SHAPE;
  if (climatology_or_null ? period < 1 : mask_channel != 0) return MSGAT_ERR_SHAPE;
  if (((long long)C + 1) * N > 0x7fffff00LL) return MSGAT_ERR_UNSUPPORTED;  // (C + 1) * N plus a tile is held in an int
  const int M = C * N, Mx = mask_channel ? M + N : M;
  const int x_tiles = (Mx + kRingBlock - 1) / kRingBlock;
  const long long blocks = (long long)R * x_tiles;
  if (blocks > 0x7fffffffLL) return MSGAT_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)blocks), block(kRingBlock);
  return dispatch_T(tau, [&](auto t) -> int {
    constexpr int TAU = decltype(t)::value;
    const unsigned* ring_w = reinterpret_cast<const unsigned*>(ring);
    const unsigned* table_w = reinterpret_cast<const unsigned*>(climatology_or_null);
    unsigned* X_w = reinterpret_cast<unsigned*>(X);
    if (climatology_or_null)
      hipLaunchKernelGGL((k_ring_windows<TAU, true>), grid, block, 0, (hipStream_t)stream, ring_w, table_w,
                         (const long long*)clock, (const long long*)offsets, X_w, (long long*)H, (long long*)D, M, Mx, N,
                         (long long)L, (int)period, x_tiles);
    else
      hipLaunchKernelGGL((k_ring_windows<TAU, false>), grid, block, 0, (hipStream_t)stream, ring_w, table_w,
                         (const long long*)clock, (const long long*)offsets, X_w, (long long*)H, (long long*)D, M, Mx, N,
                         (long long)L, 1, x_tiles);
    MSGAT_CHECK_LAUNCH();
    return MSGAT_OK;
  });
}
