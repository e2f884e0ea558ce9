// Input windows built on the device: one launch turns B forecast origins into the (X, H, D, Y) batch of a step.
//
//   reference            data_loader.py:92-115 (TimeSeriesSlice): per sample a torch.stack of R strided slices of the
//                        [C,N,T_total] series in Python, collated B at a time on the host, pinned and copied over.
//   here                 k_window_gather: the series stays in device memory, TIME-MAJOR [T_total, C*N]; a block owns 256
//                        consecutive (channel, node) rows of one (sample, component): lane m reads series[t0 + k][m] for
//                        the tau steps (each read coalesced over the lanes) and stores its tau consecutive floats of
//                        X[b,r] = [C*N, tau] as tau / 4 16-byte stores; a block's output is one contiguous piece of X.
//                        The target stays [N, T_total] as the host keeps it: one lane per element of Y[b] = [N, q]
//                        (coalesced stores, 4q-byte read runs; Y is 1/15 of the bytes at the PEMSD7 shape).  The first
//                        target block of a sample also writes H[b] and D[b].
//                        k_window_gather_imputed: the same for a series that stores its missing readings as NaN -- such
//                        a word becomes the slot table's entry of its step, and X can gain a validity channel.
// Values move as 32-bit words: in k_window_gather a NaN of the series keeps its bits.  Every offset is 64-bit.
#include "common.hpp"

namespace msgat {

constexpr int kWinBlock = 256;

__device__ __forceinline__ long long clamp_ll(long long v, long long lo, long long hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

template <int TAU>
__global__ __launch_bounds__(kWinBlock) void k_window_gather(
    const unsigned* __restrict__ series, const unsigned* __restrict__ target, const long long* __restrict__ origins,
    const long long* __restrict__ offsets, unsigned* __restrict__ X, long long* __restrict__ H, long long* __restrict__ D,
    unsigned* __restrict__ Y, int R, int M, int N, long long T_total, int q, long long history, int x_tiles,
    long long x_items, int y_tiles, long long items) {
  for (long long w = blockIdx.x; w < items; w += gridDim.x) {
    if (w < x_items) {
      const long long br = w / x_tiles;                       // sample * R + component
      const int tile = (int)(w - br * x_tiles);
      const long long b = br / R;
      const int r = (int)(br - b * R);
      const long long t = clamp_ll(origins[b], history, T_total - q);
      // offsets[r] <= history by contract; the second clamp keeps a table that breaks it inside the series too
      const long long t0 = clamp_ll(t - offsets[r], 0, T_total - TAU);
      const int m = tile * kWinBlock + (int)threadIdx.x;
      if (m < M) {
        const unsigned* src = series + t0 * M + m;
        unsigned v[TAU];
#pragma unroll
        for (int k = 0; k < TAU; ++k) v[k] = src[(long long)k * M];
        uint4* dst = reinterpret_cast<uint4*>(X + (br * M + m) * TAU);    // 16-byte aligned: TAU % 4 == 0
#pragma unroll
        for (int k = 0; k < TAU; k += 4) dst[k / 4] = make_uint4(v[k], v[k + 1], v[k + 2], v[k + 3]);
      }
    } else {
      const long long yy = w - x_items;
      const long long b = yy / y_tiles;
      const int tile = (int)(yy - b * y_tiles);
      const long long t = clamp_ll(origins[b], history, T_total - q);
      const int e = tile * kWinBlock + (int)threadIdx.x;      // n * q + j
      if (e < N * q) {
        const int n = e / q, j = e - n * q;
        Y[b * N * q + e] = target[(long long)n * T_total + t + j];
      }
      if (tile == 0 && threadIdx.x == 0) {
        const long long hour = t / TAU;
        H[b] = hour % 24;
        D[b] = (hour / 24) % 7;
      }
    }
  }
}

__device__ __forceinline__ bool is_nan_word(unsigned w) { return (w & 0x7fffffffu) > 0x7f800000u; }

// k_window_gather with the missing readings of X filled in: the series stores a missing reading as a NaN, and such a
// word is replaced by the table entry of its step, climatology[(t0 + k) % period][m] ([period, C*N], read for missing
// entries only); every other word keeps its bits.  With Mx = (C + 1) * N > M = C * N the rows m in [M, Mx) of a
// (sample, component) are the validity channel: 1.0f where all C channels of node m - M at that step are observed,
// else 0.0f -- the lane reads the C words itself.  Same ownership, clamps and stores as above; H, D and Y likewise.
template <int TAU>
__global__ __launch_bounds__(kWinBlock) void k_window_gather_imputed(
    const unsigned* __restrict__ series, const unsigned* __restrict__ climatology, const unsigned* __restrict__ target,
    const long long* __restrict__ origins, const long long* __restrict__ offsets, unsigned* __restrict__ X,
    long long* __restrict__ H, long long* __restrict__ D, unsigned* __restrict__ Y, int R, int M, int Mx, int N,
    long long T_total, int q, long long history, int period, int x_tiles, long long x_items, int y_tiles,
    long long items) {
  for (long long w = blockIdx.x; w < items; w += gridDim.x) {
    if (w < x_items) {
      const long long br = w / x_tiles;                       // sample * R + component
      const int tile = (int)(w - br * x_tiles);
      const long long b = br / R;
      const int r = (int)(br - b * R);
      const long long t = clamp_ll(origins[b], history, T_total - q);
      const long long t0 = clamp_ll(t - offsets[r], 0, T_total - TAU);
      const unsigned s0 = (unsigned)(t0 % period);            // slot of the window's first step
      const int m = tile * kWinBlock + (int)threadIdx.x;
      if (m < Mx) {
        unsigned v[TAU];
        if (m < M) {
          const unsigned* src = series + t0 * M + m;
#pragma unroll
          for (int k = 0; k < TAU; ++k) v[k] = src[(long long)k * M];
#pragma unroll
          for (int k = 0; k < TAU; ++k)
            if (is_nan_word(v[k])) v[k] = climatology[(long long)((s0 + k) % (unsigned)period) * M + m];
        } else {
          const unsigned* src = series + t0 * M + (m - M);    // channel 0 of this node
#pragma unroll
          for (int k = 0; k < TAU; ++k) v[k] = 0x3f800000u;
          for (int c = 0; c < M; c += N) {
#pragma unroll
            for (int k = 0; k < TAU; ++k)
              if (is_nan_word(src[(long long)k * M + c])) v[k] = 0u;
          }
        }
        uint4* dst = reinterpret_cast<uint4*>(X + (br * Mx + m) * TAU);   // 16-byte aligned: TAU % 4 == 0
#pragma unroll
        for (int k = 0; k < TAU; k += 4) dst[k / 4] = make_uint4(v[k], v[k + 1], v[k + 2], v[k + 3]);
      }
    } else {
      const long long yy = w - x_items;
      const long long b = yy / y_tiles;
      const int tile = (int)(yy - b * y_tiles);
      const long long t = clamp_ll(origins[b], history, T_total - q);
      const int e = tile * kWinBlock + (int)threadIdx.x;      // n * q + j
      if (e < N * q) {
        const int n = e / q, j = e - n * q;
        Y[b * N * q + e] = target[(long long)n * T_total + t + j];
      }
      if (tile == 0 && threadIdx.x == 0) {
        const long long hour = t / TAU;
        H[b] = hour % 24;
        D[b] = (hour / 24) % 7;
      }
    }
  }
}

}  // namespace msgat

extern "C" int msgat_window_gather(const float* series, const float* target, const int64_t* origins,
                                   const int64_t* offsets, float* X, int64_t* H, int64_t* D, float* Y, int32_t B,
                                   int32_t R, int32_t C, int32_t N, int64_t T_total, int32_t tau, int32_t q,
                                   int64_t history, void* stream) {
  using namespace msgat;
  if (!series || !target || !origins || !offsets || !X || !H || !D || !Y) return MSGAT_ERR_NULL;
  if (B <= 0 || R <= 0 || C <= 0 || N <= 0 || history < 0 || T_total < history + q) return MSGAT_ERR_SHAPE;
  // C * N and N * q (with a tile's 256 lanes on top) are held in an int by the kernel
  if (q < 1 || q > 64 || (long long)C * N > 0x7fffff00LL || (long long)N * q > 0x7fffff00LL)
    return MSGAT_ERR_UNSUPPORTED;
  const int M = C * N;
  const int x_tiles = (M + kWinBlock - 1) / kWinBlock, y_tiles = (N * q + kWinBlock - 1) / kWinBlock;
  const long long x_items = (long long)B * R * x_tiles, items = x_items + (long long)B * y_tiles;
  const unsigned grid = (unsigned)(items < (1LL << 20) ? items : (1LL << 20));
  return dispatch_T(tau, [&](auto t) -> int {
    constexpr int TAU = decltype(t)::value;
    if (T_total < TAU) return MSGAT_ERR_SHAPE;
    hipLaunchKernelGGL(k_window_gather<TAU>, dim3(grid), dim3(kWinBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned*>(series), reinterpret_cast<const unsigned*>(target),
                       (const long long*)origins, (const long long*)offsets, reinterpret_cast<unsigned*>(X),
                       (long long*)H, (long long*)D, reinterpret_cast<unsigned*>(Y), R, M, N, (long long)T_total, q,
                       (long long)history, x_tiles, x_items, y_tiles, items);
    MSGAT_CHECK_LAUNCH();
    return MSGAT_OK;
  });
}

extern "C" int msgat_window_gather_imputed(const float* series, const float* climatology, const float* target,
                                           const int64_t* origins, const int64_t* offsets, float* X, int64_t* H,
                                           int64_t* D, float* Y, int32_t B, int32_t R, int32_t C, int32_t N,
                                           int64_t T_total, int32_t tau, int32_t q, int64_t history, int32_t period,
                                           int32_t mask_channel, void* stream) {
  using namespace msgat;
  if (!series || !climatology || !target || !origins || !offsets || !X || !H || !D || !Y) return MSGAT_ERR_NULL;
  if (B <= 0 || R <= 0 || C <= 0 || N <= 0 || history < 0 || T_total < history + q || period < 1)
    return MSGAT_ERR_SHAPE;
  // (C + 1) * N and N * q (with a tile's 256 lanes on top) are held in an int by the kernel
  if (q < 1 || q > 64 || ((long long)C + 1) * N > 0x7fffff00LL || (long long)N * q > 0x7fffff00LL)
    return MSGAT_ERR_UNSUPPORTED;
  const int M = C * N, Mx = mask_channel ? M + N : M;
  const int x_tiles = (Mx + kWinBlock - 1) / kWinBlock, y_tiles = (N * q + kWinBlock - 1) / kWinBlock;
  const long long x_items = (long long)B * R * x_tiles, items = x_items + (long long)B * y_tiles;
  const unsigned grid = (unsigned)(items < (1LL << 20) ? items : (1LL << 20));
  return dispatch_T(tau, [&](auto t) -> int {
    constexpr int TAU = decltype(t)::value;
    if (T_total < TAU) return MSGAT_ERR_SHAPE;
    hipLaunchKernelGGL(k_window_gather_imputed<TAU>, dim3(grid), dim3(kWinBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned*>(series), reinterpret_cast<const unsigned*>(climatology),
                       reinterpret_cast<const unsigned*>(target), (const long long*)origins, (const long long*)offsets,
                       reinterpret_cast<unsigned*>(X), (long long*)H, (long long*)D, reinterpret_cast<unsigned*>(Y), R,
                       M, Mx, N, (long long)T_total, q, (long long)history, (int)period, x_tiles, x_items, y_tiles,
                       items);
    MSGAT_CHECK_LAUNCH();
    return MSGAT_OK;
  });
}
