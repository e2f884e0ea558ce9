// Online forecasting, calibrated: rolling split-conformal prediction intervals from the absolute errors the scorer
// settles -- how far to trust this forecast for this sensor at this horizon right now, for any trained point model.
//
//   reference            none: its model gives a point per sensor and horizon (msgat.py) and its engine scores a loader over
//                        a series that exists in full.  QuantileLoss heads need retraining and promise no coverage.
//   here                 per series (n, h) the last W valid settled errors |p - y| in a ring, and per level the half-width
//                        r = one order statistic of that ring.  State, in device memory, never read back in a step:
//                          window      [N, T, W] fp32     the ring of a series
//                          cursor      [N, T] int32       c as uint32: slot = c mod W, fill = min(c, W); after an insert
//                                                         c + 1 below W, else W + (slot + 1) mod W -- any word stays inside
//                          radius      [L, N, T] fp32     the current half-widths, +inf = no interval yet
//                          radius_book [P, L, N, T] fp32  the radii issued with the forecast of origin o, in row o mod P:
//                                                         the rows and stamps of the scoring book (online_score.hip)
//                          counts      [L, N, T, 2] int64 {judged, covered}
//                          ranks       [L, W + 1] int32   rank[l, m]: the 1-based order statistic at fill m, 0 = none
//     k_interval_update  BEFORE the push that advances the clock, where k_forecast_score runs.  A WAVE OWNS A SERIES: lane
//                        i holds slots i, i + 64, ... in registers (V per lane, V = 1, 2, 4, 8, 16 for W <= 64 .. 1024).
//                        For k = 0 .. K-1 origin o = s + k - h is due: stamp, y = raw[k, 0, n], p and the issued radii are
//                        wave-uniform.  With the stamp and a valid y, a = |p_point - y| (fp32, point_terms' abs_err):
//                          judge   lane l < L: if radius_book[row(o), l, n, h] is finite, judged += 1, covered += a <= r
//                          insert  if a is finite it takes the slot the cursor names, in registers; the cursor advances
//                        in that order: an error never meets an interval it helped to make.  Then the changed slots and
//                        the cursor go back, and per level radius = +inf for rank 0, else the rank-th smallest of the
//                        filled slots by a 31-step radix select from bit 30 down: the inserted values are finite and
//                        non-negative, so their bit patterns order as unsigned integers, and counting the candidates with
//                        a zero bit is a __ballot and a popcount per register.  No LDS, no sort, no atomic; the result is
//                        the bit pattern of a window element, ties included (equal values have equal bits).
//     k_interval_apply   after the forecast exists: over L N T elements, p = pred[n, point T + h], lo = p - r, hi = p + r
//                        (one fp32 operation each) and r goes into row clock[0] mod P of radius_book.  Idempotent.
// Every cell of every buffer has one owner, the wave (update) or the lane (apply) of its series.
#include "common.hpp"
#include "score_clock.hpp"
#include "tail_terms.hpp"

namespace msgat {

constexpr int kIntervalWaves = 4;          // series per block of k_interval_update
constexpr int kIntervalBlock = 64 * kIntervalWaves;
constexpr int kIntervalMaxL = 4;
constexpr int kIntervalMaxW = 1024;
constexpr int kIntervalMaxT = 64;
constexpr int kIntervalApplyBlock = 256;

__device__ __forceinline__ bool interval_finite(float v) { return fabsf(v) < __builtin_inff(); }   // false for a NaN

template <int V, bool kNull>
__global__ __launch_bounds__(kIntervalBlock) void k_interval_update(
    const float* __restrict__ raw, const float* __restrict__ book, const long long* __restrict__ issued,
    const long long* __restrict__ clock, const float* __restrict__ radius_book, const int* __restrict__ ranks,
    float* __restrict__ window, unsigned* __restrict__ cursor, float* __restrict__ radius,
    long long* __restrict__ counts, int K, long long step_stride, int N, int T, int out, int point, long long P, int L,
    int W, float null_value) {
#pragma clang fp contract(off)
  const int lane = (int)threadIdx.x & 63;
  const long long series = (long long)blockIdx.x * kIntervalWaves + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const long long NT = (long long)N * T;
  if (series >= NT) return;                                            // the whole wave: no barrier below
  const int n = (int)(series / T), h = (int)(series % T);
  float* __restrict__ win = window + series * W;
  unsigned w[V];                                                        // the ring as bit patterns
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int slot = j * 64 + lane;
    w[j] = slot < W ? __float_as_uint(win[slot]) : 0u;
  }
  unsigned c = cursor[series];
  unsigned dirty = 0;                                                   // bit j: this lane's register j changed
  long long judged = 0, covered = 0;                                    // lane l < L: level l
  const long long s = clock[0];
  for (int k = 0; k < K; ++k) {
    const long long o = score_wrap_sub(score_wrap_add(s, k), h);
    const long long row = score_floor_mod(o, P);
    const bool stamped = issued[row] == o && o >= 0;
    const float y = raw[(long long)k * step_stride + n];                // channel 0 of step s + k
    if (!(stamped && entry_valid(y, kNull ? null_value : __builtin_nanf("")))) continue;   // wave-uniform
    const float a = point_terms(book[(row * N + n) * out + (long long)point * T + h], y, 0.f).abs_err;
    if (lane < L) {                                                     // judge first
      const float r = radius_book[((row * L + lane) * N + n) * T + h];
      if (interval_finite(r)) {
        judged += 1;
        covered += a <= r ? 1 : 0;
      }
    }
    if (!interval_finite(a)) continue;                                  // a NaN forecast is judged, not inserted
    const unsigned slot = c % (unsigned)W;
#pragma unroll
    for (int j = 0; j < V; ++j)
      if ((int)slot == j * 64 + lane) {
        w[j] = __float_as_uint(a);
        dirty |= 1u << j;
      }
    c = c < (unsigned)W ? c + 1u : (unsigned)W + (slot + 1u == (unsigned)W ? 0u : slot + 1u);
  }
#pragma unroll
  for (int j = 0; j < V; ++j)
    if ((dirty >> j) & 1u) win[j * 64 + lane] = __uint_as_float(w[j]);
  if (lane == 0) cursor[series] = c;
  if (lane < L) {
    long long* __restrict__ cell = counts + (((long long)lane * N + n) * T + h) * 2;
    cell[0] += judged;
    cell[1] += covered;
  }
  const int fill = (int)(c < (unsigned)W ? c : (unsigned)W);
#pragma unroll
  for (int j = 0; j < V; ++j)                                           // slots at or beyond the fill take no part: bit 31
    if (j * 64 + lane >= fill) w[j] = 0xffffffffu;                      // set, which no prefix below has
  for (int l = 0; l < L; ++l) {
    const int rank = ranks[(long long)l * (W + 1) + fill];
    unsigned found = __float_as_uint(__builtin_inff());
    if (rank >= 1 && rank <= fill) {                                    // wave-uniform
      int remaining = rank;
      unsigned prefix = 0;                                              // the bits of the wanted element above `bit`
      for (int bit = 30; bit >= 0; --bit) {
        // a candidate (equal to the prefix above `bit`) with a zero at `bit`: (w ^ prefix) has nothing at or above it
        int zeros = 0;
#pragma unroll
        for (int j = 0; j < V; ++j)
          if (j * 64 < fill)                                            // wave-uniform: registers beyond the fill hold nothing
            zeros += __popcll(__ballot((w[j] ^ prefix) < (1u << bit)));
        if (remaining > zeros) {                                        // the wanted element has this bit set
          remaining -= zeros;
          prefix |= 1u << bit;
        }
      }
      found = prefix;
    }
    if (lane == 0) radius[((long long)l * N + n) * T + h] = __uint_as_float(found);
  }
}

__global__ __launch_bounds__(kIntervalApplyBlock) void k_interval_apply(
    const float* __restrict__ pred, const float* __restrict__ radius, const long long* __restrict__ clock,
    float* __restrict__ lo, float* __restrict__ hi, float* __restrict__ radius_book, long long NT, long long total, int T,
    int out, int point, long long P) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * kIntervalApplyBlock + threadIdx.x;
  if (i >= total) return;
  const long long at = i % NT;                                          // n T + h
  const float r = radius[i];
  const float p = pred[(at / T) * out + (long long)point * T + at % T];
  const long long row = score_floor_mod(clock[0], P);
  lo[i] = p - r;
  hi[i] = p + r;
  radius_book[row * total + i] = r;
}

// what both entry points check of the head and the book: nothing is launched on a refusal
static int check_interval_head(int32_t N, int32_t T_out, int32_t out, int32_t point, int64_t P, int32_t L) {
  if (N <= 0 || T_out <= 0 || out <= 0 || L <= 0 || P < (int64_t)T_out) return MSGAT_ERR_SHAPE;
  if (L > kIntervalMaxL || T_out > kIntervalMaxT || out > kIntervalMaxT || (long long)N > 0x7fffff00LL)
    return MSGAT_ERR_UNSUPPORTED;
  if (out % T_out || point < 0 || point >= out / T_out) return MSGAT_ERR_SHAPE;
  return MSGAT_OK;
}

template <int V>
static void launch_interval_update(bool has_null, dim3 grid, hipStream_t s, const float* raw, const float* book,
                                   const long long* issued, const long long* clock, const float* radius_book,
                                   const int* ranks, float* window, unsigned* cursor, float* radius, long long* counts,
                                   int K, long long step_stride, int N, int T, int out, int point, long long P, int L,
                                   int W, float null_value) {
  if (has_null)
    hipLaunchKernelGGL((k_interval_update<V, true>), grid, dim3(kIntervalBlock), 0, s, raw, book, issued, clock,
                       radius_book, ranks, window, cursor, radius, counts, K, step_stride, N, T, out, point, P, L, W,
                       null_value);
  else
    hipLaunchKernelGGL((k_interval_update<V, false>), grid, dim3(kIntervalBlock), 0, s, raw, book, issued, clock,
                       radius_book, ranks, window, cursor, radius, counts, K, step_stride, N, T, out, point, P, L, W,
                       null_value);
}

}  // namespace msgat

extern "C" int msgat_interval_update(const float* raw, const float* book, const int64_t* issued, const int64_t* clock,
                                     const float* radius_book, const int32_t* ranks, float* window, int32_t* cursor,
                                     float* radius, int64_t* counts, int32_t K, int32_t C, int32_t N, int32_t T_out,
                                     int32_t out, int32_t point, int64_t P, int32_t L, int32_t W, int32_t has_null,
                                     float null_value, void* stream) {
  using namespace msgat;
  if (!raw || !book || !issued || !clock || !radius_book || !ranks || !window || !cursor || !radius || !counts)
    return MSGAT_ERR_NULL;
  if (K <= 0 || C <= 0 || W <= 0) return MSGAT_ERR_SHAPE;
  if (int st = check_interval_head(N, T_out, out, point, P, L)) return st;
  if (W > kIntervalMaxW) return MSGAT_ERR_UNSUPPORTED;
  const long long blocks = ((long long)N * T_out + kIntervalWaves - 1) / kIntervalWaves;
  if (blocks > 0x7fffffffLL) return MSGAT_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)blocks);
  const long long step_stride = (long long)C * N;
  hipStream_t s = (hipStream_t)stream;
#define MSGAT_INTERVAL_CASE(v)                                                                                         \
  launch_interval_update<v>(has_null != 0, grid, s, raw, book, (const long long*)issued, (const long long*)clock,     \
                            radius_book, (const int*)ranks, window, (unsigned*)cursor, radius, (long long*)counts, K,  \
                            step_stride, N, T_out, out, point, (long long)P, L, W, null_value)
  if (W <= 64) MSGAT_INTERVAL_CASE(1);
  else if (W <= 128) MSGAT_INTERVAL_CASE(2);
  else if (W <= 256) MSGAT_INTERVAL_CASE(4);
  else if (W <= 512) MSGAT_INTERVAL_CASE(8);
  else MSGAT_INTERVAL_CASE(16);
#undef MSGAT_INTERVAL_CASE
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

extern "C" int msgat_interval_apply(const float* pred, const float* radius, const int64_t* clock, float* lo, float* hi,
                                    float* radius_book, int32_t N, int32_t T_out, int32_t out, int32_t point, int64_t P,
                                    int32_t L, void* stream) {
  using namespace msgat;
  if (!pred || !radius || !clock || !lo || !hi || !radius_book) return MSGAT_ERR_NULL;
  if (int st = check_interval_head(N, T_out, out, point, P, L)) return st;
  const long long NT = (long long)N * T_out, total = NT * L;
  const long long blocks = (total + kIntervalApplyBlock - 1) / kIntervalApplyBlock;
  if (blocks > 0x7fffffffLL) return MSGAT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_interval_apply, dim3((unsigned)blocks), dim3(kIntervalApplyBlock), 0, (hipStream_t)stream, pred,
                     radius, (const long long*)clock, lo, hi, radius_book, NT, total, T_out, out, point, (long long)P);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}
