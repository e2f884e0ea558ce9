// Online forecasting, scored: the book of the forecasts that were issued and the kernel that settles it as their
// readings arrive -- error per horizon, signed bias and per-sensor error of a running service, with nothing read back.
//
//   reference            engine.py:66-70 + metrics.py:20-35 score a loader over a series that exists in full; a forecast
//                        made beside the sensors has no path there (nor has online.hip's ring, whose readings are
//                        normalised and then forgotten as truths).
//   here                 book [P, N, out] fp32 (P >= T_out): the forecast of origin o lives in row o floor-mod P;
//                        issued [P] int64: the origin each row was written for (a fresh book: INT64_MIN = never).  A row
//                        counts for origin o only if issued[row] == o and o >= 0.
//     k_forecast_store   pred [N, out] moves as 32-bit words into row clock[0] floor-mod P, lane 0 of block 0 stamps
//                        issued[row] = clock[0]: one launch, idempotent for one origin.
//     k_forecast_score   BEFORE the push that advances the clock: raw[k] is step s + k, s = clock[0].  A LANE OWNS A NODE
//                        n (blocks of 64 nodes).  For k = 0 .. K-1, then h = 0 .. T_out-1: origin o = s + k - h is due at
//                        horizon h; if its stamp matches and y = raw[k, 0, n] is valid (not NaN, != null_value when there
//                        is one) the entry's terms are formed in fp32 from p = book[row(o), n, q T_out + h]
//                        (tail_terms.hpp: the functions k_quantile_metrics calls) and widened to double:
//                          0 count 1, 1 |e|, 2 100 |e / y| if y > mask_value else 0, 3 e^2, 4 e        e = p_point - y
//                          Q levels: 5 any p_q > p_{q+1}, 6 p_{Q-1} - p_0, 7 + q  y <= p_q, 7 + Q + q  rho_q
//                        The lane adds them (a) into its three node totals {count, |e|, e} in registers, in this k-then-h
//                        order, and (b) into its own slot part[(c T_out + h) N + n] of column c and horizon h: the slot
//                        starts as +0.0 at k = 0 and receives the settled entries of that horizon in k order (K = 1,
//                        the captured step: stores only).  At the end node_sums[n, :] += the node totals: one owner, no
//                        reduction.
//     k_forecast_score_finish   block c adds column c, a wave per horizon: the slots of nodes 64 b .. 64 b + 63 are
//                        added in node order starting from +0.0 (= lane order inside block b of the first launch), those
//                        block sums in block order starting from +0.0; sums[h, c] += that, and sums[T_out, c] += the
//                        horizon values added in horizon order starting from +0.0.
// Every sum has one fixed order and there are no floating-point atomics: a numpy restatement gives every bit.
// Rows come from a 64-bit floor-mod into [0, P) for ANY clock content (cold, negative, a wild word): no launch reads or
// writes outside book and issued, and what does not carry the stamp settles nothing.
#include "common.hpp"
#include "score_clock.hpp"
#include "tail_terms.hpp"

namespace msgat {

constexpr int kScoreBlock = 64;          // one wave: the first launch's block, and the unit the finish adds in lane order
constexpr int kScoreFinishBlock = 1024;
constexpr int kScoreMaxT = 64;
constexpr int kScoreNodeCols = 3;

__global__ __launch_bounds__(kScoreBlock) void k_forecast_store(const unsigned* __restrict__ pred,
                                                                unsigned* __restrict__ book,
                                                                long long* __restrict__ issued,
                                                                const long long* __restrict__ clock, long long words,
                                                                long long P) {
  const long long i = (long long)blockIdx.x * kScoreBlock + threadIdx.x;
  const unsigned word = i < words ? pred[i] : 0u;                    // in flight beside the clock
  const long long t = clock[0];
  const long long row = score_floor_mod(t, P);
  if (i < words) book[row * words + i] = word;
  if (blockIdx.x == 0 && threadIdx.x == 0) issued[row] = t;
}

// Q == 0: a point head (out = T, 5 columns); Q >= 1: a Q-level head (out = Q T, level-major, 7 + 2Q columns)
template <int Q, bool kNull>
__global__ __launch_bounds__(kScoreBlock) void k_forecast_score(
    const float* __restrict__ raw, const float* __restrict__ book, const long long* __restrict__ issued,
    const long long* __restrict__ clock, int K, long long step_stride, int N, int T, long long P, QuantLevels lv,
    int point, float null_value, float mask_value, double* __restrict__ part, double* __restrict__ node_sums) {
#pragma clang fp contract(off)
  constexpr int kCols = Q == 0 ? kPointCols : quant_cols(Q);
  constexpr int kLevels = Q == 0 ? 1 : Q;
  constexpr int kChunk = kLevels == 1 ? 16 : kLevels <= 4 ? 8 : 4;    // horizons whose loads are in flight together
  const int n = (int)blockIdx.x * kScoreBlock + (int)threadIdx.x;
  const int lane = (int)threadIdx.x & 63;
  const bool owner = n < N;                                           // no early return: every lane votes in the ballot
  const long long s = clock[0];
  const long long out = (long long)kLevels * T;
  double node[kScoreNodeCols] = {0.0, 0.0, 0.0};
  for (int k = 0; k < K; ++k) {
    const long long sk = score_wrap_add(s, k);
    const long long rk = score_floor_mod(sk, P);
    // the stamps of this step's T <= 64 origins in ONE round trip: lane h of every wave tests origin s + k - h, the
    // ballot hands all T answers to every lane (h < T <= P: one wrap at most)
    bool mine = false;
    if (lane < T) {
      const long long o = score_wrap_sub(sk, lane);
      mine = issued[rk >= lane ? rk - lane : rk - lane + P] == o && o >= 0;
    }
    const unsigned long long due = __ballot(mine);
    const float y = owner ? raw[(long long)k * step_stride + n] : 0.f;   // channel 0 of step s + k
    const bool valid = owner && entry_valid(y, kNull ? null_value : __builtin_nanf(""));   // no null value: NaN only
    for (int h0 = 0; h0 < T; h0 += kChunk) {
      float p[kChunk][kLevels];
      bool hit[kChunk];
#pragma unroll
      for (int u = 0; u < kChunk; ++u) {                                // every load of the chunk, then its arithmetic
        const int h = h0 + u;
        hit[u] = h < T && ((due >> h) & 1ull) != 0 && valid;
#pragma unroll
        for (int q = 0; q < kLevels; ++q) p[u][q] = 0.f;
        if (hit[u]) {
          const long long row = rk >= h ? rk - h : rk - h + P;
          const float* __restrict__ pr = book + (row * N + n) * out + h;
#pragma unroll
          for (int q = 0; q < kLevels; ++q) p[u][q] = pr[q * T];
        }
      }
#pragma unroll
      for (int u = 0; u < kChunk; ++u) {
        const int h = h0 + u;
        if (h >= T || !owner) continue;
        double t[kCols];
#pragma unroll
        for (int c = 0; c < kCols; ++c) t[c] = 0.0;
        if (hit[u]) {
          const PointTerms pt = point_terms(point_forecast(p[u], point), y, mask_value);
          t[kColCount] = 1.0;
          t[kColAbs] = (double)pt.abs_err;
          if (pt.ape_counts) t[kColApe] = pt.ape;
          t[kColSq] = pt.sq_err;
          t[kScoreBiasCol] = (double)pt.err;
          if constexpr (Q > 0) {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
              const LevelTerm lt = level_term(p[u][q], y, lv.tau[q], lv.tau_m1[q]);
              t[quant_rho_col(Q, q)] = (double)lt.rho;
              if (lt.hit) t[quant_hit_col(q)] = 1.0;
            }
            if (levels_cross(p[u])) t[kQuantCrossCol] = 1.0;
            t[kQuantWidthCol] = (double)levels_width(p[u]);
          }
          node[0] += t[kColCount];
          node[1] += t[kColAbs];
          node[2] += t[kScoreBiasCol];
        }
        if (k == 0 || hit[u]) {
#pragma unroll
          for (int c = 0; c < kCols; ++c) {
            double* slot = part + ((long long)c * T + h) * N + n;
            const double before = k == 0 ? 0.0 : *slot;
            *slot = before + t[c];
          }
        }
      }
    }
  }
  if (!owner) return;
#pragma unroll
  for (int j = 0; j < kScoreNodeCols; ++j) node_sums[(long long)n * kScoreNodeCols + j] += node[j];
}

__global__ __launch_bounds__(kScoreFinishBlock) void k_forecast_score_finish(const double* __restrict__ part, int N,
                                                                             int T, int cols,
                                                                             double* __restrict__ sums) {
  constexpr int kWaves = kScoreFinishBlock / 64;
  __shared__ double rows[kScoreMaxT];
  const int c = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long tiles = ((long long)N + kScoreBlock - 1) / kScoreBlock;
  for (int h = wave; h < T; h += kWaves) {       // a wave per horizon; no barrier inside
    const double* __restrict__ p = part + ((long long)c * T + h) * N;
    double total = 0.0;
    for (long long b0 = 0; b0 < tiles; b0 += 64) {
      // lane l adds block b0 + l of the first launch in lane order: 64 chains side by side instead of one behind another
      const long long base = (b0 + lane) * kScoreBlock;
      const int count = base >= N ? 0 : (int)(N - base < kScoreBlock ? N - base : kScoreBlock);
      double t = 0.0;
      int j = 0;
      for (; j + 16 <= count; j += 16) {         // 16 loads in flight, then their adds in order
        double w[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) w[u] = p[base + j + u];
#pragma unroll
        for (int u = 0; u < 16; ++u) t += w[u];
      }
      for (; j < count; ++j) t += p[base + j];
      const int here = tiles - b0 < 64 ? (int)(tiles - b0) : 64;   // wave-uniform
      for (int l = 0; l < here; ++l) total += __shfl(t, l);        // the block sums in block order
    }
    if (lane == 0) rows[h] = total;
  }
  __syncthreads();
  if ((int)threadIdx.x < T) sums[(long long)threadIdx.x * cols + c] += rows[threadIdx.x];
  if (threadIdx.x != 0) return;
  double all = 0.0;
  for (int h = 0; h < T; ++h) all += rows[h];
  sums[(long long)T * cols + c] += all;
}

template <int Q>
static void launch_forecast_score_q(bool has_null, dim3 grid, hipStream_t s, const float* raw, const float* book,
                                    const long long* issued, const long long* clock, int K, long long step_stride, int N,
                                    int T, long long P, const QuantLevels& lv, int point, float null_value,
                                    float mask_value, double* part, double* node_sums) {
  if (has_null)
    hipLaunchKernelGGL((k_forecast_score<Q, true>), grid, dim3(kScoreBlock), 0, s, raw, book, issued, clock, K,
                       step_stride, N, T, P, lv, point, null_value, mask_value, part, node_sums);
  else
    hipLaunchKernelGGL((k_forecast_score<Q, false>), grid, dim3(kScoreBlock), 0, s, raw, book, issued, clock, K,
                       step_stride, N, T, P, lv, point, null_value, mask_value, part, node_sums);
}

// limits first (they bound the loop over `levels`), then the levels: nothing is launched on a refusal
static int check_forecast_score(int32_t K, int32_t C, int32_t N, int32_t T_out, int32_t Q, const float* levels,
                                int32_t point, int64_t P) {
  if (K <= 0 || C <= 0 || N <= 0 || T_out <= 0 || Q < 0 || P < (int64_t)T_out) return MSGAT_ERR_SHAPE;
  if (Q > kQuantMaxQ || (int64_t)(Q > 0 ? Q : 1) * T_out > kScoreMaxT || (long long)N > 0x7fffff00LL)
    return MSGAT_ERR_UNSUPPORTED;                                         // N plus a tile is held in an int
  for (int q = 0; q < Q; ++q)   // strictly increasing inside (0, 1); a NaN fails its comparison
    if (!(levels[q] > (q == 0 ? 0.f : levels[q - 1]) && levels[q] < 1.f)) return MSGAT_ERR_SHAPE;
  if (Q > 0 && (point < 0 || point >= Q)) return MSGAT_ERR_SHAPE;
  return MSGAT_OK;
}

}  // namespace msgat

extern "C" int msgat_forecast_store(const float* pred, float* book, int64_t* issued, const int64_t* clock, int32_t N,
                                    int32_t out, int64_t P, void* stream) {
  using namespace msgat;
  if (!pred || !book || !issued || !clock) return MSGAT_ERR_NULL;
  if (N <= 0 || out <= 0 || P <= 0) return MSGAT_ERR_SHAPE;
  if ((long long)N > 0x7fffff00LL) return MSGAT_ERR_UNSUPPORTED;
  const long long words = (long long)N * out;
  const long long blocks = (words + kScoreBlock - 1) / kScoreBlock;
  if (blocks > 0x7fffffffLL) return MSGAT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_forecast_store, dim3((unsigned)blocks), dim3(kScoreBlock), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned*>(pred), reinterpret_cast<unsigned*>(book), (long long*)issued,
                     (const long long*)clock, words, (long long)P);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

extern "C" size_t msgat_forecast_score_partial_doubles(int32_t N, int32_t T_out, int32_t Q) {
  using namespace msgat;
  if (N <= 0 || T_out <= 0 || Q < 0 || Q > kQuantMaxQ || (int64_t)(Q > 0 ? Q : 1) * T_out > kScoreMaxT ||
      (long long)N > 0x7fffff00LL)
    return 0;
  return (size_t)(Q == 0 ? kPointCols : quant_cols(Q)) * (size_t)T_out * (size_t)N;
}

extern "C" int msgat_forecast_score(const float* raw, const float* book, const int64_t* issued, const int64_t* clock,
                                    int32_t K, int32_t C, int32_t N, int32_t T_out, int32_t Q, const float* levels,
                                    int32_t point, int64_t P, int32_t has_null, float null_value, float mask_value,
                                    double* partials, double* sums, double* node_sums, void* stream) {
  using namespace msgat;
  if (!raw || !book || !issued || !clock || !partials || !sums || !node_sums || (Q > 0 && !levels)) return MSGAT_ERR_NULL;
  if (int st = check_forecast_score(K, C, N, T_out, Q, levels, point, P)) return st;
  const QuantLevels lv = quant_levels(levels, Q);
  const dim3 grid((unsigned)((N + kScoreBlock - 1) / kScoreBlock));
  const long long step_stride = (long long)C * N;
  hipStream_t s = (hipStream_t)stream;
#define MSGAT_SCORE_CASE(q)                                                                                          \
  case q:                                                                                                            \
    launch_forecast_score_q<q>(has_null != 0, grid, s, raw, book, (const long long*)issued, (const long long*)clock, \
                               K, step_stride, N, T_out, (long long)P, lv, point, null_value, mask_value, partials,  \
                               node_sums);                                                                           \
    break;
  switch (Q) {
    MSGAT_SCORE_CASE(0)
    MSGAT_SCORE_CASE(1)
    MSGAT_SCORE_CASE(2)
    MSGAT_SCORE_CASE(3)
    MSGAT_SCORE_CASE(4)
    MSGAT_SCORE_CASE(5)
    MSGAT_SCORE_CASE(6)
    MSGAT_SCORE_CASE(7)
    MSGAT_SCORE_CASE(8)
    default: return MSGAT_ERR_UNSUPPORTED;
  }
#undef MSGAT_SCORE_CASE
  MSGAT_CHECK_LAUNCH();
  const int cols = Q == 0 ? kPointCols : quant_cols(Q);
  hipLaunchKernelGGL(k_forecast_score_finish, dim3(cols), dim3(kScoreFinishBlock), 0, s, partials, N, T_out, cols, sums);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}
