// What one entry of a forecast contributes to the metric totals: the terms that the masked step tail (tail.hip:
// k_masked_loss_metrics, k_quantile_metrics) and the online scorer (online_score.hip: k_forecast_score) add up, each in
// its own way -- registers per horizon in the tail, one slot per (column, horizon, node) in the scorer.  How an entry is
// scored is written here once; how the terms are accumulated stays with each kernel.
//
// Columns of a record and of the totals (the point columns are the masked tail's; a Q-level head appends the rest):
//   0 count   1 |e|   2 100 |e / y| where y > mask_value   3 e^2        e = p_point - y
//   4 the loss sum (tail) or the signed error e (scorer)
//   5 entries with any p_q > p_{q+1}   6 p_{Q-1} - p_0   7 + q entries with y <= p_q   7 + Q + q sum of rho_q
//
// k_forecast_score is compiled with contraction off, the tail kernels with the default.  Every value formed here is
// therefore one that is rounded once either way -- a difference, a single product, a quotient, a widening to double
// (100.0 * (double)x and (double)e * (double)e are exact) -- and the sums into which a caller folds them are the
// caller's: an expression such as `total * (1.0 / Q)` followed by an add stays written where it is added.
#pragma once
#include <hip/hip_runtime.h>

namespace msgat {

constexpr int kQuantMaxQ = 8;
constexpr int kQuantBase = 7;   // the columns in front of the per-level ones
constexpr int kColCount = 0, kColAbs = 1, kColApe = 2, kColSq = 3;
constexpr int kMaskLossCol = 4, kQuantLossCol = 4, kScoreBiasCol = 4;
constexpr int kQuantCrossCol = 5, kQuantWidthCol = 6;
constexpr int kPointCols = 5;   // a record without levels: columns 0-4
__host__ __device__ constexpr int quant_cols(int Q) { return kQuantBase + 2 * Q; }
__host__ __device__ constexpr int quant_hit_col(int q) { return kQuantBase + q; }
__host__ __device__ constexpr int quant_rho_col(int Q, int q) { return kQuantBase + Q + q; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// An entry of the truth counts when it is a measurement: not NaN and not the null value (a PEMS reading of 0 = sensor
// down).  With null_value = NaN only the NaN entries drop out (y != NaN holds for every y).
__device__ __forceinline__ bool entry_valid(float y, float null_value) { return y == y && y != null_value; }

// tau_q and tau_q - 1 (formed in double on the host, rounded to fp32 once); they travel by value
struct QuantLevels { float tau[kQuantMaxQ], tau_m1[kQuantMaxQ]; };

inline QuantLevels quant_levels(const float* levels, int Q) {
  QuantLevels lv = {};
  for (int q = 0; q < Q; ++q) {
    lv.tau[q] = levels[q];
    lv.tau_m1[q] = (float)((double)levels[q] - 1.0);
  }
  return lv;
}

// the level that serves as the point forecast (p[0] for a point outside the levels): one select per level at a constant
// index, in ascending order.  A compile-time recursion, not a loop: as a loop in here p[] went to scratch in both callers,
// and in descending order k_quantile_metrics<8> grew from 430 to 466 instructions.
template <int Q, int q = 1>
__device__ __forceinline__ float point_forecast(const float (&p)[Q], int point, float lower = 0.f) {
  const float pp = q == 1 ? p[0] : lower;                 // the forecast among the levels below q
  if constexpr (q < Q) return point_forecast<Q, q + 1>(p, point, q == point ? p[q] : pp);
  else return pp;
}

struct PointTerms {
  float err, abs_err;    // e = p_point - y and |e|, fp32 as the loss policies take them
  double sq_err;         // e^2
  bool ape_counts;       // y > mask_value: only then does the entry have a percentage error
  double ape;            // 100 |e / y|
};

__device__ __forceinline__ PointTerms point_terms(float p_point, float y, float mask_value) {
  const float e = p_point - y;
  return {e, fabsf(e), (double)e * (double)e, y > mask_value, 100.0 * (double)fabsf(e / y)};
}

// one level of a Q-level forecast; the caller walks its levels
struct LevelTerm {
  float rho;    // max(tau_q u, (tau_q - 1) u), u = y - p_q
  bool hit;     // y <= p_q
};

__device__ __forceinline__ LevelTerm level_term(float p_q, float y, float tau, float tau_m1) {
  const float u = y - p_q;
  return {fmaxf(tau * u, tau_m1 * u), y <= p_q};
}

template <int Q>
__device__ __forceinline__ bool levels_cross(const float (&p)[Q]) {   // any p_q > p_{q+1}
  bool crossing = false;
#pragma unroll
  for (int q = 0; q + 1 < Q; ++q) crossing = crossing || p[q] > p[q + 1];
  return crossing;
}

template <int Q>
__device__ __forceinline__ float levels_width(const float (&p)[Q]) { return p[Q - 1] - p[0]; }

}  // namespace msgat
