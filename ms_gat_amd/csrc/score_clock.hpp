// The clock arithmetic that the online scorer (online_score.hip) and the interval calibrator (online_interval.hip) share:
// the row of an origin in a book of P rows, and sums and differences of clock words.  Rows come from a 64-bit floor-mod
// into [0, P) for ANY clock content (cold, negative, a wild word), so no launch reads or writes outside a book.
#pragma once
#include <hip/hip_runtime.h>

namespace msgat {

__device__ __forceinline__ long long score_floor_mod(long long a, long long n) {   // n > 0
  const long long r = a % n;
  return r < 0 ? r + n : r;
}

// two's-complement sum and difference: a wild clock word wraps instead of overflowing a signed type
__device__ __forceinline__ long long score_wrap_add(long long a, long long b) {
  return (long long)((unsigned long long)a + (unsigned long long)b);
}

__device__ __forceinline__ long long score_wrap_sub(long long a, long long b) {
  return (long long)((unsigned long long)a - (unsigned long long)b);
}

}  // namespace msgat
