// What the lane-per-row streaming kernels of branches.hip and layernorm.hip share, each piece written once: the row helpers,
// the LayerNorm backward of one row, the block partial of a few T-vectors, the MFMA outer-product tile epilogue, the
// quarter-row LayerNorm of the head forward and the chunk staging of the head backward.  Contracts: DESIGN.md, "The row
// kernels of the branches".  Every sum below has a fixed order that output bits hang on; none of it may be re-associated.
#pragma once
#include "common.hpp"

namespace msgat {

// ---- a lane's own row of T floats -------------------------------------------------------------------------
template <int T>
__device__ __forceinline__ void load_row(const float* __restrict__ p, float (&v)[T]) {
#pragma unroll
  for (int t4 = 0; t4 < T / 4; ++t4) {
    const float4 a = reinterpret_cast<const float4*>(p)[t4];
    v[4 * t4 + 0] = a.x; v[4 * t4 + 1] = a.y; v[4 * t4 + 2] = a.z; v[4 * t4 + 3] = a.w;
  }
}
template <int T>
__device__ __forceinline__ void store_row(float* __restrict__ p, const float (&v)[T]) {
#pragma unroll
  for (int t4 = 0; t4 < T / 4; ++t4)
    reinterpret_cast<float4*>(p)[t4] = make_float4(v[4 * t4], v[4 * t4 + 1], v[4 * t4 + 2], v[4 * t4 + 3]);
}
// Centres a row in place and returns rstd.  The mean is taken of the differences to the row's first
// value (exact for nearby floats), so a large common offset costs no accuracy -- the two-pass
// formula on shifted data.
template <int T>
__device__ __forceinline__ float centre_row(float (&x)[T], float eps) {
  const float x0 = x[0];
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < T; ++t) { x[t] -= x0; s += x[t]; }
  const float md = s * (1.0f / T);
  float v = 0.f;
#pragma unroll
  for (int t = 0; t < T; ++t) { x[t] -= md; v = fmaf(x[t], x[t], v); }
  return rsqrtf(v * (1.0f / T) + eps);
}

// ---- the LayerNorm backward of one row ---------------------------------------------------------------------
// In: the row xv, its incoming gradient gv = dy, the weights w.  Out: gv = dx = rstd (g - mean(g) - xhat mean(g xhat)) with
// g = dy w, xv = xhat, and the row's terms added to dwb[0] (dweight: fma(dy, xhat)) and dwb[1] (dbias: + dy).  Returns the
// bits x[t] > 0 taken BEFORE centring: x is a ReLU output when the caller masks, and relu_mask_row applies them -- apart,
// because k_ln_bwd adds the gradient of x's other path between the two.
template <int T>
__device__ __forceinline__ unsigned ln_bwd_row(float (&xv)[T], float (&gv)[T], const float (&w)[T], float eps,
                                               float (&dwb)[2][T]) {
  unsigned positive = 0;
#pragma unroll
  for (int t = 0; t < T; ++t) positive |= (xv[t] > 0.f ? 1u : 0u) << t;
  const float rstd = centre_row<T>(xv, eps);
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    xv[t] *= rstd;                  // xhat
    dwb[1][t] += gv[t];
    dwb[0][t] = fmaf(gv[t], xv[t], dwb[0][t]);
    gv[t] *= w[t];                  // g = dy * w
    s1 += gv[t];
    s2 = fmaf(gv[t], xv[t], s2);
  }
  s1 *= (1.0f / T);
  s2 *= (1.0f / T);
#pragma unroll
  for (int t = 0; t < T; ++t) gv[t] = rstd * (gv[t] - s1 - xv[t] * s2);
  return positive;
}
// the backward of the ReLU that produced x (MEAM's tail, msgat.py:131), applied where x is at hand
template <int T>
__device__ __forceinline__ void relu_mask_row(float (&gv)[T], unsigned positive) {
#pragma unroll
  for (int t = 0; t < T; ++t) gv[t] = ((positive >> t) & 1u) ? gv[t] : 0.f;
}

// ---- the block partial of NV T-vectors ---------------------------------------------------------------------
// out[k * T + t] = the sum of v[k][t] over the block's 256 lanes: a shuffle tree over the wave (xor 32 ... 1; the NV vectors
// of a column side by side), lane 0 to red[wave][.], ONE barrier, then the four waves as (0 + 1) + (2 + 3).
template <int NV, int T>
__device__ __forceinline__ void block_partial(const float (&v)[NV][T], float (&red)[kBlock / kWave][NV * T], float* out) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    float a[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) a[k] = v[k][t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int k = 0; k < NV; ++k) a[k] += __shfl_xor(a[k], o);
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < NV; ++k) red[wave][k * T + t] = a[k];
    }
  }
  __syncthreads();
  if (threadIdx.x < NV * T)
    out[threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// ---- the MFMA outer-product tile epilogue ------------------------------------------------------------------
// acc[ot] is a wave's 16 x 16 tile D[row = 4 (lane >> 4) + reg][column = lane & 15] (mfma_16x16x4) of output tile ot.  The
// tiles go to red[wave][256 ot + 16 row + column], ONE barrier, and element i = r * COLS + c (r over the 16 OT rows, c < COLS
// <= 16) of the block's `count` sums is the four waves' as (0 + 1) + (2 + 3), written to slot[i].
template <int COLS, int OT>
__device__ __forceinline__ void mfma_tiles_partial(const f32x4 (&acc)[OT], float (&red)[kBlock / kWave][256 * OT],
                                                   float* slot, int count) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int m = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int ot = 0; ot < OT; ++ot)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) red[wave][256 * ot + (4 * kq + reg) * 16 + m] = acc[ot][reg];
  __syncthreads();
  for (int i = threadIdx.x; i < count; i += kBlock) {
    const int r = i / COLS, c = i - r * COLS;
    const int e = r * 16 + c;   // = 256 (r / 16) + 16 (r % 16) + c
    slot[i] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
  }
}

// ---- the quarter-row LayerNorm of the head forward ---------------------------------------------------------
// A row's T values lie in the float4s of the T/4 lanes 16 and 32 apart (kmask = 1; the lanes beyond hold a clamped duplicate
// and kmask = 0): mean and variance are two masked sums over xor 16 and xor 32, then normalise, scale (lw4) and shift (lb4).
template <int T>
__device__ __forceinline__ float4 ln_quarter_row(float4 v, float kmask, float eps, const float4& lw4, const float4& lb4) {
  float s1 = ((v.x + v.y) + (v.z + v.w)) * kmask;
  s1 += __shfl_xor(s1, 16);
  s1 += __shfl_xor(s1, 32);
  const float mean = s1 * (1.0f / T);
  v.x -= mean; v.y -= mean; v.z -= mean; v.w -= mean;
  float s2 = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, v.w * v.w))) * kmask;
  s2 += __shfl_xor(s2, 16);
  s2 += __shfl_xor(s2, 32);
  const float rstd = rsqrtf(s2 * (1.0f / T) + eps);
  return make_float4(fmaf(v.x * rstd, lw4.x, lb4.x), fmaf(v.y * rstd, lw4.y, lb4.y), fmaf(v.z * rstd, lw4.z, lb4.z),
                     fmaf(v.w * rstd, lw4.w, lb4.w));
}

// ---- the chunk staging of the head backward ----------------------------------------------------------------
// Wl[c][t][o] = W[o][t][c0 + c] (the convolution's [To][T][C] layout; 0 for c >= cn or o >= To) and d[o] = the lane's dout
// row `src` (0 for o >= To, or when the lane is not live).  Every load is unconditional (clamped index, masked value) and all
// of them are issued before any use: as loops with a load and its use per trip hipcc emitted load, s_waitcnt vmcnt(0), use
// -- 6 + 12 dependent round trips in front of every block's first store (110 us for a 293 MB write).  The caller's barrier
// follows.
template <int CC, int T, int OW>
__device__ __forceinline__ void head_bwd_stage(const float* __restrict__ W, const float* __restrict__ src, int C, int c0, int cn,
                                               int To, bool live, float (&d)[OW], float (&Wl)[CC][T][OW]) {
  constexpr int kWn = (CC * OW * T + kBlock - 1) / kBlock;
  float wv[kWn];
#pragma unroll
  for (int k = 0; k < kWn; ++k) {
    const int i = min((int)threadIdx.x + k * kBlock, CC * OW * T - 1);
    const int c = i / (OW * T), t = (i / OW) % T, o = i % OW;
    const float w = W[((size_t)min(o, To - 1) * T + t) * C + c0 + min(c, cn - 1)];
    wv[k] = (c < cn && o < To) ? w : 0.f;
  }
#pragma unroll
  for (int o = 0; o < OW; ++o) {
    const float v = src[min(o, To - 1)];
    d[o] = (o < To && live) ? v : 0.f;
  }
#pragma unroll
  for (int k = 0; k < kWn; ++k) {
    const int i = threadIdx.x + k * kBlock;
    if (i < CC * OW * T) (&Wl[0][0][0])[i] = wv[k];
  }
}

}  // namespace msgat
