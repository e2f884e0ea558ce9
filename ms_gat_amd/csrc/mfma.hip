// The two GEMM-shaped pieces of the hot path on the matrix cores (exact fp32 MFMA,
// v_mfma_f32_16x16x4_f32: bit-for-bit an fmaf chain, so the 1e-4 bar is untouched): the projection here, the
// contraction in contract.hip.
//
//   k_project_mfma   out[g,co,p] = sum_ci M(co,ci) in[g,ci,p] (+ addvec[co] extra[g,p]),  q = alpha . in
//                    forward: u = W x (msgat.py:27 applied before the aggregation), q (attention.py:33)
//                    backward: dy = W^T dz, dx = W^T du + alpha (x) dq
//   k_chanpair_*     part[a,c] = sum_p A[g,a,p] B[g,c,p]   (dW = du x^T, dalpha = dq . x, dW = dz y^T; contract.hip)
//
// Both stream their operands from HBM in the reference's [B,C,N,T] layout (a (group, channel)
// slab is contiguous over p = n*T + t) and are HBM-bound by design.  What limits such a kernel
// on CDNA4 is bytes in flight per SIMD, so the small 16x16 tile (4 accumulator registers) is used:
// it keeps 3-4 waves per SIMD resident, each with 8 x 1 KiB loads outstanding.
//   - projection: positions ride on the MFMA's N axis.  Lane (j = lane & 15, kq = lane >> 4)
//     loads one float4 = 4 consecutive positions of channel 4k + kq; its 4 components feed 4
//     independent 16x16 tiles, so one 16-B load per lane drives 4 MFMAs per 16 output channels
//     and the 4 result tiles re-assemble into float4 stores.  The matrix is the A operand (LDS).
//   - contraction: positions ride on K and channels on the lanes, the worst case for global
//     loads, so 256-position tiles of all rows are staged through LDS in 1-KiB row pieces by a
//     persistent split-K kernel (contract.hip).
#include "common.hpp"

namespace msgat {

// ---------------------------------------------------------------------------------------------
// projection
// ---------------------------------------------------------------------------------------------
constexpr int kKC = 8;  // k-steps (groups of 4 input channels) per register buffer
constexpr int kProjMaxMG = 7;

__host__ __device__ static inline int proj_kpad(int Kx) {
  const int K4 = (Kx + 3) & ~3;
  return K4 + 2;  // Kpad/2 odd: the 16 rows x 2 k-quarters of a half-wave fragment read hit 32 banks
}

// MG = output-channel tiles (of 16) held in accumulators per pass over the input channels.
// The k-loop keeps kKC loads in flight per wave in a register ring: slot i is re-issued for k-step
// k + kKC right after k-step k consumed it.  Every load is unconditional (addresses are clamped,
// padding is neutralised by zero matrix entries): a load inside a branch makes hipcc fall back
// to s_waitcnt vmcnt(0), which serialises the prefetch against the MFMAs.
// Global-address-space views of pointers that reach the kernel through LDS (the row-pointer table) or through a
// select between kernel arguments: hipcc cannot prove such a pointer global and falls back to flat_load, which counts
// on BOTH vmcnt and lgkmcnt -- every LDS operand read of the MFMAs then waits for the whole register ring
// (s_waitcnt vmcnt(0) lgkmcnt(0) at the top of each chunk: load burst, drain, compute, instead of a ring).
typedef const f32x4 __attribute__((address_space(1)))* gf4_in;   // (a builtin vector: float4 is a class, whose
typedef f32x4 __attribute__((address_space(1)))* gf4_out;         //  copy constructor only binds generic references)
__device__ __forceinline__ float4 load_global(const float* p) {
  const f32x4 v = *(gf4_in)(const f32x4*)p;
  return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void store_global(const float* p, const float4& v) {
  const f32x4 w = {v.x, v.y, v.z, v.w};
#ifdef MSGAT_PROJ_NT
  __builtin_nontemporal_store(w, (gf4_out)(f32x4*)const_cast<float*>(p));
#else
  *(gf4_out)(f32x4*)const_cast<float*>(p) = w;
#endif
}

#ifndef MSGAT_PROJ_LB
#define MSGAT_PROJ_LB 2   // waves per SIMD the register allocation must leave room for (= blocks per CU)
#endif
// TAPS: a causal dilated [1,2] convolution (msgat.py:69-74 behind a Chomp; its autograd with tshift > 0) in ONE pass:
//   out[co,n,t] = sum_ci W0[co,ci] in[ci,n,t + tshift] + W1[co,ci] in[ci,n,t]     (terms outside 0 <= t + tshift < T are zero)
// The input's Cr rows appear as 2 Cr virtual channels -- the first Cr shifted along time, the second Cr plain -- under
// the matrix [W0 | W1]; a lane's float4 is 4 consecutive timesteps of ONE row of T (T % 4 == 0), so the shifted
// operand is one unaligned 16-B load of the same row plus a lane-constant element mask.  Replaces the channel mixing
// Cr -> 2 Co, the [G,2Co,N,T] intermediate and the time-mixing pass of every TACN layer whose taps are constant shifts.

template <int MG, bool DO_Q, bool ONEPASS, bool SEGS, bool HAS_ADD, bool TAPS = false>
__global__ __launch_bounds__(kBlock, MSGAT_PROJ_LB) void k_project_mfma(
    SegList in, const float* __restrict__ M, int m_in_major,
    const float* __restrict__ qvec, const float* __restrict__ addvec,
    const float4* __restrict__ extra4, SegList out, float4* __restrict__ q4, int Bg,
    int P4, MixEpilogue epi, int tshift = 0, int T = 4) {
  extern __shared__ float lds[];
  const int Cr = in.total();                  // rows the input really has
  const int Ci = TAPS ? 2 * Cr : Cr, Co = out.total();
  const bool has_extra = addvec != nullptr;
  const int Kx = Ci + (has_extra ? 1 : 0);  // the extra "channel" carries addvec (x) extra
  const int K4 = (Kx + 3) >> 2;             // k-steps
  const int Kpad = proj_kpad(Kx);
  const int Mt = cdiv(Co, 16);
  const int Mrows = cdiv(Mt, MG) * MG * 16;  // rows padded to whole passes (zeros)
  float* Wl = lds;                           // [Mrows][Kpad]
  float* ql = lds + Mrows * Kpad;            // [4*K4]
  float* bl = ql + 4 * K4;                   // [Mrows] bias of every output row (0 without one)
  const int g = blockIdx.y;
  const int r = g / Bg;

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j = lane & 15, kq = lane >> 4;
  const int p4 = (blockIdx.x * 4 + wave) * 16 + j;
  const bool pvalid = p4 < P4;
  const int p4c = min(p4, P4 - 1);  // out-of-range lanes re-read the last position; their stores are masked
  const float4* ex = has_extra ? extra4 + (size_t)g * P4 + p4c : nullptr;   // already at this lane's position

  // SEGS: the segment lists (3 x 26 scalars) are resolved ONCE per block into a row-pointer table in LDS
  // -- entry c = address of channel c of this group.  Looked up per load from the kernel arguments they
  // spilled the scalar registers and halved the occupancy (203 us for a pass that takes 66 us unsegmented).
  const float** rowtab = reinterpret_cast<const float**>(lds + ((Mrows * Kpad + 4 * K4 + Mrows + 1) & ~1));  // [Ci | Co | Co]
  if (SEGS) {
    for (int c = threadIdx.x; c < Ci; c += kBlock) rowtab[c] = in.row(g, c, 4 * P4);
    for (int c = threadIdx.x; c < Co; c += kBlock) {
      rowtab[Ci + c] = out.row(g, c, 4 * P4);
      rowtab[Ci + Co + c] = HAS_ADD ? epi.add.row(g, c, 4 * P4) : nullptr;
    }
    __syncthreads();
  }

  // channel 4*kk + kq of this lane's 4 positions; padding channels alias a real one (their matrix
  // column is zero) -- never a branch
  // TAPS: lane constants of the shifted operand.  Element e of the lane's float4 is timestep t0 + e of its row; the
  // shifted value in[t0 + e + tshift] exists iff 0 <= t0 + e + tshift < T.  At the two ends of a channel row the
  // unaligned load would leave the row (and, for the first / last row of the tensor, the allocation): there the lane
  // loads its own (aligned) float4 instead and moves the elements in registers.
  const int t0 = TAPS ? (4 * p4c) % T : 0;
  const int spos = 4 * p4c + tshift;                                  // first element of the shifted float4
  const int sfix = TAPS ? (spos < 0 ? 1 : (spos > 4 * P4 - 4 ? 2 : 0)) : 0;
  float4 km = make_float4(1.f, 1.f, 1.f, 1.f);
  if (TAPS) {
    km.x = (t0 + 0 + tshift >= 0 && t0 + 0 + tshift < T) ? 1.f : 0.f;
    km.y = (t0 + 1 + tshift >= 0 && t0 + 1 + tshift < T) ? 1.f : 0.f;
    km.z = (t0 + 2 + tshift >= 0 && t0 + 2 + tshift < T) ? 1.f : 0.f;
    km.w = (t0 + 3 + tshift >= 0 && t0 + 3 + tshift < T) ? 1.f : 0.f;
  }
  const int sabs = tshift < 0 ? -tshift : tshift;
  auto loadB = [&](int kk) -> float4 {
    const int ci = 4 * min(kk, K4 - 1) + kq;
    if (TAPS) {   // raw load only: what the value still needs (tap_fix) happens when it is consumed, not in front of the ring
      const int cv = min(ci, Ci - 1);                // virtual channel: < Cr shifted, >= Cr plain
      const bool sh = cv < Cr;
      const float* base = in.template row<false>(g, sh ? cv : cv - Cr, 4 * P4);
      return load_global_a4(base + ((sh && sfix == 0) ? spos : 4 * p4c));
    }
    const float* base = SEGS ? rowtab[min(ci, Ci - 1)] : in.template row<false>(g, min(ci, Ci - 1), 4 * P4);
    const float* p = (ci == Ci && has_extra) ? reinterpret_cast<const float*>(ex) : base + 4 * (size_t)p4c;
    return load_global(p);
  };
  // TAPS, at consume time (branch-free: every lane runs the selects): a shifted channel's float4 gets its row-end
  // correction -- the own float4 moved by |tshift| elements where the unaligned load would have left the row -- and the
  // lane's timestep mask
  auto tap_fix = [&](int kk, float4 v) -> float4 {
    const bool sh = min(4 * min(kk, K4 - 1) + kq, Ci - 1) < Cr;
    const float4 right = make_float4(0.f, sabs == 1 ? v.x : 0.f, sabs == 1 ? v.y : (sabs == 2 ? v.x : 0.f),
                                     sabs == 1 ? v.z : (sabs == 2 ? v.y : (sabs == 3 ? v.x : 0.f)));
    const float4 left = make_float4(sabs == 1 ? v.y : (sabs == 2 ? v.z : (sabs == 3 ? v.w : 0.f)),
                                    sabs == 1 ? v.z : (sabs == 2 ? v.w : 0.f), sabs == 1 ? v.w : 0.f, 0.f);
    const bool r1 = sh && sfix == 1, r2 = sh && sfix == 2;
    v.x = r1 ? right.x : (r2 ? left.x : v.x); v.y = r1 ? right.y : (r2 ? left.y : v.y);
    v.z = r1 ? right.z : (r2 ? left.z : v.z); v.w = r1 ? right.w : (r2 ? left.w : v.w);
    v.x = (sh && km.x == 0.f) ? 0.f : v.x; v.y = (sh && km.y == 0.f) ? 0.f : v.y;   // selects, not products: what is
    v.z = (sh && km.z == 0.f) ? 0.f : v.z; v.w = (sh && km.w == 0.f) ? 0.f : v.w;   // masked belongs to another row
    return v;
  };

  // ONEPASS (all output tiles fit the accumulators, the usual case): the first chunk of the stream is
  // requested BEFORE the matrix is staged, so the block's prologue (matrix -> LDS, barrier) runs under
  // the HBM latency of those loads instead of ahead of it.  With several passes the ring is (re)loaded
  // at the top of each pass -- never inside a branch, which would cost the counted vmcnt waits.
  float4 ring[kKC];
  if (ONEPASS) {
#pragma unroll
    for (int i = 0; i < kKC; ++i) ring[i] = loadB(i);
  }

  // matrix -> LDS: 4 independent, unconditional (clamped) loads per trip, padding zeroed by select
  const int total = Mrows * Kpad;
  for (int i0 = threadIdx.x; i0 < total; i0 += 4 * kBlock) {
    float w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = min(i0 + u * kBlock, total - 1);
      const int co = i / Kpad, k = i - co * Kpad;
      const int coc = min(co, Co - 1), kc = min(k, Ci - 1);
      // TAPS, row-major taps [R, 2 Co, Cr] = [W0; W1]: M'(co, k) = W_{k / Cr}[co, k % Cr]; in-major (the backward's
      // transposed pass over [R, 2 Co', Cr'] with Co' = Cr here) is the plain in-major indexing of that same array
      const float m = m_in_major ? M[((size_t)r * Ci + kc) * Co + coc]
                      : (TAPS ? M[((size_t)r * 2 * Co + (size_t)(kc / Cr) * Co + coc) * Cr + kc % Cr]
                              : M[((size_t)r * Co + coc) * Ci + kc]);
      const float a = has_extra ? addvec[r * Co + coc] : 0.f;
      w[u] = (co < Co) ? ((k < Ci) ? m : ((k == Ci) ? a : 0.f)) : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i0 + u * kBlock < total) Wl[i0 + u * kBlock] = w[u];
  }
  if (DO_Q)
    for (int i = threadIdx.x; i < 4 * K4; i += kBlock) ql[i] = (i < Ci) ? qvec[r * Ci + i] : 0.f;
  for (int i = threadIdx.x; i < Mrows; i += kBlock)
    bl[i] = (epi.bias != nullptr && i < Co) ? epi.bias[(size_t)r * epi.bias_rstride + i] : 0.f;
  __syncthreads();
  const float relu_floor = epi.relu ? 0.f : -3.4e38f;   // kernel-uniform: max(v, floor) is the ReLU or nothing

  float4 qa = f4zero();
  for (int m0 = 0; m0 < Mt; m0 += MG) {
    f32x4 acc[MG][4];
#pragma unroll
    for (int mg = 0; mg < MG; ++mg)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[mg][i] = f32x4_zero();
    const float* wrow = Wl + (m0 * 16 + j) * Kpad + kq;  // A fragment: row co = tile*16 + j, column 4k + kq
    if (!ONEPASS) {
#pragma unroll
      for (int i = 0; i < kKC; ++i) ring[i] = loadB(i);
    }
    auto step = [&](int kk, const float4& braw) {
      const float4 b = TAPS ? tap_fix(kk, braw) : braw;
#pragma unroll
      for (int mg = 0; mg < MG; ++mg) {
        const float a = wrow[mg * 16 * Kpad + 4 * kk];
        acc[mg][0] = mfma_16x16x4(a, b.x, acc[mg][0]);
        acc[mg][1] = mfma_16x16x4(a, b.y, acc[mg][1]);
        acc[mg][2] = mfma_16x16x4(a, b.z, acc[mg][2]);
        acc[mg][3] = mfma_16x16x4(a, b.w, acc[mg][3]);
      }
      if (DO_Q && m0 == 0) f4fma(ql[4 * kk + kq], b, qa);
    };
    // whole chunks: one straight-line basic block per trip, so hipcc emits counted vmcnt waits
    int k0 = 0;
    for (; k0 + kKC <= K4; k0 += kKC) {
#pragma unroll
      for (int i = 0; i < kKC; ++i) {
        step(k0 + i, ring[i]);
        ring[i] = loadB(k0 + i + kKC);
      }
    }
    // tail (< kKC k-steps, already in the ring): wave-uniform branches, no loads inside
#pragma unroll
    for (int i = 0; i < kKC; ++i)
      if (k0 + i < K4) step(k0 + i, ring[i]);
    // D tile i: column = lane & 15 <-> position 4*p4 + i;  row = 4*(lane >> 4) + reg.
    // Epilogue = bias (LDS) + add operand + ReLU + store.  The add operand's 4 float4 of tile mg + 1 are requested
    // before tile mg is finished and stored, every load unconditional (clamped row and position): a load inside the
    // `co < Co` branch made hipcc emit load, s_waitcnt vmcnt(0), store -- 2 x 20 dependent round trips per wave.
    float4 addv[2][4];
    auto load_add = [&](int mg, float4 (&dst)[4]) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int coc = min((m0 + mg) * 16 + 4 * kq + reg, Co - 1);
        const float* arow = SEGS ? rowtab[Ci + Co + coc] : epi.add.template row<false>(g, coc, 4 * P4);
        dst[reg] = load_global(arow + 4 * (size_t)p4c);
      }
    };
    if (HAS_ADD) load_add(0, addv[0]);
#pragma unroll
    for (int mg = 0; mg < MG; ++mg) {
      if (HAS_ADD && mg + 1 < MG) load_add(mg + 1, addv[(mg + 1) & 1]);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int co = (m0 + mg) * 16 + 4 * kq + reg;
        const float b = bl[co];
        float4 v = make_float4(acc[mg][0][reg] + b, acc[mg][1][reg] + b, acc[mg][2][reg] + b, acc[mg][3][reg] + b);
        if (HAS_ADD) {
          const float4 a = addv[mg & 1][reg];
          v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
        }
        v.x = fmaxf(v.x, relu_floor); v.y = fmaxf(v.y, relu_floor); v.z = fmaxf(v.z, relu_floor); v.w = fmaxf(v.w, relu_floor);
        if (co < Co && pvalid) {
          const float* orow = SEGS ? rowtab[Ci + min(co, Co - 1)] : out.template row<false>(g, co, 4 * P4);
          store_global(orow + 4 * (size_t)p4, v);
        }
      }
    }
  }
  if (DO_Q) {  // the four lane quarters hold the 4k + kq channels' share of q
    qa.x += __shfl_xor(qa.x, 16); qa.y += __shfl_xor(qa.y, 16); qa.z += __shfl_xor(qa.z, 16); qa.w += __shfl_xor(qa.w, 16);
    qa.x += __shfl_xor(qa.x, 32); qa.y += __shfl_xor(qa.y, 32); qa.z += __shfl_xor(qa.z, 32); qa.w += __shfl_xor(qa.w, 32);
    if (kq == 0 && pvalid) q4[(size_t)g * P4 + p4] = qa;
  }
}

static int proj_passes_mg(int Co, int* mg_out) {
  const int Mt = cdiv(Co, 16);
  // all output tiles in one pass when they fit the accumulator registers: up to 7 x 16 channels (188 registers, two
  // waves per SIMD -- forced by the kernel's launch bounds, left alone the allocator took more than 256 and one wave).
  // A 72 -> 98 channel mixing in ONE pass over its input: 288 -> 252 us against two passes of 4 and 3 tiles.
  // Several passes: at most 6 tiles each -- the ring is re-loaded per pass there, and with 7 tiles that form needs
  // 2-4 registers more than the 256 a wave has (it spilled).
  const int passes = Mt <= kProjMaxMG ? 1 : cdiv(Mt, kProjMaxMG - 1);
  *mg_out = cdiv(Mt, passes);
  return passes;
}

size_t project_mfma_lds_bytes(int Ci, int Co, bool has_extra) {  // Ci, Co: totals over the segments
  const int Kx = Ci + (has_extra ? 1 : 0);
  int MG;
  const int passes = proj_passes_mg(Co, &MG);
  // matrix + q vector + bias per output row (+ 1 float of alignment) + the row-pointer table of the segmented form
  return (size_t)(passes * MG * 16 * proj_kpad(Kx) + 4 * ((Kx + 3) / 4) + passes * MG * 16 + 1) * sizeof(float) +
         (size_t)(Ci + 2 * Co) * sizeof(float*);
}

template <int MG>
static int launch_project_mg(const SegList& in, const float* M, int m_in_major, const float* qvec,
                             const float* addvec, const float* extra, const SegList& out, float* q, int G, int Bg,
                             int P4, const MixEpilogue& epi, hipStream_t s) {
  const int Ci = in.total(), Co = out.total();
  const size_t lds = project_mfma_lds_bytes(Ci, Co, addvec != nullptr);
  dim3 grid(cdiv(P4, 64), G);
  const bool one = cdiv(Co, 16) <= MG;
  const bool segs = in.n > 1 || out.n > 1 || epi.add.n > 1;
  const bool has_add = epi.add.n > 0;
  // (matrices beyond 64 KiB of LDS -- 96 -> 130 channels, the merged mixing of msgat96 -- need the kernel's dynamic-LDS
  // ceiling raised once per device; up to kProjLdsMax two blocks still share a CU)
#define MSGAT_PROJ(Q, ONE, SG, AD)                                                                                      \
  do {                                                                                                                  \
    static LdsGrant granted;                                                                                            \
    if (int st_ = grant_dynamic_lds(&k_project_mfma<MG, Q, ONE, SG, AD>, lds, granted)) return st_;                      \
    hipLaunchKernelGGL((k_project_mfma<MG, Q, ONE, SG, AD>), grid, dim3(kBlock), lds, s, in, M, m_in_major, qvec,        \
                       addvec, (const float4*)extra, out, (float4*)q, Bg, P4, epi);                                     \
  } while (0)
#define MSGAT_PROJ2(Q, ONE)                                                          \
  do {                                                                               \
    if (segs) { if (has_add) MSGAT_PROJ(Q, ONE, true, true); else MSGAT_PROJ(Q, ONE, true, false); }   \
    else { if (has_add) MSGAT_PROJ(Q, ONE, false, true); else MSGAT_PROJ(Q, ONE, false, false); }      \
  } while (0)
  if constexpr (MG == kProjMaxMG) {   // proj_passes_mg() hands out 7 tiles only when one pass covers the output
    if (!one) return MSGAT_ERR_UNSUPPORTED;
    if (qvec != nullptr) MSGAT_PROJ2(true, true); else MSGAT_PROJ2(false, true);
  } else {
    if (qvec != nullptr) { if (one) MSGAT_PROJ2(true, true); else MSGAT_PROJ2(true, false); }
    else { if (one) MSGAT_PROJ2(false, true); else MSGAT_PROJ2(false, false); }
  }
#undef MSGAT_PROJ2
#undef MSGAT_PROJ
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

int launch_project_mfma(const SegList& in, const float* M, int m_in_major, const float* qvec,
                        const float* addvec, const float* extra, const SegList& out, float* q, int G, int Bg,
                        int P, const MixEpilogue& epi, hipStream_t s) {
  const int P4 = P / 4;
  int MG;
  proj_passes_mg(out.total(), &MG);
  return dispatch_range<1, kProjMaxMG>(MG, [&](auto mg) {   // (a Co >= 1 gives 1 <= MG <= kProjMaxMG)
    return launch_project_mg<decltype(mg)::value>(in, M, m_in_major, qvec, addvec, extra, out, q, G, Bg, P4, epi, s);
  });
}

// ---- the same convolution with ONE load per input float4 (Cr % 4 == 0: the widths of the reference's models) ---------
// k_project_mfma<.., TAPS> loads every input row twice (the plain and the shifted operand): 12 loads per lane for 24
// channels, half of them unaligned -- it ran at 2.9 TB/s of its algorithmic bytes.  Here a wave covers GP4 = the largest
// multiple of T/4 that fits 16 lanes (15 float4 = 5 whole rows at T = 12, the 16th lane idle), so every row of T lies
// inside ONE 16-lane group and the shifted operand is a lane shuffle of the loaded values: float4 index f of a row holds
// timesteps 4f .. 4f+3, and in[t + s] for s = 4a + b comes from the float4s a and a + 1 lanes away (zero where the row
// ends).  No unaligned load, no second load, nothing that could leave the tensor.
template <int MG, int kMaxK>   // kMaxK: k-steps the registers hold (8: Cr <= 32, 16: Cr <= 64)
__global__ __launch_bounds__(kBlock, 2) void k_causal_conv(
    const float* __restrict__ in, int in_gstride, const float* __restrict__ taps, int m_in_major,
    const float* __restrict__ bias, int bias_rstride, float* __restrict__ out, int Bg, int P4, int Cr, int Co,
    int tshift, int T, int tiles, int per_block
#ifdef MSGAT_LAB
    , int lab   // MSGAT_LAB_CC: 1 = no lane shuffles (shifted operand = plain), 2 = only the plain half's MFMAs, 4 = no stores
#endif
    ) {
  extern __shared__ float lds[];
  const int Ci = 2 * Cr;                      // virtual channels [shifted | plain]
  const int K4r = Cr >> 2;                    // k-steps over the REAL channels (Cr % 4 == 0, host-checked)
  const int Kpad = proj_kpad(Ci);
  constexpr int Mrows = MG * 16;
  float* Wl = lds;                            // [Mrows][Kpad]
  float* bl = lds + Mrows * Kpad;             // [Mrows]
  const int g = blockIdx.y, r = g / Bg;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j = lane & 15, kq = lane >> 4;
  const int F = T >> 2;                       // float4s per row of T
  const int GP4 = (16 / F) * F;               // float4s a wave covers: whole rows only
  const float* gbase = in + (size_t)g * in_gstride * (4 * (size_t)P4);
  // a block works on `per_block` consecutive tiles (4 waves x GP4 float4s each); the next tile's input is requested before
  // the current one is multiplied, so only the first tile's round trip and one matrix staging are exposed per block (one
  // tile per block, 4320 blocks of 46 KB each at PEMSD7 size, ran at 2.9 TB/s)
  // the second register set fits beside the accumulators up to here (3 x 16 and 4 x 16 spill: those take one tile per
  // block, host-side per_block = 1, and a loop the compiler sees through)
  constexpr bool kPrefetch = kMaxK == 8 || MG <= 2;
  const int tile0 = blockIdx.x * (kPrefetch ? per_block : 1), tile1 = kPrefetch ? min(tile0 + per_block, tiles) : tile0 + 1;

  float4 own[kMaxK], nxt[kPrefetch ? kMaxK : 1];
  auto fetch = [&](int tile, auto& dst) {
    const int p4c = min((tile * 4 + wave) * GP4 + j, P4 - 1);
    const float* base = gbase + 4 * (size_t)p4c;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
      if (k < K4r) dst[k] = load_global(base + (size_t)(4 * k + kq) * (4 * (size_t)P4));   // kernel-uniform guard
  };
  fetch(tile0, own);                          // requested before the matrix is staged

  for (int i = threadIdx.x; i < Mrows * Kpad; i += kBlock) {
    const int co = i / Kpad, k = i - co * Kpad;
    const int coc = min(co, Co - 1), kc = min(k, Ci - 1);
    const float m = m_in_major ? taps[((size_t)r * Ci + kc) * Co + coc]
                               : taps[((size_t)r * 2 * Co + (size_t)(kc / Cr) * Co + coc) * Cr + kc % Cr];
    Wl[i] = (co < Co && k < Ci) ? m : 0.f;
  }
  for (int i = threadIdx.x; i < Mrows; i += kBlock)
    bl[i] = (bias != nullptr && i < Co) ? bias[(size_t)r * bias_rstride + i] : 0.f;
  __syncthreads();

  // lane constants of the shift: s = +-(4 a + b); source float4s a and a + 1 lanes away in the direction of the shift
  const int f = j % F;
  const int sabs = tshift < 0 ? -tshift : tshift, dir = tshift < 0 ? -1 : 1;
  const int a = sabs >> 2, b = sabs & 3;
  const bool vA = dir < 0 ? (f - a >= 0) : (f + a < F);
  const bool vB = dir < 0 ? (f - a - 1 >= 0) : (f + a + 1 < F);
  const int laneA = lane + dir * a, laneB = lane + dir * (a + 1);     // same kq group whenever the source is valid
  auto shifted = [&](const float4& v) -> float4 {
    float4 A = make_float4(__shfl(v.x, laneA), __shfl(v.y, laneA), __shfl(v.z, laneA), __shfl(v.w, laneA));
    float4 B = make_float4(__shfl(v.x, laneB), __shfl(v.y, laneB), __shfl(v.z, laneB), __shfl(v.w, laneB));
    A = vA ? A : f4zero();
    B = vB ? B : f4zero();
    if (dir < 0) {   // element e <- in[t0 + e - (4a + b)]: e >= b from A[e - b], else B[e - b + 4]
      return make_float4(b == 0 ? A.x : (b == 1 ? B.w : (b == 2 ? B.z : B.y)),
                         b == 0 ? A.y : (b == 1 ? A.x : (b == 2 ? B.w : B.z)),
                         b == 0 ? A.z : (b == 1 ? A.y : (b == 2 ? A.x : B.w)),
                         b == 0 ? A.w : (b == 1 ? A.z : (b == 2 ? A.y : A.x)));
    }
    // element e <- in[t0 + e + 4a + b]: e + b < 4 from A[e + b], else B[e + b - 4]
    return make_float4(b == 0 ? A.x : (b == 1 ? A.y : (b == 2 ? A.z : A.w)),
                       b == 0 ? A.y : (b == 1 ? A.z : (b == 2 ? A.w : B.x)),
                       b == 0 ? A.z : (b == 1 ? A.w : (b == 2 ? B.x : B.y)),
                       b == 0 ? A.w : (b == 1 ? B.x : (b == 2 ? B.y : B.z)));
  };

  const float* wrow = Wl + j * Kpad + kq;     // row co = tile*16 + j; column 4k + kq (shifted half), Cr + 4k + kq (plain half)
  for (int tile = tile0; tile < tile1; ++tile) {
    if constexpr (kPrefetch) {
      if (tile + 1 < tile1) fetch(tile + 1, nxt);   // block-uniform
    }
    f32x4 acc[MG][4];
#pragma unroll
    for (int mg = 0; mg < MG; ++mg)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[mg][i] = f32x4_zero();
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      if (k < K4r) {                            // kernel-uniform; MFMAs, shuffles and LDS reads only
        const float4 pl = own[k];
#ifdef MSGAT_LAB
        const float4 sh = (lab & 1) ? pl : shifted(pl);
#else
        const float4 sh = shifted(pl);
#endif
#pragma unroll
        for (int mg = 0; mg < MG; ++mg) {
          const float a0 = wrow[mg * 16 * Kpad + 4 * k];
          const float a1 = wrow[mg * 16 * Kpad + Cr + 4 * k];
#ifdef MSGAT_LAB
          if (!(lab & 2)) {
#endif
          acc[mg][0] = mfma_16x16x4(a0, sh.x, acc[mg][0]); acc[mg][1] = mfma_16x16x4(a0, sh.y, acc[mg][1]);
          acc[mg][2] = mfma_16x16x4(a0, sh.z, acc[mg][2]); acc[mg][3] = mfma_16x16x4(a0, sh.w, acc[mg][3]);
#ifdef MSGAT_LAB
          }
#endif
          acc[mg][0] = mfma_16x16x4(a1, pl.x, acc[mg][0]); acc[mg][1] = mfma_16x16x4(a1, pl.y, acc[mg][1]);
          acc[mg][2] = mfma_16x16x4(a1, pl.z, acc[mg][2]); acc[mg][3] = mfma_16x16x4(a1, pl.w, acc[mg][3]);
        }
      }
    }
    const int p4 = (tile * 4 + wave) * GP4 + j;
    const bool pvalid = j < GP4 && p4 < P4;
#pragma unroll
    for (int mg = 0; mg < MG; ++mg)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int co = mg * 16 + 4 * kq + reg;
        const float bb = bl[co];
        const float4 v = make_float4(acc[mg][0][reg] + bb, acc[mg][1][reg] + bb, acc[mg][2][reg] + bb, acc[mg][3][reg] + bb);
#ifdef MSGAT_LAB
        if ((lab & 4) && v.x != 12345.678f) continue;
#endif
        if (co < Co && pvalid) store_global(out + ((size_t)g * Co + co) * (4 * (size_t)P4) + 4 * (size_t)p4, v);
      }
    if constexpr (kPrefetch) {
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) own[k] = nxt[k];
    }
  }
}

// The causal dilated convolution in one pass (k_project_mfma<.., TAPS>): in [G,Cr,P] (a channel slice of a wider
// tensor when in_gstride > Cr), taps [R, 2 Co', Cr'] row-major; m_in_major = 0: forward (Co' = Co, Cr' = Cr, tshift =
// -dilation); m_in_major = 1: its input gradient (Co' = Cr, Cr' = Co: the same array read in-major, tshift = +dilation).
bool project_taps_supported(int Cr, int Co) {
  int MG;
  return Cr > 0 && Co >= 8 && proj_passes_mg(Co, &MG) == 1 && project_mfma_lds_bytes(2 * Cr, Co, false) <= (size_t)kProjLdsMax;
}

int launch_project_taps(const float* in, int in_gstride, const float* taps, int m_in_major, const float* bias,
                        int bias_rstride, float* out, int G, int Bg, int Cr, int Co, int P, int T, int tshift, hipStream_t s) {
  if (!project_taps_supported(Cr, Co) || T % 4 != 0 || P % T != 0 || tshift < -T || tshift > T) return MSGAT_ERR_UNSUPPORTED;
  SegList sin = seg_single(in, Cr);
  if (in_gstride > Cr) sin.gstride[0] = in_gstride;
  const SegList sout = seg_single(out, Co);
  MixEpilogue epi;
  epi.bias = bias;
  epi.bias_rstride = bias_rstride;
  const int P4 = P / 4;
  int MG;
  proj_passes_mg(Co, &MG);
  const size_t lds = project_mfma_lds_bytes(2 * Cr, Co, false);
#ifndef MSGAT_TAPS_TWO_LOADS
  if (Cr % 4 == 0 && Cr <= 64 && MG <= 4) {   // one load per input float4, the shifted operand by lane shuffles
    const int F = T / 4, GP4 = (16 / F) * F;
    const int tiles = cdiv(P4, 4 * GP4);
    // consecutive tiles per block (lab builds: MSGAT_LAB_CCPB).  Cold operands, G = 96, 24 -> 24 channels, tools/
    // causal_conv_time.py: N = 883 (4320 tiles) 98.6 / 85.8 / 83.3 / 92.1 us at 1 / 2 / 3 / 4; N = 307 (1536 tiles) 38.4 /
    // 35.0 / 40.8 / 39.5
    int per_block = std::max(1, std::min(3, (int)((long long)tiles * G / 768)));
    if (Cr > 32 && MG > 2) per_block = 1;      // no room for the prefetched tile's registers (kPrefetch)
#ifdef MSGAT_LAB
    per_block = lab_env("MSGAT_LAB_CCPB", per_block);
#endif
    const dim3 grid1(cdiv(tiles, per_block), G);
    const int gs = in_gstride > Cr ? in_gstride : Cr;
#ifdef MSGAT_LAB
#define MSGAT_CC_LAB , lab_env("MSGAT_LAB_CC", 0)
#else
#define MSGAT_CC_LAB
#endif
#define MSGAT_CC(mg, kk)                                                                                               \
  {                                                                                                                   \
    static LdsGrant granted;                                                                                          \
    if (int st_ = grant_dynamic_lds(&k_causal_conv<mg, kk>, lds, granted)) return st_;                                 \
    hipLaunchKernelGGL((k_causal_conv<mg, kk>), grid1, dim3(kBlock), lds, s, in, gs, taps, m_in_major, bias,           \
                       bias_rstride, out, Bg, P4, Cr, Co, tshift, T, tiles, per_block MSGAT_CC_LAB);                  \
  }
#define MSGAT_CC2(mg) case mg: if (Cr <= 32) MSGAT_CC(mg, 8) else MSGAT_CC(mg, 16) break;
    switch (MG) { MSGAT_CC2(1) MSGAT_CC2(2) MSGAT_CC2(3) MSGAT_CC2(4) }
#undef MSGAT_CC2
#undef MSGAT_CC
    MSGAT_CHECK_LAUNCH();
    return MSGAT_OK;
  }
#endif
  const dim3 grid(cdiv(P4, 64), G);
#define MSGAT_TAPS(mg)                                                                                                   \
  case mg: {                                                                                                            \
    static LdsGrant granted;                                                                                            \
    if (int st_ = grant_dynamic_lds(&k_project_mfma<mg, false, true, false, false, true>, lds, granted)) return st_;     \
  }                                                                                                                     \
    hipLaunchKernelGGL((k_project_mfma<mg, false, true, false, false, true>), grid, dim3(kBlock), lds, s, sin, taps,     \
                       m_in_major, (const float*)nullptr, (const float*)nullptr, (const float4*)nullptr, sout,           \
                       (float4*)nullptr, Bg, P4, epi, tshift, T);                                                       \
    break;
  switch (MG) {
    MSGAT_TAPS(1) MSGAT_TAPS(2) MSGAT_TAPS(3) MSGAT_TAPS(4) MSGAT_TAPS(5) MSGAT_TAPS(6) MSGAT_TAPS(7)
    default: return MSGAT_ERR_UNSUPPORTED;
  }
#undef MSGAT_TAPS
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

}  // namespace msgat
