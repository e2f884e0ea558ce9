// The channel-pair contraction of the hot path on the matrix cores (exact fp32 MFMA, v_mfma_f32_16x16x4_f32):
//   part[a,c] = sum_p A[g,a,p] B[g,c,p]   (dW = du x^T, dalpha = dq . x, dW = dz y^T: every weight gradient of the 1x1
//   and causal convolutions)
// twice -- k_chanpair_mfma stages its tiles through registers, k_chanpair_glds by LDS-DMA -- from ONE source for what
// the two share and can share at no cost: the block decode (cp_block) and the block's run of the tile stream
// (cp_tile_run); host side the z-block cut, block count, grid and form probe (cp_leaf, cp_probed).  What differs for a
// reason -- the staging itself, the column split of the z-blocks, how tail positions are zeroed -- stays in its kernel
// and says why, and so do three pieces that cost registers or time when shared (see below).
// Operands stream from HBM in the reference's [B,C,N,T] layout, like the projection's (mfma.hip).
#include "common.hpp"
#include <cstdarg>
#include <cstdio>

namespace msgat {

// ---------------------------------------------------------------------------------------------
// channel-pair contraction over positions
// ---------------------------------------------------------------------------------------------
// part[a,c] = sum_{g in r} sum_p A[g,a,p] B[g,c,p]: positions are the MFMA's K axis, channels ride
// on the lanes, so an operand fragment is "one word per channel row" -- the worst possible global
// access.  A block (8 waves, one block per CU) therefore stages 256-position tiles of all its
// Ca + Cb rows through LDS:
//   - global side: one wave-instruction reads 1 KiB contiguous of ONE row.  A row of the [N,T]
//     slab starts at an arbitrary 16-B offset (N*T*4 is not a multiple of 128), so every piece
//     straddles one extra 128-B line: 1-KiB pieces cost 9 lines per 8, 64-B pieces 2 per 1
//     (measured with 64-B pieces: 2.5 TB/s).  Every byte of A and B is read once.
//   - LDS side: rows are padded by 16 B so the 16 rows x 4 words of a fragment read
//     (ds_read_b32, row = lane & 15, word = lane >> 4 of a 16-B chunk) are 2-way banked;
//   - wave w multiplies positions [32w, 32w+32) of the tile: 8 k-steps of 4 positions.
// Persistent split-K: the tiles of a relation (its Bg groups back to back) form one stream and each
// block owns a contiguous run of it, so the load pipeline (two tiles in flight per wave, in two
// register sets) never drains between groups and there is ONE reduction per block: the 8 waves'
// accumulators are summed in a fixed order into the block's partial (no atomics).  In-kernel
// stamps showed the alternative -- one block per (group, 1024 positions) -- spending 45% of a
// block in its exposed prologue, first-tile wait and reduction.

// lds_barrier() (common.hpp): the workgroup barrier for LDS hand-offs that leaves global loads in flight.

constexpr int kCpWaves = 8;
constexpr int kCpBlock = 64 * kCpWaves;
constexpr int kTile = 32 * kCpWaves;   // positions per staged tile (default): 32 (8 k-steps) per wave

// ---- the steps both kernels are built from ---------------------------------------------------------------------------
// Block -> (relation r, run bx of the relation's tile stream, z-block zb of the channel matrix).  A channel matrix
// larger than one [MA*16 x NB*16] block is cut into nza x nzb z-blocks that each stream their own A rows and B
// columns -- the z-blocks of one A split all re-read the SAME B tiles.  With several z-blocks the grid is
// one-dimensional and XCD-aware: workgroups are dealt round-robin over the 8 XCDs (block b on XCD b % 8), so the
// z-blocks of one run take consecutive slots of ONE XCD, start together, do equal work (A rows split evenly: 49 + 49
// of 98, not 64 + 34) and stay in step -- the second reader of a B tile finds it in that XCD's L2.  (As a 3-D grid
// with z slowest, all z = 0 blocks ran first and z = 1 re-read B from HBM 170 us later.)
// False: the grid is padded to a multiple of 8 runs and this block is padding -- it returns at once and writes nothing.
__device__ __forceinline__ bool cp_block(int nz, int nblk, int R, int& bx, int& r, int& zb) {
  if (nz > 1) {
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;   // the map of xcd_group_slot (common.hpp: why it is written out)
    zb = slot % nz;
    const int k = (slot / nz) * 8 + xcd;
    r = k / nblk;
    bx = k - r * nblk;
    return k < nblk * R;
  }
  bx = blockIdx.x;
  r = blockIdx.y;
  zb = 0;
  return true;
}

// Run bx of nblk of a relation's tile stream (its Bg groups back to back, tpg tiles of `tile` positions per group, the
// last one partial): tiles t0 .. t0 + ntile - 1
struct CpRun {
  int tpg, t0, ntile;
};
__device__ __forceinline__ CpRun cp_tile_run(int P, int tile, int Bg, int bx, int nblk) {
  const int tpg = cdiv(P, tile);
  const long long ntot = (long long)Bg * tpg;
  const int t0 = (int)(ntot * bx / nblk), t1 = (int)(ntot * (bx + 1) / nblk);
  return {tpg, t0, t1 - t0};
}

// The other three pieces the kernels have in common -- where a staged row lives, one k-step of the multiply, the
// fixed-order reduction of the waves' accumulators -- stay written out in each kernel: as shared functions they moved
// the LDS-DMA forms' register allocation (10 - 27 VGPRs), the k-step cost k_chanpair_glds<2,5,128,3,1>, the hot path's
// pass, 2 us of 193, and with only the k-step written out again k_chanpair_glds<9,4,64,3,2> spilled
// (profiles/contract_shared/lab_variants.txt).  A change to the reduction order or the row plan is made in both.

// ---- staged through registers ----------------------------------------------------------------------------------------

// TWO = false: one register set in flight instead of two -- what the [64 x 80] block (MA = 4) has registers for.  It
// exists for operands with 49..64 A channels per z-block: a 98-channel gradient against 73 channels (the merged
// channel mixing of a MEAM block) takes 2 z-blocks instead of 3, i.e. reads B twice instead of three times.
// TILE = 128: half-length tiles (512-B row pieces, two rows per wave-instruction, 4 k-steps per wave).  Half the LDS
// per row, so [80 x 80] and [112 x 80] channel blocks fit: a 72- or 98-channel gradient against 73 channels is ONE
// pass over both operands instead of two z-blocks that each re-read B.
// SHIFT: the A operand's Cr real rows appear as 2 Cr virtual rows -- row a < Cr is row a read `ashift` timesteps LATER
// (A[a, n, t + ashift], zero where t + ashift >= T), row a >= Cr is row a - Cr as it stands: [dout[t+d]; dout], the
// gradient at the two taps of a causal dilated convolution (msgat.py:69-74), without a pass that writes it out.  The
// shifted float4 is an unaligned load of the same row of T (a float4 never straddles rows: T % 4 == 0); the last
// float4 of a slab, where that load would leave the tensor, is its own float4 moved in registers.
struct TimeShift {
  int d = 0;   // 0: no virtual rows
  int T = 4;
};

template <int MA, int NB, bool TWO = true, int TILE = kTile, bool SHIFT = false>
__global__ __launch_bounds__(kCpBlock) void k_chanpair_mfma(
    SegList A, const float* __restrict__ B, float* __restrict__ part, int Cb, int P, int Bg, int nzb, int b_ones,
    int nza, int nblk, int R, TimeShift ts) {
  // b_ones: B's last channel (index Cb-1) is a virtual row of ones, so part[a, Cb-1] = sum_p A[a,p] -- the bias
  // gradient of a 1x1 convolution comes out of the contraction that computes its weight gradient
  const int Cbr = Cb - b_ones;  // channels B really has
  const int Cr = A.total();     // rows A really has
  const int Ca = SHIFT ? 2 * Cr : Cr;
  extern __shared__ float4 lds4[];
  constexpr int kLPR = TILE / 4;        // lanes per row piece (64: one row per wave-instruction)
  constexpr int kRPI = 64 / kLPR;        // rows per wave-instruction
  constexpr int kRowF4 = TILE / 4 + 1;  // float4s per LDS row (piece + 16 B pad)
  constexpr int kPPW = TILE / kCpWaves;  // positions per wave and tile: 4 per k-step
  constexpr int RPW = ((MA + NB) * 16 + kCpWaves * kRPI - 1) / (kCpWaves * kRPI);  // load instructions per wave per tile
  int bx, r, zb;
  if (!cp_block(nza * nzb, nblk, R, bx, r, zb)) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j = lane & 15, kq = lane >> 4;
  const int a_per = cdiv(Ca, nza);  // A rows per z-block (<= MA * 16, host-checked)
  const int a0 = (zb / nzb) * a_per;
  const int c0 = (zb % nzb) * (NB * 16);   // whole [. x 16 NB] blocks over B: the host cut it by the block width
  const int ca = min(a_per, Ca - a0), cb = min(NB * 16, Cb - c0);
  const int rows = ca + cb;  // rows [0,ca) = A channels, [ca,rows) = B channels
  constexpr int kZeroRow = (MA + NB) * 16;  // an all-zero row for absent channels
  constexpr int kOnesRow = kZeroRow + 1;    // an all-ones row for the virtual channel
  const CpRun run = cp_tile_run(P, TILE, Bg, bx, nblk);
  const int tpg = run.tpg, t0 = run.t0, ntile = run.ntile;

  if (threadIdx.x < kRowF4) {
    lds4[kZeroRow * kRowF4 + threadIdx.x] = f4zero();
    lds4[kOnesRow * kRowF4 + threadIdx.x] = make_float4(1.f, 1.f, 1.f, 1.f);
  }

  // staging plan: instruction k of this wave covers rows (wave + kCpWaves*k)*kRPI + (lane / kLPR); a
  // lane fetches float4 (lane % kLPR) of the tile.  Rows past the last one alias row 0 (always a
  // valid address: no load sits in a branch, see k_project_mfma) and land in scratch rows nobody reads.
  const int lrow = lane / kLPR, lcol = lane % kLPR;
  const float* src[RPW];  // row pointer for group 0 of the relation
  int gstride[RPW];       // elements between consecutive groups of that row
  unsigned shifted = 0;   // SHIFT: bit k = instruction k of this lane stages a time-shifted row
  static_assert(RPW <= 32, "one flag bit per staging instruction");
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    const int rr = (wave + kCpWaves * k) * kRPI + lrow;
    const int row = rr < rows ? rr : 0;
    const size_t g0 = (size_t)r * Bg;
    const float* p;
    if (row < ca) {  // A channel a0 + row: its segment's tensor and group stride
      const int av = a0 + row;                       // virtual row
      const int a = SHIFT ? (av < Cr ? av : av - Cr) : av;
      if (SHIFT && av < Cr) shifted |= 1u << k;
      int sk = 0;
#pragma unroll
      for (int i = 1; i < kMaxSeg; ++i) sk += (i < A.n && a >= A.begin[i]) ? 1 : 0;
      p = A.row((int)g0, a, P);
      int gs = A.gstride[0];
#pragma unroll
      for (int i = 1; i < kMaxSeg; ++i) gs = (i == sk) ? A.gstride[i] : gs;
      gstride[k] = gs * P;
    } else {
      p = B + (g0 * Cbr + min(c0 + row - ca, Cbr - 1)) * P;  // the virtual row aliases a real one; nobody reads its copy
      gstride[k] = Cbr * P;
    }
    src[k] = p + 4 * lcol;
  }
  const int plast = P - 4 - 4 * lcol;  // clamp so that the float4 stays inside the row (P % 4 == 0)
  auto fetch = [&](int t, float4 (&regs)[RPW], int& pos) {  // t relative to t0, clamped to the run
    const int tau = t0 + min(t, ntile - 1);
    const int b = tau / tpg;
    const int p0 = (tau - b * tpg) * TILE;
    const float keep = (p0 + 4 * lcol < P) ? 1.f : 0.f;
    const int poff = min(p0, plast);
    pos = poff + 4 * lcol;                                   // SHIFT: the lane's first position in the slab, for stash()
    const int soff = (SHIFT && pos + ts.d <= P - 4) ? ts.d : 0;   // the slab's last float4 stays put (moved in stash())
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
      // tail positions are zeroed HERE, on the way through the registers, and by a multiply, not a select: hipcc sinks a load that only feeds a
      // select into a branch, and a load inside a branch costs the counted vmcnt waits (the
      // clamped address re-reads finite in-row data, so x * 0 is exact)
      const float* gp = src[k] + (size_t)b * gstride[k] + poff;
      float4 v;
      if (SHIFT) v = load_global_a4(gp + (((shifted >> k) & 1u) ? soff : 0));
      else v = *reinterpret_cast<const float4*>(gp);
      regs[k] = make_float4(v.x * keep, v.y * keep, v.z * keep, v.w * keep);
    }
  };
  auto stash = [&](const float4 (&regs)[RPW], int pos) {
    // SHIFT (when the values are consumed, not in front of the loads): element e of a shifted row's float4 is timestep
    // tq + e + d of its row of T and exists iff that is < T; at the slab's last float4 the own values move left by d
    const int tq = SHIFT ? pos % ts.T : 0;
    const bool atend = SHIFT && pos + ts.d > P - 4;
    const int d = ts.d;
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
      const int rr = (wave + kCpWaves * k) * kRPI + lrow;
      float4 v = regs[k];
      if (SHIFT) {
        const bool sh = (shifted >> k) & 1u;
        const float4 left = make_float4(d == 1 ? v.y : (d == 2 ? v.z : (d == 3 ? v.w : 0.f)),
                                        d == 1 ? v.z : (d == 2 ? v.w : 0.f), d == 1 ? v.w : 0.f, 0.f);
        const bool mv = sh && atend;
        v.x = mv ? left.x : v.x; v.y = mv ? left.y : v.y; v.z = mv ? left.z : v.z; v.w = mv ? left.w : v.w;
        v.x = (sh && tq + 0 + d >= ts.T) ? 0.f : v.x; v.y = (sh && tq + 1 + d >= ts.T) ? 0.f : v.y;
        v.z = (sh && tq + 2 + d >= ts.T) ? 0.f : v.z; v.w = (sh && tq + 3 + d >= ts.T) ? 0.f : v.w;
      }
      if (rr < kZeroRow) lds4[rr * kRowF4 + lcol] = v;
    }
  };

  // fragment words of this lane: word kq of chunk (8*wave + qq) of its row
  const float* ldsw = reinterpret_cast<const float*>(lds4);
  int aw[MA], bw[NB];
#pragma unroll
  for (int ma = 0; ma < MA; ++ma) {
    const int row = (ma * 16 + j < ca) ? ma * 16 + j : kZeroRow;
    aw[ma] = row * (kRowF4 * 4) + kPPW * wave + kq;
  }
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int cl = nb * 16 + j;
    const int row = (cl < cb) ? ((b_ones && c0 + cl == Cbr) ? kOnesRow : ca + cl) : kZeroRow;
    bw[nb] = row * (kRowF4 * 4) + kPPW * wave + kq;
  }

  f32x4 acc[MA][NB];
#pragma unroll
  for (int ma = 0; ma < MA; ++ma)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[ma][nb] = f32x4_zero();

  auto multiply = [&]() {
#pragma unroll
    for (int qq = 0; qq < kPPW / 4; ++qq) {
      float av[MA], bv[NB];
#pragma unroll
      for (int ma = 0; ma < MA; ++ma) av[ma] = ldsw[aw[ma] + 4 * qq];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) bv[nb] = ldsw[bw[nb] + 4 * qq];
#pragma unroll
      for (int ma = 0; ma < MA; ++ma)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[ma][nb] = mfma_16x16x4(av[ma], bv[nb], acc[ma][nb]);
    }
  };
  // two tiles in flight per wave (two register sets): while tile t is multiplied the loads of
  // t+1 and t+2 are outstanding.  All fetches are unconditional (clamped tile index) to keep
  // hipcc's vmcnt waits counted.
  if (TWO) {
    if (ntile > 0) {
      float4 ra[RPW], rb[RPW];
      int pa, pb;
      fetch(0, ra, pa);
      fetch(1, rb, pb);
      for (int t = 0; t < ntile; t += 2) {
        lds_barrier();  // every wave is done reading the previous tile
        stash(ra, pa);
        lds_barrier();
        fetch(t + 2, ra, pa);
        multiply();
        lds_barrier();
        stash(rb, pb);
        lds_barrier();
        fetch(t + 3, rb, pb);
        if (t + 1 < ntile) multiply();  // wave-uniform; LDS reads and MFMAs only
      }
    }
  } else if (ntile > 0) {
    float4 ra[RPW];
    int pa;
    fetch(0, ra, pa);
    for (int t = 0; t < ntile; ++t) {
      lds_barrier();
      stash(ra, pa);
      lds_barrier();
      fetch(t + 1, ra, pa);  // clamped to the run: the last trip re-reads its own tile
      multiply();
    }
  }

  // sum the 8 waves' accumulators in a fixed order, kRedTiles 16x16 tiles at a time (what the tile buffer holds:
  // 8 waves x 1 KiB per tile): element e = (tile * 4 + reg) * 64 + lane
  constexpr int kTiles = MA * NB;
  constexpr int kBufTiles = (((MA + NB) * 16 + 2) * kRowF4 * 16) / (kCpWaves * 1024);  // tiles the staging buffer holds
  constexpr int kRedTiles = kBufTiles >= kTiles ? kTiles : kBufTiles;
  static_assert(kRedTiles >= 1, "tile buffer too small for the reduction");
  float* red = reinterpret_cast<float*>(lds4) + (size_t)wave * (kRedTiles * 256);
  const float* all = reinterpret_cast<const float*>(lds4);
  float* out = part + ((size_t)r * nblk + bx) * ((size_t)Ca * Cb);
#pragma unroll
  for (int t0r = 0; t0r < kTiles; t0r += kRedTiles) {
    __syncthreads();  // the tile buffer (or the previous pass) is no longer read
#pragma unroll
    for (int ma = 0; ma < MA; ++ma)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int tile = ma * NB + nb;
        if (tile >= t0r && tile < t0r + kRedTiles) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) red[((tile - t0r) * 4 + reg) * 64 + lane] = acc[ma][nb][reg];
        }
      }
    __syncthreads();
    const int ntl = (kTiles - t0r < kRedTiles) ? kTiles - t0r : kRedTiles;
    for (int e = threadIdx.x; e < ntl * 256; e += kCpBlock) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < kCpWaves; ++w) v += all[w * (kRedTiles * 256) + e];
      const int el = e & 63, reg = (e >> 6) & 3, tile = t0r + (e >> 8);
      const int ma = tile / NB, nb = tile - ma * NB;
      const int a = a0 + ma * 16 + 4 * (el >> 4) + reg;  // D row = 4*(lane >> 4) + reg
      const int c = c0 + nb * 16 + (el & 15);            // D column = lane & 15
      if (a < a0 + ca && c < c0 + cb) out[(size_t)a * Cb + c] = v;   // this z-block's rows and columns only
    }
  }
}

// ---- the same contraction with LDS-DMA staging ---------------------------------------------------------------------
// k_chanpair_mfma keeps a tile in flight in REGISTERS, and its wide channel blocks have registers for one tile only:
// the next fetch cannot be issued before the previous tile has been written to LDS, so each tile pays its whole load
// time (5-7 us under load) plus the write pass in series with nothing -- 269 us for the [98 x 73] contraction whose
// load side alone takes 160 us and whose multiply side alone 180 us (profiles/r03/contraction_lab.txt).  Here the
// tiles go from global memory straight into LDS (global_load_lds_dwordx4: no destination registers) into a ring of
// NBUF buffers of TILE positions: while tile t is multiplied, tiles t+1 .. t+NBUF-2 are landing, and the accumulators
// are all the registers the kernel needs -- a [112 x 80] channel block fits, so the 98-channel gradient is ONE pass.
//   - one wave-instruction moves 1 KiB = the 4*TILE-byte pieces of 1024 / (4 TILE) consecutive rows (a "row group").
//     The LDS image of an instruction is lane-linear (base in M0 + 16 B x lane), so the group's pieces are adjacent;
//     a 16-B pad follows each group.  Rows of a group would hit the same banks: the float4 slots of row r are
//     XOR-swizzled on the SOURCE side (lane l of the piece fetches float4 l ^ swz(r)), and the fragment reads apply
//     the same XOR -- conflict-free;
//   - order (NBUF >= 3: the buffer of tile t-1 is free while tile t is multiplied): counted s_waitcnt vmcnt (own pieces
//     of tile t landed, later tiles may still fly), barrier (everyone's pieces landed, everyone is done with tile t-1),
//     re-issue into tile t-1's buffer, multiply.  Raw s_barrier with lgkmcnt(0) only: __syncthreads() would drain vmcnt;
//   - positions past the end of a row cannot be zeroed on the way (no registers): their lanes re-read in-row data and
//     the A fragment of those k-steps is zeroed instead (partial tiles only: the last tile of a group);
//   - row groups past the block's last row are not staged: their instructions (kept, so that every wave's vmcnt
//     arithmetic is the same) fetch one 16-B word into a dump group.
constexpr int kGGroupF4 = 64 + 1;  // float4s per row group: 1 KiB + 16 B

// MIX: the pass also writes mix[g,c,p] = sum_a Mx[r,a,c] A[g,a,p] -- with A = [du | dq] and Mx = [W | alpha] that is
// dx = W^T du + alpha (x) dq of the PROJ_FIRST backward (msgat.py:27's autograd), computed from the A tile the
// contraction has in LDS anyway: du and dq are read once for dW, dalpha AND dx.  Wave w owns positions 16 w .. 16 w + 15
// of a tile for all channels: D[i = position][j = channel] = sum_a A[a][position] Mx[a][channel], Mx fragments held in
// registers for the whole run (positions as D's rows: a lane ends up with four consecutive positions of a channel, one
// 16-B store; with channels as rows it was four 4-B stores: the [98 x 73] pass 456 instead of 415 us in the step).  The stores count on vmcnt like the LDS-DMA loads (in issue order), so EVERY lane
// stores every time -- lanes without a valid (channel, position) into `dump` -- and the waits are counted over both.
struct ChanMix {
  const float* Mw = nullptr;     // [R, Ca - 1, Cb]
  const float* Mlast = nullptr;  // [R, Cb]: row Ca - 1 of the matrix
  float* out = nullptr;          // [G, Cb, P]
  float* dump = nullptr;         // >= 256 floats (16-B aligned) nobody reads
};

// With several z-blocks over B (nzb > 1; the mix forms never cut A: all its rows must be in LDS) each block writes the
// mix output of ITS columns c0 .. c0 + cb.
// MODE 0: the contraction.  MODE 1 (MIX): every wave also computes the mix output of its 16 positions.  MODE 2 (SPLIT, for
// the wide channel blocks whose accumulators leave no registers for the matrix fragments): waves 0-3 contract (16
// positions of a 64-position tile each), waves 4-7 compute the mix output from the same LDS tiles -- two roles with
// equal MFMA counts, one wave of each per SIMD; all eight stage.
template <int MA, int NB, int TILE, int NBUF, int MODE = 0>
__global__ __launch_bounds__(kCpBlock) void k_chanpair_glds(
    SegList A, const float* __restrict__ B, float* __restrict__ part, int Cb, int P, int Bg, int nzb, int b_ones,
    int nza, int nblk, int R, ChanMix mix) {
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  typedef const __attribute__((address_space(1))) void* glb_ptr_t;
  static_assert(TILE == 64 || TILE == 128, "row pieces of 256 or 512 bytes");
  static_assert(NBUF >= 3, "the re-issue into tile t-1's buffer shares tile t's barrier: that buffer must not be tile t+1's");
  constexpr bool MIX = MODE != 0, SPLIT = MODE == 2;
  constexpr int kRPI = 256 / TILE;                 // rows per wave-instruction (row group)
  constexpr int kLPR = TILE / 4;                   // lanes (float4s) per row piece
  constexpr int kCWaves = SPLIT ? kCpWaves / 2 : kCpWaves;   // waves that contract
  constexpr int kPPW = TILE / kCWaves;             // positions per (contracting) wave and tile
  constexpr int kMaxGroups = (MA + NB) * 16 / kRPI;
  constexpr int RPW = (kMaxGroups + kCpWaves - 1) / kCpWaves;  // LDS-DMA instructions per wave and tile
  const int Cbr = Cb - b_ones;
  const int Ca = A.total();
  extern __shared__ float4 lds4[];
  int bx, r, zb;
  if (!cp_block(nza * nzb, nblk, R, bx, r, zb)) return;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int j = lane & 15, kq = lane >> 4;
  const int a_per = cdiv(Ca, nza);
  const int c_per = cdiv(Cb, nzb);      // EVEN split over B (<= 16 NB: the host picked nzb = ceil(Cb / 16 NB)): every z-block stages all of A, so they should do equal work
  const int a0 = (zb / nzb) * a_per;
  const int c0 = (zb % nzb) * c_per;
  const int ca = min(a_per, Ca - a0), cb = min(c_per, Cb - c0);
  const int rows = ca + cb;
  // buffer = the groups of the block's largest z-block (the host sized LDS for that), a constant group (zero row,
  // ones row), a dump group
  const int ngroups = cdiv(min(a_per, Ca) + min(c_per, Cb), kRPI);
  const int bufF4 = (ngroups + 2) * kGGroupF4;
  const int zero_row = ngroups * kRPI, ones_row = zero_row + 1;
  const CpRun run = cp_tile_run(P, TILE, Bg, bx, nblk);
  const int tpg = run.tpg, t0 = run.t0, ntile = run.ntile;
  float* out = part + ((size_t)r * nblk + bx) * ((size_t)Ca * Cb);
  if (ntile <= 0) {  // (never with the launcher's block counts) this block's partial is zero
    for (int e = threadIdx.x; e < ca * cb; e += kCpBlock) out[(size_t)(a0 + e / cb) * Cb + c0 + e % cb] = 0.f;
    return;
  }

  if (threadIdx.x < 2 * kLPR) {  // the constant rows, in every buffer
    const float4 v = (int)threadIdx.x < kLPR ? f4zero() : make_float4(1.f, 1.f, 1.f, 1.f);
#pragma unroll
    for (int b = 0; b < NBUF; ++b) lds4[b * bufF4 + ngroups * kGGroupF4 + threadIdx.x] = v;
  }

  // staging plan: instruction k of this wave fills group wave + 8k; lane l fetches float4 ((l % kLPR) ^ swz(row)) of
  // row group * kRPI + l / kLPR
  auto swz = [](int row) { return (row % kRPI) * (16 / kRPI); };   // in float4 slots: row i of a group sits 64 i / kRPI banks further
  const int lrow = lane / kLPR, lcol = lane % kLPR;
  const float* src[RPW];
  int gstride[RPW], lcs[RPW], grp[RPW];
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    const int g = wave + kCpWaves * k;
    const int rr = g * kRPI + lrow;
    const bool live = rr < rows;
    const int row = live ? rr : 0;
    const size_t g0 = (size_t)r * Bg;
    const float* p;
    if (row < ca) {
      const int a = a0 + row;
      int sk = 0;
#pragma unroll
      for (int i = 1; i < kMaxSeg; ++i) sk += (i < A.n && a >= A.begin[i]) ? 1 : 0;
      p = A.row((int)g0, a, P);
      int gs = A.gstride[0];
#pragma unroll
      for (int i = 1; i < kMaxSeg; ++i) gs = (i == sk) ? A.gstride[i] : gs;
      gstride[k] = gs * P;
    } else {
      p = B + (g0 * Cbr + min(c0 + row - ca, Cbr - 1)) * P;
      gstride[k] = Cbr * P;
    }
    src[k] = p;
    lcs[k] = live ? 4 * (lcol ^ swz(rr)) : -1;              // float offset inside the piece; -1: fetch one word only
    grp[k] = g * kRPI < rows ? g : ngroups + 1;             // wave-uniform: groups without a live row go to the dump
  }
  auto issue = [&](int t) {  // t relative to t0, clamped to the run; buffer t % NBUF
    const int tau = t0 + min(t, ntile - 1);
    const int b = tau / tpg;
    const int p0 = (tau - b * tpg) * TILE;
    float4* buf = lds4 + (t % NBUF) * bufF4;
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
      const int poff = lcs[k] < 0 ? 0 : min(p0 + lcs[k], P - 4);   // inside the row (P % 4 == 0); masked in multiply()
      const float* gp = src[k] + (size_t)b * gstride[k] + poff;
      __builtin_amdgcn_global_load_lds((glb_ptr_t)gp, (lds_ptr_t)(buf + grp[k] * kGGroupF4), 16, 0, 0);
    }
  };

  // fragment words: row `row`, positions kPPW * wave + 4 qq + kq -> float4 slot ((kPPW / 4) * wave ^ swz) + qq
  const float* ldsw = reinterpret_cast<const float*>(lds4);
  const int rwave = SPLIT ? (wave & (kCWaves - 1)) : wave;   // index within the wave's role: its slice of the tile
  auto frag_word = [&](int row) {
    return (row / kRPI) * (kGGroupF4 * 4) + (row % kRPI) * TILE + 4 * (((kPPW / 4) * rwave) ^ swz(row)) + kq;
  };
  int aw[MA], bw[NB];
#pragma unroll
  for (int ma = 0; ma < MA; ++ma) aw[ma] = frag_word((ma * 16 + j < ca) ? ma * 16 + j : zero_row);
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int cl = nb * 16 + j;
    bw[nb] = frag_word((cl < cb) ? ((b_ones && c0 + cl == Cbr) ? ones_row : ca + cl) : zero_row);
  }

  // The two roles of SPLIT are the two arms of ONE if: the accumulators exist only in the first, the matrix fragments
  // only in the second -- as two independent conditions hipcc kept both sets alive everywhere (256 VGPRs + 142 spilled).
  f32x4 acc[MA][NB];
  const bool contracts = !SPLIT || wave < kCWaves;   // wave-uniform
  auto zero_acc = [&]() {
#pragma unroll
    for (int ma = 0; ma < MA; ++ma)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[ma][nb] = f32x4_zero();
  };

  // MIX: matrix fragments A2[i = channel 16 nb + j][k = a = 4 s + kq], and the words of the B2 operand
  // B2[k = a][j = position kPPW w + j] in the A rows of the tile
  constexpr int KS = MIX ? MA * 4 : 1;
  constexpr int kStores = MIX ? NB : 0;       // per lane and tile
  static_assert(!MIX || kPPW == 16, "one 16-position tile per wave");
  float mfrag[KS][NB];
  // B2 word of k-step s: row 4 s + kq of the tile = group (4 s + kq) / kRPI -- linear in s, so one register and an
  // immediate offset per read.  Rows a >= Ca of the last k-steps hold other operands' data (B = x): those lanes read the
  // tile's zero row instead, so a non-finite x cannot reach the mix output as 0 * Inf (the two-pass fallback never reads
  // x for it either).  The launchers only pick a block shape for Ca > kCaMin, so the earlier k-steps need no select.
  constexpr int kMStep = (4 / kRPI) * (kGGroupF4 * 4);
  constexpr int kCaMin = MA <= 2 ? (MA - 1) * 16 : (MA - 2) * 16;
  const int zword = ngroups * (kGGroupF4 * 4) + j;
  const int mbase = (kq / kRPI) * (kGGroupF4 * 4) + (kq % kRPI) * TILE + 4 * (((kPPW / 4) * rwave + (j >> 2)) ^ swz(kq)) + (j & 3);
  auto load_mfrag = [&]() {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int a = 4 * s + kq;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int c = c0 + nb * 16 + j;     // this z-block's columns of the matrix
        const int cc = min(c, Cbr - 1);
        float v;
        if (mix.Mlast != nullptr) {   // kernel-uniform: the matrix's last row lives in another array
          const float wv = mix.Mw[((size_t)r * (Ca - 1) + max(min(a, Ca - 2), 0)) * Cbr + cc];
          const float lv = mix.Mlast[(size_t)r * Cbr + cc];
          v = a == Ca - 1 ? lv : wv;
        } else {
          v = mix.Mw[((size_t)r * Ca + min(a, Ca - 1)) * Cbr + cc];
        }
        mfrag[s][nb] = (nb * 16 + j < cb && c < Cbr && a < Ca) ? v : 0.f;
      }
    }
  };
  auto mix_tile = [&](int t) {
    const int tau = t0 + t;
    const int b = tau / tpg;
    const int p0 = (tau - b * tpg) * TILE;
    const float* w = ldsw + (t % NBUF) * (bufF4 * 4);
    f32x4 d[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) d[nb] = f32x4_zero();
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      int word = mbase + s * kMStep;
      if (4 * s + 3 >= kCaMin) word = (4 * s + kq < Ca) ? word : zword;
      const float bv = w[word];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) d[nb] = mfma_16x16x4(bv, mfrag[s][nb], d[nb]);
    }
    // D[i = position 4 kq + reg][j = channel]: a lane holds four consecutive positions of one channel -- one 16-B store
    const int pos = p0 + kPPW * rwave + 4 * kq;
    float* og = mix.out + ((size_t)r * Bg + b) * Cbr * P + pos;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int c = c0 + nb * 16 + j;
      float* dst = (nb * 16 + j < cb && c < Cbr && pos < P) ? og + (size_t)c * P : mix.dump + 4 * lane;   // a select on the address: no branch
      *reinterpret_cast<f32x4*>(dst) = d[nb];
    }
  };

  auto multiply = [&](int t) {
    const int tau = t0 + t;
    const int p0 = (tau - (tau / tpg) * tpg) * TILE;
    const bool partial = p0 + TILE > P;   // wave-uniform: the last tile of a group
    const float* w = ldsw + (t % NBUF) * (bufF4 * 4);
#pragma unroll
    for (int qq = 0; qq < kPPW / 4; ++qq) {
      float av[MA], bv[NB];
#pragma unroll
      for (int ma = 0; ma < MA; ++ma) av[ma] = w[aw[ma] + 4 * qq];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) bv[nb] = w[bw[nb] + 4 * qq];
      if (partial) {   // tail positions are zeroed HERE, at the A fragment: LDS-DMA passes through no register on the way in
        const float keep = (p0 + kPPW * rwave + 4 * qq + kq < P) ? 1.f : 0.f;
#pragma unroll
        for (int ma = 0; ma < MA; ++ma) av[ma] *= keep;
      }
#pragma unroll
      for (int ma = 0; ma < MA; ++ma)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[ma][nb] = mfma_16x16x4(av[ma], bv[nb], acc[ma][nb]);
    }
  };

#pragma unroll
  for (int t = 0; t < NBUF - 1; ++t) issue(t);
  static_assert(!MIX || NBUF == 3, "the counted waits of the MIX forms are written for three buffers");
  constexpr int kSteady = (NBUF - 2) * RPW + (NBUF - 1) * kStores;   // younger than tile t's loads: see below
  static_assert(kSteady < 64, "vmcnt is a 6-bit counter");
  // Per trip: this wave's pieces of tile t are in LDS (later tiles and -- waves that mix -- the stores of the last
  // NBUF - 1 trips, issued after tile t's loads, may be in flight; the first trips have fewer operations behind
  // them); barrier: ... and every other wave's, and nobody reads tile t-1's buffer any more; re-issue into that
  // buffer (clamped index: the last trips re-read the last tile); the wave's role(s).  Both roles pass the same
  // barriers.
  if (contracts) {
    zero_acc();
    if (MODE == 1) load_mfrag();
    for (int t = 0; t < ntile; ++t) {
      if (MODE == 1 && t == 0) wait_vmcnt<RPW>();
      else if (MODE == 1 && t == 1) wait_vmcnt<RPW + kStores>();
      else wait_vmcnt<MODE == 1 ? kSteady : (NBUF - 2) * RPW>();
      lds_barrier();
      issue(t + NBUF - 1);
      multiply(t);
      if (MODE == 1) mix_tile(t);
    }
  } else {   // SPLIT, waves that mix
    load_mfrag();
    for (int t = 0; t < ntile; ++t) {
      if (t == 0) wait_vmcnt<RPW>();
      else if (t == 1) wait_vmcnt<RPW + kStores>();
      else wait_vmcnt<kSteady>();
      lds_barrier();
      issue(t + NBUF - 1);
      mix_tile(t);
    }
  }
  wait_vmcnt<0>();

  // sum the 8 waves' accumulators in a fixed order, kRedTiles 16x16 tiles at a time (the launcher checks that
  // kRedTiles * 8 KiB fit the staging buffers)
  constexpr int kTiles = MA * NB;
  constexpr int kRedTiles = kTiles < 8 ? kTiles : 8;
  float* red = reinterpret_cast<float*>(lds4) + (size_t)wave * (kRedTiles * 256);
  const float* all = reinterpret_cast<const float*>(lds4);
#pragma unroll
  for (int t0r = 0; t0r < kTiles; t0r += kRedTiles) {
    __syncthreads();
    if (contracts) {
#pragma unroll
      for (int ma = 0; ma < MA; ++ma)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          const int tile = ma * NB + nb;
          if (tile >= t0r && tile < t0r + kRedTiles) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) red[((tile - t0r) * 4 + reg) * 64 + lane] = acc[ma][nb][reg];
          }
        }
    }
    __syncthreads();
    const int ntl = (kTiles - t0r < kRedTiles) ? kTiles - t0r : kRedTiles;
    for (int e = threadIdx.x; e < ntl * 256; e += kCpBlock) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < kCWaves; ++w) v += all[w * (kRedTiles * 256) + e];
      const int el = e & 63, reg = (e >> 6) & 3, tile = t0r + (e >> 8);
      const int ma = tile / NB, nb = tile - ma * NB;
      const int a = a0 + ma * 16 + 4 * (el >> 4) + reg;
      const int c = c0 + nb * 16 + (el & 15);
      if (a < a0 + ca && c < c0 + cb) out[(size_t)a * Cb + c] = v;
    }
  }
}

// Blocks per relation.  The kernels are built for ONE resident block per CU, so the grid runs in rounds of `ncu` blocks and
// what counts is how full the last round is.  Few relations: ncu / R blocks each fill one round (R = 3: 255 of 256 CUs).
// Many relations -- a per-sample matrix makes every group its own relation: R = 96 at PEMSD7 size, 160 with five components
// -- leave ncu / R = 2 or 1 blocks each, i.e. 192 or 160 busy CUs of 256 (the merged convolution backward ran 415 us at
// R = 96 where the same bytes take 345 us at R = 3, and 796 us at R = 160): there, the smallest count up to 16 whose rounds
// are at least 95 % full (8 at R = 96 and R = 160: three and five full rounds), else the fullest: 415 -> 363 us, 796 -> 613.
int chanpair_mfma_blocks(int R) {
  const int ncu = device_cu_count();
  const int kmin = max(1, ncu / R);
  if (kmin >= 16) return kmin;
  int best = kmin;
  double best_fill = 0.0;
  for (int k = kmin; k <= 16; ++k) {
    const long long blocks = (long long)R * k;
    const double fill = (double)blocks / (double)(((blocks + ncu - 1) / ncu) * ncu);
    if (fill >= 0.95) return k;
    if (fill > best_fill + 1e-9) { best_fill = fill; best = k; }
  }
  return best;
}

// ---- host side -------------------------------------------------------------------------------------------------------
// What a contraction launch is given: A's rows (segments), B [G, Cb - b_ones, P], the partials (room for nblk_max per
// relation; *nblk_used: how many the launch wrote -- fewer when the channel matrix is cut into z-blocks) and the stream
struct CpArgs {
  const SegList& A;
  const float* B;
  float* part;
  int R, Bg, Cb, P, nblk_max, b_ones;
  hipStream_t s;
  int* nblk_used;
};

// msgat_contract_form_name(): the launchers below run as usual up to the point where they would touch the device, and
// the leaf that would launch writes its kernel's name here instead.  Thread-private, set only by that query.
struct FormProbe {
  char name[96];
  int nza, nzb;
};
static thread_local FormProbe* g_form_probe = nullptr;

// What both leaf launchers settle before they launch a [16 MA x 16 NB] block on a [Ca x Cb] channel matrix: the cut
// into nza x nzb z-blocks, the blocks (runs) per relation, and the grid the kernels' cp_block() decodes.
struct CpLeaf {
  int nza, nzb, nblk;
  dim3 grid;
};
static CpLeaf cp_leaf(const CpArgs& a, int Ca, int MA, int NB, int per_cu = 1) {
  CpLeaf l;
  l.nza = cdiv(Ca, MA * 16);
  l.nzb = cdiv(a.Cb, NB * 16);
  const int nz = l.nza * l.nzb;
  // several z-blocks: all of them resident at once (per_cu = 1 block per CU; more in lab builds only), so fewer, longer
  // runs per relation
  l.nblk = nz > 1 ? min(a.nblk_max, max(1, per_cu * a.nblk_max / nz)) : a.nblk_max;
  *a.nblk_used = l.nblk;
  l.grid = nz > 1 ? dim3(xcd_grid(l.nblk * a.R, nz)) : dim3(l.nblk, a.R, 1);
  return l;
}
// true: the form query is running -- the kernel's name and z-block cut are written and nothing must be launched
__attribute__((format(printf, 2, 3))) static bool cp_probed(const CpLeaf& l, const char* fmt, ...) {
  if (!g_form_probe) return false;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_form_probe->name, sizeof g_form_probe->name, fmt, ap);
  va_end(ap);
  g_form_probe->nza = l.nza;
  g_form_probe->nzb = l.nzb;
  return true;
}

template <int MA, int NB, bool TWO = true, int TILE = kTile>
static int launch_chanpair_t(const CpArgs& a, TimeShift ts) {
  const CpLeaf l = cp_leaf(a, ts.d ? 2 * a.A.total() : a.A.total(), MA, NB);
  // tile rows + the zero row + the ones row; the reduction re-uses the buffer a few tiles at a time
  const size_t lds = sizeof(float4) * (size_t)(((MA + NB) * 16 + 2) * (TILE / 4 + 1));
  if (cp_probed(l, "k_chanpair_mfma<%d,%d,%s,%d%s>", MA, NB, TWO ? "true" : "false", TILE, ts.d ? ",shift" : "")) return MSGAT_OK;
  auto launch = [&](auto shift) -> int {
    constexpr bool SHIFT = decltype(shift)::value;
    return launch_lds<k_chanpair_mfma<MA, NB, TWO, TILE, SHIFT>>(l.grid, dim3(kCpBlock), lds, a.s, a.A, a.B, a.part, a.Cb, a.P,
                                                                 a.Bg, l.nzb, a.b_ones, l.nza, l.nblk, a.R, ts);
  };
  return ts.d ? launch(std::true_type{}) : launch(std::false_type{});
}

// LDS bytes of the LDS-DMA form for a channel matrix cut into nza x nzb z-blocks
template <int MA, int NB, int TILE, int NBUF>
static size_t chanpair_glds_lds(int Ca, int Cb) {
  const int nza = cdiv(Ca, MA * 16), nzb = cdiv(Cb, NB * 16);
  const int rows = min(cdiv(Ca, nza), Ca) + min(cdiv(Cb, nzb), Cb);
  return sizeof(float4) * (size_t)NBUF * (cdiv(rows, 256 / TILE) + 2) * kGGroupF4;
}

template <int MA, int NB, int TILE, int NBUF, int MODE = 0>
static int launch_chanpair_glds_t(const CpArgs& a, ChanMix mix = ChanMix()) {
  const int Ca = a.A.total();
  int per_cu = 1;
#ifdef MSGAT_LAB
  per_cu = lab_env("MSGAT_LAB_BPC", 1);   // resident blocks per CU
#endif
  const CpLeaf l = cp_leaf(a, Ca, MA, NB, per_cu);
  const size_t lds = chanpair_glds_lds<MA, NB, TILE, NBUF>(Ca, a.Cb);
  if (lds > (size_t)kLdsMax || lds < (size_t)(MA * NB < 8 ? MA * NB : 8) * kCpWaves * 1024) return MSGAT_ERR_UNSUPPORTED;
  if (cp_probed(l, "k_chanpair_glds<%d,%d,%d,%d,%d>", MA, NB, TILE, NBUF, MODE)) return MSGAT_OK;
  return launch_lds<k_chanpair_glds<MA, NB, TILE, NBUF, MODE>>(l.grid, dim3(kCpBlock), lds, a.s, a.A, a.B, a.part, a.Cb, a.P,
                                                               a.Bg, l.nzb, a.b_ones, l.nza, l.nblk, a.R, mix);
}

// ---- which LDS-DMA form for which channel block -----------------------------------------------------------------
// X(MA, NB, TILE, MIXMODE): a [16 MA x 16 NB] channel block staged in three buffers of TILE positions; MIXMODE says how
// the one-pass form (contraction AND mix output) runs: 1 = every wave does both (128-position tiles), 2 = waves 0-3
// contract and waves 4-7 mix (64-position tiles: what three buffers of that many rows leave room for), 0 = there is
// none.  The list covers the channel counts of the three models of the reference's registry (main.py:17,
// msgat.py:220-229: 48 / 72 / 96 hidden channels, 16 / 24 / 32 per branch):
//                       GACN projection backward     merged channel mixing          residual convolution
//                       [Co + 1 x C]                 [4 Co + 2 x C + 1]             [C x C + 1]
//   msgat48             17 x 48   <2,3,128> mix 1    66 x 49   <5,4,64> mix 2       48 x 49   <3,4,128> mix 1
//   msgat72             25 x 72   <2,3,128> mix 1    98 x 73   <7,5,64> mix 2       72 x 73   <5,5,64>  mix 2
//                       two z-blocks over B, 36 columns each (launch_glds_mix; the plain contraction: <2,5,128>)
//   msgat96             33 x 96   <3,6,64>  mix 2    130 x 97  <9,4,64> mix 2       96 x 97   <6,4,64>  mix 2
//                                                    two z-blocks over B, 49 + 48 columns each with ALL rows of A
//                                                    (a [96 x 112] accumulator block spills; A is read twice, B once)
#define MSGAT_GLDS_FORMS(X) \
  X(2, 3, 128, 1) X(2, 4, 128, 1) X(2, 5, 128, 1) X(3, 4, 128, 1) X(3, 6, 64, 2) X(5, 4, 64, 2) X(5, 5, 64, 2) \
  X(7, 5, 64, 2) X(6, 4, 64, 2) X(9, 4, 64, 2) MSGAT_GLDS_LAB_FORMS(X)
// lab builds (-DMSGAT_LAB): narrow blocks over B -- several z-blocks per run that each stage all of A (re-read from the
// XCD's L2) and write FEW mix channels over the run's whole position range
#ifdef MSGAT_LAB
#define MSGAT_GLDS_LAB_FORMS(X) \
  X(2, 1, 128, 1) X(2, 2, 128, 1) X(7, 1, 64, 2) X(7, 2, 64, 2) X(7, 3, 64, 2) X(5, 1, 64, 2) X(5, 2, 64, 2) X(5, 3, 64, 2) \
  X(6, 5, 64, 2)   /* 96 x 73: what the merged gradient would cost without its two single-channel rows */
#else
#define MSGAT_GLDS_LAB_FORMS(X)
#endif

// Launches the form [MA x NB] if the list has it (and its buffers fit LDS); *handled = 0 and nothing launched otherwise.
static int launch_glds_form(int MA, int NB, bool with_mix, const CpArgs& a, const ChanMix& mix, int* handled) {
  const int Ca = a.A.total();
  *handled = 0;
#define MSGAT_GLDS_TRY(ma, nb, tile, mode)                                                                            \
  if (MA == ma && NB == nb) {                                                                                         \
    if ((with_mix && mode == 0) || chanpair_glds_lds<ma, nb, tile, 3>(Ca, a.Cb) > (size_t)kLdsMax) return MSGAT_OK;    \
    *handled = 1;                                                                                                     \
    if (with_mix) return launch_chanpair_glds_t<ma, nb, tile, 3, mode>(a, mix);                                       \
    return launch_chanpair_glds_t<ma, nb, tile, 3, 0>(a);                                                             \
  }
  MSGAT_GLDS_FORMS(MSGAT_GLDS_TRY)
#undef MSGAT_GLDS_TRY
  return MSGAT_OK;
}

static bool glds_form_exists(int MA, int NB, bool with_mix) {
#define MSGAT_GLDS_HAS(ma, nb, tile, mode) \
  if (MA == ma && NB == nb) return !with_mix || mode != 0;
  MSGAT_GLDS_FORMS(MSGAT_GLDS_HAS)
#undef MSGAT_GLDS_HAS
  return false;
}

// rows of >= 512 positions in whole float4s: every group spans several tiles (shorter rows: the register-staged kernel)
static bool glds_rows_ok(int P) { return P % 4 == 0 && P >= 512; }

// The contraction AND mixout = M^T A in one pass (k_chanpair_glds, MODE 1 / 2): part[a, c] (c < Cb; with b_ones a virtual
// last channel of ones in B) and mixout[g, c, p] = sum_a M[r, a, c] A[g, a, p] over B's Cb - b_ones real channels, with
// M = [R, Ca, Cb - b_ones] -- or, Mlast given, [Mw | Mlast] with Mw = [R, Ca - 1, .] and Mlast = [R, .] its last row
// ([W | alpha] of the GACN projection).  All Ca rows must be in LDS at once (one z-block); a block one tile taller than
// the operand is fine (the kernels mask rows >= Ca and read the zero row for them).  *done = 0 (nothing launched) when
// no form covers the shape: the caller runs the two passes.
static int launch_glds_mix(const CpArgs& a, const float* Mw, const float* Mlast, float* mixout, int* done) {
  const int Ca = a.A.total(), Cb = a.Cb;
  *done = 0;
  if (!glds_rows_ok(a.P) || Ca <= 16) return MSGAT_OK;
  ChanMix mix;
  mix.Mw = Mw; mix.Mlast = Mlast; mix.out = mixout;
  mix.dump = a.part + (((size_t)a.R * a.nblk_max * Ca * Cb + 3) & ~(size_t)3);   // chanpair_partial_floats() leaves 260 floats behind the partials
  // z-blocks over B, each staging all of A, in the order they are tried: one block where a form covers it, else two.
  // The [25 x 72] block (the GACN projection backward of msgat72: 24 rows of du and dq against 72 channels) takes two
  // z-blocks of 36 columns first, k_chanpair_glds<2,3,128,3,1> instead of <2,5,128,3,1>: parent against tree on one box
  // the pass runs 180 -> 164-170 us in the hot-path step, k_aggfirst_bwd behind it 35 -> 32, the step 0.6794 -> 0.6524 ms,
  // HBM-side traffic 749 -> 698 MB although both z-blocks stage A (profiles/project_wide_tiles/).  The rule is one of the two channel counts alone -- never of the batch, the row
  // length or the device -- and covers nothing but that measured block; the wider blocks lose as z-blocks (round 5).
  int order[2] = {1, 2}, n_order = 2;
  if (Ca == 25 && Cb == 72) { order[0] = 2; order[1] = 1; }
#ifdef MSGAT_LAB
  if (lab_env("MSGAT_LAB_NZB", 0) > 0) { order[0] = lab_env("MSGAT_LAB_NZB", 0); n_order = 1; }   // overrides the rule above
#endif
  for (int t = 0; t < n_order; ++t) {
    const int nzb = order[t];
    // the narrowest block that covers the z-block's columns, or one tile wider (columns past the operand read the zero
    // row): the list is written for the widths WITH a bias column (49 / 73 / 97), and the same mixing without one
    // (48 / 72 / 96 columns: the merged channel mixing of the stacked schedule) must not fall back to two passes
    for (int NB = cdiv(cdiv(Cb, nzb), 16); NB <= cdiv(cdiv(Cb, nzb), 16) + 1; ++NB) {
      if (cdiv(Cb, NB * 16) != nzb) continue;      // the kernel derives nzb from the block width
      for (int MA = cdiv(Ca, 16); MA <= cdiv(Ca, 16) + 1; ++MA) {
        if (!glds_form_exists(MA, NB, true)) continue;
        const int st = launch_glds_form(MA, NB, true, a, mix, done);
        if (st || *done) return st;
      }
    }
  }
  return MSGAT_OK;
}

int launch_chanpair_mix(const SegList& A, const float* B, float* part, int R, int Bg, int Cb, int P, int nblk,
                        const float* Mw, const float* Mlast, float* mixout, hipStream_t s, int* nblk_used, int* done) {
  return launch_glds_mix({A, B, part, R, Bg, Cb, P, nblk, 0, s, nblk_used}, Mw, Mlast, mixout, done);
}

int launch_chanpair_mix_wide(const SegList& A, const float* B, float* part, int R, int Bg, int Cb, int P, int nblk,
                             int b_ones, const float* M, float* mixout, hipStream_t s, int* nblk_used, int* done) {
  return launch_glds_mix({A, B, part, R, Bg, Cb, P, nblk, b_ones, s, nblk_used}, M, nullptr, mixout, done);
}

// Which kernel form a contraction takes: an LDS-DMA form where the list above has a block for the shape, else the
// register-staged kernel -- always that one with time-shifted virtual rows (ts.d > 0), which the LDS-DMA forms cannot do
static int launch_contract(const CpArgs& a, TimeShift ts) {
  const int Cb = a.Cb, P = a.P;
  const bool shift = ts.d != 0;
  const int Ca = shift ? 2 * a.A.total() : a.A.total();
#ifndef MSGAT_NO_GLDS
  // LDS-DMA staging where the list above has a block for the shape: the fewest z-blocks over A (each re-reads B) whose
  // row count some form of this width covers, the smallest such form
  if (!shift && glds_rows_ok(P) && Ca > 16) {
    // fewest rows staged in total: nzb z-blocks over B each stage A, nza z-blocks over A each stage B
    int best_ma = 0, best_nb = 0;
    long best_cost = -1;
    for (int nzb = 1; nzb <= 2; ++nzb)
      for (int nza = 1; nza <= 3; ++nza) {
        const int NBg = cdiv(cdiv(Cb, nzb), 16);
        if (cdiv(Cb, NBg * 16) != nzb) continue;
        for (int ma = max(cdiv(cdiv(Ca, nza), 16), 2); ma <= 9; ++ma) {
          if (!glds_form_exists(ma, NBg, false) || cdiv(Ca, ma * 16) != nza) continue;
          const long cost = (long)nzb * Ca + (long)nza * Cb;
          if (best_cost < 0 || cost < best_cost) { best_cost = cost; best_ma = ma; best_nb = NBg; }
          break;   // the smallest block of this width that covers the rows
        }
      }
    if (best_cost >= 0) {
      int handled = 0;
      const int st = launch_glds_form(best_ma, best_nb, false, a, ChanMix(), &handled);
      if (st || handled) return st;
    }
  }
#endif
  // the register-staged kernel.  Block shapes whose accumulators + two register sets in flight exceed the 256
  // registers of a 2-waves-per-SIMD block are not offered ([48 x 80], [48 x 96] and [32 x 96] spilled 18 / 93 / 14
  // registers): a wider B is cut into z-blocks, which re-read A
  const int MA = min(cdiv(Ca, 16), 3), NB = min(cdiv(Cb, 16), MA == 3 ? 4 : (MA == 2 ? 5 : 6));
  // 65..80 A channels against 17..80 B channels: half-length tiles hold all of A and B in LDS at once -- ONE pass over
  // both operands where the [48 x 96] blocks take two z-blocks that each re-read B (72 x 73, the residual tail's weight
  // gradient: 286 -> 174 us).  Not for wider A (a [112 x 80] block spills and ran at 372 us against 344 for the two
  // [64 x 80] blocks below) nor for a B of one tile (re-reading it is cheap: 64 -> 84 us).
  // (49..64 rows go to the [64 x 16 NB] block below instead: 256-position tiles, 1-KiB row pieces -- the shifted
  // [64 x 33] weight gradient of msgat96's convolutions 125 -> 110 us)
  if (NB >= 2 && NB <= 5 && Ca > 64 && Ca <= 80)
    return dispatch_range<2, 5>(NB, [&](auto nb) { return launch_chanpair_t<5, decltype(nb)::value, false, 128>(a, ts); });
  // 64 A channels per z-block where that saves a pass over B (and the [64 + 16 NB] rows fit LDS: NB <= 5)
  if (NB <= 5 && cdiv(Ca, 64) < cdiv(Ca, 48))
    return dispatch_range<1, 5>(NB, [&](auto nb) { return launch_chanpair_t<4, decltype(nb)::value, false>(a, ts); });
  return dispatch_range<1, 3>(MA, [&](auto ma) {
    return dispatch_range<1, 6>(NB, [&](auto nb) -> int {
      constexpr int kMA = decltype(ma)::value, kNB = decltype(nb)::value;
      if constexpr (kNB <= (kMA == 3 ? 4 : (kMA == 2 ? 5 : 6))) return launch_chanpair_t<kMA, kNB>(a, ts);   // the widths offered above
      else return MSGAT_ERR_UNSUPPORTED;
    });
  });
}

int launch_chanpair_mfma(const SegList& A, const float* B, float* part, int R, int Bg, int Cb, int P, int nblk,
                         int b_ones, hipStream_t s, int* nblk_used) {
  return launch_contract({A, B, part, R, Bg, Cb, P, nblk, b_ones, s, nblk_used}, TimeShift());
}

// A with time-shifted virtual rows (k_chanpair_mfma<.., SHIFT>): part is [2 Cr x Cb] for A's Cr real rows
int launch_chanpair_shifted(const SegList& A, const float* B, float* part, int R, int Bg, int Cb, int P, int nblk,
                            int b_ones, int dilation, int T, hipStream_t s, int* nblk_used) {
  if (dilation <= 0 || T % 4 != 0 || P % T != 0) return MSGAT_ERR_SHAPE;
  TimeShift ts;
  ts.d = dilation < T ? dilation : T;
  ts.T = T;
  return launch_contract({A, B, part, R, Bg, Cb, P, nblk, b_ones, s, nblk_used}, ts);
}

// Which kernel a [Ca x Cb] channel-pair contraction over rows of P positions takes (with_mix: the one-pass form that also
// writes the mix output; *one_pass = 0 there means "no fused form: the contraction below plus a projection pass").
// Runs the launchers' own selection code with the probe set: nothing is launched, no device is touched.
int contract_form_name(int Ca, int Cb, int b_ones, int P, int with_mix, char* buf, int buflen, int* one_pass, int* nza,
                       int* nzb) {
  FormProbe probe{};
  SegList A = seg_single(reinterpret_cast<const float*>(16), Ca);   // never dereferenced
  float* fake = reinterpret_cast<float*>(16);
  int nblk = 0, done = 0, st = MSGAT_OK;
  const CpArgs a{A, fake, fake, 1, 1, Cb, P, 256, b_ones, nullptr, &nblk};
  g_form_probe = &probe;
  if (with_mix) st = launch_glds_mix(a, fake, nullptr, fake, &done);
  if (!st && !done) st = launch_contract(a, TimeShift());
  g_form_probe = nullptr;
  if (st) return st;
  if (one_pass) *one_pass = done;
  if (nza) *nza = probe.nza;
  if (nzb) *nzb = probe.nzb;
  if (buf && buflen > 0) snprintf(buf, (size_t)buflen, "%s", probe.name);
  return MSGAT_OK;
}

}  // namespace msgat
