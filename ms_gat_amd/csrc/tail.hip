// The tail of a training step: loss + metric sums in one pass over the prediction, and
// Adam over flat state buffers in one launch.
//
//   reference            engine.py:56 HuberLoss (loss.py:51-52: mean of 0.5 e^2 inside delta, delta |e| - 0.5 delta^2
//                        beyond), engine.py:66-70 + metrics.py:20-35: per batch `loss.item()` and three more `.item()`
//                        sums (|e|, 100 |e / y| where y > mask, e^2) -- four host syncs and ~10 elementwise / reduce
//                        launches; engine.py:106 optim.Adam(lr 1e-3, weight_decay 5e-4).
//   here                 k_loss_metrics: every block folds its elements into four double partials (fixed order inside
//                        the block), k_loss_finish adds the partials in block order: deterministic, nothing read back.
//                        k_loss_grad: the loss gradient.  The first and the last take the loss as a policy (Huber,
//                        Gauss: below), as do their masked forms further down.
//                        k_adam: torch.optim.Adam's update (L2 decay folded into the
//                        gradient, bias correction, eps outside the square root) for every parameter tensor at once,
//                        driven by a chunk table; the step counter and the learning rate live in device memory so the
//                        launch is capturable in a HIP graph.
//   guard (optional)     k_grad_sumsq + k_guard_finish: the global norm of the flat gradient, its clipping coefficient
//                        (torch.nn.utils.clip_grad_norm_'s) and whether it is finite, left in device memory; the guarded
//                        forms of k_adam_advance / k_adam read them there and scale the gradient or -- like
//                        GradScaler.step (reference engine.py:61-63) -- leave a non-finite step out altogether.
//   average (optional)   k_adam<., Shadow>: k_adam that also moves a flat shadow of the parameters towards w_new (an
//                        exponential moving average, warmed up by the tensor's step count); k_param_swap exchanges
//                        parameters and shadow in place, so validation reads the average at the addresses it holds.
#include "common.hpp"
#include "tail_terms.hpp"

namespace msgat {

constexpr int kTailBlock = 256;
constexpr int kTailPerThread = 8;  // elements per lane per block trip

// ---- the loss of the step tail: a policy of the metrics and gradient kernels, plain and masked -------------------------
// value(a) is the loss of one entry at |e| = a, slope(e) its derivative at e; both are evaluated per entry in fp32 and the
// values are added into double partials.  A policy is a few floats that travel as one by-value kernel argument, like the
// lone `delta` before it.  The finish kernels only add partials: they know no loss.
//   Huber   loss.py:51-52   e^2 / 2 inside delta, delta |e| - delta^2 / 2 beyond; slope clamp(e, -delta, delta)
//   Gauss   loss.py:94-95   sigma^2 (1 - exp(-e^2 / 2 sigma^2)) + delta |e|; slope e exp(-e^2 / 2 sigma^2) + delta sgn(e)
//           with sgn(0) = 0 (torch's abs backward).  1 - exp(-t) is taken as -expm1f(-t): for |e| << sigma,
//           1.f - expf(-t) keeps only the few bits of t that survive next to 1 (|e| = 1e-3 sigma: 3.5e-3 relative error
//           of the loss at delta = 0, against 2e-8).  The accurate library functions, not __expf.  sigma^2 and
//           1 / (2 sigma^2) are rounded to fp32 once from the host's doubles.
struct Huber {
  float delta;
  __device__ __forceinline__ float value(float a) const {
    return (a <= delta) ? 0.5f * a * a : delta * a - 0.5f * delta * delta;
  }
  __device__ __forceinline__ float slope(float e) const { return fminf(fmaxf(e, -delta), delta); }
};

struct Gauss {
  float sigma2, inv_2sigma2, delta;
  __device__ __forceinline__ float value(float a) const {
    const float t = a * a * inv_2sigma2;
    return sigma2 * -expm1f(-t) + delta * a;
  }
  __device__ __forceinline__ float slope(float e) const {
    const float t = e * e * inv_2sigma2;
    return e * expf(-t) + (e == 0.f ? 0.f : copysignf(delta, e));   // e = 0: exactly 0
  }
};

static Gauss gauss_of(double sigma, double delta) {
  return Gauss{(float)(sigma * sigma), (float)(1.0 / (2.0 * sigma * sigma)), (float)delta};
}

template <class Loss>
__global__ __launch_bounds__(kTailBlock) void k_loss_metrics(const float* __restrict__ pred,
                                                             const float* __restrict__ truth, long long n,
                                                             Loss loss, float mask_value,
                                                             double* __restrict__ part) {
  __shared__ double red[4][kTailBlock / 64];
  double s[4] = {0.0, 0.0, 0.0, 0.0};  // loss, |e|, 100 |e / y| (y > mask), e^2
  const long long stride = (long long)gridDim.x * kTailBlock;
  for (long long i = (long long)blockIdx.x * kTailBlock + threadIdx.x; i < n; i += stride) {
    const float p = pred[i], y = truth[i];
    const float e = p - y, a = fabsf(e);
    s[0] += loss.value(a);
    s[1] += a;
    if (y > mask_value) s[2] += 100.0 * (double)fabsf(e / y);
    s[3] += (double)e * (double)e;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double w = wave_sum(s[k]);
    if (lane == 0) red[k][wave] = w;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kTailBlock / 64; ++w) t += red[threadIdx.x][w];
    part[(size_t)blockIdx.x * 4 + threadIdx.x] = t;
  }
}

// loss[0] = mean loss (fp32, what the reference's loss tensor holds); sums[0..2] += AE, APE, SE and
// sums[3] += loss_weight * that mean (the epoch's running total of batch losses; a rank that holds n_r of a global
// batch's n_b samples passes n_r / n_b, so the sum over ranks is the global batch's mean loss), all double
__global__ void k_loss_finish(const double* __restrict__ part, int nblocks, long long n, float* __restrict__ loss,
                              double* __restrict__ sums, float loss_weight) {
  // wave k adds sum k: lane l takes blocks l, l + 64, ... in order, then the lanes are combined by the fixed butterfly
  // of wave_sum (a serial loop over up to 1024 partials by one lane took 19 us)
  const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double t = 0.0;
  for (int b = lane; b < nblocks; b += 64) t += part[(size_t)b * 4 + k];
  t = wave_sum(t);
  if (lane != 0) return;
  if (k == 0) {
    loss[0] = (float)(t / (double)n);
    if (sums != nullptr) sums[3] += (t / (double)n) * (double)loss_weight;
  } else if (sums != nullptr) {
    sums[k - 1] += t;
  }
}

template <class Loss>
__global__ __launch_bounds__(kTailBlock) void k_loss_grad(const float* __restrict__ pred,
                                                          const float* __restrict__ truth,
                                                          const float* __restrict__ dloss, long long n, Loss loss,
                                                          float* __restrict__ dpred) {
  const long long i = (long long)blockIdx.x * kTailBlock + threadIdx.x;
  if (i >= n) return;
  const float e = pred[i] - truth[i];
  const float g = loss.slope(e);  // d/de of the entry's loss
  dpred[i] = g * (dloss[0] / (float)n);
}

static int loss_blocks(long long n) {
  const long long want = (n + (long long)kTailBlock * kTailPerThread - 1) / ((long long)kTailBlock * kTailPerThread);
  return (int)(want < 1 ? 1 : (want > 1024 ? 1024 : want));
}

size_t huber_partial_doubles(long long n) { return (size_t)loss_blocks(n) * 4; }

template <class Loss>
static int launch_loss_metrics(const float* pred, const float* truth, long long n, Loss lf, float mask_value,
                               double* part, float* loss, double* sums, float loss_weight, hipStream_t s) {
  const int nb = loss_blocks(n);
  hipLaunchKernelGGL(k_loss_metrics<Loss>, dim3(nb), dim3(kTailBlock), 0, s, pred, truth, n, lf, mask_value, part);
  MSGAT_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_loss_finish, dim3(1), dim3(256), 0, s, part, nb, n, loss, sums, loss_weight);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

template <class Loss>
static int launch_loss_grad(const float* pred, const float* truth, const float* dloss, long long n, Loss lf,
                            float* dpred, hipStream_t s) {
  hipLaunchKernelGGL(k_loss_grad<Loss>, dim3((unsigned)((n + kTailBlock - 1) / kTailBlock)), dim3(kTailBlock), 0, s, pred,
                     truth, dloss, n, lf, dpred);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

int launch_huber_metrics(const float* pred, const float* truth, long long n, float delta, float mask_value,
                         double* part, float* loss, double* sums, float loss_weight, hipStream_t s) {
  return launch_loss_metrics(pred, truth, n, Huber{delta}, mask_value, part, loss, sums, loss_weight, s);
}

int launch_huber_grad(const float* pred, const float* truth, const float* dloss, long long n, float delta,
                      float* dpred, hipStream_t s) {
  return launch_loss_grad(pred, truth, dloss, n, Huber{delta}, dpred, s);
}

int launch_gauss_metrics(const float* pred, const float* truth, long long n, double sigma, double delta,
                         float mask_value, double* part, float* loss, double* sums, float loss_weight, hipStream_t s) {
  return launch_loss_metrics(pred, truth, n, gauss_of(sigma, delta), mask_value, part, loss, sums, loss_weight, s);
}

int launch_gauss_grad(const float* pred, const float* truth, const float* dloss, long long n, double sigma, double delta,
                      float* dpred, hipStream_t s) {
  return launch_loss_grad(pred, truth, dloss, n, gauss_of(sigma, delta), dpred, s);
}

// ---- the gated sum over the components (msgat.py:203-205, embeddings.py:36-39) --------------------------------------
//   out[b,e] = sum_r pred[r,b,e] * (h_w[H[b]][r,e] + d_w[D[b]][r,e])        e = (node, output step)
// The reference runs two embedding gathers, an add, R multiplies and R - 1 adds forward and, backward, R + R multiplies,
// a transposing copy and two dense embedding gradients (a zero fill and a scatter each): 17 launches for 4 MB tensors.
// Here one launch each way.  Indices are clamped into the tables (torch's gather would trap on the device instead).
// Static gate (msgat.py:189): H = D = nullptr, h_w = W[R,E] as a one-row table, d_w = nullptr.  gate_row: common.hpp.
constexpr int kGateMaxB = 1024;   // samples whose table rows a block of the backward keeps in LDS

__global__ __launch_bounds__(kTailBlock) void k_gate_sum(const float* __restrict__ pred, const long long* __restrict__ H,
                                                         const long long* __restrict__ D, const float* __restrict__ h_w,
                                                         const float* __restrict__ d_w, float* __restrict__ out, int R,
                                                         int B, int E, int nh, int nd) {
  const long long i = (long long)blockIdx.x * kTailBlock + threadIdx.x;
  if (i >= (long long)B * E) return;
  const int b = (int)(i / E), e = (int)(i - (long long)b * E);
  const float* hr = h_w + (size_t)gate_row(H, b, nh) * R * E + e;
  const float* dr = d_w ? d_w + (size_t)gate_row(D, b, nd) * R * E + e : nullptr;
  float acc = 0.f;
  {
#pragma clang fp contract(off)   // the reference's ops round the product and the sum separately (hipcc would fuse them)
    for (int r = 0; r < R; ++r) {   // and add in this order: term_0 + term_1 + ...
      const float gate = dr ? hr[(size_t)r * E] + dr[(size_t)r * E] : hr[(size_t)r * E];
      const float term = pred[((size_t)r * B + b) * E + e] * gate;
      acc = r == 0 ? term : acc + term;
    }
  }
  out[i] = acc;
}

// blocks [0, nblkA): dpred[r,b,e] = dout[b,e] * gate; the rest: a table row's gradient, summed over the samples that
// selected it in sample order (thread per (row, r, e); rows [0, nh) of h_w, then [nh, nh + nd) of d_w)
__global__ __launch_bounds__(kTailBlock) void k_gate_sum_bwd(const float* __restrict__ dout, const float* __restrict__ pred,
                                                             const long long* __restrict__ H, const long long* __restrict__ D,
                                                             const float* __restrict__ h_w, const float* __restrict__ d_w,
                                                             float* __restrict__ dpred, float* __restrict__ dh_w,
                                                             float* __restrict__ dd_w, int R, int B, int E, int nh, int nd,
                                                             int nblkA) {
  if ((int)blockIdx.x < nblkA) {
    const long long i = (long long)blockIdx.x * kTailBlock + threadIdx.x;
    if (dpred == nullptr || i >= (long long)R * B * E) return;
    const int e = (int)(i % E), b = (int)((i / E) % B), r = (int)(i / ((long long)E * B));
    float gate = h_w[((size_t)gate_row(H, b, nh) * R + r) * E + e];
    if (d_w) gate += d_w[((size_t)gate_row(D, b, nd) * R + r) * E + e];
    dpred[i] = dout[(size_t)b * E + e] * gate;
    return;
  }
  // the samples' table rows, once per block in LDS (read from global inside the loop below -- B dependent round trips per
  // thread -- this half of the launch took 25 us for 4 MB tensors)
  __shared__ int rows_h[kGateMaxB], rows_d[kGateMaxB];
  const bool staged = B <= kGateMaxB;   // kernel-uniform
  if (staged) {
    for (int b = threadIdx.x; b < B; b += kTailBlock) {
      rows_h[b] = gate_row(H, b, nh);
      rows_d[b] = D ? gate_row(D, b, nd) : 0;
    }
    __syncthreads();
  }
  const long long i = (long long)(blockIdx.x - nblkA) * kTailBlock + threadIdx.x;
  const long long RE = (long long)R * E;
  if (i >= (long long)(nh + nd) * RE) return;
  int row = (int)(i / RE);
  const long long re = i - (long long)row * RE;
  const int r = (int)(re / E), e = (int)(re - (long long)r * E);
  const bool day = row >= nh;
  row -= day ? nh : 0;
  float* dst = day ? dd_w : dh_w;
  if (dst == nullptr) return;
  const long long* idx = day ? D : H;
  const int rows = day ? nd : nh;
  const int* staged_rows = day ? rows_d : rows_h;
  float acc = 0.f;
  for (int b = 0; b < B; ++b) {
    const int rb = staged ? staged_rows[b] : gate_row(idx, b, rows);
    if (rb == row) acc = fmaf(dout[(size_t)b * E + e], pred[((size_t)r * B + b) * E + e], acc);
  }
  dst[(size_t)row * RE + re] = acc;
}

int launch_gate_sum(const float* pred, const long long* H, const long long* D, const float* h_w, const float* d_w, float* out,
                    int R, int B, int E, int nh, int nd, hipStream_t s) {
  const long long n = (long long)B * E;
  hipLaunchKernelGGL(k_gate_sum, dim3((unsigned)((n + kTailBlock - 1) / kTailBlock)), dim3(kTailBlock), 0, s, pred, H, D, h_w,
                     d_w, out, R, B, E, nh, nd);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

int launch_gate_sum_bwd(const float* dout, const float* pred, const long long* H, const long long* D, const float* h_w,
                        const float* d_w, float* dpred, float* dh_w, float* dd_w, int R, int B, int E, int nh, int nd,
                        hipStream_t s) {
  const long long nA = dpred ? (long long)R * B * E : 0, nB = (long long)(nh + (d_w ? nd : 0)) * R * E;
  const int nblkA = (int)((nA + kTailBlock - 1) / kTailBlock);
  const long long nblk = nblkA + (nB + kTailBlock - 1) / kTailBlock;
  if (nblk == 0) return MSGAT_OK;
  hipLaunchKernelGGL(k_gate_sum_bwd, dim3((unsigned)nblk), dim3(kTailBlock), 0, s, dout, pred, H, D, h_w, d_w, dpred, dh_w,
                     dd_w, R, B, E, nh, d_w ? nd : 0, nblkA);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

// ---- Adam ---------------------------------------------------------------------------------------------------------
// Chunk c covers chunk_len[c] <= kAdamChunk elements of parameter tensor chunk_tensor[c], starting at chunk_param[c];
// its gradient and moments sit at chunk_off[c] of the flat buffers.  steps[t] = updates tensor t has received (torch
// keeps one step count per parameter: a parameter without a gradient is skipped and its bias correction lags);
// lr[0] = learning rate.  Both live in device memory, so a captured launch follows the scheduler.
constexpr int kAdamChunk = 2048;

// ---- the guard on the update: global gradient norm, clipping coefficient, finiteness ---------------------------------
// guard [kGuardFloats] fp32, device: {pre-clip norm of this step, coef, steps skipped so far, largest finite pre-clip
// norm since the caller zeroed it, 1 if this step's sum of squares is finite else 0}.
//   k_grad_sumsq     block c squares chunk c of the flat gradient (the chunk table of k_adam: a parameter without a
//                    gradient has no chunk, its stale flat contents are never read) in double -- (1e30)^2 is no overflow
//                    there -- lane by lane with stride 256, the butterfly of wave_sum, then the four waves in order.
//   k_guard_finish   lane 0 adds the partials in index order (staged through LDS 1024 at a time by the whole block, so
//                    the serial part is ~1000 dependent adds, not ~1000 dependent loads), then
//                    norm = sqrt(S) / D, coef = min(1, max_norm / (norm + 1e-6)) in fp32 as clip_grad_norm_ computes it
//                    (max_norm = +inf: 1).  A step whose S is not finite counts as skipped.
// One fixed order throughout and no atomics: equal inputs give equal bits, on every launch and on every rank.
constexpr int kGuardNorm = 0, kGuardCoef = 1, kGuardSkipped = 2, kGuardMax = 3, kGuardFinite = 4;
constexpr int kGuardTile = 1024;

__global__ __launch_bounds__(kTailBlock) void k_grad_sumsq(const long long* __restrict__ chunk_off,
                                                           const int* __restrict__ chunk_len,
                                                           const float* __restrict__ grad, double* __restrict__ part) {
  __shared__ double red[kTailBlock / 64];
  const int c = blockIdx.x;
  const float* __restrict__ g = grad + chunk_off[c];
  const int len = chunk_len[c];
  double s = 0.0;
  for (int i = threadIdx.x; i < len; i += kTailBlock) {
    const double x = (double)g[i];
    s += x * x;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kTailBlock / 64; ++w) t += red[w];
    part[c] = t;
  }
}

__global__ __launch_bounds__(kTailBlock) void k_guard_finish(const double* __restrict__ part, int nparts,
                                                             const float* __restrict__ grad_divisor, float max_norm,
                                                             float* __restrict__ guard) {
  __shared__ double tile[kGuardTile];
  double S = 0.0;
  for (int base = 0; base < nparts; base += kGuardTile) {   // nparts is kernel-uniform: every lane meets every barrier
    const int m = nparts - base < kGuardTile ? nparts - base : kGuardTile;
    for (int i = threadIdx.x; i < m; i += kTailBlock) tile[i] = part[base + i];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < m; ++i) S += tile[i];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double D = grad_divisor != nullptr ? (double)grad_divisor[0] : 1.0;
  const bool finite = isfinite(S);
  const float norm = (float)(sqrt(S) / D);
  guard[kGuardNorm] = norm;
  guard[kGuardCoef] = finite ? fminf(1.f, max_norm / (norm + 1e-6f)) : 0.f;
  guard[kGuardFinite] = finite ? 1.f : 0.f;
  if (!finite) guard[kGuardSkipped] += 1.f;
  else if (isfinite(norm)) guard[kGuardMax] = fmaxf(guard[kGuardMax], norm);
}

int launch_grad_guard(const long long* chunk_off, const int* chunk_len, int nchunks, const float* grad,
                      const float* grad_divisor, float max_norm, double* part, float* guard, hipStream_t s) {
  if (nchunks > 0) {
    hipLaunchKernelGGL(k_grad_sumsq, dim3(nchunks), dim3(kTailBlock), 0, s, chunk_off, chunk_len, grad, part);
    MSGAT_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_guard_finish, dim3(1), dim3(kTailBlock), 0, s, part, nchunks, grad_divisor, max_norm, guard);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

// kGuard: a step whose gradient norm is not finite advances no step count and (k_adam) writes nothing at all
template <bool kGuard>
__global__ void k_adam_advance(float* __restrict__ steps, const int* __restrict__ active, int n_active,
                               const float* __restrict__ guard) {
  if (kGuard && guard[kGuardFinite] == 0.f) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_active) steps[active[i]] += 1.0f;
}

// The average of the weights (optional: msgat_adam_step_averaged).  After w_new is formed, the shadow e of the element moves
// towards it by 1 - d, d = min(decay, (1 + t) / (10 + t)) with t the tensor's own step count (already advanced): the
// warm-up of the average per tensor, on the only clock the update has.  Every operation is rounded on its own, in fp32 --
// a numpy float32 restatement gives the same bits.  Contraction is switched off in these functions: the __f*_rn spellings
// of this toolchain are plain operators, which the default (-ffp-contract=fast) would fuse into an fma after inlining.
// k_adam takes the shadow as a trailing argument pack: empty for the two kernels that existed before the average (their
// signature, and their code, are what they were), one Shadow for the averaged ones.
struct Shadow {
  float* e;      // flat, in the layout of the moments
  float decay;
};
__device__ __forceinline__ float average_rate(float) { return 0.f; }            // no shadow: nothing is averaged
__device__ __forceinline__ float average_load(long long) { return 0.f; }
__device__ __forceinline__ void average_move(long long, float, float, float) {}
__device__ __forceinline__ float average_rate(float t, Shadow s) {
#pragma clang fp contract(off)
  const float d = fminf(s.decay, (1.f + t) / (10.f + t));
  return 1.f - d;
}
__device__ __forceinline__ float average_load(long long at, Shadow s) { return s.e[at]; }
__device__ __forceinline__ void average_move(long long at, float e, float w_new, float omd, Shadow s) {
#pragma clang fp contract(off)
  const float diff = w_new - e;
  const float step = omd * diff;
  s.e[at] = e + step;
}

template <bool kGuard, class... Average>
__global__ __launch_bounds__(kTailBlock) void k_adam(float* const* __restrict__ chunk_param,
                                                     const long long* __restrict__ chunk_off,
                                                     const int* __restrict__ chunk_len,
                                                     const int* __restrict__ chunk_tensor,
                                                     const float* __restrict__ grad, float* __restrict__ m,
                                                     float* __restrict__ v, const float* __restrict__ steps,
                                                     const float* __restrict__ lrp, double beta1d, double beta2d,
                                                     float eps, float weight_decay,
                                                     const float* __restrict__ grad_divisor,
                                                     const float* __restrict__ guard, Average... shadow) {
  if (kGuard && guard[kGuardFinite] == 0.f) return;   // kernel-uniform
  // clip_grad_norm_ scales the raw gradient, optim.Adam then adds the L2 term: coef acts before weight_decay * w
  const float coef = kGuard ? guard[kGuardCoef] : 1.f;
  const int c = blockIdx.x;
  float* p = chunk_param[c];
  const long long off = chunk_off[c];
  const int len = chunk_len[c];
  const float t = steps[chunk_tensor[c]], lr = lrp[0];
  // data-parallel step: the flat buffer holds sum_ranks(w_r g_r) and *grad_divisor = sum_ranks(w_r) (the last element
  // of the same all-reduced buffer); the division that used to be a pass of its own happens on the way in
  const bool scaled = grad_divisor != nullptr;
  const float div = scaled ? grad_divisor[0] : 1.f;
  // torch.optim.Adam (_single_tensor_adam): bias_correction = 1 - beta^t; step_size = lr / bc1;
  // denom = sqrt(v) / sqrt(bc2) + eps; p -= step_size * m / denom
  // (in double, as the host-side Python floats of the reference optimizer are: 1 - 0.999^t cancels badly in fp32)
  const double bc1 = 1.0 - pow(beta1d, (double)t), bc2 = 1.0 - pow(beta2d, (double)t);
  const float beta2 = (float)beta2d, omb1 = (float)(1.0 - beta1d), omb2 = (float)(1.0 - beta2d);  // 1 - beta rounded once
  const float step_size = (float)((double)lr / bc1), bc2_sqrt = (float)sqrt(bc2);
  const float omd = average_rate(t, shadow...);       // 1 - d of this tensor
  for (int i = threadIdx.x; i < len; i += kTailBlock) {
    const float w = p[i];
    float gin = scaled ? grad[off + i] / div : grad[off + i];
    if (kGuard) gin = coef * gin;                     // coef == 1: the same bits as the unguarded kernel
    const float g = fmaf(weight_decay, w, gin);
    float mi = m[off + i], vi = v[off + i];
    const float e = average_load(off + i, shadow...);  // ahead of the parameter's store, which it cannot be moved across
    mi = fmaf(g - mi, omb1, mi);                      // exp_avg.lerp_(grad, 1 - beta1)
    vi = fmaf(g * g, omb2, vi * beta2);               // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    m[off + i] = mi;
    v[off + i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    const float w_new = w - step_size * (mi / denom);
    p[i] = w_new;
    average_move(off + i, e, w_new, omd, shadow...);
  }
}

// guard == nullptr: the unguarded update; shadow == nullptr: no averaged weights (decay is not read)
int launch_adam(float* const* chunk_param, const long long* chunk_off, const int* chunk_len, const int* chunk_tensor,
                int nchunks, const int* active, int n_active, const float* grad, float* m, float* v, float* steps,
                const float* lr, double beta1, double beta2, double eps, double weight_decay, const float* grad_divisor,
                const float* guard, float* shadow, double decay, hipStream_t s) {
  if (n_active > 0) {
    const auto advance = guard ? k_adam_advance<true> : k_adam_advance<false>;
    hipLaunchKernelGGL(advance, dim3(cdiv(n_active, kTailBlock)), dim3(kTailBlock), 0, s, steps, active, n_active, guard);
    MSGAT_CHECK_LAUNCH();
  }
  if (nchunks > 0) {
    auto launch = [&](auto kernel, auto... average) {
      hipLaunchKernelGGL(kernel, dim3(nchunks), dim3(kTailBlock), 0, s, chunk_param, chunk_off, chunk_len, chunk_tensor,
                         grad, m, v, steps, lr, beta1, beta2, (float)eps, (float)weight_decay, grad_divisor, guard,
                         average...);
    };
    if (shadow) launch(guard ? k_adam<true, Shadow> : k_adam<false, Shadow>, Shadow{shadow, (float)decay});
    else launch(guard ? k_adam<true> : k_adam<false>);
    MSGAT_CHECK_LAUNCH();
  }
  return MSGAT_OK;
}

// ---- parameters <-> a flat buffer, exchanged in place --------------------------------------------------------------
// Block c swaps chunk_param[c][i] with flat[chunk_off[c] + i] as 32-bit words (NaNs keep their bits; two calls are the
// identity).  With flat = the shadow, whatever holds the parameters' addresses -- a captured validation graph -- reads
// the averaged weights.  Parameter views are 4-byte aligned only: scalar accesses, as in k_adam.
__global__ __launch_bounds__(kTailBlock) void k_param_swap(unsigned* const* __restrict__ chunk_param,
                                                           const long long* __restrict__ chunk_off,
                                                           const int* __restrict__ chunk_len,
                                                           unsigned* __restrict__ flat) {
  const int c = blockIdx.x;
  unsigned* p = chunk_param[c];
  unsigned* __restrict__ f = flat + chunk_off[c];
  const int len = chunk_len[c];
  for (int i = threadIdx.x; i < len; i += kTailBlock) {
    const unsigned a = p[i], b = f[i];
    p[i] = b;
    f[i] = a;
  }
}

int launch_param_swap(float* const* chunk_param, const long long* chunk_off, const int* chunk_len, int nchunks,
                      float* flat, hipStream_t s) {
  hipLaunchKernelGGL(k_param_swap, dim3(nchunks), dim3(kTailBlock), 0, s, (unsigned* const*)chunk_param, chunk_off,
                     chunk_len, (unsigned*)flat);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

int adam_chunk_elems() { return kAdamChunk; }

// ---- gather of the gradients into the flat buffer a data-parallel step all-reduces -----------------------------------
// Overwriting form: flat[chunk_off[c] + i] = scale * chunk_src[c][i]; block 0 also writes flat[weight_index] = scale: the
// rank's weight (its sample count) rides in the buffer's last element, so sum(w g) and sum(w) come out of ONE collective.
// Replaces a multi-tensor copy + mul_ + fill_ over the 7.8 MB buffer by one pass.
// Accumulating form (gradient accumulation: a later micro-batch of a window): flat[chunk_off[c] + i] += scale *
// chunk_src[c][i], and block 0 does flat[weight_index] += scale.  The first micro-batch of a window overwrites (no zeroing
// pass), every later one accumulates, so after k micro-batches the buffer holds sum(w g) and sum(w) in call order -- what
// the all-reduce of k ranks would have summed.  The product and the sum are rounded one after the other in fp32
// (contraction off, as in average_move: an fma would round once), which is what makes two accumulated micro-batches
// bit-equal to the two-rank all-reduce sum of the same two gradients, and a numpy float32 restatement bit-equal to both.
// The scale travels by value (a sample count) or is read from device memory once per block (the valid count of a masked
// batch, which only the device knows and which is never read back).
// Every element is read and written by one lane of one block, block 0's lane 0 alone touches the weight: no atomics, one
// fixed order.  Parameter views and flat offsets are 4-byte aligned only: scalar accesses, as in k_adam.
__device__ __forceinline__ float scale_of(float scale) { return scale; }
__device__ __forceinline__ float scale_of(const float* scale) { return scale[0]; }

__device__ __forceinline__ void accumulate_chunk(const float* __restrict__ src, float* __restrict__ dst, int len,
                                                 float scale) {
#pragma clang fp contract(off)
  for (int i = threadIdx.x; i < len; i += kTailBlock) {
    const float term = scale * src[i];
    dst[i] = dst[i] + term;
  }
}

template <bool kAccumulate, class Scale>   // Scale: float or const float*
__global__ __launch_bounds__(kTailBlock) void k_gather(const float* const* __restrict__ chunk_src,
                                                       const long long* __restrict__ chunk_off,
                                                       const int* __restrict__ chunk_len, Scale scale,
                                                       float* __restrict__ flat, long long weight_index) {
  const int c = blockIdx.x;
  const float sc = scale_of(scale);
  const float* __restrict__ src = chunk_src[c];
  float* __restrict__ dst = flat + chunk_off[c];
  const int len = chunk_len[c];
  if (kAccumulate) {
    accumulate_chunk(src, dst, len, sc);
  } else {
    for (int i = threadIdx.x; i < len; i += kTailBlock) dst[i] = sc * src[i];   // no sum to fuse
  }
  if (c == 0 && threadIdx.x == 0 && weight_index >= 0) flat[weight_index] = kAccumulate ? flat[weight_index] + sc : sc;
}

// scale_dev != nullptr: the scale is scale_dev[0], read by the kernel; otherwise `scale`
int launch_gather(const float* const* chunk_src, const long long* chunk_off, const int* chunk_len, int nchunks, float scale,
                  const float* scale_dev, bool accumulate, float* flat, long long weight_index, hipStream_t s) {
  auto launch = [&](auto kernel, auto sc) {
    hipLaunchKernelGGL(kernel, dim3(nchunks), dim3(kTailBlock), 0, s, chunk_src, chunk_off, chunk_len, sc, flat,
                       weight_index);
  };
  if (scale_dev) launch(accumulate ? k_gather<true, const float*> : k_gather<false, const float*>, scale_dev);
  else launch(accumulate ? k_gather<true, float> : k_gather<false, float>, scale);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

// ---- masked loss (Huber or Gauss: the policies above) + per-horizon metric sums ---------------------------------------------------------------------
// An entry of the truth counts when it is a measurement (entry_valid, tail_terms.hpp).
//   k_masked_loss_metrics    the first (256 / T) * T lanes of a block walk the elements with a stride that is a multiple
//                            of T, so a lane keeps ONE horizon (element i has horizon i mod T) and its five sums
//                            {valid count, |e|, 100 |e / y| (y > mask), e^2, loss} stay in registers, while a block
//                            trip still reads consecutive addresses.
//   horizon_handover         the lanes of a horizon hand their sums over through LDS once per block and are added in
//                            lane order: one record [cols][T] per block, stored column-major over the blocks
//                            (part[(c T + h) nblocks + b]).
//   k_horizon_finish         block c adds column c: a wave per horizon, lane l takes blocks l, l + 64, ... in order, then
//                            the butterfly of wave_sum; the all-horizon row is the sum of the horizon rows in horizon
//                            order.  The block of the loss column adds the count column too and writes loss and valid.
//                            It only adds partials: the column count and the loss column are arguments.
// Every sum has one fixed order: bitwise reproducible.  No floating-point atomics.
constexpr int kMaskCols = kPointCols;
constexpr int kMaskMaxT = 64;
constexpr int kMaskMaxBlocks = 512;
constexpr int kMaskFinishBlock = 1024;

template <int kCols>
__device__ __forceinline__ void horizon_handover(const double (&s)[kCols], double (&red)[kCols][kTailBlock], int T,
                                                 int lanes, double* __restrict__ part) {
#pragma unroll
  for (int c = 0; c < kCols; ++c) red[c][threadIdx.x] = s[c];
  __syncthreads();
  for (int o = threadIdx.x; o < kCols * T; o += kTailBlock) {
    const int c = o / T, h = o - c * T;
    double t = 0.0;
    for (int j = h; j < lanes; j += T) t += red[c][j];
    part[(size_t)o * gridDim.x + blockIdx.x] = t;
  }
}

template <class Loss>
__global__ __launch_bounds__(kTailBlock) void k_masked_loss_metrics(const float* __restrict__ pred,
                                                                    const float* __restrict__ truth, long long n, int T,
                                                                    int lanes, Loss loss, float null_value,
                                                                    float mask_value, double* __restrict__ part) {
  __shared__ double red[kMaskCols][kTailBlock];
  double s[kMaskCols] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if ((int)threadIdx.x < lanes) {   // lanes % T == 0: i mod T == threadIdx.x mod T on every trip
    const long long stride = (long long)gridDim.x * lanes;
    for (long long i = (long long)blockIdx.x * lanes + threadIdx.x; i < n; i += stride) {
      const float p = pred[i], y = truth[i];
      if (!entry_valid(y, null_value)) continue;
      const PointTerms t = point_terms(p, y, mask_value);
      s[kColCount] += 1.0;
      s[kColAbs] += t.abs_err;
      if (t.ape_counts) s[kColApe] += t.ape;
      s[kColSq] += t.sq_err;
      s[kMaskLossCol] += loss.value(t.abs_err);
    }
  }
  horizon_handover(s, red, T, lanes, part);
}

__global__ __launch_bounds__(kMaskFinishBlock) void k_horizon_finish(const double* __restrict__ part, int nblocks, int T,
                                                                     int cols, int loss_col, float* __restrict__ loss,
                                                                     float* __restrict__ valid,
                                                                     double* __restrict__ sums) {
  __shared__ double rows[2][kMaskMaxT];   // [0]: this block's column per horizon, [1]: the count column (loss block)
  const int c = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool is_loss = c == loss_col;
  for (int q = 0; q < (is_loss ? 2 : 1); ++q) {
    const int col = q == 0 ? c : kColCount;
    for (int h = wave; h < T; h += kMaskFinishBlock / 64) {
      const double* __restrict__ p = part + (size_t)(col * T + h) * nblocks;
      double t = 0.0;
      for (int b = lane; b < nblocks; b += 64) t += p[b];
      t = wave_sum(t);
      if (lane == 0) rows[q][h] = t;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < T && sums != nullptr) sums[(size_t)threadIdx.x * cols + c] += rows[0][threadIdx.x];
  if (threadIdx.x != 0) return;
  double total = 0.0, count = 0.0;
  for (int h = 0; h < T; ++h) total += rows[0][h];
  if (sums != nullptr) sums[(size_t)T * cols + c] += total;
  if (!is_loss) return;
  for (int h = 0; h < T; ++h) count += rows[1][h];
  valid[0] = (float)count;
  loss[0] = (float)(total / fmax(count, 1.0));
}

// dpred = dloss[0] * slope(e) / max(valid[0], 1) at the valid entries, +0 elsewhere (a NaN of the truth
// ends in the select, not in the product); valid[0] comes from device memory: a captured launch follows its batch
template <class Loss>
__global__ __launch_bounds__(kTailBlock) void k_masked_loss_grad(const float* __restrict__ pred,
                                                                 const float* __restrict__ truth,
                                                                 const float* __restrict__ dloss,
                                                                 const float* __restrict__ valid, long long n,
                                                                 Loss loss, float null_value,
                                                                 float* __restrict__ dpred) {
  const long long i = (long long)blockIdx.x * kTailBlock + threadIdx.x;
  if (i >= n) return;
  const float y = truth[i];
  const float e = pred[i] - y;
  const float g = loss.slope(e);
  dpred[i] = entry_valid(y, null_value) ? g * (dloss[0] / fmaxf(valid[0], 1.f)) : 0.f;
}

static int horizon_lanes(int T) { return (kTailBlock / T) * T; }

static int horizon_blocks(long long n, int T) {
  const long long per_block = (long long)horizon_lanes(T) * kTailPerThread;
  const long long want = (n + per_block - 1) / per_block;
  return (int)(want < 1 ? 1 : (want > kMaskMaxBlocks ? kMaskMaxBlocks : want));
}

size_t masked_huber_partial_doubles(long long rows, int T) {
  return (size_t)horizon_blocks(rows * T, T) * kMaskCols * T;
}

template <class Loss>
static int launch_masked_loss_metrics(const float* pred, const float* truth, long long rows, int T, Loss lf,
                                      float null_value, float mask_value, double* part, float* loss, float* valid,
                                      double* sums, hipStream_t s) {
  const long long n = rows * T;
  const int nb = horizon_blocks(n, T);
  hipLaunchKernelGGL(k_masked_loss_metrics<Loss>, dim3(nb), dim3(kTailBlock), 0, s, pred, truth, n, T,
                     horizon_lanes(T), lf, null_value, mask_value, part);
  MSGAT_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_horizon_finish, dim3(kMaskCols), dim3(kMaskFinishBlock), 0, s, part, nb, T, kMaskCols, kMaskLossCol,
                     loss, valid, sums);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

template <class Loss>
static int launch_masked_loss_grad(const float* pred, const float* truth, const float* dloss, const float* valid,
                                   long long rows, int T, Loss lf, float null_value, float* dpred, hipStream_t s) {
  const long long n = rows * T;
  hipLaunchKernelGGL(k_masked_loss_grad<Loss>, dim3((unsigned)((n + kTailBlock - 1) / kTailBlock)), dim3(kTailBlock), 0, s,
                     pred, truth, dloss, valid, n, lf, null_value, dpred);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

int launch_masked_huber_metrics(const float* pred, const float* truth, long long rows, int T, float delta,
                                float null_value, float mask_value, double* part, float* loss, float* valid,
                                double* sums, hipStream_t s) {
  return launch_masked_loss_metrics(pred, truth, rows, T, Huber{delta}, null_value, mask_value, part, loss, valid, sums, s);
}

int launch_masked_huber_grad(const float* pred, const float* truth, const float* dloss, const float* valid,
                             long long rows, int T, float delta, float null_value, float* dpred, hipStream_t s) {
  return launch_masked_loss_grad(pred, truth, dloss, valid, rows, T, Huber{delta}, null_value, dpred, s);
}

int launch_masked_gauss_metrics(const float* pred, const float* truth, long long rows, int T, double sigma, double delta,
                                float null_value, float mask_value, double* part, float* loss, float* valid,
                                double* sums, hipStream_t s) {
  return launch_masked_loss_metrics(pred, truth, rows, T, gauss_of(sigma, delta), null_value, mask_value, part, loss, valid,
                                    sums, s);
}

int launch_masked_gauss_grad(const float* pred, const float* truth, const float* dloss, const float* valid,
                             long long rows, int T, double sigma, double delta, float null_value, float* dpred,
                             hipStream_t s) {
  return launch_masked_loss_grad(pred, truth, dloss, valid, rows, T, gauss_of(sigma, delta), null_value, dpred, s);
}

// ---- quantile forecasts: pinball loss, point metrics at one level, coverage / width / crossing sums ----------------------
// pred [rows, Q, T] (level-major inside a row: the lanes of a horizon group read consecutive addresses for every level),
// truth [rows, T]; validity is entry_valid of the masked tail.  Per valid entry and level, u = y - p_q in fp32:
//   rho_q = max(tau_q u, (tau_q - 1) u);  d rho_q / d p_q = -tau_q (y > p_q), 1 - tau_q (y < p_q), 1/2 - tau_q at a tie
//   (autograd's rule for torch.maximum).  tau_q - 1 and the three slopes over Q are formed in double on the host and
//   rounded to fp32 once; they travel by value (QuantLevels / QuantSlopes), like the policies above.
// Columns of a record and of sums [T + 1, 7 + 2Q] (tail_terms.hpp, where an entry's terms are formed):
//   0-3 the masked tail's {count, |e|, 100 |e / y| (y > mask), e^2} with e = p_point - y;  4 sum of (1/Q) sum_q rho_q;
//   5 entries with any p_q > p_{q+1};  6 sum of p_{Q-1} - p_0;  7 + q entries with y <= p_q;  7 + Q + q sum of rho_q.
//   k_quantile_metrics<Q>    k_masked_loss_metrics' walk (a lane keeps ONE horizon, its 7 + 2Q sums stay in registers in
//                            double -- Q is a template parameter so that they ARE registers) and horizon_handover: one
//                            [7 + 2Q][256] LDS image (26 KB at Q = 3, 46 KB at Q = 8: under the 64 KB static limit, and
//                            with at most 512 blocks of this launch on 256 CUs no limit on residency), ONE barrier.
//                            k_horizon_finish then adds 7 + 2Q columns, loss column 4.
// One fixed order for every sum, no floating-point atomics: bitwise reproducible.
struct QuantSlopes { float above[kQuantMaxQ], below[kQuantMaxQ], tie[kQuantMaxQ]; };   // y > p_q, y < p_q, y == p_q

template <int Q>
__global__ __launch_bounds__(kTailBlock) void k_quantile_metrics(const float* __restrict__ pred,
                                                                 const float* __restrict__ truth, int n, int T, int lanes,
                                                                 QuantLevels lv, int point, float null_value,
                                                                 float mask_value, double* __restrict__ part) {
  constexpr int kCols = quant_cols(Q);
  __shared__ double red[kCols][kTailBlock];
  double s[kCols];
#pragma unroll
  for (int c = 0; c < kCols; ++c) s[c] = 0.0;
  if ((int)threadIdx.x < lanes) {   // lanes % T == 0: i mod T == threadIdx.x mod T on every trip
    const int t = (int)threadIdx.x % T;
    const int stride = (int)gridDim.x * lanes;
    for (int i = (int)blockIdx.x * lanes + (int)threadIdx.x; i < n; i += stride) {   // n <= 2^24
      const float y = truth[i];
      const float* __restrict__ pr = pred + (size_t)(i / T) * (size_t)(Q * T) + t;
      float p[Q];
#pragma unroll
      for (int q = 0; q < Q; ++q) p[q] = pr[q * T];
      if (!entry_valid(y, null_value)) continue;
      const PointTerms pt = point_terms(point_forecast(p, point), y, mask_value);
      s[kColCount] += 1.0;
      s[kColAbs] += pt.abs_err;
      if (pt.ape_counts) s[kColApe] += pt.ape;
      s[kColSq] += pt.sq_err;
      double total = 0.0;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const LevelTerm lt = level_term(p[q], y, lv.tau[q], lv.tau_m1[q]);
        total += (double)lt.rho;
        s[quant_rho_col(Q, q)] += (double)lt.rho;
        if (lt.hit) s[quant_hit_col(q)] += 1.0;
      }
      s[kQuantLossCol] += total * (1.0 / Q);
      if (levels_cross(p)) s[kQuantCrossCol] += 1.0;
      s[kQuantWidthCol] += (double)levels_width(p);
    }
  }
  horizon_handover(s, red, T, lanes, part);
}

// dpred[r,q,t] = c_q (dloss[0] / max(valid[0], 1)) at the valid entries, c_q the slope of its sign case over Q; +0
// elsewhere (a NaN of the truth fails both comparisons and ends in the select).  A lane takes one (r, t) and its Q levels.
__global__ __launch_bounds__(kTailBlock) void k_quantile_grad(const float* __restrict__ pred,
                                                              const float* __restrict__ truth,
                                                              const float* __restrict__ dloss,
                                                              const float* __restrict__ valid, int n, int T, int Q,
                                                              QuantSlopes sl, float null_value,
                                                              float* __restrict__ dpred) {
  const int i = (int)blockIdx.x * kTailBlock + (int)threadIdx.x;
  if (i >= n) return;
  const float y = truth[i];
  const int r = i / T;
  const size_t base = (size_t)r * (size_t)(Q * T) + (size_t)(i - r * T);
  const bool ok = entry_valid(y, null_value);
  const float scale = dloss[0] / fmaxf(valid[0], 1.f);
#pragma unroll
  for (int q = 0; q < kQuantMaxQ; ++q) {
    if (q >= Q) break;   // kernel-uniform; unrolled, so the slopes are read at constant offsets of the argument
    const float p = pred[base + (size_t)q * T];
    const float c = y > p ? sl.above[q] : (y < p ? sl.below[q] : sl.tie[q]);
    dpred[base + (size_t)q * T] = ok ? c * scale : 0.f;
  }
}

size_t quantile_partial_doubles(long long rows, int T, int Q) {
  return (size_t)horizon_blocks(rows * T, T) * (size_t)quant_cols(Q) * T;
}

template <int Q>
static void launch_quantile_metrics_q(const float* pred, const float* truth, int n, int T, const QuantLevels& lv, int point,
                                      float null_value, float mask_value, double* part, int nb, hipStream_t s) {
  hipLaunchKernelGGL(k_quantile_metrics<Q>, dim3(nb), dim3(kTailBlock), 0, s, pred, truth, n, T, horizon_lanes(T), lv,
                     point, null_value, mask_value, part);
}

int launch_quantile_metrics(const float* pred, const float* truth, long long rows, int T, int Q, const float* levels,
                            int point, float null_value, float mask_value, double* part, float* loss, float* valid,
                            double* sums, hipStream_t s) {
  if (rows == 0) {   // nothing to walk: loss 0 and valid 0 (the bits of +0.f), the totals as they were
    hipError_t e = hipMemsetAsync(loss, 0, sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(valid, 0, sizeof(float), s);
    return e == hipSuccess ? MSGAT_OK : MSGAT_ERR_HIP_BASE - (int)e;
  }
  const QuantLevels lv = quant_levels(levels, Q);
  const int n = (int)(rows * T), nb = horizon_blocks(n, T);
  switch (Q) {
    case 1: launch_quantile_metrics_q<1>(pred, truth, n, T, lv, point, null_value, mask_value, part, nb, s); break;
    case 2: launch_quantile_metrics_q<2>(pred, truth, n, T, lv, point, null_value, mask_value, part, nb, s); break;
    case 3: launch_quantile_metrics_q<3>(pred, truth, n, T, lv, point, null_value, mask_value, part, nb, s); break;
    case 4: launch_quantile_metrics_q<4>(pred, truth, n, T, lv, point, null_value, mask_value, part, nb, s); break;
    case 5: launch_quantile_metrics_q<5>(pred, truth, n, T, lv, point, null_value, mask_value, part, nb, s); break;
    case 6: launch_quantile_metrics_q<6>(pred, truth, n, T, lv, point, null_value, mask_value, part, nb, s); break;
    case 7: launch_quantile_metrics_q<7>(pred, truth, n, T, lv, point, null_value, mask_value, part, nb, s); break;
    case 8: launch_quantile_metrics_q<8>(pred, truth, n, T, lv, point, null_value, mask_value, part, nb, s); break;
    default: return MSGAT_ERR_UNSUPPORTED;
  }
  MSGAT_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_horizon_finish, dim3(quant_cols(Q)), dim3(kMaskFinishBlock), 0, s, part, nb, T, quant_cols(Q),
                     kQuantLossCol, loss, valid, sums);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

int launch_quantile_grad(const float* pred, const float* truth, const float* dloss, const float* valid, long long rows,
                         int T, int Q, const float* levels, float null_value, float* dpred, hipStream_t s) {
  if (rows == 0) return MSGAT_OK;
  QuantSlopes sl = {};
  for (int q = 0; q < Q; ++q) {
    const double tau = (double)levels[q];
    sl.above[q] = (float)(-tau / Q);
    sl.below[q] = (float)((1.0 - tau) / Q);
    sl.tie[q] = (float)((0.5 - tau) / Q);
  }
  const int n = (int)(rows * T);
  hipLaunchKernelGGL(k_quantile_grad, dim3((unsigned)((n + kTailBlock - 1) / kTailBlock)), dim3(kTailBlock), 0, s, pred,
                     truth, dloss, valid, n, T, Q, sl, null_value, dpred);
  MSGAT_CHECK_LAUNCH();
  return MSGAT_OK;
}

}  // namespace msgat
