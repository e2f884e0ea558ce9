/*
 * msgat_hip.h -- C ABI of libmsgat_hip.so: the MI355X (gfx950) implementation of the
 * MS-GAT graph-attention hot path.
 *
 * The reference (luokn/ms-gat) has no FFI: its hot path is a sequence of PyTorch eager
 * ops.  Each entry point below names the reference lines it replaces (paths under
 * /root/reference/).  INTEGRATION.md shows the ctypes binding a maintainer adds to call
 * them from `GraphAttention.forward` / `GACN.forward`.
 *
 * Conventions
 *   - plain C, PODs only: raw device pointers, ints, a hipStream_t passed as void*.
 *   - every device entry point only ENQUEUES kernels on `stream` and returns; it never
 *     allocates, frees or synchronises (re-entrant; safe under hipGraph capture).  All
 *     buffers, including the tensors saved for backward and the workspace, are owned by
 *     the caller.  The only process-wide state is a set of per-device, write-once caches
 *     inside the launchers (csrc/common.hpp: the device's compute-unit count, and per
 *     kernel the dynamic-LDS ceiling already granted by hipFuncSetAttribute): lock-free,
 *     idempotent -- a lost race repeats a driver call -- and indexed by the CURRENT HIP
 *     device, which the caller makes the device of `stream` before the call.  Device
 *     ordinals >= 32 (or a failed hipGetDevice) are never aliased to another device's
 *     entry: for them the driver calls are simply repeated on every launch.
 *   - return value: 0 (MSGAT_OK) or a negative MSGAT_ERR_* code; hipError_t e from a
 *     launch is reported as MSGAT_ERR_HIP_BASE - e.  No exceptions cross the ABI.
 *   - all floating point is IEEE fp32; tensors are dense, contiguous, row-major.  (From N = 1536 nodes the two dense
 *     passes of the attention multiply on the bf16 / fp16 matrix core with every fp32 operand split into three bf16 or two
 *     scaled fp16 terms and fp32 accumulation -- fp32-class accuracy, see msgat_dense_scratch_bytes.)
 *
 * Vocabulary
 *   relation r in [0,R)  one independent parameter set (alpha_r, Wg_r, W_r).  The
 *                        reference evaluates R = n_components such sets over one shared
 *                        adjacency (msgat.py:191-199,204); a single GACN call has R = 1.
 *   group    g in [0,G)  one (relation, sample) pair, G = R*Bg, g = r*Bg + b.  A group is
 *                        one [N,N] attention problem (attention is per sample,
 *                        attention.py:34).
 *   signals  x[G,C,N,T]  the reference's [batch, channels, nodes, timesteps] layout
 *                        (attention.py:21), relations stacked on the batch axis.
 *   graph                CSR + CSC of the non-zeros of the [N,N] adjacency
 *                        (data_loader.py:59-66 builds it dense; msgat.py:190 holds it).
 */
#ifndef MSGAT_HIP_H
#define MSGAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 10: + msgat_adjacency_grad{,_workspace_bytes} (the gradient of a dense adjacency that requires grad); nothing else changed.
 *     Later, still 10 (new functions only; no structure, signature or status code changed): + msgat_graph_build_indices
 *     (a structure from CSR index arrays) and msgat_edge_weight_grad{,_workspace_bytes} (the gradient of the stored
 *     values of a sparse adjacency); + msgat_attention_map, msgat_gacn_backward_edge_grad,
 *     msgat_attention_backward_edge_grad and msgat_edge_softmax_grad (reading the attention weights);
 *     + msgat_edge_weight_grad_sets{,_workspace_bytes} (the gradient of a per-sample sparse adjacency's values [n_sets,nnz]);
 *     + msgat_softmax_map_grad{,_workspace_bytes} and msgat_gacn_backward_map_grad (a gradient at the dense softmax map);
 *     + msgat_masked_huber_{partial_doubles,metrics,grad} and msgat_gather_scaled_dev (the step tail with missing readings);
 *     + msgat_grad_guard{,_partial_doubles} and msgat_adam_step_guarded (global-norm clipping, non-finite steps left out);
 *     + msgat_window_gather (a step's input windows from a series resident in device memory);
 *     + msgat_gauss_{metrics,grad} and msgat_masked_gauss_{metrics,grad} (the Gauss loss in the step tail);
 *     + msgat_edge_time_weights{,_backward} (hour- and day-dependent edge weights on one shared sparse pattern);
 *     + msgat_edge_signal_weights{,_backward} (edge weights from the per-sample node signals at the edge's two ends);
 *     + msgat_window_gather_imputed (the input windows with missing readings filled in and a validity channel);
 *     + msgat_quantile_{partial_doubles,metrics,grad} (quantile forecasts: pinball loss and coverage in the step tail);
 *     + msgat_edge_dropout{,_backward} (dropout on the stored edges, masks from a counter-based generator in device memory);
 *     + msgat_adam_step_averaged and msgat_param_swap (an exponential moving average of the weights inside the update);
 *     + msgat_gather_accumulate and msgat_gather_accumulate_dev (gradient accumulation over the micro-batches of a window);
 *     + msgat_edge_validity{,_backward} (edges gated by the validity of their source node's input window, per sample);
 *     + msgat_ring_push and msgat_ring_windows (online forecasting: a ring of readings and the windows of its newest origin);
 *     + msgat_forecast_store and msgat_forecast_score{,_partial_doubles} (online forecasts scored as their readings arrive);
 *     + msgat_interval_update and msgat_interval_apply (calibrated prediction intervals from the settled errors).
 * 9: msgat_graph_t.val_sets (new last field: one adjacency value set per sample of a batched adjacency);
 * + msgat_graph_edge_values.
 * 8: - msgat_stage_aggregate_project (no caller: msgat_gacn_forward runs that stage itself); nothing else changed.
 * 7 (round 6): + msgat_dense_scratch_bytes; msgat_fwd_t.dense_scratch (new last field); msgat_stage_scores and
 * msgat_stage_dense_column_pass take a dense_scratch pointer in front of the stream.  The one process-wide environment switch,
 * MSGAT_DENSE_SPLIT = 0 | 1, forces the arithmetic of the dense passes for A/B runs and tests (read once).
 * 6 (round 5): + msgat_contract_form_name, msgat_causal_conv{,_fused,_grad_weight}, msgat_layernorm_head_backward
 * {,_partial_floats}, msgat_head_forward_ln, msgat_gate_sum{,_backward}, msgat_layernorm_{forward,backward}_pooled, msgat_layernorm_pool_partial_floats,
 * msgat_contract_mix_partial_floats; no existing signature or structure changed since 5. */
#define MSGAT_ABI_VERSION 10

enum {
  MSGAT_OK = 0,
  MSGAT_ERR_NULL = -1,        /* a required pointer is NULL                         */
  MSGAT_ERR_SHAPE = -2,       /* a dimension is <= 0 or inconsistent                 */
  MSGAT_ERR_UNSUPPORTED = -3, /* T not in {4,8,12,16}, C/Co beyond the built limits  */
  MSGAT_ERR_WORKSPACE = -4,   /* workspace smaller than msgat_bwd_workspace_bytes()  */
  MSGAT_ERR_GRAPH = -5,       /* malformed CSR/CSC                                   */
  MSGAT_ERR_HIP_BASE = -1000  /* -1000 - hipError_t                                  */
};

/* How a GACN call orders aggregation and channel projection (they commute: the
 * aggregation acts on the node axis, W on the channel axis). */
enum {
  MSGAT_MODE_PLAIN = 0,   /* Co == 0: GraphAttention only (attention.py:32-36)               */
  MSGAT_MODE_AGG_FIRST = 1, /* C <= Co: aggregate C channels, then project (msgat.py order)  */
  MSGAT_MODE_PROJ_FIRST = 2 /* C >  Co: project to Co channels, then aggregate (3x less gather) */
};

/* Sliced ELLPACK form (SELL-64, rows sorted by degree) of one sparse structure -- the rows of the
 * CSR, or the columns of the CSC -- used by the aggregate / SDDMM kernels when an [N,T] slab does
 * not fit LDS (N > ~3400 at T = 12; the N = 8192 stress graph).  Those kernels keep ONE 4-timestep
 * column of a slab in LDS per pass, so the edge lists are re-read once per (group, channel, column):
 * several times the bytes of the features themselves, and through the CSR that is dependent round
 * trips of 16-B pieces at a ~68-B stride plus a dozen address instructions per edge.  Here the rows
 * are sorted by degree (descending, stable), cut into slices of 64 (one wavefront) and every slice
 * is padded to its largest degree rounded up to a multiple of 4 and stored in "trips" of 4 edges
 * per row, lane-interleaved:
 *     entry (slice s, k-th edge, lane l)  at position  slice_off[s] + 256 (k / 4) + 4 l + k % 4
 * so lane l reads its edges 4t .. 4t+3 with ONE coalesced 16-B-per-lane load per array (1 KiB per
 * wave instruction): no dependent address, no mask (padding entries carry coefficient 0).
 * Sorting makes the degrees inside a slice nearly equal, so the padding is a few percent.  WHICH of a row's
 * edges is its k-th is the builder's choice: it fills every column so that the 16 lanes a ds_read_b128
 * serves together gather from different LDS bank quads where the graph allows (a bipartite matching per
 * column; 11.5 -> 6.5 LDS cycles per gather instruction at the stress graph).
 * Built on the host by msgat_graph_sell_build().  n_slices == 0: absent (the CSR kernels run). */
#define MSGAT_SELL_SLACK 512 /* idx (and every per-position buffer) carries this many readable trailing entries */
typedef struct msgat_sell {
  int32_t n_slices;         /* ceil(N / 64), or 0 when the layout is absent                          */
  int32_t n_pos;            /* positions in total = slice_off[n_slices] (>= nnz: padding included)    */
  const int32_t* slice_off; /* [n_slices+1]  first position of each slice; width = difference / 64    */
  const int32_t* lane_row;  /* [64 n_slices] row handled by each lane of a slice, -1 past N           */
  const uint16_t* idx;      /* [n_pos+SLACK] neighbour node of each position (0 at padding); the layout
                               is only built for N <= 10176 (one float4 per node must fit LDS)         */
  const int32_t* src;       /* [n_pos]       position -> CSR edge index, -1 at padding                */
  const int32_t* pos;       /* [nnz]         CSR edge index -> position (row form only)               */
  int32_t prefer;           /* != 0: use the SELL kernels even when a whole slab fits LDS (tests)     */
  int32_t pair_trips;       /* max over i of trips(slice i) + trips(slice n_slices-1-i), a trip = 4
                               columns: the SDDMM keeps a wave's slice PAIR in registers when it fits    */
} msgat_sell_t;

/* Device-resident sparse adjacency.  Built on the host by msgat_graph_build() and copied
 * to the device by the caller. */
typedef struct msgat_graph {
  int32_t n_nodes;
  int32_t nnz;
  const int32_t* rowptr; /* [N+1]  CSR row starts                                   */
  const int32_t* col;    /* [nnz]  column of each CSR edge                          */
  const float* val;      /* [nnz]  adjacency weight of each CSR edge                */
  const int32_t* erow;   /* [nnz]  row of each CSR edge (COO companion of col)      */
  const int32_t* colptr; /* [N+1]  CSC column starts                                */
  const int32_t* crow;   /* [nnz]  row of each CSC entry                            */
  const int32_t* cperm;  /* [nnz]  CSC position -> CSR edge index                   */
  const int32_t* cpos;   /* [nnz]  CSR edge index -> CSC position (inverse of cperm): lets the forward leave the
                                   edge coefficients in CSC order too, so backward starts without a re-ordering pass */
  msgat_sell_t sell_rows; /* SELL of the CSR (forward aggregate, SDDMM); optional     */
  msgat_sell_t sell_cols; /* SELL of the CSC (transposed aggregate of backward); opt. */
  int32_t val_sets;       /* value sets behind `val`: 0 or 1 = one [nnz] set shared by every group; Bg or R*Bg = a
                             per-sample graph (adjacency [V,N,N], attention.py:22): `val` is [val_sets, nnz] and group g
                             reads set g % val_sets (g % Bg is the sample of the relation-major layout).  The structure
                             is the union of the samples' patterns; a sample without an edge of it carries 0 there */
} msgat_graph_t;

typedef struct msgat_shape {
  int32_t R;  /* relations (parameter sets)                      */
  int32_t Bg; /* groups per relation; G = R*Bg                    */
  int32_t C;  /* input channels                                   */
  int32_t Co; /* output channels of W; 0 = no projection (PLAIN)  */
  int32_t N;  /* nodes                                            */
  int32_t T;  /* timesteps (the score contraction axis)           */
} msgat_shape_t;

/* Forward buffers.  `need_bwd` != 0 makes the call fill everything backward needs. */
typedef struct msgat_fwd {
  const float* x;     /* in  [G,C,N,T]                                                    */
  const float* alpha; /* in  [R,C]        attention.py:30                                 */
  const float* Wg;    /* in  [R,T,T]      attention.py:29                                 */
  const float* W;     /* in  [R,Co,C]     msgat.py:23 (NULL iff Co == 0)                  */
  float* z;           /* out [G,Co,N,T]   (PLAIN: [G,C,N,T])                              */
  float* q;           /* out [G,N,T]      q = k = sum_c alpha_c x_c   (attention.py:33)   */
  float* kW;          /* out [G,N,T]      k @ Wg                      (attention.py:34)   */
  float* lse;         /* out [G,N]        row log-sum-exp of the scores in log2 units:
                             log2 sum_m 2^(S[n,m] log2 e); natural log = lse * ln 2        */
  float* pq;          /* out [G,N,T]      softmax(S) @ q, only written when need_bwd      */
  float* E;           /* out [G,nnz]      softmax(S)*adj at the edges (attention.py:36)   */
  float* u;           /* out AGG_FIRST: y [G,C,N,T] when need_bwd; PROJ_FIRST: W x [G,Co,N,T];
                             PLAIN: unused (may be NULL)                                  */
  int32_t need_bwd;
  float* edge_scratch; /* tmp msgat_edge_scratch_floats() floats (0 unless the graph carries a SELL
                             layout the aggregate will use: E re-ordered for it); may be NULL then */
  float* Ec;          /* out [G,nnz]      E in CSC order (Ec[g, cpos[e]] = E[g, e]), written by the score kernel
                             itself; optional (NULL: not written).  Hand it to msgat_bwd_t.Ec */
  void* dense_scratch; /* tmp msgat_dense_scratch_bytes() bytes, 256-byte aligned (0 for the PEMS-sized graphs: may be
                             NULL then): the operand images of the score pass on large graphs (ABI v7) */
} msgat_fwd_t;

typedef struct msgat_bwd {
  /* forward inputs and what forward saved */
  const float* x;
  const float* alpha;
  const float* Wg;
  const float* W;
  const float* q;
  const float* kW;
  const float* lse;
  const float* pq;
  const float* E;
  const float* u;
  /* incoming gradient, same shape as z; contiguous unless dz_group_channels says otherwise (below) */
  const float* dz;
  /* gradients out (overwritten, not accumulated) */
  float* dx;     /* [G,C,N,T]                       */
  float* dalpha; /* [R,C]                           */
  float* dWg;    /* [R,T,T]                         */
  float* dW;     /* [R,Co,C]   (NULL iff Co == 0)   */
  /* scratch, >= msgat_bwd_workspace_bytes() bytes, 256-byte aligned */
  void* workspace;
  size_t workspace_bytes;
  /* 0, or the channel count of the tensor dz is a channel slice of: group g of dz then starts at
   * dz + g * dz_group_channels * N * T (a gradient that arrives as dout[:, a:b] of a wider [G,C',N,T] tensor is read in
   * place instead of being copied).  Only where msgat_bwd_accepts_strided_dz() says so; 0 everywhere else. */
  int32_t dz_group_channels;
  /* E in CSC order as the forward left it (msgat_fwd_t.Ec); NULL: backward re-orders E itself (one more launch) */
  const float* Ec;
} msgat_bwd_t;

/* ---- library ------------------------------------------------------------------- */
int msgat_abi_version(void);
const char* msgat_status_string(int status);
/* MSGAT_MODE_* the library uses for (C, Co); the caller sizes `u` from it. */
int msgat_gacn_mode(int32_t C, int32_t Co);

/* ---- host: dense adjacency -> CSR/CSC ---------------------------------------------
 * Replaces the dense mask `att * adjacency` of attention.py:36 by its non-zeros.
 * `adj` is a HOST pointer to the row-major [n,n] fp32 matrix with leading dimension ld.
 * An entry is an edge iff it is != 0 (NaN counts as an edge). */
int msgat_graph_count(const float* adj, int32_t n, int64_t ld, int32_t* nnz_out);
int msgat_graph_build(const float* adj, int32_t n, int64_t ld, int32_t nnz,
                      int32_t* rowptr, int32_t* col, float* val, int32_t* erow,
                      int32_t* colptr, int32_t* crow, int32_t* cperm, int32_t* cpos);
/* The same structure from the CSR index arrays of a sparse [n,n] adjacency (HOST pointers): in_rowptr [n+1], in_col
 * [nnz], columns in any order inside a row.  Every stored index is an edge, whatever its value.  The output arrays are
 * those of msgat_graph_build() except `val`, which the caller points at its values in library order: order [nnz] maps
 * the library's CSR edge k (columns ascending inside a row) to its position in the input, order[k] = input index.
 * Never touches [n,n].  A decreasing in_rowptr, in_rowptr[0] != 0 or in_rowptr[n] != nnz, a column outside [0,n) or a
 * column stored twice in a row is MSGAT_ERR_GRAPH; n <= 0 or nnz < 0 is MSGAT_ERR_SHAPE. */
int msgat_graph_build_indices(const int32_t* in_rowptr, const int32_t* in_col, int32_t n, int32_t nnz,
                              int32_t* rowptr, int32_t* col, int32_t* erow, int32_t* colptr, int32_t* crow,
                              int32_t* cperm, int32_t* cpos, int32_t* order);
/* Host-side structural check of a (host-resident) graph (its SELL forms too, when present). */
int msgat_graph_validate(const msgat_graph_t* host_graph);
/* SELL form of a CSR (ptr = rowptr, idx = col, perm = NULL) or CSC (ptr = colptr, idx = crow,
 * perm = cperm) structure, all HOST pointers: first the sizes, then the arrays (see msgat_sell_t;
 * spos may be NULL; sidx must have n_pos + MSGAT_SELL_SLACK entries; n <= 65535).  Pure index work: replaces
 * nothing in the reference, it re-orders the non-zeros of the mask of attention.py:36 for
 * coalesced reads. */
int msgat_graph_sell_count(const int32_t* ptr, int32_t n, int32_t* n_slices_out, int32_t* n_pos_out,
                           int32_t* pair_trips_out);
int msgat_graph_sell_build(const int32_t* ptr, const int32_t* idx, const int32_t* perm, int32_t n,
                           int32_t nnz, int32_t n_slices, int32_t n_pos, int32_t* slice_off,
                           int32_t* lane_row, uint16_t* sidx, int32_t* ssrc, int32_t* spos);

/* Values of a batched adjacency on a shared structure (device pointers): vals[v, e] = dense[v, erow_e, col_e] for the
 * n_sets contiguous [N,N] fp32 matrices of `dense` and the CSR (rowptr, col) of `graph`; the non-zeros of `dense` that
 * lie outside the structure (`!(x == 0)`: NaN counts) are ADDED to *outside (device int32).  One pass over the dense
 * tensor, nothing read back: capturable in a HIP graph.  vals holds n_sets * nnz floats. */
int msgat_graph_edge_values(const msgat_graph_t* graph, const float* dense, int32_t n_sets, float* vals,
                            int32_t* outside, void* stream);

/* ---- device: fused entry points --------------------------------------------------
 * msgat_gacn_forward replaces attention.py:33-36 (+ msgat.py:27-28 when Co > 0).
 * msgat_gacn_backward replaces the autograd of those lines for x, alpha, Wg and W; the adjacency's own gradient, when it
 * requires one, is msgat_adjacency_grad (below), enqueued after it. */
size_t msgat_edge_scratch_floats(const msgat_shape_t* shape, const msgat_graph_t* graph);
/* Scratch of the two dense passes over all N columns of a row (the softmax denominator of attention.py:34 and its
 * backward).  From N = 1536 nodes (T = 12) they run on the bf16 / fp16 matrix core with every fp32 operand split into
 * bf16 / fp16 terms (fp32 accuracy, fp32 accumulate) and first write those operand "images" here; 0 below that.
 * msgat_gacn_backward / msgat_attention_backward carry their share inside their workspace. */
size_t msgat_dense_scratch_bytes(const msgat_shape_t* shape);
int msgat_gacn_forward(const msgat_shape_t* shape, const msgat_graph_t* graph,
                       const msgat_fwd_t* io, void* stream);
size_t msgat_bwd_workspace_bytes(const msgat_shape_t* shape, const msgat_graph_t* graph);
/* 1 when msgat_gacn_backward reads a channel-sliced dz in place for this shape and graph (dz_group_channels), 0 when
 * the caller must pass a contiguous copy. */
int msgat_bwd_accepts_strided_dz(const msgat_shape_t* shape, const msgat_graph_t* graph);
int msgat_gacn_backward(const msgat_shape_t* shape, const msgat_graph_t* graph,
                        const msgat_bwd_t* io, void* stream);

/* ---- device: gradient of the adjacency (attention.py:36 with an adjacency that requires grad) ----
 *   dadj[v,n,m] = sum_{g : g % n_sets == v} P_g[n,m] H_g[n,m],   H_g[n,m] = sum_{c < Cu, t} dv[g,c,n,t] feat[g,c,m,t]
 *   P_g = 2^(S_g[n,m] log2 e - lse_g[n]),  S_g = kW_g q_g^T:  the softmax over ALL N columns, before the mask.
 * P does not depend on the adjacency, so dadj is DENSE: written for every (n, m), edge or not (no graph argument).
 * q, kW, lse [G,N,T] / [G,N] are what the forward saved.  dv / feat / Cu by path: PLAIN dz / x / C; PROJ_FIRST dz / u = W x
 * / Co; AGG_FIRST W^T dz (msgat_stage_mix) / x / C; the attention core dv / u / Cu.  dv_group_channels: 0 (contiguous) or the
 * channel count of the wider tensor dv is a channel slice of, as msgat_bwd_t.dz_group_channels.  n_sets: 1 (one [N,N]
 * adjacency, summed over all G groups), Bg ([Bg,N,N]: sample b shared by its R relations) or R*Bg (one per group) --
 * the convention of msgat_graph_t.val_sets; dadj is [n_sets,N,N].  shape->C / Co are those of the call (only checked).
 * Deterministic (a fixed order of additions, no atomics); nothing is read back, so it may be captured in a HIP graph.
 * workspace: msgat_adjacency_grad_workspace_bytes() bytes, 256-byte aligned (the per-split partial sums; may be 0).
 * T in {4,8,12,16} and Cu <= 256, else MSGAT_ERR_UNSUPPORTED; a bad n_sets or Cu <= 0 is MSGAT_ERR_SHAPE. */
size_t msgat_adjacency_grad_workspace_bytes(const msgat_shape_t* shape, int32_t Cu, int32_t n_sets);
int msgat_adjacency_grad(const msgat_shape_t* shape, int32_t Cu, const float* dv, int32_t dv_group_channels,
                         const float* feat, const float* q, const float* kW, const float* lse, int32_t n_sets, float* dadj,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- device: gradient of the stored values of a sparse adjacency (a learned weight per existing edge) ----
 *   dval[e] = sum_g P_g[n_e,m_e] H_g[n_e,m_e]   for the CSR edges e of `graph` (erow, col), in CSR order
 * the dense gradient of msgat_adjacency_grad restricted to the structure's edges (one value set: the adjacency is one
 * [N,N] matrix, summed over all G groups).  Nothing [N,N] is read or written: P is re-created at each edge from q, kW and
 * lse.  dv / dv_group_channels / feat / Cu exactly as for msgat_adjacency_grad.  The graph's `val` is not read.
 * Deterministic (a fixed order of additions, no atomics); nothing is read back, so it may be captured in a HIP graph.
 * workspace: msgat_edge_weight_grad_workspace_bytes() bytes, 256-byte aligned (the per-split partial sums; may be 0).
 * T in {4,8,12,16} and Cu <= 256, else MSGAT_ERR_UNSUPPORTED; Cu <= 0 or graph->n_nodes != N is MSGAT_ERR_SHAPE.
 * A graph without edges launches nothing. */
size_t msgat_edge_weight_grad_workspace_bytes(const msgat_shape_t* shape, const msgat_graph_t* graph, int32_t Cu);
int msgat_edge_weight_grad(const msgat_shape_t* shape, const msgat_graph_t* graph, int32_t Cu, const float* dv,
                           int32_t dv_group_channels, const float* feat, const float* q, const float* kW,
                           const float* lse, float* dval, void* workspace, size_t workspace_bytes, void* stream);

/* ---- device: gradient of the stored values of a per-sample sparse adjacency (one structure, n_sets value sets) ----
 *   dval[v,e] = sum_{g : g % n_sets == v} P_g[n_e,m_e] (H_g[n_e,m_e] + dE_extra[g,e])   for the CSR edges e, in CSR order
 * msgat_edge_weight_grad with the sum over the groups cut at the value sets of msgat_graph_t.val_sets: n_sets = Bg (sample
 * b's values are shared by its R relations, whose gradients add in ascending g) or R*Bg (one set per group); n_sets = 1
 * is msgat_edge_weight_grad followed by msgat_edge_softmax_grad.  dval is [n_sets,nnz].  dv / dv_group_channels / feat /
 * Cu exactly as for msgat_edge_weight_grad.  dE_extra [G,nnz] (CSR order) or NULL: the gradient arriving at the returned
 * attention weights (msgat_*_backward_edge_grad), whose share P_g dE_extra is added here, where P is formed anyway.  P is
 * re-created with the forward's score sum, not as E / A (explicit zeros).  The graph's `val` is not read.
 * Deterministic: every (v,e) has one owner that adds its groups in ascending order, no atomics; nothing is read back, so
 * it may be captured in a HIP graph.  workspace: msgat_edge_weight_grad_sets_workspace_bytes() bytes, 256-byte aligned
 * (0 unless n_sets = 1).  T in {4,8,12,16} and Cu <= 256, else MSGAT_ERR_UNSUPPORTED; n_sets not in {1, Bg, R*Bg}, Cu <= 0
 * or graph->n_nodes != N is MSGAT_ERR_SHAPE.  A graph without edges launches nothing. */
size_t msgat_edge_weight_grad_sets_workspace_bytes(const msgat_shape_t* shape, const msgat_graph_t* graph, int32_t Cu,
                                                   int32_t n_sets);
int msgat_edge_weight_grad_sets(const msgat_shape_t* shape, const msgat_graph_t* graph, int32_t Cu, const float* dv,
                                int32_t dv_group_channels, const float* feat, const float* q, const float* kW,
                                const float* lse, const float* dE_extra, int32_t n_sets, float* dval, void* workspace,
                                size_t workspace_bytes, void* stream);

/* ---- device: reading the attention (attention.py:34 `att`, :36 `att * adjacency`) ----
 * msgat_attention_map:  out[g,n,m] = P_g[n,m] = 2^(S_g[n,m] log2 e - lse_g[n]),  S_g = kW_g q_g^T, for every (n, m) of
 *   every group g < R*Bg: the dense row softmax over all N columns, before the mask.  out [G,N,N] fp32, row-major,
 *   4 G N^2 bytes (17 GB at G = 64, N = 8192: the caller sizes its batch).  q, kW [G,N,T] and lse [G,N] are what a
 *   forward saved (msgat_fwd_t, or msgat_stage_scores with the caller's q).  S is the forward's k-ordered fp32 chain on
 *   v_mfma_f32_16x16x4_f32 (k_adjacency_grad's); from N = 1536 the forward forms lse with split operands
 *   (msgat_dense_scratch_bytes), whose scores agree with it to fp32 rounding: rows sum to 1 within fp32 accuracy either
 *   way.  Deterministic; nothing is read back, so it may be captured in a HIP graph.  Needs N*N < 2^31.
 * msgat_gacn_backward_edge_grad / msgat_attention_backward_edge_grad: msgat_gacn_backward / msgat_attention_backward with
 *   an extra gradient dE_extra [G,nnz] (CSR order) arriving at E = softmax(S) (.) A itself -- a loss on the returned
 *   weights.  It is added where g_e = E_e dE_e is formed, g_e = E_e (dE_e + dE_extra_e), and everything downstream (delta,
 *   the dense column correction, dWg, dq, dx / du, dalpha, dW) follows from g as before.  dE_extra = NULL is exactly the
 *   function without the suffix (the same launches).  Deterministic and capturable as those.
 * msgat_edge_softmax_grad:  the adjacency's share of that extra gradient, ADDED to what msgat_adjacency_grad /
 *   msgat_edge_weight_grad wrote (enqueue it after them on the same stream):
 *     dadj[v, erow_e, col_e] += sum_{g % n_sets == v} P_g[e] dE_extra[g,e]     (dense [n_sets,N,N]; dval == NULL), or
 *     dval[e]                += sum_g P_g[e] dE_extra[g,e]                     (sparse values [nnz], CSR order; n_sets 1)
 *   for the CSR edges e of `graph`; exactly one of dadj / dval is given.  P_g[e] is re-created from q, kW and lse with the
 *   score sum of msgat_edge_weight_grad (not as E / A, which fails at explicit zeros).  One lane per (edge, set) sums its
 *   groups in ascending order: deterministic, no atomics, nothing read back.  n_sets as for msgat_adjacency_grad.
 * T in {4,8,12,16}, else MSGAT_ERR_UNSUPPORTED. */
int msgat_attention_map(const msgat_shape_t* shape, const float* q, const float* kW, const float* lse, float* out,
                        void* stream);
int msgat_gacn_backward_edge_grad(const msgat_shape_t* shape, const msgat_graph_t* graph, const msgat_bwd_t* io,
                                  const float* dE_extra, void* stream);
int msgat_attention_backward_edge_grad(const msgat_shape_t* shape, const msgat_graph_t* graph, const float* u,
                                       const float* dv, int32_t dv_group_channels, const float* q, const float* kW,
                                       const float* lse, const float* pq, const float* E, const float* Ec,
                                       const float* Wg, float* du, float* dq, float* dWg, void* workspace,
                                       size_t workspace_bytes, const float* dE_extra, void* stream);
int msgat_edge_softmax_grad(const msgat_shape_t* shape, const msgat_graph_t* graph, const float* q, const float* kW,
                            const float* lse, const float* dE_extra, int32_t n_sets, float* dadj, float* dval,
                            void* stream);

/* ---- device: a gradient that arrives at the dense softmax map (attention.py:34 `att` as an autograd tensor) ----
 * msgat_softmax_map_grad:  given dP [G,N,N] fp32 row-major, the gradient at P = msgat_attention_map's output,
 *     r[n]  = sum_m P[n,m] dP[n,m]          dS = P (.) (dP - r)          dkW = dS q
 *     dq_add[g,n,:]  += (dS^T kW + dkW Wg^T)[n,:]            ([G,N,T])
 *     dWg_add[rel]   += sum_{g in rel} q_g^T dkW_g            ([R,T,T]; relation rel owns the groups rel*Bg .. rel*Bg+Bg-1)
 *   both ADDED to what the buffers hold (zero them, or enqueue this after the backward that wrote them); both targets are
 *   required.  `att` depends neither on the projection W nor on the adjacency, so nothing else receives a
 *   share.  q, kW [G,N,T], lse [G,N] are what the forward saved, Wg [R,T,T] its parameter.  P is never stored: two passes
 *   re-create it per 16 x 16 tile with msgat_attention_map's k-ordered fp32 chain on v_mfma_f32_16x16x4_f32 (at every N,
 *   also where the forward formed lse with split operands) and form their products with q / kW on the matrix core; dP
 *   is read twice (once along rows for r and dkW, once for the column product), 8 G N^2 bytes in all.  sum_m P q is
 *   recomputed from the same P, not taken from the forward's pq, so that dS sums to zero along a row with the P in use.
 *   Deterministic: every output element has one owner that adds in a fixed order, no atomics; repeated runs are
 *   bit-identical.  Nothing is read back, so it may be captured in a HIP graph.  workspace:
 *   msgat_softmax_map_grad_workspace_bytes() bytes (dkW, r and the dWg partials), 256-byte aligned.
 *   Wg and dq_add are read / updated in 16-byte pieces and must be 16-byte aligned, else MSGAT_ERR_SHAPE (dP is read in
 *   16-byte pieces when it is so aligned and N % 4 == 0, in 4-byte pieces otherwise; q, kW, lse need 4 bytes).
 *   T in {4,8,12,16} and N*N < 2^31, else MSGAT_ERR_UNSUPPORTED; a short or misaligned workspace is MSGAT_ERR_WORKSPACE.
 * msgat_gacn_backward_map_grad:  msgat_gacn_backward with dq_map [G,N,T] and dWg_map [R,T,T], both required,
 *   the two outputs of msgat_softmax_map_grad on zeroed buffers: dq_map is added to the pooled signal's gradient where the
 *   dense column pass has finished it, so that dx and dalpha carry it, dWg_map to dWg after its reduction.  The backward
 *   is linear in its upstream gradients: no existing kernel changes.  The dense map is a weights form of its own, so no
 *   edge gradient dE_extra arrives together with it.  For the attention core dq and dWg are outputs of msgat_attention_backward: enqueue
 *   msgat_softmax_map_grad on them afterwards. */
size_t msgat_softmax_map_grad_workspace_bytes(const msgat_shape_t* shape);
int msgat_softmax_map_grad(const msgat_shape_t* shape, const float* q, const float* kW, const float* lse, const float* Wg,
                           const float* dP, float* dq_add, float* dWg_add, void* workspace, size_t workspace_bytes,
                           void* stream);
int msgat_gacn_backward_map_grad(const msgat_shape_t* shape, const msgat_graph_t* graph, const msgat_bwd_t* io,
                                 const float* dq_map, const float* dWg_map, void* stream);

/* ---- device: the individual stages (exposed for tests, profiling and bench.py) ----
 * Each is what the fused entry points enqueue, in order. */

/* attention.py:33 (and msgat.py:27 when projecting first): q = sum_c alpha_c x_c and,
 * if u != NULL, u[g,o] = sum_c W[r,o,c] x[g,c]. */
int msgat_stage_project(const msgat_shape_t* shape, const float* x, const float* alpha,
                        const float* W, float* q, float* u, void* stream);
/* attention.py:34 + the edge part of :36: kW = q Wg, lse = row log-sum-exp over ALL N
 * columns of kW q^T (log2 units), pq = softmax @ q (optional), E = softmax * adj at the edges (Ec, optional: the
 * same values in CSC order).  dense_scratch: msgat_dense_scratch_bytes() bytes (NULL when that is 0). */
int msgat_stage_scores(const msgat_shape_t* shape, const msgat_graph_t* graph,
                       const float* q, const float* Wg, float* kW, float* lse, float* pq,
                       float* E, float* Ec, void* dense_scratch, void* stream);
/* attention.py:36: v[g,c,n,:] = sum_{e in row n} E[g,e] u[g,c,col_e,:] over Cu channels.
 * edge_scratch: msgat_edge_scratch_floats() floats (NULL when that is 0). */
int msgat_stage_aggregate(const msgat_shape_t* shape, const msgat_graph_t* graph,
                          int32_t Cu, const float* u, const float* E, float* v, float* edge_scratch,
                          void* stream);

/* The dense column pass of the backward (autograd of the softmax of attention.py:34): given the row sums
 * delta[G,N] of the edge gradients and the edge gradients gE[G,nnz] (CSR order),
 *     dq[g,m,:] += sum_{e -> m} gE_e kW[row_e,:] - sum_n P[n,m] delta[n] kW[n,:],   P = 2^(S log2e - lse)
 * re-creating P with the forward's operands and k order (bit-identical to the forward's).  dq is updated in place.
 * dense_scratch: msgat_dense_scratch_bytes() bytes (NULL when that is 0). */
int msgat_stage_dense_column_pass(const msgat_shape_t* shape, const msgat_graph_t* graph, const float* q,
                                  const float* kW, const float* lse, const float* delta, const float* gE,
                                  float* dq, void* dense_scratch, void* stream);

/* Backward building blocks (also what msgat_gacn_backward enqueues).
 * msgat_stage_mix:      out[g,co,p] = sum_ci M[r,..] in[g,ci,p] (+ addvec[r,co] extra[g,p]);
 *                       M is [R,Co,Ci] (m_in_major = 0) or [R,Ci,Co] (m_in_major = 1, i.e. W^T applied).
 *                       P = N*T positions.  dy = W^T dz and dx = W^T du + alpha (x) dq use it.
 * msgat_stage_contract: dst[r,a,c] = sum_{g in r, p} A[g,a,p] B[g,c,p]; if Aextra != NULL it supplies
 *                       row a = Ca-1 (shape [G,P]) and A holds the other Ca-1 rows.  The first n0
 *                       outputs of a relation go to dst0, the next n1 to dst1 (dW and dalpha).
 *                       `partials` needs msgat_contract_partial_floats() floats. */
int msgat_stage_mix(const msgat_shape_t* shape, int32_t Ci, int32_t Co, const float* in, const float* M,
                    int32_t m_in_major, const float* addvec, const float* extra, float* out, void* stream);
size_t msgat_contract_partial_floats(const msgat_shape_t* shape, int32_t Ca, int32_t Cb);
int msgat_stage_contract(const msgat_shape_t* shape, int32_t Ca, int32_t Cb, const float* A,
                         const float* Aextra, const float* B, float* partials, float* dst0, int32_t n0,
                         float* dst1, int32_t n1, void* stream);
/* msgat_stage_project_backward: the last stage of the PROJ_FIRST backward as msgat_gacn_backward enqueues it --
 *   dW[r,o,c] = sum du[g,o,p] x[g,c,p],  dalpha[r,c] = sum dq[g,p] x[g,c,p],  dx = W^T du + alpha (x) dq
 * (the autograd of msgat.py:27 and attention.py:33) in ONE pass over du, dq and x where the shape has a fused form,
 * as msgat_stage_contract + msgat_stage_mix otherwise.  partials: msgat_contract_partial_floats(shape, Co + 1, C). */
int msgat_stage_project_backward(const msgat_shape_t* shape, const float* du, const float* dq, const float* x,
                                 const float* W, const float* alpha, float* partials, float* dW, float* dalpha,
                                 float* dx, void* stream);

/* ---- device: the producer of every GACN input -- LayerNorm over the timestep axis ----
 * Replaces nn.LayerNorm([n_timesteps]) of the callers (src/models/msgat.py:114 applied at :122,
 * :152 applied at :158): x is [rows, T] contiguous (rows = B*C*N), weight / bias are [T] or NULL
 * (identity), eps as torch's (1e-5 in the reference), biased variance.
 * Backward re-derives mean / rstd from x (nothing is saved but x): dx [rows,T], dweight / dbias [T]
 * (either may be NULL) summed in a fixed order through `partials`
 * (msgat_layernorm_partial_floats() floats).  dx_add (may be NULL) is added to dx in the same pass: the
 * gradient that reached x along its other path -- MEAM's residual convolution reads the block input too
 * (msgat.py:130) -- so autograd's separate accumulation pass over the activation disappears.
 * relu_mask != 0: x is the output of a ReLU (MEAM's tail, msgat.py:131) whose backward is applied here,
 * dx = 0 where x <= 0, instead of in a pass of its own (the caller then skips that ReLU's own mask).
 * T in {4, 8, 12, 16}.
 *
 * R ("relations") in this and the following entry points: the number of parameter sets evaluated in one
 * launch.  The reference loops over its components (src/models/msgat.py:204), each with its own weights;
 * here the components ride on the leading (batch) axis, relation-major -- rows / slabs / groups of relation r
 * are contiguous and R divides their count -- and every parameter gets a leading [R] axis (weight [R,T],
 * w [R,N], bias [R,Co], W [R,T_out,T,1,C]).  R = 1 is the single-module case. */
int msgat_layernorm_forward(const float* x, const float* weight, const float* bias, float* y,
                            int64_t rows, int32_t T, float eps, int32_t R, void* stream);
size_t msgat_layernorm_partial_floats(int64_t rows, int32_t T, int32_t R);
int msgat_layernorm_backward(const float* x, const float* weight, const float* dy, const float* dx_add,
                             float* dx, float* dweight, float* dbias, float* partials, int64_t rows,
                             int32_t T, float eps, int32_t R, int32_t relu_mask, void* stream);
/* msgat_layernorm_forward_pooled: msgat_layernorm_forward that also leaves the node pooling of its OUTPUT,
 * pooled[s,t] = sum_n pool_w[n] y[s,n,t] over y's [N,T] slabs (ChannelAttention's pooled signal, attention.py:89, on MEAM's
 * normalised input, msgat.py:122-125): a wave's 64 rows lie in at most two slabs (N >= 64, else MSGAT_ERR_UNSUPPORTED), every
 * 64-row trip leaves its share of both and a small second launch adds a slab's shares in trip order -- instead of
 * msgat_node_pool reading back the tensor that was just written.  pool_w [R,N], pooled [rows / N, T];
 * partials: msgat_layernorm_pool_partial_floats(rows, T, R) floats. */
size_t msgat_layernorm_pool_partial_floats(int64_t rows, int32_t T, int32_t R);
int msgat_layernorm_forward_pooled(const float* x, const float* weight, const float* bias, float* y, const float* pool_w,
                                   int32_t N, float* pooled, float* partials, int64_t rows, int32_t T, float eps, int32_t R,
                                   void* stream);
/* msgat_layernorm_backward_pooled: msgat_layernorm_backward for a LayerNorm whose output y [.., N, T] ALSO fed a node
 * pooling p[s,t] = sum_n pool_w[n] y[s,n,t] over its [N,T] slabs (ChannelAttention's pooled signal, attention.py:89, taken
 * of MEAM's normalised input, msgat.py:122-125): that consumer's gradient pool_w[n] dpooled[s,t] is rank one and is added
 * to dy row by row inside this pass, instead of by msgat_node_pool_grad_signal in a pass of its own over the activation.
 * pool_w [R,N] (one set per relation), dpooled [rows / N, T]; everything else as msgat_layernorm_backward.
 * dpool_w [R,N] (optional, with dpool_rows: `rows` floats of scratch): the pooling weights' gradient
 * sum_s y[s,n,:] . dpooled[s,:] out of the same pass (y is rebuilt from x, weight and `bias`, the LayerNorm's own), instead
 * of msgat_node_pool_grad_weight's pass over the stored y. */
int msgat_layernorm_backward_pooled(const float* x, const float* weight, const float* bias, const float* dy,
                                    const float* dx_add, const float* pool_w, const float* dpooled, int32_t N, float* dx,
                                    float* dweight, float* dbias, float* dpool_w, float* dpool_rows, float* partials,
                                    int64_t rows, int32_t T, float eps, int32_t R, int32_t relu_mask, void* stream);

/* ---- device: the temporal and channel branches of MEAM ----
 * Building blocks for TACN (src/models/msgat.py:57-80, TemporalAttention attention.py:58-66) and CACN
 * (msgat.py:83-100, ChannelAttention attention.py:88-94) and for the block's residual tail
 * (msgat.py:130-131).  The tiny [T,T] / [C,C] attention matrices are built by the caller from the
 * pooled signals; these entry points are the passes over the [B,C,N,T] activations.
 *
 * msgat_stage_mix_epilogue: msgat_stage_mix plus out = relu?(... + bias[r*bias_per_relation*Co + co]
 *     + add[g,co,p]): a 1x1 convolution with bias when R = 1; a per-sample matrix (CACN's
 *     Wconv att_b) when R = batch, Bg = 1; the residual tail relu(cat(branches) + res(x)) with `add`.
 * msgat_time_mix: forward (backward = 0)
 *         dst[g,o,n,t] = bias[o] + sum_k sum_i A[ga,k,t,i] src[g,k*Co+o,n,i]      src [G,K*Co,N,T]
 *     backward (backward = 1): dst[g,k*Co+o,n,i] = sum_t A[ga,k,t,i] src[g,o,n,t]  src [G,Co,N,T]
 *     A is [G,K,T,T] (a_per_group = 1) or [K,T,T] shared; K in {1, 2}.  With A_1 = att_b and
 *     A_0 = att_b shifted down by the dilation this is conv_[1,2],dilated(TemporalAttention(x)) after the
 *     channel mixing src = [W_0; W_1] x; with constant shift matrices it is a plain causal convolution.
 * msgat_time_mix_grad_matrix: dA[g,k,t,i] = sum_{o,n} dout[g,o,n,t] y[g,k*Co+o,n,i];
 *     `partials` needs msgat_time_mix_partial_floats() floats.
 * Gradients arriving as channel slices [:, a:b] of a wider contiguous [G, group_stride, N, T] tensor (the block's
 * concatenated gradient) are read in place: src_group_stride / dout_group_stride / (channels, group_stride) name the
 * wider tensor's channel count (0 = the operand is contiguous by itself).
 * msgat_node_pool: pooled[s,t] = sum_n w[n] x[s,n,t] over `slabs` (sample, channel) slabs (attention.py:89);
 *     msgat_node_pool_grad_signal: dx[s,n,t] = w[n] dpooled[s,t] (+ dx_add[s,n,t] when given: the gradient that
 *     reached x along its other path, so autograd's separate accumulation pass over the activation disappears);
 *     msgat_node_pool_grad_weight: dw[n] = sum_{g,c,t} x[g,c,n,t] dpooled[g,c,t] (partials:
 *     msgat_node_pool_partial_floats()).
 * The channel pooling sum_c alpha_c x[b,c] (attention.py:59) is msgat_stage_project with W = u = NULL. */
int msgat_stage_mix_epilogue(const msgat_shape_t* shape, int32_t Ci, int32_t Co, const float* in, const float* M,
                             int32_t m_in_major, const float* bias, int32_t bias_per_relation, const float* add,
                             int32_t relu, float* out, void* stream);
int msgat_time_mix(const float* src, const float* A, int32_t a_per_group, const float* bias, float* dst,
                   int32_t G, int32_t Co, int32_t K, int32_t N, int32_t T, int32_t backward, int32_t R,
                   int32_t src_group_stride, void* stream);
size_t msgat_time_mix_partial_floats(int32_t G, int32_t K, int32_t T);
/* msgat_causal_conv: a causal dilated [1,2] convolution -- nn.Conv2d(Ci, Co, [1,2], padding=[0,d], dilation=[1,d])
 * followed by Chomp(d), msgat.py:69-74: every TACN layer after the first -- in ONE pass over its input, with
 * taps [R, 2*Co, Ci] = [W0; W1] (W0 acts on in[t-d], W1 on in[t]; model.TACN.stacked_taps):
 *   backward = 0:  dst[g,co,n,t] = bias[co] + sum_ci W0[co,ci] src[g,ci,n,t-d] + W1[co,ci] src[g,ci,n,t]   src [G,Ci,N,T]
 *   backward = 1:  dst[g,ci,n,t] = sum_co W0[co,ci] src[g,co,n,t+d] + W1[co,ci] src[g,co,n,t]              src [G,Co,N,T]
 * (terms whose timestep falls outside [0,T) are zero).  It replaces msgat_mix_segments (Ci -> 2*Co), the [G,2*Co,N,T]
 * intermediate and msgat_time_mix with constant shift matrices: the shifted operand is an unaligned 16-byte load of
 * the same row of T plus a per-lane element mask.  bias [Co] or (bias_per_relation) [R,Co], forward only.
 * src_group_stride: src is a channel slice of a [G, src_group_stride, N, T] tensor (0: contiguous by itself).
 * msgat_causal_conv_fused(Ci, Co) = 1 when both directions have a one-pass form for these widths (else the entry point
 * returns MSGAT_ERR_UNSUPPORTED and the caller runs the two passes). */
/* msgat_causal_conv_grad_weight: dtaps[r, k*Co + co, ci] = sum_{g in r, n, t} dout[g,co,n,t + (k == 0 ? d : 0)] h[g,ci,n,t]
 * ([R, 2*Co, Ci + with_ones]; with_ones: column Ci = the sums of the gradient rows, whose tap-1 half [Co, 2*Co) is the
 * bias gradient) -- the gradient rows [dout[t+d]; dout] are virtual (time-shifted reads of dout inside the contraction's
 * staging loads), nothing [G,2*Co,N,T] is written.  partials: msgat_contract_segments_partial_floats(R, 2*Co, Ci + with_ones).
 * dout may be a channel slice of a [G, dout_group_stride, N, T] tensor (0: contiguous). */
int msgat_causal_conv_grad_weight(const float* dout, int32_t dout_group_stride, const float* h, float* partials, float* dtaps,
                                  int32_t R, int32_t Bg, int32_t Ci, int32_t Co, int32_t N, int32_t T, int32_t dilation,
                                  int32_t with_ones, void* stream);
int msgat_causal_conv_fused(int32_t Ci, int32_t Co);
int msgat_causal_conv(const float* src, const float* taps, const float* bias, int32_t bias_per_relation, float* dst,
                      int32_t R, int32_t Bg, int32_t Ci, int32_t Co, int32_t N, int32_t T, int32_t dilation,
                      int32_t backward, int32_t src_group_stride, void* stream);

int msgat_time_mix_grad_matrix(const float* dout, const float* y, float* dA, float* partials, int32_t G,
                               int32_t Co, int32_t K, int32_t N, int32_t T, int32_t dout_group_stride, void* stream);
int msgat_node_pool(const float* x, const float* w, float* pooled, int64_t slabs, int32_t N, int32_t T,
                    int32_t R, int32_t channels, int32_t group_stride, void* stream);
int msgat_node_pool_grad_signal(const float* w, const float* dpooled, const float* dx_add, float* dx,
                                int64_t slabs, int32_t N, int32_t T, int32_t R, void* stream);
size_t msgat_node_pool_partial_floats(int32_t G, int32_t C, int32_t N);
int msgat_node_pool_grad_weight(const float* x, const float* dpooled, float* dw, float* partials, int32_t G,
                                int32_t C, int32_t N, int32_t T, int32_t R, void* stream);

/* ---- device: channel axes assembled from several tensors ("segments") ----
 * A segment is `channels` channels of a [G, group_stride, N, T] tensor starting at `ptr` (group_stride = 0
 * means `channels`: the whole tensor; a larger value makes it a channel slice of a wider tensor).  The
 * segments of a list are concatenated along the channel axis -- without a concatenation pass:
 *   msgat_mix_segments:      out_segments = relu?(M cat(in_segments) + bias + cat(add_segments)); M is
 *       [R, Co_total, Ci_total] (or [R, Ci_total, Co_total] when m_in_major).  One pass reads cat(...) and
 *       writes each output range to its own tensor: MEAM's tail (msgat.py:123-131) without the cat, and all
 *       channel mixings of one activation (CACN's per-sample matrix, TACN's first convolution, GACN's
 *       projection and the two alpha poolings) in ONE pass; m_in_major = 1 is its backward (one dx).
 *   msgat_contract_segments: dst[r,a,c] = sum_{g in r, p} cat(A_segments)[g,a,p] B[g,c,p]; with_ones = 1 appends a
 *       virtual channel of ones to B: dst is [R, Ca, Cb+1] and dst[r,a,Cb] = sum_{g,p} A[g,a,p] -- the bias gradient of
 *       a 1x1 convolution out of the pass that computes its weight gradient (size the partials for Cb+1).
 *       with_ones = 2 (ABI 6; also msgat_contract_mix_segments and msgat_causal_conv_grad_weight): the same sums delivered
 *       apart -- dst holds the plain [R, Ca, Cb] matrix followed by the ones column as [R, Ca], R*Ca*(Cb+1) floats in all
 *       -- so weight and bias gradient are two contiguous tensors without a copy each.
 * At most 6 segments per list. */
typedef struct {
  float* ptr;
  int32_t channels;
  int32_t group_stride;
} msgat_seg_t;
int msgat_mix_segments(int32_t R, int32_t Bg, int32_t N, int32_t T, const msgat_seg_t* in, int32_t n_in,
                       const float* M, int32_t m_in_major, const float* bias, int32_t bias_per_relation,
                       const msgat_seg_t* add, int32_t n_add, int32_t relu, const msgat_seg_t* out,
                       int32_t n_out, void* stream);
size_t msgat_contract_segments_partial_floats(int32_t R, int32_t Ca, int32_t Cb);
int msgat_contract_segments(int32_t R, int32_t Bg, int32_t N, int32_t T, const msgat_seg_t* A, int32_t n_a,
                            const float* B, int32_t Cb, int32_t with_ones, float* partials, float* dst, void* stream);
/* msgat_contract_mix_segments: the whole backward of a 1x1 convolution y = M x (+ bias) in ONE pass over its
 * operands -- the autograd of the reference's nn.Conv2d(kernel_size=1) / GACN projection calls, msgat.py:27,63-66,
 * 92,116.  With A = cat(A_segments) the gradient at y [G,Ca,N,T], B = x [G,Cb,N,T], M [R,Ca,Cb]:
 *   dst[r,a,c]     = sum_{g in r, p} A[g,a,p] B[g,c,p]      (dM; with_ones: column Cb = sum A, the bias gradient)
 *   mixout[g,c,p]  = sum_a M[r,a,c] A[g,a,p]                (dx, [G,Cb,N,T] contiguous)
 * i.e. msgat_contract_segments + msgat_mix_segments(m_in_major = 1) with A streamed once; shapes without a fused
 * form run those two passes.  partials: msgat_contract_mix_partial_floats(R, Bg, N, T, Ca, Cb + with_ones). */
/* partials of msgat_contract_mix_segments for Cb = channels of B INCLUDING the virtual one (round 5: with Cb <= 4 and one
 * A segment the call is ONE pass over A -- dM | dbias and dx together, the form of the AGG_FIRST backward -- whose
 * per-block partials outnumber those of the general form; msgat_contract_segments_partial_floats stays valid for
 * msgat_contract_segments) */
size_t msgat_contract_mix_partial_floats(int32_t R, int32_t Bg, int32_t N, int32_t T, int32_t Ca, int32_t Cb);
int msgat_contract_mix_segments(int32_t R, int32_t Bg, int32_t N, int32_t T, const msgat_seg_t* A, int32_t n_a,
                                const float* B, int32_t Cb, int32_t with_ones, const float* M, float* partials,
                                float* dst, float* mixout, void* stream);
/* Host only, touches no device: the name of the kernel form a [Ca x Cb (+1 with_ones)] contraction over rows of
 * n_positions = N*T takes -- with_mix = 1: as msgat_contract_mix_segments / msgat_stage_project_backward would run it,
 * " + projection pass" appended when no one-pass form covers the shape; with_mix = 0: msgat_contract_segments.
 * E.g. "k_chanpair_glds<7,5,64,3,2>" (LDS-DMA ring, [112 x 80] block, 64-position tiles, wave roles split),
 * "k_chanpair_glds<9,4,64,3,2> nzb=2" (two z-blocks over B), "k_chanpair_mfma<3,2,true,256>" (register-staged).
 * The string comes from the launchers' own selection code (csrc/mfma.hip), so it cannot drift from what runs; the forms
 * exist for the channel counts of the reference's three models (main.py:17, msgat.py:220-229), other shapes fall back
 * to the register-staged kernels.  buf: at least 128 bytes. */
int msgat_contract_form_name(int32_t Ca, int32_t Cb, int32_t with_ones, int32_t n_positions, int32_t with_mix,
                             char* buf, int32_t buflen);

/* ---- device: the attention core on already projected features ----
 * Forward = msgat_stage_scores(q) + msgat_stage_aggregate(u) (above).  Backward of exactly that pair, for
 * callers that produced u and q themselves (e.g. in a merged channel-mixing pass):
 *   du = E^T dv  [G,Cu,N,T],   dq = total gradient at q  [G,N,T],   dWg [R,T,T].
 * shape->C is Cu (the channels of u), shape->Co is ignored.  du must not overlap u or dv (du and the edge gradients
 * come out of one pass that reads both). */
size_t msgat_attention_bwd_workspace_bytes(const msgat_shape_t* shape, const msgat_graph_t* graph);
/* dv_group_channels: as msgat_bwd_t.dz_group_channels, for dv (0 = contiguous); non-zero only where
 * msgat_attention_bwd_accepts_strided_dv() returns 1.  Ec: E in CSC order from msgat_stage_scores, or NULL. */
int msgat_attention_bwd_accepts_strided_dv(const msgat_shape_t* shape, const msgat_graph_t* graph);
int msgat_attention_backward(const msgat_shape_t* shape, const msgat_graph_t* graph, const float* u,
                             const float* dv, int32_t dv_group_channels, const float* q, const float* kW,
                             const float* lse, const float* pq, const float* E, const float* Ec, const float* Wg,
                             float* du, float* dq, float* dWg, void* workspace, size_t workspace_bytes, void* stream);

/* ---- device: the prediction head of a component ----
 * TPC's Conv2d(T_in -> T_out, kernel [1, C]) over the transposed activation (src/models/msgat.py:153,
 * applied :158-159):  out[b,n,o] = bias[o] + sum_c sum_t W[o,t,0,c] x[b,c,n,t].
 * x [B,C,N,T]; W in the convolution's own layout [T_out,T,1,C]; out [B,N,T_out] (what the reference has after
 * its squeeze + transpose); T_out <= 64 (T_out > 16 runs in ceil(T_out / 16) output tiles of 16; larger T_out returns
 * MSGAT_ERR_UNSUPPORTED); `partials` (msgat_head_forward_partial_floats floats) is scratch: the weights
 * re-ordered to [R,C,T,16 ceil(T_out / 16)] by a small pre-pass, so that the kernel stages them with contiguous copies.  Backward: dx [B,C,N,T]; dWc [R,C,T_out,T] (the caller permutes to
 * the convolution layout); partial buffers sized by the *_partial_floats queries. */
size_t msgat_head_forward_partial_floats(int32_t B, int32_t C, int32_t N, int32_t T_out);
int msgat_head_forward(const float* x, const float* W, const float* bias, float* out, float* partials,
                       int32_t B, int32_t C, int32_t N, int32_t T, int32_t T_out, int32_t R, void* stream);
int msgat_head_grad_signal(const float* dout, const float* W, float* dx, int32_t B, int32_t C, int32_t N,
                           int32_t T, int32_t T_out, int32_t R, void* stream);
size_t msgat_head_grad_weight_partial_floats(int32_t C, int32_t T, int32_t T_out, int32_t R);
int msgat_head_grad_weight(const float* dout, const float* x, float* dWc, float* partials, int32_t B, int32_t C,
                           int32_t N, int32_t T, int32_t T_out, int32_t R, void* stream);
/* msgat_head_forward_ln: msgat_head_forward on LayerNorm(x) with x the LayerNorm's INPUT (ln_weight, ln_bias [R,T] or
 * NULL): a row's T values lie in neighbouring lanes of the kernel's load layout, so it normalises what it loads (two lane
 * sums per row) -- one pass over x where msgat_layernorm_forward + msgat_head_forward made three (read, write, read).
 * normalised [B,C,N,T] or NULL: receives LayerNorm(x) when something else needs it (training: msgat_head_grad_weight
 * reads it); with NULL -- inference -- the LayerNorm output, an activation only the head reads (msgat.py:158-159), is never
 * written.  Other buffers as for msgat_head_forward. */
int msgat_head_forward_ln(const float* x, const float* ln_weight, const float* ln_bias, float eps, const float* W,
                          const float* bias, float* out, float* normalised, float* partials, int32_t B, int32_t C,
                          int32_t N, int32_t T, int32_t T_out, int32_t R, void* stream);
/* msgat_layernorm_head_backward: the head's input gradient (msgat_head_grad_signal) AND the backward of the LayerNorm in
 * front of it (msgat.py:158-159: fc(ln(x).transpose(1, 3))) in ONE pass over x: the [B,C,N,T] gradient between the two is
 * built row by row in registers and consumed on the spot.  x is the LayerNorm's INPUT; relu_mask as in
 * msgat_layernorm_backward; dln_weight / dln_bias [R,T] (either may be NULL);
 * partials: msgat_layernorm_head_backward_partial_floats(B, C, N, T) floats. */
size_t msgat_layernorm_head_backward_partial_floats(int32_t B, int32_t C, int32_t N, int32_t T);
int msgat_layernorm_head_backward(const float* dout, const float* W, const float* x, const float* ln_weight, float* dx,
                                  float* dln_weight, float* dln_bias, float* partials, int32_t B, int32_t C, int32_t N,
                                  int32_t T, int32_t To, int32_t R, float eps, int32_t relu_mask, void* stream);

/* ---- device: the tiny attention matrices of a MEAM block, one launch each way ----
 * In the reference each is a chain of batched [T x T] / [C x C] matmuls, a softmax, transposes, pads and stacks
 * (~20 eager launches forward, ~30 backward per block).  One workgroup per (relation, sample) group here;
 * parameter gradients are summed over a relation's groups in a fixed order through `partials`.
 *   channel attention (attention.py:88-94) folded with CACN's 1x1 convolution (msgat.py:93-94):
 *       att[g] = softmax_rows((p_g Wc_r) p_g^T) [C,C],  Mc[g] = conv_r att[g] [cb,C];   p = pooled [G,C,T]
 *       (the node-weighted sums of msgat_node_pool), Wc [R,T,T], conv [R,cb,C].  Mc is the per-sample channel
 *       matrix msgat_mix_segments applies.  Backward: dpooled [G,C,T], dWc [R,T,T], dconv [R,cb,C] from dMc.
 *   temporal attention (attention.py:58-66) as the taps of TACN's first causal convolution (msgat.py:66-74):
 *       left = q_g^T Wt1_r^T, right = q_g^T Wt2_r^T [T,K] (saved in lr [G,2,T,K]),  att[g] = softmax_rows(left right^T),
 *       taps[g,1] = att[g],  taps[g,0] = att[g] shifted down by `dilation` rows (rows < dilation zero);
 *       q = pooled [G,N,T] (the alpha-weighted channel sums), Wt1 / Wt2 [R,K,N], 2 T K <= 256.  taps [G,2,T,T] is what
 *       msgat_time_mix applies (K = 2).  Backward: dpooled [G,N,T], dWt1 / dWt2 [R,K,N] from dtaps.
 * The channel attention keeps its whole problem in the LDS of one workgroup, and the backward needs more of it than the
 * forward: 4 (2 C (C+1) + 3 C T + T^2 + 2 cb C) against 4 (2 C T + T^2 + C (C+1) + cb C) bytes of 160 KiB - 1 KiB; beyond
 * that either entry point returns MSGAT_ERR_UNSUPPORTED.  msgat_channel_attention_fused(C, cb, T) = 1 when BOTH fit (at
 * T = 12, cb = C / 3: up to C = 114; the forward alone up to 165): a caller that differentiates asks it before the
 * forward and evaluates the same ops elsewhere when it is 0, so that nothing fails in the middle of a backward pass. */
int msgat_channel_attention_fused(int32_t C, int32_t cb, int32_t T);
int msgat_channel_attention_forward(const float* pooled, const float* Wc, const float* conv, float* att, float* Mc,
                                    int32_t G, int32_t R, int32_t C, int32_t cb, int32_t T, void* stream);
size_t msgat_channel_attention_partial_floats(int32_t G, int32_t C, int32_t cb, int32_t T);
int msgat_channel_attention_backward(const float* dMc, const float* att, const float* pooled, const float* Wc,
                                     const float* conv, float* dpooled, float* dWc, float* dconv, float* partials,
                                     int32_t G, int32_t R, int32_t C, int32_t cb, int32_t T, void* stream);
int msgat_temporal_attention_forward(const float* pooled, const float* Wt1, const float* Wt2, float* lr, float* att,
                                     float* taps, int32_t G, int32_t R, int32_t N, int32_t K, int32_t T,
                                     int32_t dilation, void* stream);
size_t msgat_temporal_attention_partial_floats(int32_t G, int32_t K, int32_t N);
int msgat_temporal_attention_backward(const float* dtaps, const float* att, const float* lr, const float* pooled,
                                      const float* Wt1, const float* Wt2, float* dpooled, float* dWt1, float* dWt2,
                                      float* partials, int32_t G, int32_t R, int32_t N, int32_t K, int32_t T,
                                      int32_t dilation, void* stream);

/* ---- device: the tail of a training step ----
 * msgat_huber_metrics: one pass over the prediction replaces engine.py:56 (HuberLoss, loss.py:51-52) and the
 *     metric sums of engine.py:70 / metrics.py:20-35, with nothing read back to the host:
 *       loss[0]  = mean over n of (|e| <= delta ? e^2 / 2 : delta |e| - delta^2 / 2),  e = pred - truth   (fp32)
 *       sums[0] += sum |e|;  sums[1] += 100 sum_{truth > mask_value} |e / truth|;  sums[2] += sum e^2;
 *       sums[3] += loss_weight * loss[0]                                           (fp64 [4], running totals
 *     the caller zeroes per epoch; may be NULL).  loss_weight = 1 for a whole batch; a rank holding n_r of a global
 *     batch's n_b samples passes n_r / n_b, so the sum over ranks is the reference's per-batch mean loss
 *     (engine.py:66-67).  `partials`: msgat_huber_partial_doubles(n) doubles.  Fixed summation order: bitwise
 *     reproducible.
 * msgat_huber_grad: dpred = dloss[0] * clamp(e, -delta, delta) / n  -- the backward of the loss above.
 * msgat_adam_step: torch.optim.Adam's update (engine.py:106: lr 1e-3, weight_decay 5e-4 as L2 on the gradient,
 *     betas, eps outside the square root, bias correction) for ALL parameter tensors in one launch.  The
 *     gradients and both moments are flat fp32 buffers; the parameters stay where they are and are reached
 *     through a chunk table (device arrays): chunk c = chunk_len[c] <= msgat_adam_chunk_elems() elements of
 *     tensor chunk_tensor[c] at chunk_param[c], whose gradient / moments start at element chunk_off[c] of the
 *     flat buffers.  steps[t] = updates tensor t has received so far, advanced by this call for the n_active
 *     tensors listed in active_tensors (torch keeps one step count per parameter and skips parameters without a
 *     gradient); lr[0] = learning rate.  Both are device memory, so a captured launch follows the scheduler.
 *     The hyper-parameters are doubles, like the Python floats the reference's optimizer holds: 1 - beta2 must
 *     be rounded to fp32 once, not computed from an fp32 beta2.
 *     grad_divisor (device, may be NULL): when given, every gradient is divided by grad_divisor[0] on the way in.
 * msgat_gather_scaled: the front half of a data-parallel step (replaces nn.DataParallel's gradient reduce-add,
 *     main.py:52-55): flat[chunk_off[c] + i] = scale * chunk_src[c][i] for chunk_len[c] elements per chunk (device
 *     table, as above, but of GRADIENT pointers) and flat[weight_index] = scale (weight_index < 0: not written).
 *     With scale = the rank's sample count and weight_index = the buffer's last element, ONE all-reduce of `flat`
 *     yields sum_r(w_r g_r) and sum_r(w_r); msgat_adam_step(grad_divisor = flat + weight_index) finishes the mean. */
/* msgat_gate_sum: the model's last line, out = sum_r pred_r * gate_r (msgat.py:203-205) with the gate built on the fly
 *     from the two embedding tables (embeddings.py:36-39: gate[b] = h_ebd(H[b]) + d_ebd(D[b]) viewed [R,N,T_out]):
 *       out[b,e] = sum_r pred[r,b,e] * (h_w[H[b]][r,e] + d_w[D[b]][r,e]),   e < E = N * T_out, summed in the order of r.
 *     pred [R,B,E] (the R components' predictions, relation-major); H, D [B] int64 (torch's index type); h_w [nh, R*E],
 *     d_w [nd, R*E] row-major as nn.Embedding keeps them.  Indices are clamped into [0, nh) / [0, nd) (torch's gather
 *     traps on the device instead).  Static gate (msgat.py:189): H = D = d_w = NULL, nh = 1, h_w = W [R,E].
 * msgat_gate_sum_backward: dpred [R,B,E] = dout * gate, and the DENSE table gradients dh_w [nh, R*E], dd_w [nd, R*E]
 *     (every row written; a row's samples are added in sample order).  Any output may be NULL.
 *     Reference: 5 launches forward, 12 backward (gathers, multiplies, a transposing copy, two zero-fill + scatter
 *     embedding gradients); one each here. */
int msgat_gate_sum(const float* pred, const int64_t* H, const int64_t* D, const float* h_w, const float* d_w, float* out,
                   int32_t R, int32_t B, int64_t E, int32_t nh, int32_t nd, void* stream);
int msgat_gate_sum_backward(const float* dout, const float* pred, const int64_t* H, const int64_t* D, const float* h_w,
                            const float* d_w, float* dpred, float* dh_w, float* dd_w, int32_t R, int32_t B, int64_t E,
                            int32_t nh, int32_t nd, void* stream);
/* msgat_edge_time_weights: one weight per stored edge AND per sample from the sample's hour of day and day of week, the
 *     idiom of the time embedding (embeddings.py:30-36: h_ebd(H) + d_ebd(D)) applied to the edges of one sparse pattern:
 *       out[b,e] = (base[e] + h_w[H[b]][e]) + d_w[D[b]][e],   e < nnz -- plain fp32 adds in that order, no contraction: the
 *     bits of the torch expression (base + h_w[H]) + d_w[D].  base [nnz]; h_w [nh,nnz], d_w [nd,nnz] row-major as
 *     nn.Embedding keeps them; H, D [B] int64, clamped into [0, nh) / [0, nd) as msgat_gate_sum clamps them; out [B,nnz]
 *     contiguous in the order of (crow, col), which msgat_graph_t.val with val_sets = B reads where it is.
 *     d_w = D = NULL: the hour table only.  B = 0 or nnz = 0: nothing is launched, MSGAT_OK; a negative size is
 *     MSGAT_ERR_SHAPE.
 * msgat_edge_time_weights_backward: dbase[e] = sum_b dout[b,e] and the DENSE table gradients dh_w [nh,nnz], dd_w [nd,nnz]:
 *     dh_w[r][e] = sum over the samples with H[b] = r of dout[b,e], likewise dd_w.  Every sum starts at +0 and adds in
 *     ascending b (no atomics: the bits are a function of the inputs), every row of both tables is written -- a row no
 *     sample selected is zero -- so the caller zeroes nothing, and nothing is read back (capturable).  Any output may be
 *     NULL.  nnz = 0 launches nothing; B = 0 with nnz > 0 writes the zeros.
 *     The torch ops this replaces: 2 gathers + 2 adds forward; a batch sum, 2 zero fills and 2 embedding scatters
 *     (atomic, in no promised order) backward; one launch each here. */
int msgat_edge_time_weights(const float* base, const float* h_w, const float* d_w, const int64_t* H, const int64_t* D,
                            float* out, int32_t B, int64_t nnz, int32_t nh, int32_t nd, void* stream);
int msgat_edge_time_weights_backward(const float* dout, const int64_t* H, const int64_t* D, float* dbase, float* dh_w,
                                     float* dd_w, int32_t B, int64_t nnz, int32_t nh, int32_t nd, void* stream);
/* msgat_edge_signal_weights: one weight per stored edge AND per sample from the sample's own node signals, the edge strength
 *     of the dynamic-graph models as a rank-d bilinear form on the edges of `graph`'s pattern:
 *       out[b,e] = base[e] + sum_{k<d} a[b,row(e),k] * b[b,col(e),k],   e < nnz in the graph's CSR edge order,
 *     with ab [B,N,2d] contiguous, a = ab[..., :d] (the row side) and b = ab[..., d:] (the column side) -- the caller's
 *     projection f @ P.T of the node features, P [2d,F].  base [nnz]; out [B,nnz], which msgat_graph_t.val with
 *     val_sets = B reads where it is.  Reads graph->erow and graph->col; graph->val is not read.  One launch.
 *     Every product is rounded to fp32, the products are added in ascending k and base[e] is added last (no contraction):
 *     the bits of fp32 torch ops applied in that order.
 * msgat_edge_signal_weights_backward: from dout [B,nnz]
 *       dbase[e]   = sum_b dout[b,e]                                      (starts at +0, adds in ascending b: defined bits)
 *       da[b,i,:]  = sum_{e in row i}    dout[b,e] * b[b,col(e),:]        (ascending CSR edge order: rowptr, col)
 *       db[b,j,:]  = sum_{e in column j} dout[b,e] * a[b,row(e),:]        (ascending CSC position: colptr, crow, cperm)
 *     written as dab [B,N,2d] = (da, db) in the layout of ab.  No atomics, nothing zeroed by the caller, nothing read back
 *     (capturable): every element of dab is written, +0 for a node without a stored edge in its row / column, and dbase
 *     wholly.  dbase = NULL or dab = NULL skips that output.  One launch.
 *     d must be a multiple of 4 (rows are read as 16-byte pieces) and at most 32: else MSGAT_ERR_UNSUPPORTED; B < 0 or
 *     d <= 0: MSGAT_ERR_SHAPE; graph = NULL, or a needed pointer NULL with work to do: MSGAT_ERR_NULL -- all decided on the
 *     host before any launch.  B = 0: MSGAT_OK, nothing written.  nnz = 0 with B > 0: MSGAT_OK, the forward writes nothing
 *     and the backward writes dab as zeros. */
int msgat_edge_signal_weights(const msgat_graph_t* graph, const float* base, const float* ab, int32_t B, int32_t d,
                              float* out, void* stream);
int msgat_edge_signal_weights_backward(const msgat_graph_t* graph, const float* dout, const float* ab, int32_t B, int32_t d,
                                       float* dbase, float* dab, void* stream);
/* msgat_edge_dropout: dropout on the stored edges of one sparse pattern (DropEdge with inverted scaling), the mask drawn from
 *     a counter-based generator whose state lives in device memory.  Philox4x32-10 with the Random123 constants
 *     (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85): edge e of global sample s at step t under
 *     seed k reads word e & 3 of philox(counter = (e >> 2, s, t & 0xffffffff, t >> 32), key = (k & 0xffffffff, k >> 32)) and
 *     is DROPPED iff that word < thr -- an integer compare; the caller passes thr = (uint32) floor(p * 2^32) and
 *     scale = (float)(1 / (1 - p)), both computed in double.  s = sample_offset + v for row v of the output.
 *       out[v,e] = exempt[e] ? w : (dropped ? +0.0f : w * scale)      -- w * scale is one fp32 multiply
 *     w [nnz] (w_sets = 0: shared by the V samples) or [V,nnz] (w_sets != 0); exempt uint8 [nnz] or NULL (no edge is exempt);
 *     out [V,nnz] contiguous in the order of (crow, col), which msgat_graph_t.val with val_sets = V reads where it is.
 *     state int64 [2] = {seed, step} and used int64 [1] are device memory: the launch reads seed and step, writes the step it
 *     drew from into used[0], and -- advance != 0 -- a one-thread launch behind it in stream order sets step + 1, after every
 *     block has read the old one.  Nothing is read back (capturable: every replay draws the next step).  advance = 0 draws
 *     without moving the stream.
 * msgat_edge_dropout_backward: re-creates the draw from state[0] (the seed) and used[0] -- it does not read the step, so
 *     several forwards followed by their backwards each see their own masks -- and writes, m = 0 / scale / 1 as above,
 *       w_sets != 0:  dw[v,e] = dout[v,e] * m[v,e]              (one multiply: the bits of the torch expression)
 *       w_sets == 0:  dw[e]   = sum_v dout[v,e] * m[v,e]        (rounded products added from +0 in ascending v)
 *     Every entry is written, nothing is atomic; one launch.  dw = NULL: nothing is written, MSGAT_OK.
 *     Both: V < 0, nnz < 0 or sample_offset < 0: MSGAT_ERR_SHAPE; nnz >= 2^34 or sample_offset + V > 2^32 (the counter's
 *     words are 32 bits): MSGAT_ERR_UNSUPPORTED; V = 0 or nnz = 0: MSGAT_OK and nothing is launched -- an empty forward draws
 *     nothing, so it neither writes `used` nor advances the step; a required pointer NULL with work to do: MSGAT_ERR_NULL.
 *     The torch ops this replaces: a uniform draw, a compare, a select and a multiply forward, a multiply and a batch sum
 *     backward, with a mask tensor kept in between. */
int msgat_edge_dropout(const float* w, const uint8_t* exempt, int64_t* state, int64_t* used, float* out, int32_t V,
                       int64_t nnz, int32_t w_sets, int64_t sample_offset, uint32_t thr, float scale, int32_t advance,
                       void* stream);
int msgat_edge_dropout_backward(const float* dout, const uint8_t* exempt, const int64_t* state, const int64_t* used,
                                float* dw, int32_t V, int64_t nnz, int32_t w_sets, int64_t sample_offset, uint32_t thr,
                                float scale, void* stream);
/* msgat_edge_validity: validity-gated edges on the pattern of `graph` -- a sensor whose input window holds missing readings
 *     sends weaker messages, or none.  val [V,N,T] fp32 is the validity channel of the samples' input windows (1 = measured,
 *     0 = imputed): its last two dimensions are contiguous and sample v starts val_stride ELEMENTS after sample v - 1, so the
 *     strided view X[:, 0, -1] of a contiguous X [B,R,C,N,T] is read where it is.  With
 *       count[v,n] = the number of t with val[v,n,t] > 0.5f            -- a NaN is not counted
 *       g[v,n]     = table[count[v,n]]                                 -- table: T + 1 HOST floats, passed on by value
 *     edge e of the pattern in the graph's CSR edge order, with source node col(e), gets
 *       out[v,e] = exempt[e] ? w : (g[v,col(e)] == 0 ? +0.0f : w * g[v,col(e)])     -- w * g is one fp32 multiply
 *     so a fully gated edge is +0 whatever w holds (a NaN too).  w [nnz] (w_sets = 0: shared by the V samples) or [V,nnz]
 *     (w_sets != 0); exempt uint8 [nnz] or NULL (no edge is exempt); out [V,nnz] contiguous, which msgat_graph_t.val with
 *     val_sets = V reads where it is.  Reads graph->col, graph->nnz and graph->n_nodes only; graph->val is not read.
 *     One launch.  An aligned val (base and val_stride * 4 multiples of 16 bytes) is read as 16-byte pieces, any other with
 *     single loads: the same result.
 * msgat_edge_validity_backward: re-creates the gate from val -- nothing is kept between the two calls -- and writes
 *       w_sets != 0:  dw[v,e] = exempt[e] ? dout[v,e] : (g == 0 ? +0.0f : dout[v,e] * g)
 *       w_sets == 0:  dw[e]   = the sum over v of those rounded terms, from +0 in ascending v
 *     Every entry is written, nothing is atomic; one launch.  dw = NULL: nothing is written, MSGAT_OK.  val gets no gradient:
 *     it is data.
 *     Both: graph = NULL: MSGAT_ERR_NULL; V < 0, T < 0, val_stride < 0 or a negative size in graph: MSGAT_ERR_SHAPE; T not in
 *     {4, 8, 12, 16}: MSGAT_ERR_UNSUPPORTED; V = 0 or nnz = 0: MSGAT_OK and nothing is launched; a required pointer NULL with
 *     work to do: MSGAT_ERR_NULL -- all decided on the host before any launch.  Nothing is read back (capturable).
 *     The torch ops this replaces: a compare, a sum, two gathers, a compare, two selects and a multiply forward; the same
 *     gate again, a multiply and a batch sum backward. */
int msgat_edge_validity(const msgat_graph_t* graph, const float* w, const uint8_t* exempt, const float* val,
                        int64_t val_stride, const float* table, float* out, int32_t V, int32_t T, int32_t w_sets,
                        void* stream);
int msgat_edge_validity_backward(const msgat_graph_t* graph, const float* dout, const uint8_t* exempt, const float* val,
                                 int64_t val_stride, const float* table, float* dw, int32_t V, int32_t T, int32_t w_sets,
                                 void* stream);
size_t msgat_huber_partial_doubles(int64_t n);
int msgat_huber_metrics(const float* pred, const float* truth, int64_t n, float delta, float mask_value,
                        double* partials, float* loss, double* sums, float loss_weight, void* stream);
int msgat_huber_grad(const float* pred, const float* truth, const float* dloss, int64_t n, float delta,
                     float* dpred, void* stream);
int msgat_adam_chunk_elems(void);
int msgat_adam_step(float* const* chunk_param, const int64_t* chunk_off, const int32_t* chunk_len,
                    const int32_t* chunk_tensor, int32_t n_chunks, const int32_t* active_tensors, int32_t n_active,
                    const float* grad, float* exp_avg, float* exp_avg_sq, float* steps, const float* lr,
                    double beta1, double beta2, double eps, double weight_decay, const float* grad_divisor,
                    void* stream);
int msgat_gather_scaled(const float* const* chunk_src, const int64_t* chunk_off, const int32_t* chunk_len,
                        int32_t n_chunks, float scale, float* flat, int64_t weight_index, void* stream);

/* ---- device: the step tail with missing readings (no counterpart in the reference, whose only mask guards the MAPE's
 * division, metrics.py:28) ----
 * An entry of `truth` is VALID when it is not NaN and truth != null_value (PEMS files store 0 for a sensor that was
 * down); null_value = NaN masks the NaN entries only.  pred, truth [rows, T_out] fp32, rows = B * N, 1 <= T_out <= 64,
 * rows * T_out <= 2^24 (MSGAT_ERR_UNSUPPORTED beyond either), so every count below is exact in an fp32.
 * msgat_masked_huber_metrics: one pass over the two tensors and a five-block finish launch, nothing read back:
 *       valid[0] = the number of valid entries                                                        (fp32, device)
 *       loss[0]  = sum_valid huber(e) / max(valid, 1),  e = pred - truth, huber as in msgat_huber_metrics   (fp32)
 *       sums [T_out + 1, 5] fp64 running totals (the caller zeroes them per epoch; may be NULL): row t < T_out +=
 *           {valid count, sum |e|, 100 sum_{truth > mask_value} |e / truth|, sum e^2, sum huber(e)} over the valid
 *           entries of horizon t (element i has horizon i mod T_out); row T_out += the same over all horizons.
 *     A batch without a valid entry gives loss 0 and valid 0.  `partials`: msgat_masked_huber_partial_doubles(rows,
 *     T_out) doubles.  Fixed summation order (lane order inside a block, block order across blocks, horizon order for
 *     the last row), no floating-point atomics: bitwise reproducible.
 * msgat_masked_huber_grad: dpred = dloss[0] * clamp(e, -delta, delta) / max(valid[0], 1) at the valid entries and
 *     exactly 0 at the others (a NaN of `truth` does not reach dpred).  valid[0] is read from device memory -- what
 *     msgat_masked_huber_metrics wrote -- so a launch captured in a HIP graph follows the batch of every replay.
 * msgat_gather_scaled_dev: msgat_gather_scaled with the scale read from device memory (scale[0]; it is also what
 *     flat[weight_index] receives): a rank's weight in a masked data-parallel step is its batch's valid count. */
size_t msgat_masked_huber_partial_doubles(int64_t rows, int32_t T_out);
int msgat_masked_huber_metrics(const float* pred, const float* truth, int64_t rows, int32_t T_out, float delta,
                               float null_value, float mask_value, double* partials, float* loss, float* valid,
                               double* sums, void* stream);
int msgat_masked_huber_grad(const float* pred, const float* truth, const float* dloss, const float* valid, int64_t rows,
                            int32_t T_out, float delta, float null_value, float* dpred, void* stream);
int msgat_gather_scaled_dev(const float* const* chunk_src, const int64_t* chunk_off, const int32_t* chunk_len,
                            int32_t n_chunks, const float* scale, float* flat, int64_t weight_index, void* stream);

/* ---- device: the Gauss loss in the step tail, plain and masked (GaussLoss / gauss_loss, loss.py:55-95) ----
 * The reference's robust loss, whose weight on an entry saturates where Huber's grows without bound.  With
 * e = pred - truth, sigma finite and > 0, delta finite and >= 0 (0: the saturating term alone):
 *       g(e)  = sigma^2 (1 - exp(-e^2 / (2 sigma^2))) + delta |e|                       (the value of one entry)
 *       g'(e) = e exp(-e^2 / (2 sigma^2)) + delta sgn(e),  sgn(0) = 0                    (torch's abs backward)
 * The four entry points mirror msgat_huber_metrics, msgat_huber_grad, msgat_masked_huber_metrics and
 * msgat_masked_huber_grad argument for argument, with sigma in front of delta, and run the same kernels with another
 * loss: the same launches, summation order, status codes and limits, `partials` sized by the SAME
 * msgat_huber_partial_doubles(n) / msgat_masked_huber_partial_doubles(rows, T_out) with the same layout, and the same
 * totals -- sums [4] with sums[3] += loss_weight * loss[0], sums [T_out + 1, 5] with column 4 = sum g(e).
 *       plain    loss[0] = mean over n of g(e)   (= sigma^2 mean(1 - exp(...)) + delta mean |e|, loss.py:94-95);
 *                dpred = dloss[0] g'(e) / n
 *       masked   loss[0] = sum_valid g(e) / max(valid, 1);  dpred = dloss[0] g'(e) / max(valid[0], 1) at the valid
 *                entries and exactly +0 at the others
 * g and g' are evaluated per entry in fp32 -- 1 - exp(-t) as -expm1f(-t), which keeps its precision for |e| << sigma
 * where 1 - expf(-t) cancels -- and added in fp64; sigma^2 and 1 / (2 sigma^2) are formed in double and rounded once.
 * sigma or delta outside their ranges (NaN included): MSGAT_ERR_SHAPE, before any launch. */
int msgat_gauss_metrics(const float* pred, const float* truth, int64_t n, float sigma, float delta, float mask_value,
                        double* partials, float* loss, double* sums, float loss_weight, void* stream);
int msgat_gauss_grad(const float* pred, const float* truth, const float* dloss, int64_t n, float sigma, float delta,
                     float* dpred, void* stream);
int msgat_masked_gauss_metrics(const float* pred, const float* truth, int64_t rows, int32_t T_out, float sigma, float delta,
                               float null_value, float mask_value, double* partials, float* loss, float* valid,
                               double* sums, void* stream);
int msgat_masked_gauss_grad(const float* pred, const float* truth, const float* dloss, const float* valid, int64_t rows,
                            int32_t T_out, float sigma, float delta, float null_value, float* dpred, void* stream);

/* ---- device: quantile forecasts in the step tail (no counterpart in the reference, whose forecasts are single numbers) ----
 * A Q-level forecast of T_out steps is a head with Q * T_out outputs: pred [rows, Q, T_out] fp32, level-major inside a
 * row, against truth [rows, T_out], rows = B * N.  `levels` [Q] are HOST floats, strictly increasing inside (0, 1); they
 * reach the kernels by value.  `point` in [0, Q) names the level that serves as the point forecast.  An entry of
 * `truth` is valid exactly as in the masked tail above (not NaN and != null_value; null_value = NaN masks the NaN
 * entries only -- there is no unmasked form).  Per valid entry and level, with u = truth - p_q in fp32:
 *       rho_q = max(tau_q u, (tau_q - 1) u)                                                  (the pinball loss)
 *       d rho_q / d p_q = -tau_q where truth > p_q, 1 - tau_q where truth < p_q, 1/2 - tau_q at truth == p_q
 *                                                                   (autograd's rule for torch.maximum at a tie)
 * msgat_quantile_metrics: one pass and a finish launch of 7 + 2Q blocks, nothing read back:
 *       valid[0] = the number of valid entries,  loss[0] = sum_valid (1/Q) sum_q rho_q / max(valid, 1)        (fp32)
 *       sums [T_out + 1, 7 + 2Q] fp64 running totals (the caller zeroes them per epoch; may be NULL); row t < T_out holds
 *       horizon t, row T_out all horizons added in horizon order.  Columns:
 *           0-3         {valid count, sum |e|, 100 sum_{truth > mask_value} |e / truth|, sum e^2},  e = p_point - truth
 *           4           sum of (1/Q) sum_q rho_q            (the loss column, where the masked layout has it)
 *           5           the number of valid entries with any p_q > p_{q+1}                         (crossing)
 *           6           sum of p_{Q-1} - p_0                                  (width of the outermost interval)
 *           7 + q       the number of valid entries with truth <= p_q                                   (hits)
 *           7 + Q + q   sum of rho_q
 *     A batch without a valid entry gives loss 0 and valid 0; so does rows = 0 (MSGAT_OK, nothing else is written).
 *     `partials`: msgat_quantile_partial_doubles(rows, T_out, Q) doubles.  Fixed summation order as in the masked tail,
 *     no floating-point atomics: bitwise reproducible.
 * msgat_quantile_grad: dpred[r,q,t] = c_q * (dloss[0] / max(valid[0], 1)) at the valid entries, c_q the slope above
 *     divided by Q -- formed in double, one value per level and sign case, rounded to fp32 once -- and exactly +0 at
 *     every other entry.  valid[0] is read from device memory, so a captured launch follows the batch of every replay.
 * Limits, checked before any launch: 1 <= Q <= 8, 1 <= T_out, Q * T_out <= 64, rows * T_out <= 2^24
 * (MSGAT_ERR_UNSUPPORTED otherwise); levels not increasing or outside (0, 1), NaN included, point outside [0, Q) and
 * rows < 0: MSGAT_ERR_SHAPE. */
size_t msgat_quantile_partial_doubles(int64_t rows, int32_t T_out, int32_t Q);
int msgat_quantile_metrics(const float* pred, const float* truth, int64_t rows, int32_t T_out, int32_t Q,
                           const float* levels, int32_t point, float null_value, float mask_value, double* partials,
                           float* loss, float* valid, double* sums, void* stream);
int msgat_quantile_grad(const float* pred, const float* truth, const float* dloss, const float* valid, int64_t rows,
                        int32_t T_out, int32_t Q, const float* levels, float null_value, float* dpred, void* stream);

/* ---- device: the guard on the optimizer step (off unless a caller uses msgat_grad_guard and msgat_adam_step_guarded) ----
 * The reference trains under GradScaler (engine.py:61-63), whose step() leaves the update out when a gradient is Inf or
 * NaN; this build trains in fp32 without a scaler, so that protection -- and global-norm clipping, which cannot be added
 * from outside a captured step or a multi-rank step whose mean gradient exists only in the flat buffer -- lives here.
 * `guard`: MSGAT_GUARD_FLOATS fp32 in device memory that the caller allocates and zeroes once:
 *       guard[0] = the gradient's global L2 norm of this step, before clipping
 *       guard[1] = coef, what the gradient is scaled by (0 for a step that is left out)
 *       guard[2] = the number of steps left out so far (+1 per non-finite step; exact up to 2^24)
 *       guard[3] = the largest finite guard[0] since the caller last zeroed this element
 *       guard[4] = 1 if this step's sum of squares is finite, else 0
 * msgat_grad_guard: two launches, nothing read back.  (1) One block per chunk of the chunk table msgat_adam_step takes
 *     (chunk_off, chunk_len; a parameter without a gradient has no chunk and its stale part of `grad` is not read) squares
 *     its elements and adds them in double -- a finite gradient of 1e30 gives a finite norm -- into partials[c].
 *     (2) S = the partials added in index order in double; D = grad_divisor[0] if given (the summed rank weights of a
 *     data-parallel step, whose `grad` holds sum_r w_r g_r) else 1; norm = (float)(sqrt(S) / D);
 *     coef = min(1, max_norm / (norm + 1e-6)) in fp32, exactly torch.nn.utils.clip_grad_norm_'s; max_norm = INFINITY
 *     asks for no clipping (coef = 1).  max_norm <= 0 or NaN: MSGAT_ERR_SHAPE; guard NULL: MSGAT_ERR_NULL.
 *     `partials`: msgat_grad_guard_partial_doubles(n_chunks) doubles.  Every sum has one fixed order and there are no
 *     atomics: equal inputs give equal bits on every launch and, after the all-reduce, on every rank.
 * msgat_adam_step_guarded: msgat_adam_step reading guard[1] and guard[4] from device memory.  Finite step:
 *     g = weight_decay * w + coef * (grad / D) -- the clipping acts on the raw gradient before the L2 term, as
 *     clip_grad_norm_ followed by optim.Adam does -- and with coef == 1 every result has the bits msgat_adam_step gives.
 *     Non-finite step: NOTHING is written, no parameter, no moment, no step count (GradScaler.step's behaviour; it
 *     differs on purpose from clip_grad_norm_, which would scale every gradient by NaN). */
#define MSGAT_GUARD_FLOATS 5
size_t msgat_grad_guard_partial_doubles(int32_t n_chunks);
int msgat_grad_guard(const int64_t* chunk_off, const int32_t* chunk_len, int32_t n_chunks, const float* grad,
                     const float* grad_divisor, float max_norm, double* partials, float* guard, void* stream);
int msgat_adam_step_guarded(float* const* chunk_param, const int64_t* chunk_off, const int32_t* chunk_len,
                            const int32_t* chunk_tensor, int32_t n_chunks, const int32_t* active_tensors,
                            int32_t n_active, const float* grad, float* exp_avg, float* exp_avg_sq, float* steps,
                            const float* lr, double beta1, double beta2, double eps, double weight_decay,
                            const float* grad_divisor, const float* guard, void* stream);

/* ---- device: averaged weights (off unless a caller uses msgat_adam_step_averaged) ---------------------------------------
 * An exponential moving average (EMA) of the parameters, kept by the launch that forms them: it cannot be added from
 * outside a captured step (the update is inside the graph), beside the guard (the host does not know which steps were left
 * out) or across ranks (only the same launch gives every rank the same bits).
 * msgat_adam_step_averaged: msgat_adam_step (guard == NULL) or msgat_adam_step_guarded (guard given) -- the same two
 *     launches, and parameters, moments and step counts with the bits those leave -- that also moves `shadow`, a flat fp32
 *     buffer in the layout of exp_avg.  For every element of every chunk of the table, after w_new is formed:
 *         t   = steps[chunk_tensor[c]]                  (already advanced: 1 at a tensor's first update; exact up to 2^24)
 *         d   = min((float)decay, (1 + t) / (10 + t))   (the warm-up of the average, per tensor)
 *         omd = 1 - d
 *         e   = e + omd * (w_new - e)                   (e = shadow[chunk_off[c] + i])
 *     every operation of these lines rounded on its own in fp32 (no fma, no contraction): a float32 restatement gives the
 *     same bits.  The tensor's step count is the only clock.  A tensor without a gradient has no chunk and its shadow is
 *     not touched, as its parameter is not; with `guard` given a non-finite step writes nothing, the shadow included.
 *     decay outside [0, 1) or NaN: MSGAT_ERR_SHAPE; shadow NULL: MSGAT_ERR_NULL.
 * msgat_param_swap: one launch, one block per chunk, exchanges chunk_param[c][i] with flat[chunk_off[c] + i] as 32-bit
 *     words (NaNs keep their bits): two calls are the identity.  With flat = shadow, whoever holds the parameters'
 *     addresses (a captured validation graph) reads the averaged weights.  n_chunks == 0: MSGAT_OK, nothing launched;
 *     n_chunks < 0: MSGAT_ERR_SHAPE. */
int msgat_adam_step_averaged(float* const* chunk_param, const int64_t* chunk_off, const int32_t* chunk_len,
                             const int32_t* chunk_tensor, int32_t n_chunks, const int32_t* active_tensors,
                             int32_t n_active, const float* grad, float* exp_avg, float* exp_avg_sq, float* steps,
                             const float* lr, double beta1, double beta2, double eps, double weight_decay,
                             const float* grad_divisor, const float* guard, float* shadow, double decay, void* stream);
int msgat_param_swap(float* const* chunk_param, const int64_t* chunk_off, const int32_t* chunk_len, int32_t n_chunks,
                     float* flat, void* stream);

/* ---- device: gradient accumulation (off unless a caller uses these two) -------------------------------------------------
 * A window of k micro-batches is one optimizer step on their union: the first micro-batch enters the flat buffer through
 * msgat_gather_scaled{,_dev} (which overwrites: no zeroing pass), every later one through
 * msgat_gather_accumulate: one launch, one block per chunk of the same chunk table,
 *         flat[chunk_off[c] + i] = flat[chunk_off[c] + i] + scale * chunk_src[c][i]
 *         flat[weight_index]     = flat[weight_index] + scale                              (block 0; weight_index >= 0)
 *     with the product and the sum each rounded on its own in fp32 (no fma, no contraction): the buffer after two
 *     micro-batches has the bits of a two-rank all-reduce sum of the same two scaled gradients, and a float32 restatement
 *     gives them too.  No atomics, one fixed order; elements outside the table's chunks are neither read nor written.
 *     The update then divides by flat[weight_index] on the way in (grad_divisor of msgat_adam_step*).
 * msgat_gather_accumulate_dev: the same with the scale read from device memory (scale[0]: the valid count of a masked
 *     micro-batch, never read back).
 * Arguments, NULL and shape checks (before anything is enqueued) as msgat_gather_scaled / msgat_gather_scaled_dev. */
int msgat_gather_accumulate(const float* const* chunk_src, const int64_t* chunk_off, const int32_t* chunk_len,
                            int32_t n_chunks, float scale, float* flat, int64_t weight_index, void* stream);
int msgat_gather_accumulate_dev(const float* const* chunk_src, const int64_t* chunk_off, const int32_t* chunk_len,
                                int32_t n_chunks, const float* scale, float* flat, int64_t weight_index, void* stream);

/* ---- device: the input windows of a batch (replaces data_loader.py:92-115, TimeSeriesSlice, and the host collate) ----
 * msgat_window_gather: one launch builds the batch of B forecast origins from a series that stays in device memory.
 *       series  [T_total, C, N] fp32   the normalised series, TIME-MAJOR (the host keeps [C, N, T_total]; the caller
 *                                      transposes once): every read is then coalesced over the (channel, node) rows
 *       target  [N, T_total]    fp32   channel 0 of the raw series, as the host keeps it
 *       origins [B]  int64, device     the forecast origins t_b
 *       offsets [R]  int64, device     offsets[r] = hours[r] * tau, how far component r looks back; history = their
 *                                      largest (a POD: the clamp below must not depend on device data being read back)
 *     writes, with t_b = origins[b] CLAMPED into [history, T_total - q]:
 *       X [B, R, C, N, tau] fp32   X[b,r,c,n,k] = series[t_b - offsets[r] + k, c, n]
 *       Y [B, N, q]         fp32   Y[b,n,j]     = target[n, t_b + j]
 *       H [B], D [B]        int64  (t_b / tau) % 24 and (t_b / tau / 24) % 7
 *     The clamp makes ANY content of `origins` safe: no origin can make the launch read outside the two arrays (a window
 *     start is clamped into [0, T_total - tau] as well, so neither can a table with offsets[r] > history); a clamped
 *     origin yields the batch of the nearest valid origin.  Values move as 32-bit words: NaNs keep their bits.  Every
 *     offset is 64-bit (a series of 8192 nodes passes 2^31 elements).  tau in {4, 8, 12, 16} (MSGAT_ERR_UNSUPPORTED
 *     otherwise), 1 <= q <= 64, any B, R >= 1, C * N and N * q below 2^31 - 256; T_total >= history + q (MSGAT_ERR_SHAPE otherwise).
 *     X must be 16-byte aligned. */
int msgat_window_gather(const float* series, const float* target, const int64_t* origins, const int64_t* offsets,
                        float* X, int64_t* H, int64_t* D, float* Y, int32_t B, int32_t R, int32_t C, int32_t N,
                        int64_t T_total, int32_t tau, int32_t q, int64_t history, void* stream);

/* msgat_window_gather_imputed: msgat_window_gather for a series whose missing readings are stored as NaN -- the same
 * launch fills them in and, on request, appends a validity channel.
 *       climatology [period, C, N] fp32   what a missing reading of slot s = (absolute step) % period becomes
 *                                         (period = 1: one value per (channel, node)); read for missing entries only
 *     writes, with t_b clamped as above, s = t_b - offsets[r] + k (the window start clamped as above) and C' = C + 1 if
 *     mask_channel != 0, else C:
 *       X [B, R, C', N, tau] fp32   X[b,r,c,n,k] = series[s, c, n], or climatology[s % period, c, n] where that word is a
 *                                   NaN ((w & 0x7fffffff) > 0x7f800000); every other word keeps its bits
 *                                   X[b,r,C,n,k] = 1.0f where no channel of series[s, :, n] is a NaN, else 0.0f
 *       Y, H, D                     as msgat_window_gather writes them: Y keeps the raw target, null values included
 *     Arguments as msgat_window_gather, and period >= 1 (MSGAT_ERR_SHAPE otherwise), climatology non-NULL, (C + 1) * N
 *     below 2^31 - 256 (MSGAT_ERR_UNSUPPORTED otherwise) whether or not the validity channel is asked for. */
int msgat_window_gather_imputed(const float* series, const float* climatology, const float* target,
                                const int64_t* origins, const int64_t* offsets, float* X, int64_t* H, int64_t* D,
                                float* Y, int32_t B, int32_t R, int32_t C, int32_t N, int64_t T_total, int32_t tau,
                                int32_t q, int64_t history, int32_t period, int32_t mask_channel, void* stream);

/* ---- device: online forecasting -- a ring of readings in device memory and the windows of the origin "now" ----
 * (data_loader.py:92-120 slices and normalises a series that exists in full; a reading that arrives after training has
 * no path there.)  State, both in device memory and never read back:
 *       ring  [L, C, N] fp32   the normalised history, TIME-MAJOR: the row of absolute step s is s mod L; a missing
 *                              reading is stored as a NaN.  A new ring is filled with the canonical NaN 0x7fc00000.
 *       clock [2] int64        clock[0]: the absolute index of the next reading = the forecast origin t;
 *                              clock[1]: the count of readings held, saturating at L
 * "mod" is the floor-mod into [0, L): ANY clock content (a cold ring, t smaller than an offset, a wild word) addresses
 * rows inside the ring, so neither entry point can read or write outside its arrays.
 *
 * msgat_ring_push: raw [K, C, N] fp32, the readings of K consecutive steps (1 <= K <= L), go into the rows
 *     (clock[0] + k) mod L as (raw - mean[c,n]) / std[c,n] -- one IEEE subtract and one correctly rounded divide, the bits
 *     of the torch expression the training series was normalised with (mean, std [C, N] fp32).  has_null != 0: a reading
 *     that is NaN or equal to null_value is stored as the word 0x7fc00000 (null_value = NaN: the NaNs only); has_null
 *     == 0: the quotient and nothing else.  A one-thread launch that follows in stream order then sets clock[0] += K and
 *     clock[1] = min(clock[1] + K, L): two launches, capturable.
 *     A NULL pointer: MSGAT_ERR_NULL; K, C, N or L <= 0, or K > L: MSGAT_ERR_SHAPE; C * N above 2^31 - 256:
 *     MSGAT_ERR_UNSUPPORTED.
 *
 * msgat_ring_windows: X, H, D of the ONE origin t = clock[0], read on the device, in one launch -- what
 *     msgat_window_gather{,_imputed} gives for B = 1 over the full series:
 *       X [1, R, C', N, tau] fp32  X[0,r,c,n,k] = ring[(t - offsets[r] + k) mod L, c, n]; with a table, where that word
 *                                  is a NaN, climatology[(t - offsets[r] + k) mod period, c, n]; with mask_channel != 0
 *                                  C' = C + 1 and X[0,r,C,n,k] = 1.0f where no channel of that row at node n is a NaN,
 *                                  else 0.0f.  Every other word keeps its bits.  16-byte aligned.
 *       H [1], D [1] int64         floor(t / tau) mod 24 and floor(t / tau / 24) mod 7
 *     offsets [R] int64 on the device as for msgat_window_gather; the caller sees to L >= their largest and decides
 *     whether a ring that holds fewer readings may be forecast from.  climatology_or_null [period, C, N] or NULL: NULL is
 *     the plain form (no substitution; mask_channel must be 0, period is ignored).
 *     A NULL pointer (other than the table): MSGAT_ERR_NULL; R, C, N, L <= 0, L not a multiple of tau, period < 1 with a
 *     table, mask_channel without one: MSGAT_ERR_SHAPE; tau not in {4, 8, 12, 16} or (C + 1) * N above 2^31 - 256:
 *     MSGAT_ERR_UNSUPPORTED. */
int msgat_ring_push(const float* raw, const float* mean, const float* std, float* ring, int64_t* clock, int32_t K,
                    int32_t C, int32_t N, int64_t L, int32_t has_null, float null_value, void* stream);
int msgat_ring_windows(const float* ring, const float* climatology_or_null, const int64_t* clock, const int64_t* offsets,
                       float* X, int64_t* H, int64_t* D, int32_t R, int32_t C, int32_t N, int64_t L, int32_t tau,
                       int32_t period, int32_t mask_channel, void* stream);

/* ---- device: online forecasts scored as their readings arrive (no counterpart in the reference, which scores a loader
 * over a series that exists in full: engine.py:66-70, metrics.py:20-35) ----
 * The forecast issued at origin o (= clock[0] when it is made) predicts the steps o .. o + T_out - 1; it is due at
 * horizon h when the reading of absolute step o + h arrives, and its truth is channel 0 of that RAW reading.  State, all
 * in device memory and never read back during a step:
 *       book      [P, N, out] fp32   P >= T_out; the forecast of origin o lives in row o mod P (the floor-mod of the
 *                                    ring above); out = T_out for a point head, Q * T_out, level-major, for Q levels
 *       issued    [P] int64          the origin each row was written for; a fresh book holds INT64_MIN = never.  A row
 *                                    counts for origin o only if issued[row] == o and o >= 0.
 *       sums      [T_out + 1, W] fp64  running totals, zeroed by the caller.  W = 5 for a point head (Q = 0, levels may be
 *                                    NULL), 7 + 2Q for Q levels.  Row t < T_out: horizon t; row T_out: all horizons.
 *                                    Columns 0-3: the masked tail's {valid count, sum |e|, 100 sum_{y > mask_value} |e / y|,
 *                                    sum e^2} with e = p - y, p the point forecast (level `point` of a Q-level head);
 *                                    column 4: sum e, the signed error (serving has no loss; bias is what shows drift);
 *                                    Q levels: 5 crossing count, 6 width sum, 7 + q hits y <= p_q, 7 + Q + q sum rho_q,
 *                                    as msgat_quantile_metrics defines and computes them (fp32 per entry, fp64 sums).
 *       node_sums [N, 3] fp64        {valid count, sum |e|, sum e} per node over all horizons, zeroed by the caller
 * An entry is valid by the masked tail's rule: y is not NaN and, with has_null != 0, y != null_value.
 *
 * msgat_forecast_store: pred [N, out] moves, as 32-bit words, into row clock[0] mod P of book, and issued[row] = clock[0]:
 *     one launch.  Storing twice for one origin is idempotent.
 * msgat_forecast_score: raw [K, C, N] are the readings of the steps s + k, s = clock[0] -- enqueue it BEFORE the
 *     msgat_ring_push that advances the clock.  Two launches, no floating-point atomics, one fixed order for every sum:
 *     (1) a lane owns node n.  For k = 0 .. K-1 and, inside, h = 0 .. T_out-1: if origin o = s + k - h carries its stamp
 *         and y = raw[k, 0, n] is valid, the entry's W terms are formed in fp32 and widened to double (count 1, |e|,
 *         100 |e / y| or 0 where y <= mask_value, e * e in double, e, ...).  The lane adds count, |e| and e to its node totals
 *         in this k-then-h order, each starting from +0.0, and node_sums[n, :] += them at the end (one owner per node).  It
 *         adds every term to its slot partials[(c T_out + h) N + n], which starts as +0.0: the entries of a horizon in k order.
 *     (2) block c, column c: for every horizon the slots of nodes 64 b .. 64 b + 63 are added in node order from +0.0,
 *         those block sums in block order b from +0.0; sums[h, c] += the result, and sums[T_out, c] += the horizon results
 *         added in horizon order from +0.0.
 *     A numpy restatement in this order reproduces every bit.  partials: msgat_forecast_score_partial_doubles(N, T_out,
 *     Q) doubles (0 for arguments the entry point refuses).
 * Rows come from 64-bit floor-mods into [0, P): ANY clock content (cold, negative, a wild word) addresses rows inside book
 * and issued, and settles nothing unless the stamps match.
 * A NULL pointer (levels only when Q > 0): MSGAT_ERR_NULL.  K, C, N, T_out <= 0, Q < 0, P < T_out (store: N, out, P <= 0),
 * levels not strictly increasing inside (0, 1), NaN included, point outside [0, Q): MSGAT_ERR_SHAPE, before any launch.
 * Q > 8, max(Q, 1) * T_out > 64 or N above 2^31 - 256: MSGAT_ERR_UNSUPPORTED. */
int msgat_forecast_store(const float* pred, float* book, int64_t* issued, const int64_t* clock, int32_t N, int32_t out,
                         int64_t P, void* stream);
size_t msgat_forecast_score_partial_doubles(int32_t N, int32_t T_out, int32_t Q);
int msgat_forecast_score(const float* raw, const float* book, const int64_t* issued, const int64_t* clock, int32_t K,
                         int32_t C, int32_t N, int32_t T_out, int32_t Q, const float* levels, int32_t point, int64_t P,
                         int32_t has_null, float null_value, float mask_value, double* partials, double* sums,
                         double* node_sums, void* stream);

/* ---- device: calibrated prediction intervals for online forecasts (no counterpart in the reference) ----
 * Rolling split-conformal intervals around the point forecast: per series (n, h) the last W valid settled absolute errors
 * |p - y| are kept, and the half-width r of level l is one order statistic of that window.  It reads the scoring book above
 * (book, issued, clock: the same rows, stamps and validity rule) and keeps, in device memory, never read back in a step:
 *       window      [N, T_out, W] fp32       a ring per series
 *       cursor      [N, T_out] int32         c, taken as uint32: slot = c mod W, fill = min(c, W).  After an insert c + 1
 *                                            while c < W, else W + (slot + 1) mod W: any word stays inside its window.
 *       radius      [L, N, T_out] fp32       the current half-widths; +inf = no interval (a fresh state)
 *       radius_book [P, L, N, T_out] fp32    the radii issued with the forecast of origin o, in row o mod P; trusted under
 *                                            the book's test issued[row] == o && o >= 0 (a fresh one holds +inf)
 *       counts      [L, N, T_out, 2] int64   {judged, covered}, zeroed by the caller
 *       ranks       [L, W + 1] int32         ranks[l, m]: the 1-based order statistic used at fill m; 0 (or anything
 *                                            outside 1 .. m) = no interval.  Built once on the host: the policy is not here.
 * msgat_interval_update: raw [K, C, N] are the readings of the steps s + k, s = clock[0] -- enqueue it where
 *     msgat_forecast_score is, BEFORE the msgat_ring_push that advances the clock.  One launch, a wave per series, the
 *     window in registers.  For k = 0 .. K-1: if origin o = s + k - h carries its stamp and y = raw[k, 0, n] is valid,
 *     a = |p - y| in fp32 with p = book[row(o), n, point T_out + h] (the scorer's |e|).  First it is JUDGED: for every level
 *     whose issued radius r = radius_book[row(o), l, n, h] is finite, judged += 1 and covered += (a <= r) -- a NaN forecast
 *     counts as not covered.  Then, if a is finite, it is INSERTED at the cursor's slot and the cursor advances.  After the
 *     last k the changed slots and the cursor are written back and radius[l, n, h] = +inf for rank 0, else the
 *     ranks[l, fill]-th smallest of the slots below fill: exactly a window element, bit for bit (a radix select over the
 *     bit patterns, which order as unsigned integers because the inserted values are finite and non-negative).
 * msgat_interval_apply: after the forecast pred [N, out] of origin clock[0] exists (beside msgat_forecast_store): one launch
 *     over L N T_out elements, lo = p - r and hi = p + r (each one fp32 operation, p = pred[n, point T_out + h]), both
 *     [L, N, T_out], and r goes into row clock[0] mod P of radius_book.  Twice at one origin changes nothing.
 * Every cell has one owner: no reduction, no atomic.  Rows come from the 64-bit floor-mod of the scoring book: ANY clock
 * content reads and writes inside the books, and settles nothing unless the stamps match.
 * A NULL pointer: MSGAT_ERR_NULL.  K, C, N, T_out, out, L, W <= 0, P < T_out, out not a multiple of T_out or point outside
 * [0, out / T_out): MSGAT_ERR_SHAPE, before any launch.  L > 4, W > 1024, T_out > 64, out > 64 or N above 2^31 - 256:
 * MSGAT_ERR_UNSUPPORTED (apply takes no K, C, W). */
int msgat_interval_update(const float* raw, const float* book, const int64_t* issued, const int64_t* clock,
                          const float* radius_book, const int32_t* ranks, float* window, int32_t* cursor, float* radius,
                          int64_t* counts, int32_t K, int32_t C, int32_t N, int32_t T_out, int32_t out, int32_t point,
                          int64_t P, int32_t L, int32_t W, int32_t has_null, float null_value, void* stream);
int msgat_interval_apply(const float* pred, const float* radius, const int64_t* clock, float* lo, float* hi,
                         float* radius_book, int32_t N, int32_t T_out, int32_t out, int32_t point, int64_t P, int32_t L,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSGAT_HIP_H */
