"""GPU: the autograd contract of every torch.autograd.Function of ms_gat_amd/ops.py -- operands intact, backward repeatable.

Every other test runs an op once forward and once backward on tensors nobody else holds.  A loss with two terms, a
backward per forecast horizon, `retain_graph=True`, a cotangent that is a view of somebody's memory, two forwards before
the first backward: none of it was run, and a backward that uses a saved buffer or its cotangent as scratch, or per-call
state parked on the plan that every call with the same dimensions shares, would pass everything else.  Here
(autograd_contract_fixtures.py has the checks, test_autograd_contract_cpu.py shows without a GPU that each catches what it
is meant to and that the references alone meet the bars):

  (a) after the forward every input holds its bits, index tensors, tables and `state` included; after the backward so do the
      inputs, the outputs, every tensor the node saved (seen through saved_tensors_hooks) and every cotangent.
      Documented side effects, the only exemptions, each named where its case is built: `state` of edge_dropout (the
      forward moves the Philox stream one step on: ops.edge_dropout) and `sums` of the step tail (the forward adds the
      batch's sums to the caller's running fp64 totals: ops._TailMetricsFunction).  Neither is written by a backward.
  (b) two backwards of one forward give the same bits; a third with another cotangent gives the bits of a fresh forward +
      backward with it and meets the row's bar against float64; two backwards accumulated into .grad give twice one, and no
      two .grad share memory (AccumulateGrad keeps a gradient nobody else holds, and a view counts as such).
  (c) multi-output nodes, one backward per output, accumulated: the row's bar against float64 for all outputs together.
  (d) forward A, forward B (same shapes: the same cached plan and graph), then the backwards in either order: the bits of
      each run alone.
  (e) every cotangent layout autograd delivers, to every output of one row per Function: the bits of the contiguous run
      (autograd_contract_fixtures.FORM_ROWS says per Function why no strided form selects another kernel), no NaN from the
      neighbours of a channel slice, the cotangent's memory unchanged.
  (f) the five Functions outside the table, (g) every adjacency form with a gradient, stale state and cache eviction,
  (h) the whole model with a backward per horizon and two models interleaved.
No tolerance wherever bits are compared: the library has no float atomics and fixed summation orders.

What each Function saves, which library entry points its backward calls and which allocation OF THE SAME CALL every
non-const pointer receives (read before the first run on a GPU; ops = ms_gat_amd/ops.py).  No in/out parameter ever
receives a caller's tensor, a saved tensor or a cotangent: `dq_add` / `dWg_add` of msgat_softmax_map_grad get `dq_map` /
`dWg_map` (torch.zeros in _GACNFunction.backward) or the fresh `dq` / `dWg` of _AttentionCoreFunction.backward; `dadj` of
msgat_edge_softmax_grad gets the `dadj` that _AdjacencyGrad.__call__ allocated two lines above; `dx_add` of the LayerNorm
backward is read only (the second output's cotangent is ADDED into the fresh dx, never written).
  _GACNFunction           saves x, alpha, Wg, W and `buf` (q, kW, lse, pq, E, Ec, u carved by _GacnPlan, read through
                          plan.pointers); backward: msgat_gacn_backward / _edge_grad / _map_grad with a msgat_bwd_t whose dx,
                          dalpha, dWg, dW are empty_like and whose workspace is a fresh uint8 `ws`; dz is the cotangent,
                          read in place (contiguous, or a channel slice where accepted) or copied by _sliced_grad;
                          msgat_stage_mix -> fresh `dy`; _map_grad: dP copied if misaligned, fresh `ws`; the adjacency's
                          route (_AdjacencyGrad): msgat_adjacency_grad -> fresh dadj, ws; msgat_edge_weight_grad_sets ->
                          fresh dval, ws.  The plan (shared by every call with these dimensions on this graph) holds
                          dimensions, offsets and bwd_bytes only; its `keep` keeps the graph's device arrays alive.
  _AttentionCoreFunction  saves u, q, Wg, `buf` (no q, no u slot); backward: msgat_attention_backward / _edge_grad -> du, dq,
                          dWg empty_like, fresh ws; _map_grad adds into those fresh dq, dWg; the adjacency's route as above.
  _LayerNormTFunction     saves x, w; msgat_layernorm_backward -> dx, dw empty_like, db, part fresh.
  _LnPoolTeeFunction      saves x, y, pw, w, b; its second output is a view of x.  msgat_layernorm_backward_pooled /
                          msgat_layernorm_backward -> fresh dx, dw, db, dpw, rows_scratch, part; msgat_node_pool_grad_weight
                          -> fresh g, part; msgat_node_pool_grad_signal -> fresh dyp (dy is its read-only dx_add).  With only
                          the second output reaching the loss it hands dx_other straight back (threshold_backward makes a
                          new tensor for a ReLU input).
  _MixFunction            saves x, M, out (ReLU); threshold_backward / `.contiguous()` give dpre (the cotangent itself when
                          it is contiguous and there is no ReLU: read only, and handed back as the gradient of `add`);
                          msgat_stage_mix -> dx empty_like; msgat_stage_contract -> fresh part, dM; _channel_sums:
                          msgat_node_pool -> fresh pooled.
  _MixMultiFunction       saves M, the inputs, the outputs (ReLU not premasked); dpre as above, per output; msgat_mix_segments
                          -> fresh d_ins; msgat_contract_mix_segments / msgat_contract_segments -> fresh part, buf (and
                          d_ins[0]); the gradients of the add operands are views of dpre / cat(dpre).
  _TimeMixFunction        saves y, A; _as_segment reads the cotangent in place or copies; msgat_time_mix -> dy empty_like;
                          msgat_time_mix_grad_matrix -> fresh dAg, part; _channel_sums.
  _CausalConvFunction     saves h, taps; msgat_causal_conv -> dh empty_like; msgat_causal_conv_grad_weight -> fresh part, buf.
  _NodePoolFunction       saves x, w; msgat_node_pool_grad_signal -> dx empty_like; msgat_node_pool_grad_weight -> dw, part.
  _ChannelPoolFunction    saves x, alpha; msgat_stage_mix -> dx empty_like; msgat_stage_contract -> fresh part, dalpha.
  _HeadFunction           saves x, W; msgat_head_grad_signal -> dx empty_like; msgat_head_grad_weight -> fresh dWc, part;
                          msgat_node_pool -> fresh pooled (the bias gradient).
  _LnHeadFunction         saves x, W, xn (kept when W requires grad), w; msgat_layernorm_head_backward -> fresh dx, dlnw,
                          dlnb, part; the head's weight and bias gradients as _HeadFunction's.
  _GateSumFunction        saves pred, h_w, H, D, d_w; msgat_gate_sum_backward -> dpred, dh, dd empty_like.
  _ChannelAttentionMixFunction / _TemporalAttentionTapsFunction   save their inputs and att (and lr);
                          msgat_channel_attention_backward / msgat_temporal_attention_backward -> empty_like gradients, fresh part.
  _BiasJoinFunction, _AssembleRowsFunction, _Relayout   save nothing; hand out views or torch copies of the cotangent.
  _EdgeTimeWeightsFunction   saves H, D; msgat_edge_time_weights_backward -> fresh dbase, dh, dd.
  _EdgeSignalWeightsFunction saves ab, keeps the pattern's structure on ctx; msgat_edge_signal_weights_backward -> fresh dbase,
                          dab; a caller's order that is not the library's crosses by index_select (new tensors).
  _EdgeDropoutFunction    keeps exempt, state and a fresh `used` [1] on ctx (`used` holds the step the forward drew at, so a
                          backward redraws that mask whatever `state` holds by then); msgat_edge_dropout_backward -> fresh dw.
  _EdgeValidityFunction   saves validity, keeps exempt on ctx; msgat_edge_validity_backward -> fresh dw.
  _TailMetricsFunction    saves pred, truth and the valid slot (a fresh [1] per call unless the caller brings one);
                          msgat_*_grad -> dpred empty_like.
The entry points, every pointer parameter but `stream` (test_autograd_contract_cpu.py holds these lines against
include/msgat_hip.h: read only = const there, written = not const, nothing left out).  A `const msgat_seg_t*` is a read-only
array of descriptors; the memory behind the descriptors of `out` is written, behind those of `in`, `add` and `A` read:
  msgat_bwd_t                          read only: x, alpha, Wg, W, q, kW, lse, pq, E, u, dz, Ec; written: dx, dalpha, dWg, dW, workspace
  msgat_gacn_backward                  read only: shape, graph, io; written:
  msgat_gacn_backward_edge_grad        read only: shape, graph, io, dE_extra; written:
  msgat_gacn_backward_map_grad         read only: shape, graph, io, dq_map, dWg_map; written:
  msgat_attention_backward             read only: shape, graph, u, dv, q, kW, lse, pq, E, Ec, Wg; written: du, dq, dWg, workspace
  msgat_attention_backward_edge_grad   read only: shape, graph, u, dv, q, kW, lse, pq, E, Ec, Wg, dE_extra; written: du, dq, dWg, workspace
  msgat_softmax_map_grad               read only: shape, q, kW, lse, Wg, dP; written: dq_add, dWg_add, workspace
  msgat_adjacency_grad                 read only: shape, dv, feat, q, kW, lse; written: dadj, workspace
  msgat_edge_softmax_grad              read only: shape, graph, q, kW, lse, dE_extra; written: dadj, dval
  msgat_edge_weight_grad_sets          read only: shape, graph, dv, feat, q, kW, lse, dE_extra; written: dval, workspace
  msgat_stage_mix                      read only: shape, in, M, addvec, extra; written: out
  msgat_stage_contract                 read only: shape, A, Aextra, B; written: partials, dst0, dst1
  msgat_layernorm_backward             read only: x, weight, dy, dx_add; written: dx, dweight, dbias, partials
  msgat_layernorm_backward_pooled      read only: x, weight, bias, dy, dx_add, pool_w, dpooled; written: dx, dweight, dbias, dpool_w, dpool_rows, partials
  msgat_node_pool_grad_weight          read only: x, dpooled; written: dw, partials
  msgat_node_pool_grad_signal          read only: w, dpooled, dx_add; written: dx
  msgat_node_pool                      read only: x, w; written: pooled
  msgat_time_mix                       read only: src, A, bias; written: dst
  msgat_time_mix_grad_matrix           read only: dout, y; written: dA, partials
  msgat_causal_conv                    read only: src, taps, bias; written: dst
  msgat_causal_conv_grad_weight        read only: dout, h; written: partials, dtaps
  msgat_head_grad_signal               read only: dout, W; written: dx
  msgat_head_grad_weight               read only: dout, x; written: dWc, partials
  msgat_layernorm_head_backward        read only: dout, W, x, ln_weight; written: dx, dln_weight, dln_bias, partials
  msgat_gate_sum_backward              read only: dout, pred, H, D, h_w, d_w; written: dpred, dh_w, dd_w
  msgat_mix_segments                   read only: in, M, bias, add, out; written:
  msgat_contract_mix_segments          read only: A, B, M; written: partials, dst, mixout
  msgat_contract_segments              read only: A, B; written: partials, dst
  msgat_channel_attention_backward     read only: dMc, att, pooled, Wc, conv; written: dpooled, dWc, dconv, partials
  msgat_temporal_attention_backward    read only: dtaps, att, lr, pooled, Wt1, Wt2; written: dpooled, dWt1, dWt2, partials
  msgat_edge_time_weights_backward     read only: dout, H, D; written: dbase, dh_w, dd_w
  msgat_edge_signal_weights_backward   read only: graph, dout, ab; written: dbase, dab
  msgat_edge_dropout_backward          read only: dout, exempt, state, used; written: dw
  msgat_edge_validity_backward         read only: graph, dout, exempt, val, table; written: dw
  msgat_huber_grad                     read only: pred, truth, dloss; written: dpred
  msgat_gauss_grad                     read only: pred, truth, dloss; written: dpred
  msgat_masked_huber_grad              read only: pred, truth, dloss, valid; written: dpred
  msgat_masked_gauss_grad              read only: pred, truth, dloss, valid; written: dpred
  msgat_quantile_grad                  read only: pred, truth, dloss, valid, levels; written: dpred
"""
import functools

import numpy as np
import pytest
import torch

from conftest import assert_parity, elementwise_violations, record_err, rel_err

import autograd_contract_fixtures as ac
import edge_dropout_ref
import edge_validity_ref
import gauss_tail_ref
import grad_subset_fixtures as gs
import masked_tail_ref
import poison_fixtures as pf
import quantile_tail_ref
from oracle import dense_torch
from test_gpu_adjacency_grad import _case, _learned_adjacency

import ms_gat_amd
from ms_gat_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WHAT = "autograd_contract"
GUARD = pf.device_errors_end_the_session
ROW_NAMES = [r.name for r in gs.ROWS]


def _ok(found):
    assert not found, "\n".join(found[:40])


def _bar(bar, got, want, key, found):
    """The row's bar (grad_subset_fixtures: PARITY, or a max-norm bound) for one tensor; the error goes to the parity log"""
    if got is None or got.shape != want.shape or not bool(torch.isfinite(got).all()):
        found.append(f"{key}: no finite gradient of shape {tuple(want.shape)}")
        return
    e = rel_err(got, want)
    tol = 1e-4 if bar == gs.PARITY else bar[1]
    record_err(WHAT, key, e, tol)
    if not e < tol:
        found.append(f"{key}: rel err {e:.3e} >= {tol}")
    elif bar == gs.PARITY and elementwise_violations(got, want, 1e-4, 1e-5) != 0.0:
        found.append(f"{key}: entries outside 1e-4 |b| + 1e-5 max|b|")


# ---- the op table: cases (a) to (e) -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _shared_adjacency(n):
    """One device tensor per node count: every problem of a row hands the op the same adjacency object, hence the same
    cached graph and plan"""
    return gs._adjacency(n).to(DEV)


@functools.lru_cache(maxsize=None)
def _row_case(name, seed=0):
    row, inputs, cots = gs.problem(name, seed)
    inputs = dict(inputs)
    adj = inputs.pop("adj", None)

    def call(t):
        return row.lib(ops, t if adj is None else dict(t, adj=_shared_adjacency(adj.shape[0])))
    return ac.Case(gs.seed_name(name, seed), inputs, row.diff, call, cots, DEV, guard=GUARD)


@pytest.mark.parametrize("name", ROW_NAMES, ids=gs.ROW_IDS)
def test_table_op_leaves_its_operands_intact(name):
    case = _row_case(name)
    adj = gs.problem(name)[1].get("adj")
    before = None if adj is None else ac.snapshot(_shared_adjacency(adj.shape[0]))
    _ok(ac.check_operands_intact(case))
    if adj is not None:
        _ok(ac.changed(before, _shared_adjacency(adj.shape[0]), "the adjacency"))


@pytest.mark.parametrize("name", ROW_NAMES, ids=gs.ROW_IDS)
def test_table_op_backward_is_repeatable(name):
    row, _, other = gs.problem(name, 0, 1)
    found, third = ac.check_repeatable(_row_case(name), other)
    found += ac.check_accumulates(_row_case(name))
    want = gs.reference(name, row.diff, None, torch.float64, 0, 1)[1]
    for k in row.diff:
        _bar(row.bar, third[k], want[k], f"{name} third backward:d{k}", found)
    _ok(found)


MULTI_OUTPUT = [r.name for r in gs.ROWS if r.out_subsets or "with masked weights" in r.name]


@pytest.mark.parametrize("name", MULTI_OUTPUT, ids=[n.replace(" ", "_") for n in MULTI_OUTPUT])
def test_multi_output_op_one_output_at_a_time(name):
    row = gs.problem(name)[0]
    got = ac.check_one_output_at_a_time(_row_case(name))
    want = gs.reference(name, row.diff)[1]
    found = []
    for k in row.diff:
        _bar(row.bar, got[k], want[k], f"{name} one output at a time:d{k}", found)
    _ok(found)


def test_the_multi_output_rows_are_the_ones_meant():
    assert MULTI_OUTPUT == [n for n in ROW_NAMES if len(gs.problem(n)[2]) > 1]
    functions = {gs.problem(n)[0].function for n in MULTI_OUTPUT}
    assert functions == {"_LnPoolTeeFunction", "_MixMultiFunction", "_GACNFunction", "_AttentionCoreFunction"}


@pytest.mark.parametrize("name", ROW_NAMES, ids=gs.ROW_IDS)
def test_table_op_interleaved_with_a_second_problem(name):
    _ok(ac.check_interleaved(_row_case(name), _row_case(name, 1)))


FORM_ROW_NAMES = [v[0] for v in ac.FORM_ROWS.values()] + list(ac.FORM_ROWS_MORE)


@pytest.mark.parametrize("name", FORM_ROW_NAMES, ids=[n.replace(" ", "_") for n in FORM_ROW_NAMES])
def test_table_op_takes_every_cotangent_form(name):
    found, ran = ac.check_cotangent_forms(_row_case(name))
    assert ran >= 3 * len(gs.problem(name)[2])
    _ok(found)


def test_the_slice_paths_are_in_play():
    """What case (e) is about at N = 64: the library does read a channel slice in place there (else every form would be a
    copy first and the stride arguments would never be exercised)"""
    from ms_gat_amd import _lib
    import ctypes as C
    L = _lib.lib()
    for Cin, Co, N in ((72, 24, 64), (5, 9, 13)):
        graph = ms_gat_amd.graph.graph_of(_shared_adjacency(N))
        shape = _lib.Shape(gs.R, gs.BG, Cin, Co, N, 12)
        gstruct, keep = graph.on(DEV)
        accepted = L.msgat_bwd_accepts_strided_dz(C.byref(shape), C.byref(gstruct))
        print(f"gacn {Cin}->{Co} N={N}: a channel slice of dz is read in place: {bool(accepted)}")
        assert accepted == 1 or L.msgat_gacn_mode(Cin, Co) != _lib.MODE_AGG_FIRST       # aggregate-first always does (api.hip)
    dz = torch.zeros(4, 29, 64, 12, device=DEV)[:, 3:27]
    assert ops._sliced_grad(dz, lambda: True)[1] == 29 and ops._as_segment(dz)[1].group_stride == 29


# ---- (f) the five Functions outside the table --------------------------------------------------------------------------------
# Each builder -> (case, reference, bar): `reference(cots)` the gradients of the differentiable inputs for the CPU cotangents
# `cots`, from the op's own restatement; `bar(got, want)` -> an error message or None, the bar of the op's own test.

def _bits(got, want):
    want = torch.as_tensor(np.asarray(want)) if not torch.is_tensor(want) else want
    return None if pf.same_bits(got.cpu(), want.to(got.dtype)) else f"differs from the restatement's bits by {rel_err(got, want):.3e}"


def _rel(tol):
    return lambda got, want: None if rel_err(got, want) < tol else f"rel err {rel_err(got, want):.3e} >= {tol}"


def _edge_time(seed):
    """nnz = 65 (a second block that holds one edge), B = 3: the smallest shape of test_gpu_edge_time.py with more than one
    sample per table row.  The bar: out and the gradients are sums of at most B = 3 fp32 terms, each sum rounded once, so
    3 * 2^-24 = 1.8e-7 of the largest; 1e-6 is asked"""
    g = torch.Generator().manual_seed(300 + seed)
    nnz, B = 65, 3
    inputs = dict(base=torch.randn(nnz, generator=g), h_w=torch.randn(24, nnz, generator=g), d_w=torch.randn(7, nnz, generator=g),
                  H=torch.tensor([5, 23, 5]) if seed == 0 else torch.tensor([0, 7, 7]), D=torch.tensor([6, 0, 6]))
    cots = (torch.randn(B, nnz, generator=g),)

    def reference(cots):
        t = {k: inputs[k].double().requires_grad_(True) for k in ("base", "h_w", "d_w")}
        out = (t["base"] + t["h_w"][inputs["H"]]) + t["d_w"][inputs["D"]]
        return dict(zip(t, torch.autograd.grad(out, list(t.values()), cots[0].double())))
    case = ac.Case(f"edge_time_weights {seed}", inputs, ("base", "h_w", "d_w"),
                   lambda t: (ops.edge_time_weights(t["base"], t["h_w"], t["d_w"], t["H"], t["D"]),), cots, DEV, guard=GUARD)
    return case, reference, _rel(1e-6)


def _edge_signal(seed):
    """The ring of 7 nodes of test_gpu_edge_signal.py (in- and out-degrees up to 3) with every row's columns reversed, so
    that values and gradients cross the pattern's permutation; B = 3, d = 4.  The bar: dab sums at most 3 + 3 products
    of fp32 numbers and dbase B = 3 terms, every partial sum rounded once: 6 * 2^-24 = 3.6e-7 of the largest; 1e-5 is asked"""
    from test_gpu_edge_signal import PATTERNS, _csr as csr
    n, edges = PATTERNS["ring7"]()
    crow, col, row = csr(n, edges)
    perm = np.concatenate([np.arange(crow[i], crow[i + 1])[::-1] for i in range(n)])
    col, row = col[perm], row[perm]
    g = torch.Generator().manual_seed(400 + seed)
    B, d, nnz = 3, 4, len(col)
    inputs = dict(base=torch.randn(nnz, generator=g), ab=torch.randn(B, n, 2 * d, generator=g),
                  crow=torch.from_numpy(crow), col=torch.from_numpy(col))
    cots = (torch.randn(B, nnz, generator=g),)

    def reference(cots):
        base, ab = (inputs[k].double().requires_grad_(True) for k in ("base", "ab"))
        out = base + (ab[:, row, :d] * ab[:, col, d:]).sum(-1)
        return dict(zip(("base", "ab"), torch.autograd.grad(out, [base, ab], cots[0].double())))
    case = ac.Case(f"edge_signal_weights {seed}", inputs, ("base", "ab"),
                   lambda t: (ops.edge_signal_weights(t["base"], t["ab"], t["crow"], t["col"]),), cots, DEV, guard=GUARD)
    return case, reference, _rel(1e-5)


DROPOUT_SEED, DROPOUT_P = 77, 0.25


def _edge_dropout(seed, sets=False):
    """nnz = 5 (a partial quad) x V = 3, a weight shared by the samples or one per sample, some edges exempt; the stream
    starts at step 4 * seed.  `state` is exempt from (a) after the FORWARD: the op's documented side effect (it moves the
    stream one step on, ops.edge_dropout).  The bar: the bits of edge_dropout_ref.py"""
    g = torch.Generator().manual_seed(500 + seed + 10 * sets)
    V, nnz, step = 3, 5, 4 * seed
    exempt = torch.arange(nnz) % 3 == 0
    inputs = dict(w=torch.randn((V, nnz) if sets else (nnz,), generator=g), exempt=exempt,
                  state=torch.tensor([DROPOUT_SEED, step], dtype=torch.int64))
    cots = (torch.randn(V, nnz, generator=g),)

    def reference(cots, step=step):
        m = edge_dropout_ref.multipliers(DROPOUT_SEED, step, V, nnz, DROPOUT_P, exempt=exempt.numpy())
        back = edge_dropout_ref.backward_sets if sets else edge_dropout_ref.backward_shared
        return dict(w=torch.from_numpy(back(cots[0].numpy(), m)))
    case = ac.Case(f"edge_dropout sets={sets} {seed}", inputs, ("w",),
                   lambda t: (ops.edge_dropout(t["w"], DROPOUT_P, t["state"], exempt=t["exempt"], samples=None if sets else V),),
                   cots, DEV, guard=GUARD,
                   allowed={"state": "the forward moves the Philox stream {seed, step} one step on (ops.edge_dropout)"})
    return case, reference, _bits


def _edge_validity(seed, sets=False):
    """nnz = 257 on edge_validity_ref.pattern (a hub column, a self loop, nodes without an edge), V = 3, T = 12, "scale":
    the smallest of test_gpu_edge_validity.py with more than one block.  The bar: the bits of edge_validity_ref.py"""
    V, T, nnz = 3, 12, 257
    crow, col, N = edge_validity_ref.pattern(nnz, seed=seed)
    val = edge_validity_ref.validity(V, N, T, seed=seed)
    g = torch.Generator().manual_seed(600 + seed + 10 * sets)
    exempt = torch.arange(nnz) % 5 == 0
    inputs = dict(w=torch.randn((V, nnz) if sets else (nnz,), generator=g), validity=torch.from_numpy(val),
                  crow=torch.from_numpy(crow), col=torch.from_numpy(col), exempt=exempt)
    cots = (torch.randn(V, nnz, generator=g),)

    def reference(cots):
        back = edge_validity_ref.backward_sets if sets else edge_validity_ref.backward_shared
        return dict(w=torch.from_numpy(back(cots[0].numpy(), val, col, "scale", exempt.numpy())))
    case = ac.Case(f"edge_validity sets={sets} {seed}", inputs, ("w",),
                   lambda t: (ops.edge_validity(t["w"], t["validity"], t["crow"], t["col"], mode="scale", exempt=t["exempt"]),),
                   cots, DEV, guard=GUARD)
    return case, reference, _bits


LEVELS = (0.1, 0.5, 0.9)
SUMS = "the forward adds the batch's sums to the caller's running fp64 totals (ops._TailMetricsFunction)"


def _tail(kind, seed):
    """[3,7,12] (252 entries, T_out = 12: the per-horizon columns) with missing readings; running totals handed in.  `sums`
    is exempt from (a) after the FORWARD: the op's documented side effect.  Bars, each its own test's: huber 1e-6 (max norm,
    test_gpu_tail.py), masked 1e-5 per entry (test_gpu_masked_tail.py), gauss grad_violations == 0
    (gauss_tail_ref.py), quantile the bits of quantile_tail_ref.dpred_fp32"""
    shape, delta, sigma = (3, 7, 12), 50.0, 30.0
    dloss = torch.tensor(0.75 if seed == 0 else 1.7)
    if kind == "quantile":
        pred, truth = quantile_tail_ref.make_inputs(21, 12, LEVELS, seed=70 + seed)
    elif kind == "gauss":
        pred, truth = gauss_tail_ref.make_inputs(shape, 80 + seed, 45.0, n_equal=3)
    elif kind == "masked_gauss":
        pred, truth = gauss_tail_ref.make_inputs(shape, 85 + seed, 45.0, null_fraction=0.2, n_nan=3, n_equal=3)
    else:
        pred, truth = masked_tail_ref.make_inputs(shape, 90 + seed, delta, null_fraction=0.0 if kind == "huber" else 0.2,
                                                  n_nan=0 if kind == "huber" else 3)
    totals = {"huber": (4,), "gauss": (4,), "masked": (13, 5), "masked_gauss": (13, 5), "quantile": (13, ops.QUANTILE_BASE_COLUMNS + 2 * len(LEVELS))}[kind]
    inputs = dict(pred=pred, truth=truth, sums=torch.full(totals, 3.0, dtype=torch.float64))
    call = {"huber": lambda t: ops.huber_metrics(t["pred"], t["truth"], delta, 0.0, t["sums"]),
            "gauss": lambda t: ops.gauss_metrics(t["pred"], t["truth"], sigma, 0.05, 0.0, t["sums"]),
            "masked": lambda t: ops.masked_huber_metrics(t["pred"], t["truth"], delta, 0.0, 0.0, t["sums"]),
            "masked_gauss": lambda t: ops.masked_gauss_metrics(t["pred"], t["truth"], sigma, 0.05, 0.0, 0.0, t["sums"]),
            "quantile": lambda t: ops.quantile_metrics(t["pred"], t["truth"], LEVELS, 0.0, 0.0, t["sums"])}[kind]

    def reference(cots):
        d = float(cots[0])
        if kind == "huber":
            p = pred.double().requires_grad_(True)
            return dict(pred=torch.autograd.grad(dense_torch.huber(p, truth.double(), delta), p, cots[0].double())[0])
        if kind == "gauss":
            return dict(pred=gauss_tail_ref.restate(pred, truth, sigma, 0.05, None, dloss=d)["dpred"])
        if kind == "masked_gauss":
            return dict(pred=gauss_tail_ref.restate(pred, truth, sigma, 0.05, 0.0, dloss=d)["dpred"])
        if kind == "masked":
            return dict(pred=masked_tail_ref.restate(pred, truth, delta, 0.0, dloss=d)["dpred"])
        valid = quantile_tail_ref.restate(pred, truth, LEVELS, 0.0)["valid"]
        return dict(pred=quantile_tail_ref.dpred_fp32(pred, truth, LEVELS, 0.0, valid, dloss=d))

    def per_entry(got, want):
        bad = (got.double().cpu() - want).abs() > 1e-5 * want.abs()
        return f"{int(bad.sum())} entries outside 1e-5 |b|" if bool(bad.any()) else None

    def gauss_bar(got, want):
        n, worst = gauss_tail_ref.grad_violations(got, want)
        return f"{n} entries outside 1e-5 |b| + 1e-7 max|b| (worst {worst:.3e})" if n else None
    bar = {"huber": _rel(1e-6), "gauss": gauss_bar, "masked_gauss": gauss_bar, "masked": per_entry, "quantile": _bits}[kind]
    case = ac.Case(f"{kind} tail {seed}", inputs, ("pred",), lambda t: (call(t),), (dloss,), DEV, guard=GUARD, allowed={"sums": SUMS})
    return case, reference, bar


OTHER = {"edge_time_weights": _edge_time, "edge_signal_weights": _edge_signal, "edge_dropout shared": _edge_dropout,
         "edge_dropout sets": functools.partial(_edge_dropout, sets=True), "edge_validity shared": _edge_validity,
         "edge_validity sets": functools.partial(_edge_validity, sets=True),
         "huber tail": functools.partial(_tail, "huber"), "gauss tail": functools.partial(_tail, "gauss"),
         "masked tail": functools.partial(_tail, "masked"), "masked_gauss tail": functools.partial(_tail, "masked_gauss"),
         "quantile tail": functools.partial(_tail, "quantile")}


def test_the_other_cases_cover_the_functions_outside_the_table():
    assert set(ac.OTHER_FUNCTIONS) == set(gs.EXCLUDED)
    assert {k.split()[0] for k in OTHER} >= {"edge_time_weights", "edge_signal_weights", "edge_dropout", "edge_validity",
                                             "huber", "gauss", "masked", "masked_gauss", "quantile"}


@pytest.mark.parametrize("which", list(OTHER), ids=[k.replace(" ", "_") for k in OTHER])
def test_other_function_contract(which):
    """Cases (a), (b) and (d) for a Function outside the table, and the first backward against the op's own restatement"""
    (a, reference, bar), (b, _, _) = OTHER[which](0), OTHER[which](1)
    found = ac.check_operands_intact(a)
    if a.allowed:                                # the documented side effect did happen, and it is the only one
        step = ac.forward(a)
        moved = [k for k in a.allowed if not pf.same_bits(step.leaves[k].cpu(), a.inputs[k])]
        assert moved == list(a.allowed), moved
    repeat, third = ac.check_repeatable(a, b.cots)
    found += repeat + ac.check_accumulates(a)
    first = ac.alone(a)[1]
    for what, got, want in (("first", first, reference(a.cots)), ("third", third, reference(b.cots))):
        for k in a.diff:
            message = bar(got[k], want[k])
            if message:
                found.append(f"{a.name}: {what} backward d{k}: {message}")
    found += ac.check_interleaved(a, b)
    forms, ran = ac.check_cotangent_forms(a)
    assert ran >= 3
    _ok(found + forms)


@pytest.mark.parametrize("sets", [False, True], ids=["shared", "sets"])
def test_edge_dropout_backward_redraws_the_mask_of_its_own_forward(sets):
    """Two forwards on ONE state tensor (steps 0 and 1), a third after the first backward: every backward of the first
    call redraws the mask of step 0 -- the restatement's bits -- whatever the stream has moved on to, and the second
    call's backward that of step 1"""
    case, reference, bar = _edge_dropout(0, sets)
    with GUARD():
        t = case.leaves()
        cot = case.cotangents()[0]
        first = case.call(t)[0]
        second = case.call(t)[0]
        assert t["state"].tolist() == [DROPOUT_SEED, 2] and not pf.same_bits(first, second)
        grads = [torch.autograd.grad(first, t["w"], cot, retain_graph=True)[0]]
        third = case.call(t)[0]
        grads.append(torch.autograd.grad(first, t["w"], cot, retain_graph=True)[0])
        g_second = torch.autograd.grad(second, t["w"], cot)[0]
        grads.append(torch.autograd.grad(first, t["w"], cot)[0])
        torch.cuda.synchronize()
    assert t["state"].tolist() == [DROPOUT_SEED, 3] and third.shape == first.shape
    for g in grads:
        assert bar(g, reference(case.cots, 0)["w"]) is None
    assert bar(g_second, reference(case.cots, 1)["w"]) is None and not pf.same_bits(g_second, grads[0])


# ---- (g) adjacency forms with a gradient ---------------------------------------------------------------------------------------
N, T, B = 64, 12, 2
MODES = {"proj_first": (72, 24), "agg_first": (3, 24)}
ADJACENCY = [("proj_first", form) for form in ac.ADJACENCY_FORMS] + [("agg_first", "nn"), ("agg_first", "edge")]
KEYS = dict(x="dx", alpha="dalpha", Wg="dWg", W="dW", leaf="dadj")


class _Adjacency:
    """One (mode, form, seed): `case` with the adjacency's values as the leaf `leaf` -- the dense tensor, the stored values
    of the sparse forms, the weights of an edge_adjacency with every row's columns DEscending (values and gradients cross
    SparsePattern's permutation and its one shared buffer) -- and the float64 reference at any values of it"""

    def __init__(self, mode, form, seed=0):
        C, O = MODES[mode]
        self.form = form
        x, dz, Wg, alpha, W = _case(B, C, O, N, T, seed=seed + C + O)
        adj = _learned_adjacency(N, seed=17, V=B if form in ("bnn", "edge sets") else None)      # one pattern for both seeds
        if seed:
            adj = adj * np.random.default_rng(seed).uniform(0.5, 1.5, adj.shape).astype(np.float32)
        self.arrays, self.dz = (x, alpha, Wg, W), dz
        index = {}
        if form in ("nn", "bnn"):
            leaf = adj
        elif form == "1nn":
            leaf = adj[None]
        else:
            union = (adj != 0).any(0) if adj.ndim == 3 else adj != 0
            if form in ("edge", "edge sets"):
                crow, self.rows, self.cols = ac.reversed_rows(union)
            else:
                self.rows, self.cols = np.nonzero(union)
                crow = np.concatenate([[0], np.cumsum(np.bincount(self.rows, minlength=N))])
            leaf = adj[..., self.rows, self.cols]
            if form == "coo":
                index = dict(idx=torch.from_numpy(np.stack([self.rows, self.cols])))
            else:
                index = dict(crow=torch.from_numpy(crow.astype(np.int64)), col=torch.from_numpy(self.cols.astype(np.int64)))
        inputs = dict(x=torch.from_numpy(x), alpha=torch.from_numpy(alpha), Wg=torch.from_numpy(Wg), W=torch.from_numpy(W),
                      leaf=torch.from_numpy(np.ascontiguousarray(leaf)), **index)
        self.case = ac.Case(f"gacn {mode} adjacency {form} {seed}", inputs, ("x", "alpha", "Wg", "W", "leaf"), self.call,
                            (torch.from_numpy(dz),), DEV, guard=GUARD)

    def adjacency(self, t):
        if self.form == "csr":
            return torch.sparse_csr_tensor(t["crow"], t["col"], t["leaf"], (N, N))
        if self.form == "coo":
            return torch.sparse_coo_tensor(t["idx"], t["leaf"], (N, N))
        if self.form in ("edge", "edge sets"):
            return ops.edge_adjacency(t["crow"], t["col"], t["leaf"])
        return t["leaf"]

    def call(self, t):
        return (ops.gacn(t["x"], t["alpha"], t["Wg"], t["W"], self.adjacency(t)),)

    def dense(self, leaf):
        """the dense adjacency [N,N] / [V,N,N] the values `leaf` (a tensor) stand for"""
        v = leaf.detach().cpu().numpy()
        if self.form in ("nn", "bnn"):
            return v
        if self.form == "1nn":
            return v[0]
        a = np.zeros(v.shape[:-1] + (N, N), dtype=np.float32)
        a[..., self.rows, self.cols] = v
        return a

    def reference(self, leaf, dz=None, target=None):
        """-> {input name: float64 gradient} and z at the values `leaf`"""
        x, alpha, Wg, W = self.arrays
        want = ac.gacn_reference(x, alpha, Wg, W, self.dense(leaf), dz=dz, target=target, device=DEV)
        d = want["dadj"]
        want["dadj"] = d[None] if self.form == "1nn" else d if self.form in ("nn", "bnn") else d[..., self.rows, self.cols]
        return want

    def check(self, grads, want, what, found):
        for k, key in KEYS.items():
            try:
                assert_parity(grads[k], want[key].numpy(), f"{WHAT} {self.case.name} {what}", key)
            except AssertionError as err:
                found.append(str(err))


@pytest.mark.parametrize("mode,form", ADJACENCY, ids=[f"{m}-{f.replace(' ', '_')}" for m, f in ADJACENCY])
def test_adjacency_form_contract(mode, form):
    """Cases (a), (b), (d) with the adjacency's values among the differentiable inputs"""
    a, b = _Adjacency(mode, form), _Adjacency(mode, form, seed=1)
    found = ac.check_operands_intact(a.case)
    repeat, third = ac.check_repeatable(a.case, b.case.cots)
    found += repeat + ac.check_accumulates(a.case)
    a.check(third, a.reference(a.case.inputs["leaf"], dz=b.dz), "third backward", found)
    found += ac.check_interleaved(a.case, b.case)
    _ok(found)


def _factors(shape, seed):
    """test_gpu_adjacency_coherence.py's: a factor per entry, none inside [0.8, 1.25]"""
    rng = np.random.default_rng(seed)
    f = np.where(rng.random(shape) < 0.5, rng.uniform(0.3, 0.8, shape), rng.uniform(1.25, 3.0, shape)).astype(np.float32)
    return torch.from_numpy(f).to(DEV)


STALE = [(m, f, "values") for m, f in ADJACENCY] + [(m, f, "growth") for m, f in ADJACENCY if f in ("nn", "1nn", "bnn")]


@pytest.mark.parametrize("mode,form,write", STALE, ids=[f"{m}-{f.replace(' ', '_')}-{w}" for m, f, w in STALE])
def test_backward_after_the_adjacency_was_written_and_run_again(mode, form, write):
    """Forward A; the adjacency written in place under no_grad -- its values scaled, or (dense forms) every zero filled, so
    that the learned pattern grows and the graph is rebuilt; forward B on the same tensors; backward A; backward B.
    A's gradients are those of the values A's forward saw, B's of the new ones (conftest.assert_parity against float64).
    The loss is 0.5 |z - target|^2, as in test_gpu_adjacency_coherence.py and for its reason: with a fixed cotangent dadj
    would not depend on the adjacency's values.  Teeth on the reference alone: z and dadj move by more than 1e-2."""
    cell = _Adjacency(mode, form)
    case = cell.case
    target = case.cotangents()[0]
    leaves_of = lambda t: [t[k] for k in case.diff]          # noqa: E731
    with GUARD():
        t = case.leaves()
        zA = case.call(t)[0]
        cotA = zA.detach() - target
        old = t["leaf"].detach().clone()
        with torch.no_grad():
            if write == "values" and form == "csr":
                # torch's own node of sparse_csr_tensor saves the values and checks their version: the write that its
                # backward tolerates is the one through .data (an optimizer's kernels write through the address as well)
                t["leaf"].data.mul_(_factors(tuple(old.shape), 5))
            elif write == "values":
                t["leaf"].mul_(_factors(tuple(old.shape), 5))
            else:
                t["leaf"].mul_(1.5).add_((old == 0) * 0.05)
                assert bool((old == 0).any()) and bool((t["leaf"] != 0).all())
        new = t["leaf"].detach().clone()
        zB = case.call(t)[0]
        cotB = zB.detach() - target
        gA = dict(zip(case.diff, torch.autograd.grad(zA, leaves_of(t), cotA)))
        gB = dict(zip(case.diff, torch.autograd.grad(zB, leaves_of(t), cotB)))
        torch.cuda.synchronize()
    at_old, at_new = cell.reference(old, target=case.cots[0]), cell.reference(new, target=case.cots[0])
    for k in ("z", "dadj"):
        e = rel_err(at_old[k], at_new[k])
        assert e > 1e-2, f"the write moves {k} by {e:.3e} only, a stale read would pass"
    found = []
    for z, want, what in ((zA, at_old, "A"), (zB, at_new, "B")):
        try:
            assert_parity(z, want["z"].numpy(), f"{WHAT} {case.name} {write} {what}", "z")
        except AssertionError as err:
            found.append(str(err))
    cell.check(gA, at_old, f"{write} A (old values)", found)
    cell.check(gB, at_new, f"{write} B (new values)", found)
    _ok(found)


def test_backwards_after_more_forwards_than_the_graph_caches_hold():
    """20 forwards on 20 distinct frozen adjacencies at N = 13 -- more than the 16 entries of graph._GRAPHS -- then the 20
    backwards in reverse order: each holds the bits of its run alone (only `plan.keep` keeps an evicted graph's device
    arrays alive until its backward)"""
    from ms_gat_amd import graph
    name = "gacn AGG_FIRST 5->9 N=13"
    row, inputs, cots = gs.problem(name)
    assert graph._CACHE_MAX < 20
    cases, adjs = [], [ms_gat_amd.synthetic_adjacency(13, 13 + 7, seed=100 + i).to(DEV) for i in range(20)]
    for i, adj in enumerate(adjs):
        cases.append(ac.Case(f"{name} graph {i}", {k: v for k, v in inputs.items() if k != "adj"}, row.diff,
                             lambda t, adj=adj: row.lib(ops, dict(t, adj=adj)), cots, DEV, guard=GUARD))
    want = [ac.alone(c) for c in cases]
    assert not pf.same_bits(want[0], want[1])
    steps = [ac.forward(c) for c in cases]
    assert graph._GRAPHS.get(graph._tensor_key(adjs[0])) is None and graph._GRAPHS.get(graph._tensor_key(adjs[19])) is not None
    found = []
    for i in reversed(range(20)):
        got = (steps[i].outputs(), steps[i].backward())
        found += [f"graph {i}: {d}" for d in pf.differences(want[i], got, "(outputs, grads)")]
    _ok(found)


# ---- (h) the whole model ---------------------------------------------------------------------------------------------------------

def _model(seed, stack):
    net, X, H, D, dout = gs.model_problem("msgat48", 1, seed=seed)
    net.to(DEV)
    net.stack_components = stack
    return net, X.to(DEV), H.to(DEV), D.to(DEV), dout.to(DEV)


@pytest.mark.parametrize("stack", [True, False], ids=["stacked", "loop"])
def test_whole_model_one_backward_per_forecast_horizon(stack):
    """retain_graph=True and a backward per horizon, the gradients accumulated in .grad: float64 at the whole cotangent (its
    columns partition it), the bar of test_whole_model_with_part_of_it_frozen"""
    net, X, H, D, dout = _model(0, stack)
    with GUARD():
        pred = net(X, H, D)
        for t in range(gs.MODEL_T):
            column = torch.zeros_like(dout)
            column[..., t] = dout[..., t]
            pred.backward(column, retain_graph=t + 1 < gs.MODEL_T)
        torch.cuda.synchronize()
    want_pred, want, _ = gs.model_reference(net, X, H, D, dout, torch.float64, False)
    what = f"{WHAT} msgat48 per horizon {'stacked' if stack else 'loop'}"
    e = rel_err(pred, want_pred)
    record_err(what, "prediction", e, 1e-4)
    assert e < 1e-4
    found, worst = [], (0.0, None)
    for n, p in net.named_parameters():
        if n in want:
            if p.grad is None or not bool(torch.isfinite(p.grad).all()):
                found.append(f"{n}: no finite gradient")
                continue
            e = rel_err(p.grad, want[n])
            worst = max(worst, (e, n))
            if not e < 1e-4:
                found.append(f"{n}: rel err {e:.3e}")
    assert len(want) == sum(1 for p in net.parameters() if p.requires_grad) > 0
    spans = sorted((p.grad.data_ptr(), p.grad.data_ptr() + p.grad.numel() * 4, n) for n, p in net.named_parameters()
                   if p.grad is not None and p.grad.numel())
    found += [f"the .grad of {a[2]} and of {b[2]} share memory" for a, b in zip(spans, spans[1:]) if b[0] < a[1]]
    record_err(what, f"worst of {len(want)} gradients: {worst[1]}", worst[0], 1e-4)
    _ok(found)


@pytest.mark.parametrize("stack", [True, False], ids=["stacked", "loop"])
def test_two_models_interleaved(stack):
    """Two models of the same shapes on the same graph: forward A, forward B, backward B, backward A -- and the other
    order -- each with the bits of its step alone"""
    models = [_model(seed, stack) for seed in (0, 1)]

    def params(net):
        return [p for p in net.parameters() if p.requires_grad]

    def step_alone(net, X, H, D, dout):
        with GUARD():
            pred = net(X, H, D)
            grads = torch.autograd.grad(pred, params(net), dout)
            torch.cuda.synchronize()
        return ac.snapshot((pred.detach(), grads))
    want = [step_alone(*m) for m in models]
    assert not pf.same_bits(want[0][0], want[1][0])
    found = []
    for order in ((1, 0), (0, 1)):
        with GUARD():
            preds = [m[0](*m[1:4]) for m in models]
            grads = {}
            for i in order:
                grads[i] = torch.autograd.grad(preds[i], params(models[i][0]), models[i][4])
            torch.cuda.synchronize()
        for i in (0, 1):
            found += [f"model {i}, backwards in the order {order}: {d}"
                      for d in pf.differences(want[i], (preds[i].detach(), grads[i]), "(prediction, grads)")]
    _ok(found)
