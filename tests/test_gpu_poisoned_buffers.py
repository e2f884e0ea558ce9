"""GPU: no result of the library depends on what its buffers held before.

Every byte of device memory the library touches is allocated in Python (`torch.empty`, `torch.empty_like`; the C side never
allocates), and the kernels promise that none of it needs clearing first.  Every other test runs on whatever the caching
allocator hands back: a finish kernel that reads one partial more than this call wrote finds last call's (equal) partial
there, and an output element nobody writes is noticed only when the block happens to be dirty.  Here every case runs three
times with all its fresh allocations pre-filled with 0x00, 0xFF (NaN) and 0x7F (3.39e38) bytes (poison_fixtures.py) and must
give the same bits each time -- outputs and every gradient -- and finite numbers wherever the 0x00 run is finite.  No
tolerance: the library has no float atomics and fixed summation orders.

Cases: (a) the 75 rows of grad_subset_fixtures.ROWS with every subset of inputs and outputs that test_gpu_grad_subsets.py
runs (each subset selects other launches, null output pointers and other reductions, each with partials of its own), the
rows walked in a seeded shuffle under the second and third fill; (b) gacn, graph_attention and attention_core on a directed
graph with empty rows AND empty columns, a graph without an edge and a skewed one, at N = 13, 64 and 100, in all four
adjacency forms with the adjacency's gradient, the masked weights with a cotangent, the dense map with and without one;
(c) the four edge-weight ops on patterns with holes, one edge and none; (d) the step tail; (e) windows, ring and online
scoring; (f) FlatAdam in its four forms, built under the fill; (g) two optimizer steps of msgat48 through engine.Trainer,
model and Trainer built under the fill.  test_poisoned_buffers_cpu.py checks by `ast` that everything of ops.py that
allocates or launches is named by one of them, and that every site below is named here.

Every allocation that feeds the library (read before the first run on a GPU; csrc = ms_gat_amd/csrc), what is carved from
it and where it is written before it is read.  Outputs (z, y, dx, ... every `empty_like` of an input and every `_new`) are
fp32 and written whole by the launch they are handed to; the claims the tests hold them to are the ones about rows without
an edge, SELL pads, tail columns of N % 4 != 0, table rows nobody selected and null outputs.
  _GACNFunction.forward     z fp32 [G,Co|C,N,T]: the aggregate / project stage stores every row, +0 for one without an edge.
                            buf fp32, carved by _GacnPlan (64-float pieces: q, kW, lse, pq, E, Ec, u): each piece written by
                            the score stage (q, kW, lse, pq, E, Ec) or the projection (u) of the same forward; the pad
                            between pieces and the `max(nnz, 1)` slot of a graph without an edge are never read (nnz loops).
                            scratch_t fp32 (msgat_edge_scratch_floats: E in SELL order, pads included) written by the
                            score kernels' SELL store before the SELL aggregate reads it.  dense_t uint8
                            (msgat_dense_scratch_bytes: bf16 operand images of the dense column pass, 0 bytes below the
                            split-operand sizes): built by the pass's producer kernels first.
  _GACNFunction.backward    dx, dalpha, dWg, dW outputs.  ws uint8 = plan.bwd_bytes, api.hip plan_bwd's `align256` carve,
                            ALL fp32: dEp (per-edge partials per channel chunk, SELL positions + MSGAT_SELL_SLACK), gE, Ec,
                            delta [G,N], dkW, dq [G,N,T], dv (dy or du), dwg (dwg_partial_floats: one [T,T] per row block),
                            cp / cp2 (chanpair_partial_floats: one [Ca,Cb] per block of the contraction + 260 dump words),
                            dense (operand images).  Producer before consumer in stream order: SDDMM -> dEp, row pass ->
                            gE, delta, dkW, dq and the dwg partials, contraction -> cp; the reduce jobs (reduce.hip) sum
                            exactly the J partials the launcher reports (`nblk`), not the allocated count.
                            dy (AGG_FIRST with an adjacency gradient): msgat_stage_mix writes it whole.
  _AttentionCoreFunction    z, buf (no q, no u), dense_t, scratch (`_new`), du, dq, dWg, ws: as above (api.hip
                            attention_core_backward shares plan_bwd).
  _AdjacencyGrad            dadj fp32 [V,N,N]: msgat_adjacency_grad stores every element, off the pattern too.  ws uint8
                            (msgat_adjacency_grad_workspace_bytes) fp32 group-split partials, reduced over the split
                            count that wrote them.  dval fp32 [V, max(nnz,1)]: every stored edge written
                            (edge_weight_grad.hip:135); with nnz == 0 nothing is launched and the slice [:, :0] is
                            returned, the one slot never read.  ws uint8 (msgat_edge_weight_grad_sets_workspace_bytes,
                            V = 1 only) fp32 [nsplit, nnz], reduced over nsplit.
  _map_grad                 ws uint8 >= 256 B, attention_map.hip `mg_align` carve (64-float pieces), all fp32: dkW [G,N,T]
                            and r [G,N] written by k_map_grad_rows before k_map_grad_cols / k_map_grad_dwg read them, part
                            [G, chunks, T,T] written by k_map_grad_dwg before k_map_grad_dwg_sum sums Bg * chunks of them.
  _forward_weights          out fp32 [G,N,N]: msgat_attention_map stores the whole map (element by element where N % 4 != 0).
  _LayerNormTFunction, _LnPoolTeeFunction, layer_norm_t   y, dx, dw, db outputs (layer_norm_t's `empty_like` is the result
                            of an empty input); part fp32 (msgat_layernorm_partial_floats, _pool_: [R, blocks, 2T] (+ the
                            pooling's rows)): every block of the backward stores its partial, the reduce job sums `blocks`.
                            g, dpw, dyp: outputs of the pooling's own passes.
  _MixFunction, _MixMultiFunction, _TimeMixFunction, _CausalConvFunction, _NodePoolFunction, _ChannelPoolFunction,
  _HeadFunction, _LnHeadFunction   dx / dM / dy / dh / dw / dalpha / xn outputs; partials through `_new`, sized by the
                            matching msgat_*_partial_floats (contract, contract_segments, contract_mix, time_mix, node_pool,
                            head_forward, head_grad_weight, layernorm_head_backward): fp32, one per block, summed by a
                            reduce job over the block count of the same launch.
  _GateSumFunction          dpred, dh, dd outputs: a table row nobody selected is stored as zero (tail.hip).
  _ChannelAttentionMixFunction, _TemporalAttentionTapsFunction   dp, dWc, dconv / dW1, dW2 outputs; partials (`_new`,
                            msgat_channel_attention_partial_floats, msgat_temporal_attention_partial_floats) one per group,
                            summed over a relation's groups.
  _AssembleRowsFunction     rows fp32: both halves written by torch copies before anything reads it.
  _EdgeTimeWeights / _EdgeSignalWeights / _EdgeValidity / _EdgeDropout (`_new`)   out [B,nnz] written whole; dbase, dh, dd,
                            dab, dw: every row and every node written (+0 without an edge); nnz == 0 or V == 0 launches
                            nothing and `_shared_weight_grad` returns zeros.
  _TailMetricsFunction, _valid_slot   part float64 (msgat_huber / masked_huber / quantile_partial_doubles: per block 4, or
                            per block and horizon column), loss fp32 0-dim, the valid slot fp32 [1]: written by the first
                            launch, summed / read by the finish launch over the block count of the first; dpred output.
  forecast_score, OnlineForecaster   partials float64 (msgat_forecast_score_partial_doubles): written by the first of the
                            two launches, summed by the second.
  _window_gather, ring_windows   X, Y fp32 outputs, every element stored (imputed or not, mask channel included).
  FlatAdam._build           shadow fp32 [numel]: `reset_average()` copies the parameters into it before any step.
  SparsePattern             host int64 `_inverse`: assigned at every position by `_inverse[order] = arange` (order is a
                            permutation); the fp32 value buffer of `_perm` is filled by copy_ / index_select before the
                            library reads it.
  GraphAttention, GACN, StackedGACN, TemporalAttention, ChannelAttention, MSGAT   nn.Parameter(torch.empty(..)): initialised
                            by reset_parameters / the factory before use (torch ops, not the library).
The three INTEGER allocations, and why no poisoned integer reaches an index: `used` int64 [1] of _EdgeDropoutFunction is
written by the forward kernel (edge_dropout.hip:63) whenever anything is drawn and is read by the backward only then
(`if V and nnz`), as a Philox counter word, never as an index; HD int64 [2,B] of _window_gather and [2,1] of ring_windows
are outputs only (windows.hip:62-63, :128-129, online.hip:90-91), the library never reads them.  No byte workspace holds an
integer region: plan_bwd, mg_align and every *_workspace_bytes / *_partial_floats / *_partial_doubles size floats or
doubles, there is no ticket, counter or index in any of them (the only device counter, edge_values.hip `outside`, is the
caller's zero-initialised tensor).
"""
import copy
import functools
import random

import numpy as np
import pytest
import torch

from conftest import rel_err

import grad_subset_fixtures as gs
import graph_shape_fixtures as F
import poison_fixtures as pf
from ms_gat_amd import engine, model, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def _leaf(a, grad=True):
    return _dev(a).clone().requires_grad_(grad)


def _grads(*leaves):
    return tuple(None if t is None else t.grad for t in leaves)


def _detach(outs):
    return tuple(o.detach() if torch.is_tensor(o) else o for o in outs)


# ---- a. the op table -----------------------------------------------------------------------------------------------------

def _row_run(row, inputs, cots, subset, outsel=None):
    t = gs.leaves(inputs, subset, device=DEV)
    outs = tuple(row.lib(ops, t))
    sel = gs.differentiable(outs, outsel)
    if sel:
        torch.autograd.backward([outs[i] for i in sel], [cots[i].to(DEV) for i in sel])
    return _detach(outs), {k: t[k].grad for k in row.diff}


def _table_case(name):
    """Every run of one row: each subset of its inputs requiring grad (the full set among them), each subset of its outputs
    carrying a cotangent, and once nothing requiring grad"""
    row, inputs, cots = gs.problem(name)
    runs = {f"inputs {s}": _row_run(row, inputs, cots, s) for s in gs.subsets(row.diff)}
    runs.update({f"outputs {o}": _row_run(row, inputs, cots, row.diff, o) for o in row.out_subsets})
    runs["nothing requires grad"] = _row_run(row, inputs, cots, ())
    return runs


@functools.lru_cache(maxsize=None)
def _table():
    """{row: its runs under the three fills}: the rows in table order under the first fill and in a seeded shuffle under the
    other two, so that no result can depend on which shape ran before it (`_ones_cache`, the shift-tap, plan and graph
    caches) -- computed once, at the first row's test"""
    return pf.run_under_fills(_table_case, order=[r.name for r in gs.ROWS])


@pytest.mark.parametrize("name", [r.name for r in gs.ROWS], ids=gs.ROW_IDS)
def test_table_op_gives_the_same_bits_whatever_its_buffers_held(name):
    pf.check_fills(_table()[name], name)


# ---- b. the attention ops on graphs with holes ---------------------------------------------------------------------------
R, T = 2, 12
GRAPHS = ("holes", "empty", "skewed")
NODES = (13, 64, 100)          # 13: the map kernels store element by element; 100: N % 4 == 0 but N % 16 != 0
FORMS = ("dense", "sparse", "dense per sample", "sparse per sample")


@functools.lru_cache(maxsize=None)
def _adjacency(kind, N):
    """[N,N] fp32: `holes` a directed pattern with two rows and two columns without an entry, `empty` no entry at all,
    `skewed` graph_shape_fixtures' ladder (row i stores min(i, N - 1) entries, row 0 none); values as the fixtures draw them"""
    rng = F._rng(f"poisoned {kind}", N)
    if kind == "empty":
        return np.zeros((N, N), dtype=np.float32)
    if kind == "skewed":
        mask = F._ladder(N, rng, N - 1)
    else:
        mask = rng.random((N, N)) < 0.15
        mask[[1, N - 2], :] = False
        mask[:, [0, 5]] = False
        assert mask.any() and not mask[1].any() and not mask[:, 5].any()
    return F._values(mask, F._rng(f"poisoned {kind}", N, 1))


def _csr(adj):
    rows, cols = np.nonzero(adj)
    crow = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=adj.shape[0]))]).astype(np.int64)
    return crow, cols.astype(np.int64), adj[rows, cols]


def _attention_problem(op, kind, N, form, Tn):
    """-> (inputs as CPU tensors, the adjacency's values as a CPU tensor, how to make the adjacency from a leaf)"""
    Bg = 3 if "per sample" in form else 2
    G = R * Bg
    g = torch.Generator().manual_seed(1000 * N + 10 * GRAPHS.index(kind) + FORMS.index(form) + Tn)
    if op == "attention_core":
        ins = dict(u=torch.randn(G, 9, N, Tn, generator=g), q=torch.randn(G, N, Tn, generator=g),
                   Wg=torch.randn(R, Tn, Tn, generator=g) * 0.3)
    else:
        C, Co = (5, 9) if N == 13 else (40, 8)                  # AGG_FIRST and PROJ_FIRST (plain for graph_attention)
        ins = dict(x=torch.randn(G, C, N, Tn, generator=g), alpha=torch.randn(R, C, generator=g) * C ** -0.5,
                   Wg=torch.randn(R, Tn, Tn, generator=g) * 0.3)
        if op == "gacn":
            ins["W"] = torch.randn(R, Co, C, generator=g) * C ** -0.5
    adj = _adjacency(kind, N)
    crow, col, val = _csr(adj)
    if form == "dense":
        values, make = torch.from_numpy(adj), lambda v: v
    elif form == "dense per sample":
        scale = 1.0 + 0.25 * torch.arange(Bg, dtype=torch.float32).view(Bg, 1, 1)
        values, make = torch.from_numpy(adj)[None] * scale, lambda v: v
    else:
        crow_t, col_t = _dev(crow), _dev(col)
        values = torch.from_numpy(val)
        if form == "sparse per sample":
            values = values[None] * (1.0 + 0.25 * torch.arange(Bg, dtype=torch.float32).view(Bg, 1))
        make = lambda v: ops.edge_adjacency(crow_t, col_t, v)   # noqa: E731
    return ins, values, make, g


def _call(op, t, adj, **kw):
    if op == "gacn":
        return ops.gacn(t["x"], t["alpha"], t["Wg"], t["W"], adj, **kw)
    if op == "graph_attention":
        return ops.graph_attention(t["x"], t["alpha"], t["Wg"], adj, **kw)
    return ops.attention_core(t["u"], t["q"], t["Wg"], adj, **kw)


def _attention_case(op, kind, N, form, Tn=T):
    """Forward and backward with the adjacency's gradient; with the masked weights and a cotangent on them; the dense map
    without a gradient; the dense map with a cotangent on it (msgat_softmax_map_grad and its workspace)"""
    ins, values, make, g = _attention_problem(op, kind, N, form, Tn)
    runs = {}
    for what in ("plain", "masked", "softmax", "softmax_grad"):
        gen = torch.Generator().manual_seed(7)
        if what == "softmax":
            with torch.no_grad():
                z, w = _call(op, {k: _dev(v) for k, v in ins.items()}, make(_dev(values)), need_weights=True, weights="softmax")
            runs[what] = (z, w)
            continue
        t = {k: _leaf(v) for k, v in ins.items()}
        v = _leaf(values)
        if what == "plain":
            z, w = _call(op, t, make(v)), None
        else:
            z, w = _call(op, t, make(v), need_weights=True, weights=what)
        outs, cots = [z], [_dev(torch.randn(z.shape, generator=gen))]
        if w is not None:
            wd = w.to_dense() if w.layout != torch.strided else w
            outs.append(wd)
            cots.append(_dev(torch.randn(wd.shape, generator=gen)))
        torch.autograd.backward(outs, cots)
        runs[what] = (_detach(outs), {k: x.grad for k, x in t.items()}, v.grad)
    return runs


_ATTENTION = [(op, kind, N, form) for op in ("gacn", "graph_attention", "attention_core") for kind in GRAPHS for N in NODES
              for form in FORMS]


@pytest.mark.parametrize("op,kind,N,form", _ATTENTION, ids=[f"{o}-{k}-N{n}-{f.replace(' ', '_')}" for o, k, n, f in _ATTENTION])
def test_attention_on_a_graph_with_holes(op, kind, N, form):
    pf.check_fills(pf.run_under_fills(lambda: _attention_case(op, kind, N, form)), f"{op} {kind} N={N} {form}")


@pytest.mark.parametrize("op", ["gacn", "graph_attention", "attention_core"])
def test_attention_on_a_graph_with_holes_at_eight_timesteps(op):
    for form in ("dense", "sparse per sample"):
        pf.check_fills(pf.run_under_fills(lambda: _attention_case(op, "holes", 64, form, 8)), f"{op} holes N=64 {form} T=8")


# ---- c. the edge-weight ops ----------------------------------------------------------------------------------------------
# the patterns of test_gpu_edge_signal.py: a ring of 7 nodes, 65 nodes of which some have no out-edge, no in-edge or neither,
# a row and a column longer than a wave, one self loop (a single edge), five nodes without an edge (nnz == 0)
EDGE_PATTERNS = ("ring7", "holes65", "hub70", "loop1", "empty5")


@functools.lru_cache(maxsize=None)
def _edge_patterns():
    from test_gpu_edge_signal import PATTERNS, _csr as csr
    return {name: (PATTERNS[name]()[0],) + csr(*PATTERNS[name]())[:2] for name in EDGE_PATTERNS}


def _edge_case(op, pattern, B=3):
    n, crow, col = _edge_patterns()[pattern]
    nnz = col.size
    crow_t, col_t = _dev(crow.astype(np.int64)), _dev(col.astype(np.int64))
    g = torch.Generator().manual_seed(100 * n + len(op))
    runs = {}
    if op == "edge_time_weights":
        H, D = _dev(torch.randint(0, 24, (B,), generator=g)), _dev(torch.randint(0, 7, (B,), generator=g))
        ins = [torch.randn(nnz, generator=g), torch.randn(24, nnz, generator=g), torch.randn(7, nnz, generator=g)]
        dout = _dev(torch.randn(B, nnz, generator=g))
        for need in ((True, True, True), (True, False, False), (False, True, True)):
            leaves = [_leaf(t, on) for t, on in zip(ins, need)]
            out = ops.edge_time_weights(*leaves, H, D)
            out.backward(dout)
            runs[str(need)] = (out.detach(), _grads(*leaves))
    elif op == "edge_signal_weights":
        ins = [torch.randn(nnz, generator=g), torch.randn(B, n, 16, generator=g)]
        dout = _dev(torch.randn(B, nnz, generator=g))
        for need in ((True, True), (True, False), (False, True)):
            leaves = [_leaf(t, on) for t, on in zip(ins, need)]
            out = ops.edge_signal_weights(*leaves, crow_t, col_t)
            out.backward(dout)
            runs[str(need)] = (out.detach(), _grads(*leaves))
    elif op == "edge_dropout":
        exempt = _dev(torch.arange(nnz) % 3 == 0)
        dout = _dev(torch.randn(B, nnz, generator=g))
        for sets in (False, True):
            for ex in (None, exempt):
                state = ops.edge_dropout_state(77, DEV)        # a fresh stream per run: the three fills draw the same masks
                w = _leaf(torch.randn((B, nnz) if sets else (nnz,), generator=g))
                out = ops.edge_dropout(w, 0.25, state, exempt=ex, samples=None if sets else B)
                out.backward(dout)
                runs[f"sets={sets} exempt={ex is not None}"] = (out.detach(), w.grad, state.clone())
    else:
        val = _dev((torch.rand(B, n, 12, generator=g) < 0.7).float())
        val[0, 0] = 0.0
        exempt = _dev(torch.arange(nnz) % 3 == 0)
        dout = _dev(torch.randn(B, nnz, generator=g))
        for mode in ("scale", "drop", 7):
            for sets in (False, True):
                w = _leaf(torch.randn((B, nnz) if sets else (nnz,), generator=g))
                out = ops.edge_validity(w, val, crow_t, col_t, mode=mode, exempt=exempt if sets else None)
                out.backward(dout)
                runs[f"mode={mode} sets={sets}"] = (out.detach(), w.grad)
    return runs


@pytest.mark.parametrize("pattern", EDGE_PATTERNS)
@pytest.mark.parametrize("op", ["edge_time_weights", "edge_signal_weights", "edge_dropout", "edge_validity"])
def test_edge_weight_op(op, pattern):
    pf.check_fills(pf.run_under_fills(lambda: _edge_case(op, pattern)), f"{op} {pattern}")


# ---- d. the step tail ----------------------------------------------------------------------------------------------------
LEVELS = (0.1, 0.5, 0.9)
PLAIN_SHAPES = ((1,), (257,), (3, 7, 12))
HORIZON_SHAPES = ((1, 1), (257, 1), (3, 7, 12), (5, 11, 7))      # T = 12 and T = 7: (256 / T) * T < 256 leaves idle lanes


def _tail_case(kind, shape):
    g = torch.Generator().manual_seed(sum(shape) + len(kind))
    y = torch.randn(shape, generator=g) * 40 + 60
    t_out = shape[-1]
    if kind != "huber" and kind != "gauss":
        y[(torch.rand(shape, generator=g) < 0.2)] = 0.0         # missing readings
    if kind == "quantile":
        p = y.repeat(*([1] * (len(shape) - 1)), len(LEVELS)) + torch.randn(*shape[:-1], len(LEVELS) * t_out, generator=g) * 45
    else:
        p = y + torch.randn(shape, generator=g) * 45
    y = _dev(y)
    call = {"huber": lambda p, s: ops.huber_metrics(p, y, 50.0, 0.0, s),
            "gauss": lambda p, s: ops.gauss_metrics(p, y, 30.0, 0.05, 0.0, s),
            "masked_huber": lambda p, s: ops.masked_huber_metrics(p, y, 50.0, 0.0, 0.0, s),
            "masked_gauss": lambda p, s: ops.masked_gauss_metrics(p, y, 30.0, 0.05, 0.0, 0.0, s),
            "quantile": lambda p, s: ops.quantile_metrics(p, y, LEVELS, 0.0, 0.0, s)}[kind]
    totals = {"huber": (4,), "gauss": (4,), "masked_huber": (t_out + 1, 5), "masked_gauss": (t_out + 1, 5),
              "quantile": (t_out + 1, ops.QUANTILE_BASE_COLUMNS + 2 * len(LEVELS))}[kind]
    runs = {}
    for with_sums in (False, True):
        sums = torch.zeros(totals, device=DEV, dtype=torch.float64) if with_sums else None
        leaf = _leaf(p)
        loss = call(leaf, sums)
        loss.backward(torch.tensor(1.7, device=DEV))
        if with_sums:
            call(leaf.detach(), sums)                           # a second call adds to the totals
        runs[f"sums={with_sums}"] = (loss.detach(), leaf.grad, sums)
    return runs


_TAIL = [(k, s) for k in ("huber", "gauss") for s in PLAIN_SHAPES] + \
        [(k, s) for k in ("masked_huber", "masked_gauss", "quantile") for s in HORIZON_SHAPES]


@pytest.mark.parametrize("kind,shape", _TAIL, ids=[f"{k}-{'x'.join(map(str, s))}" for k, s in _TAIL])
def test_step_tail(kind, shape):
    pf.check_fills(pf.run_under_fills(lambda: _tail_case(kind, shape)), f"{kind} {shape}")


# ---- e. windows, ring and online scoring ---------------------------------------------------------------------------------
HOURS, TAU, Q = [1, 2], 4, 3


def _series(C=2, N=13, total=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    series = torch.randn(total, C, N, generator=g)
    series[torch.rand(total, C, N, generator=g) < 0.15] = float("nan")
    return series, torch.randn(5, C, N, generator=g), torch.randn(N, total, generator=g)


def _window_case():
    series, clim, target = (_dev(t) for t in _series())
    origins = _dev(torch.tensor([8, 9, 20, 37, 0, 100]))        # the last two are clamped by the kernel
    clean = torch.nan_to_num(series)
    runs = {"window_gather": ops.window_gather(clean, target, origins, HOURS, TAU, Q)}
    for mask in (False, True):
        runs[f"window_gather_imputed mask_channel={mask}"] = ops.window_gather_imputed(series, clim, target, origins, HOURS,
                                                                                        TAU, Q, mask_channel=mask)
    return runs


def test_window_gather():
    pf.check_fills(pf.run_under_fills(_window_case), "window_gather")


def _ring_case():
    C, N, L = 2, 13, 8
    series, clim, _ = _series(C, N, 30, seed=1)
    raw = _dev(series * 20 + 60)
    mean, std = _dev(torch.full((C, N), 60.0)), _dev(torch.full((C, N), 20.0))
    ring = torch.full((L, C, N), float("nan"), device=DEV)
    clock = torch.zeros(2, dtype=torch.int64, device=DEV)
    clim = _dev(clim)
    runs = {}
    for a, b in ((0, 8), (8, 9), (9, 12), (12, 19)):            # one step and several at a time, across the wrap
        ops.ring_push(raw[a:b].contiguous(), mean, std, ring, clock, null_value=float("nan"))
        runs[f"after {b} plain"] = ops.ring_windows(ring, clock, HOURS, TAU)
        for mask in (False, True):
            runs[f"after {b} imputed mask_channel={mask}"] = ops.ring_windows(ring, clock, HOURS, TAU, climatology=clim,
                                                                                mask_channel=mask)
    runs["ring"], runs["clock"] = ring, clock
    return runs


def test_ring_push_and_ring_windows():
    pf.check_fills(pf.run_under_fills(_ring_case), "ring")


def _score_case(levels):
    N, t_out, P, C = 13, 3, 4, 2
    out = max(len(levels), 1) * t_out
    g = torch.Generator().manual_seed(5 + len(levels))
    book = torch.zeros(P, N, out, device=DEV)
    issued = torch.full((P,), ops.SCORE_NEVER, dtype=torch.int64, device=DEV)
    clock = torch.zeros(2, dtype=torch.int64, device=DEV)
    sums = torch.zeros(t_out + 1, ops.score_columns(len(levels)), dtype=torch.float64, device=DEV)
    node_sums = torch.zeros(N, ops.SCORE_NODE_COLUMNS, dtype=torch.float64, device=DEV)
    ring = torch.zeros(8, C, N, device=DEV)
    stat = torch.ones(C, N, device=DEV)
    for step in range(7):
        K = 1 if step % 3 else 2
        raw = torch.randn(K, C, N, generator=g) * 20 + 60
        raw[torch.rand(K, C, N, generator=g) < 0.2] = 0.0
        raw = _dev(raw)
        ops.forecast_score(raw, book, issued, clock, t_out, sums, node_sums, levels=levels or None, null_value=0.0)
        ops.ring_push(raw, stat, stat, ring, clock)
        ops.forecast_store(_dev(torch.randn(N, out, generator=g) * 20 + 60), book, issued, clock)
    return dict(book=book, issued=issued, clock=clock, sums=sums, node_sums=node_sums)


@pytest.mark.parametrize("levels", [(), LEVELS], ids=["point", "quantile"])
def test_forecast_store_and_forecast_score(levels):
    pf.check_fills(pf.run_under_fills(lambda: _score_case(levels)), f"forecast_score levels={levels}")


# ---- f. the optimizer ----------------------------------------------------------------------------------------------------
ADAM_FORMS = {"plain": {}, "guarded": dict(max_grad_norm=0.5, skip_nonfinite=True), "averaged": dict(ema_decay=0.9),
              "accumulating": {}}


def _adam_case(form):
    from test_gpu_tail import _param_set
    params = _param_set(DEV)
    opt = engine.FlatAdam(params, lr=1e-3, weight_decay=5e-4, **ADAM_FORMS[form])     # its flat buffers are poisoned too
    g = torch.Generator(device=DEV).manual_seed(9)
    swapped = None
    for step in range(4):
        for micro in range(2 if form == "accumulating" else 1):
            for p in params:
                p.grad = torch.randn(p.shape, device=DEV, generator=g) * (0.1 + step)
            if step == 1:
                params[1].grad = None                           # torch's Adam skips a parameter without a gradient
            if form == "guarded" and step == 2:
                params[3].grad[17] = float("inf")               # the guard leaves this step out
            if form == "accumulating" and micro == 0:
                opt.accumulate(3.0)
        opt.step(rank_weight=5.0) if form == "accumulating" else opt.step()
        if form == "averaged" and step == 2:
            opt.swap_averaged()
            swapped = [p.detach().clone() for p in params]
            opt.swap_averaged()
    out = dict(params=[p.detach() for p in params], exp_avg=opt.exp_avg, exp_avg_sq=opt.exp_avg_sq, steps=opt._dev_steps,
               shadow=opt.shadow, swapped=swapped, guard=opt._guard)
    if form == "guarded":
        assert opt.guard_stats()["skipped_steps"] == 1
    return out


@pytest.mark.parametrize("form", list(ADAM_FORMS))
def test_flat_adam(form):
    pf.check_fills(pf.run_under_fills(lambda: _adam_case(form)), f"FlatAdam {form}")


# ---- g. a whole training step --------------------------------------------------------------------------------------------
# Tensors whose bits already differ between two runs under the SAME fill, and the torch op outside the library that causes it;
# they are held to 4x the distance between those two runs instead (a margin for a different rounding path).  Everything the
# library produces gets no such allowance.
NOT_REPRODUCIBLE = {}


def _numbers(obj):
    """Every number of a nested dict / list of floats, in a fixed order, as one float64 tensor"""
    if isinstance(obj, dict):
        return [x for k in sorted(obj) for x in _numbers(obj[k])]
    if isinstance(obj, (list, tuple)):
        return [x for v in obj for x in _numbers(v)]
    return [float(obj)] if isinstance(obj, (int, float)) else []


def _training_case(tmp_path, stack, hip_graph, everything):
    N, B, Rm, Tn = gs.MODEL_N, gs.MODEL_B, gs.MODEL_R, gs.MODEL_T
    import ms_gat_amd
    torch.manual_seed(7)
    gen = torch.Generator().manual_seed(11)
    adj = ms_gat_amd.synthetic_adjacency(N, N + 7, seed=5)
    cin = 2 if everything else 1
    extra = dict(learn_edge_weights="signal", edge_dropout=0.25, edge_dropout_seed=3, missing_edges="scale") if everything else {}
    net = model.msgat48(n_components=Rm, in_channels=cin, in_timesteps=Tn, out_timesteps=Tn * (len(LEVELS) if everything else 1),
                        use_te=True, adj=adj, **extra)
    batches = []
    for _ in range(2 * (2 if everything else 1)):
        X = torch.randn(B, Rm, cin, N, Tn, generator=gen)
        Y = torch.randn(B, N, Tn, generator=gen) * 40 + 60
        if everything:
            X[:, :, -1] = (torch.rand(B, 1, N, Tn, generator=gen) < 0.8).float()      # the validity channel, some missing
            Y[torch.rand(B, N, Tn, generator=gen) < 0.1] = 0.0
        batches.append([X, torch.randint(0, 24, (B,), generator=gen), torch.randint(0, 7, (B,), generator=gen), Y])
    net.to(DEV)
    net.stack_components = stack
    kw = dict(loss=engine.QuantileLoss(LEVELS, null_value=0.0), max_grad_norm=0.5, ema_decay=0.9, accumulate_steps=2) \
        if everything else {}
    tr = engine.Trainer(net, 50.0, str(tmp_path), hip_graph=hip_graph, **kw)
    per = len(batches) // 2
    losses, stats = [], []
    for k in range(2):                                          # two optimizer steps, an epoch each
        losses.append(tr.run_epoch(batches[k * per:(k + 1) * per], gpu_id=0, epoch=k + 1, mode="train"))
        stats.append(torch.tensor(_numbers(tr.last_stats), dtype=torch.float64))
    torch.cuda.synchronize()
    out = {"losses": torch.tensor(losses, dtype=torch.float64), "totals": torch.stack(stats)}
    out.update({n: p.detach().clone() for n, p in net.named_parameters()})
    if everything:
        out["shadow"] = tr.optimizer.shadow.clone()
    return out


_counter = [0]


@pytest.mark.parametrize("everything", [False, True], ids=["plain", "everything"])
@pytest.mark.parametrize("hip_graph", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("stack", [True, False], ids=["stacked", "loop"])
def test_two_training_steps(tmp_path, stack, hip_graph, everything):
    def run():
        _counter[0] += 1
        return _training_case(tmp_path / str(_counter[0]), stack, hip_graph, everything)
    with pf.device_errors_end_the_session(), pf.poisoned(pf.FILLS[0]):
        twin = run()
        torch.cuda.synchronize()
    results = pf.run_under_fills(run)
    assert float(results[0]["losses"].min()) > 0 and not pf.same_bits(results[0]["losses"][0], results[0]["losses"][1])
    failures = [f"{name}: not finite under the 0x00 fill" for name, t in results[0].items() if not bool(torch.isfinite(t).all())]
    for name, base in results[0].items():
        spread = rel_err(twin[name], base) if not pf.same_bits(twin[name], base) else 0.0
        if spread and name not in NOT_REPRODUCIBLE:
            failures.append(f"{name}: two runs under the 0x00 fill differ by {spread:.3e} and no torch op is named for it")
        for byte, r in zip(pf.FILLS[1:], results[1:]):
            if spread:
                e = rel_err(r[name], base)
                if not e <= 4 * spread:
                    failures.append(f"{name} ({NOT_REPRODUCIBLE.get(name)}): fill 0x{byte:02X} is {e:.3e} from the 0x00 run, two "
                                    f"0x00 runs are {spread:.3e} apart")
            else:
                failures += [f"{name} fill 0x{byte:02X}: {d}" for d in pf.differences(base, r[name])]
            failures += [f"{name} fill 0x{byte:02X}: {d}" for d in pf.nonfinite_where_finite(base, r[name])]
    assert not failures, "\n".join(failures[:40])
