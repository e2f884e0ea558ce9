"""Autograd binding of the HIP hot path.

`gacn(x, alpha, Wg, W, adjacency)` is the functional form of the reference's
`GACN.forward` (/root/reference/src/models/msgat.py:25-28) -- and of
`GraphAttention.forward` (src/models/attention.py:32-36) when `W is None` -- for
R stacked relations at once.  PyTorch only owns memory and streams here: every
arithmetic step runs in libmsgat_hip.so through the C ABI of include/msgat_hip.h.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import threading
from typing import Optional

import torch

from . import _lib
from ._lib import stream_handle as _stream_handle
from .graph import _dense_graph_for, edge_pattern_of, is_sparse_adjacency, sparse_graph_for, sparse_parts


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _require_device_tensor(name: str, t: torch.Tensor, device=None):
    if not t.is_cuda:
        raise _lib.MsgatError(
            f"{name} is on {t.device}: ms_gat_amd runs on MI355X (PyTorch-ROCm 'cuda' device) only; "
            "there is no CPU path -- the CPU oracle lives under oracle/ and is test infrastructure.")
    if t.dtype != torch.float32 and not (t.dtype in (torch.float16, torch.bfloat16) and torch.is_autocast_enabled("cuda")):
        # inside an autocast region (the reference's engine.py:54) half-precision outputs of neighbouring matmuls are
        # accepted and cast back to float32 at the op boundary (see _guard below)
        raise TypeError(f"{name} must be float32 (the reference arithmetic type), got {t.dtype}")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, expected {device}")


class _GacnPlan:
    """Everything of a GACN call that depends only on its dimensions, its graph and whether backward state is kept:
    the shape / graph structures handed to the library, the layout of the one buffer that carries what a forward saves
    (q, kW, lse, pq, E, E in CSC order, u), the sizes of the per-call scratch and the backward workspace size.  Built once
    per (graph, device, dims, need_bwd, own_q): the library queries and the offset arithmetic were ~10 us of host time per
    call.  own_q = False: the caller brings q (the attention core), the buffer has no slot for it."""
    __slots__ = ("shape", "gstruct", "keep", "mode", "sizes", "offs", "total", "bwd_bytes", "z_channels", "nscratch", "ndense")

    def __init__(self, graph, dev, R, Bg, Cin, Co, N, T, need_bwd, own_q=True):
        L = _lib.checked()
        G = R * Bg
        self.shape = _lib.Shape(R, Bg, Cin, Co, N, T)
        self.gstruct, self.keep = graph.on(dev)
        self.mode = L.msgat_gacn_mode(Cin, Co)
        nnz = max(graph.nnz, 1)
        if self.mode == _lib.MODE_PROJ_FIRST:
            n_u = G * Co * N * T
        elif self.mode == _lib.MODE_AGG_FIRST and need_bwd:
            n_u = G * Cin * N * T
        else:
            n_u = 0
        nscratch = int(L.msgat_edge_scratch_floats(C.byref(self.shape), C.byref(self.gstruct)))  # E in the SELL layout's order
        # (the SELL scratch is the forward's own workspace: allocated per call and dropped at its end, not carved from the
        # saved buffer -- it is at least the size of E and would stay resident until backward for every GACN layer)
        self.nscratch = nscratch
        # operand images of the score pass on large graphs (msgat_dense_scratch_bytes; 0 at PEMS sizes): per call as well
        self.ndense = int(L.msgat_dense_scratch_bytes(C.byref(self.shape)))
        self.sizes = (G * N * T if own_q else 0, G * N * T, G * N, G * N * T if need_bwd else 0, G * nnz, G * nnz if need_bwd else 0, n_u)
        offs, total = [], 0
        for n in self.sizes:                 # 256-byte aligned pieces
            offs.append(total if n else -1)
            total += (n + 63) & ~63
        self.offs, self.total = tuple(offs), max(total, 64)
        self.bwd_bytes = None                # asked for by the first backward
        self.z_channels = Co if Co else Cin

    def pointers(self, buf: torch.Tensor):
        """(q, kW, lse, pq, E, Ec, u): the device addresses of the pieces of the saved buffer `buf` (None: absent)."""
        base = buf.data_ptr()
        return tuple(None if o < 0 else base + 4 * o for o in self.offs)


def _gacn_plan(graph, dev, R, Bg, Cin, Co, N, T, need_bwd, own_q=True) -> _GacnPlan:
    # the plans live ON the graph object and die with it (a module-level table keyed by id(graph) kept every graph a
    # process had ever used, and its device tensors, alive)
    plans = graph.__dict__.get("_gacn_plans")
    if plans is None:
        plans = graph.__dict__["_gacn_plans"] = {}
    key = (dev.index, R, Bg, Cin, Co, N, T, need_bwd, own_q)
    plan = plans.get(key)
    if plan is None:
        if len(plans) > 256:
            plans.clear()
        plan = plans[key] = _GacnPlan(graph, dev, R, Bg, Cin, Co, N, T, need_bwd, own_q)
    return plan


# ---- an adjacency that requires grad ----------------------------------------------------------------------------------
# The adjacency tensor rides into the autograd Function as a last input, so that its gradient has somewhere to go; the
# graph is built from the tensor itself.  Whoever uses that gradient writes the tensor, and the writers that matter leave
# no trace on it: FlatAdam's kernels write through the address, a replay of a captured step runs no Python, `.data` skips
# the version counter.  So for a dense adjacency that requires grad the caches keep the pattern only, and every call --
# eager or captured -- refills the values from the tensor with one launch (graph._learned_graph_of); a sparse adjacency's
# values are read where they sit.  A frozen adjacency -- every caller of the reference's models -- costs one
# `requires_grad` check and is trusted by identity and version; a prebuilt SparseGraph / BatchedGraph is not a tensor
# and gets no gradient.

def edge_adjacency(crow: torch.Tensor, col: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """The sparse CSR adjacency [N,N] (N = crow.numel() - 1) with a learned weight per stored edge: `weight` [nnz] in
    the order of (crow, col), columns ascending inside a row.  Every op and module accepts it like any sparse adjacency;
    `weight` gets its gradient at the stored edges, dense [nnz], and a step that uses it can be captured in a HIP graph.
    `weight` [V,nnz] is a weight per stored edge AND per sample on the one shared pattern, V = the batch size (shared
    by stacked relations) or relations x batch size: a batched CSR adjacency [V,N,N] whose `to_dense()` is the
    reference's `adjacency: [..., n_nodes, n_nodes]`; `weight` gets a dense [V,nnz] gradient in its own order
    (msgat_edge_weight_grad_sets).  Contiguous weights in the library's order are read where they are.

    It is a CSR tensor on weight.detach() (the same storage: the library reads the current weights) that carries the
    weight itself as an attribute.  The ops hand the weight to their autograd Function: torch's own backward of
    `sparse_csr_tensor` densifies the gradient to [N,N] and reads the pattern back with `nonzero` (a host sync, which a
    captured step cannot contain), and adding the sparse gradients of several layers needs the pattern on the host too."""
    n = crow.numel() - 1
    if weight.dim() == 2:
        V = weight.shape[0]
        adj = torch.sparse_csr_tensor(crow.expand(V, -1), col.expand(V, -1), weight.detach(), (V, n, n))
        adj._msgat_edge_index = (crow, col)       # the pattern is keyed on these, not on torch's expanded views
    elif weight.dim() == 1:
        adj = torch.sparse_csr_tensor(crow, col, weight.detach(), (n, n))
    else:
        raise ValueError(f"weight must be [nnz] or [V, nnz], got {tuple(weight.shape)}")
    adj._msgat_edge_weight = weight
    return adj


class _AdjacencyGrad:
    """The gradient route of an adjacency that requires grad, built by `_resolve_adjacency`.  Called by backward with
    `(dv, feat, Cu)` and the saved q, kW, lse, it returns the gradient in the caller's own shape and layout: dense [N,N] /
    [V,N,N] from msgat_adjacency_grad (n_sets = V, the convention of `val_sets`), or from msgat_edge_weight_grad_sets at
    the stored entries of a sparse adjacency, [N,N] (n_sets = 1) or [V,N,N] (`pattern` a `graph.SparseSets`) -- dense
    [nnz] / [V,nnz] in input order for an `edge_adjacency` weight, else a sparse tensor with the caller's layout and
    indices.  Either is enqueued on `stream` after the backward of the other inputs."""

    def __init__(self, target: torch.Tensor, pattern=None, parts=None, sets: bool = False):
        self.shape, self.pattern, self.parts, self.sets = tuple(target.shape), pattern, parts, sets
        if pattern is None:
            self.n_sets = 1 if target.dim() == 2 else self.shape[0]
        else:
            self.n_sets = pattern.n_sets if sets else 1

    def __call__(self, plan: _GacnPlan, Cu: int, dv: torch.Tensor, dv_gs: int, feat: int, q: int, kW: int, lse: int,
                 stream, dE: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`dE` [G,nnz]: the gradient at the returned attention weights (`need_weights`), or None; its share
        sum_g P_g dE_g is added at the edges (msgat_edge_softmax_grad, inside the library for a sparse adjacency)."""
        L = _lib.checked()
        shape, dev = C.byref(plan.shape), dv.device
        gstruct = C.byref(plan.gstruct)
        if self.pattern is None:
            dadj = torch.empty((self.n_sets, plan.shape.N, plan.shape.N), device=dev, dtype=torch.float32)
            nbytes = int(L.msgat_adjacency_grad_workspace_bytes(shape, Cu, self.n_sets))
            ws = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
            L.msgat_adjacency_grad(shape, Cu, _ptr(dv), dv_gs, feat, q, kW, lse, self.n_sets, _ptr(dadj), _ptr(ws),
                                   nbytes, stream)
            if dE is not None:
                L.msgat_edge_softmax_grad(shape, gstruct, q, kW, lse, _ptr(dE), self.n_sets, _ptr(dadj), None, stream)
            return dadj.view(self.shape)
        # dval [n_sets, nnz] on the structure (the union of the samples' patterns), gathered back to the stored entries
        nnz = self.pattern.structure.nnz
        dval = torch.empty((self.n_sets, max(nnz, 1)), device=dev, dtype=torch.float32)
        nbytes = int(L.msgat_edge_weight_grad_sets_workspace_bytes(shape, gstruct, Cu, self.n_sets))
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
        L.msgat_edge_weight_grad_sets(shape, gstruct, Cu, _ptr(dv), dv_gs, feat, q, kW, lse, _ptr(dE), self.n_sets,
                                      _ptr(dval), _ptr(ws), nbytes, stream)
        dval = dval[:, :nnz]
        dval = self.pattern.to_input_order(dval if self.sets else dval.reshape(-1))
        if self.parts is None:                            # the weight [nnz] / [V,nnz] of an edge_adjacency
            return dval.view(self.shape)
        layout, idx = self.parts
        if layout == "csr":
            return torch.sparse_csr_tensor(idx[0], idx[1], dval.view(idx[1].shape), self.shape)
        return torch.sparse_coo_tensor(idx[0], dval, self.shape, is_coalesced=True)


def _resolve_adjacency(adjacency, device, groups: int, relations: int, n_nodes: int, recording: bool):
    """(graph, the tensor that receives the adjacency's gradient or None, its `_AdjacencyGrad` or None) for an op on
    signals of `groups` groups on `device`.  A sparse adjacency must be float32, [N,N] or [V,N,N], on the signals' device
    (`graph.sparse_graph_for` checks it); an uncoalesced COO tensor is coalesced (duplicates add, as in torch.sparse) --
    by an autograd op, so its gradient still reaches the caller's values.  For an `edge_adjacency` the tensor that
    receives the gradient is its weight.  Anything else goes through `graph.graph_for`."""
    target = route = None
    if is_sparse_adjacency(adjacency):
        if adjacency.device != device:
            raise ValueError(f"the sparse adjacency is on {adjacency.device}, the signals on {device}")
        if adjacency.layout == torch.sparse_coo and not adjacency.is_coalesced():
            adjacency = adjacency.coalesce()
        graph, pattern = sparse_graph_for(adjacency, groups, relations)
        if recording:
            weight = adjacency.__dict__.get("_msgat_edge_weight")
            target = adjacency if weight is None else weight
            if target.requires_grad:
                layout, idx, _ = sparse_parts(adjacency)
                parts = None if weight is not None else (layout, tuple(t.detach() for t in idx))
                route = _AdjacencyGrad(target, pattern, parts, sets=adjacency.dim() == 3)
            else:
                target = None
    else:
        graph = _dense_graph_for(adjacency, groups, relations, refuse_grad=False)
        if recording and getattr(adjacency, "requires_grad", False):
            target, route = adjacency, _AdjacencyGrad(adjacency)
    if graph.n_nodes != n_nodes:
        raise ValueError(f"adjacency has {graph.n_nodes} nodes, signals have {n_nodes}")
    return graph, target, route


# ---- reading the attention (need_weights) -----------------------------------------------------------------------------
# The forward keeps E = softmax(S) * A at the edges ([G,nnz], CSR order) and q, kW, lse, from which the dense softmax is
# re-created (msgat_attention_map).  "masked" hands out a copy of E as a sparse COO tensor on the graph's structure,
# differentiable (its gradient reaches the backward as an extra edge gradient); "softmax" the dense map, without one;
# "softmax_grad" the same dense map from the same launch, differentiable: its gradient dP [G,N,N] goes through
# msgat_softmax_map_grad, which re-creates P from q, kW, lse and hands back its share of dq and dWg (`_map_grad`).

_WEIGHT_FORMS = ("masked", "softmax", "softmax_grad")


def _check_weights(weights: str) -> str:
    if weights not in _WEIGHT_FORMS:
        raise ValueError(f"weights must be 'masked' or 'softmax' (or 'softmax_grad', the dense map with a gradient), "
                         f"got {weights!r}")
    return weights


def _map_grad(plan: _GacnPlan, q: int, kW: int, lse: int, Wg: torch.Tensor, dP: torch.Tensor, dq_add: torch.Tensor,
              dWg_add: torch.Tensor, stream) -> None:
    """dq_add [G,N,T] += and dWg_add [R,T,T] += the share of the gradient dP [G,N,N] at the dense map
    (msgat_softmax_map_grad), enqueued on `stream`."""
    L = _lib.checked()
    shape = C.byref(plan.shape)
    dP = dP.contiguous()
    if dP.data_ptr() % 16:                  # the row pass reads 16-byte pieces when N % 4 == 0
        dP = dP.clone()
    nbytes = int(L.msgat_softmax_map_grad_workspace_bytes(shape))
    ws = torch.empty(max(nbytes, 256), device=dP.device, dtype=torch.uint8)
    L.msgat_softmax_map_grad(shape, q, kW, lse, _ptr(Wg), _ptr(dP), _ptr(dq_add), _ptr(dWg_add), _ptr(ws),
                             ws.numel(), stream)


def _refuse_softmax_grad(*inputs) -> None:
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in inputs):
        raise ValueError("weights='softmax' has no gradient (the dense map is not differentiable here): ask for "
                         "weights='masked', whose values carry one, or run the call under torch.no_grad()")


def _weight_indices(graph, device, lead) -> torch.Tensor:
    """[len(lead) + 2, prod(lead) * nnz] int64: the coalesced COO indices of `lead` copies of the graph's edges in CSR
    (= row-major) order, cached on the structure."""
    structure = getattr(graph, "structure", graph)
    cache = structure.__dict__.setdefault("_weight_indices", {})
    key = (str(device), tuple(lead))
    idx = cache.get(key)
    if idx is None:
        nnz = structure.nnz
        edges = torch.stack([structure.erow[:nnz].long(), structure.col[:nnz].long()])          # [2,nnz], host
        G = 1
        for d in lead:
            G *= d
        groups = torch.arange(G).repeat_interleave(nnz)
        lead_idx, rest = [], groups
        for d in reversed(lead):
            lead_idx.insert(0, rest % d)
            rest = rest // d
        idx = torch.cat([torch.stack(lead_idx), edges.repeat(1, G)]).to(device)
        if len(cache) > 16:
            cache.clear()
        cache[key] = idx
    return idx


def _weights_out(w: torch.Tensor, graph, weights: str, lead) -> torch.Tensor:
    """The tensor handed to the caller: the sparse COO [*lead,N,N] of the edge values w [G,nnz] ("masked"), or the dense
    map w [G,N,N] viewed as [*lead,N,N] ("softmax", "softmax_grad")."""
    N = graph.n_nodes
    if weights != "masked":
        return w.view(*lead, N, N)
    return torch.sparse_coo_tensor(_weight_indices(graph, w.device, lead), w.reshape(-1), (*lead, N, N),
                                   is_coalesced=True)


def _forward_weights(weights, plan: _GacnPlan, nnz: int, buf: torch.Tensor, q: int, kW: int, lse: int,
                     stream) -> torch.Tensor:
    """After a forward: E copied out of the saved buffer (an in-place edit by the caller must not reach backward), or the
    dense softmax map from q, kW, lse."""
    shape = plan.shape
    G, N = shape.R * shape.Bg, shape.N
    if weights == "masked":
        return buf.narrow(0, plan.offs[4], G * nnz).view(G, nnz).clone()
    out = torch.empty((G, N, N), device=buf.device, dtype=torch.float32)
    _lib.checked().msgat_attention_map(C.byref(shape), q, kW, lse, _ptr(out), stream)
    return out


class _GACNFunction(torch.autograd.Function):
    """x[G,C,N,T], alpha[R,C], Wg[R,T,T], W[R,Co,C] or None -> z[G,Co|C,N,T];  G = R*Bg.  `adj`: the tensor that
    receives the adjacency's gradient and `adj_grad` its route (`_resolve_adjacency`), or None both."""

    @staticmethod
    def forward(ctx, x, alpha, Wg, W, graph, recording: bool = True, adj_grad=None, adj=None, weights=None):
        # graph: see graph_for.  weights: None, or "masked" / "softmax" / "softmax_grad" -- then a second output (see
        # _forward_weights), whose gradient arrives in backward as `dE`: [G,nnz] at the edges, or [G,N,N] at the dense map
        L = _lib.checked()
        dev = x.device
        G, Cin, N, T = x.shape
        R = alpha.shape[0] if alpha.dim() == 2 else 1     # alpha [C], Wg [T,T], W [Co,C]: ONE relation, no leading axis
        if G % R != 0:
            raise ValueError(f"{G} groups cannot be split over {R} relations")
        Co = 0 if W is None else W.shape[-2]
        # `needs_input_grad` is True under torch.no_grad() as well (it mirrors requires_grad); whether a graph is being
        # recorded is known only to the caller (inside forward grad mode is always off).  Inference then skips everything
        # backward alone needs: pq (4 of the 7 matrix-core instructions per score tile), E in CSC order, the saved y.
        # The FORM of the forward follows the grad mode alone: the score kernel that also forms pq takes its row sums
        # from the matrix core and rounds lse differently, so a form chosen by `needs_input_grad` would let a frozen
        # backbone change the bits of a prediction.  What is frozen decides only whether anything is saved.
        training_form = bool(recording)
        need_bwd = training_form and any(ctx.needs_input_grad)
        plan = _gacn_plan(graph, dev, R, G // R, Cin, Co, N, T, training_form)

        if not x.is_contiguous():
            x = x.contiguous()
        alpha, Wg = alpha.contiguous(), Wg.contiguous()
        W = None if W is None else W.contiguous()

        # Everything backward needs besides the inputs (q, kW, lse, pq, E, E in CSC order, the projected / aggregated
        # features u) and the SELL scratch lives in ONE allocation, addressed by offset: seven `torch.empty` calls
        # per forward were a quarter of its host time, which is what a PEMSD4-sized step is bound by.
        z = torch.empty((G, plan.z_channels, N, T), device=dev, dtype=torch.float32)
        buf = torch.empty(plan.total, device=dev, dtype=torch.float32)
        q, kW, lse, pq, E, Ec, u = plan.pointers(buf)
        scratch_t = torch.empty(plan.nscratch, device=dev, dtype=torch.float32) if plan.nscratch else None
        scratch = _ptr(scratch_t)
        dense_t = torch.empty(plan.ndense, device=dev, dtype=torch.uint8) if plan.ndense else None
        io = _lib.Fwd(_ptr(x), _ptr(alpha), _ptr(Wg), _ptr(W), _ptr(z), q, kW, lse, pq, E, u, int(training_form), scratch, Ec,
                      _ptr(dense_t))
        L.msgat_gacn_forward(C.byref(plan.shape), C.byref(plan.gstruct), C.byref(io), _stream_handle(dev))

        if need_bwd:
            ctx.plan, ctx.has_W, ctx.adj_grad, ctx.weights = plan, W is not None, adj_grad, weights
            if W is not None:
                ctx.save_for_backward(x, alpha, Wg, buf, W)
            else:
                ctx.save_for_backward(x, alpha, Wg, buf)
        if weights is None:
            return z
        ctx.set_materialize_grads(False)      # a weights output nobody differentiates arrives as None: the plain backward
        w = _forward_weights(weights, plan, graph.nnz, buf, q, kW, lse, _stream_handle(dev))
        if weights == "softmax":
            ctx.mark_non_differentiable(w)
        return z, w

    @staticmethod
    def backward(ctx, dz, dE=None):
        # All four gradients are computed whatever `ctx.needs_input_grad` says: they are by-products of shared passes, not
        # separate work.  PROJ_FIRST: dW, dalpha AND dx leave ONE launch that reads du, dq and x once
        # (msgat_stage_project_backward); AGG_FIRST: dW rides in the pass that forms dy, dalpha in the transposed aggregate
        # that forms dx; dWg is a [T,T] partial of the row pass that every other gradient needs.  The only input that
        # is ever frozen in the reference's models is none of these (adj, msgat.py:190), and x always requires one (it is
        # a LayerNorm output with learnable weights, msgat.py:122).  An adjacency that requires grad gets it from one more
        # launch after that backward (its `_AdjacencyGrad`), which re-creates the softmax from q, kW and lse:
        # dv / feat are dz / x (plain), dz / u = W x (project-first), W^T dz / x (aggregate-first, one more mix).
        L = _lib.checked()
        saved = ctx.saved_tensors
        x, alpha, Wg, buf = saved[:4]
        W = saved[4] if ctx.has_W else None
        plan = ctx.plan
        q, kW, lse, pq, E, Ec, u = plan.pointers(buf)
        dev = x.device
        shape, gstruct = plan.shape, plan.gstruct
        if dz is None:                        # only the attention weights reached the loss
            dz = torch.zeros((x.shape[0], plan.z_channels, shape.N, shape.T), device=dev, dtype=torch.float32)
        dP = None
        if dE is not None and ctx.weights == "softmax_grad":
            dP, dE = dE, None                 # the gradient at the dense map: att depends on neither W nor the adjacency
        if dE is not None:
            dE = dE.contiguous()
        # a gradient that arrives as a channel slice dout[:, a:b] of a wider tensor is read in place where the library
        # can (one 98 MB copy less per GACN at PEMSD7 size), copied otherwise
        dz, dz_gs = _sliced_grad(dz, lambda: L.msgat_bwd_accepts_strided_dz(C.byref(shape), C.byref(gstruct)))

        dx = torch.empty_like(x)
        dalpha = torch.empty_like(alpha)
        dWg = torch.empty_like(Wg)
        dW = None if W is None else torch.empty_like(W)
        if plan.bwd_bytes is None:
            plan.bwd_bytes = max(int(L.msgat_bwd_workspace_bytes(C.byref(shape), C.byref(gstruct))), 256)
        ws = torch.empty(plan.bwd_bytes, device=dev, dtype=torch.uint8)
        io = _lib.Bwd(_ptr(x), _ptr(alpha), _ptr(Wg), _ptr(W), q, kW, lse, pq, E, u, _ptr(dz), _ptr(dx), _ptr(dalpha),
                      _ptr(dWg), _ptr(dW), _ptr(ws), ws.numel(), dz_gs, Ec)
        stream = _stream_handle(dev)
        if dP is not None:
            # its share of dq and dWg first, on zeroed buffers; the backward adds them where dq and dWg are final, so that
            # dx and dalpha carry the map's term as well
            dq_map = torch.zeros((x.shape[0], shape.N, shape.T), device=dev, dtype=torch.float32)
            dWg_map = torch.zeros_like(Wg)
            _map_grad(plan, q, kW, lse, Wg, dP, dq_map, dWg_map, stream)
            L.msgat_gacn_backward_map_grad(C.byref(shape), C.byref(gstruct), C.byref(io), _ptr(dq_map),
                                           _ptr(dWg_map), stream)
        elif dE is None:
            L.msgat_gacn_backward(C.byref(shape), C.byref(gstruct), C.byref(io), stream)
        else:
            L.msgat_gacn_backward_edge_grad(C.byref(shape), C.byref(gstruct), C.byref(io), _ptr(dE), stream)
        if ctx.adj_grad is None:
            return dx, dalpha, dWg, dW, None, None, None, None, None
        Cin = x.shape[1]
        if plan.mode == _lib.MODE_AGG_FIRST:
            dy = torch.empty_like(x)
            dzc = dz if dz_gs == 0 else dz.contiguous()
            L.msgat_stage_mix(C.byref(shape), shape.Co, Cin, _ptr(dzc), _ptr(W), 1, None, None, _ptr(dy), stream)
            Cu, dv, dv_gs, feat = Cin, dy, 0, _ptr(x)
        elif plan.mode == _lib.MODE_PROJ_FIRST:
            Cu, dv, dv_gs, feat = shape.Co, dz, dz_gs, u
        else:
            Cu, dv, dv_gs, feat = Cin, dz, dz_gs, _ptr(x)
        return dx, dalpha, dWg, dW, None, None, None, ctx.adj_grad(plan, Cu, dv, dv_gs, feat, q, kW, lse, stream, dE), None


def gacn(x: torch.Tensor, alpha: torch.Tensor, Wg: torch.Tensor, W: Optional[torch.Tensor],
         adjacency, need_weights: bool = False, weights: str = "masked", _lead=None):
    """Graph attention (+ channel projection when `W` is given) over R stacked relations.

    x [R*Bg, C, N, T] (relation-major), alpha [R,C], Wg [R,T,T], W [R,Co,C] or None,
    adjacency: dense [N,N] tensor or a prebuilt `SparseGraph`; or a per-sample adjacency -- dense [Bg,N,N] (one graph per
    sample, shared by the R relations), [R*Bg,N,N] (one per group) or a prebuilt `BatchedGraph` of either ([1,N,N] is
    [N,N]; `graph.graph_for`).  Returns [R*Bg, Co|C, N, T].
    A dense adjacency tensor that requires grad gets its gradient, in its own shape: dense, non-zero off the edges too,
    since softmax(k Wg q^T) does not depend on it.  A prebuilt SparseGraph / BatchedGraph is not a tensor and gets none.
    A torch sparse COO / CSR [N,N] adjacency is its stored indices (explicit zeros included) with its values; one that
    requires grad gets the gradient at those indices only (msgat_edge_weight_grad), sparse with the same layout.  From
    there torch's own backward of the sparse constructor carries it to the values tensor, and that backward densifies
    the gradient to [N,N] and reads the pattern back with `nonzero` (a host sync): fine for small graphs in eager mode,
    but it cannot be captured in a HIP graph and costs N^2.  For learned edge weights at scale or under capture use
    `edge_adjacency(crow, col, weight)`, whose gradient reaches `weight` directly, dense [nnz].
    `need_weights=True` returns `(output, weights)` with the attention of every group, [R*Bg,N,N]:
    weights="masked" is the reference's `att * adjacency` (attention.py:36) as a coalesced sparse COO tensor on the
    graph's structure in row-major order (a dense adjacency's non-zeros, a sparse one's stored indices, a batched one's
    union pattern with explicit zeros), differentiable -- a loss on it reaches x, alpha, Wg and the adjacency;
    weights="softmax" is `att` (attention.py:34), the dense row softmax over all N columns before the mask, without a
    gradient (a ValueError if grad mode is on and an input requires grad); weights="softmax_grad" is the same dense
    map, bit for bit and from the same launch, as an ordinary autograd tensor: a loss on it -- an entropy or sparsity
    penalty on the rows, supervision against a flow matrix, distillation -- reaches x, alpha and Wg, and neither W nor
    the adjacency, on which `att` does not depend (msgat_softmax_map_grad re-creates the map from the saved q, kW, lse,
    so an in-place edit of the returned tensor does not reach backward).  `output` is the same in every form.
    One relation may come without the leading axis -- alpha [C], Wg [T,T], W [Co,C], the reference's own parameter
    shapes (attention.py:29-30, msgat.py:23): the module classes call it that way, so that no view nodes sit between
    the parameters and the op (three `unsqueeze` forward and three more nodes backward were a sixth of a call's host time).
    """
    if need_weights and _check_weights(weights) == "softmax":
        _refuse_softmax_grad(x, alpha, Wg, W, adjacency, getattr(adjacency, "_msgat_edge_weight", None))
    if x.dim() != 4:
        raise ValueError(f"signals must be [batch, channels, nodes, timesteps], got {tuple(x.shape)}")
    _require_device_tensor("signals", x)
    for name, t in (("alpha", alpha), ("Wg", Wg)) + ((("W", W),) if W is not None else ()):
        _require_device_tensor(name, t, x.device)
    G, Cin, N, T = x.shape
    if alpha.dim() == 1:                                  # one relation, the reference's parameter shapes
        if alpha.shape[0] != Cin:
            raise ValueError(f"alpha must be [{Cin}], got {tuple(alpha.shape)}")
        if tuple(Wg.shape) != (T, T):
            raise ValueError(f"Wg must be [{T},{T}], got {tuple(Wg.shape)}")
        if W is not None and (W.dim() != 2 or W.shape[1] != Cin):
            raise ValueError(f"W must be [Co,{Cin}], got {tuple(W.shape)}")
    else:
        if alpha.dim() != 2 or alpha.shape[1] != Cin:
            raise ValueError(f"alpha must be [R,{Cin}], got {tuple(alpha.shape)}")
        R = alpha.shape[0]
        if tuple(Wg.shape) != (R, T, T):
            raise ValueError(f"Wg must be [{R},{T},{T}], got {tuple(Wg.shape)}")
        if W is not None and (W.dim() != 3 or W.shape[0] != R or W.shape[2] != Cin):
            raise ValueError(f"W must be [{R},Co,{Cin}], got {tuple(W.shape)}")
    return _gacn_checked(x, alpha, Wg, W, adjacency, need_weights, weights, _lead or (G,))


def _gacn_checked(x, alpha, Wg, W, adjacency, need_weights: bool, weights: str, lead):
    """gacn after its argument checks; `lead`: the leading shape of the weights ((G,), or (R, Bg) for StackedGACN)."""
    G, N = x.shape[0], x.shape[2]
    recording = torch.is_grad_enabled()
    graph, adj, adj_grad = _resolve_adjacency(adjacency, x.device, G, alpha.shape[0] if alpha.dim() == 2 else 1, N, recording)
    if not need_weights:
        sink = _sink_slot.sink
        if sink is None:
            return _GACNFunction.apply(x, alpha, Wg, W, graph, recording, adj_grad, adj)
        z, w = _GACNFunction.apply(x, alpha, Wg, W, graph, recording, adj_grad, adj, sink.form)
        sink.append(w, graph)
        return z
    z, w = _GACNFunction.apply(x, alpha, Wg, W, graph, recording, adj_grad, adj, weights)
    return z, _weights_out(w, graph, weights, lead)


class _WeightSink(list):
    """What `collect_weights` records: (weights [G,nnz] or [G,N,N], graph) of every graph-attention call, in order."""

    def __init__(self, form: str):
        super().__init__()
        self.form = form

    def append(self, w, graph):
        super().append((w, graph))


class _SinkSlot(threading.local):
    sink: Optional[_WeightSink] = None


_sink_slot = _SinkSlot()      # per thread: a collection in one thread changes no call of another


class collect_weights:
    """Within this context every `gacn` / `attention_core` call of the current thread also records its attention weights
    (`weights` as for need_weights) in the list it yields, in call order, while returning only its output: how
    `MSGAT.attention_maps` reads the attention of every block on either evaluation path.  Meanwhile those calls run their
    autograd Function with the weights as a second output (its gradient None unless used): recorded "masked" weights
    stay differentiable under grad mode, "softmax" ones never are, "softmax_grad" ones are the differentiable dense maps
    [G,N,N] -- around a grad-enabled `MSGAT.forward`, on the stacked path and the component loop alike, a training step
    can put a regulariser on the map of every block.  `weights_of(entry, form, lead)` turns an entry into
    the caller's tensor.  Not re-entrant; calls in other threads are not affected."""

    def __init__(self, weights: str = "masked"):
        self.form = _check_weights(weights)

    def __enter__(self) -> _WeightSink:
        if _sink_slot.sink is not None:
            raise RuntimeError("collect_weights is not re-entrant")
        _sink_slot.sink = _WeightSink(self.form)
        return _sink_slot.sink

    def __exit__(self, *exc):
        _sink_slot.sink = None
        return False


def weights_of(entry, form: str, lead, groups: slice = slice(None)):
    """The caller's weights tensor [*lead,N,N] of a `collect_weights` entry, restricted to `groups`."""
    w, graph = entry
    return _weights_out(w[groups], graph, form, lead)


def graph_attention(x, alpha, Wg, adjacency, need_weights: bool = False, weights: str = "masked"):
    """`GraphAttention.forward` (attention.py:32-36) for R stacked relations."""
    return gacn(x, alpha, Wg, None, adjacency, need_weights=need_weights, weights=weights)


class _LayerNormTFunction(torch.autograd.Function):
    """x[..., T], weight[T] | None, bias[T] | None -> LayerNorm over the last axis."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps: float, relu_input: bool = False):
        L = _lib.checked()
        x = x.contiguous()
        T = x.shape[-1]
        rows = x.numel() // T if T else 0
        ctx.relu_input = bool(relu_input)
        y = torch.empty_like(x)
        w = None if weight is None else weight.contiguous()
        b = None if bias is None else bias.contiguous()
        R, ctx.param_shape = _ln_sets(w, b, T)          # weight / bias [T] or [R,T]: R parameter sets, relation-major rows
        L.msgat_layernorm_forward(_ptr(x), _ptr(w), _ptr(b), _ptr(y), rows, T, eps, R, _stream_handle(x.device))
        ctx.eps, ctx.has_w, ctx.has_b, ctx.R = eps, weight is not None, bias is not None, R
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(*([x] + ([w] if w is not None else [])))
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.checked()
        saved = ctx.saved_tensors
        x, w = saved[0], (saved[1] if ctx.has_w else None)
        T = x.shape[-1]
        rows = x.numel() // T
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        R = ctx.R
        dw = torch.empty_like(w) if ctx.has_w else None
        db = torch.empty(ctx.param_shape, device=x.device, dtype=torch.float32) if ctx.has_b else None
        part = _scratch(x, L.msgat_layernorm_partial_floats(rows, T, R))
        L.msgat_layernorm_backward(_ptr(x), _ptr(w), _ptr(dy), None, _ptr(dx), _ptr(dw), _ptr(db), _ptr(part),
                                   rows, T, ctx.eps, R, int(ctx.relu_input), _stream_handle(x.device))
        return dx, dw, db, None, None


class _LnPoolTeeFunction(torch.autograd.Function):
    """x -> (LayerNorm(x), x, node_pool(LayerNorm(x), pool_w)): MEAM's first three reads of its input (msgat.py:122-125 with
    attention.py:89 inside CACN) as one autograd node, so that backward adds the pooling's rank-one gradient
    pool_w[n] dpooled[s,t] inside the LayerNorm-backward kernel (msgat_layernorm_backward_pooled) instead of in a pass of
    its own over the activation, next to the gradient of the residual path's read of x (the second output)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps: float, relu_input: bool, pool_w):
        L = _lib.checked()
        x = x.contiguous()
        B, Cc, N, T = x.shape
        rows = B * Cc * N
        y = torch.empty_like(x)
        w = None if weight is None else weight.contiguous()
        b = None if bias is None else bias.contiguous()
        pw = pool_w.contiguous()
        R, ctx.param_shape = _ln_sets(w, b, T)
        stream = _stream_handle(x.device)
        pooled = _new(x, B, Cc, T)
        Rp = pw.numel() // N
        if Rp == R and N >= 64:     # the pooling's sums come out of the LayerNorm pass itself (+ a small launch adding the shares)
            part = _scratch(x, L.msgat_layernorm_pool_partial_floats(rows, T, R))
            L.msgat_layernorm_forward_pooled(_ptr(x), _ptr(w), _ptr(b), _ptr(y), _ptr(pw), N, _ptr(pooled), _ptr(part),
                                             rows, T, eps, R, stream)
        else:
            L.msgat_layernorm_forward(_ptr(x), _ptr(w), _ptr(b), _ptr(y), rows, T, eps, R, stream)
            L.msgat_node_pool(_ptr(y), _ptr(pw), _ptr(pooled), B * Cc, N, T, Rp, 0, 0, stream)
        ctx.eps, ctx.relu_input, ctx.has_w, ctx.has_b, ctx.R, ctx.Rp = eps, bool(relu_input), w is not None, b is not None, R, Rp
        ctx.save_for_backward(*([x, y, pw] + ([w] if w is not None else []) + ([b] if b is not None else [])))
        ctx.set_materialize_grads(False)      # an output nobody differentiates arrives as None (backward handles each): no
        return y, x.view_as(x), pooled        # zero-filled [B,C,N,T] for the second output of a frozen x

    @staticmethod
    def backward(ctx, dy, dx_other, dpooled):
        L = _lib.checked()
        saved = ctx.saved_tensors
        x, y, pw = saved[:3]
        w = saved[3] if ctx.has_w else None
        lnb = saved[3 + int(ctx.has_w)] if ctx.has_b else None      # the LayerNorm's bias: y is rebuilt from x for dpool_w
        B, Cc, N, T = x.shape
        rows = B * Cc * N
        stream = _stream_handle(x.device)
        need = ctx.needs_input_grad
        dpw = None
        fused = dpooled is not None and ctx.Rp == ctx.R           # the pooling's gradients inside the LayerNorm-backward kernel

        def pool_weight_grad():     # its own pass over the stored y (msgat_node_pool_grad_weight)
            g = torch.empty_like(pw)
            part = _scratch(x, L.msgat_node_pool_partial_floats(B, Cc, N))
            L.msgat_node_pool_grad_weight(_ptr(y), _ptr(dpooled.contiguous()), _ptr(g), _ptr(part), B, Cc, N, T, ctx.Rp,
                                          stream)
            return g
        if dy is None and dpooled is None:
            if dx_other is not None and ctx.relu_input:
                dx_other = torch.ops.aten.threshold_backward(dx_other.contiguous(), x, 0.0)
            return dx_other, None, None, None, None, None
        dy = torch.zeros_like(x) if dy is None else dy.contiguous()
        other = None if dx_other is None else dx_other.contiguous()
        dx = torch.empty_like(x)
        dw = torch.empty_like(w) if ctx.has_w else None
        db = torch.empty(ctx.param_shape, device=x.device, dtype=torch.float32) if ctx.has_b else None
        part = _scratch(x, L.msgat_layernorm_partial_floats(rows, T, ctx.R))
        if fused:
            want_pw = bool(need[5])
            dpw = torch.empty_like(pw) if want_pw else None
            rows_scratch = _new(x, rows) if want_pw else None
            L.msgat_layernorm_backward_pooled(_ptr(x), _ptr(w), _ptr(lnb), _ptr(dy), _ptr(other), _ptr(pw),
                                              _ptr(dpooled.contiguous()), N, _ptr(dx), _ptr(dw), _ptr(db), _ptr(dpw),
                                              _ptr(rows_scratch), _ptr(part), rows, T, ctx.eps, ctx.R,
                                              int(ctx.relu_input), stream)
        else:
            if dpooled is not None:      # parameter-set counts differ: the pooling's gradients in their own passes, then the LayerNorm
                if need[5]:
                    dpw = pool_weight_grad()
                dyp = torch.empty_like(x)
                L.msgat_node_pool_grad_signal(_ptr(pw), _ptr(dpooled.contiguous()), _ptr(dy), _ptr(dyp), B * Cc, N, T,
                                              ctx.Rp, stream)
                dy = dyp
            L.msgat_layernorm_backward(_ptr(x), _ptr(w), _ptr(dy), _ptr(other), _ptr(dx), _ptr(dw), _ptr(db), _ptr(part),
                                       rows, T, ctx.eps, ctx.R, int(ctx.relu_input), stream)
        return dx, dw, db, None, None, dpw


def _check_ln_params(x: torch.Tensor, **params):
    """LayerNorm parameters over the last axis of x: each None, [T] or [R,T] with R dividing the leading axis, and all
    that are given of one shape (the kernels index both by the relation: a [T] bias beside an [R,T] weight would be read
    past its end)."""
    T = x.shape[-1]
    given = {name: t for name, t in params.items() if t is not None}
    for name, t in given.items():
        _require_device_tensor(name, t, x.device)
        if t.shape[-1] != T or t.dim() > 2 or (t.dim() == 2 and x.shape[0] % t.shape[0]):
            raise ValueError(f"{name} must be [{T}] or [R,{T}] with R dividing the leading axis, got {tuple(t.shape)}")
    if len({tuple(t.shape) for t in given.values()}) > 1:
        raise ValueError(" and ".join(given) + " must have the same shape, got "
                         + " and ".join(str(tuple(t.shape)) for t in given.values()))


def _ln_sets(weight, bias, T: int):
    """(parameter sets R, shape of a parameter gradient) of a LayerNorm: read from the weight, or from the bias where there
    is no weight -- a [R,T] bias alone is R sets too, and its gradient has R rows."""
    ref = weight if weight is not None else bias
    if ref is None:
        return 1, (T,)
    return ref.numel() // T, tuple(ref.shape)


def layer_norm_pool_tee(x: torch.Tensor, weight, bias, eps: float, relu_input: bool, pool_w: torch.Tensor):
    """(layer_norm_t(x), x, node_pool(layer_norm_t(x), pool_w)) as one node whose backward adds the gradients of the
    second output and of the pooling inside the LayerNorm-backward kernel (`relu_input`: the mask then covers the
    gradients of both uses of x).  pool_w [N] or [R,N]."""
    _require_device_tensor("signals", x)
    _require_device_tensor("weights", pool_w, x.device)
    if x.dim() != 4 or pool_w.shape[-1] != x.shape[2] or pool_w.dim() > 2 or (pool_w.dim() == 2 and x.shape[0] % pool_w.shape[0]):
        raise ValueError(f"layer_norm_pool_tee: signals {tuple(x.shape)}, pooling weights {tuple(pool_w.shape)}")
    _check_ln_params(x, weight=weight, bias=bias)
    # The node's forward takes the pooling's sums out of the LayerNorm pass (other bits than node_pool's own pass) when
    # the two have the same parameter-set count and N >= 64.  There the form follows the grad mode alone, as the graph
    # attention's does (_GACNFunction.forward): in grad mode everything goes through the node, whatever requires grad --
    # a frozen x (every component's first block in ordinary training, where x is the model's input), a wholly frozen
    # block of a fine-tuned model -- so that what is frozen does not change the forward.  A frozen x gets back the x it
    # gave, not the node's output, and nothing downstream forms a gradient for it.  Elsewhere, and under no_grad, a
    # frozen x takes the two ops, which launch what the node would.
    same_sets = pool_w.numel() // x.shape[2] == _ln_sets(weight, bias, x.shape[-1])[0] if x.numel() else False
    if x.numel() == 0 or not (x.requires_grad or (torch.is_grad_enabled() and same_sets and x.shape[2] >= 64)):
        normed = layer_norm_t(x, weight, bias, eps, relu_input)
        return normed, x, node_pool(normed, pool_w)
    normed, again, pooled = _LnPoolTeeFunction.apply(x, weight, bias, float(eps), bool(relu_input), pool_w)
    return normed, (again if x.requires_grad else x), pooled


def layer_norm_t(x: torch.Tensor, weight: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                 eps: float = 1e-5, relu_input: bool = False) -> torch.Tensor:
    """`F.layer_norm(x, [T], weight, bias, eps)` over the timestep axis, the op the reference applies
    to every GACN input (msgat.py:122, :158), as one HBM-speed pass in libmsgat_hip.so.

    `relu_input=True`: x is the output of a ReLU whose backward mask (gradient 0 where x <= 0) this op's backward
    applies -- for a producer that was told to skip it (`mix_multi(..., relu=True, relu_grad_premasked=True)`)."""
    _require_device_tensor("signals", x)
    _check_ln_params(x, weight=weight, bias=bias)
    if x.numel() == 0:
        return torch.empty_like(x)
    return _LayerNormTFunction.apply(x, weight, bias, float(eps), bool(relu_input))


# ---- the temporal / channel branches of MEAM and its residual tail -----------

def _new(like: torch.Tensor, *shape) -> torch.Tensor:
    return torch.empty(shape, device=like.device, dtype=torch.float32)


def _scratch(like: torch.Tensor, n_floats: int) -> torch.Tensor:
    """The float32 scratch a `msgat_*_partial_floats` query asked for, on `like`'s device; never empty."""
    return _new(like, max(int(n_floats), 1))


_ones_cache = {}


def _ones(device, N: int) -> torch.Tensor:
    """A cached [N] vector of ones on `device`: the weights of a node pooling that sums over the nodes."""
    ones = _ones_cache.get((device, N))
    if ones is None:
        ones = _ones_cache[(device, N)] = torch.ones(N, device=device, dtype=torch.float32)
    return ones


def _channel_sums(t: torch.Tensor, R: int = 0) -> torch.Tensor:
    """[G,C,N,T] -> [C] (or [R,C] per relation when R > 0): the bias gradient of a convolution.  One streaming
    pass (node pooling with unit weights) instead of torch's strided reduction kernel (87 us vs 12 us at
    [32,24,883,12])."""
    G, Cc, N, T = t.shape
    pooled = _new(t, G, Cc, T)
    keep, seg = _as_segment(t)                    # a channel slice of a wider gradient tensor is read in place
    _lib.checked().msgat_node_pool(seg.ptr, _ptr(_ones(t.device, N)), _ptr(pooled), G * Cc, N, T, 1, Cc if seg.group_stride else 0,
                                   seg.group_stride, _stream_handle(t.device))
    if R > 0:
        return pooled.view(R, G // R, Cc, T).sum(dim=(1, 3))
    return pooled.sum(dim=(0, 2))


class _MixFunction(torch.autograd.Function):
    """x[G,Ci,N,T], M[R,Co,Ci] (R | G), bias[Co] | None, add[G,Co,N,T] | None -> relu?(M x + bias + add)."""

    @staticmethod
    def forward(ctx, x, M, bias, add, relu: bool):
        L = _lib.checked()
        x, M = x.contiguous(), M.contiguous()
        G, Ci, N, T = x.shape
        R, Co = M.shape[0], M.shape[1]
        shape = _lib.Shape(R, G // R, Ci, Co, N, T)
        out = _new(x, G, Co, N, T)
        b = None if bias is None else bias.contiguous()
        a = None if add is None else add.contiguous()
        L.msgat_stage_mix_epilogue(C.byref(shape), Ci, Co, _ptr(x), _ptr(M), 0, _ptr(b), 0, _ptr(a), int(relu),
                                   _ptr(out), _stream_handle(x.device))
        ctx.relu, ctx.has_bias, ctx.has_add = relu, bias is not None, add is not None
        ctx.save_for_backward(x, M, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        L = _lib.checked()
        x, M, out = ctx.saved_tensors
        G, Ci, N, T = x.shape
        R, Co = M.shape[0], M.shape[1]
        # ReLU mask in one pass: aten's threshold_backward is dout where out > 0, else 0
        dpre = torch.ops.aten.threshold_backward(dout.contiguous(), out, 0.0) if ctx.relu else dout.contiguous()
        stream = _stream_handle(x.device)
        need = ctx.needs_input_grad
        dx = dM = dbias = None
        if need[0]:
            dx = torch.empty_like(x)
            shape = _lib.Shape(R, G // R, Co, Ci, N, T)
            L.msgat_stage_mix(C.byref(shape), Co, Ci, _ptr(dpre), _ptr(M), 1, None, None, _ptr(dx), stream)
        if need[1]:
            dM = torch.empty_like(M)
            shape = _lib.Shape(R, G // R, Ci, Co, N, T)
            part = _scratch(x, L.msgat_contract_partial_floats(C.byref(shape), Co, Ci))
            L.msgat_stage_contract(C.byref(shape), Co, Ci, _ptr(dpre), None, _ptr(x), _ptr(part), _ptr(dM),
                                   Co * Ci, None, 0, stream)
        if ctx.has_bias and need[2]:
            dbias = _channel_sums(dpre)
        return dx, dM, dbias, (dpre if ctx.has_add and need[3] else None), None


def mix(x: torch.Tensor, M: torch.Tensor, bias: Optional[torch.Tensor] = None, add: Optional[torch.Tensor] = None,
        relu: bool = False) -> torch.Tensor:
    """out[g,o] = relu?(sum_c M[r,o,c] x[g,c] + bias[o] + add[g,o]), r = g // (G/R): a 1x1 convolution (R = 1), a
    per-sample channel matrix (R = batch), or MEAM's tail relu(cat(branches) + res(x)) (msgat.py:130-131)."""
    _require_device_tensor("signals", x)
    _require_device_tensor("matrix", M, x.device)
    if x.dim() != 4 or M.dim() != 3 or M.shape[2] != x.shape[1] or x.shape[0] % M.shape[0]:
        raise ValueError(f"mix: signals {tuple(x.shape)} and matrix {tuple(M.shape)} do not match")
    if bias is not None and tuple(bias.shape) != (M.shape[1],):
        raise ValueError(f"bias must be [{M.shape[1]}]")
    if add is not None and tuple(add.shape) != (x.shape[0], M.shape[1], x.shape[2], x.shape[3]):
        raise ValueError(f"add must be [{x.shape[0]},{M.shape[1]},{x.shape[2]},{x.shape[3]}], got {tuple(add.shape)}")
    return _MixFunction.apply(x, M, bias, add, bool(relu))


class _TimeMixFunction(torch.autograd.Function):
    """y[G,K*Co,N,T], A[G|1,K,T,T], bias[Co] | None -> out[g,o,n,t] = bias[o] + sum_k sum_i A[g,k,t,i] y[g,k*Co+o,n,i]."""

    @staticmethod
    def forward(ctx, y, A, bias):
        L = _lib.checked()
        y, A = y.contiguous(), A.contiguous()
        G, KC, N, T = y.shape
        K = A.shape[1]
        Co = KC // K
        per_group = int(A.shape[0] != 1 or G == 1)
        out = _new(y, G, Co, N, T)
        b = None if bias is None else bias.contiguous()
        Rb = 1 if b is None or b.dim() == 1 else b.shape[0]     # bias [Co] or [R,Co]
        L.msgat_time_mix(_ptr(y), _ptr(A), per_group, _ptr(b), _ptr(out), G, Co, K, N, T, 0, Rb, 0,
                         _stream_handle(y.device))
        ctx.dims, ctx.per_group, ctx.has_bias = (G, Co, K, N, T), per_group, bias is not None
        ctx.bias_R = 0 if b is None or b.dim() == 1 else b.shape[0]
        ctx.save_for_backward(y, A)
        return out

    @staticmethod
    def backward(ctx, dout):
        L = _lib.checked()
        y, A = ctx.saved_tensors
        G, Co, K, N, T = ctx.dims
        dout, seg = _as_segment(dout)              # a channel slice of the block's concatenated gradient is read in place
        stream = _stream_handle(y.device)
        need = ctx.needs_input_grad
        dy = dA = dbias = None
        if need[0]:
            dy = torch.empty_like(y)
            L.msgat_time_mix(seg.ptr, _ptr(A), ctx.per_group, None, _ptr(dy), G, Co, K, N, T, 1, 1, seg.group_stride,
                             stream)
        if need[1]:
            dAg = _new(y, G, K, T, T)
            part = _scratch(y, L.msgat_time_mix_partial_floats(G, K, T))
            L.msgat_time_mix_grad_matrix(seg.ptr, _ptr(y), _ptr(dAg), _ptr(part), G, Co, K, N, T, seg.group_stride, stream)
            dA = dAg if A.shape[0] == G else dAg.sum(dim=0, keepdim=True)
        if ctx.has_bias and need[2]:
            dbias = _channel_sums(dout, ctx.bias_R)
        return dy, dA, dbias


def time_mix(y: torch.Tensor, A: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Applies K [T,T] matrices along the time axis of K channel groups and adds them up (see
    include/msgat_hip.h: msgat_time_mix).  K = 1 with A = att is TemporalAttention's product
    (attention.py:66); K = 2 is a causal dilated [1,2] convolution after its channel mixing."""
    _require_device_tensor("signals", y)
    _require_device_tensor("matrices", A, y.device)
    if y.dim() != 4 or A.dim() != 4 or A.shape[2] != y.shape[3] or A.shape[3] != y.shape[3]:
        raise ValueError(f"time_mix: signals {tuple(y.shape)} and matrices {tuple(A.shape)} do not match")
    if A.shape[0] not in (1, y.shape[0]) or y.shape[1] % A.shape[1]:
        raise ValueError(f"time_mix: {tuple(A.shape)} matrices for signals {tuple(y.shape)}")
    return _TimeMixFunction.apply(y, A, bias)


class _CausalConvFunction(torch.autograd.Function):
    """h[G,Ci,N,T], taps[R,2Co,Ci] = [W0; W1], bias[Co] | [R,Co] | None -> bias + W0 h[t-d] + W1 h[t]: one pass each way
    (msgat_causal_conv); the weight gradient contracts [dout[t+d]; dout] with h."""

    @staticmethod
    def forward(ctx, h, taps, bias, dilation: int):
        L = _lib.checked()
        h, taps = h.contiguous(), taps.contiguous()
        G, Ci, N, T = h.shape
        R, Co = taps.shape[0], taps.shape[1] // 2
        out = _new(h, G, Co, N, T)
        b = None if bias is None else bias.contiguous()
        L.msgat_causal_conv(_ptr(h), _ptr(taps), _ptr(b), int(b is not None and b.dim() == 2), _ptr(out), R, G // R,
                            Ci, Co, N, T, int(dilation), 0, 0, _stream_handle(h.device))
        ctx.dilation, ctx.bias_R = int(dilation), (None if b is None else (b.shape[0] if b.dim() == 2 else 0))
        ctx.save_for_backward(h, taps)
        return out

    @staticmethod
    def backward(ctx, dout):
        L = _lib.checked()
        h, taps = ctx.saved_tensors
        G, Ci, N, T = h.shape
        R, Co = taps.shape[0], taps.shape[1] // 2
        keep, seg = _as_segment(dout)             # a channel slice of the block's concatenated gradient is read in place
        stream = _stream_handle(h.device)
        need = ctx.needs_input_grad
        dh = dtaps = dbias = None
        if need[0]:
            dh = torch.empty_like(h)
            L.msgat_causal_conv(seg.ptr, _ptr(taps), None, 0, _ptr(dh), R, G // R, Ci, Co, N, T, ctx.dilation, 1,
                                seg.group_stride, stream)
        want_bias = ctx.bias_R is not None and need[2]
        if need[1] or want_bias:
            # d[W0; W1] = [dout[t+d]; dout] h^T with the 2 Co gradient rows read as time-shifted views of dout inside the
            # contraction (and a virtual channel of ones: the bias gradient is its tap-1 half)
            ones = int(bool(want_bias))
            buf = _new(h, R * 2 * Co * (Ci + ones))
            part = _scratch(h, L.msgat_contract_segments_partial_floats(R, 2 * Co, Ci + ones))
            # with_ones = 2: the matrix [R,2Co,Ci] and, behind it, the ones column [R,2Co] (no slice copies)
            L.msgat_causal_conv_grad_weight(seg.ptr, seg.group_stride, _ptr(h), _ptr(part), _ptr(buf), R, G // R, Ci, Co,
                                            N, T, ctx.dilation, 2 * ones, stream)
            dM = buf[: R * 2 * Co * Ci].view(R, 2 * Co, Ci)
            if ones:
                colsum = buf[R * 2 * Co * Ci:].view(R, 2, Co)[:, 1]      # [R,Co]: sum of dout over the relation's groups and positions
                dbias = colsum if ctx.bias_R else colsum.sum(dim=0)
            dtaps = dM if need[1] else None
        return dh, dtaps, dbias, None


def causal_conv_fused(Ci: int, Co: int) -> bool:
    """Whether `causal_conv` has its one-pass kernels for these widths (else use mix_multi + time_mix)."""
    return bool(_lib.checked().msgat_causal_conv_fused(int(Ci), int(Co)))


def causal_conv(h: torch.Tensor, taps: torch.Tensor, bias: Optional[torch.Tensor], dilation: int) -> torch.Tensor:
    """A causal dilated [1,2] convolution -- `Conv2d(Ci, Co, [1,2], padding=[0,d], dilation=[1,d])` + `Chomp(d)`,
    msgat.py:69-74 -- with both taps stacked on the output axis, taps [R, 2*Co, Ci] = [W0; W1] (W0 acts on h[t-d]):
    out = bias + W0 h[t-d] + W1 h[t], R parameter sets over R*Bg groups, in one pass over h."""
    _require_device_tensor("signals", h)
    _require_device_tensor("taps", taps, h.device)
    if h.dim() != 4 or taps.dim() != 3 or taps.shape[2] != h.shape[1] or taps.shape[1] % 2 or h.shape[0] % taps.shape[0]:
        raise ValueError(f"causal_conv: signals {tuple(h.shape)} and taps {tuple(taps.shape)} do not match")
    Co = taps.shape[1] // 2
    if bias is not None and tuple(bias.shape) not in ((Co,), (taps.shape[0], Co)):
        raise ValueError(f"bias must be [{Co}] or [{taps.shape[0]},{Co}]")
    if dilation <= 0:
        raise ValueError("dilation must be positive")
    return _CausalConvFunction.apply(h, taps, bias, int(dilation))


class _NodePoolFunction(torch.autograd.Function):
    """x[B,C,N,T], w[N] -> pooled[B,C,T] = sum_n w[n] x[b,c,n,:]   (attention.py:89)."""

    @staticmethod
    def forward(ctx, x, w):
        L = _lib.checked()
        x, w = x.contiguous(), w.contiguous()
        B, Cc, N, T = x.shape
        pooled = _new(x, B, Cc, T)
        R = w.numel() // N                                   # weights [N] or [R,N]
        L.msgat_node_pool(_ptr(x), _ptr(w), _ptr(pooled), B * Cc, N, T, R, 0, 0, _stream_handle(x.device))
        ctx.save_for_backward(x, w)
        return pooled

    @staticmethod
    def backward(ctx, dp):
        L = _lib.checked()
        x, w = ctx.saved_tensors
        B, Cc, N, T = x.shape
        dp = dp.contiguous()
        stream = _stream_handle(x.device)
        R = w.numel() // N
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            L.msgat_node_pool_grad_signal(_ptr(w), _ptr(dp), None, _ptr(dx), B * Cc, N, T, R, stream)
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(w)
            part = _scratch(x, L.msgat_node_pool_partial_floats(B, Cc, N))
            L.msgat_node_pool_grad_weight(_ptr(x), _ptr(dp), _ptr(dw), _ptr(part), B, Cc, N, T, R, stream)
        return dx, dw


def node_pool(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    _require_device_tensor("signals", x)
    _require_device_tensor("weights", w, x.device)
    if x.dim() != 4 or w.shape[-1] != x.shape[2] or w.dim() > 2 or (w.dim() == 2 and x.shape[0] % w.shape[0]):
        raise ValueError(f"node_pool: signals {tuple(x.shape)}, weights {tuple(w.shape)}")
    return _NodePoolFunction.apply(x, w)


class _ChannelPoolFunction(torch.autograd.Function):
    """x[B,C,N,T], alpha[C] -> mixed[B,N,T] = sum_c alpha[c] x[b,c]   (attention.py:59; the hot path's q)."""

    @staticmethod
    def forward(ctx, x, alpha):
        L = _lib.checked()
        x, alpha = x.contiguous(), alpha.contiguous()
        B, Cc, N, T = x.shape
        R = alpha.numel() // Cc                              # alpha [C] or [R,C]
        shape = _lib.Shape(R, B // R, Cc, 0, N, T)
        q = _new(x, B, N, T)
        L.msgat_stage_project(C.byref(shape), _ptr(x), _ptr(alpha), None, _ptr(q), None, _stream_handle(x.device))
        ctx.save_for_backward(x, alpha)
        return q

    @staticmethod
    def backward(ctx, dq):
        L = _lib.checked()
        x, alpha = ctx.saved_tensors
        B, Cc, N, T = x.shape
        dq = dq.contiguous()
        stream = _stream_handle(x.device)
        R = alpha.numel() // Cc
        dx = dalpha = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            shape = _lib.Shape(R, B // R, 1, Cc, N, T)
            L.msgat_stage_mix(C.byref(shape), 1, Cc, _ptr(dq), _ptr(alpha), 0, None, None, _ptr(dx), stream)
        if ctx.needs_input_grad[1]:
            dalpha = torch.empty_like(alpha)
            shape = _lib.Shape(R, B // R, Cc, 0, N, T)
            part = _scratch(x, L.msgat_contract_partial_floats(C.byref(shape), 1, Cc))
            L.msgat_stage_contract(C.byref(shape), 1, Cc, None, _ptr(dq), _ptr(x), _ptr(part), _ptr(dalpha), Cc,
                                   None, 0, stream)
        return dx, dalpha


def channel_pool(x: torch.Tensor, alpha: torch.Tensor) -> torch.Tensor:
    _require_device_tensor("signals", x)
    _require_device_tensor("alpha", alpha, x.device)
    if x.dim() != 4 or alpha.shape[-1] != x.shape[1] or alpha.dim() > 2 or (alpha.dim() == 2 and x.shape[0] % alpha.shape[0]):
        raise ValueError(f"channel_pool: signals {tuple(x.shape)}, alpha {tuple(alpha.shape)}")
    return _ChannelPoolFunction.apply(x, alpha)


def _head_weight_grad(dout, x, W, B, Cc, N, T, To, R, stream) -> torch.Tensor:
    """The head's weight gradient, [R,To,T,1,C] (or [To,T,1,C] for a weight without the leading axis), from the
    incoming gradient dout[B,N,To] and the head's input x."""
    L = _lib.checked()
    dWc = _new(x, R, Cc, To, T)
    part = _scratch(x, L.msgat_head_grad_weight_partial_floats(Cc, T, To, R))
    L.msgat_head_grad_weight(_ptr(dout), _ptr(x), _ptr(dWc), _ptr(part), B, Cc, N, T, To, R, stream)
    # [R,To,T,1,C], made contiguous HERE, once for all R components: each component's parameter receives its row,
    # and a non-contiguous row would be copied per component when it is accumulated into .grad
    dW = dWc.permute(0, 2, 3, 1).contiguous().unsqueeze(3)
    return dW[0] if W.dim() == 4 else dW


def _head_bias_grad(dout, W, B, N, To, R, stream) -> torch.Tensor:
    """The head's bias gradient, [R,To] (or [To] for a weight without the leading axis), from dout[B,N,To]."""
    if To in (4, 8, 12, 16):   # one streaming pass over dout (node pooling with unit weights), then a tiny sum
        pooled = _new(dout, B, To)
        _lib.checked().msgat_node_pool(_ptr(dout), _ptr(_ones(dout.device, N)), _ptr(pooled), B, N, To, 1, 0, 0, stream)
        return pooled.view(R, B // R, To).sum(dim=1) if W.dim() == 5 else pooled.sum(dim=0)
    return dout.view(R, B // R, N, To).sum(dim=(1, 2)) if W.dim() == 5 else dout.sum(dim=(0, 1))


class _HeadFunction(torch.autograd.Function):
    """x[B,C,N,T], W[To,T,1,C], bias[To] | None -> out[B,N,To] = bias + sum_{c,t} W[o,t,0,c] x[b,c,n,t]  (msgat.py:153,:159)."""

    @staticmethod
    def forward(ctx, x, W, bias):
        L = _lib.checked()
        x, W = x.contiguous(), W.contiguous()
        B, Cc, N, T = x.shape
        To = W.shape[-4]
        R = 1 if W.dim() == 4 else W.shape[0]               # weight [To,T,1,C] or [R,To,T,1,C]
        out = _new(x, B, N, To)
        part = _scratch(x, L.msgat_head_forward_partial_floats(B, Cc, N, To))
        b = None if bias is None else bias.contiguous()
        L.msgat_head_forward(_ptr(x), _ptr(W), _ptr(b), _ptr(out), _ptr(part), B, Cc, N, T, To, R, _stream_handle(x.device))
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, W)
        return out

    @staticmethod
    def backward(ctx, dout):
        L = _lib.checked()
        x, W = ctx.saved_tensors
        B, Cc, N, T = x.shape
        To = W.shape[-4]
        R = 1 if W.dim() == 4 else W.shape[0]
        dout = dout.contiguous()
        stream = _stream_handle(x.device)
        dx = dW = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            L.msgat_head_grad_signal(_ptr(dout), _ptr(W), _ptr(dx), B, Cc, N, T, To, R, stream)
        if ctx.needs_input_grad[1]:
            dW = _head_weight_grad(dout, x, W, B, Cc, N, T, To, R, stream)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = _head_bias_grad(dout, W, B, N, To, R, stream)
        return dx, dW, db


class _LnHeadFunction(torch.autograd.Function):
    """x[B,C,N,T] -> head(layer_norm_t(x)): a component's last two steps (msgat.py:158-160).  Forward is one pass over x:
    the head kernel normalises the rows it loads (msgat_head_forward_ln) and writes LayerNorm(x) only when the weight
    gradient will need it.  Backward builds the head's input gradient in registers inside the LayerNorm-backward pass
    (msgat_layernorm_head_backward), so the [B,C,N,T] gradient between the two is never written."""

    @staticmethod
    def forward(ctx, x, lnw, lnb, eps: float, W, bias, relu_input: bool):
        L = _lib.checked()
        x, W = x.contiguous(), W.contiguous()
        B, Cc, N, T = x.shape
        To = W.shape[-4]
        R = 1 if W.dim() == 4 else W.shape[0]
        stream = _stream_handle(x.device)
        w = None if lnw is None else lnw.contiguous()
        lb = None if lnb is None else lnb.contiguous()
        out = _new(x, B, N, To)
        part = _scratch(x, L.msgat_head_forward_partial_floats(B, Cc, N, To))
        b = None if bias is None else bias.contiguous()
        # the head normalises what it loads; LayerNorm(x) is written only when the weight gradient will read it
        keep = ctx.needs_input_grad[4]
        xn = torch.empty_like(x) if keep else None
        L.msgat_head_forward_ln(_ptr(x), _ptr(w), _ptr(lb), eps, _ptr(W), _ptr(b), _ptr(out), _ptr(xn), _ptr(part), B, Cc, N, T,
                                To, R, stream)
        ctx.eps, ctx.relu_input, ctx.has_lnw, ctx.has_lnb, ctx.has_bias = eps, bool(relu_input), w is not None, lb is not None, bias is not None
        ctx.has_xn = keep
        ctx.param_shape = _ln_sets(w, lb, T)[1]
        ctx.save_for_backward(*([x, W] + ([xn] if keep else []) + ([w] if w is not None else [])))
        return out

    @staticmethod
    def backward(ctx, dout):
        L = _lib.checked()
        saved = ctx.saved_tensors
        x, W = saved[:2]
        xn = saved[2] if ctx.has_xn else None
        w = saved[2 + int(ctx.has_xn)] if ctx.has_lnw else None
        B, Cc, N, T = x.shape
        To = W.shape[-4]
        R = 1 if W.dim() == 4 else W.shape[0]
        dout = dout.contiguous()
        stream = _stream_handle(x.device)
        need = ctx.needs_input_grad
        dx = dlnw = dlnb = dW = db = None
        if need[0] or need[1] or need[2]:
            dx = torch.empty_like(x)
            dlnw = torch.empty_like(w) if (ctx.has_lnw and need[1]) else None
            dlnb = torch.empty(ctx.param_shape, device=x.device, dtype=torch.float32) if (ctx.has_lnb and need[2]) else None
            part = _scratch(x, L.msgat_layernorm_head_backward_partial_floats(B, Cc, N, T))
            L.msgat_layernorm_head_backward(_ptr(dout), _ptr(W), _ptr(x), _ptr(w), _ptr(dx), _ptr(dlnw), _ptr(dlnb),
                                            _ptr(part), B, Cc, N, T, To, R, ctx.eps, int(ctx.relu_input), stream)
        if need[4]:
            dW = _head_weight_grad(dout, xn, W, B, Cc, N, T, To, R, stream)
        if ctx.has_bias and need[5]:
            db = _head_bias_grad(dout, W, B, N, To, R, stream)
        return dx if need[0] else None, dlnw, dlnb, None, dW, db, None


def ln_head(x: torch.Tensor, ln_weight: Optional[torch.Tensor], ln_bias: Optional[torch.Tensor], eps: float,
            W: torch.Tensor, bias: Optional[torch.Tensor] = None, relu_input: bool = False) -> torch.Tensor:
    """`head(layer_norm_t(x, ln_weight, ln_bias, eps, relu_input), W, bias)` -- TPC's last two steps, msgat.py:158-160 --
    with ONE backward pass over x for the head's input gradient and the LayerNorm backward together."""
    _require_device_tensor("signals", x)
    _require_device_tensor("weight", W, x.device)
    T = x.shape[-1]
    if (x.dim() != 4 or W.dim() not in (4, 5) or W.shape[-3] != T or W.shape[-2] != 1 or W.shape[-1] != x.shape[1]
            or (W.dim() == 5 and x.shape[0] % W.shape[0])):
        raise ValueError(f"ln_head: signals {tuple(x.shape)} and weight {tuple(W.shape)} do not match")
    _check_ln_params(x, ln_weight=ln_weight, ln_bias=ln_bias)
    if ln_weight is not None and W.dim() == 5 and ln_weight.dim() == 2 and ln_weight.shape[0] != W.shape[0]:
        raise ValueError("ln_head: the LayerNorm and the head must have the same number of parameter sets")
    if x.numel() == 0 or ((ln_weight is not None or ln_bias is not None)
                          and _ln_sets(ln_weight, ln_bias, T)[0] != (1 if W.dim() == 4 else W.shape[0])):
        return head(layer_norm_t(x, ln_weight, ln_bias, eps, relu_input), W, bias)   # mixed parameter-set counts: the two ops
    return _LnHeadFunction.apply(x, ln_weight, ln_bias, float(eps), W, bias, bool(relu_input))


def head(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The component's prediction head: `fc(x.transpose(1, 3))[..., 0].transpose(1, 2)` of msgat.py:159-160
    with `fc = Conv2d(T, T_out, [1, C])`, as one pass over x."""
    _require_device_tensor("signals", x)
    _require_device_tensor("weight", W, x.device)
    if (x.dim() != 4 or W.dim() not in (4, 5) or W.shape[-3] != x.shape[3] or W.shape[-2] != 1 or W.shape[-1] != x.shape[1]
            or (W.dim() == 5 and x.shape[0] % W.shape[0])):
        raise ValueError(f"head: signals {tuple(x.shape)} and weight {tuple(W.shape)} do not match")
    return _HeadFunction.apply(x, W, bias)


class _GateSumFunction(torch.autograd.Function):
    """pred [R,B,N,To], H [B], D [B], h_w [nh, R*N*To], d_w [nd, R*N*To] -> sum_r pred_r * (h_w[H] + d_w[D])_r
    (msgat.py:203-205 with embeddings.py:36-39 inside); H = D = d_w = None: the static gate h_w = W [R,N,To]."""

    @staticmethod
    def forward(ctx, pred, H, D, h_w, d_w):
        L = _lib.checked()
        pred, h_w = pred.contiguous(), h_w.contiguous()
        d_w = None if d_w is None else d_w.contiguous()
        R, B = pred.shape[:2]
        E = pred[0, 0].numel()
        nh = h_w.shape[0] if H is not None else 1
        nd = d_w.shape[0] if d_w is not None else 0
        out = _new(pred, *pred.shape[1:])
        L.msgat_gate_sum(_ptr(pred), _ptr(H), _ptr(D), _ptr(h_w), _ptr(d_w), _ptr(out), R, B, E, nh, nd,
                         _stream_handle(pred.device))
        ctx.dims = (R, B, E, nh, nd)
        ctx.has_idx, ctx.has_day = H is not None, d_w is not None
        ctx.save_for_backward(*([pred, h_w] + ([H, D] if H is not None else []) + ([d_w] if d_w is not None else [])))
        return out

    @staticmethod
    def backward(ctx, dout):
        L = _lib.checked()
        saved = list(ctx.saved_tensors)
        pred, h_w = saved[:2]
        H, D = (saved[2], saved[3]) if ctx.has_idx else (None, None)
        d_w = saved[-1] if ctx.has_day else None
        R, B, E, nh, nd = ctx.dims
        need = ctx.needs_input_grad
        dout = dout.contiguous()
        dpred = torch.empty_like(pred) if need[0] else None
        dh = torch.empty_like(h_w) if need[3] else None
        dd = torch.empty_like(d_w) if (d_w is not None and need[4]) else None
        L.msgat_gate_sum_backward(_ptr(dout), _ptr(pred), _ptr(H), _ptr(D), _ptr(h_w), _ptr(d_w), _ptr(dpred), _ptr(dh),
                                  _ptr(dd), R, B, E, nh, nd, _stream_handle(pred.device))
        return dpred, None, None, dh, dd


def gate_sum(pred: torch.Tensor, H: Optional[torch.Tensor], D: Optional[torch.Tensor], h_weight: torch.Tensor,
             d_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`sum_r pred[r] * gate[:, r]` with `gate = (h_ebd(H) + d_ebd(D)).view(B, R, N, T_out)` -- the model's last line
    (msgat.py:203-205, embeddings.py:36-39) -- as one launch forward and one backward; the embedding tables receive
    dense gradients, as nn.Embedding's do.  `H = D = d_weight = None`: the static gate `h_weight = W [R,N,T_out]`
    (msgat.py:189).  Indices outside a table are clamped to its ends (torch's gather traps on the device)."""
    _require_device_tensor("pred", pred)
    _require_device_tensor("h_weight", h_weight, pred.device)
    if pred.dim() < 3:
        raise ValueError(f"gate_sum: pred {tuple(pred.shape)} must be [R, B, ...]")
    R, B = pred.shape[:2]
    RE = pred[:, 0].numel()
    if (H is None) != (D is None) or (H is None) != (d_weight is None):
        raise ValueError("gate_sum: H, D and d_weight come together (time embedding) or not at all (static gate)")
    if H is None:
        if h_weight.numel() != RE:
            raise ValueError(f"gate_sum: static gate {tuple(h_weight.shape)} does not match pred {tuple(pred.shape)}")
    else:
        _require_device_tensor("d_weight", d_weight, pred.device)
        if H.dtype in (torch.int32, torch.int16, torch.uint8) and D.dtype in (torch.int32, torch.int16, torch.uint8):
            H, D = H.long(), D.long()                      # nn.Embedding takes these too
        if (h_weight.dim() != 2 or d_weight.dim() != 2 or h_weight.shape[1] != RE or d_weight.shape[1] != RE
                or H.shape != (B,) or D.shape != (B,) or H.dtype != torch.int64 or D.dtype != torch.int64
                or H.device != pred.device or D.device != pred.device):
            raise ValueError(f"gate_sum: pred {tuple(pred.shape)}, H {tuple(H.shape)} {H.dtype}, D {tuple(D.shape)} {D.dtype}, "
                             f"tables {tuple(h_weight.shape)} / {tuple(d_weight.shape)} do not match")
        H, D = H.contiguous(), D.contiguous()
    return _GateSumFunction.apply(pred, H, D, h_weight, d_weight)


class _EdgeTimeWeightsFunction(torch.autograd.Function):
    """base [nnz], h_w [nh,nnz], d_w [nd,nnz], H [B], D [B] -> (base + h_w[H]) + d_w[D] [B,nnz], one launch each way."""

    @staticmethod
    def forward(ctx, base, h_w, d_w, H, D):
        L = _lib.checked()
        base, h_w, d_w = base.contiguous(), h_w.contiguous(), d_w.contiguous()
        B, nnz = H.shape[0], base.shape[0]
        nh, nd = h_w.shape[0], d_w.shape[0]
        out = _new(base, B, nnz)
        L.msgat_edge_time_weights(_ptr(base), _ptr(h_w), _ptr(d_w), _ptr(H), _ptr(D), _ptr(out), B, nnz, nh, nd,
                                  _stream_handle(base.device))
        ctx.dims = (B, nnz, nh, nd)
        ctx.save_for_backward(H, D)
        return out

    @staticmethod
    def backward(ctx, dout):
        L = _lib.checked()
        H, D = ctx.saved_tensors
        B, nnz, nh, nd = ctx.dims
        need = ctx.needs_input_grad
        dout = dout.contiguous()
        dbase = _new(dout, nnz) if need[0] else None
        dh = _new(dout, nh, nnz) if need[1] else None
        dd = _new(dout, nd, nnz) if need[2] else None
        L.msgat_edge_time_weights_backward(_ptr(dout), _ptr(H), _ptr(D), _ptr(dbase), _ptr(dh), _ptr(dd), B, nnz, nh, nd,
                                           _stream_handle(dout.device))
        return dbase, dh, dd, None, None


def edge_time_weights(base: torch.Tensor, h_weight: torch.Tensor, d_weight: torch.Tensor, H: torch.Tensor,
                      D: torch.Tensor) -> torch.Tensor:
    """`(base + h_weight[H]) + d_weight[D]` [B,nnz]: a weight per stored edge and per sample from the sample's hour of day
    and day of week -- the time embedding's `h_ebd(H) + d_ebd(D)` (embeddings.py:30-36) on the edges of one sparse pattern --
    as one launch forward (the bits of that torch expression) and one backward: `base` [nnz] gets the batch sum, the tables
    [24,nnz] / [7,nnz] dense gradients summed in sample order, every row written (msgat_edge_time_weights_backward).  The
    result is contiguous in the order of (crow, col): `edge_adjacency(crow, col, weights)` reads it where it is.  Indices
    outside a table are clamped to its ends, as `gate_sum` does."""
    _require_device_tensor("base", base)
    _require_device_tensor("h_weight", h_weight, base.device)
    _require_device_tensor("d_weight", d_weight, base.device)
    if H.dtype in (torch.int32, torch.int16, torch.uint8) and D.dtype in (torch.int32, torch.int16, torch.uint8):
        H, D = H.long(), D.long()                          # nn.Embedding takes these too
    nnz = base.numel()
    if (base.dim() != 1 or h_weight.dim() != 2 or d_weight.dim() != 2 or h_weight.shape[1] != nnz or d_weight.shape[1] != nnz
            or h_weight.shape[0] < 1 or d_weight.shape[0] < 1 or H.dim() != 1 or D.shape != H.shape
            or H.dtype != torch.int64 or D.dtype != torch.int64 or H.device != base.device or D.device != base.device):
        raise ValueError(f"edge_time_weights: base {tuple(base.shape)}, tables {tuple(h_weight.shape)} / {tuple(d_weight.shape)}, "
                         f"H {tuple(H.shape)} {H.dtype}, D {tuple(D.shape)} {D.dtype} do not match")
    return _EdgeTimeWeightsFunction.apply(base, h_weight, d_weight, H.contiguous(), D.contiguous())


class _CallerOrder:
    """The crossing between a SparsePattern's caller order of (crow, col) and the library's edge order: a pattern whose order
    inside a row is not the library's is permuted with torch gathers on either side of a launch, any other passes through.
    The edge axis is a tensor's last ([nnz], [V,nnz])."""

    def __init__(self, pattern, device):
        self.perm = None if pattern.identity else pattern._perm(device)      # (library edge -> input position, its inverse)

    def to_library(self, t):
        """`t` (or None) contiguous, its edges in library order"""
        if t is None:
            return None
        return t.contiguous() if self.perm is None else t.index_select(t.dim() - 1, self.perm[0])

    def to_caller(self, t):
        """a launch's result (or None), its edges back in the caller's order"""
        return t if t is None or self.perm is None else t.index_select(t.dim() - 1, self.perm[1])


def _edge_exempt(op: str, exempt, nnz: int, device):
    """`exempt` of `op`, checked as uint8 or bool [nnz] on `device`, as a launch reads it: contiguous uint8 (None stays)."""
    if exempt is None:
        return None
    if (not torch.is_tensor(exempt) or exempt.dtype not in (torch.uint8, torch.bool) or tuple(exempt.shape) != (nnz,)
            or exempt.device != device):
        raise ValueError(f"{op}: exempt must be uint8 or bool [{nnz}] on {device}, got "
                         f"{getattr(exempt, 'dtype', type(exempt).__name__)} {tuple(getattr(exempt, 'shape', ()))}")
    exempt = exempt.contiguous()
    return exempt.view(torch.uint8) if exempt.dtype == torch.bool else exempt


def _shared_weight_grad(dout: torch.Tensor, V: int, nnz: int, sets):
    """The gradient of a weight [V,nnz] (`sets`) or [nnz] shared by the samples, for a backward launch to fill -- or, with no
    sample or no edge, the empty sum: the caller launches nothing then (`V and nnz`)."""
    shape = (V, nnz) if sets else (nnz,)
    return torch.zeros(shape, device=dout.device, dtype=dout.dtype) if V == 0 or nnz == 0 else _new(dout, *shape)


class _EdgeSignalWeightsFunction(torch.autograd.Function):
    """base [nnz], ab [B,N,2d] -> base[e] + <a[b,row(e)], b[b,col(e)]> [B,nnz] on `pattern`'s structure, one launch each way.
    Values cross in the caller's order of (crow, col) (`_CallerOrder`)."""

    @staticmethod
    def forward(ctx, base, ab, pattern):
        L = _lib.checked()
        ab = ab.contiguous()
        B, N, d = ab.shape[0], ab.shape[1], ab.shape[2] // 2
        nnz = pattern.structure.nnz
        gstruct, keep = pattern.structure.on(ab.device)
        order = _CallerOrder(pattern, ab.device)
        base = order.to_library(base)
        out = _new(ab, B, nnz)
        L.msgat_edge_signal_weights(C.byref(gstruct), _ptr(base), _ptr(ab), B, d, _ptr(out), _stream_handle(ab.device))
        ctx.call = (gstruct, keep, order, B, N, d, nnz)
        ctx.save_for_backward(ab)
        return order.to_caller(out)

    @staticmethod
    def backward(ctx, dout):
        L = _lib.checked()
        ab, = ctx.saved_tensors
        gstruct, _, order, B, N, d, nnz = ctx.call
        need = ctx.needs_input_grad
        dout = order.to_library(dout)
        dbase = _new(dout, nnz) if need[0] else None
        dab = _new(dout, B, N, 2 * d) if need[1] else None
        L.msgat_edge_signal_weights_backward(C.byref(gstruct), _ptr(dout), _ptr(ab), B, d, _ptr(dbase), _ptr(dab),
                                             _stream_handle(dout.device))
        return order.to_caller(dbase), dab, None


def edge_signal_weights(base: torch.Tensor, ab: torch.Tensor, crow: torch.Tensor, col: torch.Tensor) -> torch.Tensor:
    """`base[e] + sum_k a[b,row(e),k] * b[b,col(e),k]` [B,nnz]: a weight per stored edge and per sample from the sample's own
    node signals at the edge's two ends -- the edge strength of the dynamic-graph traffic models as a rank-d bilinear form
    on the edges of one sparse pattern.  `ab` [B,N,2d] is the node projection, `a = ab[..., :d]` the row side and
    `b = ab[..., d:]` the column side, d in {4, 8, ..., 32}; `base` [nnz] and the result follow the order of (`crow` [N+1],
    `col` [nnz]), the result contiguous: `edge_adjacency(crow, col, weights)` reads it where it is, on the structure this op
    resolved (crow, col) to.  One launch forward; one backward for `base` (the batch sum, in sample order) and `ab` (row
    sums in CSR order, column sums in CSC order, every node written), no atomics (msgat_edge_signal_weights{,_backward})."""
    _require_device_tensor("base", base)
    _require_device_tensor("ab", ab, base.device)
    if crow.device != base.device or col.device != base.device:
        raise ValueError(f"edge_signal_weights: crow is on {crow.device} and col on {col.device}, base on {base.device}")
    if (base.dim() != 1 or ab.dim() != 3 or crow.dim() != 1 or col.dim() != 1 or col.numel() != base.numel()
            or crow.numel() != ab.shape[1] + 1 or ab.shape[2] % 2):
        raise ValueError(f"edge_signal_weights: base {tuple(base.shape)}, ab {tuple(ab.shape)}, crow {tuple(crow.shape)} and "
                         f"col {tuple(col.shape)} must be [nnz], [B, N, 2d], [N+1] and [nnz]")
    d = ab.shape[2] // 2
    if d < 4 or d > 32 or d % 4:
        raise ValueError(f"edge_signal_weights: the rank d = {d} (ab {tuple(ab.shape)}) must be one of 4, 8, ..., 32")
    return _EdgeSignalWeightsFunction.apply(base, ab, edge_pattern_of(crow, col))


def edge_dropout_constants(p: float) -> tuple:
    """(thr, scale) of a drop probability p in [0,1): an edge is dropped iff its 32-bit draw is `< thr`,
    `thr = floor(p * 2^32)`, and a kept one is multiplied by `scale = 1 / (1 - p)` -- both computed in double, the scale then
    rounded once to fp32 (by the call)."""
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not (0.0 <= float(p) < 1.0):
        raise ValueError(f"edge_dropout: p must be a number in [0, 1), got {p!r}")
    p = float(p)
    return int(math.floor(p * 4294967296.0)), 1.0 / (1.0 - p)


def edge_dropout_state(seed: int, device) -> torch.Tensor:
    """`tensor([seed, 0])` int64 on `device`: the state {seed, step} of a fresh mask stream for `edge_dropout`."""
    seed = int(seed)
    if not -(1 << 63) <= seed < (1 << 64):
        raise ValueError(f"edge_dropout: the seed must fit 64 bits, got {seed}")
    if seed >= (1 << 63):
        seed -= 1 << 64                                    # the same 64 bits in torch's signed type
    return torch.tensor([seed, 0], dtype=torch.int64, device=device)


class _EdgeDropoutFunction(torch.autograd.Function):
    """w [nnz] or [V,nnz] -> w * m [V,nnz], m drawn from `state` {seed, step} (msgat_edge_dropout); backward re-creates m
    from the seed and the step the forward left in `used`, a fresh int64 [1] per call."""

    @staticmethod
    def forward(ctx, w, exempt, state, V, sample_offset, thr, scale):
        L = _lib.checked()
        w = w.contiguous()
        nnz = w.shape[-1]
        sets = int(w.dim() == 2)
        out = _new(w, V, nnz)
        used = torch.empty(1, device=w.device, dtype=torch.int64)
        L.msgat_edge_dropout(_ptr(w), _ptr(exempt), _ptr(state), _ptr(used), _ptr(out), V, nnz, sets, sample_offset, thr,
                             scale, 1, _stream_handle(w.device))
        ctx.call = (V, nnz, sets, sample_offset, thr, scale)
        ctx.operands = (exempt, state, used)               # integer tensors the launch reads by address: nothing to version
        return out

    @staticmethod
    def backward(ctx, dout):
        L = _lib.checked()
        exempt, state, used = ctx.operands
        V, nnz, sets, sample_offset, thr, scale = ctx.call
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        dout = dout.contiguous()
        dw = _shared_weight_grad(dout, V, nnz, sets)
        if V and nnz:                                      # else nothing was drawn
            L.msgat_edge_dropout_backward(_ptr(dout), _ptr(exempt), _ptr(state), _ptr(used), _ptr(dw), V, nnz, sets,
                                          sample_offset, thr, scale, _stream_handle(dout.device))
        return (dw,) + (None,) * 6


def edge_dropout(weight: torch.Tensor, p: float, state: torch.Tensor, *, sample_offset: int = 0,
                 exempt: Optional[torch.Tensor] = None, samples: Optional[int] = None) -> torch.Tensor:
    """Dropout on the stored edges of one sparse pattern (DropEdge with inverted scaling; the layer is linear in the
    adjacency, so this is dropout on the masked attention coefficients): `weight` [nnz] -- shared by `samples` = V samples --
    or [V,nnz] -> [V,nnz], an edge of a sample dropped (+0) with probability `p` and multiplied by `1 / (1 - p)` otherwise,
    contiguous in the order of (crow, col): `edge_adjacency(crow, col, ·)` reads it where it is.  Edges flagged in `exempt`
    (bool or uint8 [nnz]) pass through unchanged.

    The mask of sample v is a pure function of (`state` = int64 [2] {seed, step} in device memory, `sample_offset` + v,
    the edge): Philox4x32-10, see msgat_edge_dropout.  The call draws at the current step and moves `state` one step on, on
    the device -- inside a captured HIP graph every replay draws fresh masks -- and rows
    [lo, hi) of a V-row draw are the (hi - lo)-row draw at `sample_offset=lo`, whichever process draws them.  Backward
    re-creates the mask instead of storing it: `weight` [V,nnz] gets `dout * m`, `weight` [nnz] the sum over the samples in
    ascending order, one launch.  `p == 0` still runs (nothing is dropped, the step advances)."""
    if not torch.is_tensor(weight) or not weight.is_cuda:
        raise ValueError(f"edge_dropout: weight is on {getattr(weight, 'device', type(weight).__name__)}: the op runs on the GPU "
                         "only, there is no CPU path")
    if weight.dtype != torch.float32:
        raise TypeError(f"edge_dropout: weight must be float32, got {weight.dtype}")
    thr, scale = edge_dropout_constants(p)
    if weight.dim() == 1:
        if samples is None or isinstance(samples, bool) or not isinstance(samples, int) or samples < 0:
            raise ValueError(f"edge_dropout: weight {tuple(weight.shape)} is shared by the samples, pass their number as "
                             f"samples=V (got {samples!r})")
        V = samples
    elif weight.dim() == 2:
        V = weight.shape[0]
        if samples is not None and samples != V:
            raise ValueError(f"edge_dropout: weight {tuple(weight.shape)} has {V} samples, samples={samples!r}")
    else:
        raise ValueError(f"edge_dropout: weight must be [nnz] or [V, nnz], got {tuple(weight.shape)}")
    nnz = weight.shape[-1]
    if (not torch.is_tensor(state) or state.dtype != torch.int64 or tuple(state.shape) != (2,) or state.device != weight.device
            or not state.is_contiguous()):
        raise ValueError(f"edge_dropout: state must be int64 [2] {{seed, step}} on {weight.device} (edge_dropout_state), got "
                         f"{getattr(state, 'dtype', type(state).__name__)} {tuple(getattr(state, 'shape', ()))} on "
                         f"{getattr(state, 'device', None)}")
    if isinstance(sample_offset, bool) or not isinstance(sample_offset, int) or sample_offset < 0 or sample_offset + V > 1 << 32:
        raise ValueError(f"edge_dropout: sample_offset = {sample_offset!r} with {V} samples: global sample indices are 32 bits")
    if nnz >= 1 << 34:
        raise ValueError(f"edge_dropout: {nnz} stored edges, at most 2^34 - 1 are supported")
    exempt = _edge_exempt("edge_dropout", exempt, nnz, weight.device)
    return _EdgeDropoutFunction.apply(weight, exempt, state, V, sample_offset, thr, scale)


EDGE_VALIDITY_T = (4, 8, 12, 16)           # the package's T_in set: what msgat_edge_validity is built for


def edge_validity_table(mode, T: int) -> tuple:
    """The gate of a source node by its count of valid readings: `table[c]`, c = 0..T, T + 1 floats computed in double and
    rounded once to fp32.  `mode="scale"`: c / T; `"drop"`: 1 at c == T and 0 below; an int m in 1..T: 1 where c >= m and 0
    below.  `table[T] == 1` in every mode: a window without a missing reading leaves its edges bit for bit as they were."""
    if isinstance(T, bool) or not isinstance(T, int) or T not in EDGE_VALIDITY_T:
        raise ValueError(f"edge_validity: T = {T!r} readings per window, supported are {EDGE_VALIDITY_T}")
    if isinstance(mode, str) and mode == "scale":
        table = [c / T for c in range(T + 1)]
    elif isinstance(mode, str) and mode == "drop":
        table = [1.0 if c == T else 0.0 for c in range(T + 1)]
    elif isinstance(mode, int) and not isinstance(mode, bool) and 1 <= mode <= T:
        table = [1.0 if c >= mode else 0.0 for c in range(T + 1)]
    else:
        raise ValueError(f'edge_validity: mode must be "scale", "drop" or an int in 1..{T} (the least number of valid '
                         f"readings that keeps the edges), got {mode!r}")
    return tuple(C.c_float(x).value for x in table)


def _edge_validity_operands(weight, validity, crow, col, exempt, samples):
    """Shape and type checks shared by the op and its restatement; returns (V, N, T, nnz, exempt as contiguous uint8)."""
    if not torch.is_tensor(weight) or not torch.is_tensor(validity):
        raise ValueError("edge_validity: weight and validity must be tensors")
    if weight.dtype != torch.float32 or validity.dtype != torch.float32:
        raise TypeError(f"edge_validity: weight and validity must be float32, got {weight.dtype} and {validity.dtype}")
    if validity.dim() != 3 or crow.dim() != 1 or col.dim() != 1 or crow.numel() != validity.shape[1] + 1:
        raise ValueError(f"edge_validity: validity {tuple(validity.shape)}, crow {tuple(crow.shape)} and col {tuple(col.shape)} "
                         "must be [V, N, T], [N+1] and [nnz]")
    V, N, T = validity.shape
    nnz = col.numel()
    if weight.dim() not in (1, 2) or weight.shape[-1] != nnz or (weight.dim() == 2 and weight.shape[0] != V):
        raise ValueError(f"edge_validity: weight {tuple(weight.shape)} must be [{nnz}] or [{V}, {nnz}] (validity "
                         f"{tuple(validity.shape)}, {nnz} stored edges)")
    if samples is not None and samples != V:
        raise ValueError(f"edge_validity: samples={samples!r}, validity {tuple(validity.shape)} has {V}")
    if any(t.device != weight.device for t in (validity, crow, col)):
        raise ValueError(f"edge_validity: weight is on {weight.device}, validity on {validity.device}, crow on {crow.device} "
                         f"and col on {col.device}")
    return V, N, T, nnz, _edge_exempt("edge_validity", exempt, nnz, weight.device)


_EDGE_VALIDITY_TABLES = {}            # (mode, T, device) -> the table as a tensor there, for the torch restatement


def edge_validity_reference(weight: torch.Tensor, validity: torch.Tensor, crow: torch.Tensor, col: torch.Tensor, *,
                            mode="scale", exempt: Optional[torch.Tensor] = None,
                            samples: Optional[int] = None) -> torch.Tensor:
    """`edge_validity` restated with torch ops, on whichever device the operands are: a compare and a sum for the counts, a
    table gather, a gather by source node, a compare, a select, one fp32 multiply and the exempt edges' select.  What the op
    runs for CPU tensors, and the torch-op formulation the measurements compare against."""
    V, N, T, nnz, exempt = _edge_validity_operands(weight, validity, crow, col, exempt, samples)
    key = (mode, T, str(weight.device))
    table = _EDGE_VALIDITY_TABLES.get(key)
    if table is None:                  # kept per (mode, T, device): a captured step cannot copy it from the host
        table = _EDGE_VALIDITY_TABLES[key] = torch.tensor(edge_validity_table(mode, T), dtype=torch.float32,
                                                          device=weight.device)
    g = table[(validity > 0.5).sum(-1)].index_select(1, col.long())          # [V,nnz]: the gate of each edge's source node
    w = weight if weight.dim() == 2 else weight[None, :].expand(V, nnz)
    out = torch.where(g == 0, torch.zeros((), dtype=torch.float32, device=weight.device), w * g)
    return out if exempt is None else torch.where(exempt.bool()[None, :], w, out)


class _EdgeValidityFunction(torch.autograd.Function):
    """w [nnz] or [V,nnz], validity [V,N,T] -> w * g [V,nnz] on `pattern`'s structure (msgat_edge_validity); backward
    re-creates the gate from `validity`.  Values cross in the caller's order of (crow, col) (`_CallerOrder`)."""

    @staticmethod
    def forward(ctx, w, validity, exempt, pattern, table):
        L = _lib.checked()
        V, N, T = validity.shape
        if validity.stride(2) != 1 or validity.stride(1) != T or (V > 1 and validity.stride(0) < 0):
            validity = validity.contiguous()               # the kernel wants [N,T] rows contiguous; any sample stride is read
        nnz = pattern.structure.nnz
        sets = int(w.dim() == 2)
        gstruct, keep = pattern.structure.on(w.device)
        order = _CallerOrder(pattern, w.device)
        w, exempt = order.to_library(w), order.to_library(exempt)
        stride = validity.stride(0) if V > 1 else N * T
        ctable = (C.c_float * (T + 1))(*table)
        out = _new(w, V, nnz)
        L.msgat_edge_validity(C.byref(gstruct), _ptr(w), _ptr(exempt), _ptr(validity), stride, ctable, _ptr(out), V, T,
                              sets, _stream_handle(w.device))
        ctx.call = (gstruct, keep, order, V, T, nnz, sets, stride, ctable)
        ctx.operands = (exempt,)                           # an integer tensor the launch reads by address: nothing to version
        ctx.save_for_backward(validity)
        return order.to_caller(out)

    @staticmethod
    def backward(ctx, dout):
        L = _lib.checked()
        validity, = ctx.saved_tensors
        exempt, = ctx.operands
        gstruct, _, order, V, T, nnz, sets, stride, ctable = ctx.call
        if not ctx.needs_input_grad[0]:
            return (None,) * 5
        dout = order.to_library(dout)
        dw = _shared_weight_grad(dout, V, nnz, sets)
        if V and nnz:
            L.msgat_edge_validity_backward(C.byref(gstruct), _ptr(dout), _ptr(exempt), _ptr(validity), stride, ctable,
                                           _ptr(dw), V, T, sets, _stream_handle(dout.device))
        return (order.to_caller(dw),) + (None,) * 4


def edge_validity(weight: torch.Tensor, validity: torch.Tensor, crow: torch.Tensor, col: torch.Tensor, *, mode="scale",
                  exempt: Optional[torch.Tensor] = None, samples: Optional[int] = None) -> torch.Tensor:
    """Validity-gated edges on one sparse pattern: a sensor whose input window has missing readings sends weaker messages
    to its neighbours, or none.  `weight` [nnz] -- shared by the V samples -- or [V,nnz] in the order of (`crow` [N+1], `col`
    [nnz]); `validity` [V,N,T]: the validity channel of the samples' input windows (1 = measured, 0 = imputed,
    `make_loaders(..., input_null_value=..., mask_channel=True)`), T in {4, 8, 12, 16}.  Edge e, whose SOURCE node is
    col(e) (row i of the adjacency gathers from its columns), gets `weight * table[count]` with `count` the number of
    readings `> 0.5` in the source node's window and `table = edge_validity_table(mode, T)`: "scale" c / T, "drop" all or
    nothing, an int m keeps the edges of a node with at least m readings.  A gate of 0 gives +0 whatever the weight holds;
    edges flagged in `exempt` (bool or uint8 [nnz]) pass through unchanged.  The result [V,nnz] is contiguous:
    `edge_adjacency(crow, col, ·)` reads it where it is.

    `validity` is read where it is when its last two dimensions are contiguous (the view `X[:, 0, -1]` of a contiguous
    X [B,R,C,N,T]), aligned or not; it is data and gets no gradient.  Backward re-creates the gate instead of storing it:
    `weight` [V,nnz] gets `dout * g`, `weight` [nnz] the sum over the samples in ascending order; one launch each way, no
    atomics, capturable (msgat_edge_validity{,_backward}).  Row v depends on sample v alone, so rows [lo, hi) of a V-row
    call are the call on that shard.  CPU tensors run `edge_validity_reference`, the same arithmetic in torch ops."""
    V, N, T, nnz, exempt = _edge_validity_operands(weight, validity, crow, col, exempt, samples)
    table = edge_validity_table(mode, T)
    if not weight.is_cuda:
        return edge_validity_reference(weight, validity, crow, col, mode=mode, exempt=exempt, samples=samples)
    return _EdgeValidityFunction.apply(weight, validity.detach(), exempt, edge_pattern_of(crow, col), table)


# ---- channel axes assembled from several tensors: one pass instead of cat / several mixes -------------------

def _sliced_grad(dz: torch.Tensor, accepts):
    """(tensor, group stride in channels) for an incoming [G,Ck,N,T] gradient: used in place when it is contiguous
    (stride 0 = "its own width") or a channel slice [:, a:b] of a contiguous wider tensor AND the library reads such
    slices in place for this shape and graph (`accepts()`); a contiguous copy otherwise."""
    if dz.is_contiguous():
        return dz, 0
    G, Ck, N, T = dz.shape
    st = dz.stride()
    if dz.numel() > 0 and st[1:] == (N * T, T, 1) and st[0] % (N * T) == 0 and st[0] // (N * T) > Ck and accepts():
        return dz, st[0] // (N * T)
    return dz.contiguous(), 0


def _as_segment(t: torch.Tensor):
    """(tensor to keep alive, Seg) for a [G,Ck,N,T] tensor: used in place when it is contiguous or a channel
    slice [:, a:b] of a contiguous wider tensor (the library addresses such slices directly), copied otherwise."""
    G, Ck, N, T = t.shape
    st = t.stride()
    if t.numel() > 0 and st[1:] == (N * T, T, 1) and st[0] % (N * T) == 0 and st[0] // (N * T) >= Ck:
        return t, _lib.Seg(t.data_ptr(), Ck, st[0] // (N * T))
    t = t.contiguous()
    return t, _lib.Seg(t.data_ptr(), Ck, 0)


def _seg_array(tensors):
    keep, segs = [], []
    for t in tensors:
        k, sg = _as_segment(t)
        keep.append(k)
        segs.append(sg)
    arr = (_lib.Seg * max(len(segs), 1))(*segs)
    return keep, arr, len(segs)


class _MixMultiFunction(torch.autograd.Function):
    """outs = split(relu?(M cat(ins) + bias + cat(adds))): see include/msgat_hip.h, msgat_mix_segments."""

    @staticmethod
    def forward(ctx, M, bias, relu, n_in, n_add, out_channels, premasked, *tensors):
        L = _lib.checked()
        ins, adds = tensors[:n_in], tensors[n_in:n_in + n_add]
        G, _, N, T = ins[0].shape
        M = M.contiguous()
        R = M.shape[0]
        outs = [_new(ins[0], G, c, N, T) for c in out_channels]
        kin, ain, _ = _seg_array(ins)
        _kad, aad, _ = _seg_array(adds)
        _, aout, _ = _seg_array(outs)
        b = None if bias is None else bias.contiguous()
        per_rel = int(b is not None and b.dim() == 2)         # bias [Co] or [R,Co] (one row per matrix)
        L.msgat_mix_segments(R, G // R, N, T, ain, n_in, _ptr(M), 0, _ptr(b), per_rel, aad, n_add, int(relu), aout,
                             len(outs), _stream_handle(M.device))
        relu_bwd = bool(relu and not premasked)   # premasked: the consumer of the output applies the ReLU's backward mask
        ctx.meta = (relu_bwd, n_in, tuple(out_channels), (0 if bias is None else (R if per_rel else -1)),
                    [t.shape[1] for t in ins], [t.shape[1] for t in adds])
        ctx.save_for_backward(M, *kin, *(outs if relu_bwd else []))
        return tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        L = _lib.checked()
        relu, n_in, out_channels, has_bias, in_channels, add_channels = ctx.meta
        saved = ctx.saved_tensors
        M, ins, outs = saved[0], saved[1:1 + n_in], saved[1 + n_in:]
        like = ins[0]
        G, _, N, T = like.shape
        R = M.shape[0]
        stream = _stream_handle(M.device)
        dpre = []
        for i, (d, c) in enumerate(zip(douts, out_channels)):
            if d is None:
                d = torch.zeros(G, c, N, T, device=like.device, dtype=torch.float32)
            if relu:  # ReLU mask in one pass: dout where out > 0, else 0
                d = torch.ops.aten.threshold_backward(d.contiguous(), outs[i], 0.0)
            dpre.append(d)
        kd, ad, nd = _seg_array(dpre)
        need = ctx.needs_input_grad
        dM = dbias = None
        d_ins = [None] * n_in
        # one input, its gradient and the matrix gradient both wanted: ONE pass over cat(dpre) and the input gives both
        both = n_in == 1 and need[0] and need[7]
        if any(need[7:7 + n_in]):   # d cat(ins) = M^T cat(dpre), each input's range to its own tensor
            d_ins = [_new(like, G, c, N, T) for c in in_channels]
        if any(need[7:7 + n_in]) and not both:
            _, ai, _ = _seg_array(d_ins)
            L.msgat_mix_segments(R, G // R, N, T, ad, nd, _ptr(M), 1, None, 0, None, 0, 0, ai, n_in, stream)
        want_bias = bool(has_bias and need[1])   # has_bias: 0 none, -1 shared [Co], R per matrix [R,Co]
        if need[0]:
            Co = sum(out_channels)
            parts = []
            for i, (x, c) in enumerate(zip(ins, in_channels)):
                x = x.contiguous()
                ones = int(want_bias and i == 0)   # the bias gradient = contraction with a virtual channel of ones
                buf = _new(like, R * Co * (c + ones))
                part = _scratch(like, L.msgat_contract_mix_partial_floats(R, G // R, N, T, Co, c + ones) if both
                                else L.msgat_contract_segments_partial_floats(R, Co, c + ones))
                # with_ones = 2: the matrix [R,Co,c] and, behind it, the ones column [R,Co] -- two contiguous tensors (a
                # column slice handed down to the components' parameters would cost a copy per component in AccumulateGrad)
                if both:
                    L.msgat_contract_mix_segments(R, G // R, N, T, ad, nd, _ptr(x), c, 2 * ones, _ptr(M), _ptr(part),
                                                  _ptr(buf), _ptr(d_ins[0]), stream)
                else:
                    L.msgat_contract_segments(R, G // R, N, T, ad, nd, _ptr(x), c, 2 * ones, _ptr(part), _ptr(buf), stream)
                if ones:
                    colsum = buf[R * Co * c:].view(R, Co)                   # [R,Co]: sum over the relation's groups and positions
                    dbias = colsum if has_bias > 0 else colsum.sum(dim=0)
                parts.append(buf[: R * Co * c].view(R, Co, c))
            dM = parts[0] if len(parts) == 1 else torch.cat(parts, dim=2)
        elif want_bias:
            dbias = torch.cat([_channel_sums(k.contiguous(), max(has_bias, 0)) for k in kd], dim=-1)
        d_adds = []
        if add_channels:   # channel ranges of cat(dpre), as views (the library reads channel slices in place)
            whole = dpre[0] if len(dpre) == 1 else torch.cat(dpre, dim=1)
            a = 0
            for c in add_channels:
                d_adds.append(whole[:, a:a + c])
                a += c
        return (dM, dbias, None, None, None, None, None, *d_ins, *d_adds)


def mix_multi(ins, M, bias=None, adds=(), relu=False, out_channels=None, relu_grad_premasked=False):
    """One channel-mixing pass over cat(ins) with the [R, Co, Ci] matrix M (R | batch): relu?(M cat(ins) + bias +
    cat(adds)), the output channel ranges `out_channels` written to separate tensors (default: one).  Returns a
    tuple.  Replaces torch.cat + several 1x1 convolutions by a single read of the inputs.

    `relu_grad_premasked=True` (with relu): EVERY consumer of the output promises to hand back a gradient that is
    already zero where the output is <= 0 (`layer_norm_t(..., relu_input=True)` does, inside its backward kernel), so
    this op's backward skips its own mask pass over the activation."""
    ins, adds = list(ins), list(adds)
    for t in ins + adds:
        _require_device_tensor("signals", t)
    _require_device_tensor("matrix", M, ins[0].device)
    Ci, Co = sum(t.shape[1] for t in ins), M.shape[1]
    out_channels = [Co] if out_channels is None else list(out_channels)
    if M.dim() != 3 or M.shape[2] != Ci or sum(out_channels) != Co or ins[0].shape[0] % M.shape[0]:
        raise ValueError(f"mix_multi: matrix {tuple(M.shape)} for {Ci} input / {out_channels} output channels")
    if adds and sum(t.shape[1] for t in adds) != Co:
        raise ValueError("mix_multi: the add operands must cover the output channels")
    if relu and len(out_channels) != 1:
        raise ValueError("mix_multi: relu needs a single output tensor")
    if bias is not None and tuple(bias.shape) not in ((Co,), (M.shape[0], Co)):
        raise ValueError(f"bias must be [{Co}] or [{M.shape[0]},{Co}]")
    if max(len(ins), len(adds), len(out_channels)) > 6:
        raise ValueError("mix_multi: at most 6 tensors per channel axis")
    return _MixMultiFunction.apply(M, bias, bool(relu), len(ins), len(adds), tuple(out_channels),
                                   bool(relu and relu_grad_premasked), *ins, *adds)


class _AttentionCoreFunction(torch.autograd.Function):
    """u[G,Cu,N,T], q[G,N,T], Wg[R,T,T] -> z = (softmax(q Wg q^T) . adj) u: attention.py:34-36 on features and
    pooled signals that were produced elsewhere (msgat_stage_scores + msgat_stage_aggregate; backward
    msgat_attention_backward)."""

    @staticmethod
    def forward(ctx, u, q, Wg, graph, recording: bool = True, adj_grad=None, adj=None, weights=None):   # see _GACNFunction
        L = _lib.checked()
        u, q, Wg = u.contiguous(), q.contiguous(), Wg.contiguous()
        G, Cu, N, T = u.shape
        R = Wg.shape[0]
        dev = u.device
        training_form = bool(recording)                              # see _GACNFunction.forward: the grad mode alone
        need_bwd = training_form and any(ctx.needs_input_grad)
        # the GACN plan of a graph attention over Cu channels, without the q slot: kW, lse, pq, E, E in CSC order in one
        # buffer, the scratch sizes asked for once
        plan = _gacn_plan(graph, dev, R, G // R, Cu, 0, N, T, training_form, own_q=False)
        z = torch.empty_like(u)
        buf = torch.empty(plan.total, device=dev, dtype=torch.float32)
        _, kW, lse, pq, E, Ec, _ = plan.pointers(buf)
        dense_t = torch.empty(plan.ndense, device=dev, dtype=torch.uint8) if plan.ndense else None
        scratch = _new(u, plan.nscratch) if plan.nscratch else None
        stream = _stream_handle(dev)
        shape, gstruct = C.byref(plan.shape), C.byref(plan.gstruct)
        L.msgat_stage_scores(shape, gstruct, _ptr(q), _ptr(Wg), kW, lse, pq, E, Ec, _ptr(dense_t), stream)
        L.msgat_stage_aggregate(shape, gstruct, Cu, _ptr(u), E, _ptr(z), _ptr(scratch), stream)
        if need_bwd:
            ctx.plan, ctx.adj_grad, ctx.weights = plan, adj_grad, weights
            ctx.save_for_backward(u, q, Wg, buf)
        if weights is None:
            return z
        ctx.set_materialize_grads(False)
        w = _forward_weights(weights, plan, graph.nnz, buf, _ptr(q), kW, lse, stream)
        if weights == "softmax":
            ctx.mark_non_differentiable(w)
        return z, w

    @staticmethod
    def backward(ctx, dz, dE=None):
        L = _lib.checked()
        u, q, Wg, buf = ctx.saved_tensors
        plan = ctx.plan
        _, kW, lse, pq, E, Ec, _ = plan.pointers(buf)
        shape, gstruct = C.byref(plan.shape), C.byref(plan.gstruct)
        if dz is None:                        # only the attention weights reached the loss
            dz = torch.zeros_like(u)
        dP = None
        if dE is not None and ctx.weights == "softmax_grad":
            dP, dE = dE, None                 # the gradient at the dense map (see _GACNFunction.backward)
        if dE is not None:
            dE = dE.contiguous()
        dz, dz_gs = _sliced_grad(dz, lambda: L.msgat_attention_bwd_accepts_strided_dv(shape, gstruct))
        du, dq, dWg = torch.empty_like(u), torch.empty_like(q), torch.empty_like(Wg)
        if plan.bwd_bytes is None:
            plan.bwd_bytes = max(int(L.msgat_attention_bwd_workspace_bytes(shape, gstruct)), 256)
        ws = torch.empty(plan.bwd_bytes, device=u.device, dtype=torch.uint8)
        stream = _stream_handle(u.device)
        if dE is None:
            L.msgat_attention_backward(shape, gstruct, _ptr(u), _ptr(dz), dz_gs, _ptr(q), kW, lse, pq, E, Ec, _ptr(Wg),
                                       _ptr(du), _ptr(dq), _ptr(dWg), _ptr(ws), ws.numel(), stream)
        else:
            L.msgat_attention_backward_edge_grad(shape, gstruct, _ptr(u), _ptr(dz), dz_gs, _ptr(q), kW, lse, pq, E, Ec,
                                                 _ptr(Wg), _ptr(du), _ptr(dq), _ptr(dWg), _ptr(ws), ws.numel(),
                                                 _ptr(dE), stream)
        if dP is not None:                    # dq and dWg are outputs here: the map's share is added to them
            _map_grad(plan, _ptr(q), kW, lse, Wg, dP, dq, dWg, stream)
        dadj = None if ctx.adj_grad is None else ctx.adj_grad(plan, u.shape[1], dz, dz_gs, _ptr(u), _ptr(q), kW, lse, stream,
                                                              dE)
        return du, dq, dWg, None, None, None, dadj, None


def attention_core(u: torch.Tensor, q: torch.Tensor, Wg: torch.Tensor, adjacency, need_weights: bool = False,
                   weights: str = "masked"):
    """Graph attention on already projected features `u` [G,Cu,N,T] with pooled signals `q` [G,N,T].  `adjacency` as in
    `gacn`, its gradient included; `need_weights` / `weights` as in `gacn` (a loss on a "softmax_grad" map reaches `q`
    and `Wg`, not `u`)."""
    if need_weights and _check_weights(weights) == "softmax":
        _refuse_softmax_grad(u, q, Wg, adjacency, getattr(adjacency, "_msgat_edge_weight", None))
    _require_device_tensor("features", u)
    _require_device_tensor("pooled signals", q, u.device)
    _require_device_tensor("Wg", Wg, u.device)
    G, Cu, N, T = u.shape
    if tuple(q.shape) != (G, N, T) or Wg.dim() != 3 or tuple(Wg.shape[1:]) != (T, T) or G % Wg.shape[0]:
        raise ValueError(f"attention_core: u {tuple(u.shape)}, q {tuple(q.shape)}, Wg {tuple(Wg.shape)}")
    recording = torch.is_grad_enabled()
    graph, adj, adj_grad = _resolve_adjacency(adjacency, u.device, G, Wg.shape[0], N, recording)
    if not need_weights:
        sink = _sink_slot.sink
        if sink is None:
            return _AttentionCoreFunction.apply(u, q, Wg, graph, recording, adj_grad, adj)
        z, w = _AttentionCoreFunction.apply(u, q, Wg, graph, recording, adj_grad, adj, sink.form)
        sink.append(w, graph)
        return z
    z, w = _AttentionCoreFunction.apply(u, q, Wg, graph, recording, adj_grad, adj, weights)
    return z, _weights_out(w, graph, weights, (G,))


# ---- the tiny attention matrices of a MEAM block, one launch each way ----------------------------------------------

class _ChannelAttentionMixFunction(torch.autograd.Function):
    """pooled[G,C,T], Wc[R,T,T], conv[R,cb,C] -> Mc[G,cb,C] = conv_r softmax((p Wc_r) p^T): attention.py:88-94 folded
    with CACN's 1x1 convolution weight (msgat.py:93-94)."""

    @staticmethod
    def forward(ctx, pooled, Wc, conv):
        L = _lib.checked()
        pooled, Wc, conv = pooled.contiguous(), Wc.contiguous(), conv.contiguous()
        G, Cc, T = pooled.shape
        R, cb = Wc.shape[0], conv.shape[1]
        att, Mc = _new(pooled, G, Cc, Cc), _new(pooled, G, cb, Cc)
        L.msgat_channel_attention_forward(_ptr(pooled), _ptr(Wc), _ptr(conv), _ptr(att), _ptr(Mc), G, R, Cc, cb, T,
                                          _stream_handle(pooled.device))
        ctx.save_for_backward(pooled, Wc, conv, att)
        return Mc

    @staticmethod
    def backward(ctx, dMc):
        L = _lib.checked()
        pooled, Wc, conv, att = ctx.saved_tensors
        G, Cc, T = pooled.shape
        R, cb = Wc.shape[0], conv.shape[1]
        dMc = dMc.contiguous()
        dp, dWc, dconv = torch.empty_like(pooled), torch.empty_like(Wc), torch.empty_like(conv)
        part = _scratch(pooled, L.msgat_channel_attention_partial_floats(G, Cc, cb, T))
        L.msgat_channel_attention_backward(_ptr(dMc), _ptr(att), _ptr(pooled), _ptr(Wc), _ptr(conv), _ptr(dp),
                                           _ptr(dWc), _ptr(dconv), _ptr(part), G, R, Cc, cb, T,
                                           _stream_handle(pooled.device))
        return dp, dWc, dconv


def channel_attention_fused(C: int, cb: int, T: int) -> bool:
    """Whether `channel_attention_mix` has its one-launch kernels for these sizes in BOTH directions (the backward keeps
    more in LDS than the forward: include/msgat_hip.h, msgat_channel_attention_fused); else use `channel_matrix`."""
    return bool(_lib.checked().msgat_channel_attention_fused(int(C), int(cb), int(T)))


def channel_attention_mix(pooled: torch.Tensor, Wc: torch.Tensor, conv: torch.Tensor) -> torch.Tensor:
    """The per-sample channel matrix of CACN: conv @ softmax(pooled Wc pooled^T)  ([G,cb,C]).  pooled [G,C,T] (node-weighted
    sums, `node_pool`), Wc [T,T] or [R,T,T], conv [cb,C] or [R,cb,C] with R dividing G.  Sizes whose backward has no
    kernel (`channel_attention_fused`) are refused here, under autograd, not in the middle of `backward()`."""
    _require_device_tensor("pooled signals", pooled)
    _require_device_tensor("Wc", Wc, pooled.device)
    _require_device_tensor("conv weight", conv, pooled.device)
    if Wc.dim() == 2:
        Wc, conv = Wc.unsqueeze(0), conv.unsqueeze(0)
    G, Cc, T = pooled.shape
    if tuple(Wc.shape[1:]) != (T, T) or conv.dim() != 3 or conv.shape[0] != Wc.shape[0] or conv.shape[2] != Cc or G % Wc.shape[0]:
        raise ValueError(f"channel_attention_mix: pooled {tuple(pooled.shape)}, Wc {tuple(Wc.shape)}, conv {tuple(conv.shape)}")
    if torch.is_grad_enabled() and (pooled.requires_grad or Wc.requires_grad or conv.requires_grad) and \
            not channel_attention_fused(Cc, conv.shape[1], T):
        raise ValueError(f"channel_attention_mix: no backward kernel for C = {Cc}, cb = {conv.shape[1]}, T = {T} "
                         "(channel_attention_fused); channel_matrix evaluates these sizes with torch ops")
    return _ChannelAttentionMixFunction.apply(pooled, Wc, conv)


def channel_matrix(pooled: torch.Tensor, Wc: torch.Tensor, conv: torch.Tensor) -> torch.Tensor:
    """`channel_attention_mix` where its kernels hold the problem in both directions, decided from the shapes before
    anything is launched; beyond that (wider than 114 channels at T = 12, cb = C / 3) the same chain as batched torch ops,
    as the temporal attention does beyond its lane budget (model.TACN.first_taps).  What CACN calls, in both schedules."""
    if Wc.dim() == 2:
        Wc, conv = Wc.unsqueeze(0), conv.unsqueeze(0)
    G, Cc, T = pooled.shape
    R, cb = Wc.shape[0], conv.shape[1]
    if channel_attention_fused(Cc, cb, T):
        return channel_attention_mix(pooled, Wc, conv)
    per_r = pooled.reshape(R, G // R, Cc, T)
    att = torch.softmax(per_r @ Wc.unsqueeze(1) @ per_r.transpose(2, 3), dim=-1)       # [R,B,C,C]
    return (conv.unsqueeze(1) @ att).reshape(G, cb, Cc)


class _TemporalAttentionTapsFunction(torch.autograd.Function):
    """pooled[G,N,T], Wt1/Wt2[R,K,N] -> taps[G,2,T,T]: (att shifted down by the dilation, att) with
    att = softmax((q^T Wt1^T)(q^T Wt2^T)^T), attention.py:58-66 as the taps of TACN's first convolution (msgat.py:66-74)."""

    @staticmethod
    def forward(ctx, pooled, Wt1, Wt2, dilation: int):
        L = _lib.checked()
        pooled, Wt1, Wt2 = pooled.contiguous(), Wt1.contiguous(), Wt2.contiguous()
        G, N, T = pooled.shape
        R, K = Wt1.shape[0], Wt1.shape[1]
        lr, att, taps = _new(pooled, G, 2, T, K), _new(pooled, G, T, T), _new(pooled, G, 2, T, T)
        L.msgat_temporal_attention_forward(_ptr(pooled), _ptr(Wt1), _ptr(Wt2), _ptr(lr), _ptr(att), _ptr(taps), G, R, N,
                                           K, T, int(dilation), _stream_handle(pooled.device))
        ctx.dilation = int(dilation)
        ctx.save_for_backward(pooled, Wt1, Wt2, lr, att)
        return taps

    @staticmethod
    def backward(ctx, dtaps):
        L = _lib.checked()
        pooled, Wt1, Wt2, lr, att = ctx.saved_tensors
        G, N, T = pooled.shape
        R, K = Wt1.shape[0], Wt1.shape[1]
        dtaps = dtaps.contiguous()
        dp, dW1, dW2 = torch.empty_like(pooled), torch.empty_like(Wt1), torch.empty_like(Wt2)
        part = _scratch(pooled, L.msgat_temporal_attention_partial_floats(G, K, N))
        L.msgat_temporal_attention_backward(_ptr(dtaps), _ptr(att), _ptr(lr), _ptr(pooled), _ptr(Wt1), _ptr(Wt2), _ptr(dp),
                                            _ptr(dW1), _ptr(dW2), _ptr(part), G, R, N, K, T, ctx.dilation,
                                            _stream_handle(pooled.device))
        return dp, dW1, dW2, None


def temporal_attention_taps(pooled: torch.Tensor, Wt1: torch.Tensor, Wt2: torch.Tensor, dilation: int) -> torch.Tensor:
    """[G,2,T,T] taps of TACN's first causal convolution: (temporal attention shifted down by `dilation`, temporal
    attention).  pooled [G,N,T] (alpha-weighted channel sums, `channel_pool`), Wt1 / Wt2 [K,N] or [R,K,N]."""
    _require_device_tensor("pooled signals", pooled)
    _require_device_tensor("Wt1", Wt1, pooled.device)
    _require_device_tensor("Wt2", Wt2, pooled.device)
    if Wt1.dim() == 2:
        Wt1, Wt2 = Wt1.unsqueeze(0), Wt2.unsqueeze(0)
    G, N, T = pooled.shape
    if Wt1.shape != Wt2.shape or Wt1.dim() != 3 or Wt1.shape[2] != N or G % Wt1.shape[0] or 2 * T * Wt1.shape[1] > 256:
        raise ValueError(f"temporal_attention_taps: pooled {tuple(pooled.shape)}, Wt1 {tuple(Wt1.shape)}, Wt2 {tuple(Wt2.shape)}")
    return _TemporalAttentionTapsFunction.apply(pooled, Wt1, Wt2, int(dilation))


class _BiasJoinFunction(torch.autograd.Function):
    """wide [R,Co] + narrow [R,cb] added into its first cb columns: CACN's convolution bias joining the residual bias in
    front of MEAM's ReLU (both per-channel constants, msgat.py:94,123-131).  pad + add cost three launches forward and a
    slice copy backward; here a copy and an in-place add, and backward hands the incoming gradient to `wide` and a copy
    of its leading columns to `narrow`.  (Not a view of them: AccumulateGrad keeps a gradient it is the only holder of,
    and a view counts as one, so the .grad of CACN's bias lay INSIDE the .grad of the residual bias -- a second backward
    into them, or any in-place edit of one, changed the other.)"""

    @staticmethod
    def forward(ctx, wide, narrow):
        out = wide.clone()
        out[:, : narrow.shape[1]].add_(narrow)
        ctx.cb = narrow.shape[1]
        return out

    @staticmethod
    def backward(ctx, g):
        return g, g[:, : ctx.cb].clone()


def bias_join(wide: torch.Tensor, narrow: torch.Tensor) -> torch.Tensor:
    """`wide + pad(narrow)`: [R,Co] plus [R,cb <= Co] in the leading columns."""
    if wide.dim() != 2 or narrow.dim() != 2 or wide.shape[0] != narrow.shape[0] or narrow.shape[1] > wide.shape[1]:
        raise ValueError(f"bias_join: {tuple(wide.shape)} and {tuple(narrow.shape)}")
    return _BiasJoinFunction.apply(wide, narrow)


class _AssembleRowsFunction(torch.autograd.Function):
    """per_group [G,A,C], per_relation [R,Kr,C] -> rows [G,A+Kr,C]: each group's own rows followed by its relation's.
    Two copies forward; backward = a view of the first block and ONE sum over each relation's groups for the second
    (torch.cat of expanded tensors costs a copy per operand forward and a reduction per operand backward)."""

    @staticmethod
    def forward(ctx, per_group, per_relation):
        G, A, Cc = per_group.shape
        R, Kr, _ = per_relation.shape
        rows = torch.empty(G, A + Kr, Cc, device=per_group.device, dtype=torch.float32)
        rows[:, :A].copy_(per_group)
        rows.view(R, G // R, A + Kr, Cc)[:, :, A:].copy_(per_relation.unsqueeze(1))
        ctx.dims = (G, A, Cc, R, Kr)
        return rows

    @staticmethod
    def backward(ctx, drows):
        G, A, Cc, R, Kr = ctx.dims
        d_rel = drows.view(R, G // R, A + Kr, Cc)[:, :, A:].sum(dim=1) if ctx.needs_input_grad[1] else None
        return (drows[:, :A] if ctx.needs_input_grad[0] else None), d_rel


def assemble_rows(per_group: torch.Tensor, per_relation: torch.Tensor) -> torch.Tensor:
    """[G,A,C] rows of every group followed by the [Kr,C] rows of its relation (per_relation [R,Kr,C], R | G)."""
    if per_group.dim() != 3 or per_relation.dim() != 3 or per_group.shape[2] != per_relation.shape[2] or \
            per_group.shape[0] % per_relation.shape[0]:
        raise ValueError(f"assemble_rows: {tuple(per_group.shape)} and {tuple(per_relation.shape)}")
    return _AssembleRowsFunction.apply(per_group, per_relation)


_shift_taps_cache = {}


def causal_shift_taps(T: int, dilation: int, device) -> torch.Tensor:
    """[1,2,T,T] constant taps of a plain causal dilated [1,2] convolution (identity shifted down by `dilation`, identity):
    built once per (T, dilation, device)."""
    key = (T, int(dilation), str(device))
    taps = _shift_taps_cache.get(key)
    if taps is None:
        eye = torch.eye(T, device=device, dtype=torch.float32)
        shifted = torch.zeros_like(eye)
        if dilation < T:
            shifted[dilation:] = eye[: T - dilation]
        taps = _shift_taps_cache[key] = torch.stack([shifted, eye], dim=0).unsqueeze(0).contiguous()
    return taps


class _Relayout(torch.autograd.Function):
    """t.permute(perm).contiguous() whose backward is ALSO one contiguous copy (autograd's own backward of a permute is a
    strided view: handed down to R per-component parameters it is copied R times by AccumulateGrad)."""

    @staticmethod
    def forward(ctx, t, perm):
        ctx.perm = tuple(perm)
        return t.permute(*perm).contiguous()

    @staticmethod
    def backward(ctx, g):
        inv = [0] * len(ctx.perm)
        for i, p in enumerate(ctx.perm):
            inv[p] = i
        return g.permute(*inv).contiguous(), None


def relayout(t: torch.Tensor, perm) -> torch.Tensor:
    return _Relayout.apply(t, tuple(perm))


# ---- step tail: fused loss + metric sums ----------------------------------------------
# The tail runs one of two losses (csrc/tail.hip: a policy of the same kernels), named here by the prefix of its entry
# points and the parameters in front of which they are called: ("huber", (delta,)) or ("gauss", (sigma, delta)).

def gauss_params(sigma, delta) -> tuple:
    """(sigma, delta) as floats, or ValueError: sigma finite and > 0, delta finite and >= 0 (0: no linear term)."""
    sigma, delta = float(sigma), float(delta)
    if not (math.isfinite(sigma) and sigma > 0.0):
        raise ValueError(f"sigma must be a finite number > 0, not {sigma!r}")
    if not (math.isfinite(delta) and delta >= 0.0):
        raise ValueError(f"delta must be a finite number >= 0, not {delta!r}")
    return sigma, delta


@dataclasses.dataclass(frozen=True)
class _TailCall:
    """One call of the step tail, as its entry points take it: `msgat_<stem>_metrics(pred, truth, *dims, *params, *null,
    mask_value, partials, loss, [valid,] sums, *weight, stream)`, sized by `<partials>(*dims)`, and the backward
    `msgat_<stem>_grad(pred, truth, dloss, [valid,] *dims, *grad_params, *null, dpred, stream)`."""
    stem: str              # "huber", "masked_gauss", "quantile", ...
    partials: str          # the entry that sizes the partials
    dims: tuple            # the leading dimension arguments: (n,), (rows, T_out) or (rows, T_out, Q)
    params: tuple          # the loss parameters of the forward ...
    grad_params: tuple     # ... and of the backward
    null: tuple = ()       # (null_value,) of a masked tail
    weight: tuple = ()     # (loss_weight,) of the plain tail


class _TailMetricsFunction(torch.autograd.Function):
    """pred, truth -> the mean loss (0-dim) of the tail `call` describes; adds the batch's sums to the running fp64 totals
    `sums` on the device (engine.py:56,66-70; loss.py:51-52 or :94-95; metrics.py:20-35).  With a `valid` slot [1] the
    mean is over the VALID entries of truth (not NaN, != null_value) and the slot receives their count."""

    @staticmethod
    def forward(ctx, pred, truth, call: _TailCall, mask_value: float, sums, valid):
        L = _lib.checked()
        pred_c, truth_c = pred.contiguous(), truth.contiguous()
        n_part = int(getattr(L, call.partials)(*call.dims))
        part = torch.empty(max(n_part, 1), device=pred.device, dtype=torch.float64)
        loss = torch.empty((), device=pred.device, dtype=torch.float32)
        slot = () if valid is None else (_ptr(valid),)
        name = f"msgat_{call.stem}_metrics"
        getattr(L, name)(_ptr(pred_c), _ptr(truth_c), *call.dims, *call.params, *call.null, float(mask_value),
                         _ptr(part), _ptr(loss), *slot, _ptr(sums), *call.weight, _stream_handle(pred.device))
        ctx.call = call
        ctx.save_for_backward(pred_c, truth_c, *(() if valid is None else (valid,)))
        return loss

    @staticmethod
    def backward(ctx, dloss):
        pred, truth, *valid = ctx.saved_tensors
        call = ctx.call
        dpred = torch.empty_like(pred)
        name = f"msgat_{call.stem}_grad"
        getattr(_lib.checked(), name)(_ptr(pred), _ptr(truth), _ptr(dloss.contiguous()), *(_ptr(v) for v in valid),
                                      *call.dims, *call.grad_params, *call.null, _ptr(dpred), _stream_handle(pred.device))
        return dpred, None, None, None, None, None


def _check_tail_operands(pred, truth, per_horizon: bool) -> None:
    """Prediction and target on one device, of one non-empty shape (`per_horizon`: whose last dimension is T_out)."""
    _require_device_tensor("prediction", pred)
    _require_device_tensor("target", truth, pred.device)
    if pred.shape != truth.shape or pred.numel() == 0 or (per_horizon and pred.dim() == 0):
        raise ValueError(f"prediction {tuple(pred.shape)} and target {tuple(truth.shape)} must match and be non-empty")


def _check_totals(sums, shape: tuple, device) -> None:
    """`sums` is None or the running float64 totals of `shape` on `device`: contiguous and of exactly that shape, except
    the plain tail's flat [4], of which only the element count is asked."""
    flat = len(shape) == 1
    if sums is not None and (sums.dtype != torch.float64 or sums.device != device or (
            sums.numel() != shape[0] if flat else tuple(sums.shape) != shape or not sums.is_contiguous())):
        raise ValueError(f"sums must be a {'' if flat else 'contiguous '}float64 {list(shape)} tensor on the prediction's device")


def _valid_slot(valid, device) -> torch.Tensor:
    """The float32 [1] device tensor that receives a batch's valid count: the caller's, checked, or a fresh one."""
    if valid is None:
        return torch.empty(1, device=device, dtype=torch.float32)
    if valid.dtype != torch.float32 or valid.numel() != 1 or valid.device != device:
        raise ValueError("valid must be a float32 [1] tensor on the prediction's device")
    return valid


def _loss_metrics(kind: str, params: tuple, pred, truth, mask_value, sums, loss_weight) -> torch.Tensor:
    _check_tail_operands(pred, truth, per_horizon=False)
    _check_totals(sums, (4,), pred.device)
    call = _TailCall(kind, "msgat_huber_partial_doubles", (pred.numel(),), params, params, weight=(float(loss_weight),))
    return _TailMetricsFunction.apply(pred, truth, call, mask_value, sums, None)


def _masked_loss_metrics(kind: str, params: tuple, pred, truth, null_value, mask_value, sums, valid) -> torch.Tensor:
    _check_tail_operands(pred, truth, per_horizon=True)
    t_out = pred.shape[-1]
    if t_out > 64:
        raise ValueError(f"T_out = {t_out}: the masked step tail supports forecast horizons up to 64 steps")
    _check_totals(sums, (t_out + 1, 5), pred.device)
    call = _TailCall(f"masked_{kind}", "msgat_masked_huber_partial_doubles", (pred.numel() // t_out, t_out), params, params,
                     null=(float(null_value),))
    return _TailMetricsFunction.apply(pred, truth, call, mask_value, sums, _valid_slot(valid, pred.device))


def huber_metrics(pred: torch.Tensor, truth: torch.Tensor, delta: float, mask_value: float = 0.0,
                  sums: Optional[torch.Tensor] = None, loss_weight: float = 1.0) -> torch.Tensor:
    """Mean Huber loss of `pred` against `truth` in one pass that also feeds the epoch's metric totals.
    `loss_weight` scales what is added to the running loss total (a rank's share n_r / n_b of a global batch)."""
    return _loss_metrics("huber", (float(delta),), pred, truth, mask_value, sums, loss_weight)


def gauss_metrics(pred: torch.Tensor, truth: torch.Tensor, sigma: float, delta: float, mask_value: float = 0.0,
                  sums: Optional[torch.Tensor] = None, loss_weight: float = 1.0) -> torch.Tensor:
    """`huber_metrics` with the Gauss loss (loss.py:94-95): the mean of sigma^2 (1 - exp(-e^2 / 2 sigma^2)) + delta |e|.
    `sigma` finite and > 0, `delta` finite and >= 0 (ValueError otherwise)."""
    return _loss_metrics("gauss", gauss_params(sigma, delta), pred, truth, mask_value, sums, loss_weight)


def masked_huber_metrics(pred: torch.Tensor, truth: torch.Tensor, delta: float, null_value: float,
                         mask_value: float = 0.0, sums: Optional[torch.Tensor] = None,
                         valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Huber loss of `pred` against `truth` [..., T_out] (e.g. [B, N, T_out]) averaged over the valid entries -- those
    whose truth is neither NaN nor `null_value` -- in one pass that also feeds the epoch's per-horizon metric totals
    `sums` (float64 [T_out + 1, 5], see `engine.Metrics`).  A batch without a valid entry gives 0.
    `valid` (float32 [1] on the device, optional) receives the batch's valid count; the backward divides by it on the
    device, so it must keep that value until the backward has run."""
    return _masked_loss_metrics("huber", (float(delta),), pred, truth, null_value, mask_value, sums, valid)


def masked_gauss_metrics(pred: torch.Tensor, truth: torch.Tensor, sigma: float, delta: float, null_value: float,
                         mask_value: float = 0.0, sums: Optional[torch.Tensor] = None,
                         valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`masked_huber_metrics` with the Gauss loss (see `gauss_metrics`): column 4 of `sums` receives its sums."""
    return _masked_loss_metrics("gauss", gauss_params(sigma, delta), pred, truth, null_value, mask_value, sums, valid)


# ---- step tail: quantile forecasts (pinball loss, point metrics at one level, coverage / width / crossing sums) ------
QUANTILE_MAX_LEVELS = 8
QUANTILE_BASE_COLUMNS = 7     # columns of the totals in front of the per-level ones: [T_out + 1, 7 + 2Q]


def quantile_levels(quantiles) -> tuple:
    """The levels as floats, or ValueError: 1 to 8 of them, strictly increasing inside (0, 1) -- judged on the fp32 values
    the kernels receive (0.99999999 is 1.0f)."""
    try:
        levels = tuple(float(q) for q in quantiles)
    except TypeError:
        raise ValueError(f"quantiles must be a sequence of numbers, not {quantiles!r}") from None
    if not 1 <= len(levels) <= QUANTILE_MAX_LEVELS:
        raise ValueError(f"between 1 and {QUANTILE_MAX_LEVELS} quantile levels, not {len(levels)}")
    seen = 0.0
    for q in levels:
        q32 = C.c_float(q).value
        if not (q32 > seen and q32 < 1.0):        # NaN fails both
            raise ValueError(f"quantile levels must be strictly increasing inside (0, 1), not {levels!r}")
        seen = q32
    return levels


def quantile_point(levels) -> int:
    """The index of the level nearest 0.5 (the lower one on a tie): the level that serves as the point forecast."""
    return min(range(len(levels)), key=lambda i: (abs(levels[i] - 0.5), i))


def quantile_slopes(levels, dtype=torch.float32) -> torch.Tensor:
    """[3, Q]: the slope of (1/Q) rho_q with respect to p_q where y > p_q, y < p_q and y == p_q, formed in double from the
    fp32 levels and rounded once -- the constants `msgat_quantile_grad` multiplies with."""
    tau = torch.tensor([C.c_float(q).value for q in levels], dtype=torch.float64)
    n = float(len(levels))
    return torch.stack([-tau / n, (1.0 - tau) / n, (0.5 - tau) / n]).to(dtype)


def quantile_widths(pred: torch.Tensor, truth: torch.Tensor, n_levels: int) -> int:
    """T_out of a quantile batch, or ValueError: pred [..., Q * T_out] (or [..., Q, T_out]) against truth [..., T_out]."""
    t_out = truth.shape[-1] if truth.dim() else 0
    if pred.dim() == truth.dim() + 1 and pred.dim() >= 2 and tuple(pred.shape[-2:]) == (n_levels, t_out) \
            and pred.shape[:-2] == truth.shape[:-1]:
        return t_out
    if pred.dim() != truth.dim() or pred.dim() == 0 or pred.shape[:-1] != truth.shape[:-1] or pred.shape[-1] != n_levels * t_out:
        raise ValueError(f"a forecast of {n_levels} quantile levels needs {n_levels} x {t_out} = {n_levels * t_out} outputs "
                         f"for a target of {t_out} steps, got {pred.shape[-1] if pred.dim() else 0}: prediction "
                         f"{tuple(pred.shape)}, target {tuple(truth.shape)}")
    return t_out


def quantile_metrics(pred: torch.Tensor, truth: torch.Tensor, levels, null_value: Optional[float] = None,
                     mask_value: float = 0.0, sums: Optional[torch.Tensor] = None, valid: Optional[torch.Tensor] = None,
                     point: Optional[int] = None) -> torch.Tensor:
    """Pinball loss of a quantile forecast in one pass that also feeds the epoch's totals (`msgat_quantile_metrics`;
    the backward is `msgat_quantile_grad`).

    `pred` [..., Q * T_out] holds, level-major, the `Q = len(levels)` quantile forecasts of `truth` [..., T_out]
    (e.g. [B, N, Q * T_out] against [B, N, T_out]; [..., Q, T_out] is accepted too); `levels` strictly increasing inside
    (0, 1).  The loss is sum_valid (1/Q) sum_q max(tau_q u, (tau_q - 1) u), u = truth - p_q, over max(valid count, 1),
    the valid entries being those whose truth is neither NaN nor `null_value` (None: NaN only).  `sums` (float64
    [T_out + 1, 7 + 2Q], optional; see `engine.Metrics`) receives per horizon and over all horizons the masked tail's
    {count, |e|, 100 |e / y| (y > mask_value), e^2} with e = p_point - y, the loss sum, the crossing count, the width sum
    p_{Q-1} - p_0, the Q hit counts y <= p_q and the Q sums of rho_q.  `point` (default: the level nearest 0.5) names the
    level of the point forecast.  `valid` as in `masked_huber_metrics`."""
    levels = quantile_levels(levels)
    n_levels = len(levels)
    _require_device_tensor("prediction", pred)
    _require_device_tensor("target", truth, pred.device)
    if truth.dim() == 0 or truth.numel() == 0:
        raise ValueError(f"target {tuple(truth.shape)} must be non-empty")
    t_out = quantile_widths(pred, truth, n_levels)
    if n_levels * t_out > 64:
        raise ValueError(f"Q * T_out = {n_levels} * {t_out}: the quantile step tail supports up to 64 outputs per node")
    point = quantile_point(levels) if point is None else int(point)
    if not 0 <= point < n_levels:
        raise ValueError(f"point = {point} outside the {n_levels} levels")
    _check_totals(sums, (t_out + 1, QUANTILE_BASE_COLUMNS + 2 * n_levels), pred.device)
    host_levels = (C.c_float * n_levels)(*levels)
    call = _TailCall("quantile", "msgat_quantile_partial_doubles", (truth.numel() // t_out, t_out, n_levels),
                     (host_levels, point), (host_levels,), null=(float("nan") if null_value is None else float(null_value),))
    return _TailMetricsFunction.apply(pred, truth, call, mask_value, sums, _valid_slot(valid, pred.device))


# ---- input windows of a batch from a series resident in device memory ---------------------------------------------
def window_offsets(hours, tau: int, device) -> torch.Tensor:
    """`hours[r] * tau` as the int64 device array `window_gather` reads; a loader builds it once and passes it on."""
    return torch.tensor([int(h) * int(tau) for h in hours], dtype=torch.int64).to(device)


def window_gather(inputs_dev: torch.Tensor, target_dev: torch.Tensor, origins: torch.Tensor, hours, tau: int, q: int,
                  offsets: Optional[torch.Tensor] = None):
    """The batch `(X [B,R,C,N,tau], H [B], D [B], Y [B,N,q])` of the forecast origins `origins` [B] (int64, on the device)
    in one launch (`msgat_window_gather`): what collating `data.PeriodicWindows` items gives, without the host.

    `inputs_dev` is the normalised series TIME-MAJOR, [T_total, C, N] float32 (`data.upload_series` makes it from the
    host's [C, N, T_total]); `target_dev` [N, T_total] float32 is channel 0 of the raw series; `hours` a sequence of
    ints; `offsets`: what `window_offsets(hours, tau, device)` gave, for a caller that keeps it (without it the array
    is built, and copied to the device, by this call).  Origins outside [tau * max(hours), T_total - q] are clamped into
    it by the kernel.  No autograd: data."""
    return _window_gather("window_gather", inputs_dev, target_dev, origins, hours, tau, q, offsets)


def window_gather_imputed(inputs_dev: torch.Tensor, climatology_dev: torch.Tensor, target_dev: torch.Tensor,
                          origins: torch.Tensor, hours, tau: int, q: int, mask_channel: bool = True,
                          offsets: Optional[torch.Tensor] = None):
    """`window_gather` for a series whose missing readings are stored as NaN (`data.prepare_missing`), in one launch
    (`msgat_window_gather_imputed`): a NaN of a window becomes `climatology_dev[step % period, c, n]`, every other value
    keeps its bits, and with `mask_channel` X is `[B, R, C + 1, N, tau]`, its last channel 1.0 where all C channels of
    that node at that step are observed and 0.0 elsewhere.  H, D and Y as `window_gather` gives them.

    `climatology_dev` is float32 `[period, C, N]` on the device of the series (period = 1: one value per row); the
    other arguments are `window_gather`'s.  No autograd: data."""
    return _window_gather("window_gather_imputed", inputs_dev, target_dev, origins, hours, tau, q, offsets,
                          climatology_dev, bool(mask_channel))


def _window_gather(what, inputs_dev, target_dev, origins, hours, tau, q, offsets, climatology_dev=None, mask_channel=False):
    """The argument checks and the launch of `window_gather` and, with a table, of `window_gather_imputed`."""
    floats = [("inputs_dev", inputs_dev), ("target_dev", target_dev)]
    if climatology_dev is not None:
        floats.append(("climatology_dev", climatology_dev))
    for name, t in floats:
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be float32, got {t.dtype}")
    if origins.dtype != torch.int64:
        raise TypeError(f"{what}: origins must be int64, got {origins.dtype}")
    for name, t in floats[1:] + [("origins", origins)]:
        if t.device != inputs_dev.device:
            raise ValueError(f"{what}: inputs_dev on {inputs_dev.device} and {name} on {t.device} must share one device")
    hours = [int(h) for h in hours]
    if not hours or min(hours) < 1:
        raise ValueError(f"{what}: hours {hours} must be a non-empty sequence of positive ints")
    if tau not in (4, 8, 12, 16) or not 1 <= q <= 64:
        raise ValueError(f"{what}: tau = {tau} must be 4, 8, 12 or 16 and q = {q} between 1 and 64")
    if inputs_dev.dim() != 3 or target_dev.dim() != 2 or origins.dim() != 1 or origins.numel() == 0:
        raise ValueError(f"{what}: inputs_dev {tuple(inputs_dev.shape)} must be [T_total, C, N], target_dev "
                         f"{tuple(target_dev.shape)} [N, T_total] and origins {tuple(origins.shape)} a non-empty [B]")
    T_total, C_, N = inputs_dev.shape
    if tuple(target_dev.shape) != (N, T_total):
        raise ValueError(f"{what}: target_dev {tuple(target_dev.shape)} does not fit inputs_dev [T_total = {T_total}, "
                         f"C = {C_}, N = {N}]: expected [{N}, {T_total}]")
    if climatology_dev is not None and (climatology_dev.dim() != 3 or climatology_dev.shape[0] < 1
                                        or tuple(climatology_dev.shape[1:]) != (C_, N)):
        raise ValueError(f"{what}: climatology_dev {tuple(climatology_dev.shape)} must be [period >= 1, {C_}, {N}]")
    history = tau * max(hours)
    if T_total < history + q:
        raise ValueError(f"{what}: a series of {T_total} steps is shorter than tau * max(hours) + q = {history + q}")
    if not all(t.is_contiguous() for _, t in floats + [("origins", origins)]):
        raise ValueError(f"{what}: {', '.join(name for name, _ in floats)} and origins must be contiguous")
    _require_device_tensor("inputs_dev", inputs_dev)
    dev, B, R = inputs_dev.device, origins.numel(), len(hours)
    if offsets is None:
        offsets = window_offsets(hours, tau, dev)
    elif offsets.dtype != torch.int64 or offsets.device != dev or tuple(offsets.shape) != (R,) or not offsets.is_contiguous():
        raise ValueError(f"{what}: offsets must be a contiguous int64 [{R}] tensor on {dev}")
    X = torch.empty((B, R, C_ + int(mask_channel), N, tau), device=dev, dtype=torch.float32)
    Y = torch.empty((B, N, q), device=dev, dtype=torch.float32)
    HD = torch.empty((2, B), device=dev, dtype=torch.int64)
    outs, dims = (_ptr(X), _ptr(HD[0]), _ptr(HD[1]), _ptr(Y)), (B, R, C_, N, T_total, tau, q, history)
    with torch.cuda.device(dev):
        if climatology_dev is None:
            _lib.checked().msgat_window_gather(_ptr(inputs_dev), _ptr(target_dev), _ptr(origins), _ptr(offsets), *outs,
                                               *dims, _stream_handle(dev))
        else:
            _lib.checked().msgat_window_gather_imputed(_ptr(inputs_dev), _ptr(climatology_dev), _ptr(target_dev),
                                                       _ptr(origins), _ptr(offsets), *outs, *dims,
                                                       climatology_dev.shape[0], int(mask_channel), _stream_handle(dev))
    return X, HD[0], HD[1], Y


# ---- online forecasting: a ring of readings in device memory and the windows of its newest origin ------------------
def _check_ring(what, ring, clock, others):
    """`ring` float32 [L,C,N] and `clock` int64 [2] on one device with the float32 tensors `others` = [(name, tensor,
    shape)], all contiguous; returns (L, C, N)."""
    for name, t, _ in [("ring", ring, None)] + others:
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be float32, got {t.dtype}")
    if clock.dtype != torch.int64:
        raise TypeError(f"{what}: clock must be int64, got {clock.dtype}")
    if ring.dim() != 3 or ring.numel() == 0:
        raise ValueError(f"{what}: ring {tuple(ring.shape)} must be a non-empty [L, C, N]")
    if tuple(clock.shape) != (2,):
        raise ValueError(f"{what}: clock {tuple(clock.shape)} must be [2]: the next step and the count of readings held")
    for name, t, shape in others + [("clock", clock, None)]:
        if t.device != ring.device:
            raise ValueError(f"{what}: ring on {ring.device} and {name} on {t.device} must share one device")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: {name} {tuple(t.shape)} must be {list(shape)}")
    if not all(t.is_contiguous() for t in [ring, clock] + [t for _, t, _ in others]):
        raise ValueError(f"{what}: ring, clock, {', '.join(name for name, _, _ in others)} must be contiguous")
    _require_device_tensor("ring", ring)
    return tuple(ring.shape)


def ring_push(raw: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, ring: torch.Tensor, clock: torch.Tensor,
              null_value: Optional[float] = None) -> None:
    """The readings `raw` [K,C,N] (float32, on the device) of K consecutive steps go, normalised as `(raw - mean) / std`
    with the bits of that torch expression, into the rows `(clock[0] + k) mod L` of `ring` [L,C,N]; then `clock[0] += K`
    and `clock[1] = min(clock[1] + K, L)`, on the device (`msgat_ring_push`: two launches, nothing read back).

    `mean`, `std` [C,N] are `data.SeriesStats`'; `clock` int64 [2].  With `null_value` a reading that is NaN or equal to it
    is stored as the canonical NaN (`null_value = nan`: the NaNs only), which `ring_windows` takes for missing.  Writes
    `ring` and `clock` in place.  No autograd: data."""
    if raw.dim() != 3 or raw.shape[0] < 1:
        raise ValueError(f"ring_push: raw {tuple(raw.shape)} must be [K >= 1, C, N]")
    L, C_, N = _check_ring("ring_push", ring, clock, [("raw", raw, (raw.shape[0], *ring.shape[1:])),
                                                       ("mean", mean, ring.shape[1:]), ("std", std, ring.shape[1:])])
    K = raw.shape[0]
    if K > L:
        raise ValueError(f"ring_push: raw holds K = {K} steps, more than the ring's L = {L}")
    dev = ring.device
    with torch.cuda.device(dev):
        _lib.checked().msgat_ring_push(_ptr(raw), _ptr(mean), _ptr(std), _ptr(ring), _ptr(clock), K, C_, N, L,
                                       int(null_value is not None), 0.0 if null_value is None else float(null_value),
                                       _stream_handle(dev))


def ring_windows(ring: torch.Tensor, clock: torch.Tensor, hours, tau: int, climatology: Optional[torch.Tensor] = None,
                 mask_channel: bool = False, offsets: Optional[torch.Tensor] = None, out=None):
    """`(X [1,R,C,N,tau], H [1], D [1])` of the forecast origin `t = clock[0]`, read on the device, in one launch
    (`msgat_ring_windows`): what `window_gather` gives for that one origin over the full series, the row of absolute step
    s read at `s mod L` of `ring` [L,C,N].  With `climatology` [period,C,N] it is `window_gather_imputed`: a NaN becomes
    `climatology[s mod period]`, and `mask_channel` appends the validity channel.

    L must be a multiple of `tau` and at least `tau * max(hours)`; whether the ring holds enough readings is the caller's
    to know (`clock[1]`; `OnlineForecaster.ready`).  `offsets` as for `window_gather`.  `out=(X, H, D)`: caller-owned
    buffers of those shapes to write into (a captured step needs them).  No autograd: data."""
    what = "ring_windows"
    others = [] if climatology is None else [("climatology", climatology, None)]
    L, C_, N = _check_ring(what, ring, clock, others)
    hours = [int(h) for h in hours]
    if not hours or min(hours) < 1:
        raise ValueError(f"{what}: hours {hours} must be a non-empty sequence of positive ints")
    if tau not in (4, 8, 12, 16):
        raise ValueError(f"{what}: tau = {tau} must be 4, 8, 12 or 16")
    if L % tau or L < tau * max(hours):
        raise ValueError(f"{what}: the ring's L = {L} must be a multiple of tau = {tau} and at least tau * max(hours) = "
                         f"{tau * max(hours)}")
    if climatology is None and mask_channel:
        raise ValueError(f"{what}: mask_channel needs a climatology (a ring without a table has no missing readings)")
    if climatology is not None and (climatology.dim() != 3 or climatology.shape[0] < 1
                                    or tuple(climatology.shape[1:]) != (C_, N)):
        raise ValueError(f"{what}: climatology {tuple(climatology.shape)} must be [period >= 1, {C_}, {N}]")
    dev, R = ring.device, len(hours)
    if offsets is None:
        offsets = window_offsets(hours, tau, dev)
    elif offsets.dtype != torch.int64 or offsets.device != dev or tuple(offsets.shape) != (R,) or not offsets.is_contiguous():
        raise ValueError(f"{what}: offsets must be a contiguous int64 [{R}] tensor on {dev}")
    x_shape = (1, R, C_ + int(bool(mask_channel)), N, tau)
    if out is None:
        X = torch.empty(x_shape, device=dev, dtype=torch.float32)
        HD = torch.empty((2, 1), device=dev, dtype=torch.int64)
        H, D = HD[0], HD[1]
    else:
        X, H, D = out
        for name, t, shape, dtype in (("X", X, x_shape, torch.float32), ("H", H, (1,), torch.int64),
                                      ("D", D, (1,), torch.int64)):
            if t.dtype != dtype or t.device != dev or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{what}: out's {name} must be a contiguous {dtype} {list(shape)} tensor on {dev}")
    with torch.cuda.device(dev):
        _lib.checked().msgat_ring_windows(_ptr(ring), _ptr(climatology), _ptr(clock), _ptr(offsets), _ptr(X), _ptr(H),
                                          _ptr(D), R, C_, N, L, tau, 1 if climatology is None else climatology.shape[0],
                                          int(bool(mask_channel)), _stream_handle(dev))
    return X, H, D


# ---- online forecasting, scored: the book of issued forecasts and the totals it is settled into -----------------------
SCORE_NODE_COLUMNS = 3        # node_sums [N, 3]: {valid count, sum |e|, sum e}
SCORE_NEVER = -2 ** 63        # what `issued` holds for a row that was never written


def score_columns(n_levels: int) -> int:
    """Columns of the totals `forecast_score` adds to: 5 for a point head, 7 + 2Q for Q quantile levels."""
    return 5 if not n_levels else QUANTILE_BASE_COLUMNS + 2 * int(n_levels)


def _check_book(what, book, issued, clock, others):
    """`book` float32 [P,N,out], `issued` int64 [P] and `clock` int64 [2] on one device with the tensors `others` =
    [(name, tensor, dtype, shape)], all contiguous; returns (P, N, out)."""
    for name, t, dtype, _ in [("book", book, torch.float32, None), ("issued", issued, torch.int64, None),
                              ("clock", clock, torch.int64, None)] + others:
        if t.dtype != dtype:
            raise TypeError(f"{what}: {name} must be {dtype}, got {t.dtype}")
    if book.dim() != 3 or book.numel() == 0:
        raise ValueError(f"{what}: book {tuple(book.shape)} must be a non-empty [P, N, out]")
    for name, t, _, shape in [("issued", issued, None, (book.shape[0],)), ("clock", clock, None, (2,))] + others:
        if t.device != book.device:
            raise ValueError(f"{what}: book on {book.device} and {name} on {t.device} must share one device")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: {name} {tuple(t.shape)} must be {list(shape)}")
    if not all(t.is_contiguous() for t in [book, issued, clock] + [t for _, t, _, _ in others]):
        raise ValueError(f"{what}: book, issued, clock, {', '.join(name for name, _, _, _ in others)} must be contiguous")
    _require_device_tensor("book", book)
    return tuple(book.shape)


def forecast_store(pred: torch.Tensor, book: torch.Tensor, issued: torch.Tensor, clock: torch.Tensor) -> None:
    """The forecast `pred` [N,out] of origin `clock[0]` goes into row `clock[0] mod P` of `book` [P,N,out] and that row of
    `issued` [P] (int64) is stamped with the origin, on the device (`msgat_forecast_store`: one launch, nothing read
    back; twice for one origin changes nothing).  Writes `book` and `issued` in place.  No autograd: data."""
    if pred.dim() != 2:
        raise ValueError(f"forecast_store: pred {tuple(pred.shape)} must be [N, out]")
    P, N, out = _check_book("forecast_store", book, issued, clock, [("pred", pred, torch.float32, book.shape[1:])])
    dev = book.device
    with torch.cuda.device(dev):
        _lib.checked().msgat_forecast_store(_ptr(pred), _ptr(book), _ptr(issued), _ptr(clock), N, out, P,
                                            _stream_handle(dev))


def forecast_score(raw: torch.Tensor, book: torch.Tensor, issued: torch.Tensor, clock: torch.Tensor, t_out: int,
                   sums: torch.Tensor, node_sums: torch.Tensor, levels=None, point: Optional[int] = None,
                   null_value: Optional[float] = None, mask_value: float = 0.0,
                   partials: Optional[torch.Tensor] = None) -> None:
    """Settles the forecasts in `book` [P,N,out] that the readings `raw` [K,C,N] (float32, RAW, of the steps
    `clock[0] + k`) make due: call it BEFORE the `ring_push` of the same readings.  For k in order and every horizon
    h < t_out the forecast of origin `clock[0] + k - h` counts if `issued` carries its stamp; its truth is `raw[k, 0]`,
    valid unless NaN or equal to `null_value`.  Adds to `sums` (float64 [t_out + 1, W], W = `score_columns(Q)`: per horizon
    and over all, {count, |e|, 100 |e / y| (y > mask_value), e^2, e} and for `levels` the crossing count, width sum, hit
    counts and pinball sums of `quantile_metrics`) and to `node_sums` (float64 [N, 3]: count, |e|, e per node), both
    zeroed by the caller (`msgat_forecast_score`: two launches, a fixed summation order, nothing read back).

    `levels`: None for a point head (out = t_out) or the Q quantile levels of a head with out = Q * t_out, `point` the
    level that serves as the point forecast (default: nearest 0.5).  `partials`: a caller-owned float64 buffer of
    `msgat_forecast_score_partial_doubles(N, t_out, Q)` elements (a captured step keeps one).  No autograd: data."""
    what = "forecast_score"
    levels = () if levels is None else quantile_levels(levels)
    n_levels, t_out = len(levels), int(t_out)
    if raw.dim() != 3 or raw.shape[0] < 1:
        raise ValueError(f"{what}: raw {tuple(raw.shape)} must be [K >= 1, C, N]")
    if t_out < 1 or max(n_levels, 1) * t_out > 64:
        raise ValueError(f"{what}: t_out = {t_out} with {n_levels} levels: between 1 and 64 outputs per node")
    cols = score_columns(n_levels)
    if book.dim() == 3 and raw.shape[2] != book.shape[1]:
        raise ValueError(f"{what}: raw {tuple(raw.shape)} and book {tuple(book.shape)} must agree in N")
    P, N, out = _check_book(what, book, issued, clock, [
        ("raw", raw, torch.float32, None), ("sums", sums, torch.float64, (t_out + 1, cols)),
        ("node_sums", node_sums, torch.float64, (book.shape[1] if book.dim() == 3 else 0, SCORE_NODE_COLUMNS))])
    if out != max(n_levels, 1) * t_out:
        raise ValueError(f"{what}: a head of {max(n_levels, 1)} x {t_out} outputs needs book [P, N, "
                         f"{max(n_levels, 1) * t_out}], got out = {out}")
    if P < t_out:
        raise ValueError(f"{what}: the book's P = {P} rows must be at least t_out = {t_out}")
    point = (quantile_point(levels) if n_levels else 0) if point is None else int(point)
    if n_levels and not 0 <= point < n_levels:
        raise ValueError(f"{what}: point = {point} outside the {n_levels} levels")
    dev, K, C_ = book.device, raw.shape[0], raw.shape[1]
    L = _lib.checked()
    need = int(L.msgat_forecast_score_partial_doubles(N, t_out, n_levels))
    if partials is None:
        partials = torch.empty(max(need, 1), device=dev, dtype=torch.float64)
    elif partials.dtype != torch.float64 or partials.device != dev or partials.numel() < need or not partials.is_contiguous():
        raise ValueError(f"{what}: partials must be a contiguous float64 tensor of at least {need} elements on {dev}")
    host_levels = (C.c_float * n_levels)(*levels) if n_levels else None
    with torch.cuda.device(dev):
        L.msgat_forecast_score(_ptr(raw), _ptr(book), _ptr(issued), _ptr(clock), K, C_, N, t_out, n_levels,
                               host_levels, point, P, int(null_value is not None),
                               0.0 if null_value is None else float(null_value), float(mask_value), _ptr(partials),
                               _ptr(sums), _ptr(node_sums), _stream_handle(dev))


# ---- boundary hygiene for every autograd.Function above -----------------------------------------------------------
# (a) the library's launches act on the CURRENT HIP device (hipFuncSetAttribute for > 64 KB LDS, occupancy queries),
#     while the reference's API lets the caller name any device (`run_epoch(..., gpu_id=k)`, engine.py:40,50):
#     make the tensors' device current for the duration of the call;
# (b) the reference runs the forward under CUDA AMP (engine.py:54): inside an autocast region these ops receive
#     half-precision outputs of neighbouring matmuls -- cast them back to fp32 (the parity type) and switch
#     autocast off inside, as torch.amp.custom_fwd(cast_inputs=torch.float32) does.
def _guard(fn, is_forward: bool):
    import functools

    @functools.wraps(fn)
    def wrapped(ctx, *args):
        dev = next((a.device for a in args if torch.is_tensor(a) and a.is_cuda), None)
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(ctx, *args)
        with torch.cuda.device(dev):
            return fn(ctx, *args)

    # Outside an autocast region -- every call of this package's own engine, and the autograd thread unless the caller
    # ran backward inside one -- torch.amp.custom_fwd is a no-op and custom_bwd an `autocast(enabled=False)` context
    # around a region that has autocast off already: ~5 us of host time per backward call for nothing (a sixth of a
    # GACN module call's host time, tools/host_overhead.py --dropin).  Both keep their exact semantics inside a region.
    if is_forward:
        in_region = torch.amp.custom_fwd(wrapped, device_type="cuda", cast_inputs=torch.float32)

        @functools.wraps(fn)
        def forward(ctx, *args):
            if torch.is_autocast_enabled("cuda"):
                return in_region(ctx, *args)
            return wrapped(ctx, *args)
        return forward

    @functools.wraps(fn)
    def backward(ctx, *args):
        if torch.is_autocast_enabled("cuda"):
            with torch.autocast(device_type="cuda", enabled=False):
                return wrapped(ctx, *args)
        return wrapped(ctx, *args)
    return backward


# (c) every backward here launches library kernels on raw pointers: it cannot be differentiated a second time.
#     `once_differentiable` says so to autograd -- `backward(create_graph=True)` / a grad-of-grad then fails AT this node
#     with PyTorch's own message ("trying to differentiate twice a function that was marked with @once_differentiable")
#     instead of silently returning gradients that are constants of the outer graph.
from torch.autograd.function import once_differentiable  # noqa: E402


def _once(fn):
    """`once_differentiable`, entered only when it has something to do: in an ordinary backward grad mode is off already and
    the decorator's `no_grad` context is ~2 us of host time per call for nothing (28 calls per training step)."""
    import functools
    guarded = once_differentiable(fn)

    @functools.wraps(fn)
    def backward(ctx, *args):
        if torch.is_grad_enabled():      # backward(create_graph=True): hand the gradients over behind an error node
            return guarded(ctx, *args)
        return fn(ctx, *args)
    return backward


for _name, _cls in list(globals().items()):
    if isinstance(_cls, type) and issubclass(_cls, torch.autograd.Function) and _cls is not torch.autograd.Function:
        _cls.forward = staticmethod(_guard(_cls.forward, True))
        _cls.backward = staticmethod(_once(_guard(_cls.backward, False)))
