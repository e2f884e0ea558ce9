"""Sensor-graph adjacency: the sym-normalised dense matrix the reference uses and the
CSR/CSC form the HIP kernels walk; `BatchedGraph` is a per-sample adjacency [V,N,N] on one shared structure, `SparseSets`
the same for a sparse [V,N,N] tensor (a weight per stored edge and per sample).

Reference: /root/reference/src/data_loader.py:49-66 builds `D^-1/2 (A + I) D^-1/2` from a
csv edge list; src/models/msgat.py:190 keeps it as a frozen parameter `adj`;
src/models/attention.py:36 applies it as a dense mask.  Only its non-zeros matter to that
product, so `SparseGraph` holds them (built by the native host routine
`msgat_graph_build`, include/msgat_hip.h).
"""
from __future__ import annotations

import collections
import ctypes as C
import weakref
from typing import Iterable, Tuple

import numpy as np
import torch

from . import _lib


def sym_norm_adjacency(n_nodes: int, edges: Iterable[Tuple[int, int]]) -> torch.Tensor:
    """`D^-1/2 (A + I) D^-1/2` as a dense fp32 [N,N] tensor (data_loader.py:59-66).

    `edges` are undirected (src, dst) pairs; duplicates and self pairs collapse to a
    single unit entry, as the assignment `A[s, d] = A[d, s] = 1` does in the reference.
    """
    a = torch.eye(n_nodes, dtype=torch.float32)
    e = torch.as_tensor(np.asarray(list(edges), dtype=np.int64).reshape(-1, 2))
    if e.numel():
        a[e[:, 0], e[:, 1]] = 1.0
        a[e[:, 1], e[:, 0]] = 1.0
    d = a.sum(dim=1).rsqrt()
    return d[:, None] * a * d[None, :]


def random_edges(n_nodes: int, n_edges: int, seed: int = 0) -> np.ndarray:
    """`n_edges` distinct undirected non-self edges, uniform over node pairs."""
    max_edges = n_nodes * (n_nodes - 1) // 2
    if n_edges > max_edges:
        raise ValueError(f"{n_edges} edges requested, a simple graph on {n_nodes} nodes has {max_edges}")
    rng = np.random.default_rng(seed)
    seen, out = set(), []
    while len(out) < n_edges:
        s, d = (int(v) for v in rng.integers(0, n_nodes, size=2))
        if s == d:
            continue
        key = (s, d) if s < d else (d, s)
        if key in seen:
            continue
        seen.add(key)
        out.append((s, d))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def synthetic_adjacency(n_nodes: int, n_edges: int, seed: int = 0) -> torch.Tensor:
    """PEMS-like synthetic sensor graph (no PEMS files ship with the reference)."""
    return sym_norm_adjacency(n_nodes, random_edges(n_nodes, n_edges, seed))


# one float4 per node must fit LDS for the SELL kernels (csrc/common.hpp: kLdsMax - 1024); below _SELL_AUTO_MIN
# nodes a whole [N,T] slab fits LDS for every supported T, so the layout would never be used
_SELL_MAX_NODES = (160 * 1024 - 1024) // 16
_SELL_AUTO_MIN = 2048


class SparseGraph:
    """CSR + CSC of a dense adjacency, host arrays plus (lazily) device copies.

    `sell`: "auto" also builds the degree-sorted sliced-ELLPACK layouts (include/msgat_hip.h, msgat_sell_t) for
    graphs large enough that an [N,T] slab may not fit LDS; "always" builds them and makes the library prefer the
    SELL kernels (tests exercise them on small graphs this way); "never" omits them."""

    def __init__(self, adjacency: torch.Tensor, sell: str = "auto"):
        if adjacency.dim() > 2:
            # the reference documents `adjacency: [..., n_nodes, n_nodes]` (attention.py:22: `att * adjacency`
            # broadcasts, attention.py:36); its only caller passes ONE [N,N] matrix (msgat.py:127, :190), and so does
            # everything here: the CSR / CSC / SELL structures are built per graph, not per sample
            raise ValueError(
                f"adjacency must be one [n_nodes, n_nodes] matrix, got {tuple(adjacency.shape)}: the batched form "
                "`[..., n_nodes, n_nodes]` that the reference's attention.py:22 documents is not supported by "
                "SparseGraph -- a [B, n_nodes, n_nodes] adjacency goes through BatchedGraph / batched_graph_of "
                "(the ops and modules accept it directly)")
        if adjacency.dim() != 2 or adjacency.size(0) != adjacency.size(1):
            raise ValueError(f"adjacency must be [N,N], got {tuple(adjacency.shape)}")
        a = adjacency.detach().to(device="cpu", dtype=torch.float32).contiguous()
        n = a.size(0)
        L = _lib.checked()
        nnz = C.c_int32(0)
        L.msgat_graph_count(a.data_ptr(), n, n, C.byref(nnz))
        self._alloc(n, int(nnz.value))
        L.msgat_graph_build(a.data_ptr(), n, n, self.nnz, *self._ptrs(self._FIELDS))
        self._finish(sell)

    @classmethod
    def from_indices(cls, rowptr: torch.Tensor, col: torch.Tensor, n_nodes: int, sell: str = "auto") -> "SparseGraph":
        """The structure of a sparse [N,N] adjacency from its CSR index arrays (`msgat_graph_build_indices`): every stored
        index is an edge, an explicit 0 included, columns in any order inside a row, and [N,N] is never formed.  `val`
        is left at 0 (the caller's values are pointed at on the device); `order` [nnz] maps the library's edge k to
        its input position."""
        self = cls.__new__(cls)
        rp = rowptr.detach().to(device="cpu", dtype=torch.int32).contiguous()
        ci = col.detach().to(device="cpu", dtype=torch.int32).contiguous()
        n = int(n_nodes)
        if rp.dim() != 1 or rp.numel() != n + 1 or ci.dim() != 1:
            raise ValueError(f"rowptr must be [{n + 1}] and col 1-D, got {tuple(rp.shape)} and {tuple(ci.shape)}")
        self._alloc(n, int(ci.numel()))
        self.order = torch.zeros(max(self.nnz, 1), dtype=torch.int32)
        _lib.checked().msgat_graph_build_indices(
            rp.data_ptr(), ci.data_ptr(), n, self.nnz,
            *self._ptrs(("rowptr", "col", "erow", "colptr", "crow", "cperm", "cpos", "order")))
        self._finish(sell)
        return self

    def _alloc(self, n: int, nnz: int) -> None:
        """Zeroed host arrays for `nnz` edges on `n` nodes (one entry at least per edge array)."""
        self.n_nodes, self.nnz = n, nnz
        for name in self._FIELDS:
            size = n + 1 if name in ("rowptr", "colptr") else max(nnz, 1)
            setattr(self, name, torch.zeros(size, dtype=torch.float32 if name == "val" else torch.int32))

    def _ptrs(self, names):
        return [getattr(self, name).data_ptr() for name in names]

    def _finish(self, sell: str) -> None:
        self._dev = {}
        if sell not in ("auto", "always", "never"):
            raise ValueError(f"sell must be 'auto', 'always' or 'never', got {sell!r}")
        self.sell_prefer = sell == "always"
        self._sell = {}
        n = self.n_nodes
        if sell != "never" and self.nnz > 0 and n <= _SELL_MAX_NODES and (self.sell_prefer or n >= _SELL_AUTO_MIN):
            self._sell["sell_rows"] = self._build_sell(self.rowptr, self.col, None, with_pos=True)
            self._sell["sell_cols"] = self._build_sell(self.colptr, self.crow, self.cperm, with_pos=False)

    _FIELDS = ("rowptr", "col", "val", "erow", "colptr", "crow", "cperm", "cpos")
    _SELL_FIELDS = ("slice_off", "lane_row", "idx", "src", "pos")

    def _build_sell(self, ptr, idx, perm, with_pos: bool):
        L = _lib.checked()
        ns, npos, pair = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        L.msgat_graph_sell_count(ptr.data_ptr(), self.n_nodes, C.byref(ns), C.byref(npos), C.byref(pair))
        ns, npos = int(ns.value), int(npos.value)
        t = dict(slice_off=torch.zeros(ns + 1, dtype=torch.int32), lane_row=torch.zeros(64 * ns, dtype=torch.int32),
                 idx=torch.zeros(npos + _lib.SELL_SLACK, dtype=torch.int16), src=torch.zeros(max(npos, 1), dtype=torch.int32))
        if with_pos:
            t["pos"] = torch.zeros(self.nnz, dtype=torch.int32)
        L.msgat_graph_sell_build(ptr.data_ptr(), idx.data_ptr(), None if perm is None else perm.data_ptr(),
                                 self.n_nodes, self.nnz, ns, npos, t["slice_off"].data_ptr(),
                                 t["lane_row"].data_ptr(), t["idx"].data_ptr(), t["src"].data_ptr(),
                                 t["pos"].data_ptr() if with_pos else None)
        t["n_slices"], t["n_pos"], t["pair_trips"] = ns, npos, int(pair.value)
        return t

    @property
    def has_sell(self) -> bool:
        return bool(self._sell)

    def _struct(self, tensors) -> _lib.Graph:
        g = _lib.Graph()
        g.n_nodes, g.nnz = self.n_nodes, self.nnz
        for name in self._FIELDS:
            setattr(g, name, tensors[name].data_ptr())
        for form, host in self._sell.items():
            j = getattr(g, form)
            j.n_slices, j.n_pos, j.prefer = host["n_slices"], host["n_pos"], int(self.sell_prefer)
            j.pair_trips = host["pair_trips"]
            for name in self._SELL_FIELDS:
                if name in host:
                    setattr(j, name, tensors[f"{form}.{name}"].data_ptr())
        return g

    def _host_tensors(self):
        t = {k: getattr(self, k) for k in self._FIELDS}
        for form, host in self._sell.items():
            for name in self._SELL_FIELDS:
                if name in host:
                    t[f"{form}.{name}"] = host[name]
        return t

    def host_struct(self) -> _lib.Graph:
        return self._struct(self._host_tensors())

    def validate(self) -> None:
        hs = self.host_struct()
        _lib.checked().msgat_graph_validate(C.byref(hs))

    def on(self, device: torch.device):
        """(ctypes struct of device pointers, tensors kept alive) for `device`."""
        key = str(device)
        if key not in self._dev:
            tensors = {k: v.to(device) for k, v in self._host_tensors().items()}
            self._dev[key] = (self._struct(tensors), tensors)
        return self._dev[key]

    def dense(self) -> torch.Tensor:
        return _dense(self, self.val)


def _dense(structure: SparseGraph, val: torch.Tensor) -> torch.Tensor:
    """[..., N, N] (host) of the values val [..., >= nnz] on the edges of `structure`."""
    n, nnz = structure.n_nodes, structure.nnz
    a = torch.zeros(tuple(val.shape[:-1]) + (n, n))
    if nnz:
        a[..., structure.erow[:nnz].long(), structure.col[:nnz].long()] = val[..., :nnz].cpu()
    return a


class ValuedGraph:
    """Values on a shared structure: what the ops hand the library for a per-sample adjacency (`BatchedGraph`) and for a
    sparse one.  `structure` is a `SparseGraph` shared by every graph with its pattern; `val` holds this graph's values
    in the structure's edge order, a tensor [n_sets, nnz] or the address of values on the device (a sparse adjacency's
    own, read where they are); group g of a call reads value set g % n_sets.

    Exposes what the ops use of a `SparseGraph` (`n_nodes`, `nnz`, `has_sell`, `on(device)`, a `__dict__` for the
    per-shape plans) plus `n_sets`; `on()` hands the library the structure's device arrays with `val` pointing at this
    graph's values and `val_sets = n_sets`."""

    def __init__(self, structure: SparseGraph, val, n_sets: int):
        self.structure, self.val, self.n_sets = structure, val, n_sets
        self.n_nodes, self.nnz = structure.n_nodes, structure.nnz
        self._dev = {}

    @property
    def has_sell(self) -> bool:
        return self.structure.has_sell

    def on(self, device: torch.device):
        """(ctypes struct of device pointers, what it keeps alive) for `device`: the shared structure, this graph's
        values."""
        key = str(device)
        if key not in self._dev:
            _, tensors = self.structure.on(device)
            val = self.val
            if isinstance(val, torch.Tensor) and val.device != torch.device(device):
                val = val.to(device)
            g = self.structure._struct(tensors)
            g.val, g.val_sets = val if isinstance(val, int) else val.data_ptr(), self.n_sets
            self._dev[key] = (g, (tensors, val))
        return self._dev[key]

    def dense(self) -> torch.Tensor:
        """[n_sets,N,N] of the values on the structure (host; `val` a tensor)."""
        return _dense(self.structure, self.val)


# ---- caches ----------------------------------------------------------------------------------------------------------

class _Lru(collections.OrderedDict):
    """A table that keeps the `bound` entries used last."""

    def __init__(self, bound: int):
        super().__init__()
        self.bound = bound

    def hit(self, key):
        value = self.get(key)
        if value is not None:
            self.move_to_end(key)
        return value

    def put(self, key, value):
        self[key] = value
        self.move_to_end(key)
        while len(self) > self.bound:
            self.popitem(last=False)
        return value


def _tensor_key(t: torch.Tensor) -> tuple:
    return (t.data_ptr(), tuple(t.shape), str(t.device), t._version)


class _TensorCache(_Lru):
    """An LRU keyed on tensors' `_tensor_key` (storage address, shape, device, version).  Another tensor object can have
    the key of an entry -- a view, or a new tensor the allocator placed at a recycled address -- so each entry holds the
    object it was made for by weakref, and `lookup` tells a hit on that very object apart."""

    def lookup(self, key, obj):
        """(the value cached under `key` or None, whether it was cached for `obj` itself)."""
        entry = self.hit(key)
        if entry is None:
            return None, False
        return entry[0], entry[1]() is obj

    def remember(self, key, obj, value):
        self.put(key, (value, weakref.ref(obj)))
        return value


_CACHE_MAX = 16
_GRAPHS = _TensorCache(_CACHE_MAX)     # frozen dense [N,N] / [1,N,N] -> (SparseGraph, a copy of the contents)
_BATCHED = _TensorCache(_CACHE_MAX)    # frozen dense [V,N,N], sell -> BatchedGraph
_LEARNED = _Lru(_CACHE_MAX)            # a dense adjacency that requires grad: address, shape, strides, device, sell -> BatchedGraph
_SPARSE = _TensorCache(_CACHE_MAX)     # index tensors of a sparse adjacency, layout, N, sell -> (SparsePattern | SparseSets, indices)
_PATTERNS = _Lru(8)                    # CSR content (N, sell, rowptr, col) -> SparsePattern


def _capturing(t: torch.Tensor) -> bool:
    return t.is_cuda and torch.cuda.is_current_stream_capturing()


def _not_cached(what: str) -> _lib.MsgatError:
    # a first build reads the adjacency (or its indices) back to the host, which a stream capture cannot contain
    return _lib.MsgatError(f"{what}: run one forward outside the HIP-graph capture first (engine.Trainer does this in "
                           "its warm-up)")


def _learned_graph_of(adjacency: torch.Tensor, sets: torch.Tensor, sell: str) -> "BatchedGraph":
    """The graph of a dense adjacency that requires grad; `sets` is `adjacency.detach()` as [V,N,N].

    Whoever trains a tensor writes it, and most writers leave no trace: `FlatAdam` and its kernels (`msgat_adam_step` and
    its guarded and averaged forms, `msgat_param_swap`) write through the address, a replay of a captured step runs no
    Python, `.data` skips the version counter.  So neither identity nor version proves anything about the contents, and
    the cache keeps only what a write cannot change cheaply -- the pattern: a `BatchedGraph` (one value set for [N,N]
    and [1,N,N]) keyed on (storage address, shape, strides, device, sell) and good while the tensor it was made for
    lives (a weakref), whose values are refilled from the tensor on
    EVERY call by `msgat_graph_edge_values` (one launch that reads the V N^2 floats and writes V nnz).  The launch
    counts the non-zeros outside the pattern.  Eagerly the two counters are read back (8 bytes) and a non-zero eager
    count rebuilds the pattern from the tensor (N^2 mask bytes to the host; one optimizer step on a learned graph makes
    every entry an edge).  Inside a HIP-graph capture nothing is read back and the pattern cannot grow: the count
    accumulates at every replay, and if a replay dropped edges the next eager call on the tensor raises `MsgatError`
    -- or `check_captured_patterns()`, which `engine.Trainer` calls at the end of every epoch, where no eager call may
    come; what was reported is cleared.  A graph that a captured step refills is pinned (`_CAPTURED`) while its tensor
    lives: the step holds its addresses, so the LRU must not free it."""
    key = (adjacency.data_ptr(), tuple(adjacency.shape), tuple(adjacency.stride()), str(adjacency.device), sell)
    g = _LEARNED.hit(key)
    capturing = _capturing(adjacency)
    if g is not None and g.owner() is None:
        # the tensor this entry was made for is gone: the allocator recycled its address, or the adjacency is computed
        # anew at every call.  Neither the entry's counters and captured steps nor its pattern (a superset would do, but
        # a full one would make a sparse graph pay for N^2 edges from then on) are this tensor's: built anew
        g = None
    if g is None:
        if capturing:
            raise _not_cached("the pattern of this learned adjacency is not known yet")
        g = BatchedGraph(sets, sell)
        g.owner, g.sell = weakref.ref(adjacency), sell
        return _LEARNED.put(key, g)
    # (another live object at this address is a view of the owner's memory: the same contents, refilled all the same)
    g.update_(sets)
    if capturing:
        if not g.in_capture:
            g.in_capture = True
            _CAPTURED.append(g)      # the captured step holds its addresses: it outlives the LRU
        return g
    captured, eager = g.outside_counts()
    # a graph that a captured step refills and that the tensor outgrew eagerly: the step keeps its addresses and its
    # pattern, so it stays alive behind its successor and its replays stay checked (one more read-back each, only then)
    _refuse_dropped(g, captured)
    if eager:
        new = BatchedGraph(sets, sell)
        new.owner, new.sell = g.owner, sell
        new.retired = g.retired + [g] if g.in_capture else g.retired
        g = _LEARNED.put(key, new)
    return g


_CAPTURED = []     # the learned graphs that captured steps refill, while their tensors live (pruned by check_captured_patterns)


def _refuse_dropped(g: "BatchedGraph", captured: int) -> None:
    """Raise if replays of captured steps dropped entries of the learned adjacency behind `g` (`captured`: the count of
    `g` itself, already read; its retired predecessors are read here).  What is reported is cleared: the error comes
    back only if a step captured on an outgrown pattern is replayed again."""
    stale = [old for old in g.retired if old.outside_counts()[0]]
    if not captured and not stale:
        return
    total = captured + sum(old.outside_counts()[0] for old in stale)
    for each in stale + ([g] if captured else []):
        each._outside[0] = 0
    owner = g.owner()
    raise _lib.MsgatError(
        f"the pattern of the learned dense adjacency{'' if owner is None else ' ' + str(tuple(owner.shape))} grew under a "
        f"captured step: replays found {total} non-zero entries outside the pattern the step was captured with and "
        "dropped them (a captured step cannot rebuild the pattern; the results of those replays are wrong).  Capture the "
        "step again after the pattern has grown -- one eager optimizer step fills every zero of a dense learned "
        "adjacency; engine.Trainer does both by itself -- or start from values without a zero entry, or keep the pattern "
        "fixed with ops.edge_adjacency")


def _owned(g: "BatchedGraph", tensors) -> bool:
    owner = g.owner()
    return owner is not None and (tensors is None or any(owner is t for t in tensors))


def check_captured_patterns(tensors=None) -> None:
    """Raise `MsgatError` if a replay of a captured step dropped entries of a learned dense adjacency (one of `tensors`;
    None: any): 8 bytes read back per learned graph that a captured step refills.  `engine.Trainer` calls it at the
    end of `run_epoch` for the model's parameters, where no eager call on the tensor may ever come."""
    _CAPTURED[:] = [g for g in _CAPTURED if g.owner() is not None]       # a dead tensor's capture cannot be replayed
    for g in _CAPTURED:
        if _owned(g, tensors):
            _refuse_dropped(g, g.outside_counts()[0])


def learned_patterns_grew(tensors=None) -> bool:
    """After an eager write (an optimizer step outside the captured step): whether a learned dense adjacency (one of
    `tensors`; None: any) that a captured step refills has outgrown the pattern the step was captured with.  The pattern
    is rebuilt here, and the caller must drop its captured steps: they hold the old one.  A pattern that is full
    cannot grow and costs nothing; any other costs the launch and the 8-byte read-back of an eager call."""
    grew = False
    for g in list(_LEARNED.values()):
        n = g.n_nodes
        if g.in_capture and g.nnz < n * n and _owned(g, tensors):
            t = g.owner()
            now = batched_graph_of(t, g.sell) if t.dim() == 3 and t.shape[0] != 1 else graph_of(t)
            grew = grew or now is not g
    return grew


def graph_of(adjacency: torch.Tensor) -> "SparseGraph | BatchedGraph":
    """Cached graph of a dense adjacency tensor [N,N] (or [1,N,N], its one matrix).

    A tensor that requires grad is somebody's to train: its values are re-read from the tensor on every call, whoever
    wrote them and however (`_learned_graph_of`; the graph is then a one-set `BatchedGraph`, which runs the same
    kernels).

    A frozen tensor (msgat.py:190) gets a `SparseGraph`: one CSR build per tensor version.  Keyed on (storage address,
    shape, device, version).  A hit on the very same tensor object is free; a hit through a different object (a view,
    or a new tensor the allocator placed at a recycled address) is confirmed by comparing contents before it is trusted.
    What a frozen tensor promises: every write that moves its version counter (an in-place torch op, directly or
    through a view) is seen; a write that does not (`.data`, a kernel or a NumPy alias that writes through the address)
    is NOT seen while the same object is passed again -- the price of a free hit.  Who writes a frozen adjacency that way
    passes `adjacency.detach()` (a new object: compared by content), bumps the version (`adjacency.add_(0)`), or lets
    the tensor require grad.
    """
    if adjacency.requires_grad and adjacency.dim() in (2, 3) and adjacency.shape[-1] == adjacency.shape[-2] \
            and (adjacency.dim() == 2 or adjacency.shape[0] == 1):
        n = adjacency.shape[-1]
        return _learned_graph_of(adjacency, adjacency.detach().reshape(1, n, n), "auto")
    key = _tensor_key(adjacency)
    hit, same = _GRAPHS.lookup(key, adjacency)
    if same:
        return hit[0]
    capturing = _capturing(adjacency)
    # another tensor object at a cached address: compare contents ONCE (a device read-back, which a HIP-graph capture
    # cannot contain) and remember the new object, so that its later calls -- the captured one included -- hit by
    # identity.  (A model built where a freed model's adjacency lived used to compare on every call, and its first
    # capture failed with "operation not permitted when stream is capturing".)
    if hit is not None and not capturing and torch.equal(hit[1], adjacency.detach()):
        return _GRAPHS.remember(key, adjacency, hit)[0]
    if capturing:
        raise _not_cached("the CSR of this adjacency is not cached yet")
    g = SparseGraph(adjacency[0] if adjacency.dim() == 3 and adjacency.shape[0] == 1 else adjacency)
    return _GRAPHS.remember(key, adjacency, (g, adjacency.detach().clone()))[0]


# ---- per-sample adjacency [V,N,N] ------------------------------------------------------------------------------------
# The reference's `softmax(k Wg q^T) * adjacency` (attention.py:36) broadcasts over the batch, so [B,N,N] gives every
# sample its own graph.  The kernels read adjacency values in one place only (the edge tail of the score kernels), so a
# batched adjacency is ONE structure -- the union of the samples' patterns, shared by every object with that pattern --
# and one value set per sample, val [V,nnz], with explicit zeros where a sample lacks a union edge (E = 0 there).

def _row_pointers(rows: torch.Tensor, n: int) -> torch.Tensor:
    """CSR row pointers [n+1] of the row indices of edges in row-major order."""
    crow = torch.zeros(n + 1, dtype=torch.int64)
    crow[1:] = torch.bincount(rows, minlength=n).cumsum(0)
    return crow


def _check_batched(adjacency: torch.Tensor):
    if adjacency.dim() != 3 or adjacency.shape[1] != adjacency.shape[2] or adjacency.shape[0] < 1:
        raise ValueError(f"a batched adjacency must be [V, N, N], got {tuple(adjacency.shape)}")


class BatchedGraph(ValuedGraph):
    """A per-sample adjacency [V,N,N]: one shared sparse structure (the union of the samples' non-zero patterns, the
    `SparseGraph` of the [N,N] mask `(adj != 0).any(0)`) and this object's own values val [V,nnz], n_sets = V.  Group g
    of a call reads value set g % V: V = B for a [B,...] batch (shared by R stacked relations), V = R*B for one set per
    group.

    `update_(adj)` refills the values in place from a device tensor with the `msgat_graph_edge_values` kernel, which also
    adds the non-zeros it finds outside the structure to a device counter; nothing is read back, so it may sit inside a
    HIP-graph capture.  `check()` reads the counter and raises if any sample had an edge the structure lacks (those edges
    would be silently dropped).  A CPU tensor is gathered on the host by indexing (no GPU needed).  There are two
    counters, one for refreshes enqueued inside a HIP-graph capture (every replay adds to it) and one for eager ones:
    `outside_counts()` reads both in one read-back, `outside()` is their sum."""

    def __init__(self, adjacency: torch.Tensor, sell: str = "auto", structure: SparseGraph = None):
        _check_batched(adjacency)
        V, N = int(adjacency.shape[0]), int(adjacency.shape[1])
        if structure is None:            # the shared CSR / CSC (/ SELL) of the union mask
            rows, cols = (adjacency.detach() != 0).any(0).cpu().nonzero(as_tuple=True)
            structure = _pattern(_row_pointers(rows, N), cols, N, sell).structure
        elif structure.n_nodes != N:
            raise ValueError(f"structure has {structure.n_nodes} nodes, the adjacency {N}")
        self.device = adjacency.device
        super().__init__(structure, torch.zeros((V, max(structure.nnz, 1)), dtype=torch.float32, device=self.device), V)
        self._outside = torch.zeros(2, dtype=torch.int32, device=self.device)   # [inside a capture, eager]
        self.in_capture = False          # a captured step refills this graph (`_learned_graph_of`) ...
        self.retired = []                # ... and these, its predecessors, which the tensor has outgrown
        self.owner = lambda: None        # weakref to the learned tensor this graph is cached for
        self.sell = sell
        self.update_(adjacency)

    def update_(self, adjacency: torch.Tensor) -> "BatchedGraph":
        """Refill the values from `adjacency` [V,N,N] (same V, N and device); non-zeros outside the structure are added
        to the counter that `check()` reads."""
        _check_batched(adjacency)
        if tuple(adjacency.shape) != (self.n_sets, self.n_nodes, self.n_nodes):
            raise ValueError(f"adjacency {tuple(adjacency.shape)} does not match this graph's "
                             f"[{self.n_sets}, {self.n_nodes}, {self.n_nodes}]")
        if adjacency.device != self.device:
            raise ValueError(f"adjacency is on {adjacency.device}, this graph's values on {self.device}")
        a = adjacency.detach()
        if a.dtype != torch.float32:
            a = a.float()
        if not a.is_contiguous():        # an expanded [N,N] too: the kernel streams contiguous rows
            a = a.contiguous()
        s = self.structure
        if not a.is_cuda:
            if self.nnz:
                self.val[:, : self.nnz] = a[:, s.erow[: self.nnz].long(), s.col[: self.nnz].long()]
            inside = int((self.val[:, : self.nnz] != 0).sum())
            self._outside[0 if _capturing(a) else 1] += int((a != 0).sum()) - inside
            return self
        gstruct, _ = s.on(a.device)
        counter = self._outside.data_ptr() + (0 if _capturing(a) else 4)
        _lib.checked().msgat_graph_edge_values(C.byref(gstruct), a.data_ptr(), self.n_sets, self.val.data_ptr(),
                                               counter, _lib.stream_handle(a.device))
        return self

    def outside_counts(self) -> Tuple[int, int]:
        """Non-zeros found outside the structure by every refresh so far: (by those enqueued inside a HIP-graph capture,
        once per replay; by the eager ones).  One read-back of 8 bytes."""
        captured, eager = self._outside.tolist()
        return int(captured), int(eager)

    def outside(self) -> int:
        """Non-zeros found outside the structure by every refresh so far (a read-back)."""
        return sum(self.outside_counts())

    def check(self) -> "BatchedGraph":
        n = self.outside()
        if n:
            raise _lib.MsgatError(f"{n} non-zero adjacency entries lie outside this BatchedGraph's pattern: build a "
                                  "new one for this adjacency (batched_graph_of does so)")
        return self


def batched_graph_of(adjacency: torch.Tensor, sell: str = "auto") -> BatchedGraph:
    """Cached `BatchedGraph` of a dense [V,N,N] adjacency, keyed on (storage address, shape, device, version).

    A hit on the very same tensor object is free, except under a HIP-graph capture, where it enqueues the refresh: a
    captured static input keeps its identity while its contents change at every replay.  A miss reuses the pattern used
    last for this N when there is one: the values are filled by the kernel and the 4-byte outside count is read back;
    a non-zero count rebuilds the union pattern (N^2 mask bytes to the host) and fills again.  Under capture nothing is
    read back: the known pattern is used and the count only accumulates (`check()` reads it later); with no known
    pattern it raises, as graph_of does.

    All of that is the frozen tensor's path, with graph_of's promise: a write that moves the version counter is seen, one
    that does not (`.data`, a kernel or an alias writing through the address) is not while the same object is passed
    eagerly again.  A tensor that requires grad has its values refilled from the tensor on every call, eager or captured,
    and its pattern rebuilt when they outgrow it (`_learned_graph_of`)."""
    _check_batched(adjacency)
    if adjacency.requires_grad:
        return _learned_graph_of(adjacency, adjacency.detach(), sell)
    capturing = _capturing(adjacency)
    key = _tensor_key(adjacency) + (sell,)
    hit, same = _BATCHED.lookup(key, adjacency)
    if same:
        return hit.update_(adjacency) if capturing else hit
    if hit is not None:
        known = hit.structure
    else:                                # the pattern on N nodes used last: the latest entry of _PATTERNS with (N, sell)
        n_sell = (int(adjacency.shape[1]), sell)
        known = next((p.structure for key, p in reversed(_PATTERNS.items()) if key[:2] == n_sell), None)
    if not adjacency.is_cuda:
        g = BatchedGraph(adjacency, sell)
    elif known is not None:
        g = BatchedGraph(adjacency, sell, structure=known)
        if not capturing and g.outside() != 0:
            g = BatchedGraph(adjacency, sell)
    elif capturing:
        raise _not_cached("the pattern of this batched adjacency is not known yet")
    else:
        g = BatchedGraph(adjacency, sell)
    return _BATCHED.remember(key, adjacency, g)


# ---- a sparse adjacency [N,N] (torch COO / CSR): a learned weight per stored edge --------------------------------------
# The pattern is the set of stored indices; the values stay on the device and the library reads them where they are
# (msgat_graph_t.val, val_sets = 1): the edge tail of the score kernels is their only reader.  The structure is built once
# per pattern -- keyed on the index tensors' storage (kept alive by the cache, so an address is never reused under it) and
# version, confirmed by content on first sight -- and after that a call reads nothing back and may be captured.

def is_sparse_adjacency(adjacency) -> bool:
    return isinstance(adjacency, torch.Tensor) and adjacency.layout in (torch.sparse_coo, torch.sparse_csr)


class SparsePattern:
    """The structure of one sparse pattern (`SparseGraph.from_indices`) plus, when the caller's order inside a row is
    not the library's, the device permutations between them (computed once): values are gathered into a buffer of
    this pattern's, and the gradient is gathered back."""

    def __init__(self, crow: torch.Tensor, col: torch.Tensor, n_nodes: int, sell: str = "auto"):
        self.structure = SparseGraph.from_indices(crow, col, n_nodes, sell=sell)
        nnz = self.structure.nnz
        order = self.structure.order[:nnz].long()
        self.identity = bool(torch.equal(order, torch.arange(nnz)))
        self._order = order
        self._inverse = torch.empty_like(order)
        self._inverse[order] = torch.arange(nnz)
        self._dev = {}
        self._views = _Lru(8)     # (values address, device) -> ValuedGraph: its per-shape plans live on it

    def _perm(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (self._order.to(device), self._inverse.to(device),
                              torch.empty(max(self.structure.nnz, 1), dtype=torch.float32, device=device))
        return self._dev[key]

    def graph(self, values: torch.Tensor) -> ValuedGraph:
        """The graph whose `val` holds `values` (input order, on the device) in library order.  Values in another order,
        or not contiguous (a strided view), are copied into this pattern's own buffer: the library keeps only a pointer,
        so it must point at memory that outlives the call (a temporary copy would be freed before the score kernels
        read it) and that a captured step re-reads at every replay."""
        if not self.identity or not values.is_contiguous():
            order, _, buf = self._perm(values.device)
            dst = buf[: self.structure.nnz]
            if self.identity:
                dst.copy_(values)
            else:
                torch.index_select(values, 0, order, out=dst)
            values = buf
        key = (values.data_ptr(), str(values.device))
        g = self._views.hit(key)
        return g if g is not None else self._views.put(key, ValuedGraph(self.structure, values.data_ptr(), 1))

    def to_input_order(self, dval: torch.Tensor) -> torch.Tensor:
        """A gradient in library order -> the caller's order of the values."""
        if self.identity:
            return dval
        return dval.index_select(0, self._perm(dval.device)[1])


def _pattern(crow: torch.Tensor, col: torch.Tensor, n: int, sell: str) -> SparsePattern:
    """The `SparsePattern` of host CSR indices (int64), shared by every caller with the same content."""
    key = (n, sell, crow.numpy().tobytes(), col.numpy().tobytes())
    pattern = _PATTERNS.hit(key)
    return pattern if pattern is not None else _PATTERNS.put(key, SparsePattern(crow, col, n, sell))


def sparse_parts(adjacency: torch.Tensor):
    """(layout, index tensors, values) of a sparse [N,N] adjacency; an uncoalesced COO tensor must be coalesced first."""
    if adjacency.layout == torch.sparse_csr:
        return "csr", (adjacency.crow_indices(), adjacency.col_indices()), adjacency.values()
    return "coo", (adjacency._indices(),), adjacency._values()


def check_sparse_adjacency(adjacency: torch.Tensor) -> None:
    """One [N,N] matrix, or [V,N,N] (one value set per sample or per group: `sparse_sets_of`)."""
    if adjacency.dim() not in (2, 3) or adjacency.shape[-2] != adjacency.shape[-1]:
        raise ValueError(f"a sparse adjacency must be [n_nodes, n_nodes] or [V, n_nodes, n_nodes], got "
                         f"{tuple(adjacency.shape)}")
    if adjacency.layout == torch.sparse_coo and adjacency.sparse_dim() != adjacency.dim():
        raise ValueError(f"a sparse COO adjacency {tuple(adjacency.shape)} must have {adjacency.dim()} sparse dimensions and "
                         "no dense ones (hybrid tensors are not supported)")
    if adjacency.dtype != torch.float32:
        raise TypeError(f"a sparse adjacency must be float32 (the reference arithmetic type), got {adjacency.dtype}")


def sparse_pattern_of(adjacency: torch.Tensor, sell: str = "auto") -> SparsePattern:
    """Cached `SparsePattern` of a (coalesced, if COO) sparse [N,N] adjacency, after `check_sparse_adjacency`.  A hit is
    keyed on the index tensors' storage address, shape and version; the first sight of a key reads the indices back,
    and a pattern with the same content is shared.  The first sight inside a HIP-graph capture raises, as graph_of
    does."""
    check_sparse_adjacency(adjacency)
    if adjacency.dim() != 2:
        raise ValueError(f"sparse_pattern_of takes one [n_nodes, n_nodes] matrix, got {tuple(adjacency.shape)}: a sparse "
                         "[V, n_nodes, n_nodes] adjacency goes through sparse_sets_of")
    layout, idx, _ = sparse_parts(adjacency)
    n = int(adjacency.shape[0])
    key = (layout, n, sell) + tuple(_tensor_key(t) for t in idx)
    hit, _ = _SPARSE.lookup(key, adjacency)
    if hit is not None:
        return hit[0]
    if _capturing(adjacency):
        raise _not_cached("the structure of this sparse adjacency is not cached yet")
    if layout == "csr":
        crow, col = (t.detach().to(device="cpu", dtype=torch.int64) for t in idx)
    else:
        ij = idx[0].detach().to(device="cpu", dtype=torch.int64)
        crow, col = _row_pointers(ij[0], n), ij[1]
    if crow.numel() != n + 1 or int(crow[-1]) != col.numel():
        raise ValueError("malformed sparse adjacency indices")
    # the index tensors stay alive with the entry: their addresses cannot be reused under it
    return _SPARSE.remember(key, adjacency, (_pattern(crow, col, n, sell), idx))[0]


# ---- a per-sample sparse adjacency [V,N,N]: a weight per stored edge and per sample ---------------------------------------
# torch COO with three sparse dimensions, torch batched CSR, or `ops.edge_adjacency` with weights [V,nnz] on one shared
# pattern.  The samples may store different patterns: the structure is the union of their stored indices (built from the
# indices, never from an [N,N] mask) and a flat map sends stored entry k to v_k * nnz_union + (its position in the union's
# CSR order).  Values are scattered through it into a [V,nnz_union] buffer (an edge a sample lacks stays an explicit 0,
# E = 0 there) and the [V,nnz_union] gradient is gathered back through it -- torch ops on V * nnz floats.  When the map
# is the identity (one shared pattern in the library's order) and the values are contiguous, they are read where they
# are: no copy.  Built once per index tensors and cached like `sparse_pattern_of`.

class SparseSets:
    """The union structure (`pattern`, a `SparsePattern` shared by content), the number of value sets `n_sets` and
    `flat` [entries] int64 (host), the position of every stored entry in the [n_sets, nnz_union] value buffer -- None
    when it is the identity."""

    def __init__(self, pattern: SparsePattern, n_sets: int, flat):
        self.pattern, self.structure, self.n_sets, self.flat = pattern, pattern.structure, int(n_sets), flat
        self._dev = {}
        self._views = _Lru(8)     # (values address, device) -> ValuedGraph read in place

    def _on(self, device):
        """(flat map on the device, this object's value buffer [n_sets, nnz_union] with its ValuedGraph)"""
        key = str(device)
        if key not in self._dev:
            buf = torch.zeros((self.n_sets, max(self.structure.nnz, 1)), dtype=torch.float32, device=device)
            flat = None if self.flat is None else self.flat.to(device)
            self._dev[key] = (flat, buf, ValuedGraph(self.structure, buf, self.n_sets))
        return self._dev[key]

    def graph(self, values: torch.Tensor) -> ValuedGraph:
        """The graph whose `val` holds `values` (the stored entries in input order, on their device) as [n_sets,
        nnz_union] in library order.  Read in place when they already are that, else scattered into this object's own
        buffer, which outlives the call and is re-filled at every replay of a captured step; the entries nobody stores
        were zeroed when it was made and are never written."""
        nnz = self.structure.nnz
        entries = self.n_sets * nnz if self.flat is None else self.flat.numel()
        if values.numel() != entries:    # the library is handed a bare pointer: it must cover every entry it reads
            raise ValueError(f"the sparse adjacency stores {values.numel()} values ({tuple(values.shape)}), its indices "
                             f"{entries} entries ({self.n_sets} value set(s))")
        if self.flat is None and values.is_contiguous():
            key = (values.data_ptr(), str(values.device))
            g = self._views.hit(key)
            return g if g is not None else self._views.put(key, ValuedGraph(self.structure, values.data_ptr(), self.n_sets))
        flat, buf, g = self._on(values.device)
        if nnz:
            if flat is None:
                buf[:, :nnz].copy_(values.reshape(self.n_sets, nnz))
            else:
                buf.view(-1).index_copy_(0, flat, values.reshape(-1))
        return g

    def to_input_order(self, dval: torch.Tensor) -> torch.Tensor:
        """A gradient [n_sets, nnz_union] in library order -> one per stored entry, in the caller's order (flat)."""
        if self.flat is None:
            return dval.reshape(-1)
        return dval.reshape(-1).index_select(0, self._on(dval.device)[0])


def sparse_sets_parts(adjacency: torch.Tensor):
    """(layout, index tensors, values) of a sparse [V,N,N] adjacency: "edge" for an `ops.edge_adjacency` (its one shared
    (crow, col) and the weight [V,nnz] itself), else as `sparse_parts`."""
    edge = adjacency.__dict__.get("_msgat_edge_index")
    if edge is not None:
        return "edge", edge, adjacency.__dict__["_msgat_edge_weight"].detach()
    return sparse_parts(adjacency)


def _union_map(v: np.ndarray, i: np.ndarray, j: np.ndarray, V: int, n: int, sell: str):
    """(SparsePattern of the union of the stored (i, j), flat map entry -> v * nnz_union + position) from host arrays"""
    for name, a, hi in (("sample", v, V), ("row", i, n), ("column", j, n)):
        if a.size and (int(a.min()) < 0 or int(a.max()) >= hi):
            raise ValueError(f"malformed sparse adjacency indices: a {name} index outside [0, {hi})")
    edges, pos = np.unique(i * n + j, return_inverse=True)           # sorted: the union in row-major = CSR order
    crow = _row_pointers(torch.from_numpy(edges // n), n)
    pattern = _pattern(crow, torch.from_numpy(edges % n), n, sell)
    if not pattern.identity:             # sorted unique (row, column) keys are CSR order
        raise _lib.MsgatError("the union of a sparse adjacency's patterns did not come out in CSR order")
    flat = v * max(len(edges), 1) + pos.reshape(-1)
    if np.unique(flat).size != flat.size:
        raise ValueError("malformed sparse adjacency indices: an entry is stored twice in one sample")
    return pattern, flat


def sparse_sets_of(adjacency: torch.Tensor, sell: str = "auto") -> SparseSets:
    """Cached `SparseSets` of a (coalesced, if COO) sparse [V,N,N] adjacency, after `check_sparse_adjacency`.  Keyed on
    the index tensors' storage address, shape and version; the first sight of a key reads the indices back and builds
    the union and the flat map, and a union with the same content shares its structure.  The first sight inside a
    HIP-graph capture raises, as graph_of does."""
    check_sparse_adjacency(adjacency)
    layout, idx, values = sparse_sets_parts(adjacency)
    if adjacency.dim() != 3:
        raise ValueError(f"sparse_sets_of takes a [V, n_nodes, n_nodes] adjacency, got {tuple(adjacency.shape)}")
    V, n = int(adjacency.shape[0]), int(adjacency.shape[1])
    key = ("sets", layout, V, n, sell) + tuple(_tensor_key(t) for t in idx)
    hit, _ = _SPARSE.lookup(key, adjacency)
    if hit is not None:
        return hit[0]
    if _capturing(adjacency):
        raise _not_cached("the structure of this sparse adjacency is not cached yet")
    host = [t.detach().to(device="cpu", dtype=torch.int64) for t in idx]
    if layout == "edge":                 # one shared pattern; the order inside a row may not be the library's
        crow, col = host
        if crow.dim() != 1 or crow.numel() != n + 1 or col.dim() != 1 or int(crow[-1]) != col.numel():
            raise ValueError("malformed sparse adjacency indices")
        pattern = _pattern(crow, col, n, sell)
        nnz = pattern.structure.nnz
        flat = None if pattern.identity else \
            (torch.arange(V)[:, None] * max(nnz, 1) + pattern._inverse[None, :]).reshape(-1)
        sets = SparseSets(pattern, V, flat)
    else:
        if layout == "csr":
            crow, col = (t.numpy() for t in host)
            if crow.shape != (V, n + 1) or col.ndim != 2 or (crow[:, 0] != 0).any() or (crow[:, -1] != col.shape[1]).any() \
                    or (np.diff(crow, axis=1) < 0).any():
                raise ValueError("malformed sparse adjacency indices")
            v = np.repeat(np.arange(V), col.shape[1])
            i = np.repeat(np.tile(np.arange(n), V), np.diff(crow, axis=1).reshape(-1))
            j = col.reshape(-1)
        else:
            v, i, j = host[0].numpy()
        pattern, flat = _union_map(v, i, j, V, n, sell)
        identity = flat.size == V * pattern.structure.nnz and bool((flat == np.arange(flat.size)).all())
        sets = SparseSets(pattern, V, None if identity else torch.from_numpy(flat))
    # the index tensors stay alive with the entry: their addresses cannot be reused under it
    return _SPARSE.remember(key, adjacency, (sets, idx))[0]


def edge_pattern_of(crow: torch.Tensor, col: torch.Tensor, sell: str = "auto") -> SparsePattern:
    """Cached `SparsePattern` of the CSR index tensors `crow` [N+1], `col` [nnz] themselves: the pattern -- and through
    `_pattern` the very structure -- that `sparse_sets_of` gives an `ops.edge_adjacency(crow, col, weights)`, for an op that
    forms those weights.  Keyed and kept like every entry of `_SPARSE`; the first sight inside a HIP-graph capture raises."""
    if crow.dim() != 1 or col.dim() != 1 or crow.numel() < 1:
        raise ValueError(f"crow {tuple(crow.shape)} and col {tuple(col.shape)} must be [N+1] and [nnz]")
    n = crow.numel() - 1
    key = ("edge-pattern", n, sell, _tensor_key(crow), _tensor_key(col))
    hit, _ = _SPARSE.lookup(key, crow)
    if hit is not None:
        return hit[0]
    if _capturing(crow):
        raise _not_cached("the structure of this edge pattern is not cached yet")
    host_crow, host_col = (t.detach().to(device="cpu", dtype=torch.int64) for t in (crow, col))
    if int(host_crow[-1]) != host_col.numel():
        raise ValueError("malformed sparse adjacency indices")
    return _SPARSE.remember(key, crow, (_pattern(host_crow, host_col, n, sell), (crow, col)))[0]


def _check_sets(adjacency, groups: int, relations: int) -> None:
    V, Bg = int(adjacency.shape[0]), groups // relations
    if V not in (1, Bg, groups):
        raise ValueError(f"a batched sparse adjacency {tuple(adjacency.shape)} needs a leading size in {sorted({1, Bg, groups})} "
                         f"for signals of {groups} groups ({relations} relation(s) x {Bg} samples)")


def sparse_graph_for(adjacency: torch.Tensor, groups: int, relations: int):
    """(graph, its `SparsePattern` or `SparseSets`) of a sparse adjacency (coalesced, if COO): [N,N] with `val` at its
    values on the device, [V,N,N] with V in {1, groups / relations, groups} as its union structure and value sets."""
    check_sparse_adjacency(adjacency)
    if adjacency.dim() == 2:
        pattern = sparse_pattern_of(adjacency)
        return pattern.graph(sparse_parts(adjacency)[2].detach()), pattern
    _check_sets(adjacency, groups, relations)
    sets = sparse_sets_of(adjacency)
    return sets.graph(sparse_sets_parts(adjacency)[2].detach()), sets


def graph_for(adjacency, groups: int, relations: int):
    """What the ops hand the library for `adjacency`: a prebuilt SparseGraph / BatchedGraph as it is; a dense [N,N] or
    [1,N,N] through graph_of; [V,N,N] with V = groups / relations (one set per sample) or V = groups (one per group)
    through batched_graph_of; a sparse [N,N] as its cached pattern with `val` at its values on the device, a sparse
    [V,N,N] as the union of its samples' patterns with V value sets (`sparse_sets_of`).  The graph
    carries no gradient: a batched adjacency that requires grad while autograd records is refused here.  The ops
    (`ops.gacn`, `graph_attention`, `attention_core`, and the modules on them) accept one -- they route its gradient
    themselves."""
    if is_sparse_adjacency(adjacency):
        return sparse_graph_for(adjacency, groups, relations)[0]
    return _dense_graph_for(adjacency, groups, relations, refuse_grad=True)


def _dense_graph_for(adjacency, groups: int, relations: int, refuse_grad: bool):
    """graph_for of anything but a sparse tensor; `refuse_grad=False` for a caller that routes the gradient itself."""
    if isinstance(adjacency, (SparseGraph, ValuedGraph)):
        g = adjacency
    elif not isinstance(adjacency, torch.Tensor):
        raise TypeError(f"adjacency must be a tensor, a SparseGraph or a BatchedGraph, got {type(adjacency).__name__}")
    elif adjacency.dim() == 3 and adjacency.shape[0] != 1:
        V = adjacency.shape[0]
        Bg = groups // relations
        if V != Bg and V != groups:
            allowed = sorted({1, Bg, groups})
            raise ValueError(f"a batched adjacency {tuple(adjacency.shape)} needs a leading size in {allowed} for signals of "
                             f"{groups} groups ({relations} relation(s) x {Bg} samples)")
        if refuse_grad and adjacency.requires_grad and torch.is_grad_enabled():
            raise ValueError(f"the batched adjacency {tuple(adjacency.shape)} requires grad: graph_for builds a graph without "
                             "one; call ops.gacn / graph_attention / attention_core (or a module) with it, which give it its "
                             "gradient, or pass adjacency.detach()")
        g = batched_graph_of(adjacency)
    else:
        g = graph_of(adjacency)
    if isinstance(g, ValuedGraph) and g.n_sets not in (1, groups // relations, groups):
        raise ValueError(f"BatchedGraph with {g.n_sets} value sets for signals of {groups} groups ({relations} relation(s))")
    return g
